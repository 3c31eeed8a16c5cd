"""Loudness: an ITU-R BS.1770 meter and a causal adaptive leveller: the definition of every energy and of every output sample, and the
host's bookkeeping.  csrc/loudness.hip evaluates the same definition on the device (Engine.loudness / apply_loudness / measure_loudness /
segment_energies), with no tolerance; this module needs no GPU and is what the kernels are tested against.

The stage runs at 24 kHz only (RATE), the rate of the model.  S = 2400 samples is a segment (100 ms), T = 2400 the taps of the filter.

K-weighting as an exact FIR.  h is the impulse response at 24 kHz of the standard's pre-filter, the shelving biquad followed by the RLB
high-pass, each from its analogue parameters (SHELF, HIGHPASS) through the bilinear transform (biquads()); at 48 kHz those give the
coefficients the standard prints.  h is evaluated in float64 by the direct-form-II-transposed recurrence and cut at T taps (the tail
behind them sums to 8.2e-10 in absolute value; sum |h| = 3.2494, max |h| = 1.4879).

    hq[k] = rint(h[k] 2^24)                               int32
    xq[i] = rint(fl(clamp(x[i], -8, 8) 2^20))             fp32, round to nearest even; a non-finite x[i] counts as 0; |xq| <= 2^23;
                                                          xq = 0 before the stream's first sample
    z[i]  = sum_{k < T} hq[k] xq[i - k]                   an exact integer, |z| < 2^23 3.25 2^24 < 2^49: every partial sum, in any order,
                                                          is exact in int64 and in fp64, with or without fma
    zs[i] = z[i] >> 28                                    arithmetic floor, |zs| < 2^21
    E[m]  = sum_{i in segment m} zs[i]^2                  int64 below 2^54; only complete segments have one

The mean square of segment m in the standard's units is E[m] / (S 2^32), its loudness -0.691 + 10 log10 of that.

The meter reads the same sums at 16 times the resolution: zf[i] = z[i] >> 24 (|zf| < 2^25), F[m] = sum zf[i]^2, an int64 below
2400 2^50 < 2^62, mean square F[m] / (S 2^40).  At -60 LUFS zs is a few dozen units of 2^-16 and its floor shows in a reading (an 8 kHz
sine, three samples a period, read 0.019 LU high from E); from F the same signal reads within 0.001 LU.  The leveller, which ignores
what lies under -50 LUFS, works on E.

Meter (measure_ref).  Blocks P[b] = F[b] + F[b+1] + F[b+2] + F[b+3] (400 ms, 75 % overlap).  Gating of BS.1770-4 over Python integers and
float64: blocks under -70 LUFS are dropped, then blocks more than 10 LU under the loudness of the mean of the rest; the result is the
loudness of the mean of what remains.  No block over the absolute gate, or fewer than four segments: -inf.

Leveller (leveller_ref): causal, holds nothing back, as many outputs as inputs.  Per stream target_lufs in [-36, -10], start_db in
[-24, +24] (the gain before there is a measurement), max_boost_db in [0, 24]; as float32 values
t = float32(10^((target + 0.691) / 10)), g0 = float32(10^(start_db / 20)), wmax = float32(10^(max_boost_db / 20)),
wmin = float32(10^(-24 / 20)).  Segment m counts if E[m] >= EG = floor(S 2^32 10^((-50 + 0.691) / 10)).  After segment m, M30 and c30
are the sum and the number of the last up to 30 counted segments, M4 the sum of the last 4 counted ones, and the wanted gain is

    w[m] = w[m-1]                                          while c30 < 4;  w[-1] = w[-2] = g0
    p30  = fl(float32(M30 >> 8) / float32(c30 S 2^24))     the shifted integer is exact in float64 and rounds once to fp32
    p4   = fl(float32(M4 >> 8) / float32(4 S 2^24))
    w[m] = min(max(fl(sqrt(fl(t / max(p30, p4)))), wmin), wmax)      IEEE division and square root, no fma

Sample i = m S + k of segment m:

    a[i] = fl(w[m-2] + fl(fl(w[m-1] - w[m-2]) fl(float32(k) / float32(S))))
    y[i] = fl(a[i] x[i])                                   a non-finite x[i] counts as 0

so a segment's gain depends only on segments complete before it starts: p4 brings the gain down within 400 ms of a louder speaker, p30
brings it back over seconds.

Streaming.  A stream keeps its last T - 1 quantised inputs (history()), the running sum and position of the open segment, the ring of
30 counted energies, two gains and total_in, and nothing else that depends on the data: what it emits depends on its input so far, never
on how that was cut into pushes.  A push emits as many samples as it brings (counts()); the flush emits nothing, it closes the stream.
"""
import math

import numpy as np
import torch

RATE = 24000
S = 2400                        # samples of a segment (100 ms)
SHIFT, FINE_SHIFT = 28, 24      # zs = z >> 28 (the leveller's E), zf = z >> 24 (the meter's F)
T = 2400                        # taps of the K-weighting FIR
RING = 30                       # counted segments the slow mean looks back over (3 s)
SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)      # f0 (Hz), gain (dB), Q
HIGHPASS = (38.13547087602444, 0.5003270373238773)                      # f0 (Hz), Q
MIN_TARGET, MAX_TARGET = -36.0, -10.0
MIN_START_DB, MAX_START_DB = -24.0, 24.0
MIN_BOOST_DB, MAX_BOOST_DB = 0.0, 24.0
DEFAULT_BOOST_DB = 12.0
ABS_GATE, REL_GATE, SEG_GATE = -70.0, -10.0, -50.0

# mirrored from the C side (csrc/vv_common.h): VV_LD_MAX_IN, the input samples one row of a device push may bring, and VV_LD_GATE = EG
MAX_IN = 3200
EG = 120856803
assert EG == math.floor(S * 2.0 ** 32 * 10.0 ** ((SEG_GATE + 0.691) / 10.0))


def _rate(rate):
    if int(rate) != RATE:
        raise ValueError(f"loudness: the stage runs at {RATE} Hz, the model's rate; rate = {rate!r} is not served")
    return RATE


def biquads(rate=RATE):
    """((b, a) of the shelf, (b, a) of the high-pass) at `rate` Hz, float64, a[0] = 1: SHELF and HIGHPASS through the bilinear transform"""
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    hp = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, hp


def _df2t(b, a, x):
    y = np.empty_like(x)
    s1 = s2 = 0.0
    b0, b1, b2, a1, a2 = float(b[0]), float(b[1]), float(b[2]), float(a[1]), float(a[2])
    for i in range(x.shape[0]):
        v = float(x[i])
        o = b0 * v + s1
        s1 = b1 * v - a1 * o + s2
        s2 = b2 * v - a2 * o
        y[i] = o
    return y


_TAPS = {}


def impulse_response(n=T, rate=RATE):
    """h: the first n samples of the pre-filter's impulse response at `rate` Hz, float64"""
    key = (int(n), int(rate))
    if key not in _TAPS:
        d = np.zeros(key[0], dtype=np.float64)
        d[0] = 1.0
        (sb, sa), (hb, ha) = biquads(key[1])
        _TAPS[key] = _df2t(hb, ha, _df2t(sb, sa, d))
    return _TAPS[key].copy()


def taps():
    """hq, int32 [T]"""
    return np.rint(impulse_response(T, RATE) * 2.0 ** 24).astype(np.int32)


def _range(what, value, lo, hi, unit):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"loudness: {what} must be a number in [{lo}, {hi}] {unit}, got {value!r}") from None
    if not (lo <= v <= hi):                                   # a NaN compares false
        raise ValueError(f"loudness: {what} must lie in [{lo}, {hi}] {unit}, got {value!r}")
    return v


def target_of(target_lufs):
    """t, float32, of a target in [-36, -10] LUFS; anything else (NaN included) is refused with a ValueError naming it"""
    return np.float32(10.0 ** ((_range("target_lufs", target_lufs, MIN_TARGET, MAX_TARGET, "LUFS") + 0.691) / 10.0))


def start_of(start_db):
    """g0, float32, of a start gain in [-24, +24] dB"""
    return np.float32(10.0 ** (_range("start_db", start_db, MIN_START_DB, MAX_START_DB, "dB") / 20.0))


def boost_of(max_boost_db):
    """wmax, float32, of an upper bound in [0, 24] dB"""
    return np.float32(10.0 ** (_range("max_boost_db", max_boost_db, MIN_BOOST_DB, MAX_BOOST_DB, "dB") / 20.0))


WMIN = np.float32(10.0 ** (-24.0 / 20.0))


def history():
    """quantised input samples a stream keeps between two pushes"""
    return T - 1


def counts(total_in, n_in, flush=False):
    """(o0, n_out) of a push of n_in samples to a stream that has taken total_in so far: the index of the first output it emits and how
    many.  The stage holds nothing back: as many as it brings, and the flush adds none."""
    return int(total_in), int(n_in)


def push_width():
    """input samples one row of a device push may bring"""
    return MAX_IN


def quantise(x):
    """xq, int64, of float32 samples"""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)
    return np.rint(np.clip(x, np.float32(-8.0), np.float32(8.0)) * np.float32(2.0 ** 20)).astype(np.int64)


def _fir(xq_with_history):
    """z of every sample behind the first T - 1 of an int64 array, int64: the products and sums run in float64, where they are exact"""
    z = np.convolve(xq_with_history.astype(np.float64), taps().astype(np.float64), mode="valid")
    return z.astype(np.int64)


def _zs2(xq_with_history, shift=SHIFT):
    zs = _fir(xq_with_history) >> shift
    return zs * zs


def segment_energies_ref(x, fine=False):
    """E[m] (fine: F[m]) of every complete segment of a 1-D signal, int64 [len(x) // S]"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n_seg = x.shape[0] // S
    if n_seg == 0:
        return np.zeros(0, dtype=np.int64)
    xq = np.concatenate([np.zeros(T - 1, dtype=np.int64), quantise(x[:n_seg * S])])
    return _zs2(xq, FINE_SHIFT if fine else SHIFT).reshape(n_seg, S).sum(axis=1)


def lufs_of(mean_square):
    return -0.691 + 10.0 * math.log10(mean_square) if mean_square > 0 else -math.inf


def gated(E, fine=False):
    """the gated loudness in LUFS (float, -inf where nothing passes the absolute gate) of segment energies E (fine: F)"""
    E = [int(e) for e in E]
    unit = 4 * S * 2 ** (88 - 2 * (FINE_SHIFT if fine else SHIFT))      # z = y 2^44: P / unit is a block's mean square (2^32, fine 2^40)
    P = [E[b] + E[b + 1] + E[b + 2] + E[b + 3] for b in range(len(E) - 3)]
    kept = [p for p in P if lufs_of(p / unit) > ABS_GATE]
    if not kept:
        return -math.inf
    rel = lufs_of(sum(kept) / (len(kept) * unit)) + REL_GATE
    kept = [p for p in kept if lufs_of(p / unit) > rel]
    return lufs_of(sum(kept) / (len(kept) * unit)) if kept else -math.inf


def measure_ref(x):
    """the BS.1770 loudness of a 1-D signal at 24 kHz in LUFS, a Python float"""
    return gated(segment_energies_ref(x, fine=True), fine=True)


class _Gains:
    """the leveller's state behind the energies: the ring of counted segments and the last two wanted gains"""

    def __init__(self, t, g0, wmax):
        self.t, self.wmax = np.float32(t), np.float32(wmax)
        self.w1 = self.w2 = np.float32(g0)                    # w[m-1], w[m-2] of the open segment m
        self.ring = []

    def close_segment(self, E):
        """segment m is complete with energy E: -> w[m]; the open segment is now m + 1"""
        E, w = int(E), self.w1
        if E >= EG:
            self.ring = (self.ring + [E])[-RING:]
        c30 = len(self.ring)
        if c30 >= 4:
            p30 = np.float32(float(sum(self.ring) >> 8)) / np.float32(c30 * S * 2 ** 24)
            p4 = np.float32(float(sum(self.ring[-4:]) >> 8)) / np.float32(4 * S * 2 ** 24)
            p = max(p30, p4)
            w = min(max(np.sqrt(np.float32(self.t / p)), WMIN), self.wmax)
        self.w2, self.w1 = self.w1, np.float32(w)
        return self.w1


def _ramp():
    return (np.arange(S, dtype=np.float32) / np.float32(S)).astype(np.float32)


def _apply(x, k0, gains):
    """y and a of samples x (float32) that start at position k0 of the open segment; gains[r] = (w[m-2], w[m-1]) of the r-th segment
    they touch"""
    n = x.shape[0]
    pos = k0 + np.arange(n)
    r, k = pos // S, pos % S
    g = np.asarray(gains, dtype=np.float32).reshape(-1, 2)
    w2, w1 = g[r, 0], g[r, 1]
    a = (w2 + ((w1 - w2).astype(np.float32) * _ramp()[k]).astype(np.float32)).astype(np.float32)
    xf = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)
    return (a * xf).astype(np.float32), a


class HostLoudness:
    """The streaming leveller on the host, one stream, float32 torch: push(chunk) -> as many samples, flush() -> none, it closes the
    stream.  Whatever the cuts, the concatenation equals leveller_ref of the whole signal, bit for bit.  AudioStreamer runs CPU chunks
    through it."""

    def __init__(self, target_lufs, start_db=0.0, max_boost_db=DEFAULT_BOOST_DB, rate=RATE):
        _rate(rate)
        self.t, self.g0, self.wmax = target_of(target_lufs), start_of(start_db), boost_of(max_boost_db)
        self.reset()

    def reset(self):
        self.total_in = 0
        self.flushed = False
        self._hist = np.zeros(T - 1, dtype=np.int64)          # xq[total_in - (T - 1) .. total_in)
        self._acc = 0                                         # the open segment's running sum
        self._g = _Gains(self.t, self.g0, self.wmax)
        self.energies = []                                    # E of every segment completed so far

    def counts(self, n_in, flush=False):
        return counts(self.total_in, n_in, flush)

    def push(self, chunk, flush=False, return_gain=False):
        if self.flushed:
            raise RuntimeError("HostLoudness: the stream has been flushed; reset() it before its next push")
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu().numpy()
        n, k0 = x.shape[0], self.total_in % S
        gains = [(self._g.w2, self._g.w1)]
        if n:
            buf = np.concatenate([self._hist, quantise(x)])
            e = _zs2(buf)
            at = 0
            while at < n:                                     # the stretch of the chunk inside one segment
                m = min(n - at, S - (self.total_in + at) % S)
                self._acc += int(e[at:at + m].sum())
                at += m
                if (self.total_in + at) % S == 0:
                    self.energies.append(self._acc)
                    self._g.close_segment(self._acc)
                    self._acc = 0
                    gains.append((self._g.w2, self._g.w1))
            self._hist = buf[n:].copy()
        y, a = _apply(x, k0, gains)
        self.total_in += n
        self.flushed = bool(flush)
        y, a = torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(np.ascontiguousarray(a))
        return (y, a) if return_gain else y

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def leveller_ref(x, target_lufs, start_db=0.0, max_boost_db=DEFAULT_BOOST_DB, return_gain=False, rate=RATE):
    """The definition in numpy: a 1-D signal of n samples -> n float32 samples (and a, on request)"""
    _rate(rate)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    g = _Gains(target_of(target_lufs), start_of(start_db), boost_of(max_boost_db))
    gains = [(g.w2, g.w1)]
    for E in segment_energies_ref(x):
        g.close_segment(E)
        gains.append((g.w2, g.w1))
    y, a = _apply(x, 0, gains)
    return (y, a) if return_gain else y


def loudness_host(x, target_lufs, start_db=0.0, max_boost_db=DEFAULT_BOOST_DB, rate=RATE):
    """one-shot float32 on the host: HostLoudness over the whole signal"""
    return HostLoudness(target_lufs, start_db, max_boost_db, rate).push(x, flush=True)
