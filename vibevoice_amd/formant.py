"""Formants: a warp A / B moves the spectral envelope of a signal, and with it the formants, up by A / B and leaves the pitch where it
is -- the piece the pitch stage (pitch.py) lacks.  In front of the resampler at P / Q, a warp by exactly Q / P puts the envelope back
where it was ("the same voice, a third lower"); alone it is a timbre control (voice size).  This module is the definition of every
output sample and the host's bookkeeping; csrc/formant.hip evaluates the same definition on the device in fp32, each row of a launch
at its own fraction (Engine.formant / Engine.formant_warp).  It needs no GPU and is what the kernels are tested against.

Ratio.  warp_of(f), f in [-12, +12] semitones, is pitch.ratio(f).  Combined with a pitch shift at pitch.ratio(s) = P / Q the stage's
fraction is fraction(f, s) = ratio(f) * Q / P, reduced: both terms stay at or below 10^4; outside [1/2, 2] it is refused, naming both
arguments.  f = 0 with a pitch shift is exactly Q / P: the formants stay.  A / B = 1 / 1 is the identity BY DEFINITION: y = x bit for
bit, nothing held back (the rule of pitch.py's unison, so the rows of one launch mix).

Frames.  N = 1024, hop H = 256, at 24 kHz.  w[i] = 0.5 - 0.5 cos(2 pi i / N), the periodic Hann window (window(): from the cosines of
twiddles(), one rounding), for analysis and synthesis; four overlapping w^2 sum to 3/2, so a synthesised frame is scaled by 2/3.  The
signal is zero outside itself and a non-finite input sample counts as 0.  Frame j = 0, 1, ... covers input samples
[(j - 3) H, (j + 1) H).  Per frame, K = N / 2 + 1 = 513 bins:

    X = rfft(w x),  p[k] = |X[k]|^2
    L[k] = 0.5 ln(p[k] + EPS mean(p) + 2^-100),  EPS = 2^-26            (a floor 78 dB under the frame's mean power)
    c = irfft(L)                                                       (the real cepstrum, N points)
    E = Re rfft(c * lifter),  lifter = 1 for quefrency |q| < QC = 64    (the log envelope: it ignores any pitch below 375 Hz)
    num = k B, i = num // A, f = (num % A) / A                         (an exactly integer position, as pitch.py reads its table)
    Ew[k] = E[i] + f (E[i + 1] - E[i])  where i < K - 1,  E[K - 1] beyond
    G[k] = exp(clamp(Ew[k] - E[k], +-GMAX)),  GMAX = 30 dB in nepers    (a real gain: the phases of X stay, no phase vocoder)
    y_j = (2/3) w irfft(G X)

Output.  out[n] = ((y_j0[n] + y_j0+1[n]) + y_j0+2[n]) + y_j0+3[n], j0 = n // H: the frames are added in ascending order, from the zero
a stream's partial sums start at.  The fixed order makes the streaming form bit-identical to the one-shot form.  n samples in, n out.

Trig.  twiddles(): cos and sin of 2 pi i / N, computed in float64 and rounded to float32, [2, N], read-only, cached.  The host uploads
it the way the pitch stage's prototype table is uploaded; the device's transforms and its window read nothing else.  warp_ref is the
definition in float64: over numpy's float64 transforms, or (table=True) over THAT table, its transforms the sums over cos / sin
[(k n) % N] of the table, widened.  warp_host / HostFormant is the float32 form: numpy's float32 transforms, the window from the
table.  Its distance from warp_ref(table=True) is the yardstick the kernel is held to (tests/test_gpu_formant.py).

Streaming.  Output block b = samples [b H, (b + 1) H) needs input through (b + 4) H: emitted(total) = H max(0, total // H - 3) before
the flush, which emits the rest against zeros; counts() is that rule in integers (correct for totals beyond 2^32), and the engine's C
side (vv_formant_rows) computes the same figures.  A stream keeps N - H = 768 input samples of history behind the at most H - 1 of its
incomplete block, and the 768 partial sums of its overlap-add tail.  It holds back at most 4 H - 1 = 1023 input samples (42.6 ms):
more than the tempo stage's 640.  One push takes at most MAX_IN = 7552 samples per row, as in the pitch stage.
"""
import functools
import math

import numpy as np
import torch

from . import pitch as _pt

N, H = 1024, 256
K = N // 2 + 1
QC = 64                                          # the lifter keeps quefrencies |q| < QC samples
EPS = 2.0 ** -26
TINY = 2.0 ** -100
GMAX = 30.0 / 20.0 * math.log(10.0)              # 30 dB in nepers
DELAY = 4 * H - 1                                # input samples a stream holds back at most
MAX_TERM = 10 ** 4
MIN_SEMITONES, MAX_SEMITONES = _pt.MIN_SEMITONES, _pt.MAX_SEMITONES
MAX_IN = 7552                                    # what one push of the device kernel takes per row (VV_FM_MAX_IN, csrc/vv_common.h)


@functools.lru_cache(maxsize=1)
def twiddles():
    """[2, N] float32 (read-only): cos and sin of 2 pi i / N, computed in float64"""
    a = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    t = np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)]).astype(np.float32))
    t.setflags(write=False)
    return t


def window(dtype=np.float32):
    """w [N]: 0.5 - 0.5 cos, from the table's cosines in `dtype`"""
    return dtype(0.5) - dtype(0.5) * twiddles()[0].astype(dtype)


def warp_of(semitones):
    """(A, B) of a formant shift in [-12, +12] semitones: pitch.ratio of it; anything else is refused with a ValueError naming it"""
    try:
        return _pt.ratio(semitones)
    except ValueError as e:
        raise ValueError(str(e).replace("pitch:", "formant:", 1)) from None


def fraction(formant, pitch=None):
    """(A, B) of the stage in front of a pitch stage at pitch.ratio(pitch) = P / Q (None: no pitch stage) for formants that end up
    `formant` semitones from the untouched voice: ratio(formant) * Q / P, reduced.  Outside [1/2, 2] it is refused, naming both."""
    A, B = warp_of(formant)
    if pitch is not None:
        P, Q = _pt.ratio(pitch)
        A, B = A * Q, B * P
        g = math.gcd(A, B)
        A, B = A // g, B // g
    if A > 2 * B or B > 2 * A:
        raise ValueError(f"formant: formant={formant!r} with pitch={pitch!r} asks the stage for a warp of {A} / {B}, outside [1/2, 2]")
    return A, B


def check(A, B):
    """the fractions the stage takes: both terms in 1..10^4, A / B in [1/2, 2]"""
    if not (isinstance(A, (int, np.integer)) and isinstance(B, (int, np.integer)) and 1 <= A <= MAX_TERM and 1 <= B <= MAX_TERM
            and A <= 2 * B and B <= 2 * A):
        raise ValueError(f"formant: the warp {A!r} / {B!r} must have both terms in [1,{MAX_TERM}] and lie in [1/2, 2]")
    return int(A), int(B)


def emitted(total_in, A=2, B=1):
    """outputs a stream has emitted before its flush once total_in samples have arrived (all of them at 1 / 1)"""
    return int(total_in) if A == B else H * max(0, int(total_in) // H - 3)


def counts(total_in, n_in, flush=False, A=2, B=1):
    """(m0, n_out) of a push of n_in samples to a stream that has taken total_in so far: the index of the first output it emits and
    how many.  Integers only: the streamer sizes its copies with it, without a device sync."""
    m0 = emitted(total_in, A, B)
    m1 = int(total_in) + int(n_in) if flush else emitted(int(total_in) + int(n_in), A, B)
    return m0, m1 - m0


def push_width(remaining):
    """input samples per row the next push accepts from rows that still have remaining[i]"""
    return max(1, min(MAX_IN, max(remaining)))


# ---- the frame: X -> y_j, in float32 over numpy's transforms and in float64 over the table
def _gain(E, A, B, dt):
    k = np.arange(K, dtype=np.int64)
    num = k * B
    i, r = num // A, num % A
    f = (r.astype(np.float32) / np.float32(A)).astype(dt)
    inside = i < K - 1
    i = np.minimum(i, K - 2)
    e0 = E[:, i]
    Ew = np.where(inside, e0 + f * (E[:, i + 1] - e0), E[:, K - 1:K])
    return np.exp(np.clip(Ew - E, dt(-GMAX), dt(GMAX)))


def _log_power(X, dt):
    p = X.real * X.real + X.imag * X.imag
    return dt(0.5) * np.log(p + dt(EPS) * p.mean(axis=1, keepdims=True, dtype=dt) + dt(TINY))


def _frames_host(fr, A, B):
    """y_j of the frames fr [n, N] float32, every operation in float32"""
    f32 = np.float32
    w = window(f32)
    X = np.fft.rfft(fr * w, axis=1).astype(np.complex64)
    c = np.fft.irfft(_log_power(X, f32), n=N, axis=1).astype(f32)
    q = np.arange(N)
    E = np.fft.rfft(c * ((q < QC) | (q > N - QC)).astype(f32), axis=1).real.astype(f32)
    Y = (_gain(E, A, B, f32) * X).astype(np.complex64)
    return (f32(2.0 / 3.0) * w * np.fft.irfft(Y, n=N, axis=1).astype(f32)).astype(f32)


@functools.lru_cache(maxsize=1)
def _dft():
    """cos and sin of the table at (n k) % N, [N, K] float64: the transforms of warp_ref over the table"""
    t = twiddles().astype(np.float64)
    idx = (np.arange(N, dtype=np.int64)[:, None] * np.arange(K, dtype=np.int64)[None, :]) % N
    return t[0][idx], t[1][idx]


_WK = np.full(K, 2.0)
_WK[0] = _WK[K - 1] = 1.0                                             # a real signal's bins 1 .. K - 2 stand for two


def _rfft_table(x):
    C, S = _dft()
    return x @ C - 1j * (x @ S)


def _irfft_table(Y):
    C, S = _dft()
    Yi = Y.imag * _WK
    Yi[:, 0] = Yi[:, K - 1] = 0.0                                     # an inverse real transform ignores them
    return ((Y.real * _WK) @ C.T - Yi @ S.T) / N


def _frames_ref(fr, A, B, table=True, unit_gain=False):
    """y_j of the frames fr [n, N] in float64; table: the transforms as sums over the float32 table (and its window), else numpy's in
    float64 and the window of float64 cosines.  unit_gain: G = 1, what the window and the 2/3 scale alone do"""
    f64 = np.float64
    rfft, irfft = (_rfft_table, _irfft_table) if table else (lambda v: np.fft.rfft(v, axis=1), lambda v: np.fft.irfft(v, n=N, axis=1))
    w = window(f64) if table else 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    X = rfft(fr * w)
    if unit_gain:
        return (2.0 / 3.0) * w * irfft(X)
    q = np.arange(N)
    E = rfft(irfft(_log_power(X, f64).astype(np.complex128)) * ((q < QC) | (q > N - QC))).real
    return (2.0 / 3.0) * w * irfft(_gain(E, A, B, f64) * X)


class _Stream:
    """the streaming form in `dtype` with frames(fr, A, B): push(x, flush) -> what the push completes (numpy)"""

    def __init__(self, A, B, dtype, frames):
        self.A, self.B = check(A, B)
        self.dtype, self._frames = dtype, frames
        self.delay_samples = 0 if self.A == self.B else DELAY
        self.reset()

    def reset(self):
        self.total_in = 0
        self.flushed = False
        self._buf = np.zeros(N - H, dtype=self.dtype)                 # the input from (F - 3) H on, F = frames done: zeros before 0
        self._tail = np.zeros((3, H), dtype=self.dtype)               # partial sums of blocks F - 3, F - 2, F - 1

    def counts(self, n_in, flush=False):
        return counts(self.total_in, n_in, flush, self.A, self.B)

    def _push(self, x, flush):
        if self.flushed:
            raise RuntimeError("HostFormant: the stream has been flushed; reset() it before its next push")
        n_in = x.shape[0]
        n_out = self.counts(n_in, flush)[1]
        before, self.total_in, self.flushed = self.total_in, self.total_in + n_in, bool(flush)
        if self.A == self.B:
            return x.copy()
        x = np.where(np.isfinite(x), x, 0).astype(self.dtype)
        F0 = before // H
        F1 = -(-self.total_in // H) + 3 if flush else self.total_in // H
        nf = F1 - F0
        buf = np.concatenate([self._buf, x])
        if nf <= 0:
            self._buf = buf
            return np.zeros(0, dtype=self.dtype)
        need = (nf + 3) * H
        if buf.shape[0] < need:
            buf = np.concatenate([buf, np.zeros(need - buf.shape[0], dtype=self.dtype)])
        fr = np.lib.stride_tricks.sliding_window_view(buf, N)[::H][:nf]
        y = self._frames(np.ascontiguousarray(fr), self.A, self.B).astype(self.dtype)
        blocks = np.zeros((nf + 3, H), dtype=self.dtype)              # blocks F0 - 3 ...: a block's frames ascend as the segment descends
        blocks[:3] = self._tail
        for s in (3, 2, 1, 0):
            blocks[s:s + nf] = blocks[s:s + nf] + y[:, s * H:(s + 1) * H]
        self._tail = blocks[nf:].copy()
        self._buf = buf[nf * H:].copy()
        c_min = max(0, 3 - F0)
        return blocks[c_min:nf].reshape(-1)[:n_out].copy()


class HostFormant(_Stream):
    """The warp's streaming form on the host, one stream, float32 torch: push(chunk) -> the samples that chunk completes, flush() ->
    the tail.  Whatever the cuts, the concatenation equals warp_host(whole signal), bit for bit.  AudioStreamer runs CPU chunks
    through it, between tempo.HostTempo and pitch.HostPitch."""

    def __init__(self, A, B):
        super().__init__(A, B, np.float32, _frames_host)

    def push(self, chunk, flush=False):
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu().numpy()
        return torch.from_numpy(np.ascontiguousarray(self._push(x, flush), dtype=np.float32))

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def warp_host(x, A, B):
    """one-shot float32 on the host: HostFormant over the whole signal"""
    return HostFormant(A, B).push(x, flush=True)


def warp_ref(x, A, B, table=False, unit_gain=False):
    """The definition in numpy at the warp A / B: a 1-D signal -> as many samples, in float64.  table: over the float32 table of
    twiddles() (its transforms are the sums over cos / sin [(k n) % N] of the table, widened, and its window comes from the table's
    cosines): what the device is held to; else over numpy's float64 transforms and the window of float64 cosines.  unit_gain: G = 1
    computed through the frames anyway (at 1 / 1 too, where the definition is y = x without them): the input, to 1e-15."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    s = _Stream(2 if unit_gain else A, 1 if unit_gain else B, np.float64, functools.partial(_frames_ref, table=table, unit_gain=unit_gain))
    return s._push(x, True)
