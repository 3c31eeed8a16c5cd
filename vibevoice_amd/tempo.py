"""Speaking rate: a pitch-preserving tempo change by a rational factor P / Q (WSOLA with an exact integer similarity search): the
definition of every output sample and the host's bookkeeping.  csrc/tempo.hip evaluates the same definition on the device
(Engine.tempo / Engine.time_stretch) and chooses the same offsets, with no tolerance; this module needs no GPU and is what the kernels
are tested against.

Definition, at 24 kHz.  HS = 240 (output hop), N = 480 = 2 HS (window), DELTA = 160 (search radius, +-6.7 ms),
w[i] = float32(0.5 - 0.5 cos(2 pi i / N)) the periodic Hann window, computed in float64 and rounded once (window()).  speed in
[0.5, 2.0] is taken as P / Q = Fraction(speed).limit_denominator(100).  The signal x of n samples is zero outside [0, n); the search
runs on s[i] = int(rint(float32(clamp(x[i], -1, 1)) * float32(32767))): one fp32 product, round half to even (a NaN counts as -1
there).  The output has total = ceil(n Q / P) samples in blocks k = 0 .. ceil(total / HS) - 1 of HS samples, the last cut at total:

    a_k = (k HS P) // Q                                           where the block sits in the input
    t_k = p_{k-1} + HS,  p_{-1} = -HS                             the natural continuation of the previous segment
    ssd(d) = sum_{i < N} (s[t_k + i] - s[a_k + d + i])^2          for d in [-DELTA, DELTA], exact integers (below 2^43)
    delta_k = the d of the smallest ssd; ties: the smallest |d|, then the negative d
    p_k = a_k + delta_k
    y[k HS + i] = fl(fl(w[HS + i] x[t_k + i]) + fl(w[i] x[p_k + i]))      i < HS: two rounded products, one rounded sum, no fma

Streaming.  Block k is emitted once total_in >= max(a_k, a_{k-1} + HS) + DELTA + N (a_{-1} = -HS): everything it can read has
arrived.  The flush emits the rest against zeros.  What a stream emits therefore depends on its input only, never on how that was cut
into pushes, and how much a push emits is a matter of integers (counts()): the streamer sizes its copies with it, without a device
sync.  A stream holds back at most N + DELTA = 640 input samples (26.7 ms) until its next push (held()); the only state that depends
on the data is delta_{k-1}, and the input a stream still needs starts at a_{k-1} - DELTA: fewer than HISTORY = 1280 samples.
"""
import math
from fractions import Fraction

import numpy as np
import torch

HS, N, DELTA = 240, 480, 160
HISTORY = 1280                  # > DELTA + (a_k - a_{k-1} <= 480) + 639: what a stream keeps of its input between two pushes
MIN_SPEED, MAX_SPEED = 0.5, 2.0

_W = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)
_W.setflags(write=False)
_D = np.arange(-DELTA, DELTA + 1, dtype=np.int64)
_TIE = (np.abs(_D) << 1) | (_D >= 0)             # the low bits of the packed key (ssd, |d|, d >= 0)


def window():
    """w [N] float32 (read-only): the table the kernels read"""
    return _W


def ratio(speed):
    """(P, Q) of a speed in [0.5, 2.0]; anything else (NaN included) is refused with a ValueError naming it"""
    try:
        v = float(speed)
    except (TypeError, ValueError):
        raise ValueError(f"tempo: speed must be a number in [{MIN_SPEED}, {MAX_SPEED}], got {speed!r}") from None
    if not (MIN_SPEED <= v <= MAX_SPEED):                     # a NaN compares false
        raise ValueError(f"tempo: speed must lie in [{MIN_SPEED}, {MAX_SPEED}], got {speed!r}")
    f = Fraction(v).limit_denominator(100)
    return f.numerator, f.denominator


def delay_samples():
    """input samples a stream holds back, at most, until its next push (or its flush)"""
    return N + DELTA


def total_out(n_in, P, Q):
    """outputs of a whole signal of n_in samples: ceil(n_in Q / P)"""
    return -((-int(n_in) * Q) // P)


def _a(k, P, Q):
    return (k * HS * P) // Q if k >= 0 else -HS


def emitted_blocks(total_in, P, Q):
    """blocks a stream has emitted before its flush once total_in samples have arrived: every k with
    max(a_k, a_{k-1} + HS) + DELTA + N <= total_in"""
    room = int(total_in) - DELTA - N
    if room < 0:
        return 0
    k = ((room + 1) * Q) // (HS * P) + 1                      # a_k <= room implies k below this
    while k > 0 and max(_a(k - 1, P, Q), _a(k - 2, P, Q) + HS) > room:
        k -= 1
    return k


def counts(P, Q, total_in, n_in, flush=False):
    """(o0, n_out) of a push of n_in samples to a stream that has taken total_in so far: the index of the first output sample it
    emits and how many.  Integers only."""
    k0 = emitted_blocks(total_in, P, Q)
    if flush:
        return k0 * HS, total_out(total_in + n_in, P, Q) - k0 * HS
    return k0 * HS, (emitted_blocks(total_in + n_in, P, Q) - k0) * HS


def held(total_in, P, Q):
    """input samples that have arrived and still wait for the stream's next block: total_in - max(a_K, a_{K-1} + HS), K the next
    block; below N + DELTA"""
    k = emitted_blocks(total_in, P, Q)
    return int(total_in) - max(_a(k, P, Q), _a(k - 1, P, Q) + HS)


def search_signal(x):
    """s of the definition: int64 from float32 samples"""
    c = np.fmin(np.fmax(np.asarray(x, dtype=np.float32), np.float32(-1.0)), np.float32(1.0))
    return np.rint(c * np.float32(32767.0)).astype(np.int64)


def _blocks(buf, base, k0, k1, P, Q, d_prev, total, radius=DELTA):
    """Blocks k0 .. k1 - 1 from buf = x[base ...] (float32, zeros where the signal has none, long enough for every read):
    (y, offsets, delta_{k1 - 1}); d_prev: delta_{k0 - 1}; the output is cut at sample index `total`.  radius < DELTA narrows the search
    (0: plain overlap-add, what the tests compare against)."""
    s = search_signal(buf)
    win = np.lib.stride_tricks.sliding_window_view(s, N)
    lo, hi = DELTA - radius, DELTA + radius + 1
    ys, offs = [], []
    for k in range(k0, k1):
        a = _a(k, P, Q) - base
        t = _a(k - 1, P, Q) + d_prev + HS - base
        diff = win[a - DELTA + lo:a - DELTA + hi] - s[t:t + N]
        key = ((diff * diff).sum(axis=1) << 9) | _TIE[lo:hi]
        d_prev = int(_D[lo + int(np.argmin(key))])
        p = a + d_prev
        y = _W[HS:] * buf[t:t + HS] + _W[:HS] * buf[p:p + HS]          # float32 throughout: a rounding per product and per sum
        ys.append(y[:max(0, min(HS, total - k * HS))])
        offs.append(d_prev)
    y = np.concatenate(ys) if ys else np.zeros(0, dtype=np.float32)
    return y, np.asarray(offs, dtype=np.int64), d_prev


def stretch_ref(x, speed, return_offsets=False, radius=DELTA):
    """The definition in numpy: a 1-D signal of n samples -> ceil(n Q / P) float32 samples (and the delta_k, on request)."""
    P, Q = ratio(speed)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.shape[0]
    total = total_out(n, P, Q)
    buf = np.concatenate([np.zeros(HISTORY, dtype=np.float32), x, np.zeros(HISTORY, dtype=np.float32)])
    y, offs, _ = _blocks(buf, -HISTORY, 0, -(-total // HS), P, Q, 0, total, radius)
    return (y, offs) if return_offsets else y


class HostTempo:
    """The streaming form on the host, one stream, float32 torch: push(chunk) -> the samples that chunk completes, flush() -> the
    tail.  Whatever the cuts, the concatenation equals stretch_ref of the whole signal, bit for bit, with the same offsets
    (self.offsets collects them).  AudioStreamer runs CPU chunks through it."""

    def __init__(self, speed):
        self.P, self.Q = ratio(speed)
        self.delay_samples = delay_samples()
        self.reset()

    def reset(self):
        self.total_in = 0
        self.flushed = False
        self.offsets = []
        self._d_prev = 0
        self._hist = np.zeros(HISTORY, dtype=np.float32)            # x[total_in - HISTORY .. total_in)

    def counts(self, n_in, flush=False):
        return counts(self.P, self.Q, self.total_in, n_in, flush)

    def push(self, chunk, flush=False):
        if self.flushed:
            raise RuntimeError("HostTempo: the stream has been flushed; reset() it before its next push")
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu().numpy()
        n_in = x.shape[0]
        o0, n_out = self.counts(n_in, flush)
        after = self.total_in + n_in
        buf = np.concatenate([self._hist, x, np.zeros(HISTORY, dtype=np.float32)])
        k0, total = o0 // HS, (o0 + n_out if flush else 1 << 62)
        y, offs, self._d_prev = _blocks(buf, self.total_in - HISTORY, k0, -(-(o0 + n_out) // HS), self.P, self.Q, self._d_prev, total)
        self.offsets.extend(int(d) for d in offs)
        self._hist = buf[n_in:n_in + HISTORY].copy()
        self.total_in = after
        self.flushed = bool(flush)
        return torch.from_numpy(np.ascontiguousarray(y))

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def stretch_host(x, speed):
    """one-shot float32 on the host: HostTempo over the whole signal"""
    return HostTempo(speed).push(x, flush=True)
