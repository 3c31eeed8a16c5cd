"""Output level: a gain in dB and a look-ahead peak limiter: the definition of every output sample and the host's bookkeeping.
csrc/level.hip evaluates the same definition on the device (Engine.level / Engine.apply_level), with no tolerance; this module needs
no GPU and is what the kernels are tested against.

Definition, in samples at the rate the stage runs at.  A = max(1, rate * 5 // 1000) (look-ahead and ramp, 5 ms), H = rate * 50 // 1000
(hold, 50 ms), g = float32(10 ** (volume_db / 20)), c = float32(10 ** (ceiling_db / 20)) with ceiling_db <= 0.  x is zero outside
[0, n); fl is one fp32 rounding, no fma anywhere:

    u[i] = fl(g x[i]);  a non-finite u[i] counts as 0
    r[i] = 1 where |u[i]| <= c, fl(c / |u[i]|) elsewhere;  r = 1 outside [0, n)
    q[i] = floor(r[i] 2^20)                               an integer in [0, 2^20], the product is exact
    h[j] = min_{k in [j - H, j + A - 1]} q[k]             exact
    S[i] = sum_{j in [i - A + 1, i]} h[j]                 an exact integer below 2^31 (A <= 2047)
    a[i] = fl(float32(S[i]) / float32(A 2^20))            int -> fp32 round to nearest even, IEEE division
    y[i] = min(max(fl(a[i] u[i]), -c), c)

Ceiling: every h[j] in S[i] has a window that holds i, so a[i] <= r[i] up to the two roundings and |y| <= c; the clamp moves a value
by a rounding error at most.  Hold: the gain comes down linearly over A samples before a peak, stays for H samples after it and comes
back over A, so a periodic signal of period <= H + A sees one constant gain while it lasts.  Passthrough: where nothing within reach
exceeds c, S = A 2^20, a = 1 exactly and y = fl(g x) bit for bit (x at 0 dB).  min and integer sums do not depend on their order: a
parallel evaluation agrees with this one to the last bit.

Streaming.  As many outputs as inputs; output i needs the input up to i + A - 1.  Before its flush a stream that has taken total_in
samples has emitted max(0, total_in - (A - 1)) (emitted()); the flush emits the rest against r = 1.  A stream keeps its last
H + 2 A - 2 input samples between pushes (history()) and nothing else that depends on the data, so what it emits depends on its input
only, never on how that was cut into pushes, and how much a push emits is a matter of integers (counts()).
"""
import numpy as np
import torch

MIN_VOLUME_DB, MAX_VOLUME_DB = -40.0, 24.0
MIN_CEILING_DB, MAX_CEILING_DB = -20.0, 0.0
DEFAULT_CEILING_DB = -1.0
MAX_A = 2047                    # keeps S below 2^31
ONE = 1 << 20                   # q of r = 1

# What one push of the device kernel takes per row, mirrored from the C side (VV_LV_BUF, csrc/vv_common.h): the stream's history, the
# chunk and A - 1 zeros within BUF samples of LDS.
BUF = 8128


def params(rate):
    """(A, H) of a sample rate: the 5 ms look-ahead / ramp and the 50 ms hold, in samples"""
    rate = int(rate)
    if rate < 1:
        raise ValueError(f"level: the sample rate must be positive, got {rate}")
    A, H = max(1, rate * 5 // 1000), rate * 50 // 1000
    if A > MAX_A or history(A, H) + A > BUF:
        raise ValueError(f"level: {rate} Hz asks for a look-ahead of {A} samples and {history(A, H) + A} staged ones; the stage serves "
                         f"up to {MAX_A} and {BUF} (about 125 kHz)")
    return A, H


def _db(what, value, lo, hi):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"level: {what} must be a number in [{lo}, {hi}] dB, got {value!r}") from None
    if not (lo <= v <= hi):                                   # a NaN compares false
        raise ValueError(f"level: {what} must lie in [{lo}, {hi}] dB, got {value!r}")
    return np.float32(10.0 ** (v / 20.0))


def gain_of(volume_db):
    """g, float32, of a volume in [-40, +24] dB; anything else (NaN included) is refused with a ValueError naming it"""
    return _db("volume_db", volume_db, MIN_VOLUME_DB, MAX_VOLUME_DB)


def ceiling_of(ceiling_db):
    """c, float32, of a ceiling in [-20, 0] dB; anything else (NaN included) is refused with a ValueError naming it"""
    return _db("ceiling_db", ceiling_db, MIN_CEILING_DB, MAX_CEILING_DB)


def delay_samples(A):
    """input samples a stream holds back until its next push (or its flush)"""
    return A - 1


def history(A, H):
    """input samples a stream keeps between two pushes"""
    return H + 2 * A - 2


def emitted(total_in, A):
    """outputs a stream has emitted before its flush once total_in samples have arrived"""
    return max(0, int(total_in) - (A - 1))


def counts(A, total_in, n_in, flush=False):
    """(o0, n_out) of a push of n_in samples to a stream that has taken total_in so far: the index of the first output it emits and
    how many.  Integers only: the streamer sizes its copies with it, without a device sync."""
    o0 = emitted(total_in, A)
    o1 = int(total_in) + int(n_in) if flush else emitted(int(total_in) + int(n_in), A)
    return o0, o1 - o0


def push_width(A, H):
    """input samples one row of a device push may bring"""
    return BUF - history(A, H) - (A - 1)


def _window_min(q, W):
    """out[t] = min q[t .. t + W - 1], t < len(q) - W + 1, by doubling"""
    m, s = q, 1
    while 2 * s <= W:
        m = np.minimum(m[:-s], m[s:])
        s *= 2
    n = q.shape[0] - W + 1
    return np.minimum(m[:n], m[W - s:W - s + n])


def _solve(x, g, c, A, H):
    """(y, a) of every sample of x (float32), r = 1 outside it"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        u = np.float32(g) * x
        u = np.where(np.isfinite(u), u, np.float32(0.0)).astype(np.float32)
        au = np.abs(u)
        r = np.where(au <= c, np.float32(1.0), np.float32(c) / np.where(au <= c, np.float32(1.0), au)).astype(np.float32)
    q = np.floor(r * np.float32(ONE)).astype(np.int64)
    qp = np.concatenate([np.full(H + A - 1, ONE, dtype=np.int64), q, np.full(A - 1, ONE, dtype=np.int64)])
    h = _window_min(qp, H + A)                                 # h[j], j = -(A - 1) .. n - 1
    cs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(h)])
    S = cs[A:] - cs[:-A]                                       # S[i], i = 0 .. n - 1
    a = S.astype(np.float32) / np.float32(A * ONE)
    y = np.minimum(np.maximum(a * u, -np.float32(c)), np.float32(c))
    return y.astype(np.float32), a.astype(np.float32)


def level_ref(x, volume_db=0.0, ceiling_db=DEFAULT_CEILING_DB, rate=24000, return_gain=False, A=None, H=None):
    """The definition in numpy: a 1-D signal of n samples -> n float32 samples (and a, on request).  A, H: in place of params(rate)."""
    g, c = gain_of(volume_db), ceiling_of(ceiling_db)
    pa, ph = params(rate) if A is None or H is None else (None, None)
    A, H = int(pa if A is None else A), int(ph if H is None else H)
    if not (1 <= A <= MAX_A) or H < 0:
        raise ValueError(f"level: A = {A} must lie in [1, {MAX_A}] and H = {H} be >= 0")
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    y, a = _solve(x, g, c, A, H)
    return (y, a) if return_gain else y


class HostLevel:
    """The streaming form on the host, one stream, float32 torch: push(chunk) -> the samples that chunk completes, flush() -> the
    tail.  Whatever the cuts, the concatenation equals level_ref of the whole signal, bit for bit.  AudioStreamer runs CPU chunks
    through it."""

    def __init__(self, volume_db=0.0, ceiling_db=DEFAULT_CEILING_DB, rate=24000, A=None, H=None):
        self.gain, self.ceiling = gain_of(volume_db), ceiling_of(ceiling_db)
        pa, ph = params(rate) if A is None or H is None else (None, None)
        self.A, self.H = int(pa if A is None else A), int(ph if H is None else H)
        if not (1 <= self.A <= MAX_A) or self.H < 0:
            raise ValueError(f"level: A = {self.A} must lie in [1, {MAX_A}] and H = {self.H} be >= 0")
        self.delay_samples, self._nh = delay_samples(self.A), history(self.A, self.H)
        self.reset()

    def reset(self):
        self.total_in = 0
        self.flushed = False
        self._hist = np.zeros(self._nh, dtype=np.float32)           # x[total_in - history .. total_in)

    def counts(self, n_in, flush=False):
        return counts(self.A, self.total_in, n_in, flush)

    def push(self, chunk, flush=False):
        if self.flushed:
            raise RuntimeError("HostLevel: the stream has been flushed; reset() it before its next push")
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu().numpy()
        n_in = x.shape[0]
        o0, n_out = self.counts(n_in, flush)
        buf = np.concatenate([self._hist, x, np.zeros(self.A - 1, dtype=np.float32)])
        y, _ = _solve(buf, self.gain, self.ceiling, self.A, self.H)
        b0 = o0 - self.total_in + self._nh
        self._hist = buf[n_in:n_in + self._nh].copy()
        self.total_in += n_in
        self.flushed = bool(flush)
        return torch.from_numpy(np.ascontiguousarray(y[b0:b0 + n_out]))

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def level_host(x, volume_db=0.0, ceiling_db=DEFAULT_CEILING_DB, rate=24000):
    """one-shot float32 on the host: HostLevel over the whole signal"""
    return HostLevel(volume_db, ceiling_db, rate).push(x, flush=True)
