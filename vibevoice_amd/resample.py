"""Sample-rate conversion by a rational factor L / M: the filter design, the definition of every output sample and the host's
bookkeeping.  csrc/resample.hip evaluates the same definition on the device in fp32 (Engine.resampler / Engine.resample); this
module needs no GPU and is what the kernels are tested against.

Definition.  design() gives L / M = dst / src reduced, T taps per phase and coef [L][T], the phases of one Kaiser-windowed sinc h of
odd length N0 = L * T - 1 at L * src_rate (coef[p][t] = h[p + t * L], one zero tap appended).  Output sample m is the input signal at
time m * M / L input samples, the input taken as zero before its first sample and after its last:

    k = m * M + (N0 - 1) / 2,  q = k // L,  p = k % L:      y[m] = sum_{t = 0 .. T - 1} coef[p][t] * x[q - t]      (in that order)

and a signal of n samples yields ceil(n * L / M) outputs.  The prototype's length is odd so that its centre (N0 - 1) / 2 is a whole
tap: with an even length the output sits a fraction of a sample off the input.

Streaming.  The value of output m depends on m and the input only, never on how the input was cut into pushes: a push emits every
output whose newest input sample q has arrived and holds the rest back, the flush emits the tail against zeros.  The last T / 2 input
samples of a stream therefore wait for the next push: T / 2 / src_rate seconds, 1.3 ms at 24 -> 48 kHz (T = 64), 4 ms at 24 -> 8 kHz
(T = 192).  emitted() and counts() are that rule in integers; the engine's C side (vv_resample_rows) computes the same figures.
"""
import functools
import math

import numpy as np
import torch


@functools.lru_cache(maxsize=64)
def _design(src_rate, dst_rate, zeros, atten_db):
    src_rate, dst_rate = int(src_rate), int(dst_rate)
    if src_rate < 1 or dst_rate < 1:
        raise ValueError(f"sample rates must be positive: {src_rate} -> {dst_rate}")
    g = math.gcd(src_rate, dst_rate)
    L, M = dst_rate // g, src_rate // g
    T = -((-2 * zeros * max(L, M)) // L)            # ceil(2 zeros max(1, M / L)) in integers
    T += T & 1
    h, _ = _prototype(L, M, T, atten_db)
    coef = np.ascontiguousarray(h.reshape(T, L).T.astype(np.float32))      # coef[p][t] = h[p + t L]
    coef.setflags(write=False)
    return L, M, T, coef


def design(src_rate, dst_rate, zeros=32, atten_db=80.0):
    """(L, M, T, coef): L / M = dst_rate / src_rate reduced, T taps per phase (even), coef [L, T] float32 (read-only, shared between
    calls).  zeros: zero crossings of the sinc on either side at the lower of the two rates; atten_db: the Kaiser window's stopband."""
    return _design(int(src_rate), int(dst_rate), int(zeros), float(atten_db))


def _prototype(L, M, T, atten_db):
    n0 = L * T - 1
    beta = 0.1102 * (atten_db - 8.7)
    dw = (atten_db - 7.95) / (2.285 * (n0 - 1)) / (2.0 * np.pi)       # transition width, cycles per sample at L * src_rate
    fc = 0.5 / max(L, M) - dw / 2.0                                   # the stopband starts at the lower Nyquist frequency
    n = np.arange(n0, dtype=np.float64) - (n0 - 1) / 2.0
    h = L * 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(n0, beta)    # gain L: one input sample in L at the prototype's rate
    h = 0.5 * (h + h[::-1])                                           # symmetric to the last bit
    return np.concatenate([h, np.zeros(1)]), dw


def prototype(src_rate, dst_rate, zeros=32, atten_db=80.0):
    """The float64 prototype h (length L * T, the appended zero tap included) that design() rounds to float32, and its transition
    width dw in cycles per sample at L * src_rate."""
    L, M, T, _ = design(src_rate, dst_rate, zeros, atten_db)
    return _prototype(L, M, T, float(atten_db))


def delay_samples(T):
    """input samples a stream holds back until its next push (or its flush)"""
    return T // 2


def total_out(n_in, L, M):
    """outputs of a whole signal of n_in samples: ceil(n_in L / M)"""
    return -((-int(n_in) * L) // M)


def emitted(total_in, L, M, T):
    """outputs a stream has emitted before its flush once total_in samples have arrived: every m with (m M + D) // L < total_in,
    D = (L T - 2) / 2"""
    a = int(total_in) * L - (L * T - 2) // 2 - 1
    return 0 if a < 0 else a // M + 1


def counts(L, M, T, total_in, n_in, flush=False):
    """(m0, n_out) of a push of n_in samples to a stream that has taken total_in so far: the index of the first output it emits and
    how many.  Integers only: the streamer sizes its copies with it, without a device sync."""
    m0 = emitted(total_in, L, M, T)
    m1 = total_out(total_in + n_in, L, M) if flush else emitted(total_in + n_in, L, M, T)
    return m0, m1 - m0


# What one push of the device kernel takes per row, mirrored from the C side (vv_resample_rows refuses more of either): at most
# MAX_OUT outputs (VV_RS_MAX_OUT, csrc/vv_common.h), and the filter table [L][T + 1], the T history samples, the chunk and T / 2 zeros
# within LDS_BYTES of LDS (vv_resample_lds_bytes, csrc/resample.hip).
MAX_OUT, LDS_BYTES = 8192, 65536 - 64


def push_width(L, M, T, totals, remaining, flush=False):
    """input samples per row the next push accepts from rows that still have remaining[i] for a stream that has taken totals[i]: all of
    them where that fits the kernel, else a width that fits whatever the streams' state"""
    lds_max = LDS_BYTES // 4 - L * (T + 1) - T - T // 2
    if max(remaining) <= lds_max and all(counts(L, M, T, t, r, flush)[1] <= MAX_OUT for t, r in zip(totals, remaining)):
        return max(remaining)
    return max(1, min((MAX_OUT - 1) * M // L - T // 2 - 1, lds_max))


def _outputs(coef, L, M, T, buf, first_index, m0, n_out, xp):
    """y[m0 .. m0 + n_out) from buf, which holds x[first_index ...] (zeros where the signal has none); xp: numpy or torch"""
    m = np.arange(m0, m0 + n_out, dtype=np.int64)
    k = m * M + (L * T - 2) // 2
    q, p = k // L, k % L
    at = q - first_index
    if xp is torch:
        at, p = torch.from_numpy(at), torch.from_numpy(p)
    acc = xp.zeros(n_out, dtype=buf.dtype)
    for t in range(T):                                  # the sum in tap order, one rounding per product and per addition
        acc = acc + coef[p, t] * buf[at - t]
    return acc


def resample_ref(x, src_rate, dst_rate, dtype=np.float64, zeros=32, atten_db=80.0):
    """The definition in numpy: a 1-D signal -> ceil(n L / M) samples, products and sums in `dtype` (the float32 table widened)."""
    L, M, T, coef = design(src_rate, dst_rate, zeros, atten_db)
    x = np.asarray(x, dtype=dtype).reshape(-1)
    n = x.shape[0]
    buf = np.concatenate([np.zeros(T, dtype=dtype), x, np.zeros(T, dtype=dtype)])
    return _outputs(coef.astype(dtype), L, M, T, buf, -T, 0, total_out(n, L, M), np)


class HostResampler:
    """The streaming form on the host, one stream, float32 torch: push(chunk) -> the samples that chunk completes, flush() -> the tail.
    Whatever the cuts, the concatenation equals push(whole signal) + flush(), bit for bit.  AudioStreamer runs CPU chunks through it."""

    def __init__(self, src_rate, dst_rate, zeros=32, atten_db=80.0):
        self.src_rate, self.dst_rate = int(src_rate), int(dst_rate)
        self.L, self.M, self.T, coef = design(src_rate, dst_rate, zeros, atten_db)
        self.taps, self.delay_samples = self.T, delay_samples(self.T)
        self._coef = torch.from_numpy(np.array(coef))
        self.reset()

    def reset(self):
        self.total_in = 0
        self.flushed = False
        self._hist = torch.zeros(self.T, dtype=torch.float32)       # x[total_in - T .. total_in)

    def counts(self, n_in, flush=False):
        return counts(self.L, self.M, self.T, self.total_in, n_in, flush)

    def push(self, chunk, flush=False):
        if self.flushed:
            raise RuntimeError("HostResampler: the stream has been flushed; reset() it before its next push")
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu()
        n_in = x.shape[0]
        m0, n_out = self.counts(n_in, flush)
        buf = torch.cat([self._hist, x, torch.zeros(self.T // 2, dtype=torch.float32)])
        y = _outputs(self._coef, self.L, self.M, self.T, buf, self.total_in - self.T, m0, n_out, torch)
        self._hist = buf[n_in:n_in + self.T].clone()
        self.total_in += n_in
        self.flushed = bool(flush)
        return y

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def resample_host(x, src_rate, dst_rate):
    """one-shot float32 on the host: HostResampler over the whole signal"""
    return HostResampler(src_rate, dst_rate).push(x, flush=True)
