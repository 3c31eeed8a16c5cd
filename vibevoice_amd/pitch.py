"""Pitch: a shift by s semitones is a tempo change by 1 / r (tempo.py, which keeps the pitch and absorbs the change of duration)
followed by resampling by r = 2^(s / 12), here a variable-ratio band-limited resampler P / Q over ONE prototype table that every ratio
shares: the definition of every output sample and the host's bookkeeping.  csrc/pitch.hip evaluates the same definition on the device
in fp32, each row of a launch at its own ratio (Engine.pitch / Engine.pitch_shift); this module needs no GPU and is what the kernels are
tested against.

This is a resampling shifter: FORMANTS MOVE WITH THE PITCH.  A few semitones read as the same voice, higher or lower; beyond that the
character of the voice changes (towards a smaller or a larger speaker).  Nothing here estimates or restores the spectral envelope:
formant.py does, as a stage of its own in front of this one -- a warp of the envelope by exactly Q / P (AudioStreamer(pitch=s,
formant=0.0), Engine.pitch_shift(..., formant=0.0)) puts the formants back where they were.

Ratio.  ratio(s), s in [-12, +12]: the fraction P / Q with 1 <= P, Q <= 100 (and 1/2 <= P / Q <= 2) nearest to 2^(s / 12) in log
frequency, reduced, ties to the smaller Q.  Both terms stay at or below 100 so that tempo.ratio(Q / P) recovers Q / P exactly.  The
worst error is 600 log2(100 / 99) = 8.70 cents, next to unison (the neighbours of 1/1 are 100/99 and 99/100); whole semitones are far
closer (+1: 89/84, +7: 3/2).  s = 0 gives (1, 1): no stage.

Resampler.  Output m of a stream is the input at time m P / Q input samples, the input taken as zero outside itself.  With
den = max(P, Q), rho = float32(Q) / float32(den) (the cutoff scale, below 1 when the pitch goes up), k = m P, q = k // Q, a = k % Q and
Tn = ceil(Z den / Q) (at most 64):

    y[m] = sum_{t = -Tn .. Tn} (rho c(a, t)) x[q - t]                      in that order, from 0

c(a, t) is the prototype at (a + t Q) / den zero crossings: a Kaiser-windowed sinc with Z = 32 zero crossings either side, by the design
rule of resample._prototype (80 dB, the stopband starts at the Nyquist frequency, symmetrised), sampled R = 256 times per crossing
into the float32 table H [Z R + 1] of its non-negative half (table(): 32 KB + 4 B).  The look-up is linear interpolation at an exactly
integer position, by the symmetry on the magnitude:

    num = |a + t Q| R,  i = num // den,  f = float32(num % den) / float32(den)            (one correctly rounded division)
    c = H[i] + f (H[i + 1] - H[i])  where i < Z R,  0 beyond the table

Rounding, fp32.  The kernels (streaming and one-shot, the same bits for the same m): d = fl(H[i + 1] - H[i]), c = fma(f, d, H[i]),
w = fl(rho c), acc = fma(w, x[q - t], acc).  This module's float32 forms (HostPitch, pitch_host): the same operations with a rounding
per product and per sum, no fma.  pitch_ref: the same operations in float64 over the float32 table, f and rho.

Unison.  The stopband starts at the Nyquist frequency, so the cutoff lies below it: the prototype's centre is 0.92, not 1, and its
values at the whole crossings are not 0.  Forcing those table entries to 1 and 0 would break every ratio that reads them (2/1 reads a
whole crossing at every other tap).  P / Q = 1 / 1 is therefore the identity BY DEFINITION: Tn = 0 and c = 1, y[m] = x[m], bit for bit,
nothing held back.  That is what a sample index at 0 semitones passes through in a batch where others are shifted.

Streaming.  The value of output m depends on m and the input only, never on how the input was cut into pushes: a push emits every
output whose newest input sample q + Tn has arrived and holds the rest back, the flush emits the tail against zeros; a signal of n
samples yields total_out = ceil(n Q / P).  A stream holds back Tn <= 64 input samples (2.7 ms) until its next push and keeps 2 * 64 of
history.  emitted() and counts() are that rule in integers (correct for totals beyond 2^32); the engine's C side (vv_pitch_rows)
computes the same figures.

The whole effect.  shift_ref(x, s, speed): tempo.stretch_ref at tempo.ratio(speed Q / P), then the resampler at P / Q:
ceil(ceil(n Qt / Pt) Q / P) samples, n / speed to within a sample and tempo's own rounding of the combined speed.  A combined speed
outside [0.5, 2.0] is refused; one of exactly 1 (speed 1.5 with +7 semitones) means no tempo stage, plain resampling.
"""
import functools
import math

import numpy as np
import torch

from . import tempo as _tp

Z, R = 32, 256                  # zero crossings either side, table entries per crossing
ATTEN_DB = 80.0
HISTORY = 128                   # 2 * 64 >= 2 Tn: what a stream keeps of its input between two pushes
MAX_TN = 64
MIN_SEMITONES, MAX_SEMITONES = -12.0, 12.0
# What one push of the device kernel takes per row, mirrored from the C side (VV_PT_MAX_IN / VV_PT_MAX_OUT, csrc/vv_common.h)
MAX_IN, MAX_OUT = 7552, 8192


@functools.lru_cache(maxsize=1)
def table():
    """H [Z R + 1] float32 (read-only): the non-negative half of the prototype, H[j] at j / R zero crossings"""
    n0 = 2 * Z * R + 1
    beta = 0.1102 * (ATTEN_DB - 8.7)
    dw = (ATTEN_DB - 7.95) / (2.285 * (n0 - 1)) / (2.0 * np.pi)      # transition width, cycles per table entry
    fc = 0.5 / R - dw / 2.0                                           # the stopband starts at the Nyquist frequency
    n = np.arange(n0, dtype=np.float64) - Z * R
    h = R * 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(n0, beta)    # gain R: one sample in R at the table's rate
    h = 0.5 * (h + h[::-1])                                           # symmetric to the last bit
    H = np.ascontiguousarray(h[Z * R:].astype(np.float32))
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=4096)
def _ratio(v):
    target = v / 12.0
    best, best_err = (1, 1), abs(target)
    for Q in range(1, 101):
        x = 2.0 ** target * Q
        for P in (math.floor(x), math.ceil(x)):
            if 1 <= P <= 100 and P <= 2 * Q and Q <= 2 * P:
                err = abs(math.log2(P / Q) - target)
                if err < best_err:                                    # Q ascends: a tie stays with the smaller Q, the reduced form
                    best, best_err = (P, Q), err
    return best


def ratio(semitones):
    """(P, Q) of a shift in [-12, +12] semitones; anything else (NaN included) is refused with a ValueError naming it"""
    try:
        v = float(semitones)
    except (TypeError, ValueError):
        raise ValueError(f"pitch: semitones must be a number in [{MIN_SEMITONES:g}, {MAX_SEMITONES:g}], got {semitones!r}") from None
    if not (MIN_SEMITONES <= v <= MAX_SEMITONES):                     # a NaN compares false
        raise ValueError(f"pitch: semitones must lie in [{MIN_SEMITONES:g}, {MAX_SEMITONES:g}], got {semitones!r}")
    return _ratio(v)


def cents_off(semitones):
    """how far ratio(semitones) lies from the shift asked for, in cents"""
    P, Q = ratio(semitones)
    return 1200.0 * math.log2(P / Q) - 100.0 * float(semitones)


def tempo_speed(speed, semitones):
    """the speed the tempo stage in front of the resampler runs at: speed Q / P.  Outside [0.5, 2.0] it is refused, naming both"""
    P, Q = ratio(semitones)
    try:
        v = float(speed) * Q / P
    except (TypeError, ValueError):
        raise ValueError(f"pitch: speed must be a number, got {speed!r}") from None
    if not (_tp.MIN_SPEED <= v <= _tp.MAX_SPEED):
        raise ValueError(f"pitch: speed={speed!r} with semitones={semitones!r} asks the tempo stage for speed * {Q} / {P} = {v:g}, "
                         f"outside [{_tp.MIN_SPEED}, {_tp.MAX_SPEED}]")
    return v


def taps(P, Q):
    """Tn: the filter reaches Tn input samples either side of an output's position (0 at 1/1: the identity)"""
    return 0 if P == Q else -((-Z * max(P, Q)) // Q)


def delay_samples(P, Q):
    """input samples a stream holds back until its next push (or its flush)"""
    return taps(P, Q)


def total_out(n_in, P, Q):
    """outputs of a whole signal of n_in samples: ceil(n_in Q / P)"""
    return -((-int(n_in) * Q) // P)


def emitted(total_in, P, Q):
    """outputs a stream has emitted before its flush once total_in samples have arrived: every m with (m P) // Q + Tn < total_in"""
    room = int(total_in) - taps(P, Q)
    return 0 if room <= 0 else (room * Q - 1) // P + 1


def counts(P, Q, total_in, n_in, flush=False):
    """(m0, n_out) of a push of n_in samples to a stream that has taken total_in so far: the index of the first output it emits and
    how many.  Integers only: the streamer sizes its copies with it, without a device sync."""
    m0 = emitted(total_in, P, Q)
    m1 = total_out(total_in + n_in, P, Q) if flush else emitted(total_in + n_in, P, Q)
    return m0, m1 - m0


def push_width(ratios, totals, remaining, flush=False):
    """input samples per row the next push accepts from rows at ratios[i] = (P, Q) that still have remaining[i] for a stream that has
    taken totals[i]: all of them where that fits the kernel, else a width that fits whatever the streams' state"""
    if max(remaining) <= MAX_IN and all(counts(P, Q, t, r, flush)[1] <= MAX_OUT for (P, Q), t, r in zip(ratios, totals, remaining)):
        return max(remaining)
    return max(1, min(MAX_IN, min((MAX_OUT - 1) * P // Q - taps(P, Q) - 1 for P, Q in ratios)))


def _outputs(H, P, Q, buf, first_index, m0, n_out):
    """y[m0 .. m0 + n_out) from buf, which holds x[first_index ...] (zeros where the signal has none); the arithmetic runs in buf's
    dtype over H of the same dtype, one rounding per product and per sum"""
    dt = buf.dtype.type
    m = np.arange(m0, m0 + n_out, dtype=np.int64)
    if P == Q:
        return dt(0.0) + dt(1.0) * buf[m - first_index]
    den, Tn = max(P, Q), taps(P, Q)
    rho = dt(np.float32(Q) / np.float32(den))
    k = m * P
    q, a = k // Q, k % Q
    at = q - first_index
    acc = np.zeros(n_out, dtype=buf.dtype)
    for t in range(-Tn, Tn + 1):
        num = np.abs(a + t * Q) * R
        i, r = num // den, num % den
        f = (r.astype(np.float32) / np.float32(den)).astype(buf.dtype)
        inside = i < Z * R
        i = np.minimum(i, Z * R - 1)
        h0 = H[i]
        c = np.where(inside, h0 + f * (H[i + 1] - h0), dt(0.0))
        acc = acc + (rho * c) * buf[at - t]
    return acc


def resample_ref(x, P, Q, dtype=np.float64):
    """The resampler's definition in numpy at a given ratio: a 1-D signal -> ceil(n Q / P) samples, products and sums in `dtype`"""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    pad = np.zeros(MAX_TN, dtype=dtype)
    return _outputs(table().astype(dtype), P, Q, np.concatenate([pad, x, pad]), -MAX_TN, 0, total_out(x.shape[0], P, Q))


def pitch_ref(x, semitones, dtype=np.float64):
    """The resampler's definition at ratio(semitones): what the pitch stage alone does to a signal (its duration changes by Q / P)"""
    return resample_ref(x, *ratio(semitones), dtype=dtype)


def shift_ref(x, semitones, speed=1.0, dtype=np.float64):
    """The whole effect in numpy: the pitch moves by `semitones`, the duration by 1 / speed.  tempo.stretch_ref at speed Q / P (none
    where that is exactly 1), then the resampler at P / Q (none at 1/1)."""
    P, Q = ratio(semitones)
    v = tempo_speed(speed, semitones)
    y = np.asarray(x, dtype=np.float32).reshape(-1)
    Pt, Qt = _tp.ratio(v)
    if Pt != Qt:
        y = _tp.stretch_ref(y, v)
    return y.astype(dtype) if P == Q else resample_ref(y, P, Q, dtype=dtype)


def shift_len(n_in, semitones, speed=1.0):
    """samples shift_ref delivers for n_in: ceil(ceil(n Qt / Pt) Q / P)"""
    P, Q = ratio(semitones)
    Pt, Qt = _tp.ratio(tempo_speed(speed, semitones))
    return total_out(_tp.total_out(n_in, Pt, Qt), P, Q)


class HostPitch:
    """The resampler's streaming form on the host, one stream, float32 torch: push(chunk) -> the samples that chunk completes,
    flush() -> the tail.  Whatever the cuts, the concatenation equals push(whole signal) + flush(), bit for bit.  AudioStreamer runs
    CPU chunks through it, behind tempo.HostTempo."""

    def __init__(self, semitones):
        self.P, self.Q = ratio(semitones)
        self.taps = self.delay_samples = taps(self.P, self.Q)
        self.reset()

    def reset(self):
        self.total_in = 0
        self.flushed = False
        self._hist = np.zeros(HISTORY, dtype=np.float32)            # x[total_in - HISTORY .. total_in)

    def counts(self, n_in, flush=False):
        return counts(self.P, self.Q, self.total_in, n_in, flush)

    def push(self, chunk, flush=False):
        if self.flushed:
            raise RuntimeError("HostPitch: the stream has been flushed; reset() it before its next push")
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu().numpy()
        n_in = x.shape[0]
        m0, n_out = self.counts(n_in, flush)
        buf = np.concatenate([self._hist, x, np.zeros(MAX_TN, dtype=np.float32)])
        y = _outputs(table(), self.P, self.Q, buf, self.total_in - HISTORY, m0, n_out)
        self._hist = buf[n_in:n_in + HISTORY].copy()
        self.total_in += n_in
        self.flushed = bool(flush)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def pitch_host(x, semitones):
    """one-shot float32 on the host: HostPitch over the whole signal"""
    return HostPitch(semitones).push(x, flush=True)
