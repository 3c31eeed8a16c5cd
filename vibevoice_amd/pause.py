"""Pauses: cap the silences of a stream and trim its lead-in: the definition of every delivered sample and the host's bookkeeping.
csrc/pause.hip evaluates the same definition on the device (Engine.pause / Engine.shorten_pauses), with no tolerance; this module needs
no GPU and is what the kernels are tested against.

Definition, at the delivered rate (8000 .. 48000 Hz), in segments of seg = rate // 100 samples (10 ms; 80 at 8 kHz, 220 at 22.05 kHz,
240 at 24 kHz, 480 at 48 kHz).  Every decision is an integer one:

    q = clamp(rint(fl32(x 32768)), -32768, 32768), a non-finite x counts as q = 0;   E = sum of q^2 over the segment (64-bit)
    a segment is quiet iff E < Theta,   Theta = floor(seg (32768 10^(threshold_db / 20))^2)       (theta(), float64 on the host, once)

A cap of ms milliseconds is C = int(ms rate / (1000 seg) + 0.5) segments (caps()); no cap is C = 2^31 - 1.  max_pause_ms caps every quiet
run, max_lead_ms the one in front of the stream's first loud segment (None there: max_pause_ms applies).  With the cap C in force,
T = min(C // 2, 10) and H = C - T, a quiet run of R whole segments is delivered like this:

    the first H segments go out as they arrive;
    from segment H + 1 on the stream holds the last T quiet segments back (a ring) and keeps a copy of segment H + 1 (`first`);
    the next loud segment, or the flush (the end of the stream counts as speech resuming), releases what is held:
        R <= C: everything held, verbatim: nothing was dropped;
        R >  C: (R - C) seg samples are dropped; the first held segment b goes out joined with a = first, sample j of it
                fl(fl(a[j] u[j]) + fl(b[j] w[j])), w[j] = fl32((j + 0.5) / seg), u[j] = fl32(1 - (j + 0.5) / seg) (weights(): two
                products and one sum, each rounded once, never fused); the other T - 1 follow verbatim;
    then the loud segment.

So a run keeps min(R, C) segments, its first H and its last T, the seam between them a 10 ms cross-fade; a stream with no run above its
cap passes bit for bit with the same length, and speech is never delayed by more than one segment: only silence is held back.  Samples
that do not yet fill a segment wait for the next push (at most seg - 1, under 10 ms); the flush releases the held tail, then emits the
partial segment verbatim.  What a stream delivers depends on its input only, never on how that was cut into pushes.  How MUCH a push
delivers depends on the data: unlike the other stages' counts this one's are not host integers; at most max_out() samples a push.
"""
import numpy as np
import torch

MIN_RATE, MAX_RATE = 8000, 48000
MIN_PAUSE_MS, MAX_PAUSE_MS = 100.0, 5000.0
MIN_LEAD_MS, MAX_LEAD_MS = 0.0, 5000.0
MIN_THRESHOLD_DB, MAX_THRESHOLD_DB = -80.0, -20.0
DEFAULT_THRESHOLD_DB = -50.0
NO_CAP = (1 << 31) - 1          # C of "no cap"
MAX_T = 10                      # segments a stream holds back at most
MAX_IN = 7680                   # input samples one row of a device push may bring (csrc/vv_common.h: VV_PS_MAX_IN)
STATE_FLOATS = (2 + MAX_T) * (MAX_RATE // 100)      # samples a stream keeps on the device: open segment, ring, first (VV_PS_FLOATS)


def seg_of(rate):
    """samples of a segment (10 ms) at `rate`; a rate outside 8000 .. 48000 is refused by name"""
    try:
        r = int(rate)
    except (TypeError, ValueError):
        raise ValueError(f"pause: rate must be an integer in [{MIN_RATE}, {MAX_RATE}] Hz, got {rate!r}") from None
    if not (MIN_RATE <= r <= MAX_RATE) or r != rate:
        raise ValueError(f"pause: rate must be an integer in [{MIN_RATE}, {MAX_RATE}] Hz, got {rate!r}")
    return r // 100


def _ms(what, value, lo, hi):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"pause: {what} must be a number in [{lo:g}, {hi:g}], got {value!r}") from None
    if not (lo <= v <= hi):                                   # a NaN compares false
        raise ValueError(f"pause: {what} must lie in [{lo:g}, {hi:g}], got {value!r}")
    return v


def pause_ms_of(max_pause_ms):
    """max_pause_ms as a float in [100, 5000] or None (no cap); anything else (NaN included) is refused with a ValueError naming it"""
    return None if max_pause_ms is None else _ms("max_pause_ms", max_pause_ms, MIN_PAUSE_MS, MAX_PAUSE_MS)


def lead_ms_of(max_lead_ms):
    """max_lead_ms as a float in [0, 5000] or None (max_pause_ms applies); anything else is refused with a ValueError naming it"""
    return None if max_lead_ms is None else _ms("max_lead_ms", max_lead_ms, MIN_LEAD_MS, MAX_LEAD_MS)


def threshold_of(threshold_db):
    """threshold_db as a float in [-80, -20]; anything else (NaN included) is refused with a ValueError naming it"""
    return _ms("threshold_db", threshold_db, MIN_THRESHOLD_DB, MAX_THRESHOLD_DB)


def theta(rate, threshold_db=DEFAULT_THRESHOLD_DB):
    """Theta, the integer a segment's energy is compared with"""
    seg, db = seg_of(rate), threshold_of(threshold_db)
    return int(np.floor(np.float64(seg) * (np.float64(32768.0) * np.float64(10.0) ** (np.float64(db) / np.float64(20.0))) ** 2))


def caps(rate, max_pause_ms=None, max_lead_ms=None):
    """(C, C0): the cap of every quiet run and of the one in front of the first loud segment, in segments"""
    seg = seg_of(rate)
    p, l = pause_ms_of(max_pause_ms), lead_ms_of(max_lead_ms)
    C = NO_CAP if p is None else int(p * rate / (1000 * seg) + 0.5)
    C0 = C if l is None else int(l * rate / (1000 * seg) + 0.5)
    return C, C0


def hold(C):
    """(T, H) of a cap: the segments held back at most, and the ones that go out as they arrive"""
    T = min(int(C) // 2, MAX_T)
    return T, int(C) - T


def weights(rate):
    """(w, u), float32 [seg] each: the join is fl(fl(a u) + fl(b w))"""
    seg = seg_of(rate)
    t = (np.arange(seg, dtype=np.float64) + 0.5) / np.float64(seg)
    return t.astype(np.float32), (np.float64(1.0) - t).astype(np.float32)


def max_out(n_in, rate=24000):
    """upper bound of what one push of n_in samples delivers, the flush included: the partial segment and the held tail with it"""
    seg = seg_of(rate)
    return int(n_in) + (seg - 1) + MAX_T * seg


def energies(x, rate):
    """E of every whole segment of x: int64 [len(x) // seg]"""
    seg = seg_of(rate)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.shape[0] // seg
    x = x[:n * seg]
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * np.float32(32768.0)
        q = np.where(np.isfinite(x), np.clip(np.rint(np.where(np.isfinite(x), v, np.float32(0.0))), -32768.0, 32768.0), 0.0).astype(np.int64)
    return (q * q).reshape(n, seg).sum(axis=1)


def classify(x, rate, threshold_db=DEFAULT_THRESHOLD_DB):
    """quiet (True) or loud of every whole segment of x"""
    return energies(x, rate) < theta(rate, threshold_db)


def join(a, b, w, u):
    """the seam: a fades out under u while b fades in under w, three roundings a sample"""
    return (a * u).astype(np.float32) + (b * w).astype(np.float32)


class HostPause:
    """The streaming form on the host, one stream, float32 torch: push(chunk) -> what that chunk releases, flush() -> the tail.
    Whatever the cuts, the concatenation equals shorten() of the whole signal, bit for bit.  dropped: the samples dropped so far.
    AudioStreamer runs CPU chunks through it."""

    def __init__(self, rate=24000, max_pause_ms=None, max_lead_ms=None, threshold_db=DEFAULT_THRESHOLD_DB):
        self.seg, self.rate = seg_of(rate), int(rate)
        self.C, self.C0 = caps(rate, max_pause_ms, max_lead_ms)
        self.theta = theta(rate, threshold_db)
        self.w, self.u = weights(rate)
        self.reset()

    def reset(self):
        self.total_in = self.total_out = self.dropped = 0
        self.flushed = False
        self.run, self.started = 0, False
        self._held, self._first = [], None                    # the ring, oldest first; segment H + 1 of the run
        self._carry = np.zeros(0, dtype=np.float32)

    def _release(self, out):
        cap = self.C if self.started else self.C0
        if self.run > cap:
            self.dropped += (self.run - cap) * self.seg
            if self._held:
                out.append(join(self._first, self._held[0], self.w, self.u))
                out.extend(self._held[1:])
        else:
            out.extend(self._held)
        self._held = []

    def push(self, chunk, flush=False):
        if self.flushed:
            raise RuntimeError("HostPause: the stream has been flushed; reset() it before its next push")
        x = torch.as_tensor(chunk).detach().reshape(-1).to(torch.float32).cpu().numpy()
        buf = np.concatenate([self._carry, x])
        seg, n = self.seg, buf.shape[0] // self.seg
        quiet = energies(buf, self.rate) < self.theta
        out = []
        for s in range(n):
            piece = buf[s * seg:(s + 1) * seg]
            if quiet[s]:
                T, H = hold(self.C if self.started else self.C0)
                self.run = min(self.run + 1, NO_CAP)
                if self.run <= H:
                    out.append(piece)
                else:
                    if self.run == H + 1:
                        self._first = piece
                    if T:
                        self._held = (self._held + [piece])[-T:]
            else:
                self._release(out)
                out.append(piece)
                self.run, self.started = 0, True
        self._carry = buf[n * seg:].copy()
        if flush:
            self._release(out)
            out.append(self._carry)
            self._carry = np.zeros(0, dtype=np.float32)
            self.flushed = True
        y = np.concatenate(out).astype(np.float32) if out else np.zeros(0, dtype=np.float32)
        self._held = [h.copy() for h in self._held]
        self._first = None if self._first is None else self._first.copy()
        self.total_in += x.shape[0]
        self.total_out += y.shape[0]
        return torch.from_numpy(np.ascontiguousarray(y))

    def flush(self):
        return self.push(torch.zeros(0), flush=True)


def shorten(x, rate=24000, max_pause_ms=None, max_lead_ms=None, threshold_db=DEFAULT_THRESHOLD_DB):
    """The definition over a whole 1-D signal -> (y float32, dropped): len(x) - len(y) == dropped"""
    h = HostPause(rate, max_pause_ms, max_lead_ms, threshold_db)
    y = h.push(np.asarray(x, dtype=np.float32).reshape(-1), flush=True).numpy()
    return y, h.dropped
