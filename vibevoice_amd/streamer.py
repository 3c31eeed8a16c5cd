"""AudioStreamer / AsyncAudioStreamer for the HIP path.  Same surface as the reference's
(vibevoice/modular/streamer.py: batch_size / stop_signal / timeout, put(audio_chunks, sample_indices),
end(sample_indices=None), finished_flags, audio_queues, iteration, get_stream; AsyncAudioStreamer :150-264) -- but put()
never blocks the generation loop: the chunk batch is copied into a pinned ring slot with ONE asynchronous D2H copy on a copy
stream ordered behind the producing stream, an event marks it, and a background thread hands finished chunks to the per-sample queues (the
reference does `.detach().cpu()` per sample = one stream sync each).

`pcm16=engine` converts each chunk to 16-bit PCM on the device before it leaves (vv_audio_to_pcm16: the arithmetic of the
gradio demo's convert_to_16_bit_wav, demo/gradio_demo.py:404-418,1058-1073), so the consumer receives int16 tensors and
the D2H copy is half the size of a bf16->fp32 round trip.

`sample_rate=R` (R other than 24000) delivers the audio at R Hz: put() resamples the chunk batch on the device, on the producing
stream, before the copy -- one launch (Engine.resampler, csrc/resample.hip), the int16 conversion included under pcm16 -- and the
delivered chunks are trimmed to what each sample emitted (a put that completes no output sample delivers nothing for that row).
The resampler is chunk-continuous: per sample, the concatenated chunks equal Engine.resample() of the concatenated 24 kHz chunks,
ceil(n * R / 24000) samples, bit for bit in float mode.  The price is latency: the last taps / 2 input samples of a sample wait for
its next chunk (1.3 ms at 48 kHz, 4 ms at 8 kHz); end(indices) flushes those tails as a last chunk in front of the stop signal,
close() does not.  Device chunks need an engine: the `pcm16=` one, or `engine=` where the chunks stay float; CPU chunks go through
resample.HostResampler on the host.  Stream id = sample index.

`speed=S` (a float in [0.5, 2.0], or one per sample index; anything but 1) changes the speaking rate and keeps the pitch: put() runs the
chunk batch through the engine's tempo stage (Engine.tempo, csrc/tempo.hip: WSOLA, vibevoice_amd/tempo.py is the definition) on the
producing stream, at 24 kHz; float chunks arrive as fp32.  Chunk-continuous like the resampler: per sample, the concatenated
chunks equal Engine.time_stretch() of the concatenated input (then Engine.resample() of that, under sample_rate), ceil(n / S) samples,
bit for bit in float mode.  A sample holds back at most 640 input samples (26.7 ms) until its next chunk; a put that completes no
block of 240 delivers nothing for that row; end(indices) flushes the tempo tail, then the resampler's.  Device chunks need an engine
(as above), CPU chunks go through tempo.HostTempo.

`pitch=S` (a float in [-12, +12] semitones, or one per sample index; anything but 0) moves the pitch and keeps the duration: the tempo
stage runs each index at speed * Q / P and a variable-ratio resampler behind it (Engine.pitch, csrc/pitch.hip; vibevoice_amd/pitch.py is the
definition) plays its output at P / Q = the fraction within 1..100 nearest to 2^(S / 12), each row of a launch at its own ratio, at 24 kHz,
in front of the rate resampler; float chunks arrive as fp32.  A resampling shifter: the formants move with the pitch, so a few semitones
read as the same voice higher or lower and more changes its character -- unless formant=0.0 is given with it (below).  Chunk-continuous: per sample, the concatenated chunks equal
Engine.pitch_shift(whole signal, S, speed), n / speed samples to within one and the tempo stage's rounding, bit for bit in float mode.
An index at 0 semitones passes the stage bit for bit; a combined speed outside [0.5, 2.0] is refused, one of exactly 1 (speed 1.5 with
+7 semitones) builds no tempo stage.  A sample holds back at most 64 more input samples (2.7 ms) behind the tempo stage's; end(indices)
flushes the tails in order: tempo, formant, pitch, resampler, level.  Device chunks need an engine (as above), CPU chunks go through
tempo.HostTempo and pitch.HostPitch.

`formant=F` (a float in [-12, +12] semitones, or one per sample index, None among them) says where the formants end up relative to the
untouched voice: a spectral-envelope warp (Engine.formant, csrc/formant.hip; vibevoice_amd/formant.py is the definition) between the tempo
stage and the pitch stage, at 24 kHz, each index at its own fraction ratio(F) * Q / P, reduced, P / Q the index's pitch ratio.  With
pitch=S, formant=0.0 is exactly Q / P and keeps the voice's formants (the same voice, higher or lower); formant=None leaves the pitch
stage's behaviour as it is.  Without pitch it is a timbre control on its own (voice size).  An index whose fraction is 1 / 1 (or None)
passes the stage bit for bit; a fraction outside [1/2, 2] is refused at construction, naming both arguments.  Chunk-continuous: per
sample, what reaches the next stage equals Engine.formant_warp() of what the stages in front deliver, as many samples, bit for bit.  A
sample holds back at most 1023 more input samples (42.6 ms, more than the tempo stage's 640) until its next chunk: a put that completes
no block of 256 delivers nothing for that row.  A gain of up to +30 dB per bin can pass full scale, so, as with loudness_lufs, such a
streamer always has a level stage behind it (ceiling -1 dB unless ceiling_db is given): no delivered sample exceeds the ceiling, and
under pcm16 the per-chunk rescale of the 16-bit rule never fires.  Device chunks need an engine (as above), CPU chunks go through
formant.HostFormant.

`volume_db=V` (a float in [-40, +24], or one per sample index) and `ceiling_db=C` (in [-20, 0]) set the output level: a gain and a
look-ahead peak limiter (Engine.level, csrc/level.hip; vibevoice_amd/level.py is the definition), the last stage, at the delivered rate.
The stage exists when ceiling_db is given or any volume_db is not 0 (the ceiling is then -1 dB unless given; an index at 0 dB still gets
the limiter); float chunks arrive as fp32.  Chunk-continuous like the other two: per sample, the concatenated chunks equal
Engine.apply_level() of what the stages in front deliver, as many samples, bit for bit in float mode.  No delivered sample exceeds
the ceiling, so under pcm16 the per-chunk rescale of the 16-bit rule never fires for such a stream: a loud passage is turned down
smoothly across chunk boundaries.  A sample holds back 5 ms less one sample until its next chunk; end(indices) flushes that tail last.
Device chunks need an engine (as above), CPU chunks go through level.HostLevel.

`loudness_lufs=T` (a float in [-36, -10], or one per sample index) brings each sample towards T LUFS (ITU-R BS.1770) while it is produced:
a causal adaptive leveller (Engine.loudness, csrc/loudness.hip; vibevoice_amd/loudness.py is the definition), the first stage, at
24 kHz, in front of the tempo change.  Its gain follows the loudness of the last three seconds of speech, comes down within 400 ms of a
louder speaker, starts at `loudness_start_db` (default 0 dB: the first 400 ms of speech pass at that gain) and never exceeds
`max_boost_db` (default 12); the two are refused without a target.  It holds nothing back and its flush adds nothing.  A boost can pass
full scale, so such a streamer always has a level stage behind it (ceiling -1 dB unless ceiling_db is given): no delivered sample
exceeds the ceiling.  Chunk-continuous: per sample, what reaches the next stage equals Engine.apply_loudness() of the concatenated
input, bit for bit.  Device chunks need an engine (as above), CPU chunks go through loudness.HostLoudness.

`max_pause_ms=P` (a float in [100, 5000], or one per sample index, None among them) caps every silence, `max_lead_ms=L` (in [0, 5000],
likewise) the one in front of a sample's first speech (None there: P applies), `pause_threshold_db` (in [-80, -20], default -50) says
what counts as silence: 10 ms segments whose energy lies below it (Engine.pause, csrc/pause.hip; vibevoice_amd/pause.py is the
definition), the last stage, behind the level, at the delivered rate (8 .. 48 kHz), so the caps mean what the listener gets.  A silence
longer than its cap keeps its beginning and its end around a 10 ms cross-fade; everything else passes bit for bit, an index with neither
cap included.  The stage exists when either cap is given for any index; the threshold alone is refused; float chunks arrive as fp32.
Chunk-continuous: per sample, the concatenated chunks equal pause.shorten() of what the stages in front deliver, bit for bit in float
mode.  Speech waits for its 10 ms segment to fill and no longer; only silence is held back (up to ten segments, released by the next
speech or by end()).  This is the one stage whose counts depend on the data: the host does not know how much a put delivers.  The launch
writes each row's count to device memory, the count words ride to a pinned companion of the ring slot on the copy stream in front of the
event the drain thread waits on anyway, and the thread trims the rows by them: put() still never waits for the device.  A put that
releases nothing for a row delivers nothing for it; end(indices) flushes this stage last: tempo, formant, pitch, resampler, level, pause.
Device chunks need an engine (as above), CPU chunks go through pause.HostPause.

The device stages form one chain (self._stages, _put_device): the leveller, the tempo change, the formant warp, the pitch resampler, the rate resampler, the level, the pauses, whichever exist, each an engine
row stage (engine._RowStage) pushed on the producing stream; the last one writes the ring slot's staging, as int16 under pcm16 (over
each row's own chunk), and with no stage the 16-bit conversion does, else the chunk itself is copied.  A chunk longer than one push of
a stage takes (stage.take()) is pushed in pieces and arrives as several.

The drain thread exits when every sample has ended (or on close()); its pinned ring goes back to a process-wide pool.
"""
import asyncio
import threading
from queue import Queue
from typing import Optional

import torch

_CLOSE = object()

# Pinned ring buffers outlive their streamer: a serving process creates one AudioStreamer per request, and a fresh pinned
# allocation per ring slot (hipHostMalloc, ~1 ms apiece; torch's host allocator only starts re-using freed blocks a couple of
# requests later) sat in front of every request's FIRST chunk -- 14 ms instead of 10.8 ms to first audio on the 1.5B request.
# A finished streamer hands its buffers back (every copy into them has completed: the drain thread waited on their events);
# the next one takes buffers of the same shape / dtype.  Bounded: _POOL_CAP buffers (a 3200-sample chunk is 6-13 KB).
_POOL_LOCK = threading.Lock()
_POOL: dict = {}
_POOL_CAP = 64


# ... and so does the copy stream: a stream's first operations pay for its hardware queue (measured: 2 ms per wait_event on a
# streamer's fresh stream, in front of the first request's first chunk); one per device, created once, warmed by warmup()
_COPY_STREAMS: dict = {}


def _copy_stream_for(device):
    key = (device.type, device.index)
    with _POOL_LOCK:
        st = _COPY_STREAMS.get(key)
        if st is None:
            st = _COPY_STREAMS[key] = torch.cuda.Stream(device=device)
        return st


def _pinned_take(shape, dtype):
    with _POOL_LOCK:
        lst = _POOL.get((tuple(shape), dtype))
        if lst:
            return lst.pop()
    return torch.empty(tuple(shape), dtype=dtype).pin_memory()


def _pinned_give(bufs):
    with _POOL_LOCK:
        held = sum(len(v) for v in _POOL.values())
        for b in bufs:
            if b is not None and held < _POOL_CAP:
                _POOL.setdefault((tuple(b.shape), b.dtype), []).append(b)
                held += 1


SOURCE_RATE = 24000      # what the acoustic decoder produces


def _speeds_of(speed, batch_size):
    """AudioStreamer's speed argument as one float per sample index; None where it asks for no change (absent, or 1 everywhere)"""
    if speed is None:
        return None
    from .tempo import ratio
    speeds = [float(speed)] * batch_size if not hasattr(speed, "__len__") else [float(v) for v in speed]
    if len(speeds) != batch_size:
        raise ValueError(f"AudioStreamer(speed=...): one value, or one per sample index ({batch_size}), got {len(speeds)}")
    if all(p == q for p, q in map(ratio, speeds)):            # ratio() refuses what lies outside [0.5, 2.0]
        return None
    return speeds


def _pitch_of(pitch, speed, batch_size):
    """AudioStreamer's pitch argument as (semitones, one per sample index; the speed the tempo stage in front runs each index at,
    speed * Q / P); None where it asks for no change (absent, or every index at the ratio 1 / 1)"""
    if pitch is None:
        return None
    from .pitch import ratio, tempo_speed
    semis = [float(pitch)] * batch_size if not hasattr(pitch, "__len__") else [float(v) for v in pitch]
    if len(semis) != batch_size:
        raise ValueError(f"AudioStreamer(pitch=...): one value, or one per sample index ({batch_size}), got {len(semis)}")
    if all(p == q for p, q in map(ratio, semis)):             # ratio() refuses what lies outside [-12, +12]
        return None
    speeds = [1.0] * batch_size if speed is None else ([float(speed)] * batch_size if not hasattr(speed, "__len__") else [float(v) for v in speed])
    return semis, [tempo_speed(v, s) for v, s in zip(speeds, semis)]    # refuses a combined speed outside [0.5, 2.0], naming both


def _formant_of(formant, pitch, batch_size):
    """AudioStreamer's formant argument as the warp (A, B) of each sample index, ratio(formant) * Q / P reduced ((1, 1) where the index
    has None); None where it asks for no stage (absent, or every index at 1 / 1)"""
    if formant is None:
        return None
    from .formant import fraction
    shifts = [formant] * batch_size if not hasattr(formant, "__len__") else list(formant)
    if len(shifts) != batch_size:
        raise ValueError(f"AudioStreamer(formant=...): one value (or None), or one per sample index ({batch_size}), got {len(shifts)}")
    semis = [None] * batch_size if pitch is None else ([float(pitch)] * batch_size if not hasattr(pitch, "__len__") else [float(v) for v in pitch])
    if len(semis) != batch_size:
        raise ValueError(f"AudioStreamer(pitch=...): one value, or one per sample index ({batch_size}), got {len(semis)}")
    ab = [(1, 1) if f is None else fraction(float(f), s) for f, s in zip(shifts, semis)]   # refuses a warp outside [1/2, 2], naming both
    return None if all(a == b for a, b in ab) else ab


def _volumes_of(volume_db, ceiling_db, batch_size):
    """AudioStreamer's level arguments as (one volume in dB per sample index, the ceiling in dB); None where they ask for no level
    stage (no ceiling, and no volume or 0 dB everywhere)"""
    from .level import DEFAULT_CEILING_DB, ceiling_of, gain_of
    vols = [0.0] * batch_size
    if volume_db is not None:
        vols = [float(volume_db)] * batch_size if not hasattr(volume_db, "__len__") else [float(v) for v in volume_db]
        if len(vols) != batch_size:
            raise ValueError(f"AudioStreamer(volume_db=...): one value, or one per sample index ({batch_size}), got {len(vols)}")
        for v in vols:
            gain_of(v)                                        # refuses what lies outside [-40, +24]
    if ceiling_db is None and all(v == 0.0 for v in vols):
        return None
    ceiling = DEFAULT_CEILING_DB if ceiling_db is None else float(ceiling_db)
    ceiling_of(ceiling)                                       # refuses what lies outside [-20, 0]
    return vols, ceiling


def _loudness_of(loudness_lufs, loudness_start_db, max_boost_db, batch_size):
    """AudioStreamer's loudness arguments as (targets in LUFS, start gains in dB, upper bounds in dB), one per sample index each; None
    where there is no target.  The other two alone are refused."""
    from .loudness import DEFAULT_BOOST_DB, boost_of, start_of, target_of
    if loudness_lufs is None:
        for name, v in (("loudness_start_db", loudness_start_db), ("max_boost_db", max_boost_db)):
            if v is not None:
                raise ValueError(f"AudioStreamer({name}=...) belongs to loudness_lufs=..., which is not given")
        return None
    cols = []
    for name, v, default, check in (("loudness_lufs", loudness_lufs, None, target_of), ("loudness_start_db", loudness_start_db, 0.0, start_of),
                                    ("max_boost_db", max_boost_db, DEFAULT_BOOST_DB, boost_of)):
        v = default if v is None else v
        col = [float(v)] * batch_size if not hasattr(v, "__len__") else [float(u) for u in v]
        if len(col) != batch_size:
            raise ValueError(f"AudioStreamer({name}=...): one value, or one per sample index ({batch_size}), got {len(col)}")
        for u in col:
            check(u)                                          # refuses what lies outside the parameter's range, by name
        cols.append(col)
    return tuple(cols)


def _pauses_of(max_pause_ms, max_lead_ms, pause_threshold_db, batch_size):
    """AudioStreamer's pause arguments as (caps in ms, lead caps in ms, thresholds in dB), one per sample index each, None among the
    caps where an index has none; None where no index has a cap.  The threshold alone is refused."""
    from .pause import DEFAULT_THRESHOLD_DB, MAX_THRESHOLD_DB, MIN_THRESHOLD_DB, lead_ms_of, pause_ms_of
    cols = []
    for name, v, check in (("max_pause_ms", max_pause_ms, pause_ms_of), ("max_lead_ms", max_lead_ms, lead_ms_of)):
        col = [v] * batch_size if not hasattr(v, "__len__") else list(v)
        if len(col) != batch_size:
            raise ValueError(f"AudioStreamer({name}=...): one value (or None), or one per sample index ({batch_size}), got {len(col)}")
        cols.append([check(u) for u in col])                  # refuses what lies outside the parameter's range, by name
    if all(u is None for col in cols for u in col):
        if pause_threshold_db is not None:
            raise ValueError("AudioStreamer(pause_threshold_db=...) belongs to max_pause_ms=... / max_lead_ms=..., neither of which is given")
        return None
    th = [pause_threshold_db] * batch_size if not hasattr(pause_threshold_db, "__len__") else list(pause_threshold_db)
    if len(th) != batch_size:
        raise ValueError(f"AudioStreamer(pause_threshold_db=...): one value, or one per sample index ({batch_size}), got {len(th)}")
    for i, u in enumerate(th):
        try:
            th[i] = DEFAULT_THRESHOLD_DB if u is None else float(u)
        except (TypeError, ValueError):
            th[i] = float("nan")
        if not (MIN_THRESHOLD_DB <= th[i] <= MAX_THRESHOLD_DB):   # a NaN compares false
            raise ValueError(f"AudioStreamer(pause_threshold_db=...) must lie in [{MIN_THRESHOLD_DB:g}, {MAX_THRESHOLD_DB:g}] dB, got {u!r}")
    return cols[0], cols[1], th


class AudioStreamer:
    def __init__(self, batch_size: int, stop_signal=None, timeout: Optional[float] = None, ring_slots: int = 8, pcm16=None,
                 sample_rate: Optional[int] = None, engine=None, speed=None, volume_db=None, ceiling_db=None, loudness_lufs=None,
                 loudness_start_db=None, max_boost_db=None, pitch=None, formant=None, max_pause_ms=None, max_lead_ms=None,
                 pause_threshold_db=None):
        self.batch_size = batch_size
        self._pause = _pauses_of(max_pause_ms, max_lead_ms, pause_threshold_db, batch_size)   # (caps, lead caps, thresholds) or None
        self._ps = None                            # Engine.pause (device chunks), one stream per sample index
        self._ps_host = {}                         # sample index -> pause.HostPause (CPU chunks)
        self._loud = _loudness_of(loudness_lufs, loudness_start_db, max_boost_db, batch_size)   # (targets, start gains, bounds) or None
        self._ld = None                            # Engine.loudness (device chunks), one stream per sample index
        self._ld_host = {}                         # sample index -> loudness.HostLoudness (CPU chunks)
        self._formant = _formant_of(formant, pitch, batch_size)   # the warp (A, B) of each sample index, or None: no formant stage
        self._fm = None                            # Engine.formant (device chunks), one stream per sample index
        self._fm_host = {}                         # sample index -> formant.HostFormant (CPU chunks)
        if (self._loud is not None or self._formant is not None) and ceiling_db is None:
            from .level import DEFAULT_CEILING_DB
            ceiling_db = DEFAULT_CEILING_DB        # a boost can pass full scale: the leveller and the warp are always followed by the limiter
        self._level = _volumes_of(volume_db, ceiling_db, batch_size)    # (volumes in dB, one per sample index; ceiling in dB), or None
        self._lv = None                            # Engine.level (device chunks), one stream per sample index
        self._lv_host = {}                         # sample index -> level.HostLevel (CPU chunks)
        self._speeds = _speeds_of(speed, batch_size)   # one per sample index, or None: no tempo stage anywhere
        self._pitch = None                         # semitones, one per sample index, or None: no pitch stage anywhere
        self._pt = None                            # Engine.pitch (device chunks), one stream per sample index
        self._pt_host = {}                         # sample index -> pitch.HostPitch (CPU chunks)
        shifted = _pitch_of(pitch, speed, batch_size)
        if shifted is not None:                    # the tempo stage absorbs the change of duration: it runs at speed * Q / P
            from .tempo import ratio as _tempo_ratio
            self._pitch = shifted[0]
            self._speeds = shifted[1] if any(p != q for p, q in map(_tempo_ratio, shifted[1])) else None
        self._tp = None                            # Engine.tempo (device chunks), one stream per sample index
        self._tp_host = {}                         # sample index -> tempo.HostTempo (CPU chunks)
        self.sample_rate = SOURCE_RATE if sample_rate is None else int(sample_rate)
        self._rs = None                            # Engine.resampler (device chunks), one stream per sample index
        self._rs_host = {}                         # sample index -> resample.HostResampler (CPU chunks)
        self._prod = None                          # the producing stream of the last device put: the tails are flushed on it
        self._lead = ()                            # a chunk's dimensions between the row and the samples, kept for the tail
        if self.sample_rate != SOURCE_RATE:
            eng = engine if engine is not None else pcm16
            if eng is not None:                    # without one, only CPU chunks are served (resample.HostResampler); put() refuses others
                self._rs = eng.resampler(SOURCE_RATE, self.sample_rate, batch_size)
        if self._loud is not None:
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._ld = eng.loudness(batch_size)
        if self._speeds is not None:
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._tp = eng.tempo(batch_size)
        if self._formant is not None:
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._fm = eng.formant(batch_size)
        if self._pitch is not None:
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._pt = eng.pitch(batch_size)
        if self._level is not None:
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._lv = eng.level(batch_size, rate=self.sample_rate, ceiling_db=self._level[1])
        if self._pause is not None:
            from .pause import seg_of
            seg_of(self.sample_rate)               # refuses a delivered rate outside 8 .. 48 kHz, by name
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._ps = eng.pause(batch_size, rate=self.sample_rate)
        # the device stages between a chunk and the ring, in the order they run; a further stage takes its place in this list
        self._stages = [st for st in (self._ld, self._tp, self._fm, self._pt, self._rs, self._lv, self._ps) if st is not None]
        self.stop_signal = stop_signal
        self.timeout = timeout
        self.audio_queues = [self._make_queue() for _ in range(batch_size)]
        self.finished_flags = [False for _ in range(batch_size)]
        self._pcm_engine = pcm16                  # vibevoice_amd.Engine (or None: chunks keep the producer's dtype)
        self._ring = [None] * ring_slots          # pinned host buffers, allocated on first use (shape of the first chunk)
        self._pcm_dev = [None] * ring_slots       # device staging per ring slot: what the last stage, or the 16-bit conversion, writes
        self._ring_cnt = [None] * ring_slots      # pinned int32 per ring slot: the rows' counts where the last stage counts on the device
        self._copy_stream = None                  # D2H copies run here: the module's copy stream of the chunks' device
        self._free = Queue()
        for i in range(ring_slots):
            self._free.put(i)
        self._work = Queue()
        self._ended = 0                            # samples whose end marker has been queued
        self._lock = threading.Lock()
        self._closed = False
        self._thread = threading.Thread(target=self._drain, daemon=True)
        self._thread.start()

    def _make_queue(self):
        return Queue()

    def _deliver(self, idx, item):
        self.audio_queues[idx].put(item, timeout=self.timeout)

    # ---- producer side (generation loop) ----
    def put(self, audio_chunks: torch.Tensor, sample_indices: torch.Tensor):
        idxs = [int(i) for i in sample_indices.tolist()]
        live = [(row, idx) for row, idx in enumerate(idxs) if idx < self.batch_size and not self.finished_flags[idx]]
        if not live or self._closed:
            return
        if not audio_chunks.is_cuda:
            for row, idx in live:
                chunk = audio_chunks[row].detach().clone()
                if self.sample_rate != SOURCE_RATE or self._speeds is not None or self._level is not None or self._pitch is not None \
                        or self._pause is not None:
                    chunk = self._host_chunk(idx, chunk)
                    if chunk is None:
                        continue
                self._work.put(("chunk", idx, chunk, None, None))
            return
        if self._loud is not None and self._ld is None:
            raise ValueError("AudioStreamer(loudness_lufs=...): device chunks are levelled on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self.sample_rate != SOURCE_RATE and self._rs is None:
            raise ValueError(f"AudioStreamer(sample_rate={self.sample_rate}): device chunks are resampled on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self._formant is not None and self._fm is None:
            raise ValueError("AudioStreamer(formant=...): device chunks are warped on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self._pitch is not None and self._pt is None:
            raise ValueError("AudioStreamer(pitch=...): device chunks are shifted on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self._speeds is not None and self._tp is None:
            raise ValueError("AudioStreamer(speed=...): device chunks are stretched on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self._level is not None and self._lv is None:
            raise ValueError("AudioStreamer(volume_db=... / ceiling_db=...): device chunks are levelled on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self._pause is not None and self._ps is None:
            raise ValueError("AudioStreamer(max_pause_ms=... / max_lead_ms=...): device chunks are shortened on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        self._put_device(audio_chunks, live)

    def _host_chunk(self, idx, chunk):
        """a CPU chunk of sample idx (None: its flush) at the streamer's speed, rate and level, None where it completes no output sample"""
        flush = chunk is None
        y = None
        if not flush:
            self._lead = tuple(chunk.shape[:-1])
            y = chunk.reshape(-1)
        if self._loud is not None:
            from .loudness import HostLoudness
            ld = self._ld_host.get(idx)
            if ld is None and not flush:
                ld = self._ld_host[idx] = HostLoudness(self._loud[0][idx], self._loud[1][idx], self._loud[2][idx])
            if ld is not None:
                if flush:
                    ld.flush()                                # emits nothing: it closes the stream
                else:
                    y = ld.push(y)
        if self._speeds is not None:
            from .tempo import HostTempo
            t = self._tp_host.get(idx)
            if t is None and not flush:
                t = self._tp_host[idx] = HostTempo(self._speeds[idx])
            if t is not None:
                y = t.flush() if flush else t.push(y)
        if self._formant is not None:
            from .formant import HostFormant
            fm = self._fm_host.get(idx)
            if fm is None:
                if y is None:
                    return None
                fm = self._fm_host[idx] = HostFormant(*self._formant[idx])
            y = fm.push(y if y is not None else torch.zeros(0), flush=flush)
        if self._pitch is not None:
            from .pitch import HostPitch
            p = self._pt_host.get(idx)
            if p is None:
                if y is None:
                    return None
                p = self._pt_host[idx] = HostPitch(self._pitch[idx])
            y = p.push(y if y is not None else torch.zeros(0), flush=flush)
        if self.sample_rate != SOURCE_RATE:
            from .resample import HostResampler
            h = self._rs_host.get(idx)
            if h is None:
                if y is None:
                    return None
                h = self._rs_host[idx] = HostResampler(SOURCE_RATE, self.sample_rate)
            y = h.push(y if y is not None else torch.zeros(0), flush=flush)
        if self._level is not None:
            from .level import HostLevel
            lv = self._lv_host.get(idx)
            if lv is None:
                if y is None:
                    return None
                lv = self._lv_host[idx] = HostLevel(self._level[0][idx], self._level[1], self.sample_rate)
            y = lv.push(y if y is not None else torch.zeros(0), flush=flush)
        if self._pause is not None:
            from .pause import HostPause
            ps = self._ps_host.get(idx)
            if ps is None:
                if y is None:
                    return None
                ps = self._ps_host[idx] = HostPause(self.sample_rate, self._pause[0][idx], self._pause[1][idx], self._pause[2][idx])
            y = ps.push(y if y is not None else torch.zeros(0), flush=flush)
        if y is None or not y.shape[0]:
            return None
        return y.reshape(self._lead + (y.shape[0],))

    def _put_device(self, audio_chunks, live, flush=False):
        """The live rows of a device chunk batch (audio_chunks None: their flush) through the stage chain on the producing stream, then
        the ring.  Every stage but the last writes an fp32 temporary there; the last one writes the slot's staging, as int16 under pcm16
        (the launch converts, over each row's own chunk), with each row's count in the work item (a last stage that counts on the device,
        the pauses: a word of the slot's pinned companion, filled by the copy stream in front of the slot's event); one ring slot and one work item per
        last-stage launch that delivers.  A chunk longer than a stage's push takes (stage.take()) goes in pieces and arrives as several.
        No stages: the chunk batch itself is the source of the ring copy, behind Engine.audio_to_pcm16 into the staging under pcm16."""
        pcm = self._pcm_engine
        if audio_chunks is not None:
            src = audio_chunks.detach()
            self._lead = tuple(src.shape[1:-1])
            self._prod = torch.cuda.current_stream(src.device)
        prod = self._prod
        if not self._stages:
            n, rows = src.shape[0], [(row, idx, None) for row, idx in live]
            if pcm is None:
                self._with_slot(lambda slot: self._ring_copy(src, rows, slot, prod))
                return
            # int16 on device, on the producing stream, before the copy (demo/gradio_demo.py:1058-1073 per chunk)
            flat = src.reshape(n, -1).to(torch.float32).contiguous()

            def convert(slot):
                pd = self._staging(slot, n, flat.shape[1], torch.int16, src.device, exact=True)
                pcm.audio_to_pcm16(flat, pd[:n], stream=prod)
                self._ring_copy(pd[:n].view((n,) + tuple(src.shape[1:])), rows, slot, prod)
            self._with_slot(convert)
            return
        flat = None
        if audio_chunks is not None:
            flat = src.reshape(src.shape[0], -1).to(torch.float32)
            if [row for row, _ in live] != list(range(len(live))):
                flat = flat[[row for row, _ in live]]
            flat = flat.contiguous()
        if prod is None:                                   # a flush with no put before it
            prod = torch.cuda.current_stream(self._stages[0].engine.device)
        n = len(live)
        self._through(0, flat, [0 if flat is None else flat.shape[1]] * n, [idx for _, idx in live], flush, prod)

    def _through(self, k, x, counts, ids, flush, prod):
        """rows x (fp32 [n, >= max(counts)], None where no row has samples), counts[i] samples for stream ids[i], through stage k and
        the stages behind it; flush: these are the streams' last samples.  False once the streamer is closed"""
        stage, n, ends = self._stages[k], len(ids), k == len(self._stages) - 1
        dev = stage.engine.device
        kw = {"speeds": [self._speeds[idx] for idx in ids]} if stage is self._tp else {}
        tk = {}
        if stage is self._pt:
            kw = tk = {"semitones": [self._pitch[idx] for idx in ids]}
        if stage is self._fm:
            kw = {"fractions": [self._formant[idx] for idx in ids]}
        if stage is self._lv:
            kw = {"volumes_db": [self._level[0][idx] for idx in ids]}
        if stage is self._ld:
            kw = {"targets_lufs": [self._loud[0][idx] for idx in ids], "start_db": [self._loud[1][idx] for idx in ids],
                  "max_boost_db": [self._loud[2][idx] for idx in ids]}
        if stage is self._ps:
            kw = {"max_pause_ms": [self._pause[0][idx] for idx in ids], "max_lead_ms": [self._pause[1][idx] for idx in ids],
                  "threshold_db": [self._pause[2][idx] for idx in ids]}
        dt = torch.int16 if ends and self._pcm_engine is not None else torch.float32
        at = 0
        while True:                                        # one push, but for a chunk longer than it takes
            rem = [max(c - at, 0) for c in counts]
            w = stage.take(ids, rem, flush, **tk)
            final = w >= max(rem)

            def push(out):
                with torch.cuda.stream(prod):
                    return stage.push(x if at == 0 or x is None else x[:, at:].contiguous(), ids, flush=flush and final, out=out,
                                      pcm16=dt == torch.int16, n_in=[min(r, w) for r in rem], stream=prod, **kw)[1]
            if ends:
                def deliver(slot):
                    pd = self._staging(slot, n, stage.max_out(w), dt, dev)
                    cnts = push(pd)
                    if torch.is_tensor(cnts):              # the stage counts on the device: the counts travel with the copy
                        self._ring_copy(pd[:n], [(i, idx, None) for i, idx in enumerate(ids)], slot, prod, counts_dev=cnts)
                    else:
                        self._ring_copy(pd[:n], [(i, idx, cnts[i]) for i, idx in enumerate(ids)], slot, prod)
                if not self._with_slot(deliver):
                    return False
            else:
                with torch.cuda.stream(prod):
                    td = torch.empty((n, stage.max_out(w)), dtype=dt, device=dev)      # this stream's: the next stage reads it there
                ct = push(td)
                # no sample completed: nothing for the next stage, nothing to deliver
                if (any(ct) or (flush and final)) and not self._through(k + 1, td, ct, ids, flush and final, prod):
                    return False
            if final:
                return True
            at += w

    def _ring_copy(self, src, rows, slot, prod, counts_dev=None):
        """the device rows src to the slot's pinned buffer behind the producing stream; rows: (row of src, sample index, samples of the row
        that count or None: the row as it is) for the drain thread.  counts_dev (int32, one per row of src, on the device): the counts
        are the device's; they go to the slot's pinned companion on the copy stream in front of the same event, and the drain thread
        reads them there once it has waited for it.  Nothing here waits for the device."""
        cbuf = None
        if counts_dev is not None:
            cbuf = self._ring_cnt[slot]
            if cbuf is None or cbuf.shape[0] < counts_dev.shape[0]:
                if cbuf is not None:
                    _pinned_give([cbuf])
                cbuf = self._ring_cnt[slot] = _pinned_take((max(counts_dev.shape[0], self.batch_size),), torch.int32)
            rows = [(row, idx, cbuf[row]) for row, idx, _ in rows]      # a view of the pinned word: read behind the event
        buf = self._ring[slot]
        if buf is None or buf.shape[1:] != src.shape[1:] or buf.shape[0] < src.shape[0] or buf.dtype != src.dtype:
            if buf is not None:
                _pinned_give([buf])
            buf = _pinned_take((max(src.shape[0], self.batch_size),) + tuple(src.shape[1:]), src.dtype)
            self._ring[slot] = buf
        # The D2H copy runs on the streamer's OWN stream, ordered behind the producer by an event: the drain thread then waits on an
        # event of a stream that never enters hipGraph capture.  (Waiting on an event of the producing stream raced with the
        # engine's stream captures -- hipEventSynchronize refuses an event whose stream is capturing, hipErrorCapturedEvent --
        # whenever a new graph key was captured while a chunk was still in flight.)
        if self._copy_stream is None:
            self._copy_stream = _copy_stream_for(src.device)
        ready = torch.cuda.Event()
        ready.record(prod)
        self._copy_stream.wait_event(ready)
        with torch.cuda.stream(self._copy_stream):
            buf[:src.shape[0]].copy_(src, non_blocking=True)       # staged rows are whole rows: both sides contiguous, one asynchronous copy
            if counts_dev is not None:
                cbuf[:counts_dev.shape[0]].copy_(counts_dev, non_blocking=True)
        src.record_stream(self._copy_stream)
        if counts_dev is not None:
            counts_dev.record_stream(self._copy_stream)
        ev = torch.cuda.Event()
        ev.record(self._copy_stream)
        self._work.put(("slot", rows, slot, ev, self._lead))

    def _with_slot(self, fn):
        """fn(slot) with a free ring slot (back-pressure only if the consumer is > ring_slots behind), under the lock the drain thread
        hands the ring back under; False once the streamer is closed"""
        slot = self._free.get()
        with self._lock:
            if self._closed:
                self._free.put(slot)
                return False
            fn(slot)
            return True

    def _staging(self, slot, n, cap, dt, dev, exact=False):
        """the slot's device staging with at least n rows of at least (exact: exactly) cap columns"""
        pd = self._pcm_dev[slot]
        if pd is None or pd.shape[0] < n or pd.dtype != dt or (pd.shape[1] != cap if exact else pd.shape[1] < cap):
            pd = torch.empty((max(n, self.batch_size), cap), dtype=dt, device=dev)
            self._pcm_dev[slot] = pd
        return pd

    def end(self, sample_indices=None):
        if sample_indices is None:
            idxs = list(range(self.batch_size))
        else:
            idxs = [int(i.item()) if torch.is_tensor(i) else int(i) for i in sample_indices]
        idxs = [idx for idx in dict.fromkeys(idxs) if idx < self.batch_size and not self.finished_flags[idx]]
        if (self.sample_rate != SOURCE_RATE or self._speeds is not None or self._level is not None or self._pitch is not None
                or self._pause is not None) and idxs and not self._closed:
            self._flush_tails(idxs)
        for idx in idxs:
            self.finished_flags[idx] = True
            self._work.put(("end", idx, None, None, None))       # ordered after that sample's pending chunks

    def _flush_tails(self, idxs):
        """the samples the stages still hold for these sample indices, as last chunks, in front of their stop signals"""
        for idx in idxs:
            tail = self._host_chunk(idx, None)
            if tail is not None:
                self._work.put(("chunk", idx, tail, None, None))
        if self._stages:                         # the first stage's tail runs through the ones behind it, whose own follow in the same pass
            live = list(enumerate(i for i in idxs if self._stages[0].total[i] > 0))
            if live:
                self._put_device(None, live, flush=True)

    def close(self):
        """Stop the drain thread and release the pinned ring (also happens by itself once every sample has ended)."""
        with self._lock:                     # under the lock put() queues its copies: every one of them precedes the marker below
            was_open = not self._closed
            self._closed = True
        if was_open:
            # a consumer blocked in get_stream() / __iter__ with timeout=None must wake up: every sample that has not ended
            # gets its stop signal (ordered after its pending chunks) before the thread stops
            for idx in range(self.batch_size):
                if not self.finished_flags[idx]:
                    self.finished_flags[idx] = True
                    self._work.put(("end", idx, None, None, None))
            self._work.put((_CLOSE, None, None, None, None))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- background thread: event -> per-sample queues, in production order ----
    def _drain(self):
        while True:
            kind, a, b, ev, n = self._work.get()
            if kind is _CLOSE:
                break
            if kind == "slot":                           # a: (ring row, sample index, samples or None: the whole row), n: the lead shape
                ev.synchronize()
                buf = self._ring[b]
                for row, idx, cnt in a:
                    if torch.is_tensor(cnt):             # a word of the slot's pinned companion: the copy behind ev has filled it
                        cnt = min(int(cnt), buf.shape[1])
                    if cnt is None:
                        self._deliver(idx, buf[row].clone())
                    elif cnt:
                        self._deliver(idx, buf[row, :cnt].clone().reshape(n + (cnt,)))
                self._free.put(b)
            elif kind == "chunk":
                self._deliver(a, b)
            elif kind == "end":
                self._deliver(a, self.stop_signal)
                self._ended += 1
                if self._ended >= self.batch_size:       # nothing can arrive any more (put() drops chunks of ended samples)
                    break
        with self._lock:                                 # no put() is between its closed check and its copy
            self._closed = True
        # a put() that raced with an end() / close() from another thread may have queued its copy behind the marker that ended the
        # loop: wait for those copies too before the buffers change hands
        import queue as _q
        while True:
            try:
                item = self._work.get_nowait()
            except _q.Empty:
                break
            if item[0] == "slot":
                item[3].synchronize()
                self._free.put(item[2])                  # a producer still blocked in _free.get() wakes up, sees _closed, returns
        with self._lock:
            _pinned_give(self._ring)                     # every copy into them has completed (their events have been waited on)
            _pinned_give(self._ring_cnt)
            self._ring = [None] * len(self._ring)
            self._ring_cnt = [None] * len(self._ring_cnt)
            self._pcm_dev = [None] * len(self._pcm_dev)  # release the device staging
            if self._rs is not None:
                self._rs.close()                         # the engine's resampler configuration is free for the next streamer
            if self._tp is not None:
                self._tp.close()                         # ... and its tempo configuration
            if self._pt is not None:
                self._pt.close()                         # ... and its pitch configuration
            if self._fm is not None:
                self._fm.close()                         # ... and its formant configuration
            if self._lv is not None:
                self._lv.close()                         # ... and its level configuration
            if self._ld is not None:
                self._ld.close()                         # ... and its loudness configuration
            if self._ps is not None:
                self._ps.close()                         # ... and its pause configuration

    # ---- consumer side ----
    def __iter__(self):
        return AudioBatchIterator(self)

    def get_stream(self, sample_idx: int):
        if sample_idx >= self.batch_size:
            raise ValueError(f"Sample index {sample_idx} exceeds batch size {self.batch_size}")
        return AudioSampleIterator(self, sample_idx)


class AudioSampleIterator:
    def __init__(self, streamer: AudioStreamer, sample_idx: int):
        self.streamer = streamer
        self.sample_idx = sample_idx

    def __iter__(self):
        return self

    def __next__(self):
        value = self.streamer.audio_queues[self.sample_idx].get(timeout=self.streamer.timeout)
        if value is self.streamer.stop_signal or (not torch.is_tensor(value) and value == self.streamer.stop_signal):
            raise StopIteration()
        return value


class AudioBatchIterator:
    """Yields {sample index: chunk} for every sample that has a chunk ready, until all samples have ended."""

    def __init__(self, streamer: AudioStreamer):
        self.streamer = streamer
        self.active = set(range(streamer.batch_size))

    def __iter__(self):
        return self

    def __next__(self):
        import queue as _q
        import time
        while self.active:
            out = {}
            for idx in sorted(self.active):
                try:
                    v = self.streamer.audio_queues[idx].get(block=False)
                except _q.Empty:
                    continue
                if v is self.streamer.stop_signal or (not torch.is_tensor(v) and v == self.streamer.stop_signal):
                    self.active.discard(idx)
                else:
                    out[idx] = v
            if out:
                return out
            if self.active:
                time.sleep(0.001)
        raise StopIteration()


class AsyncAudioStreamer(AudioStreamer):
    """Async variant (vibevoice/modular/streamer.py:150-264): per-sample asyncio queues owned by the event loop that was
    running at construction; the drain thread hands chunks over with loop.call_soon_threadsafe, so generate() -- running in
    a worker thread, as in the reference's gradio path -- never touches the loop and never syncs the stream.
        async for chunk in streamer.get_stream(0): ...      async for batch in streamer: ..."""

    def __init__(self, batch_size: int, stop_signal=None, timeout: Optional[float] = None, ring_slots: int = 8, pcm16=None,
                 sample_rate: Optional[int] = None, engine=None, speed=None, volume_db=None, ceiling_db=None, loudness_lufs=None,
                 loudness_start_db=None, max_boost_db=None, pitch=None, formant=None, max_pause_ms=None, max_lead_ms=None,
                 pause_threshold_db=None):
        self.loop = asyncio.get_running_loop()
        super().__init__(batch_size, stop_signal, timeout, ring_slots=ring_slots, pcm16=pcm16, sample_rate=sample_rate, engine=engine,
                         speed=speed, volume_db=volume_db, ceiling_db=ceiling_db, loudness_lufs=loudness_lufs,
                         loudness_start_db=loudness_start_db, max_boost_db=max_boost_db, pitch=pitch, formant=formant,
                         max_pause_ms=max_pause_ms, max_lead_ms=max_lead_ms, pause_threshold_db=pause_threshold_db)

    def _make_queue(self):
        return asyncio.Queue()

    def _deliver(self, idx, item):
        self.loop.call_soon_threadsafe(self.audio_queues[idx].put_nowait, item)

    def _is_stop(self, value):
        return value is self.stop_signal or (not torch.is_tensor(value) and value == self.stop_signal)

    async def get_stream(self, sample_idx: int):
        if sample_idx >= self.batch_size:
            raise ValueError(f"Sample index {sample_idx} exceeds batch size {self.batch_size}")
        while True:
            value = await self.audio_queues[sample_idx].get()
            if self._is_stop(value):
                break
            yield value

    def __iter__(self):
        raise TypeError("AsyncAudioStreamer is consumed with `async for`")

    def __aiter__(self):
        return AsyncAudioBatchIterator(self)


class AsyncAudioBatchIterator:
    """{sample index: chunk} for the samples whose next chunk is ready first; ends when every sample has ended."""

    def __init__(self, streamer: AsyncAudioStreamer):
        self.streamer = streamer
        self.active = set(range(streamer.batch_size))
        self._pending = {}                      # idx -> task waiting on that sample's queue (kept across calls: no chunk is lost)

    def __aiter__(self):
        return self

    async def __anext__(self):
        while self.active:
            for idx in self.active:
                if idx not in self._pending:
                    self._pending[idx] = asyncio.ensure_future(self.streamer.audio_queues[idx].get())
            done, _ = await asyncio.wait(self._pending.values(), return_when=asyncio.FIRST_COMPLETED, timeout=self.streamer.timeout)
            if not done:
                raise asyncio.TimeoutError()
            out = {}
            for idx in sorted(self.active):
                t = self._pending.get(idx)
                if t is not None and t in done:
                    del self._pending[idx]
                    v = t.result()
                    if self.streamer._is_stop(v):
                        self.active.discard(idx)
                    else:
                        out[idx] = v
            if out:
                return out
        raise StopAsyncIteration()
