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
producing stream, at 24 kHz, IN FRONT of whatever follows it today -- the resampler, else the 16-bit conversion (over each row's
stretched chunk), else the copy; float chunks arrive as fp32.  Chunk-continuous like the resampler: per sample, the concatenated
chunks equal Engine.time_stretch() of the concatenated input (then Engine.resample() of that, under sample_rate), ceil(n / S) samples,
bit for bit in float mode.  A sample holds back at most 640 input samples (26.7 ms) until its next chunk; a put that completes no
block of 240 delivers nothing for that row; end(indices) flushes the tempo tail, then the resampler's.  Device chunks need an engine
(as above), CPU chunks go through tempo.HostTempo.  A chunk too long for one launch is pushed in pieces and arrives as several.

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


class AudioStreamer:
    def __init__(self, batch_size: int, stop_signal=None, timeout: Optional[float] = None, ring_slots: int = 8, pcm16=None,
                 sample_rate: Optional[int] = None, engine=None, speed=None):
        self.batch_size = batch_size
        self._speeds = _speeds_of(speed, batch_size)   # one per sample index, or None: no tempo stage anywhere
        self._tp = None                            # Engine.tempo (device chunks), one stream per sample index
        self._tp_host = {}                         # sample index -> tempo.HostTempo (CPU chunks)
        self.sample_rate = SOURCE_RATE if sample_rate is None else int(sample_rate)
        self._rs = None                            # Engine.resampler (device chunks), one stream per sample index
        self._rs_host = {}                         # sample index -> resample.HostResampler (CPU chunks)
        self._rs_stream = None                     # the producing stream of the last resampled put: the tails are flushed on it
        self._lead = ()                            # a chunk's dimensions between the row and the samples, kept for the tail
        if self.sample_rate != SOURCE_RATE:
            eng = engine if engine is not None else pcm16
            if eng is not None:                    # without one, only CPU chunks are served (resample.HostResampler); put() refuses others
                self._rs = eng.resampler(SOURCE_RATE, self.sample_rate, batch_size)
        if self._speeds is not None:
            eng = engine if engine is not None else pcm16
            if eng is not None:
                self._tp = eng.tempo(batch_size)
        self.stop_signal = stop_signal
        self.timeout = timeout
        self.audio_queues = [self._make_queue() for _ in range(batch_size)]
        self.finished_flags = [False for _ in range(batch_size)]
        self._pcm_engine = pcm16                  # vibevoice_amd.Engine (or None: chunks keep the producer's dtype)
        self._ring = [None] * ring_slots          # pinned host buffers, allocated on first use (shape of the first chunk)
        self._pcm_dev = [None] * ring_slots       # device int16 staging per ring slot (pcm16 mode)
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
                if self.sample_rate != SOURCE_RATE or self._speeds is not None:
                    chunk = self._host_chunk(idx, chunk)
                    if chunk is None:
                        continue
                self._work.put(("chunk", idx, chunk, None, None))
            return
        if self.sample_rate != SOURCE_RATE and self._rs is None:
            raise ValueError(f"AudioStreamer(sample_rate={self.sample_rate}): device chunks are resampled on the device and need an engine "
                             "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
        if self._speeds is not None:
            if self._tp is None:
                raise ValueError("AudioStreamer(speed=...): device chunks are stretched on the device and need an engine "
                                 "(pcm16=engine for 16-bit chunks, engine=engine for float chunks)")
            self._put_tempo(audio_chunks, live)
            return
        slot = self._free.get()                                    # back-pressure only if the consumer is > ring_slots behind
        with self._lock:                                           # the drain thread hands the ring back to the pool under this lock
            if self._closed:
                self._free.put(slot)
                return
            if self._rs is not None:
                self._put_resampled(audio_chunks, live, slot)
            else:
                self._put_slot(audio_chunks, live, slot)

    def _host_chunk(self, idx, chunk):
        """a CPU chunk of sample idx (None: its flush) at the streamer's speed and rate, None where it completes no output sample"""
        flush = chunk is None
        y = None
        if not flush:
            self._lead = tuple(chunk.shape[:-1])
            y = chunk.reshape(-1)
        if self._speeds is not None:
            from .tempo import HostTempo
            t = self._tp_host.get(idx)
            if t is None and not flush:
                t = self._tp_host[idx] = HostTempo(self._speeds[idx])
            if t is not None:
                y = t.flush() if flush else t.push(y)
        if self.sample_rate != SOURCE_RATE:
            from .resample import HostResampler
            h = self._rs_host.get(idx)
            if h is None:
                if y is None:
                    return None
                h = self._rs_host[idx] = HostResampler(SOURCE_RATE, self.sample_rate)
            y = h.push(y if y is not None else torch.zeros(0), flush=flush)
        if y is None or not y.shape[0]:
            return None
        return y.reshape(self._lead + (y.shape[0],))

    def _put_resampled(self, audio_chunks, live, slot, flush=False):
        """One Resampler.push for the live rows (audio_chunks None: their flush), then the ring copy of _put_slot; the work item carries
        each row's sample count."""
        rs, pcm = self._rs, self._pcm_engine is not None
        dev = rs.engine.device
        ids = [idx for _, idx in live]
        n = len(live)
        if audio_chunks is not None:
            src = audio_chunks.detach()
            self._lead = tuple(src.shape[1:-1])
            flat = src.reshape(src.shape[0], -1).to(torch.float32)
            if [row for row, _ in live] != list(range(n)):
                flat = flat[[row for row, _ in live]]
            flat = flat.contiguous()
            samples = flat.shape[1]
            self._rs_stream = torch.cuda.current_stream(dev)
        else:
            flat, samples = None, 0
        prod = self._rs_stream if self._rs_stream is not None else torch.cuda.current_stream(dev)
        cap, dt = rs.max_out(samples), torch.int16 if pcm else torch.float32
        pd = self._staging(slot, n, cap, dt, dev)
        with torch.cuda.stream(prod):
            _, cnts = rs.push(flat, ids, flush=flush, out=pd, pcm16=pcm, n_in=None if flat is not None else [0] * n, stream=prod)
        self._ring_copy(pd, ids, cnts, slot, prod)

    def _ring_copy(self, pd, ids, cnts, slot, prod):
        """rows [0, len(ids)) of the device staging pd, cnts[i] samples each, to the slot's pinned buffer behind the producing stream"""
        n, dt, dev = len(ids), pd.dtype, pd.device
        buf = self._ring[slot]
        if buf is None or buf.dim() != 2 or buf.shape[1] != pd.shape[1] or buf.shape[0] < n or buf.dtype != dt:
            if buf is not None:
                _pinned_give([buf])
            buf = _pinned_take((max(n, self.batch_size), pd.shape[1]), dt)
            self._ring[slot] = buf
        if self._copy_stream is None:
            self._copy_stream = _copy_stream_for(dev)
        ready = torch.cuda.Event()
        ready.record(prod)
        self._copy_stream.wait_event(ready)
        with torch.cuda.stream(self._copy_stream):
            buf[:n].copy_(pd[:n], non_blocking=True)              # whole rows: both sides contiguous, one asynchronous copy
        pd.record_stream(self._copy_stream)
        ev = torch.cuda.Event()
        ev.record(self._copy_stream)
        self._work.put(("rslot", [(i, idx, cnts[i]) for i, idx in enumerate(ids)], slot, ev, self._lead))

    def _with_slot(self, fn):
        """fn(slot) with a free ring slot, under the lock the drain thread hands the ring back under; False once the streamer is closed"""
        slot = self._free.get()
        with self._lock:
            if self._closed:
                self._free.put(slot)
                return False
            fn(slot)
            return True

    def _staging(self, slot, n, cap, dt, dev):
        pd = self._pcm_dev[slot]
        if pd is None or pd.shape[0] < n or pd.shape[1] < cap or pd.dtype != dt:
            pd = torch.empty((max(n, self.batch_size), cap), dtype=dt, device=dev)
            self._pcm_dev[slot] = pd
        return pd

    def _rs_width(self, ids, rem, flush):
        """how many of the rows' remaining stretched samples (rem[i] for stream ids[i]) the next Resampler.push takes: all of them where
        that fits the kernel -- at most 8192 outputs per row, the chunk within its LDS beside the filter table (vv_resample_rows
        refuses more) -- else a width that fits whatever the streams' state"""
        rs = self._rs
        lds_max = (65536 - 64) // 4 - rs.L * (rs.T + 1) - rs.T - rs.T // 2
        if max(rem) <= lds_max and all(rs.counts(i, r, flush) <= 8192 for i, r in zip(ids, rem)):
            return max(rem)
        return max(1, min(8191 * rs.M // rs.L - rs.T // 2 - 1, lds_max))

    def _put_tempo(self, audio_chunks, live, flush=False):
        """Tempo.push for the live rows (audio_chunks None: their flush), then what follows today on the stretched rows with their
        per-row counts: the resampler push, else nothing more (the tempo launch converts to 16 bits itself); one ring slot and one work
        item per launch that delivers.  A chunk longer than one launch takes goes in pieces."""
        tp, rs, pcm = self._tp, self._rs, self._pcm_engine is not None
        dev = tp.engine.device
        ids = [idx for _, idx in live]
        n = len(live)
        speeds = [self._speeds[idx] for idx in ids]
        if audio_chunks is not None:
            src = audio_chunks.detach()
            self._lead = tuple(src.shape[1:-1])
            flat = src.reshape(src.shape[0], -1).to(torch.float32)
            if [row for row, _ in live] != list(range(n)):
                flat = flat[[row for row, _ in live]]
            flat = flat.contiguous()
            samples = flat.shape[1]
            self._rs_stream = torch.cuda.current_stream(dev)
        else:
            flat, samples = None, 0
        prod = self._rs_stream if self._rs_stream is not None else torch.cuda.current_stream(dev)
        dt = torch.int16 if pcm else torch.float32
        for c0 in range(0, max(samples, 1), tp.max_in):
            w = min(tp.max_in, samples - c0)
            piece = flat[:, c0:c0 + w].contiguous() if flat is not None else None      # the whole chunk but for one longer than a launch takes
            last = c0 + w >= samples
            tcap = tp.max_out(w)
            if rs is None:
                def stage(slot):
                    pd = self._staging(slot, n, tcap, dt, dev)
                    with torch.cuda.stream(prod):
                        _, cnts = tp.push(piece, ids, speeds, flush=flush and last, out=pd, n_in=[w] * n, stream=prod, pcm16=pcm)
                    self._ring_copy(pd, ids, cnts, slot, prod)
                if not self._with_slot(stage):
                    return
                continue
            with torch.cuda.stream(prod):
                td = torch.empty((n, tcap), dtype=torch.float32, device=dev)       # this stream's: the resampler push below reads it there
                _, ct = tp.push(piece, ids, speeds, flush=flush and last, out=td, n_in=[w] * n, stream=prod)
            if not any(ct) and not (flush and last):
                continue                                 # no block completed: nothing for the resampler, nothing to deliver
            at = 0
            while True:                                # one resampler push, but for a stretched chunk longer than it takes
                rem = [max(c - at, 0) for c in ct]
                wr = self._rs_width(ids, rem, flush and last)
                final = wr >= max(rem)
                nin = [min(r, wr) for r in rem]

                def stage(slot):
                    pd = self._staging(slot, n, rs.max_out(wr), dt, dev)
                    with torch.cuda.stream(prod):
                        _, cnts = rs.push(td if at == 0 else td[:, at:].contiguous(), ids, flush=flush and last and final, out=pd, pcm16=pcm,
                                          n_in=nin, stream=prod)
                    self._ring_copy(pd, ids, cnts, slot, prod)
                if not self._with_slot(stage):
                    return
                if final:
                    break
                at += wr

    def _put_slot(self, audio_chunks, live, slot):
        src = audio_chunks.detach()
        if self._pcm_engine is not None:
            # int16 on device, on the producing stream, before the copy (demo/gradio_demo.py:1058-1073 per chunk)
            n = src.shape[0]
            flat = src.reshape(n, -1).to(torch.float32).contiguous()
            pd = self._pcm_dev[slot]
            if pd is None or pd.shape[0] < n or pd.shape[1] != flat.shape[1]:
                pd = torch.empty((max(n, self.batch_size), flat.shape[1]), dtype=torch.int16, device=src.device)
                self._pcm_dev[slot] = pd
            self._pcm_engine.audio_to_pcm16(flat, pd[:n], stream=torch.cuda.current_stream(src.device))
            src = pd[:n].view((n,) + tuple(audio_chunks.shape[1:]))
        need = src.shape
        buf = self._ring[slot]
        if buf is None or buf.shape[1:] != need[1:] or buf.shape[0] < need[0] or buf.dtype != src.dtype:
            if buf is not None:
                _pinned_give([buf])
            buf = _pinned_take((max(need[0], self.batch_size),) + tuple(need[1:]), src.dtype)
            self._ring[slot] = buf
        # The D2H copy runs on the streamer's OWN stream, ordered behind the producer by an event: the drain thread then waits on an
        # event of a stream that never enters hipGraph capture.  (Waiting on an event of the producing stream raced with the
        # engine's stream captures -- hipEventSynchronize refuses an event whose stream is capturing, hipErrorCapturedEvent --
        # whenever a new graph key was captured while a chunk was still in flight.)
        prod = torch.cuda.current_stream(audio_chunks.device)
        if self._copy_stream is None:
            self._copy_stream = _copy_stream_for(audio_chunks.device)
        ready = torch.cuda.Event()
        ready.record(prod)
        self._copy_stream.wait_event(ready)
        with torch.cuda.stream(self._copy_stream):
            buf[:need[0]].copy_(src, non_blocking=True)
        src.record_stream(self._copy_stream)
        ev = torch.cuda.Event()
        ev.record(self._copy_stream)
        self._work.put(("slot", live, slot, ev, need[0]))

    def end(self, sample_indices=None):
        if sample_indices is None:
            idxs = list(range(self.batch_size))
        else:
            idxs = [int(i.item()) if torch.is_tensor(i) else int(i) for i in sample_indices]
        idxs = [idx for idx in dict.fromkeys(idxs) if idx < self.batch_size and not self.finished_flags[idx]]
        if (self.sample_rate != SOURCE_RATE or self._speeds is not None) and idxs and not self._closed:
            self._flush_tails(idxs)
        for idx in idxs:
            self.finished_flags[idx] = True
            self._work.put(("end", idx, None, None, None))       # ordered after that sample's pending chunks

    def _flush_tails(self, idxs):
        """the samples the resampler still holds for these sample indices, as a last chunk each, in front of their stop signals"""
        for idx in idxs:
            tail = self._host_chunk(idx, None)
            if tail is not None:
                self._work.put(("chunk", idx, tail, None, None))
        if self._tp is not None:                 # the tempo tail first, then (in the same pass) the resampler's
            live = [(row, idx) for row, idx in enumerate(i for i in idxs if self._tp.total[i] > 0)]
            if live:
                self._put_tempo(None, live, flush=True)
            return
        live = [(row, idx) for row, idx in enumerate(i for i in idxs if self._rs is not None and self._rs.total[i] > 0)]
        for i0 in range(0, len(live), 16):
            slot = self._free.get()
            with self._lock:
                if self._closed:
                    self._free.put(slot)
                    return
                self._put_resampled(None, [(r - i0, idx) for r, idx in live[i0:i0 + 16]], slot, flush=True)

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
            if kind == "slot":
                ev.synchronize()
                buf = self._ring[b]
                for row, idx in a:
                    self._deliver(idx, buf[row].clone())
                self._free.put(b)
            elif kind == "rslot":
                ev.synchronize()
                buf = self._ring[b]
                for row, idx, cnt in a:
                    if cnt:
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
            if item[0] in ("slot", "rslot"):
                item[3].synchronize()
                self._free.put(item[2])                  # a producer still blocked in _free.get() wakes up, sees _closed, returns
        with self._lock:
            _pinned_give(self._ring)                     # every copy into them has completed (their events have been waited on)
            self._ring = [None] * len(self._ring)
            self._pcm_dev = [None] * len(self._pcm_dev)  # release the device staging
            if self._rs is not None:
                self._rs.close()                         # the engine's resampler configuration is free for the next streamer
            if self._tp is not None:
                self._tp.close()                         # ... and its tempo configuration

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
                 sample_rate: Optional[int] = None, engine=None, speed=None):
        self.loop = asyncio.get_running_loop()
        super().__init__(batch_size, stop_signal, timeout, ring_slots=ring_slots, pcm16=pcm16, sample_rate=sample_rate, engine=engine,
                         speed=speed)

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
