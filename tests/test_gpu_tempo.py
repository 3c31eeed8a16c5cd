"""GPU tests of the tempo stage (csrc/tempo.hip: vv_tempo_rows, vv_tempo_once) against vibevoice_amd/tempo.py: samples AND chosen
offsets bit for bit -- the search is exact integer arithmetic and the overlap-add two rounded products and a rounded sum, so there is
no tolerance anywhere in this file.  Also its chunk invariance and state handling, its refusals, and AudioStreamer(speed=...) on device
chunks in front of the resampler and the 16-bit conversion.  One engine serves the whole file: the small one of test_gpu_noise_rows.py."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import build_small
from vibevoice_amd import tempo as T
from vibevoice_amd.engine import EngineError, TempoCapacityError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

SPEEDS = [0.5, 0.8, 1.13, 1.25, 2.0]
LENGTHS = [1, 239, 241, 3200, 7001]
CUTS = [0, 1, 7, 639, 641, 3200]
GUARD, SENTINEL = 64, -77.25
N_STREAMS = 7
IDS5 = [5, 0, 3, 6, 2]                       # non-identity stream ids


@pytest.fixture(scope="module")
def small():
    lm = synth.LMCfg(hidden=256, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
    s = build_small(lm, xsplit=3, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    yield s
    s.eng.close()


@pytest.fixture()
def make(small):
    made = []

    def _make(n_streams=N_STREAMS):
        made.append(small.eng.tempo(n_streams))
        return made[-1]
    yield _make
    for t in made:
        t.close()


def _voice(seed, n, amp=0.3):
    """seeded noise plus harmonics, peak near amp"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    h = sum(np.sin(2 * np.pi * f * t / 24000.0 + rng.uniform(0, 6.28)) / (j + 1) for j, f in enumerate((110.0, 220.0, 330.0, 455.0)))
    return (amp * (0.35 * h + 0.3 * rng.uniform(-1, 1, n))).astype(np.float32)


def _square(n, shift=0):
    """a clipped square wave of period 80: the search signal is +-32767 exactly, every offset that keeps the phase ties at ssd 0"""
    return (4.0 * np.where(((np.arange(n) + shift) % 80) < 40, 1.0, -1.0)).astype(np.float32)


def _signal(kind, row, n):
    if kind == "voice":
        return _voice(10 + row, n)
    if kind == "loud":
        return 4.0 * _voice(20 + row, n)             # most of it beyond +-1: the clamp of the search signal
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    return _square(n, 13 * row)


_REF = {}


def _ref(kind, row, n, speed):
    """stretch_ref of a test signal, computed once: (samples, offsets)"""
    key = (kind, row, n, speed)
    if key not in _REF:
        _REF[key] = T.stretch_ref(_signal(kind, row, n), speed, return_offsets=True)
    return _REF[key]


@pytest.mark.parametrize("kind", ["voice", "loud", "zeros", "square"])
def test_time_stretch_is_the_definition(small, kind):
    """Engine.time_stretch over 1 and 3 rows of 1 .. 7001 samples (one block, a cut last block, several tiles' worth of blocks) at five
    speeds: ceil(n Q / P) samples, samples and offsets equal to stretch_ref's"""
    eng = small.eng
    jobs = []
    with torch.cuda.stream(eng.stream):
        for n in LENGTHS:
            for rows in (1, 3):
                x = torch.from_numpy(np.stack([_signal(kind, r, n) for r in range(rows)]))
                xd = (x[0] if rows == 1 else x).to(eng.device)
                for s in SPEEDS:
                    jobs.append((n, rows, s, xd, eng.time_stretch(xd, s, return_offsets=True)))
    eng.sync()
    for n, rows, s, xd, (y, offs) in jobs:
        P, Q = T.ratio(s)
        assert y.dtype == torch.float32 and y.shape[-1] == -(-n * Q // P) and y.dim() == xd.dim()
        y, offs = y.cpu().reshape(rows, -1), offs.cpu().reshape(rows, -1)
        for r in range(rows):
            want, want_offs = _ref(kind, r, n, s)
            assert np.array_equal(offs[r].numpy(), want_offs), (kind, n, rows, s, r)
            assert torch.equal(y[r], torch.from_numpy(want)), (kind, n, rows, s, r)
    if kind == "square":
        assert any((_ref(kind, 0, 7001, s)[1] == -40).any() for s in SPEEDS)      # the symmetric tie occurred


def _push(eng, tp, chunks, ids, speeds, flush=False, pcm16=False, cap=None):
    """One push of the rows `chunks` (1-D numpy arrays, lengths may differ: n_in per row) into guarded buffers: a sentinel row above
    and below the output rows and sentinel columns behind every row's count.  Checks the guards and that the counts are what
    tempo.counts says -> (per-row outputs, per-row offsets)."""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[i, :c.shape[0]] = torch.from_numpy(c)
    fl = [flush] * n if isinstance(flush, bool) else list(flush)
    want = [T.counts(*T.ratio(speeds[i]), tp.total[ids[i]], int(chunks[i].shape[0]), fl[i])[1] for i in range(n)]
    cap = max(want) + GUARD if cap is None else cap
    dt, sent = (torch.int16, int(SENTINEL)) if pcm16 else (torch.float32, SENTINEL)
    out = torch.full((n + 2, cap), sent, dtype=dt, device=eng.device)
    xd = xin.to(eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        _, cnts, offs = tp.push(xd, ids, speeds, flush=fl, out=out[1:n + 1], n_in=[int(c.shape[0]) for c in chunks], pcm16=pcm16,
                                return_offsets=True)
    eng.sync()
    host, offs = out.cpu(), offs.cpu()
    assert cnts == want, (cnts, want)
    assert bool((host[0] == sent).all()) and bool((host[n + 1] == sent).all()), "guard rows were written"
    for i in range(n):
        assert bool((host[1 + i, cnts[i]:] == sent).all()), f"row {i}: written beyond its {cnts[i]} samples"
    return [host[1 + i, :cnts[i]].clone() for i in range(n)], [offs[i, :-(-cnts[i] // 240)].clone() for i in range(n)]


def test_five_streams_five_speeds_one_launch(small, make):
    """5 streams at five speeds in one launch per step; row i of step k brings chunk (k + i) % 6 of the ragged cuts, so the rows stand at
    different totals and some pushes emit nothing; the rows travel in reversed order on alternate steps.  After step 7 two streams are
    reset and start a new signal.  The last step flushes.  Every stream's concatenation (since its reset) is stretch_ref of its
    concatenated input, offsets included, and equals the one-shot kernel's result."""
    eng, tp = small.eng, make()
    steps, reset_at, reset_rows = 14, 8, (1, 3)
    feed = [[CUTS[(k + i) % 6] for k in range(steps)] for i in range(5)]
    sig = [_voice(30 + i, sum(feed[i])) for i in range(5)]
    at, got, goff, fed = [0] * 5, [[] for _ in range(5)], [[] for _ in range(5)], [[] for _ in range(5)]
    saw_zero = False
    for k in range(steps):
        if k == reset_at:
            with torch.cuda.stream(eng.stream):
                tp.reset([IDS5[i] for i in reset_rows])
            for i in reset_rows:
                got[i], goff[i], fed[i] = [], [], []
                assert tp.total[IDS5[i]] == 0
        order = list(range(5)) if k % 2 == 0 else list(range(4, -1, -1))
        chunks = [sig[i][at[i]:at[i] + feed[i][k]] for i in order]
        outs, offs = _push(eng, tp, chunks, [IDS5[i] for i in order], [SPEEDS[i] for i in order], flush=k == steps - 1)
        for j, i in enumerate(order):
            saw_zero |= outs[j].shape[0] == 0 and feed[i][k] > 0
            got[i].append(outs[j]); goff[i].append(offs[j]); fed[i].append(chunks[j])
            at[i] += feed[i][k]
    assert saw_zero
    for i in range(5):
        x = np.concatenate(fed[i])
        assert x.shape[0] == (sum(feed[i][reset_at:]) if i in reset_rows else sum(feed[i]))
        want, want_offs = T.stretch_ref(x, SPEEDS[i], return_offsets=True)
        assert np.array_equal(torch.cat(goff[i]).numpy(), want_offs), i
        assert torch.equal(torch.cat(got[i]), torch.from_numpy(want)), i
        with torch.cuda.stream(eng.stream):
            once = eng.time_stretch(torch.from_numpy(x), SPEEDS[i])
        eng.sync()
        assert torch.equal(once.cpu(), torch.from_numpy(want))


def test_sixty_small_pushes(small, make):
    """60 pushes of 97 samples: the history rolls over many times.  A push brings less than a block's 120 (speed 0.5) or 271 (1.13)
    input samples, so it emits one block at most, and before the flush at most (5820 - 640) / 120 + 1 = 44 blocks leave: at least 15
    of the 59 pushes emit nothing at either speed"""
    eng, tp = small.eng, make(2)
    x = _voice(40, 60 * 97)
    for speed, sid in ((1.13, 1), (0.5, 0)):
        got = []
        for k in range(60):
            outs, _ = _push(eng, tp, [x[k * 97:(k + 1) * 97]], [sid], [speed], flush=k == 59)
            got.append(outs[0])
        assert sum(o.shape[0] == 0 for o in got) >= 15 and all(o.shape[0] in (0, 240) for o in got[:59])
        assert torch.equal(torch.cat(got), torch.from_numpy(T.stretch_ref(x, speed)))


def test_sixteen_rows_and_seventeen_ids(small, make):
    """16 rows in one launch; 17 ids through push (two launches): every row the one-shot result of its own signal at its own speed"""
    eng, tp = small.eng, make(17)
    for n in (16, 17):
        tp.reset()
        x = np.stack([_voice(50 + i, 1500) for i in range(n)])
        ids = [(7 * i + 3) % n for i in range(n)]
        speeds = [SPEEDS[i % 5] for i in range(n)]
        a, _ = _push(eng, tp, list(x[:, :900]), ids, speeds)
        b, _ = _push(eng, tp, list(x[:, 900:]), ids, speeds, flush=True)
        for i in range(n):
            assert torch.equal(torch.cat([a[i], b[i]]), torch.from_numpy(T.stretch_ref(x[i], speeds[i]))), (n, i)


def _pcm16_rule(rows):
    """the numpy rule of test_pcm16_reference_arithmetic (test_dropin_cpu.py), per chunk"""
    out = []
    for r in rows:
        data = r.numpy()
        peak = np.float32(np.abs(data).max()) if data.size else np.float32(0)
        mine = data / peak if peak > 1.0 else data
        out.append(torch.from_numpy(np.trunc(mine * np.float32(32767.0)).astype(np.int16)))
    return out


def test_int16_mode_is_the_pcm16_rule_on_the_float_rows(small, make):
    """two tempo configurations in the same state; one push as float, one as int16 (the same single launch): the int16 rows equal the
    numpy rule applied to the float rows -- a row whose stretched peak exceeds 1 (normalised), one below, one of 5 samples"""
    eng = small.eng
    a, b = make(3), make(3)
    rows = [4.0 * _voice(60, 3200), _voice(61, 3200), _voice(62, 5)]
    speeds = [0.8, 1.25, 2.0]
    f, _ = _push(eng, a, rows, [2, 0, 1], speeds)
    q, _ = _push(eng, b, rows, [2, 0, 1], speeds, pcm16=True)
    assert float(f[0].abs().max()) > 1.0 and 0.0 < float(f[1].abs().max()) < 1.0 and f[2].shape[0] == 0
    for got, want in zip(q, _pcm16_rule(f)):
        assert got.dtype == torch.int16 and torch.equal(got, want)
    f, _ = _push(eng, a, [np.zeros(0, dtype=np.float32)] * 3, [2, 0, 1], speeds, flush=True)
    q, _ = _push(eng, b, [np.zeros(0, dtype=np.float32)] * 3, [2, 0, 1], speeds, flush=True, pcm16=True)
    assert f[2].shape[0] == 3
    for got, want in zip(q, _pcm16_rule(f)):
        assert torch.equal(got, want)


def test_refusals_change_nothing(small, make):
    """a row beyond the launch's capacity (input, or output rows too short) raises TempoCapacityError; the other refusals EngineError
    with their message; the sentinel-filled outputs stay untouched and the streams where they were: stream 1 goes on like its twin"""
    eng = small.eng
    tp, twin = make(4), make(4)
    first = _voice(70, 1000)
    _push(eng, tp, [first], [1], [0.8])
    _push(eng, twin, [first], [1], [0.8])
    _push(eng, tp, [first], [3], [1.25], flush=True)
    assert tp.max_in == 7680
    big = torch.zeros((2, 7681), dtype=torch.float32, device=eng.device)
    x = torch.from_numpy(np.stack([_voice(71, 3200), _voice(72, 3200)])).to(eng.device)
    out = torch.full((4, 8000), SENTINEL, dtype=torch.float32, device=eng.device)
    small_out = torch.full((4, 700), SENTINEL, dtype=torch.float32, device=eng.device)
    cases = [
        (TempoCapacityError, dict(audio=big, stream_ids=[0, 1], speeds=0.8), "at most 7680 per row"),
        (TempoCapacityError, dict(audio=x, stream_ids=[0, 1], speeds=0.8, out=small_out), "the output rows hold 700"),
        (EngineError, dict(audio=x, stream_ids=[0, 4], speeds=0.8), "stream id 4 out of range"),
        (EngineError, dict(audio=x, stream_ids=[1, 1], speeds=0.8), "stream 1 is named twice"),
        (EngineError, dict(audio=x, stream_ids=[0, 1], speeds=0.8, n_in=[400, -1]), "n_in = -1 must be >= 0"),
        (EngineError, dict(audio=x, stream_ids=[0, 1], speeds=[0.8, 1.25]), "stream 1 runs at speed 4 / 5"),
        (EngineError, dict(audio=x, stream_ids=[0, 3], speeds=[0.8, 1.25]), "stream 3 has been flushed"),
    ]
    for err, kw, msg in cases:
        o = kw.pop("out", out)
        with torch.cuda.stream(eng.stream):
            with pytest.raises(err, match=msg):
                tp.push(kw.pop("audio"), kw.pop("stream_ids"), kw.pop("speeds"), out=o, **kw)
        eng.sync()
        assert bool((o == SENTINEL).all()), msg
    assert issubclass(TempoCapacityError, EngineError)
    with pytest.raises(ValueError, match="2.5"):
        tp.push(x, [0, 1], [0.8, 2.5], out=out)
    with pytest.raises(ValueError, match="2.5"):
        eng.time_stretch(x, 2.5)
    with pytest.raises(ValueError, match="samples"):
        eng.time_stretch(x[None], 0.8)
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_tempo_reset(eng._ctx, eng._s, 9, 1, None), "vv_tempo_reset")
    assert tp.total == [0, 1000, 0, 1000] and tp.ratio[0] is None
    nxt = _voice(73, 2000)
    a, oa = _push(eng, tp, [nxt], [1], [0.8], flush=True)
    b, ob = _push(eng, twin, [nxt], [1], [0.8], flush=True)
    assert a[0].shape[0] > 0 and torch.equal(a[0], b[0]) and torch.equal(oa[0], ob[0])
    with torch.cuda.stream(eng.stream):
        tp.reset([3])
    a, _ = _push(eng, tp, [nxt], [3], [2.0], flush=True)                   # after its reset a stream takes another speed
    assert torch.equal(a[0], torch.from_numpy(T.stretch_ref(nxt, 2.0)))


def _collect(st, idx):
    return list(st.get_stream(idx))


def test_streamer_speed_then_48k_int16_end_to_end(small):
    """AudioStreamer(2, pcm16=eng, sample_rate=48000, speed=[0.8, 1.25]) over 6 device chunks of 3200 and end(): per sample the float
    streamer's chunks concatenate to Engine.resample(Engine.time_stretch(whole)) bit for bit, ceil(ceil(n Q / P) * 2) samples, and the
    int16 streamer's chunks are the pcm16 rule applied chunk by chunk to the float ones"""
    eng = small.eng
    speeds = [0.8, 1.25]
    n = 6 * 3200
    x = torch.from_numpy(np.stack([3.0 * _voice(80, n), _voice(81, n)])[:, None, :]).to(eng.device)
    sts = [AudioStreamer(2, pcm16=eng, sample_rate=48000, speed=speeds, timeout=20),
           AudioStreamer(2, engine=eng, sample_rate=48000, speed=speeds, timeout=20)]
    with torch.cuda.stream(eng.stream):
        for st in sts:
            for k in range(6):
                st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
            st.end()
        want = [eng.resample(eng.time_stretch(x[i, 0], speeds[i]), 24000, 48000) for i in range(2)]
    eng.sync()
    for idx in range(2):
        P, Q = T.ratio(speeds[idx])
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert len(q) == len(f) == 7 and all(c.dtype == torch.int16 for c in q) and all(c.dtype == torch.float32 for c in f)
        assert [c.shape for c in q] == [c.shape for c in f] and all(c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        cat = torch.cat(f, dim=-1)[0]
        assert cat.shape[0] == 2 * -(-n * Q // P) and torch.equal(cat, want[idx].cpu())
        assert torch.equal(want[idx].cpu(), eng.resample(torch.from_numpy(T.stretch_ref(x[idx, 0].cpu().numpy(), speeds[idx])), 24000, 48000).cpu())
        for got, rule in zip(q, _pcm16_rule([c[0] for c in f])):
            assert torch.equal(got[0], rule)
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._rs_used == [None] * 4 and eng._tp_used == [None] * 4         # finished streamers gave their configurations back


def test_streamer_speed_alone_float_and_int16(small):
    """no sample_rate: the tempo launch feeds the ring itself, as fp32 or, under pcm16, as int16 over each row's stretched chunk; a sample
    that ends early, a put that completes no block, a chunk longer than one launch takes (pushed in pieces)"""
    eng = small.eng
    speeds = [1.13, 0.5]
    x = torch.from_numpy(np.stack([3.0 * _voice(82, 12000), _voice(83, 12000)])[:, None, :]).to(eng.device)
    sts = [AudioStreamer(2, pcm16=eng, speed=speeds, timeout=20), AudioStreamer(2, engine=eng, speed=speeds, timeout=20)]
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :300], torch.tensor([0, 1]))                   # below 640 samples: nothing is delivered
            st.put(x[:, :, 300:3200], torch.tensor([0, 1]))
            st.end(torch.tensor([1]))
            st.put(x[:1, :, 3200:], torch.tensor([0]))                    # 8800 samples: two launches, two chunks
            st.end()
    eng.sync()
    for idx, n in ((0, 12000), (1, 3200)):
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert len(q) == len(f) == (4 if idx == 0 else 2)
        assert [c.shape for c in q] == [c.shape for c in f] and all(c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        assert torch.equal(torch.cat(f, dim=-1)[0], torch.from_numpy(T.stretch_ref(x[idx, 0, :n].cpu().numpy(), speeds[idx])))
        for got, rule in zip(q, _pcm16_rule([c[0] for c in f])):
            assert got.dtype == torch.int16 and torch.equal(got[0], rule)
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._tp_used == [None] * 4


def test_streamer_put_that_completes_no_block_in_front_of_the_resampler(small):
    """speed and sample_rate: a first put below 640 samples completes no block, reaches no resampler push and delivers nothing; the
    sample's chunks still concatenate to Engine.resample(Engine.time_stretch(whole))"""
    eng = small.eng
    x = torch.from_numpy(_voice(87, 3200)[None, None, :]).to(eng.device)
    st = AudioStreamer(1, engine=eng, sample_rate=16000, speed=0.8, timeout=20)
    with torch.cuda.stream(eng.stream):
        st.put(x[:, :, :300], torch.tensor([0]))
        assert st._rs.total == [0] and st._tp.total == [300]
        st.put(x[:, :, 300:], torch.tensor([0]))
        st.end()
        want = eng.resample(eng.time_stretch(x[0, 0], 0.8), 24000, 16000)
    eng.sync()
    chunks = _collect(st, 0)
    assert len(chunks) == 2 and torch.equal(torch.cat(chunks, dim=-1)[0], want.cpu()) and want.shape[0] == -(-4000 * 2 // 3)
    st._thread.join(timeout=20)


def test_streamer_stretched_chunk_longer_than_one_resampler_push(small):
    """speed 0.5 in front of 48 kHz: a put of 3200 samples stretches row 0 to about 6400 and those to about 12800 at 48 kHz, beyond the
    8192 outputs of one resampler push, so the stretched chunk goes to the resampler in pieces and arrives as several.  Per sample the
    float chunks concatenate to Engine.resample(Engine.time_stretch(whole)) bit for bit and the int16 chunks are the pcm16 rule of the
    float ones chunk by chunk; both streamers give their configurations back"""
    eng = small.eng
    speeds = [0.5, 1.25]
    x = torch.from_numpy(np.stack([3.0 * _voice(90, 6400), _voice(91, 6400)])[:, None, :]).to(eng.device)
    sts = [AudioStreamer(2, pcm16=eng, sample_rate=48000, speed=speeds, timeout=20),
           AudioStreamer(2, engine=eng, sample_rate=48000, speed=speeds, timeout=20)]
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :3200], torch.tensor([0, 1]))
            st.put(x[:, :, 3200:], torch.tensor([0, 1]))
            st.end()
        want = [eng.resample(eng.time_stretch(x[i, 0], speeds[i]), 24000, 48000) for i in range(2)]
    eng.sync()
    for idx in range(2):
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        print(f"[stretched chunk beyond one resampler push] sample {idx}: {len(q)} int16 chunks, {len(f)} float chunks of {[c.shape[-1] for c in f]}")
        assert all(c.dtype == torch.int16 for c in q) and all(c.dtype == torch.float32 for c in f)
        assert [c.shape for c in q] == [c.shape for c in f] and all(c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        assert max(c.shape[-1] for c in f) <= 8192
        assert torch.equal(torch.cat(f, dim=-1)[0], want[idx].cpu())
        for got, rule in zip(q, _pcm16_rule([c[0] for c in f])):
            assert torch.equal(got[0], rule)
        assert len(q) == len(f) == (5, 3)[idx]
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._rs_used == [None] * 4 and eng._tp_used == [None] * 4


@pytest.mark.parametrize("mode", ["16k", "speed", "speed_16k"])
def test_streamer_live_rows_that_are_no_prefix(small, mode):
    """a batch of 3 whose sample 1 ends after the first put while the second put still passes all three rows: the live rows 0 and 2 are
    gathered out of the chunk batch.  Samples 0 and 2 equal the definitions over their 2400 samples, sample 1 over its 1200"""
    eng = small.eng
    rate, speed = (16000 if "16k" in mode else None), (0.8 if "speed" in mode else None)
    x = torch.from_numpy(np.stack([_voice(92 + i, 2400) for i in range(3)])[:, None, :]).to(eng.device)
    st = AudioStreamer(3, engine=eng, sample_rate=rate, speed=speed, timeout=20)
    with torch.cuda.stream(eng.stream):
        st.put(x[:, :, :1200], torch.tensor([0, 1, 2]))
        st.end([1])
        st.put(x[:, :, 1200:], torch.tensor([0, 1, 2]))
        st.end()
        want = []
        for idx, n in ((0, 2400), (1, 1200), (2, 2400)):
            y = x[idx, 0, :n]
            y = eng.time_stretch(y, speed) if speed is not None else y
            want.append(eng.resample(y, 24000, rate) if rate is not None else y)
    eng.sync()
    counts = []
    for idx in range(3):
        f = _collect(st, idx)
        counts.append(len(f))
        assert all(c.dtype == torch.float32 and c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        assert torch.equal(torch.cat(f, dim=-1)[0], want[idx].cpu()), (mode, idx)
    print(f"[live rows 0 and 2 of 3, {mode}] chunks per sample: {counts}")
    assert counts == {"16k": [3, 2, 3], "speed": [3, 2, 3], "speed_16k": [3, 2, 3]}[mode]
    st._thread.join(timeout=20)
    assert eng.__dict__.get("_rs_used", [None] * 4) == [None] * 4 and eng.__dict__.get("_tp_used", [None] * 4) == [None] * 4


@pytest.mark.parametrize("mode", ["plain", "pcm16", "48k"])
def test_streamer_without_a_speed_is_unchanged(small, mode):
    """a streamer built without `speed`, and one built with speed 1, deliver what a second streamer without the keyword delivers on the
    same input, byte for byte, and take no tempo configuration"""
    eng = small.eng
    kw = {"plain": {}, "pcm16": dict(pcm16=eng), "48k": dict(pcm16=eng, sample_rate=48000)}[mode]
    x = torch.from_numpy(np.stack([3.0 * _voice(84, 6400), _voice(85, 6400)])[:, None, :]).to(eng.device).to(torch.bfloat16)
    sts = [AudioStreamer(2, timeout=20, **kw), AudioStreamer(2, timeout=20, **kw), AudioStreamer(2, timeout=20, speed=1.0, **kw)]
    assert all(st._tp is None and st._speeds is None for st in sts) and eng.__dict__.get("_tp_used", [None] * 4) == [None] * 4
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :3200], torch.tensor([0, 1]))
            st.put(x[:, :, 3200:], torch.tensor([0, 1]))
            st.end()
    eng.sync()
    for idx in range(2):
        a, b, c = (_collect(st, idx) for st in sts)
        assert len(a) == len(b) == len(c) == (3 if mode == "48k" else 2)
        for u, v, w in zip(a, b, c):
            assert u.dtype == v.dtype == w.dtype and torch.equal(u, v) and torch.equal(u, w)
    for st in sts:
        st._thread.join(timeout=20)


def test_model_time_stretch(small):
    from vibevoice_amd.modeling import _AudioRates

    class Model(_AudioRates):
        engine = small.eng
    x = _voice(86, 3000)
    with torch.cuda.stream(small.eng.stream):
        y = Model().time_stretch(torch.from_numpy(x), 1.25)
    small.eng.sync()
    assert torch.equal(y.cpu(), torch.from_numpy(T.stretch_ref(x, 1.25)))
