"""GPU tests of the level stage (csrc/level.hip: vv_level_rows, vv_level_once) against vibevoice_amd/level.py.  The definition's middle
is integer arithmetic (minima and sums, free of order) between single fp32 roundings, so there is no tolerance anywhere in this file:
fp32 outputs are compared with level_ref bit for bit (as 32-bit patterns: a negative zero counts), int16 outputs with
trunc(level_ref * 32767).  Also the stage's chunk invariance and state handling, its refusals, and AudioStreamer(volume_db=...,
ceiling_db=...) on device chunks behind the tempo change and the resampler.  Where the resampler stands in front, the level stage is held
to level_ref of what Engine.resample delivers: the resampler itself meets its definition within a derived bound (test_gpu_resample.py),
not bit for bit, and this file's subject is the stage behind it.  One engine serves the whole file: the small one of test_gpu_tempo.py."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import build_small
from vibevoice_amd import level as V
from vibevoice_amd import tempo as T
from vibevoice_amd.engine import EngineError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

RATES = [24000, 8000]                        # A = 120, H = 1200 and A = 40, H = 400
CEIL_DB = -1.0
GUARD, SENTINEL = 64, -77.25
N_STREAMS = 7
IDS5 = [5, 0, 3, 6, 2]                       # non-identity stream ids
VOLS5 = [0.0, 6.0, -9.5, 12.0, 3.0]
KINDS = ["quiet", "loud", "click_first", "click_a", "click_last", "zeros", "nonfinite"]


@pytest.fixture(scope="module")
def small():
    lm = synth.LMCfg(hidden=256, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
    s = build_small(lm, xsplit=3, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    yield s
    s.eng.close()


@pytest.fixture()
def make(small):
    made = []

    def _make(n_streams=N_STREAMS, rate=24000, ceiling_db=CEIL_DB):
        made.append(small.eng.level(n_streams, rate=rate, ceiling_db=ceiling_db))
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


def _lengths(rate):
    A, H = V.params(rate)
    return [1, A - 1, A, A + 1, H + 2 * A, 3200, 7001, 16001]      # 16001: three tiles of the one-shot kernel at either rate


def _signal(kind, row, n, rate):
    A, _ = V.params(rate)
    if kind == "quiet":
        return _voice(10 + row, n, amp=0.3)                        # never limited at 0 dB
    if kind == "loud":
        return _voice(20 + row, n, amp=3.0)                        # most of it beyond c
    x = np.zeros(n, dtype=np.float32)
    if kind.startswith("click"):
        at = {"click_first": 0, "click_a": A - 1, "click_last": n - 1}[kind]
        x[min(at, n - 1)] = 1.0 if row % 2 == 0 else -1.0          # full scale, above c = -1 dB
    elif kind == "nonfinite":
        x = _voice(30 + row, n, amp=1.5)
        x[n // 3] = np.nan
        x[(2 * n) // 3] = np.inf if row % 2 == 0 else -np.inf
    return x


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same(got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    return got.dtype == want.dtype == torch.float32 and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _pcm(y):
    """trunc(y * 32767) of float32 samples within +-1: what the 16-bit rule gives where its rescale does not fire"""
    y = np.asarray(y, dtype=np.float32)
    assert y.size == 0 or np.abs(y).max() <= 1.0
    return torch.from_numpy(np.trunc(y * np.float32(32767.0)).astype(np.int16))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_apply_level_is_the_definition(small, kind, rate):
    """Engine.apply_level over 1 and 3 rows of 1 .. 16001 samples at two volumes: as many samples, equal to level_ref's"""
    eng = small.eng
    jobs = []
    with torch.cuda.stream(eng.stream):
        for n in _lengths(rate):
            for rows in (1, 3):
                x = np.stack([_signal(kind, r, n, rate) for r in range(rows)])
                xd = torch.from_numpy(x[0] if rows == 1 else x).to(eng.device)
                for db in (0.0, 7.5):
                    jobs.append((n, rows, db, x, xd, eng.apply_level(xd, db, CEIL_DB, rate)))
    eng.sync()
    c = float(V.ceiling_of(CEIL_DB))
    for n, rows, db, x, xd, y in jobs:
        assert y.dtype == torch.float32 and y.shape == xd.shape
        y = y.cpu().reshape(rows, -1)
        for r in range(rows):
            want = V.level_ref(x[r], db, CEIL_DB, rate)
            assert _same(y[r], torch.from_numpy(want)), (kind, rate, n, rows, db, r)
            assert float(y[r].abs().max()) <= c
            if kind == "quiet" and db == 0.0:
                assert _same(y[r], torch.from_numpy(x[r]))            # passthrough: the input itself
    if kind == "loud":
        assert float(np.abs(V.level_ref(_signal(kind, 0, 7001, rate), 0.0, CEIL_DB, rate, return_gain=True)[1]).min()) < 0.5


def _push(eng, lv, chunks, ids, vols, flush=False, pcm16=False, cap=None):
    """One push of the rows `chunks` (1-D numpy arrays, lengths may differ: n_in per row) into guarded buffers: a sentinel row above
    and below the output rows and sentinel columns behind every row's count.  Checks the guards and that the counts are what
    level.counts says -> per-row outputs."""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[i, :c.shape[0]] = torch.from_numpy(c)
    fl = [flush] * n if isinstance(flush, bool) else list(flush)
    want = [V.counts(lv.A, lv.total[ids[i]], int(chunks[i].shape[0]), fl[i])[1] for i in range(n)]
    assert want == [lv.counts(ids[i], int(chunks[i].shape[0]), fl[i]) for i in range(n)]
    cap = max(want) + GUARD if cap is None else cap
    dt, sent = (torch.int16, int(SENTINEL)) if pcm16 else (torch.float32, SENTINEL)
    out = torch.full((n + 2, cap), sent, dtype=dt, device=eng.device)
    xd = xin.to(eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        _, cnts = lv.push(xd, ids, vols, flush=fl, out=out[1:n + 1], n_in=[int(c.shape[0]) for c in chunks], pcm16=pcm16)
    eng.sync()
    host = out.cpu()
    assert cnts == want, (cnts, want)
    assert bool((host[0] == sent).all()) and bool((host[n + 1] == sent).all()), "guard rows were written"
    for i in range(n):
        assert bool((host[1 + i, cnts[i]:] == sent).all()), f"row {i}: written beyond its {cnts[i]} samples"
    return [host[1 + i, :cnts[i]].clone() for i in range(n)]


@pytest.mark.parametrize("rate", RATES)
def test_five_streams_five_volumes_one_launch(small, make, rate):
    """5 streams at five volumes in one launch per step, as fp32 in one configuration and as int16 in a twin; row i of step k brings chunk
    (k + i) % 6 of the ragged cuts {0, 1, A - 1, A, 641, 3200}, so the rows stand at different totals and some pushes emit nothing; the
    rows travel in reversed order on alternate steps.  After step 7 two streams are reset and start a new signal while the others go
    on.  The last step flushes.  Every stream's concatenation (since its reset) is level_ref of its concatenated input, the int16 twin
    trunc(level_ref * 32767), and the one-shot kernel gives the same."""
    eng = small.eng
    lv, twin = make(rate=rate), make(rate=rate)
    A, H = V.params(rate)
    assert (lv.A, lv.H, lv.delay_samples, lv.max_in) == (A, H, A - 1, 8128 - (H + 3 * A - 3))
    cuts = [0, 1, A - 1, A, 641, 3200]
    steps, reset_at, reset_rows = 14, 8, (1, 3)
    feed = [[cuts[(k + i) % 6] for k in range(steps)] for i in range(5)]
    sig = [_voice(30 + i, sum(feed[i]), amp=(0.2, 1.5, 3.0, 0.4, 1.0)[i]) for i in range(5)]
    at, got, gq, fed = [0] * 5, [[] for _ in range(5)], [[] for _ in range(5)], [[] for _ in range(5)]
    saw_zero = False
    for k in range(steps):
        if k == reset_at:
            with torch.cuda.stream(eng.stream):
                lv.reset([IDS5[i] for i in reset_rows])
                twin.reset([IDS5[i] for i in reset_rows])
            for i in reset_rows:
                got[i], gq[i], fed[i] = [], [], []
                assert lv.total[IDS5[i]] == 0
        order = list(range(5)) if k % 2 == 0 else list(range(4, -1, -1))
        chunks = [sig[i][at[i]:at[i] + feed[i][k]] for i in order]
        ids, vols = [IDS5[i] for i in order], [VOLS5[i] for i in order]
        outs = _push(eng, lv, chunks, ids, vols, flush=k == steps - 1)
        outq = _push(eng, twin, chunks, ids, vols, flush=k == steps - 1, pcm16=True)
        for j, i in enumerate(order):
            saw_zero |= outs[j].shape[0] == 0 and feed[i][k] > 0
            got[i].append(outs[j]); gq[i].append(outq[j]); fed[i].append(chunks[j])
            at[i] += feed[i][k]
    assert saw_zero
    limited = 0
    for i in range(5):
        x = np.concatenate(fed[i])
        assert x.shape[0] == (sum(feed[i][reset_at:]) if i in reset_rows else sum(feed[i]))
        want, a = V.level_ref(x, VOLS5[i], CEIL_DB, rate, return_gain=True)
        limited += bool(a.min() < 1.0)
        assert _same(torch.cat(got[i]), torch.from_numpy(want)), (rate, i)
        assert torch.equal(torch.cat(gq[i]), _pcm(want)), (rate, i)
        with torch.cuda.stream(eng.stream):
            once = eng.apply_level(torch.from_numpy(x), VOLS5[i], CEIL_DB, rate)
        eng.sync()
        assert _same(once.cpu(), torch.from_numpy(want))
    assert 2 <= limited <= 4                                          # limited streams and untouched ones side by side


def test_sixty_small_pushes(small, make):
    """60 pushes of 97 samples (below A) of a loud signal: the history rolls over many times"""
    eng, lv = small.eng, make(2)
    x = _voice(40, 60 * 97, amp=2.5)
    got = [_push(eng, lv, [x[k * 97:(k + 1) * 97]], [1], [4.0], flush=k == 59)[0] for k in range(60)]
    assert got[0].shape[0] == 0 and got[1].shape[0] == 2 * 97 - 119 and got[59].shape[0] == 97 + 119
    assert _same(torch.cat(got), torch.from_numpy(V.level_ref(x, 4.0)))


def test_sixteen_rows_and_seventeen_ids(small, make):
    """16 rows in one launch; 17 ids through push (two launches): every row level_ref of its own signal at its own volume"""
    eng, lv = small.eng, make(17)
    for n in (16, 17):
        with torch.cuda.stream(eng.stream):
            lv.reset()
        x = np.stack([_voice(50 + i, 1500, amp=0.3 + 0.2 * i) for i in range(n)])
        ids = [(7 * i + 3) % n for i in range(n)]
        vols = [VOLS5[i % 5] for i in range(n)]
        a = _push(eng, lv, list(x[:, :900]), ids, vols)
        b = _push(eng, lv, list(x[:, 900:]), ids, vols, flush=True)
        for i in range(n):
            assert _same(torch.cat([a[i], b[i]]), torch.from_numpy(V.level_ref(x[i], vols[i]))), (n, i)


@pytest.mark.parametrize("rate", RATES)
def test_a_chunk_longer_than_one_push_goes_in_pieces_of_take(small, make, rate):
    """a chunk of max_in + 1000 samples: refused whole, by name; in pieces of take() the definition; a push of exactly max_in fills the
    staging buffer to its last word"""
    eng, lv = small.eng, make(2, rate=rate)
    n = lv.max_in + 1000
    x = _voice(55, n, amp=2.0)
    xd = torch.from_numpy(x[None]).to(eng.device)
    with pytest.raises(EngineError, match=f"at most {lv.max_in} per row"):
        lv.push(xd, [0], 0.0)
    assert lv.total == [0, 0]
    got, at = [], 0
    while at < n:
        w = lv.take([0], [n - at])
        assert w == min(lv.max_in, n - at)
        got.append(_push(eng, lv, [x[at:at + w]], [0], [0.0], flush=at + w == n)[0])
        at += w
    assert len(got) == 2 and _same(torch.cat(got), torch.from_numpy(V.level_ref(x, 0.0, CEIL_DB, rate)))


def test_refusals_change_nothing(small, make):
    """every refusal is an EngineError with its message; the sentinel-filled outputs stay untouched and the streams where they were:
    stream 1 goes on like its twin"""
    eng = small.eng
    lv, twin = make(4), make(4)
    first = _voice(70, 1000, amp=1.5)
    _push(eng, lv, [first], [1], [3.0])
    _push(eng, twin, [first], [1], [3.0])
    _push(eng, lv, [first], [3], [0.0], flush=True)
    x = torch.from_numpy(np.stack([_voice(71, 3200), _voice(72, 3200)])).to(eng.device)
    out = torch.full((4, 4000), SENTINEL, dtype=torch.float32, device=eng.device)
    small_out = torch.full((4, 700), SENTINEL, dtype=torch.float32, device=eng.device)
    cases = [
        (dict(audio=x, stream_ids=[0, 1], volumes_db=3.0, out=small_out), "the output rows hold 700"),
        (dict(audio=x, stream_ids=[0, 4], volumes_db=3.0), "stream id 4 out of range"),
        (dict(audio=x, stream_ids=[0, -1], volumes_db=3.0), "stream id -1 out of range"),
        (dict(audio=x, stream_ids=[1, 1], volumes_db=3.0), "stream 1 is named twice"),
        (dict(audio=x, stream_ids=[0, 1], volumes_db=3.0, n_in=[400, -1]), "n_in = -1 must be >= 0"),
        (dict(audio=x, stream_ids=[0, 1], volumes_db=[3.0, 6.0]), "stream 1 runs at gain"),
        (dict(audio=x, stream_ids=[0, 3], volumes_db=[3.0, 0.0]), "stream 3 has been flushed"),
        (dict(audio=x, stream_ids=[], volumes_db=3.0), r"n = 0 must be in \[1,16\]"),
    ]
    for kw, msg in cases:
        o = kw.pop("out", out)
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                lv.push(kw.pop("audio"), kw.pop("stream_ids"), kw.pop("volumes_db"), out=o, **kw)
        eng.sync()
        assert bool((o == SENTINEL).all()), msg
    with pytest.raises(ValueError, match="30.0"):
        lv.push(x, [0, 1], [3.0, 30.0], out=out)
    with pytest.raises(ValueError, match="30.0"):
        eng.apply_level(x, 30.0)
    with pytest.raises(ValueError, match="0.5"):
        eng.apply_level(x, 0.0, 0.5)
    with pytest.raises(ValueError, match="samples"):
        eng.apply_level(x[None])
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_level_reset(eng._ctx, eng._s, 9, 1, None), "vv_level_reset")
    with pytest.raises(EngineError, match="A = 0 must be"):
        eng._chk(eng.lib.vv_level_set(eng._ctx, 3, 0, 100, 0.5, 1, eng._s), "vv_level_set")
    with pytest.raises(EngineError, match="H = 8000"):
        eng._chk(eng.lib.vv_level_set(eng._ctx, 3, 120, 8000, 0.5, 1, eng._s), "vv_level_set")
    assert lv.total == [0, 1000, 0, 1000]
    nxt = _voice(73, 2000, amp=1.5)
    a = _push(eng, lv, [nxt], [1], [3.0], flush=True)
    b = _push(eng, twin, [nxt], [1], [3.0], flush=True)
    assert a[0].shape[0] == 2000 + 119 and _same(a[0], b[0])
    with torch.cuda.stream(eng.stream):
        lv.reset([3])
    a = _push(eng, lv, [nxt], [3], [-6.0], flush=True)                    # after its reset a stream takes another volume
    assert _same(a[0], torch.from_numpy(V.level_ref(nxt, -6.0)))
    assert _push(eng, lv, [np.zeros(0, dtype=np.float32)], [2], [0.0], flush=True)[0].shape[0] == 0      # a flush with no push before it


def test_other_dtypes_and_rates(small):
    eng = small.eng
    x = _voice(74, 500, amp=1.5)
    with torch.cuda.stream(eng.stream):
        h = eng.apply_level(torch.from_numpy(x).to(torch.float16))           # any float dtype, any device
        d = eng.apply_level(torch.from_numpy(x).to(torch.float64), 3.0, -6.0, 48000)
    eng.sync()
    assert _same(h.cpu(), torch.from_numpy(V.level_ref(x.astype(np.float16).astype(np.float32))))
    assert _same(d.cpu(), torch.from_numpy(V.level_ref(x, 3.0, -6.0, 48000)))


def _collect(st, idx):
    return list(st.get_stream(idx))


@pytest.mark.parametrize("mode", ["alone", "speed", "48k", "speed_48k"])
def test_streamer_level_float_and_int16(small, mode):
    """AudioStreamer(volume_db=[0, 9], ceiling_db=-1) over device chunks, alone, behind speed=1.25, behind sample_rate=48000 and behind
    both; sample 1 ends early, the first put completes nothing at sample 0's level stage.  Per sample the float chunks concatenate to
    level_ref of what reaches the stage -- the input, stretch_ref of it, Engine.resample of that -- bit for bit, and the int16 streamer
    delivers, chunk for chunk, trunc(* 32767) of the float one: no chunk is rescaled."""
    eng = small.eng
    speed, rate = (1.25 if "speed" in mode else None), (48000 if "48k" in mode else None)
    vols = [0.0, 9.0]
    n = 3 * 3200 + 100
    x = torch.from_numpy(np.stack([_voice(80, n, amp=2.0), _voice(81, n, amp=0.5)])[:, None, :]).to(eng.device)
    sts = [AudioStreamer(2, pcm16=eng, sample_rate=rate, speed=speed, volume_db=vols, ceiling_db=CEIL_DB, timeout=20),
           AudioStreamer(2, engine=eng, sample_rate=rate, speed=speed, volume_db=vols, ceiling_db=CEIL_DB, timeout=20)]
    assert all(st._stages[-1] is st._lv and st._lv.rate == (rate or 24000) and len(st._stages) == 1 + (speed is not None) + (rate is not None)
               for st in sts)
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :100], torch.tensor([0, 1]))
            for k in range(2):
                st.put(x[:, :, 100 + k * 3200:100 + (k + 1) * 3200], torch.tensor([0, 1]))
            st.end(torch.tensor([1]))
            st.put(x[:1, :, 100 + 2 * 3200:], torch.tensor([0]))
            st.end()
        front = []
        for idx, m in ((0, n), (1, 100 + 2 * 3200)):
            y = x[idx, 0, :m]
            if speed is not None:
                y = torch.from_numpy(T.stretch_ref(y.cpu().numpy(), speed)).to(eng.device)
            front.append(eng.resample(y, 24000, rate) if rate is not None else y)
    eng.sync()
    c = float(V.ceiling_of(CEIL_DB))
    for idx in range(2):
        want = V.level_ref(front[idx].cpu().numpy(), vols[idx], CEIL_DB, rate or 24000)
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert all(ch.dtype == torch.int16 for ch in q) and all(ch.dtype == torch.float32 for ch in f)
        assert [ch.shape for ch in q] == [ch.shape for ch in f] and all(ch.dim() == 2 and ch.shape[0] == 1 and ch.shape[1] > 0 for ch in f)
        cat = torch.cat(f, dim=-1)[0]
        assert _same(cat, torch.from_numpy(want)), (mode, idx)
        assert float(cat.abs().max()) <= c < float(front[idx].abs().max()) * float(V.gain_of(vols[idx]))
        assert torch.equal(torch.cat(q, dim=-1)[0], _pcm(want)), (mode, idx)
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._lv_used == [None] * 4                                     # finished streamers gave their configurations back
    assert eng.__dict__.get("_rs_used", [None] * 4) == [None] * 4 and eng.__dict__.get("_tp_used", [None] * 4) == [None] * 4


def test_streamer_pcm16_seam(small):
    """What the stage is for.  Two consecutive chunks with peaks 0.5 and 1.8: the plain 16-bit streamer divides the second chunk by its
    own peak, a gain step at the chunk boundary; through the level stage the delivered samples are trunc(level_ref(whole) * 32767),
    sample for sample: no per-chunk rescale, no seam."""
    eng = small.eng
    a, b = _voice(95, 3200), _voice(96, 3200)
    whole = np.concatenate([a * np.float32(0.5 / np.abs(a).max()), b * np.float32(1.8 / np.abs(b).max())]).astype(np.float32)
    assert abs(float(np.abs(whole[:3200]).max()) - 0.5) < 1e-3 and abs(float(np.abs(whole[3200:]).max()) - 1.8) < 1e-3
    x = torch.from_numpy(whole[None, None, :]).to(eng.device)
    sts = [AudioStreamer(1, pcm16=eng, ceiling_db=CEIL_DB, timeout=20), AudioStreamer(1, pcm16=eng, timeout=20)]
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :3200], torch.tensor([0]))
            st.put(x[:, :, 3200:], torch.tensor([0]))
            st.end()
    eng.sync()
    want, gain = V.level_ref(whole, 0.0, CEIL_DB, return_gain=True)
    got = torch.cat(_collect(sts[0], 0), dim=-1)[0]
    plain = torch.cat(_collect(sts[1], 0), dim=-1)[0]
    assert got.dtype == torch.int16 and torch.equal(got, _pcm(want))
    # the limiter's gain is continuous across the boundary (steps of at most 1 / A of its range), the plain rule's is not
    assert float(np.abs(np.diff(gain)).max()) <= 1.0 / 120 + 1e-6 and gain[3199 - 119] == 1.0 and gain[3200:].min() < 0.55
    assert torch.equal(plain[:3200], _pcm(whole[:3200])) and not torch.equal(plain[3200:], _pcm(np.clip(whole[3200:], -1, 1)))
    assert int(plain[3200:].abs().max()) == 32767 and int(got.abs().max()) <= int(V.ceiling_of(CEIL_DB) * np.float32(32767.0))
    for st in sts:
        st._thread.join(timeout=20)


def test_streamer_chunk_longer_than_one_level_push(small):
    """a put of 9000 samples at 24 kHz is more than one level push takes (6571): it goes in two pieces and arrives as two chunks"""
    eng = small.eng
    x = torch.from_numpy(_voice(97, 9000, amp=1.7)[None, None, :]).to(eng.device)
    st = AudioStreamer(1, engine=eng, volume_db=2.0, timeout=20)
    with torch.cuda.stream(eng.stream):
        st.put(x, torch.tensor([0]))
        st.end()
    eng.sync()
    f = _collect(st, 0)
    assert [ch.shape[-1] for ch in f] == [6571 - 119, 9000 - 6571, 119]
    assert _same(torch.cat(f, dim=-1)[0], torch.from_numpy(V.level_ref(x[0, 0].cpu().numpy(), 2.0)))
    st._thread.join(timeout=20)


def test_streamer_device_chunks_need_an_engine(small):
    x = torch.zeros((1, 1, 3200), device=small.eng.device)
    for kw in (dict(volume_db=3.0), dict(ceiling_db=-1.0)):
        st = AudioStreamer(1, timeout=5, **kw)
        with pytest.raises(ValueError, match="volume_db"):
            st.put(x, torch.tensor([0]))
        st.close()


@pytest.mark.parametrize("mode", ["plain", "pcm16", "48k"])
def test_streamer_without_a_level_is_unchanged(small, mode):
    """a streamer built with volume_db=0 and no ceiling delivers what one without the keywords delivers, byte for byte, and takes no
    level configuration"""
    eng = small.eng
    kw = {"plain": {}, "pcm16": dict(pcm16=eng), "48k": dict(pcm16=eng, sample_rate=48000)}[mode]
    x = torch.from_numpy(np.stack([3.0 * _voice(84, 6400), _voice(85, 6400)])[:, None, :]).to(eng.device).to(torch.bfloat16)
    sts = [AudioStreamer(2, timeout=20, **kw), AudioStreamer(2, timeout=20, volume_db=0.0, **kw)]
    assert all(st._lv is None and st._level is None for st in sts) and eng.__dict__.get("_lv_used", [None] * 4) == [None] * 4
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :3200], torch.tensor([0, 1]))
            st.put(x[:, :, 3200:], torch.tensor([0, 1]))
            st.end()
    eng.sync()
    for idx in range(2):
        a, b = (_collect(st, idx) for st in sts)
        assert len(a) == len(b) == (3 if mode == "48k" else 2)
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and torch.equal(u, v)
    for st in sts:
        st._thread.join(timeout=20)


def test_model_apply_level(small):
    from vibevoice_amd.modeling import _AudioRates

    class Model(_AudioRates):
        engine = small.eng
    x = _voice(86, 3000, amp=1.2)
    with torch.cuda.stream(small.eng.stream):
        y = Model().apply_level(torch.from_numpy(x), 5.0, -2.0)
    small.eng.sync()
    assert _same(y.cpu(), torch.from_numpy(V.level_ref(x, 5.0, -2.0)))
