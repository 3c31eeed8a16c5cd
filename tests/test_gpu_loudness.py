"""GPU tests of the loudness stage (csrc/loudness.hip: vv_loud_rows, vv_loud_once, vv_loud_energy) against vibevoice_amd/loudness.py.
The FIR is an exact integer sum evaluated in fp64, the energies are 64-bit integers and everything behind them is a single fp32
rounding per operation, so there is no tolerance anywhere in this file but one: the int64 energies are compared with ==, fp32 outputs
and gains with the definition's bit for bit (as 32-bit patterns).  The exception is the normalised signal of
test_model_loudness_functions, which the issue holds to its target within 0.01 LU.  Also the stage's chunk invariance and state
handling, its refusals, and AudioStreamer(loudness_lufs=...) on device chunks in front of the tempo change, the resampler and the level
stage.  Where the resampler stands behind it, the chain is held to the definitions over what Engine.resample delivers, as
test_gpu_level.py does.  A stream needs 4 counted segments (0.4 s) before its gain moves and 31 before it settles: the long cases are
3.5 s, the others 0.5 s and more."""
import types

import numpy as np
import pytest
import torch

import synth
from gpu_util import build_small
from vibevoice_amd import level as V
from vibevoice_amd import loudness as L
from vibevoice_amd import tempo as T
from vibevoice_amd.engine import EngineError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -77.25
HALF, LONG = 12000 + 17, 84000               # 0.5 s and an open sixth segment; 3.5 s
KINDS = ["sine", "noise", "impulses", "silence", "nonfinite", "worst", "beyond_clamp"]
IDS5 = [5, 0, 3, 6, 2]
TARGETS5 = [-16.0, -23.0, -30.0, -12.0, -20.0]
STARTS5 = [0.0, 6.0, -6.0, 3.0, -12.0]
BOOSTS5 = [12.0, 6.0, 24.0, 0.0, 18.0]


@pytest.fixture(scope="module")
def small():
    lm = synth.LMCfg(hidden=256, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
    s = build_small(lm, xsplit=3, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    yield s
    s.eng.close()


@pytest.fixture()
def make(small):
    made = []

    def _make(n_streams=7):
        made.append(small.eng.loudness(n_streams))
        return made[-1]
    yield _make
    for t in made:
        t.close()


def _signal(kind, n, seed=0):
    rng = np.random.default_rng(100 + seed)
    t = np.arange(n)
    if kind == "sine":
        return ((0.05 + 0.03 * seed) * np.sin(2 * np.pi * (997.0 + 50 * seed) * t / 24000.0)).astype(np.float32)
    if kind == "noise":
        env = 1.0 + 0.8 * np.sin(2 * np.pi * t / 9000.0)                # the level moves: so does the gain
        return (0.08 * env * rng.standard_normal(n)).astype(np.float32)
    if kind == "impulses":
        x = np.zeros(n, dtype=np.float32)
        x[::397] = rng.choice([-1.0, 1.0], size=x[::397].shape[0]) * 0.9
        return x
    if kind == "silence":
        return np.zeros(n, dtype=np.float32)
    if kind == "nonfinite":
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        if n >= 8:
            x[n // 3], x[n // 2], x[(2 * n) // 3] = np.nan, np.inf, -np.inf
        return x
    if kind == "worst":                                                 # +-8 in the sign pattern of the reversed taps
        sg = np.where(L.taps()[::-1] < 0, -8.0, 8.0).astype(np.float32)
        return np.tile(sg, n // L.T + 1)[:n]
    if kind == "beyond_clamp":
        return (20.0 * rng.standard_normal(n)).astype(np.float32)
    raise KeyError(kind)


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same(got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    return got.dtype == want.dtype == torch.float32 and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


_REF = {}


def _ref(kind, n, seed, target, start, boost):
    """leveller_ref (output, gain) of a test signal, computed once per file"""
    key = (kind, n, seed, target, start, boost)
    if key not in _REF:
        _REF[key] = L.leveller_ref(_signal(kind, n, seed), target, start, boost, return_gain=True)
    return _REF[key]


@pytest.mark.parametrize("kind", KINDS)
def test_segment_energies_are_the_definition(small, kind):
    """Engine.segment_energies over the lengths around one and two segments and one of three segments and a rest, 1 row and 3: the
    int64 energies of segment_energies_ref, integer for integer"""
    eng = small.eng
    jobs = []
    with torch.cuda.stream(eng.stream):
        for n in (1, 2399, 2400, 2401, 4800, 7217):
            x = _signal(kind, n)
            jobs.append((n, [x], eng.segment_energies(torch.from_numpy(x)), eng.segment_energies(torch.from_numpy(x), fine=True)))
        xs = [_signal(kind, 7217, seed) for seed in range(3)]
        xd = torch.from_numpy(np.stack(xs))
        jobs.append((7217, xs, eng.segment_energies(xd), eng.segment_energies(xd, fine=True)))
    eng.sync()
    for n, xs, E, F in jobs:
        assert E.dtype == F.dtype == torch.int64 and E.shape[-1] == F.shape[-1] == n // L.S
        E, F = E.cpu().reshape(len(xs), -1), F.cpu().reshape(len(xs), -1)
        for r, x in enumerate(xs):
            assert E[r].tolist() == L.segment_energies_ref(x).tolist(), (kind, n, r)
            assert F[r].tolist() == L.segment_energies_ref(x, fine=True).tolist(), (kind, n, r)      # the meter's, at 16 times the resolution
    if kind == "worst":                                                  # the bound itself is reached, not only approached
        z = int(np.abs(L.taps().astype(np.int64)).sum()) * 8 * 2 ** 20
        assert 2 ** 48 < z < 2 ** 49 and max(L.segment_energies_ref(_signal(kind, 4800)).tolist()) < 2 ** 54
        assert 2 ** 53 < int(F.max()) < 2 ** 62                           # past what a float64 sum would keep exact
    if kind == "silence":
        assert not E.any()


@pytest.mark.parametrize("kind,n", [(k, HALF) for k in KINDS] + [("sine", LONG), ("noise", LONG)])
def test_apply_loudness_is_the_definition(small, kind, n):
    """Engine.apply_loudness(return_gain=True): output and gain of leveller_ref, bit for bit; at 3.5 s the gain has moved many times"""
    eng = small.eng
    x = _signal(kind, n)
    with torch.cuda.stream(eng.stream):
        y, g = eng.apply_loudness(torch.from_numpy(x), -18.0, 3.0, 15.0, return_gain=True)
        y2 = eng.apply_loudness(torch.from_numpy(np.stack([x, _signal(kind, n, 1)])), -18.0, 3.0, 15.0)
    eng.sync()
    want, a = _ref(kind, n, 0, -18.0, 3.0, 15.0)
    assert y.shape == (n,) and _same(y.cpu(), torch.from_numpy(want)), (kind, n)
    assert _same(g.cpu(), torch.from_numpy(a)), (kind, n)
    assert _same(y2[0].cpu(), torch.from_numpy(want)) and _same(y2[1].cpu(), torch.from_numpy(_ref(kind, n, 1, -18.0, 3.0, 15.0)[0]))
    g0 = L.start_of(3.0)
    assert (a[:4 * L.S + 1] == g0).all()                                  # start_db holds until 4 segments have counted
    if kind in ("sine", "noise", "nonfinite"):
        assert (a[5 * L.S:] != g0).any()
    if kind == "silence":
        assert (a == g0).all()
    if n == LONG:
        assert len(set(a[::L.S].tolist())) >= (3 if kind == "sine" else 20)


def _push(eng, ld, chunks, ids, par, flush=False):
    """One push of the rows `chunks` (1-D numpy arrays, lengths may differ: n_in per row) into guarded buffers: a sentinel row above and
    below the output rows and sentinel columns behind every row's count -> per-row outputs"""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[i, :c.shape[0]] = torch.from_numpy(c)
    want = [int(c.shape[0]) for c in chunks]
    assert want == [ld.counts(ids[i], want[i], flush) for i in range(n)]
    out = torch.full((n + 2, max(want) + GUARD), SENTINEL, dtype=torch.float32, device=eng.device)
    xd = xin.to(eng.device)
    torch.cuda.synchronize()
    tg, sd, mb = par
    with torch.cuda.stream(eng.stream):
        _, cnts = ld.push(xd, ids, tg, sd, mb, flush=flush, out=out[1:n + 1], n_in=want)
    eng.sync()
    host = out.cpu()
    assert cnts == want, (cnts, want)
    assert bool((host[0] == SENTINEL).all()) and bool((host[n + 1] == SENTINEL).all()), "guard rows were written"
    for i in range(n):
        assert bool((host[1 + i, cnts[i]:] == SENTINEL).all()), f"row {i}: written beyond its {cnts[i]} samples"
    return [host[1 + i, :cnts[i]].clone() for i in range(n)]


def test_five_streams_five_targets_one_launch(small, make):
    """5 streams with five targets, start gains and bounds in one push per step; row i of step k brings cut (k + i) % 6 of
    {0, 1, 2399, 2400, 641, 3200}: unequal totals, rows of no samples, and row 0 stands exactly on a segment boundary after step 2.
    The rows travel in reversed order on alternate steps.  Every stream's concatenation is leveller_ref of its input, and the one-shot
    kernel gives the same."""
    eng, ld = small.eng, make()
    assert (ld.max_in, ld.delay_samples, ld.rate) == (3200, 0, 24000)
    cuts = [0, 1, 2399, 2400, 641, 3200]
    steps = 14
    feed = [[cuts[(k + i) % 6] for k in range(steps)] for i in range(5)]
    assert sum(feed[0][:3]) == L.S
    kinds = ["noise", "sine", "nonfinite", "noise", "impulses"]
    sig = [_signal(kinds[i], sum(feed[i]), 10 + i) for i in range(5)]
    at, got = [0] * 5, [[] for _ in range(5)]
    for k in range(steps):
        order = list(range(5)) if k % 2 == 0 else list(range(4, -1, -1))
        chunks = [sig[i][at[i]:at[i] + feed[i][k]] for i in order]
        par = tuple([p[i] for i in order] for p in (TARGETS5, STARTS5, BOOSTS5))
        outs = _push(eng, ld, chunks, [IDS5[i] for i in order], par, flush=k == steps - 1)
        for j, i in enumerate(order):
            got[i].append(outs[j])
            at[i] += feed[i][k]
    moved = 0
    for i in range(5):
        want, a = L.leveller_ref(sig[i], TARGETS5[i], STARTS5[i], BOOSTS5[i], return_gain=True)
        moved += len(set(a[::L.S].tolist())) > 2
        assert _same(torch.cat(got[i]), torch.from_numpy(want)), i
        with torch.cuda.stream(eng.stream):
            once = eng.apply_loudness(torch.from_numpy(sig[i]), TARGETS5[i], STARTS5[i], BOOSTS5[i])
        eng.sync()
        assert _same(once.cpu(), torch.from_numpy(want)), i
    assert moved >= 4


def test_sixty_small_pushes(small, make):
    """60 pushes of 211 samples: segments close in the middle of pushes, the ring of inputs wraps five times"""
    eng, ld = small.eng, make(2)
    x = _signal("noise", 60 * 211, 3)
    par = ([-20.0], [2.0], [9.0])
    got = [_push(eng, ld, [x[k * 211:(k + 1) * 211]], [1], par, flush=k == 59)[0] for k in range(60)]
    want, a = L.leveller_ref(x, -20.0, 2.0, 9.0, return_gain=True)
    assert a[-1] != a[0] and _same(torch.cat(got), torch.from_numpy(want))


def test_sixteen_rows_and_seventeen_ids(small, make):
    """16 rows in one launch; 17 ids through push (two launches): every row leveller_ref of its own signal with its own target"""
    eng, ld = small.eng, make(17)
    for n in (16, 17):
        with torch.cuda.stream(eng.stream):
            ld.reset()
        x = np.stack([_signal("noise", HALF, 20 + i) * np.float32(0.5 + 0.2 * i) for i in range(n)])
        ids = [(7 * i + 3) % n for i in range(n)]
        par = ([TARGETS5[i % 5] for i in range(n)], [STARTS5[i % 5] for i in range(n)], [BOOSTS5[i % 5] for i in range(n)])
        parts = [_push(eng, ld, list(x[:, a:b]), ids, par, flush=b == HALF) for a, b in ((0, 3200), (3200, 6400), (6400, 9600), (9600, HALF))]
        for i in range(n):
            want = L.leveller_ref(x[i], par[0][i], par[1][i], par[2][i])
            assert _same(torch.cat([p[i] for p in parts]), torch.from_numpy(want)), (n, i)


def test_a_chunk_longer_than_one_push_goes_in_pieces_of_take(small, make):
    """a chunk of 2 * max_in + 1000 samples: refused whole, by name, with nothing changed; in pieces of take() the definition"""
    eng, ld = small.eng, make(2)
    n = 2 * ld.max_in + 1000
    x = _signal("noise", n, 4) * np.float32(3.0)
    xd = torch.from_numpy(x[None]).to(eng.device)
    with pytest.raises(EngineError, match=f"at most {ld.max_in} per row"):
        ld.push(xd, [0], -16.0)
    assert ld.total == [0, 0]
    got, at = [], 0
    while at < n:
        w = ld.take([0], [n - at])
        assert w == min(ld.max_in, n - at)
        got.append(_push(eng, ld, [x[at:at + w]], [0], ([-16.0], [0.0], [12.0]), flush=at + w == n)[0])
        at += w
    assert len(got) == 3 and _same(torch.cat(got), torch.from_numpy(L.leveller_ref(x, -16.0)))


def test_refusals_change_nothing(small, make):
    """every refusal is an EngineError (or a ValueError for a parameter out of range) with its message; the sentinel-filled outputs stay
    untouched and stream 1 goes on to the definition of its whole input"""
    eng, ld = small.eng, make(4)
    sig = _signal("noise", 9600 + 3000, 5)
    par = ([-16.0], [0.0], [12.0])
    got = [_push(eng, ld, [sig[a:a + 3200]], [1], par)[0] for a in (0, 3200, 6400)]
    _push(eng, ld, [sig[:500]], [3], par, flush=True)
    x = torch.from_numpy(np.stack([_signal("noise", 3200, 6), _signal("noise", 3200, 7)])).to(eng.device)
    wide = torch.zeros((2, 3201), dtype=torch.float32, device=eng.device)
    out = torch.full((4, 4000), SENTINEL, dtype=torch.float32, device=eng.device)
    small_out = torch.full((4, 700), SENTINEL, dtype=torch.float32, device=eng.device)
    out16 = torch.full((4, 4000), int(SENTINEL), dtype=torch.int16, device=eng.device)
    cases = [
        (dict(audio=wide, stream_ids=[0, 2], targets_lufs=-16.0), "at most 3200 per row"),
        (dict(audio=x, stream_ids=[0, 1], targets_lufs=-16.0, out=small_out), "the output rows hold 700"),
        (dict(audio=x, stream_ids=[0, 4], targets_lufs=-16.0), "stream id 4 out of range"),
        (dict(audio=x, stream_ids=[0, -1], targets_lufs=-16.0), "stream id -1 out of range"),
        (dict(audio=x, stream_ids=[1, 1], targets_lufs=-16.0), "stream 1 is named twice"),
        (dict(audio=x, stream_ids=[0, 1], targets_lufs=[-16.0, -20.0]), "stream 1 runs at t ="),
        (dict(audio=x, stream_ids=[0, 1], targets_lufs=-16.0, start_db=[0.0, 1.0]), "stream 1 runs at t ="),
        (dict(audio=x, stream_ids=[0, 3], targets_lufs=-16.0), "stream 3 has been flushed"),
        (dict(audio=x, stream_ids=[0, 1], targets_lufs=-16.0, pcm16=True, out=out16), "int16.*never the last stage"),
        (dict(audio=x, stream_ids=[], targets_lufs=-16.0), r"n = 0 must be in \[1,16\]"),
    ]
    for kw, msg in cases:
        o = kw.pop("out", out)
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                ld.push(kw.pop("audio"), kw.pop("stream_ids"), kw.pop("targets_lufs"), out=o, **kw)
        eng.sync()
        assert bool((o == (int(SENTINEL) if o.dtype == torch.int16 else SENTINEL)).all()), msg
        assert ld.total == [0, 9600, 0, 500], msg
    for kw, name in ((dict(targets_lufs=-9.0), "target_lufs"), (dict(targets_lufs=float("nan")), "target_lufs"),
                     (dict(targets_lufs=-16.0, start_db=25.0), "start_db"), (dict(targets_lufs=-16.0, max_boost_db=-1.0), "max_boost_db")):
        with pytest.raises(ValueError, match=name):
            ld.push(x, [0, 2], out=out, **kw)
        with pytest.raises(ValueError, match=name):
            eng.apply_loudness(x, kw["targets_lufs"], kw.get("start_db", 0.0), kw.get("max_boost_db", 12.0))
    with pytest.raises(ValueError, match="samples"):
        eng.apply_loudness(x[None])
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_loud_reset(eng._ctx, eng._s, 9, 1, None), "vv_loud_reset")
    eng.sync()
    assert bool((out == SENTINEL).all()) and ld.total == [0, 9600, 0, 500]
    got.append(_push(eng, ld, [sig[9600:]], [1], par, flush=True)[0])
    want, a = L.leveller_ref(sig, -16.0, return_gain=True)
    assert a[-1] != a[0] and _same(torch.cat(got), torch.from_numpy(want))


def test_reset_of_some_streams_leaves_the_others(small, make):
    """streams 0 and 2 are reset in the middle of stream 1's signal and start over with other parameters; stream 1 goes on"""
    eng, ld = small.eng, make(3)
    sig = [_signal("noise", HALF, 30 + i) for i in range(3)]
    par = ([-16.0] * 3, [0.0] * 3, [12.0] * 3)
    a = [_push(eng, ld, [s[k:min(k + 3200, 9700)] for s in sig], [0, 1, 2], par) for k in (0, 3200, 6400, 9600)]
    with torch.cuda.stream(eng.stream):
        ld.reset([0, 2])
    assert ld.total == [0, 9700, 0]
    par2 = ([-25.0, -16.0, -12.0], [4.0, 0.0, -4.0], [6.0, 12.0, 20.0])
    b = _push(eng, ld, [sig[0][:3200], sig[1][9700:], sig[2][:3200]], [0, 1, 2], par2)
    assert _same(torch.cat([p[1] for p in a] + [b[1]]), torch.from_numpy(L.leveller_ref(sig[1], -16.0)))
    rest = [_push(eng, ld, [sig[0][k:k + 3200], sig[2][k:k + 3200]], [0, 2], ([-25.0, -12.0], [4.0, -4.0], [6.0, 20.0])) for k in (3200, 6400, 9600)]
    for j, i in enumerate((0, 2)):
        want = L.leveller_ref(sig[i], par2[0][i], par2[1][i], par2[2][i])
        assert _same(torch.cat([b[i]] + [r[j] for r in rest]), torch.from_numpy(want)), i


def _collect(st, idx):
    return list(st.get_stream(idx))


@pytest.mark.parametrize("mode", ["alone", "speed", "48k", "speed_48k"])
def test_streamer_loudness_float_and_int16(small, mode):
    """AudioStreamer(loudness_lufs=[-10, -23], loudness_start_db=[0, 6], max_boost_db=[24, 12]) over device chunks, alone, in front of
    speed=1.25, of sample_rate=48000 and of both; sample 1 ends early.  Per sample the float chunks concatenate to the host chain of the
    definitions over the whole signal -- leveller_ref, stretch_ref, Engine.resample, level_ref under the -1 dB ceiling the streamer
    adds -- bit for bit: no seam between chunks.  The int16 streamer delivers trunc(* 32767) of the float one, chunk for chunk, and no
    delivered sample exceeds the ceiling although the boost passes full scale."""
    eng = small.eng
    speed, rate = (1.25 if "speed" in mode else None), (48000 if "48k" in mode else None)
    tg, sd, mb = [-10.0, -23.0], [0.0, 6.0], [24.0, 12.0]
    n = 4 * 3200 + 100
    xs = np.stack([_signal("noise", n, 40) * np.float32(0.6), _signal("sine", n, 2)])
    x = torch.from_numpy(xs[:, None, :]).to(eng.device)
    kw = dict(sample_rate=rate, speed=speed, loudness_lufs=tg, loudness_start_db=sd, max_boost_db=mb, timeout=20)
    sts = [AudioStreamer(2, pcm16=eng, **kw), AudioStreamer(2, engine=eng, **kw)]
    for st in sts:
        assert st._stages[0] is st._ld and st._stages[-1] is st._lv and st._lv.ceiling_db == -1.0
        assert len(st._stages) == 2 + (speed is not None) + (rate is not None)
    with torch.cuda.stream(eng.stream):
        for st in sts:
            st.put(x[:, :, :100], torch.tensor([0, 1]))
            for k in range(3):
                st.put(x[:, :, 100 + k * 3200:100 + (k + 1) * 3200], torch.tensor([0, 1]))
            st.end(torch.tensor([1]))
            st.put(x[:1, :, 100 + 3 * 3200:], torch.tensor([0]))
            st.end()
        front = []
        for idx, m in ((0, n), (1, 100 + 3 * 3200)):
            y = L.leveller_ref(xs[idx, :m], tg[idx], sd[idx], mb[idx])
            if speed is not None:
                y = T.stretch_ref(y, speed)
            y = torch.from_numpy(y).to(eng.device)
            front.append(eng.resample(y, 24000, rate) if rate is not None else y)
    eng.sync()
    c = float(V.ceiling_of(-1.0))
    for idx in range(2):
        want = V.level_ref(front[idx].cpu().numpy(), 0.0, -1.0, rate or 24000)
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert all(ch.dtype == torch.int16 for ch in q) and all(ch.dtype == torch.float32 for ch in f)
        assert [ch.shape for ch in q] == [ch.shape for ch in f] and all(ch.dim() == 2 and ch.shape[0] == 1 and ch.shape[1] > 0 for ch in f)
        cat = torch.cat(f, dim=-1)[0]
        assert _same(cat, torch.from_numpy(want)), (mode, idx)
        assert float(cat.abs().max()) <= c
        assert torch.equal(torch.cat(q, dim=-1)[0], torch.from_numpy(np.trunc(want * np.float32(32767.0)).astype(np.int16))), (mode, idx)
    assert float(front[0].abs().max()) > c                                 # the boost passed the ceiling: the limiter had work
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._ld_used == [None] * 4 and eng._lv_used == [None] * 4      # finished streamers gave their configurations back


def test_streamer_device_chunks_need_an_engine(small):
    x = torch.zeros((1, 1, 3200), device=small.eng.device)
    st = AudioStreamer(1, timeout=5, loudness_lufs=-16.0)
    with pytest.raises(ValueError, match="loudness_lufs"):
        st.put(x, torch.tensor([0]))
    st.close()


@pytest.mark.parametrize("mode", ["plain", "pcm16", "48k"])
def test_streamer_without_loudness_is_unchanged(small, mode):
    """a streamer without the new arguments has no loudness stage, takes no loudness configuration and delivers what the stages it has
    define: the chunks themselves, Engine.audio_to_pcm16 of each chunk, Engine.resample of the whole signal"""
    eng = small.eng
    kw = {"plain": {}, "pcm16": dict(pcm16=eng), "48k": dict(engine=eng, sample_rate=48000)}[mode]
    xs = np.stack([3.0 * _signal("noise", 6400, 50), _signal("sine", 6400, 1)]).astype(np.float32)
    x = torch.from_numpy(xs[:, None, :]).to(eng.device)
    st = AudioStreamer(2, timeout=20, **kw)
    assert st._ld is None and st._loud is None and not any(type(s).__name__ == "Loudness" for s in st._stages)
    assert eng.__dict__.get("_ld_used", [None] * 4) == [None] * 4
    with torch.cuda.stream(eng.stream):
        st.put(x[:, :, :3200], torch.tensor([0, 1]))
        st.put(x[:, :, 3200:], torch.tensor([0, 1]))
        st.end()
        pcm = torch.empty((2, 2, 3200), dtype=torch.int16, device=eng.device)
        for k in range(2):
            eng.audio_to_pcm16(x[:, 0, k * 3200:(k + 1) * 3200].contiguous(), pcm[k])
        rs = eng.resample(x[:, 0], 24000, 48000)
    eng.sync()
    for idx in range(2):
        got = _collect(st, idx)
        if mode == "plain":
            assert len(got) == 2 and all(torch.equal(g, x[idx, :, k * 3200:(k + 1) * 3200].cpu()) for k, g in enumerate(got))
        elif mode == "pcm16":
            assert len(got) == 2 and all(torch.equal(g[0], pcm[k, idx].cpu()) for k, g in enumerate(got))
        else:
            assert _same(torch.cat(got, dim=-1)[0], rs[idx].cpu())
    st._thread.join(timeout=20)


def test_model_loudness_functions(small):
    """model.measure_loudness is measure_ref; normalize_loudness brings a 0.1-amplitude sine to -16 LUFS within 0.01 LU (the gain keeps
    its peak under the ceiling: the limiter does not engage); apply_loudness is leveller_ref; silence is refused by name"""
    from vibevoice_amd.modeling import _AudioRates

    class Model(_AudioRates):
        engine = small.eng
    m, eng = Model(), small.eng
    t = np.arange(5 * 24000)
    x = (0.1 * np.sin(2 * np.pi * 1000.0 * t / 24000.0)).astype(np.float32)
    two = np.stack([x[:48000], _signal("noise", 48000, 60)])
    with torch.cuda.stream(eng.stream):
        lu = m.measure_loudness(torch.from_numpy(x))
        lu2 = m.measure_loudness(torch.from_numpy(two))
        y = m.normalize_loudness(torch.from_numpy(x), -16.0)
        after = m.measure_loudness(y)
        z = m.apply_loudness(torch.from_numpy(x[:HALF]), -16.0)
    eng.sync()
    assert lu.dtype == torch.float64 and lu.shape == () and float(lu) == L.measure_ref(x)
    assert lu2.shape == (2,) and lu2.tolist() == [L.measure_ref(two[0]), L.measure_ref(two[1])]
    assert float(y.abs().max()) < float(V.ceiling_of(-1.0))
    print(f"normalised to {float(after):.5f} LUFS from {float(lu):.5f}")
    assert abs(float(after) - (-16.0)) <= 0.01
    assert _same(z.cpu(), torch.from_numpy(L.leveller_ref(x[:HALF], -16.0)))
    with pytest.raises(ValueError, match="-inf"):
        m.normalize_loudness(torch.zeros(24000))
    with pytest.raises(ValueError, match="-inf"):
        m.normalize_loudness(torch.from_numpy(x[:7000]))                  # shorter than 400 ms
    with pytest.raises(ValueError, match="volume_db"):
        m.normalize_loudness(torch.from_numpy(x * np.float32(0.02)), -10.0)   # reads about -57 LUFS: +47 dB is not apply_level's
    assert float(m.measure_loudness(torch.zeros(24000))) == float("-inf")
    # under one segment there is no energy at all, 1-D and 2-D: -inf, and the refusal by name
    for short in (x[:1], x[:2399], two[:, :1000], two[:, :2399]):
        lu = m.measure_loudness(torch.from_numpy(short))
        assert lu.dtype == torch.float64 and lu.shape == short.shape[:-1] and bool((lu == float("-inf")).all())
        with pytest.raises(ValueError, match="-inf"):
            m.normalize_loudness(torch.from_numpy(short))
    assert eng.segment_energies(torch.from_numpy(two[:, :1000])).shape == (2, 0)


def test_generate_with_a_levelled_streamer_is_graph_safe():
    """generate() at toy shapes on a graph engine with AudioStreamer(loudness_lufs=...): the stage's launches on the producing stream
    leave the captured sequences kernel-only (vv_stat 5 = 0) and Engine.sync() does not raise; the delivered audio is the host chain of
    what generate() returns"""
    import test_gpu_generate as tg
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    s = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=512, use_graph=True)
    try:
        ids, mask, _, _, _ = tg.make_inputs(s, 1, False, 55)
        cfgd = {"decoder_config": {"max_position_embeddings": s.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
        tok = types.SimpleNamespace(speech_start_id=tg.TOK.speech_start_id, speech_end_id=tg.TOK.speech_end_id,
                                    speech_diffusion_id=tg.TOK.speech_diffusion_id, eos_token_id=tg.TOK.eos_token_id, bos_token_id=None,
                                    pad_token_id=tg.TOK.pad_token_id)
        m = VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.float32)
        m.set_speech_factors(s.scaling, s.bias)
        m.set_ddpm_inference_steps(5)
        st = AudioStreamer(1, engine=s.eng, loudness_lufs=-16.0, loudness_start_db=3.0, timeout=20.0)
        D, X = tg.D, tg.X
        torch.manual_seed(7)
        out = m.generate(input_ids=ids, attention_mask=mask, cfg_scale=1.3, tokenizer=tok, generation_config={"do_sample": False},
                         _forced_tokens=[[D, D, D, D, D, D, X]], show_progress_bar=False, audio_streamer=st)
        s.eng.sync()
        assert s.eng.stat(1) > 0 and s.eng.stat(5) == 0
        got = torch.cat([c.flatten() for c in st.get_stream(0)])
        wav = out.speech_outputs[0].detach().float().cpu().numpy().reshape(-1)
        want = V.level_ref(L.leveller_ref(wav, -16.0, 3.0), 0.0, -1.0)
        assert _same(got, torch.from_numpy(want))
    finally:
        s.eng.close()
