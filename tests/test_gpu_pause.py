"""GPU tests of the pause stage (csrc/pause.hip: vv_pause_rows, vv_pause_once) against vibevoice_amd/pause.py.  Every decision of the
definition is an integer one and the join is three single roundings, so there is no tolerance anywhere in this file: fp32 outputs are
compared with pause.shorten bit for bit (as 32-bit patterns), int16 outputs with trunc(shorten * 32767) exactly, counts and dropped
totals exactly.  The counts come from the device: the stage is the one whose host does not know them.  Also the stage's chunk
invariance and state handling, its refusals, and AudioStreamer(max_pause_ms=..., max_lead_ms=..., pause_threshold_db=...) on device
chunks behind the resampler and the level stage, held to shorten() of what Engine.apply_level(Engine.resample(x)) delivers.  One engine
serves the whole file: the small one of test_gpu_level.py.  Every signal is under two seconds."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import build_small
from vibevoice_amd import pause as P
from vibevoice_amd.engine import EngineError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

RATES = [8000, 24000, 48000]
GUARD, SENTINEL = 64, -77.25
N_STREAMS = 7


@pytest.fixture(scope="module")
def small():
    lm = synth.LMCfg(hidden=256, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
    s = build_small(lm, xsplit=3, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    yield s
    s.eng.close()


@pytest.fixture()
def make(small):
    made = []

    def _make(n_streams=N_STREAMS, rate=24000):
        made.append(small.eng.pause(n_streams, rate=rate))
        return made[-1]
    yield _make
    for t in made:
        t.close()


def _noise(rng, n, db):
    return (rng.standard_normal(n) * 10.0 ** (db / 20.0)).astype(np.float32)


def _bursts(rate, gaps, seed=0, burst=2, tail=0):
    """a gap of gaps[i] segments of -70 dBFS noise in front of every burst of `burst` segments of -20 dBFS noise, then `tail` quiet
    samples; within +-1"""
    seg, rng, parts = rate // 100, np.random.default_rng(seed), []
    for g in gaps:
        parts += [_noise(rng, g * seg, -70.0), _noise(rng, burst * seg, -20.0)]
    x = np.concatenate(parts + [_noise(rng, tail, -70.0)]).astype(np.float32)
    assert np.abs(x).max() < 1.0
    return x


def _runs_of(cap_ms, rate):
    """the run lengths the issue names for a cap: H, H + 1, C, C + 1, C + T, C + T + 1, 3 C"""
    C, _ = P.caps(rate, cap_ms)
    T, H = P.hold(C)
    return [H, H + 1, C, C + 1, C + T, C + T + 1, 3 * C]


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


def _push(eng, ps, chunks, ids, par, flush=False, pcm16=False):
    """One push of the rows `chunks` (1-D numpy arrays, lengths may differ: n_in per row) under par[i] = (max_pause_ms, max_lead_ms,
    threshold_db) into guarded buffers: a sentinel row above and below the output rows and sentinel columns behind every row's count.
    The counts are the device's.  Checks the guards -> per-row outputs."""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[i, :c.shape[0]] = torch.from_numpy(c)
    fl = [flush] * n if isinstance(flush, bool) else list(flush)
    cap = ps.max_out(width) + GUARD
    dt, sent = (torch.int16, int(SENTINEL)) if pcm16 else (torch.float32, SENTINEL)
    out = torch.full((n + 2, cap), sent, dtype=dt, device=eng.device)
    xd = xin.to(eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        _, cnts = ps.push(xd, ids, [p[0] for p in par], [p[1] for p in par], [p[2] for p in par], flush=fl, out=out[1:n + 1],
                          n_in=[int(c.shape[0]) for c in chunks], pcm16=pcm16)
    assert cnts.is_cuda and cnts.dtype == torch.int32 and tuple(cnts.shape) == (n,)
    eng.sync()
    host, cnts = out.cpu(), cnts.cpu().tolist()
    assert bool((host[0] == sent).all()) and bool((host[n + 1] == sent).all()), "guard rows were written"
    for i in range(n):
        assert 0 <= cnts[i] <= ps.max_out(int(chunks[i].shape[0]))
        assert bool((host[1 + i, cnts[i]:] == sent).all()), f"row {i}: written beyond its {cnts[i]} samples"
    return [host[1 + i, :cnts[i]].clone() for i in range(n)]


def _feed(eng, ps, sigs, ids, par, widths, pcm16=False):
    """every signal in pushes of `widths` (cycled; the last one repeats where it is a list that ends in None), a row flushing with the
    push that brings its last sample and leaving the launch behind it -> per row, the pieces it emitted"""
    at, got, live, k = [0] * len(sigs), [[] for _ in sigs], list(range(len(sigs))), 0
    while live:
        w = widths[k % len(widths)]
        k += 1
        chunks = [sigs[i][at[i]:at[i] + w] for i in live]
        fl = [at[i] + w >= len(sigs[i]) for i in live]
        outs = _push(eng, ps, chunks, [ids[i] for i in live], [par[i] for i in live], flush=fl, pcm16=pcm16)
        for j, i in enumerate(live):
            got[i].append(outs[j])
            at[i] += w
        live = [i for i, f in zip(live, fl) if not f]
    return got


def _pieces(eng, ps, x, sid, par, flush):
    """x to stream sid in pushes of max_in, the last one the flush where asked -> what they emitted"""
    out = [_push(eng, ps, [x[at:at + ps.max_in]], [sid], par, flush=flush and at + ps.max_in >= len(x))[0]
           for at in range(0, max(len(x), 1), ps.max_in)]
    return torch.cat(out)


@pytest.mark.parametrize("cuts", ["whole", "cycle"])
@pytest.mark.parametrize("rate", RATES)
def test_rows_are_the_definition(small, make, rate, cuts):
    """vv_pause_rows against pause.shorten: caps of 100 ms (C = 10, T = 5: a ring shorter than 10) and 200 ms (C = 20, T = 10) side by
    side in one launch, runs of H, H + 1, C, C + 1, C + T, C + T + 1 and 3 C segments each; as 7680-wide pushes (hold, join and release
    inside single pushes) and as a cycle of seg - 1, 1, seg + 1, 7 and the frame size; fp32 in one configuration, int16 in a twin"""
    eng, seg = small.eng, rate // 100
    ps, twin = make(rate=rate), make(rate=rate)
    assert (ps.seg, ps.delay_samples, ps.max_in, ps.max_out(3200)) == (seg, seg - 1, 7680, 3200 + seg - 1 + 10 * seg)
    par = [(100, None, -50.0), (200, None, -50.0)]
    sigs = [_bursts(rate, _runs_of(ms, rate), seed=ms, tail=seg // 3) for ms, _, _ in par]
    assert all(len(s) < 2 * rate for s in sigs)
    widths = [7680] if cuts == "whole" else [seg - 1, 1, seg + 1, 7, 3200]
    ids = [4, 1]
    got = _feed(eng, ps, sigs, ids, par, widths)
    gq = _feed(eng, twin, sigs, ids, par, widths, pcm16=True)
    dropped = []
    for i in range(2):
        want, d = P.shorten(sigs[i], rate, *par[i])
        C, _ = P.caps(rate, par[i][0])
        assert d == (1 + P.hold(C)[0] + P.hold(C)[0] + 1 + 2 * C) * seg
        dropped.append(d)
        assert _same(torch.cat(got[i]), torch.from_numpy(want)), (rate, cuts, i)
        assert torch.equal(torch.cat(gq[i]), _pcm(want)), (rate, cuts, i)
    assert ps.dropped(ids, stream=eng.stream) == dropped == twin.dropped(ids, stream=eng.stream)
    assert ps.totals(ids, stream=eng.stream) == [(len(s), len(s) - d, d) for s, d in zip(sigs, dropped)]
    assert [ps.total[i] for i in ids] == [len(s) for s in sigs]


@pytest.mark.parametrize("rate", RATES)
def test_cuts_at_the_edges_of_the_hold(small, make, rate):
    """a push that ends with segment H + 1 of a run (the one kept as `first`, the first one held) while the loud segment opens the next
    push; the same with the cut behind segment C + 1 and behind the whole run of 3 C"""
    eng, seg = small.eng, rate // 100
    ps = make(rate=rate)
    T, H = P.hold(10)
    sid = 0
    for R in (H + 1, 11, 30):
        for cut_at in sorted({H + 1, min(R, 11), R}):
            x = _bursts(rate, [0, R, 3], seed=R)
            par = [(100, None, -50.0)]
            first = (2 + cut_at) * seg
            a = _pieces(eng, ps, x[:first], sid, par, False)
            b = _pieces(eng, ps, x[first:], sid, par, True)
            want, d = P.shorten(x, rate, 100)
            assert d == max(R - 10, 0) * seg
            assert a.shape[0] == (2 + min(cut_at, H)) * seg              # what is held has not left
            assert _same(torch.cat([a, b]), torch.from_numpy(want)), (rate, R, cut_at)
            sid += 1
    assert sid <= N_STREAMS


@pytest.mark.parametrize("rate", RATES)
def test_flushes(small, make, rate):
    """four streams flushed in one launch: while holding with R > C, with R <= C, with only a partial segment, and with nothing but quiet
    shorter than the lead cap; then a flush that brings nothing, for a stream that holds a run above its cap and one never pushed"""
    eng, seg = small.eng, rate // 100
    ps = make(rate=rate)
    rng = np.random.default_rng(rate)
    loud, q = _noise(rng, 2 * seg, -20.0), _noise(rng, 30 * seg, -70.0)
    sigs = [np.concatenate([loud, q[:13 * seg + 33]]), np.concatenate([loud, q[:8 * seg + 1]]), q[:33], q[:4 * seg + 9]]
    par = [(100, None, -50.0), (100, None, -50.0), (100, 0, -50.0), (100, 50, -50.0)]
    ids = [3, 0, 5, 2]
    outs = _push(eng, ps, sigs, ids, par, flush=True)
    for i in range(4):
        want, d = P.shorten(sigs[i], rate, *par[i])
        assert d == (3 * seg if i == 0 else 0) and (i == 0 or len(want) == len(sigs[i]))
        assert _same(outs[i], torch.from_numpy(want)), (rate, i)
    assert ps.dropped(ids, stream=eng.stream) == [3 * seg, 0, 0, 0]
    a = _push(eng, ps, [sigs[0]], [1], par[:1])[0]
    assert a.shape[0] == 7 * seg                                         # the burst and H = 5 segments: T are held, 33 samples wait
    b, c = _push(eng, ps, [np.zeros(0, dtype=np.float32)] * 2, [1, 6], par[:2], flush=True)
    assert _same(torch.cat([a, b]), outs[0]) and c.shape[0] == 0
    with pytest.raises(EngineError, match="stream 1 has been flushed"):
        ps.push(None, [1], 100, flush=True)


def test_seventeen_rows_two_launches(small, make):
    """17 rows through one push call (two launches), non-identity stream ids, every row with its own caps and threshold; the uncapped
    row equals its input, a NaN and an inf inside loud segments are copied as they are"""
    eng, rate, seg = small.eng, 24000, 240
    ps = make(17, rate=rate)
    n = 17
    ids = [(7 * i + 3) % n for i in range(n)]
    par = [((None, 100, 150, 400)[i % 4], (None, 0, 50, 20, None)[i % 5], (-50.0, -45.0, -60.0)[i % 3]) for i in range(n)]
    assert par[0] == (None, None, -50.0)
    sigs = [_bursts(rate, [3 + i, 11 + i, 2], seed=100 + i, tail=i) for i in range(n)]
    for i in (0, 5):
        sigs[i][(3 + i) * seg + 7], sigs[i][(3 + i) * seg + 300] = np.nan, -np.inf
    assert max(len(s) for s in sigs) <= 7000 + ps.max_in
    a = _push(eng, ps, [s[:3000] for s in sigs], ids, par)
    m = _push(eng, ps, [s[3000:7000] for s in sigs], ids, par)
    b = _push(eng, ps, [s[7000:] for s in sigs], ids, par, flush=True)
    some = 0
    for i in range(n):
        want, d = P.shorten(sigs[i], rate, *par[i])
        some += d > 0
        assert _same(torch.cat([a[i], m[i], b[i]]), torch.from_numpy(want)), i
    assert _same(torch.cat([a[0], m[0], b[0]]), torch.from_numpy(sigs[0])) and some >= 8
    assert ps.dropped(stream=eng.stream) == [P.shorten(sigs[ids.index(k)], rate, *par[ids.index(k)])[1] for k in range(n)]


def test_reset_makes_a_reused_stream_a_fresh_one(small, make):
    eng, rate, seg = small.eng, 8000, 80
    ps = make(3, rate=rate)
    par = [(100, 0, -50.0)]
    x = _bursts(rate, [4, 26], seed=7)
    _push(eng, ps, [x[:(4 + 2 + 19) * seg + 11]], [1], par)               # a loud segment seen, a run above the cap held, 11 samples wait
    _push(eng, ps, [x], [2], par, flush=True)
    assert ps.total == [0, (4 + 2 + 19) * seg + 11, len(x)]
    with torch.cuda.stream(eng.stream):
        ps.reset([1, 2])
    assert ps.total == [0, 0, 0] and ps.totals(stream=eng.stream) == [(0, 0, 0)] * 3
    y = _bursts(rate, [6, 13], seed=8, tail=5)
    other = [(100, None, -40.0)]                                        # after its reset a stream takes other parameters
    got = [_push(eng, ps, [y[:1000]], [k], other)[0] for k in (0, 1, 2)]
    got = [torch.cat([g, _push(eng, ps, [y[1000:]], [k], other, flush=True)[0]]) for k, g in zip((0, 1, 2), got)]
    want, d = P.shorten(y, rate, *other[0])
    assert d == 3 * seg and all(_same(g, torch.from_numpy(want)) for g in got)
    assert ps.dropped(stream=eng.stream) == [d, d, d]


def test_refusals_change_nothing(small, make):
    """every refusal is an EngineError with its message; the sentinel-filled outputs stay untouched and the streams where they were:
    stream 1 goes on like its twin"""
    eng, rate, seg = small.eng, 24000, 240
    ps, twin = make(4, rate=rate), make(4, rate=rate)
    par = [(100, None, -50.0)]
    first = _bursts(rate, [0, 17], seed=70)[:(2 + 14) * seg + 5]          # stream 1 holds T segments of a run above its cap
    _push(eng, ps, [first], [1], par)
    _push(eng, twin, [first], [1], par)
    _push(eng, ps, [first], [3], par, flush=True)
    before = ps.totals(stream=eng.stream)
    x = torch.from_numpy(np.stack([_bursts(rate, [5], seed=71, burst=8)[:3000], _bursts(rate, [5], seed=72, burst=8)[:3000]])).to(eng.device)
    wide = torch.zeros((2, 7681), dtype=torch.float32, device=eng.device)
    out = torch.full((4, 7681 + 11 * seg), SENTINEL, dtype=torch.float32, device=eng.device)
    small_out = torch.full((4, 3000 + seg - 1 + 10 * seg - 1), SENTINEL, dtype=torch.float32, device=eng.device)
    cases = [
        (dict(audio=x, stream_ids=[0, 1], max_pause_ms=[100, 200]), "stream 1 runs at C = 10"),
        (dict(audio=x, stream_ids=[0, 1], max_pause_ms=100, max_lead_ms=[None, 50]), "stream 1 runs at C = 10, C0 = 10"),
        (dict(audio=x, stream_ids=[0, 1], max_pause_ms=100, threshold_db=[-50.0, -49.0]), "stream 1 runs at"),
        (dict(audio=x, stream_ids=[0, 3], max_pause_ms=100), "stream 3 has been flushed"),
        (dict(audio=wide, stream_ids=[0, 2], max_pause_ms=100), "at most 7680 per row"),
        (dict(audio=x, stream_ids=[0, 2], max_pause_ms=100, out=small_out), f"may emit {3000 + 11 * seg - 1} samples, the output rows hold {3000 + 11 * seg - 2}"),
        (dict(audio=x, stream_ids=[0, 4], max_pause_ms=100), "stream id 4 out of range"),
        (dict(audio=x, stream_ids=[1, 1], max_pause_ms=100), "stream 1 is named twice"),
        (dict(audio=x, stream_ids=[0, 2], max_pause_ms=100, n_in=[400, -1]), "n_in = -1 must be >= 0"),
        (dict(audio=x, stream_ids=[], max_pause_ms=100), r"n = 0 must be in \[1,16\]"),
    ]
    for kw in cases:
        kw, msg = kw
        o = kw.pop("out", out)
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                ps.push(kw.pop("audio"), kw.pop("stream_ids"), out=o, **kw)
        eng.sync()
        assert bool((o == SENTINEL).all()), msg
    with pytest.raises(ValueError, match="max_pause_ms"):
        ps.push(x, [0, 2], [100, 50], out=out)
    with pytest.raises(ValueError, match="threshold_db"):
        eng.shorten_pauses(x, 100, threshold_db=-10.0)
    with pytest.raises(ValueError, match="samples"):
        eng.shorten_pauses(x[None], 100)
    with pytest.raises(ValueError, match="rate"):
        eng.pause(1, rate=96000)
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_pause_reset(eng._ctx, eng._s, 9, 1, None), "vv_pause_reset")
    with pytest.raises(EngineError, match="seg = 79 must be"):
        eng._chk(eng.lib.vv_pause_set(eng._ctx, 3, 79, None, 1, eng._s), "vv_pause_set")
    assert ps.total == [0, len(first), 0, len(first)] and ps.totals(stream=eng.stream) == before
    # the 5 waiting samples and 235 more make the run's 15th segment, three more follow: 18 under a cap of 10, then 12
    nxt = np.concatenate([_noise(np.random.default_rng(74), seg - 5, -70.0), _bursts(rate, [3, 12], seed=73)])
    a = _push(eng, ps, [nxt], [1], par, flush=True)
    b = _push(eng, twin, [nxt], [1], par, flush=True)
    assert a[0].shape[0] == (5 + 2 + 10 + 2) * seg and _same(a[0], b[0])
    assert ps.dropped([1], stream=eng.stream) == [(8 + 2) * seg]
    want, d = P.shorten(np.concatenate([first, nxt]), rate, 100)
    assert d == 10 * seg and _same(a[0], torch.from_numpy(want[7 * seg:]))


@pytest.mark.parametrize("rate", RATES)
def test_once_equals_push_and_flush(small, make, rate):
    """Engine.shorten_pauses (vv_pause_once) over 1 and 3 rows, many pushes long: the definition, so push + flush; lengths and dropped
    counts exactly; an uncapped call gives the input back"""
    eng, seg = small.eng, rate // 100
    sigs = [_bursts(rate, _runs_of(200, rate), seed=40 + r, tail=r * 7 + 1) for r in range(3)]
    n = min(len(s) for s in sigs)
    x = np.stack([s[:n] for s in sigs])
    with torch.cuda.stream(eng.stream):
        one, d1 = eng.shorten_pauses(torch.from_numpy(x[0]), 200, 0, rate=rate)
        three, d3 = eng.shorten_pauses(torch.from_numpy(x).to(eng.device), 200, 0, rate=rate)
        same, d0 = eng.shorten_pauses(torch.from_numpy(x[1]).to(torch.float64), rate=rate)
        tiny, dt = eng.shorten_pauses(torch.from_numpy(x[2, :seg - 1]), 100, 0, rate=rate)
    eng.sync()
    assert len(one) == 1 and len(three) == 3 and d0 == [0] and dt == [0]
    assert _same(same[0].cpu(), torch.from_numpy(x[1])) and _same(tiny[0].cpu(), torch.from_numpy(x[2, :seg - 1]))
    for r in range(3):
        want, d = P.shorten(x[r], rate, 200, 0)
        assert d > 0 and d3[r] == d and three[r].dim() == 1 and _same(three[r].cpu(), torch.from_numpy(want)), (rate, r)
    assert d1 == [d3[0]] and _same(one[0].cpu(), three[0].cpu())
    ps = make(1, rate=rate)
    got = _feed(eng, ps, [x[2]], [0], [(200, 0, -50.0)], [3200])
    assert _same(torch.cat(got[0]), three[2].cpu())


def test_model_shorten_pauses(small):
    from vibevoice_amd.modeling import _AudioRates

    class Model(_AudioRates):
        engine = small.eng
    x = _bursts(24000, [20, 30], seed=86)
    with torch.cuda.stream(small.eng.stream):
        y, d = Model().shorten_pauses(torch.from_numpy(x), 100, 0)
    small.eng.sync()
    want, dropped = P.shorten(x, 24000, 100, 0)
    assert d == [dropped] and _same(y[0].cpu(), torch.from_numpy(want))


def _collect(st, idx):
    return list(st.get_stream(idx))


def test_streamer_pauses_float_and_int16(small):
    """AudioStreamer(sample_rate=8000, volume_db=..., max_pause_ms=[100, None, 100], max_lead_ms=[0, None, None]) over 3200-sample device
    puts, float and pcm16; sample 2 ends early.  Per index the concatenated float chunks equal the definition applied to
    Engine.apply_level(Engine.resample(x)), the int16 streamer delivers, chunk for chunk, trunc(* 32767) of the float one; the index with
    neither cap passes bit for bit; index 0's first put is all lead-in and delivers nothing; end() delivers the tails in front of the
    stop signals; a streamer without the arguments has no such stage"""
    eng = small.eng
    vols = [3.0, 0.0, 6.0]
    pauses, leads = [100, None, 100], [0, None, None]
    rng = np.random.default_rng(90)
    x = np.stack([np.concatenate([_noise(rng, 4800, -70.0), _noise(rng, 2400, -20.0), _noise(rng, 8400, -70.0), _noise(rng, 2400, -20.0),
                                  _noise(rng, 1200, -70.0)]) for _ in range(3)])
    assert x.shape == (3, 6 * 3200)
    xd = torch.from_numpy(x[:, None, :]).to(eng.device)
    kw = dict(sample_rate=8000, volume_db=vols, max_pause_ms=pauses, max_lead_ms=leads, pause_threshold_db=-50.0, timeout=20)
    sts = [AudioStreamer(3, pcm16=eng, **kw), AudioStreamer(3, engine=eng, **kw)]
    assert all(st._stages == [st._rs, st._lv, st._ps] and st._ps.rate == 8000 for st in sts)
    plain = AudioStreamer(3, engine=eng, sample_rate=8000, volume_db=vols, timeout=20)
    assert plain._ps is None and plain._pause is None and plain._stages == [plain._rs, plain._lv]
    plain.close()
    with torch.cuda.stream(eng.stream):
        for st in sts:
            for k in range(3):
                st.put(xd[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1, 2]))
            st.end(torch.tensor([2]))
            for k in range(3, 6):
                st.put(xd[:2, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
            st.end()
        front = [eng.apply_level(eng.resample(xd[idx, 0, :m], 24000, 8000), vols[idx], -1.0, 8000)
                 for idx, m in ((0, 6 * 3200), (1, 6 * 3200), (2, 3 * 3200))]
    eng.sync()
    for idx in range(3):
        lv = front[idx].cpu().numpy()
        want, dropped = P.shorten(lv, 8000, pauses[idx], leads[idx])
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert all(ch.dtype == torch.int16 for ch in q) and all(ch.dtype == torch.float32 for ch in f)
        assert [ch.shape for ch in q] == [ch.shape for ch in f] and all(ch.dim() == 2 and ch.shape[0] == 1 and ch.shape[1] > 0 for ch in f)
        assert _same(torch.cat(f, dim=-1)[0], torch.from_numpy(want)), idx
        assert torch.equal(torch.cat(q, dim=-1)[0], _pcm(want)), idx
        assert (dropped > 0) == (idx != 1) and (idx != 1 or _same(torch.from_numpy(want), torch.from_numpy(lv)))
        if idx == 0:
            assert len(f) <= 6                                           # 6 puts and a tail, and the first put delivered nothing
            assert bool(P.classify(lv, 8000)[:13].all()) and not bool(P.classify(want, 8000)[0])
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._ps_used == [None] * 4 and eng._lv_used == [None] * 4 and eng._rs_used == [None] * 4


def test_streamer_device_chunks_need_an_engine(small):
    x = torch.zeros((1, 1, 3200), device=small.eng.device)
    for kw in (dict(max_pause_ms=400), dict(max_lead_ms=0)):
        st = AudioStreamer(1, timeout=5, **kw)
        with pytest.raises(ValueError, match="max_pause_ms"):
            st.put(x, torch.tensor([0]))
        st.close()
