"""vibevoice_amd/pause.py: the definition of the pause stage (quiet segments by an integer energy rule, caps in segments, the held
tail and its join), its streaming form on the host, the range checks, and AudioStreamer(max_pause_ms=..., max_lead_ms=...,
pause_threshold_db=...) on CPU chunks.  The device kernels are held to the same definition, bit for bit, in test_gpu_pause.py.  Nothing
here has a tolerance: runs are counted, lengths are integers, samples are compared as bits; the one inequality (the step across a
join) is the issue's."""
import numpy as np
import pytest
import torch

from vibevoice_amd import pause as P
from vibevoice_amd.streamer import AsyncAudioStreamer, AudioStreamer

RATES = [8000, 22050, 24000, 48000]
GAPS = [30, 5, 40, 41, 150, 39, 300, 77]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _noise(rng, n, db):
    """white noise of n samples at db dBFS (rms), float32"""
    return (rng.standard_normal(n) * 10.0 ** (db / 20.0)).astype(np.float32)


def _bursts(rate, gaps, seed=0, burst=7, gap_db=-70.0, fill=None):
    """a gap in front of every burst: gaps[i] segments of gap_db noise (or fill(n, at)), then `burst` segments of -20 dBFS noise"""
    seg, rng, parts, at = rate // 100, np.random.default_rng(seed), [], 0
    for g in gaps:
        parts.append(_noise(rng, g * seg, gap_db) if fill is None else fill(g * seg, at))
        parts.append(_noise(rng, burst * seg, -20.0))
        at += (g + burst) * seg
    return np.concatenate(parts).astype(np.float32)


def _runs(quiet):
    out, c = [], 0
    for f in quiet:
        if f:
            c += 1
        elif c:
            out.append(c)
            c = 0
    return out + ([c] if c else [])


def test_parameters():
    assert [P.seg_of(r) for r in RATES] == [80, 220, 240, 480]
    assert all(P.caps(r, 400, 50) == (40, 5) for r in RATES)
    assert P.caps(24000, None, None) == (P.NO_CAP, P.NO_CAP) and P.caps(24000, 400, None) == (40, 40) and P.caps(24000, None, 0) == (P.NO_CAP, 0)
    assert P.hold(40) == (10, 30) and P.hold(10) == (5, 5) and P.hold(5) == (2, 3) and P.hold(1) == (0, 1) and P.hold(0) == (0, 0)
    assert P.theta(24000, -50.0) == int(np.floor(240.0 * (32768.0 * 10.0 ** (-50.0 / 20.0)) ** 2)) == 2576980
    assert P.theta(48000, -20.0) > 2 ** 32                          # a 64-bit figure
    assert P.max_out(3200, 24000) == 3200 + 239 + 2400 and P.max_out(7680, 48000) == 7680 + 479 + 4800
    w, u = P.weights(8000)
    assert w.dtype == u.dtype == np.float32 and w.shape == u.shape == (80,)
    assert w[0] == np.float32(0.5 / 80) and u[0] == np.float32(1 - 0.5 / 80) and w[79] == u[0] and u[79] == w[0]
    assert P.STATE_FLOATS == 5760


@pytest.mark.parametrize("rate", RATES)
def test_the_issue_s_gaps(rate):
    """gaps of 30, 5, 40, 41, 150, 39, 300, 77 segments under a 400 ms cap and a 50 ms lead come out as 5, 5, 40, 40, 40, 39, 40, 40,
    re-measured with the definition's own classifier (the joins included: 30 and 20 dB either side of the threshold)"""
    x = _bursts(rate, GAPS)
    assert _runs(P.classify(x, rate)) == GAPS
    y, dropped = P.shorten(x, rate, 400, 50)
    assert y.dtype == np.float32
    assert _runs(P.classify(y, rate)) == [5, 5, 40, 40, 40, 39, 40, 40]
    assert len(x) - len(y) == dropped == (25 + 1 + 110 + 260 + 37) * (rate // 100)


@pytest.mark.parametrize("rate", [8000, 24000])
def test_host_stream_is_chunk_invariant(rate):
    """HostPause fed in pieces of 1, seg - 1, seg, seg + 1, the frame size and random widths equals shorten bit for bit"""
    seg = rate // 100
    x = _bursts(rate, [12, 3, 25, 10, 11], seed=1, burst=2)
    x = np.concatenate([x, _noise(np.random.default_rng(2), 14 * seg + 17, -70.0)])      # ends inside a held run, with a partial segment
    want, dropped = P.shorten(x, rate, 100, 30)
    assert dropped == (9 + 15 + 1 + 4) * seg
    rng = np.random.default_rng(3)
    for piece in (1, seg - 1, seg, seg + 1, 3200, None):
        h, at, got = P.HostPause(rate, 100, 30), 0, []
        while at < len(x):
            k = int(rng.integers(0, 900)) if piece is None else piece
            got.append(h.push(torch.from_numpy(x[at:at + k])))
            at += k
        got.append(h.flush())
        assert _same(torch.cat(got).numpy(), want), (rate, piece)
        assert (h.total_in, h.total_out, h.dropped) == (len(x), len(want), dropped)
        with pytest.raises(RuntimeError, match="flushed"):
            h.push(torch.zeros(3))
        h.reset()
        assert _same(torch.cat([h.push(x), h.flush()]).numpy(), want)


@pytest.mark.parametrize("rate", RATES)
def test_no_run_above_the_cap_passes_bit_for_bit(rate):
    x = _bursts(rate, [10, 3, 9, 1, 10], seed=4)[:-17]              # caps of 10 segments: every run fits; a partial segment at the end
    x[5], x[6], x[7] = -0.0, 1e-41, np.nan                          # a negative zero, a denormal and a NaN survive
    for kw in (dict(max_pause_ms=100), dict(max_pause_ms=100, max_lead_ms=100), dict(), dict(max_pause_ms=5000, max_lead_ms=5000)):
        y, dropped = P.shorten(x, rate, **kw)
        assert dropped == 0 and _same(y, x), kw


def _squares(total, slots):
    """integers q in [0, 32768], `slots` of them, whose squares sum to `total`"""
    q = []
    while total:
        r = min(int(np.sqrt(total)), 32768)
        while r * r > total:
            r -= 1
        q.append(r)
        total -= r * r
    assert len(q) <= slots
    return np.array(q + [0] * (slots - len(q)), dtype=np.int64)


@pytest.mark.parametrize("rate,db", [(8000, -50.0), (24000, -50.0), (48000, -20.0), (22050, -80.0)])
def test_the_threshold_is_an_integer(rate, db):
    """a segment of integer samples with E = Theta - 1 is quiet, with E = Theta it is not; under max_lead_ms=0 the first goes, the
    second stays"""
    seg, th = P.seg_of(rate), P.theta(rate, db)
    for E, quiet in ((th - 1, True), (th, False)):
        q = _squares(E, seg)
        x = (q.astype(np.float64) / 32768.0).astype(np.float32)
        x[::2] *= -1
        assert int(P.energies(x, rate)[0]) == E
        assert bool(P.classify(x, rate, db)[0]) is quiet
        y, dropped = P.shorten(x, rate, None, 0, db)
        assert (len(y), dropped) == ((0, seg) if quiet else (seg, 0))
    x = np.full(seg, np.inf, dtype=np.float32)                      # non-finite samples count as 0 and are copied as they are
    assert int(P.energies(x, rate)[0]) == 0
    assert int(P.energies(np.full(seg, 3.0, dtype=np.float32), rate)[0]) == seg * 32768 ** 2      # the clamp


@pytest.mark.parametrize("rate", RATES)
def test_a_lead_of_zero_starts_at_the_first_loud_segment(rate):
    seg = rate // 100
    x = _bursts(rate, [23, 4], seed=5)
    for pause in (None, 400):
        y, dropped = P.shorten(x, rate, pause, 0)
        assert dropped == 23 * seg and _same(y, x[23 * seg:])
    h = P.HostPause(rate, None, 0)
    assert h.push(x[:23 * seg + 5]).shape == (0,) and _same(h.push(x[23 * seg + 5:24 * seg]).numpy(), x[23 * seg:24 * seg])


@pytest.mark.parametrize("rate", RATES)
def test_the_join_is_no_louder_than_the_sine_it_joins(rate):
    """a -60 dBFS 100 Hz sine in the gaps: the largest step across a join does not exceed twice the sine's own largest step"""
    seg = rate // 100

    def sine(n, at):
        return (10.0 ** (-60.0 / 20.0) * np.sin(2 * np.pi * 100.0 * (np.arange(n) + at) / rate)).astype(np.float32)
    x = _bursts(rate, [4, 57, 133], seed=6, fill=sine)
    own = float(np.abs(np.diff(sine(4 * seg, 0))).max())
    y, dropped = P.shorten(x, rate, 400, 50)
    assert dropped == (17 + 93) * seg
    T, H = P.hold(40)
    for start in ((4 + 7) * seg, (4 + 7 + 40 + 7) * seg):           # where the two capped runs start in y
        a, b = start + H * seg, start + (H + 1) * seg                # the join segment
        assert float(np.abs(np.diff(y[a - 1:b + 1])).max()) <= 2 * own
    # the join by hand, for the first capped run: first = segment H + 1 of the run, b = segment R - T + 1
    r0 = (4 + 7) * seg
    w, u = P.weights(rate)
    first, held = x[r0 + H * seg:r0 + (H + 1) * seg], x[r0 + (57 - T) * seg:r0 + (57 - T + 1) * seg]
    want = (first * u).astype(np.float32) + (held * w).astype(np.float32)
    assert _same(y[r0 + H * seg:r0 + (H + 1) * seg], want)
    assert _same(y[r0 + (H + 1) * seg:r0 + 40 * seg], x[r0 + (57 - T + 1) * seg:r0 + 57 * seg])


def test_flushes():
    """the end of the stream counts as speech resuming: a held run above its cap is cut, one within it is released, a partial segment
    follows verbatim, and nothing but quiet below the lead cap passes"""
    rate, seg = 8000, 80
    rng = np.random.default_rng(7)
    loud, q = _noise(rng, 2 * seg, -20.0), _noise(rng, 40 * seg + 33, -70.0)
    y, d = P.shorten(np.concatenate([loud, q[:27 * seg + 33]]), rate, 100, None)
    assert d == 17 * seg and len(y) == 12 * seg + 33 and _same(y[-33:], q[27 * seg:27 * seg + 33]) and _same(y[-33 - 4 * seg:-33], q[23 * seg:27 * seg])
    y, d = P.shorten(np.concatenate([loud, q[:8 * seg + 1]]), rate, 100, None)
    assert d == 0 and _same(y, np.concatenate([loud, q[:8 * seg + 1]]))
    y, d = P.shorten(q[:33], rate, 100, 0)
    assert d == 0 and _same(y, q[:33])
    y, d = P.shorten(q[:4 * seg + 9], rate, 100, 50)
    assert d == 0 and _same(y, q[:4 * seg + 9])
    y, d = P.shorten(np.zeros(0, dtype=np.float32), rate, 100, 50)
    assert d == 0 and y.shape == (0,)
    assert P.HostPause(rate, 100).flush().shape == (0,)


@pytest.mark.parametrize("name,bad", [("max_pause_ms", 99.0), ("max_pause_ms", 5000.5), ("max_pause_ms", float("nan")), ("max_pause_ms", "long"),
                                      ("max_lead_ms", -1.0), ("max_lead_ms", 5001.0), ("max_lead_ms", float("nan")),
                                      ("threshold_db", -80.5), ("threshold_db", -19.0), ("threshold_db", float("nan")), ("threshold_db", None)])
def test_arguments_outside_their_range_are_refused_by_name(name, bad):
    good = dict(max_pause_ms=400.0, max_lead_ms=50.0, threshold_db=-50.0)
    kw = dict(good, **{name: bad})
    streamer = {("pause_" + k if k == "threshold_db" else k): v for k, v in kw.items()}
    calls = [lambda: P.shorten(np.zeros(10, dtype=np.float32), 24000, **kw), lambda: P.HostPause(24000, **kw)]
    if bad is not None:
        calls += [lambda: AudioStreamer(1, **streamer), lambda: AudioStreamer(2, **{k: [good.get(k[6:] if k.startswith("pause_t") else k), v]
                                                                               for k, v in streamer.items()})]
    for call in calls:
        with pytest.raises(ValueError, match=name):
            call()


def test_rates_and_orphans_are_refused_by_name():
    for rate in (7999, 48001, 24000.5, "fast"):
        with pytest.raises(ValueError, match="rate"):
            P.seg_of(rate)
        with pytest.raises(ValueError, match="rate"):
            P.shorten(np.zeros(10, dtype=np.float32), rate, 400)
    with pytest.raises(ValueError, match="rate"):
        AudioStreamer(1, max_pause_ms=400, sample_rate=96000)
    with pytest.raises(ValueError, match="pause_threshold_db.*belongs to max_pause_ms"):
        AudioStreamer(1, pause_threshold_db=-40.0)
    with pytest.raises(ValueError, match="pause_threshold_db.*belongs to max_pause_ms"):
        AudioStreamer(2, max_pause_ms=[None, None], pause_threshold_db=-40.0)
    for name in ("max_pause_ms", "max_lead_ms", "pause_threshold_db"):
        with pytest.raises(ValueError, match=f"{name}.*one per sample index"):
            AudioStreamer(2, **dict(dict(max_pause_ms=400), **{name: [100.0, 200.0, 300.0]}))


def _drain(st, idx):
    return list(st.get_stream(idx))


def test_streamer_pauses_on_cpu_chunks():
    """AudioStreamer(max_pause_ms=[100, None, None], max_lead_ms=[0, 30, None]) on CPU chunks behind volume_db, sample 1 ending early: per
    sample index the delivered chunks, concatenated, are shorten() of level_host of the concatenated input, bit for bit; the index with
    neither cap passes as the level stage delivers it; a put that releases nothing delivers nothing"""
    from vibevoice_amd.level import level_host
    rate, seg = 24000, 240
    x = np.stack([_bursts(rate, [14, 3, 25], seed=10 + i, burst=3)[:48 * seg + 100] for i in range(3)])
    xt = torch.from_numpy(x[:, None, :])
    st = AudioStreamer(3, volume_db=3.0, max_pause_ms=[100, None, None], max_lead_ms=[0, 30, None], timeout=10)
    assert st._stages == [] and st._ps is None and st._pause == ([100.0, None, None], [0.0, 30.0, None], [-50.0] * 3)
    st.put(xt[:, :, :300], torch.tensor([0, 1, 2]))
    st.put(xt[:, :, 300:3200], torch.tensor([0, 1, 2]))
    st.end(torch.tensor([1]))
    st.put(xt[[2, 0], :, 3200:], torch.tensor([2, 0]))
    st.end()
    caps = [(100, 0), (None, 30), (None, None)]
    for idx in range(3):
        n = 3200 if idx == 1 else x.shape[1]
        lv = level_host(torch.from_numpy(x[idx, :n]), 3.0).numpy()
        want, dropped = P.shorten(lv, rate, *caps[idx])
        got = _drain(st, idx)
        assert all(ch.dim() == 2 and ch.shape[0] == 1 and ch.shape[1] > 0 and ch.dtype == torch.float32 for ch in got)
        assert _same(torch.cat(got, dim=-1)[0].numpy(), want), idx
        assert (dropped > 0) == (idx != 2) and (idx != 2 or _same(want, lv))
    st._thread.join(timeout=10)


def test_streamer_without_the_arguments_is_unchanged():
    x = torch.from_numpy(np.random.default_rng(3).uniform(-0.5, 0.5, (2, 1, 6400)).astype(np.float32))
    a, b = AudioStreamer(2, timeout=10), AudioStreamer(2, timeout=10, max_pause_ms=[None, None], max_lead_ms=None)
    assert b._pause is None and b._ps is None and b._stages == [] and a._pause is None
    for st in (a, b):
        st.put(x[:, :, :3200], torch.tensor([0, 1]))
        st.put(x[:, :, 3200:], torch.tensor([0, 1]))
        st.end()
    for idx in range(2):
        u, v = _drain(a, idx), _drain(b, idx)
        assert len(u) == len(v) == 2 and all(torch.equal(p, q) for p, q in zip(u, v))


def test_streamer_arguments():
    import asyncio
    import inspect
    for name in ("max_pause_ms", "max_lead_ms", "pause_threshold_db"):
        assert name in inspect.signature(AsyncAudioStreamer.__init__).parameters
        assert name in inspect.signature(AudioStreamer.__init__).parameters

    async def run():
        st = AsyncAudioStreamer(1, max_pause_ms=100, max_lead_ms=0)
        x = torch.from_numpy(_bursts(24000, [20, 30], seed=12)[None, None, :])
        st.put(x, torch.tensor([0]))
        st.end()
        got = [ch async for ch in st.get_stream(0)]
        return x, got
    x, got = asyncio.run(run())
    want, dropped = P.shorten(x[0, 0].numpy(), 24000, 100, 0)
    assert dropped == 40 * 240 and _same(torch.cat(got, dim=-1)[0].numpy(), want)
