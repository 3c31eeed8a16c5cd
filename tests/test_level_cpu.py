"""CPU tests of the level stage's definition (vibevoice_amd/level.py: level_ref, HostLevel, counts) and of
AudioStreamer(volume_db=..., ceiling_db=...) on CPU chunks.  The device kernels are held to the same definition, bit for bit, in
test_gpu_level.py.  Nothing here has a tolerance: the ceiling is an inequality, everything else an equality of bits."""
import numpy as np
import pytest
import torch

from vibevoice_amd import level as V
from vibevoice_amd import resample as R
from vibevoice_amd import tempo as T
from vibevoice_amd.streamer import AsyncAudioStreamer, AudioStreamer


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _voice(seed, n, amp=0.3):
    """seeded noise plus harmonics, peak near amp"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    h = sum(np.sin(2 * np.pi * f * t / 24000.0 + rng.uniform(0, 6.28)) / (j + 1) for j, f in enumerate((110.0, 220.0, 330.0, 455.0)))
    return (amp * (0.35 * h + 0.3 * rng.uniform(-1, 1, n))).astype(np.float32)


def _naive(x, g, c, A, H):
    """the definition, one sample at a time, in Python integers and numpy float32 scalars"""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    g, c = np.float32(g), np.float32(c)
    u = np.zeros(n, dtype=np.float32)
    q = {}
    with np.errstate(all="ignore"):
        for i in range(n):
            v = g * x[i]
            u[i] = v if np.isfinite(v) else np.float32(0.0)
            r = np.float32(1.0) if abs(u[i]) <= c else c / np.abs(u[i])
            q[i] = int(np.floor(r * np.float32(2 ** 20)))
    h = {j: min(q.get(k, 2 ** 20) for k in range(j - H, j + A)) for j in range(-A + 1, n)}
    y, a = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    for i in range(n):
        S = sum(h[j] for j in range(i - A + 1, i + 1))
        a[i] = np.float32(S) / np.float32(A * 2 ** 20)
        y[i] = min(max(a[i] * u[i], -c), c)
    return y, a


def test_parameters():
    assert V.params(24000) == (120, 1200) and V.params(48000) == (240, 2400) and V.params(8000) == (40, 400)
    assert V.params(100) == (1, 5)
    assert V.history(120, 1200) == 1438 and V.delay_samples(120) == 119
    assert V.gain_of(0) == np.float32(1.0) and V.gain_of(6.0) == np.float32(10 ** 0.3) and V.gain_of(6.0).dtype == np.float32
    assert V.ceiling_of(-1.0) == np.float32(10 ** -0.05) and V.ceiling_of(0) == np.float32(1.0)
    with pytest.raises(ValueError, match="500000"):
        V.params(500000)


@pytest.mark.parametrize("A,H", [(1, 0), (1, 3), (2, 5), (5, 2), (7, 16), (8, 8)])
def test_the_vectorised_definition_is_the_definition(A, H):
    """level_ref against the definition evaluated one sample at a time, small windows (powers of two and not), a NaN and an inf inside"""
    rng = np.random.default_rng(A * 100 + H)
    for n in (1, 2, A, H + 2 * A + 3, 97):
        x = (rng.uniform(-1, 1, n) * rng.choice([0.2, 1.0, 3.0], n)).astype(np.float32)
        if n > 40:
            x[17], x[30] = np.nan, np.inf
        for db in (0.0, 7.5, -12.0):
            y, a = V.level_ref(x, db, -1.0, A=A, H=H, return_gain=True)
            wy, wa = _naive(x, V.gain_of(db), V.ceiling_of(-1.0), A, H)
            assert _same(y, wy) and _same(a, wa)


def test_ceiling():
    """peaks near 2 c: no output sample exceeds c, and the limiter did act"""
    for rate, cdb in ((24000, -1.0), (8000, -6.0), (48000, 0.0)):
        c = V.ceiling_of(cdb)
        x = _voice(rate, 9000, amp=2.2 * float(c))
        assert 1.7 * c < np.abs(x).max() < 2.4 * c
        y, a = V.level_ref(x, 0.0, cdb, rate, return_gain=True)
        assert y.dtype == np.float32 and y.shape == x.shape
        assert np.abs(y).max() <= c and a.min() < 0.6 and a.max() <= 1.0
    x = _voice(2, 5000, amp=0.25)
    assert np.abs(V.level_ref(x, 18.0, -3.0)).max() <= V.ceiling_of(-3.0) < np.abs(V.gain_of(18.0) * x).max()


def test_passthrough():
    """g * peak below c: y = fl(g x) bit for bit, a = 1 exactly; at 0 dB the input itself"""
    x = _voice(3, 7001, amp=0.3)
    x[10], x[11] = -0.0, 1e-41                                 # a negative zero and a denormal survive
    y, a = V.level_ref(x, 0.0, return_gain=True)
    assert _same(y, x) and np.all(a == np.float32(1.0))
    g = V.gain_of(6.0)
    assert np.abs(g * x).max() < V.ceiling_of(-1.0)
    assert _same(V.level_ref(x, 6.0), g * x)
    assert _same(V.level_ref(x, -17.0), V.gain_of(-17.0) * x)
    assert V.level_ref(np.zeros(0)).shape == (0,)


def test_steady_tone_sees_one_gain():
    """a sine of period 160 at amplitude 2 c, A = 120, H = 1200: away from the ends a is the one value the peak sample asks for"""
    c = V.ceiling_of(-1.0)
    n, A, H = 12000, 120, 1200
    x = (np.float32(2.0) * c * np.sin(2 * np.pi * np.arange(n) / 160.0)).astype(np.float32)
    peak = np.abs(x).max()
    y, a = V.level_ref(x, 0.0, -1.0, 24000, return_gain=True)
    q = int(np.floor(np.float32(c / peak) * np.float32(2 ** 20)))
    want = np.float32(np.float32(A * q) / np.float32(A * 2 ** 20))
    mid = a[H + 2 * A:n - (H + 2 * A)]
    assert mid.shape[0] > 9000 and np.all(mid == want) and 0.49 < want < 0.51
    assert _same(y[H + 2 * A:n - (H + 2 * A)], want * x[H + 2 * A:n - (H + 2 * A)])
    assert a[0] > want and a[-1] == want                       # the gain comes down into the tone; the hold outlasts its end


def _cuts(rng, n, A):
    special = [0, 1, max(A - 2, 0), A - 1, A, 3200, 0]
    cuts, at = [], 0
    while at < n:
        c = special.pop(0) if special else int(rng.integers(0, 900))
        c = min(c, n - at)
        cuts.append(c)
        at += c
    return cuts


@pytest.mark.parametrize("rate,db", [(24000, 0.0), (24000, 9.0), (8000, -3.0), (48000, 14.0)])
def test_host_stream_is_chunk_invariant(rate, db):
    """HostLevel over cuts of 0, 1, A - 2, A - 1, A, 3200 and random widths equals level_ref bit for bit, and counts() is what every
    push emitted"""
    A, H = V.params(rate)
    rng = np.random.default_rng(rate)
    n = 9001
    x = _voice(rate + 1, n, amp=1.1)
    x[4000:4003] = 0.0
    want = V.level_ref(x, db, -1.0, rate)
    h = V.HostLevel(db, -1.0, rate)
    assert (h.A, h.H, h.delay_samples) == (A, H, A - 1)
    got, at = [], 0
    for c in _cuts(rng, n, A):
        exp = V.counts(A, at, c)
        assert exp == h.counts(c) == (max(0, at - (A - 1)), max(0, at + c - (A - 1)) - max(0, at - (A - 1)))
        y = h.push(torch.from_numpy(x[at:at + c]))
        assert y.dtype == torch.float32 and y.shape == (exp[1],)
        got.append(y)
        at += c
        assert h.total_in == at and sum(g.shape[0] for g in got) == V.emitted(at, A)
    assert V.counts(A, n, 0, True) == (n - (A - 1), A - 1)
    got.append(h.flush())
    assert _same(torch.cat(got).numpy(), want)
    assert _same(V.level_host(x, db, -1.0, rate).numpy(), want)
    with pytest.raises(RuntimeError, match="flushed"):
        h.push(torch.zeros(1))
    h.reset()
    assert _same(h.push(torch.from_numpy(x), flush=True).numpy(), want)


def test_flush_with_no_push_before_it_and_short_streams():
    h = V.HostLevel(3.0)
    assert h.flush().shape == (0,)
    with pytest.raises(RuntimeError, match="flushed"):
        h.flush()
    for n in (1, 118, 119, 120, 121):
        x = _voice(n, n, amp=1.5)
        h = V.HostLevel(3.0)
        first = h.push(torch.from_numpy(x))
        assert first.shape == (max(0, n - 119),)
        assert _same(torch.cat([first, h.flush()]).numpy(), V.level_ref(x, 3.0))


@pytest.mark.parametrize("bad", [float("nan"), -40.5, 24.01, float("inf"), -1000.0])
def test_volumes_outside_the_range_are_refused_by_name(bad):
    for call in (lambda: V.gain_of(bad), lambda: V.level_ref(np.zeros(10), bad), lambda: V.HostLevel(bad), lambda: AudioStreamer(1, volume_db=bad),
                 lambda: AudioStreamer(2, volume_db=[0.0, bad])):
        with pytest.raises(ValueError, match="nan" if bad != bad else str(bad).replace("-", r"\-").replace(".", r"\.")):
            call()


@pytest.mark.parametrize("bad", [float("nan"), 0.5, -20.5, float("-inf")])
def test_ceilings_outside_the_range_are_refused_by_name(bad):
    for call in (lambda: V.ceiling_of(bad), lambda: V.level_ref(np.zeros(10), 0.0, bad), lambda: V.HostLevel(0.0, bad),
                 lambda: AudioStreamer(1, ceiling_db=bad)):
        with pytest.raises(ValueError, match="nan" if bad != bad else str(bad).replace("-", r"\-").replace(".", r"\.")):
            call()


def _drain(st, idx):
    return list(st.get_stream(idx))


def test_streamer_level_on_cpu_chunks():
    """AudioStreamer(volume_db=[0, 12], ceiling_db=-2) on CPU chunks, sample 1 ending early: per sample index the delivered chunks,
    concatenated, are level_host of the concatenated input, bit for bit; the index at 0 dB still gets the limiter"""
    x = torch.from_numpy(np.stack([_voice(3, 4 * 3200, amp=1.6), _voice(4, 4 * 3200, amp=0.4)])[:, None, :])
    st = AudioStreamer(2, volume_db=[0.0, 12.0], ceiling_db=-2.0, timeout=10)
    st.put(x[:, :, :100], torch.tensor([0, 1]))                           # fewer than A - 1 samples: nothing leaves
    st.put(x[:, :, 100:3200], torch.tensor([0, 1]))
    st.put(x[[1, 0], :, 3200:6400], torch.tensor([1, 0]))
    st.end(torch.tensor([1]))
    st.put(x[:1, :, 6400:], torch.tensor([0]))
    st.end()
    for idx, n, db in ((0, 4 * 3200, 0.0), (1, 2 * 3200, 12.0)):
        chunks = _drain(st, idx)
        want = V.level_host(x[idx, 0, :n], db, -2.0)
        assert all(c.dim() == 2 and c.shape[0] == 1 and c.dtype == torch.float32 and c.shape[1] > 0 for c in chunks)
        assert len(chunks) == (4 if idx == 0 else 3)                       # its puts less the first, which delivered nothing, and the tail
        got = torch.cat(chunks, dim=-1)[0]
        assert _same(got.numpy(), want.numpy()) and got.shape == (n,)
        assert got.abs().max() <= float(V.ceiling_of(-2.0)) < (x[idx, 0, :n] * float(V.gain_of(db))).abs().max()
    st._thread.join(timeout=10)


def test_streamer_level_behind_speed_and_rate_on_cpu_chunks():
    x = torch.from_numpy(_voice(5, 7001, amp=1.2)[None, None, :])
    st = AudioStreamer(1, speed=1.25, sample_rate=16000, volume_db=4.0, timeout=10)
    assert st._level == ([4.0], -1.0)
    at = 0
    for c in (3200, 1, 3800):
        st.put(x[:, :, at:at + c], torch.tensor([0]))
        at += c
    st.end()
    want = V.level_host(R.resample_host(T.stretch_ref(x[0, 0].numpy(), 1.25), 24000, 16000), 4.0, -1.0, 16000)
    assert _same(torch.cat(_drain(st, 0), dim=-1)[0].numpy(), want.numpy())
    assert st._lv_host[0].A == 80


def test_streamer_ceiling_alone_and_end_without_a_put():
    x = torch.from_numpy(_voice(6, 3200, amp=1.4)[None, None, :])
    st = AudioStreamer(2, ceiling_db=-1.0, timeout=10)
    st.put(x, torch.tensor([0]))
    st.end()
    assert _same(torch.cat(_drain(st, 0), dim=-1)[0].numpy(), V.level_ref(x[0, 0].numpy()))
    assert _drain(st, 1) == []


@pytest.mark.parametrize("volume", [None, 0, 0.0, [0.0, 0.0]])
def test_streamer_without_a_level_is_unchanged(volume):
    """no volume, or 0 dB, and no ceiling: the very tensors the streamer delivers without the keywords, and no level stage anywhere"""
    x = torch.from_numpy(np.random.default_rng(3).uniform(-2, 2, (2, 1, 6400)).astype(np.float32)).to(torch.bfloat16)
    a, b = AudioStreamer(2, timeout=10), AudioStreamer(2, timeout=10, volume_db=volume)
    assert b._level is None and b._lv is None and b._stages == []
    for st in (a, b):
        st.put(x[:, :, :3200], torch.tensor([0, 1]))
        st.put(x[:, :, 3200:], torch.tensor([1, 0]))
        st.end()
    for idx in range(2):
        ca, cb = _drain(a, idx), _drain(b, idx)
        assert len(ca) == len(cb) == 2
        for u, v in zip(ca, cb):
            assert u.dtype == v.dtype == torch.bfloat16 and u.shape == v.shape == (1, 3200) and torch.equal(u, v)
    assert not b._lv_host


def test_streamer_arguments():
    import asyncio
    import inspect
    for name in ("volume_db", "ceiling_db"):
        assert name in inspect.signature(AsyncAudioStreamer.__init__).parameters
    with pytest.raises(ValueError, match="one per sample index"):
        AudioStreamer(2, volume_db=[1.0, 2.0, 3.0])

    async def run():
        st = AsyncAudioStreamer(1, volume_db=10.0, ceiling_db=-3.0)
        x = torch.from_numpy(_voice(6, 3200, amp=0.8)[None, None, :])
        st.put(x, torch.tensor([0]))
        st.end()
        return [c async for c in st.get_stream(0)], x
    chunks, x = asyncio.run(run())
    assert _same(torch.cat(chunks, dim=-1)[0].numpy(), V.level_ref(x[0, 0].numpy(), 10.0, -3.0))
