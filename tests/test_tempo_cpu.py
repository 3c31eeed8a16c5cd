"""CPU tests of the tempo stage's definition (vibevoice_amd/tempo.py: stretch_ref, HostTempo, counts) and of AudioStreamer(speed=...)
on CPU chunks.  The device kernels are held to the same definition, offsets included, in test_gpu_tempo.py.

Bounds.  At speed 1 every offset is 0 and y = fl(fl(w[HS + i] x) + fl(w[i] x)) with w[HS + i] + w[i] = 1 up to the table's rounding:
three roundings of magnitudes below 1/2, one fp32 ulp there, 2^-23 = 1.2e-7 (measured 6.0e-8 to 1.2e-7).  A signal of period 160 is
continued exactly by an offset that is a multiple of 160 away, which the search (radius 160, so one such offset always lies inside)
finds because the integer search signal is periodic too: the output's period error is again a rounding or two, 1e-6 is ample (measured
6.0e-8), while plain overlap-add (radius 0) adds segments out of phase: 0.65 to 0.79."""
import numpy as np
import pytest
import torch

from vibevoice_amd import resample as R
from vibevoice_amd import tempo as T
from vibevoice_amd.streamer import AsyncAudioStreamer, AudioStreamer

SPEEDS = [1.25, 0.8, 2.0, 0.5, 1.13]
RATIOS = {1.25: (5, 4), 0.8: (4, 5), 2.0: (2, 1), 0.5: (1, 2), 1.13: (113, 100)}
CUTS = [0, 1, 7, 639, 641, 3200]


def _voice(seed, n, amp=0.3):
    """seeded noise plus harmonics, peak near amp"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    h = sum(np.sin(2 * np.pi * f * t / 24000.0 + rng.uniform(0, 6.28)) / (j + 1) for j, f in enumerate((110.0, 220.0, 330.0, 455.0)))
    return (amp * (0.35 * h + 0.3 * rng.uniform(-1, 1, n))).astype(np.float32)


def _harmonic(n):
    t = np.arange(n)
    return sum(a * np.sin(2 * np.pi * j * t / 160 + ph) for j, (a, ph) in enumerate([(0.3, 0.1), (0.2, 1.0), (0.1, 2.0)], 1)).astype(np.float32)


def _square(n, amp=4.0):
    """a clipped square wave of period 80: the integer search signal is +-32767, exactly periodic"""
    return (amp * np.where((np.arange(n) % 80) < 40, 1.0, -1.0)).astype(np.float32)


def test_constants_and_window():
    assert (T.HS, T.N, T.DELTA, T.delay_samples()) == (240, 480, 160, 640)
    w = T.window()
    assert w.dtype == np.float32 and w.shape == (480,) and w[0] == 0.0 and w[240] == 1.0
    assert np.array_equal(w, (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(480) / 480)).astype(np.float32))
    assert [T.ratio(s) for s in SPEEDS] == [RATIOS[s] for s in SPEEDS] and T.ratio(1) == (1, 1)


@pytest.mark.parametrize("n", [0, 1, 239, 240, 241, 7001])
def test_output_length(n):
    x = _voice(n, n)
    for s in SPEEDS + [1.0]:
        P, Q = T.ratio(s)
        y, offs = T.stretch_ref(x, s, return_offsets=True)
        assert y.dtype == np.float32 and y.shape == (-(-n * Q // P),) == (T.total_out(n, P, Q),)
        assert offs.shape == (-(-y.shape[0] // 240),)


def test_speed_one_is_the_input():
    x = _voice(1, 7001)
    y, offs = T.stretch_ref(x, 1.0, return_offsets=True)
    err = float(np.abs(y - x).max())
    print(f"speed 1: max|y - x| = {err:.3g}")
    assert not offs.any() and err <= 1.2e-7


@pytest.mark.parametrize("speed", SPEEDS)
def test_a_periodic_signal_stays_periodic(speed):
    x = _harmonic(24000)
    y, plain = T.stretch_ref(x, speed), T.stretch_ref(x, speed, radius=0)
    mid = slice(480, y.shape[0] - 1200)                   # away from the zeros in front of and behind the signal
    err, err_plain = (float(np.abs(v[mid][160:] - v[mid][:-160]).max()) for v in (y, plain))
    rms = float(np.sqrt((y[mid].astype(np.float64) ** 2).mean()) / np.sqrt((x.astype(np.float64) ** 2).mean()))
    print(f"speed {speed}: period error {err:.3g} (plain overlap-add {err_plain:.3g}), rms ratio {rms:.5f}")
    assert err <= 1e-6 and err_plain > 0.5


def test_tie_order():
    """all zeros: every ssd is 0, the offset is 0.  The clipped square wave of period 80: every offset that keeps the phase ties at ssd 0,
    four of them inside the radius; the smallest |d| wins, and of +-40 the negative one."""
    for s in SPEEDS:
        assert not T.stretch_ref(np.zeros(3000, dtype=np.float32), s, return_offsets=True)[1].any()
    x = _square(8000)
    assert set(np.unique(T.search_signal(x))) == {-32767, 32767}
    saw_symmetric = False
    for s in SPEEDS:
        P, Q = T.ratio(s)
        _, offs = T.stretch_ref(x, s, return_offsets=True)
        p_prev = -240
        for k, d in enumerate(offs[:-8]):                  # the last blocks see the zeros behind the signal
            a, t = (k * 240 * P) // Q, p_prev + 240
            phase = (t - a) % 80                          # d = phase (mod 80) continues the wave exactly
            best = min(range(phase - 160, 161, 80), key=lambda c: (abs(c), c >= 0))
            assert -160 <= best <= 160 and d == best, (s, k, d, best)
            saw_symmetric |= phase == 40 and d == -40
            p_prev = a + d
    assert saw_symmetric


@pytest.mark.parametrize("speed", SPEEDS)
def test_host_tempo_is_cut_invariant(speed):
    """ragged pushes, every one announced by counts(), and the flush: the reference bit for bit, offsets included; the stream never holds
    back more than 640 samples"""
    x = _voice(2, 9001)
    want, want_offs = T.stretch_ref(x, speed, return_offsets=True)
    P, Q = T.ratio(speed)
    h = T.HostTempo(speed)
    assert h.delay_samples == 640
    got, at, k, emitted = [], 0, 0, 0
    while at < x.shape[0]:
        c = min(CUTS[k % len(CUTS)], x.shape[0] - at)
        k += 1
        o0, cnt = T.counts(P, Q, h.total_in, c)
        assert o0 == emitted and h.counts(c) == (o0, cnt)
        y = h.push(torch.from_numpy(x[at:at + c]))
        assert y.dtype == torch.float32 and y.shape == (cnt,) and cnt % 240 == 0
        got.append(y)
        at += c
        emitted += cnt
        assert 0 <= T.held(h.total_in, P, Q) <= 640 and emitted == T.emitted_blocks(h.total_in, P, Q) * 240
    assert T.counts(P, Q, h.total_in, 0, True) == (emitted, want.shape[0] - emitted)
    got.append(h.flush())
    assert torch.equal(torch.cat(got), torch.from_numpy(want)) and np.array_equal(np.asarray(h.offsets), want_offs)
    assert torch.equal(T.stretch_host(x, speed), torch.from_numpy(want))
    with pytest.raises(RuntimeError, match="flushed"):
        h.push(torch.zeros(1))


def test_emission_rule_and_hold_back():
    """block k leaves with the push that brings total_in to max(a_k, a_{k-1} + HS) + 640, not one sample earlier; below that threshold
    the stream holds back less than 640 samples, whatever the speed"""
    for s in SPEEDS + [1.0, 1.99, 0.51]:
        P, Q = T.ratio(s)
        a = lambda k: (k * 240 * P) // Q if k >= 0 else -240
        for k in range(0, 40):
            need = max(a(k), a(k - 1) + 240) + 640
            assert T.emitted_blocks(need - 1, P, Q) == k and T.emitted_blocks(need, P, Q) >= k + 1
        assert max(T.held(n, P, Q) for n in range(0, 6000)) <= 639
        assert T.counts(P, Q, 0, 639) == (0, 0) and T.counts(P, Q, 0, 640) == (0, 240)


@pytest.mark.parametrize("bad", [0.49, 2.01, 0.0, -1.0, float("nan"), float("inf")])
def test_speeds_outside_the_range_are_refused_by_name(bad):
    for call in (lambda: T.ratio(bad), lambda: T.stretch_ref(np.zeros(10), bad), lambda: T.HostTempo(bad), lambda: AudioStreamer(1, speed=bad),
                 lambda: AudioStreamer(2, speed=[1.0, bad])):
        with pytest.raises(ValueError, match="nan" if bad != bad else str(bad).replace("-", r"\-").replace(".", r"\.")):
            call()


def _drain(st, idx):
    return list(st.get_stream(idx))


def test_streamer_speed_then_16k_on_cpu_chunks():
    """AudioStreamer(speed=[0.8, 1.25], sample_rate=16000) on CPU chunks, sample 1 ending early: per sample index the delivered chunks,
    concatenated, are resample_host(stretch_ref(concatenated input)) bit for bit; a put that completes no block delivers nothing"""
    x = torch.from_numpy(np.stack([_voice(3, 4 * 3200), _voice(4, 4 * 3200)])[:, None, :])
    st = AudioStreamer(2, sample_rate=16000, speed=[0.8, 1.25], timeout=10)
    st.put(x[:, :, :500], torch.tensor([0, 1]))                          # fewer than 640 samples: nothing leaves
    st.put(x[:, :, 500:3200], torch.tensor([0, 1]))
    st.put(x[[1, 0], :, 3200:6400], torch.tensor([1, 0]))
    st.end(torch.tensor([1]))
    st.put(x[:1, :, 6400:], torch.tensor([0]))
    st.end()
    for idx, n, speed in ((0, 4 * 3200, 0.8), (1, 2 * 3200, 1.25)):
        chunks = _drain(st, idx)
        want = R.resample_host(T.stretch_ref(x[idx, 0, :n].numpy(), speed), 24000, 16000)
        assert all(c.dim() == 2 and c.shape[0] == 1 and c.dtype == torch.float32 and c.shape[1] > 0 for c in chunks)
        assert len(chunks) == (4 if idx == 0 else 3)                      # its puts less the first, which delivered nothing, and the tail
        assert torch.equal(torch.cat(chunks, dim=-1)[0], want)
        P, Q = T.ratio(speed)
        assert want.shape[0] == -(-(-(-n * Q // P)) * 2 // 3)
    st._thread.join(timeout=10)


def test_streamer_speed_alone_on_cpu_chunks():
    x = torch.from_numpy(_voice(5, 7001)[None, None, :])
    st = AudioStreamer(1, speed=1.13, timeout=10)
    at = 0
    for c in (3200, 1, 3800):
        st.put(x[:, :, at:at + c], torch.tensor([0]))
        at += c
    st.end()
    chunks = _drain(st, 0)
    assert torch.equal(torch.cat(chunks, dim=-1)[0], torch.from_numpy(T.stretch_ref(x[0, 0].numpy(), 1.13)))


@pytest.mark.parametrize("speed", [None, 1, 1.0, [1.0, 1.0]])
def test_streamer_without_a_speed_is_unchanged(speed):
    """no speed, or 1: the very tensors the streamer delivers without the keyword, and no tempo stage anywhere"""
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, 1, 6400)).astype(np.float32)).to(torch.bfloat16)
    a, b = AudioStreamer(2, timeout=10), AudioStreamer(2, timeout=10, speed=speed)
    assert b._speeds is None and b._tp is None
    for st in (a, b):
        st.put(x[:, :, :3200], torch.tensor([0, 1]))
        st.put(x[:, :, 3200:], torch.tensor([1, 0]))
        st.end()
    for idx in range(2):
        ca, cb = _drain(a, idx), _drain(b, idx)
        assert len(ca) == len(cb) == 2
        for u, v in zip(ca, cb):
            assert u.dtype == v.dtype == torch.bfloat16 and u.shape == v.shape == (1, 3200) and torch.equal(u, v)
    assert not b._tp_host and not b._rs_host


def test_streamer_arguments():
    import asyncio
    import inspect
    assert "speed" in inspect.signature(AsyncAudioStreamer.__init__).parameters
    with pytest.raises(ValueError, match="one per sample index"):
        AudioStreamer(2, speed=[0.8, 1.0, 1.2])

    async def run():
        st = AsyncAudioStreamer(1, speed=0.8)
        x = torch.from_numpy(_voice(6, 3200)[None, None, :])
        st.put(x, torch.tensor([0]))
        st.end()
        return [c async for c in st.get_stream(0)], x
    chunks, x = asyncio.run(run())
    assert torch.equal(torch.cat(chunks, dim=-1)[0], torch.from_numpy(T.stretch_ref(x[0, 0].numpy(), 0.8)))
