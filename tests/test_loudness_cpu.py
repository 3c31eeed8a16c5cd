"""CPU tests of the loudness definition (vibevoice_amd/loudness.py: measure_ref, segment_energies_ref, leveller_ref, HostLoudness) and of
AudioStreamer(loudness_lufs=...) on CPU chunks.  The device kernels are held to the same definition, bit for bit, in
test_gpu_loudness.py.

The meter is held to an independent float64 BS.1770-4 meter written here (the two biquads run as IIR filters, the standard's 400 ms
blocks and gates, no quantisation, no FIR cut) within 0.01 LU.  Largest deviation seen over the signals of
test_meter_against_an_independent_float64_meter: 1.6e-3 LU, the 8 kHz sine at -60 LUFS (the table is in that test's docstring);
1e-4 LU and less from -40 LUFS up.  Everything about the leveller is an equality of bits or of integers."""
import math

import numpy as np
import pytest
import torch

from vibevoice_amd import level as V
from vibevoice_amd import loudness as L
from vibevoice_amd import resample as R
from vibevoice_amd import tempo as T
from vibevoice_amd.streamer import AsyncAudioStreamer, AudioStreamer

FIVE = 5 * 24000


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _sine(f, amp, n=FIVE):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / 24000.0)).astype(np.float32)


def _speech(seed, n, amp=0.1):
    """seeded noise under a slow envelope: its loudness moves, so does the leveller's gain"""
    rng = np.random.default_rng(seed)
    env = 1.0 + 0.7 * np.sin(2 * np.pi * np.arange(n) / 11000.0 + seed)
    return (amp * env * rng.standard_normal(n)).astype(np.float32)


def _bilinear(num, den, K):
    """(b, a), a[0] = 1, of the analogue biquad (num[0] s^2 + num[1] s + num[2]) / (den[0] s^2 + den[1] s + den[2]), s in units of the
    corner frequency, through s = (1 - z^-1) / (K (1 + z^-1)), K = tan(pi f0 / rate): the generic substitution, written out here"""
    def poly(c):
        c2, c1, c0 = c[0], c[1] * K, c[2] * K * K                 # times K^2 (1 + z^-1)^2
        return np.array([c2 + c1 + c0, 2.0 * (c0 - c2), c2 - c1 + c0])
    b, a = poly(num), poly(den)
    return b / a[0], a / a[0]


def _coefficients(rate):
    """the test's own pre-filter from the analogue parameters: shelf (Vh s^2 + Vb s / Q + 1) / (s^2 + s / Q + 1), Vb = Vh^0.49967,
    and the high-pass s^2 / (s^2 + s / Q + 1) with its numerator left at (1, -2, 1) as the standard prints it"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    Vh = 10.0 ** (G / 20.0)
    shelf = _bilinear((Vh, Vh ** 0.4996667741545416 / Q, 1.0), (1.0, 1.0 / Q, 1.0), math.tan(math.pi * f0 / rate))
    f0, Q = 38.13547087602444, 0.5003270373238773
    _, ha = _bilinear((1.0, 0.0, 0.0), (1.0, 1.0 / Q, 1.0), math.tan(math.pi * f0 / rate))
    return shelf, (np.array([1.0, -2.0, 1.0]), ha)


def _iir(b, a, x):
    """one biquad run as the direct-form-I recurrence over Python floats"""
    b0, b1, b2, a1, a2 = (float(v) for v in (b[0], b[1], b[2], a[1], a[2]))
    x1 = x2 = y1 = y2 = 0.0
    out = [0.0] * len(x)
    for i, v in enumerate(x.tolist()):
        y = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, v, y1, y
        out[i] = y
    return np.array(out)


def _meter64(x, rate=24000):
    """BS.1770-4 in float64, independent of the module: its own coefficients, the two biquads run as IIR filters"""
    (sb, sa), (hb, ha) = _coefficients(rate)
    y = _iir(hb, ha, _iir(sb, sa, np.asarray(x, dtype=np.float64)))
    blk, hop = int(0.4 * rate), int(0.1 * rate)
    ms = np.array([np.mean(y[i:i + blk] ** 2) for i in range(0, y.shape[0] - blk + 1, hop)])
    if ms.size == 0:
        return -math.inf
    lk = -0.691 + 10 * np.log10(np.maximum(ms, 1e-300))
    ms = ms[lk > -70.0]
    if ms.size == 0:
        return -math.inf
    rel = -0.691 + 10 * np.log10(ms.mean()) - 10.0
    ms = ms[-0.691 + 10 * np.log10(ms) > rel]
    return -0.691 + 10 * np.log10(ms.mean())


def test_coefficients_at_48k_are_the_standards():
    """the module's formula and the test meter's own substitution both give the standard's printed coefficients at 48 kHz, and each
    other at 24 kHz"""
    for (sb, sa), (hb, ha) in (L.biquads(48000), _coefficients(48000)):
        assert np.allclose(sb, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=5e-15)
        assert np.allclose(sa, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=5e-15)
        assert np.array_equal(hb, [1.0, -2.0, 1.0])
        assert np.allclose(ha, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=5e-15)
    for mine, theirs in zip(_coefficients(24000), L.biquads(24000)):
        assert np.allclose(mine[0], theirs[0], rtol=0, atol=1e-14) and np.allclose(mine[1], theirs[1], rtol=0, atol=1e-14)


def test_taps_and_constants():
    h, hq = L.impulse_response(), L.taps()
    assert hq.dtype == np.int32 and hq.shape == (L.T,) == (2400,) and L.S == 2400 and L.history() == 2399 and L.push_width() == 3200
    assert abs(np.abs(h).sum() - 3.2494) < 1e-4 and abs(np.abs(h).max() - 1.4879) < 1e-4
    assert np.abs(L.impulse_response(40000)[L.T:]).sum() < 1e-9          # what the cut drops
    assert np.array_equal(hq, np.rint(h * 2.0 ** 24))
    assert L.EG == math.floor(2400 * 2 ** 32 * 10 ** ((-50 + 0.691) / 10)) and L.counts(77, 5) == (77, 5) and L.counts(77, 0, True) == (77, 0)
    assert L.WMIN == np.float32(10 ** -1.2) and L.target_of(-16).dtype == np.float32 == L.start_of(0).dtype == L.boost_of(12).dtype


_BASE = {}


def _base(name):
    if not _BASE:
        rng = np.random.default_rng(7)
        _BASE.update({"997": _sine(997.0, 0.5), "60": _sine(60.0, 0.5), "8k": _sine(8000.0, 0.5),
                      "noise": (0.1 * rng.standard_normal(FIVE)).astype(np.float32)})
        _BASE["at"] = {k: _meter64(v) for k, v in _BASE.items()}
    return _BASE[name], _BASE["at"][name]


@pytest.mark.parametrize("level", [-60.0, -40.0, -23.0, -3.0, 0.0])
@pytest.mark.parametrize("name", ["997", "60", "8k", "noise"])
def test_meter_against_an_independent_float64_meter(name, level):
    """5 s sines at 997 Hz, 60 Hz and 8 kHz and seeded Gaussian noise, each scaled to read -60, -40, -23, -3 and 0 LUFS: measure_ref agrees
    with the float64 meter within 0.01 LU.

    Measured deviations (measure_ref - float64 meter, LU), at -60 / -40 / -23 / -3 / 0 LUFS:
        997 Hz   -4.6e-5  -2.1e-6  -4.3e-6  -5.5e-6  -5.5e-6
        60 Hz    +1.4e-4  -4.5e-5  +3.5e-6  +3.6e-6  +3.9e-6
        8 kHz    +1.6e-3  +6.1e-5  +6.6e-5  -2.4e-7  +1.1e-6
        noise    +4.6e-6  +1.0e-6  -1.5e-7  -1.5e-7  -1.4e-7
    The meter reads the fine energies F = sum (z >> 24)^2.  From the leveller's E = sum (z >> 28)^2 the 8 kHz sine at -60 LUFS read
    0.0186 LU high and missed this bound: at 24 kHz it has a period of exactly three samples, so the filtered signal takes three
    values, about +-56 units of 2^-16 at that level, and the floor moves each by the same fraction of a unit in every period instead
    of averaging out."""
    x, at = _base(name)
    y = (x.astype(np.float64) * 10 ** ((level - at) / 20)).astype(np.float32)
    assert np.abs(y).max() < 8.0                                         # inside the clamp
    want, got = _meter64(y), L.measure_ref(y)
    print(f"{name} at {level} LUFS: measure_ref - float64 meter = {got - want:+.2e} LU")
    assert abs(want - level) < 0.01
    assert abs(got - want) <= 0.01, (name, level, got, want)


def test_anchors():
    assert abs(L.measure_ref(_sine(997.0, 1.0)) - (-2.984)) < 5e-4          # -3.01 at 48 kHz; the bilinear shelf moves it at 24 kHz
    assert L.measure_ref(np.zeros(FIVE, dtype=np.float32)) == -math.inf
    assert L.measure_ref(_sine(997.0, 0.5, 7200)) == -math.inf and L.measure_ref(_speech(1, 7200)) == -math.inf     # 300 ms
    assert L.measure_ref(_sine(997.0, 0.5, 9600)) > -20.0                   # 400 ms: one block
    assert L.segment_energies_ref(np.zeros(2399)).shape == (0,) and L.segment_energies_ref(np.zeros(2400)).tolist() == [0]
    # the fine energies are the coarse ones at 256 times the scale, up to the floors: |zf / 16 - zs| < 1 per sample
    sp = _speech(12, 4800, amp=0.01)
    E, F = L.segment_energies_ref(sp), L.segment_energies_ref(sp, fine=True)
    assert F.dtype == np.int64 and F.shape == E.shape == (2,) and (np.abs(F / 256.0 / E - 1.0) < 0.02).all() and (F != 256 * E).all()
    assert L.gated([10 ** 9] * 4) == L.gated([256 * 10 ** 9] * 4, fine=True)
    # a loud passage beside one 20 LU quieter reads as the loud one alone: the relative gate drops the quiet blocks.  Of the 30 blocks
    # it keeps, 27 are loud and the three across the seam hold 75, 50 and 25 % of it: 10 log10(28.5 / 30) = -0.22 LU; without the
    # gate the 57 blocks would read 10 log10(28.5 / 57) = -3 LU
    loud = _sine(997.0, 0.3, 3 * 24000)
    both = np.concatenate([loud, loud * np.float32(0.1)])
    diff = L.measure_ref(both) - L.measure_ref(loud)
    assert abs(diff - 10 * math.log10(28.5 / 30)) < 0.01 and abs(L.measure_ref(both) - _meter64(both)) < 0.01
    assert L.measure_ref(loud * np.float32(0.1)) < L.measure_ref(loud) - 19.9


def test_steady_sine_settles_on_one_gain_and_the_target():
    """a 1 kHz sine of amplitude 0.1 (24 samples a period, 100 periods a segment) for 5 s towards -16 LUFS"""
    x = _sine(1000.0, 0.1)
    E = L.segment_energies_ref(x)
    assert len(E) == 50 and len(set(E[1:].tolist())) == 1 and E[0] != E[1]
    y, a = L.leveller_ref(x, -16.0, return_gain=True)
    assert (a[:4 * L.S + 1] == 1.0).all()
    w = a[31 * L.S]
    assert (a[31 * L.S:] == w).all() and w > 2.0                            # one constant from segment 31 on
    assert _same(y[31 * L.S:], w * x[31 * L.S:])                            # fl(w x) bit for bit
    settled = L.measure_ref(y[84000:])
    print(f"behind 3.5 s: {settled:.5f} LUFS")
    assert abs(settled - (-16.0)) <= 0.001


def test_bounds_of_the_leveller():
    x = _speech(2, 3 * 24000, amp=0.05)
    for start in (-24.0, 0.0, 7.5, 24.0):
        a = L.leveller_ref(x, -20.0, start, return_gain=True)[1]
        assert (a[:4 * L.S + 1] == L.start_of(start)).all() and a[5 * L.S] != L.start_of(start)     # start_db holds until 4 segments count
    # the gain never leaves [wmin, wmax], and reaches both
    a = L.leveller_ref(x * np.float32(0.1), -10.0, 0.0, 6.0, return_gain=True)[1]      # about -46 LUFS: over the segment gate
    assert a.max() == L.boost_of(6.0) and a.min() >= L.WMIN
    a = L.leveller_ref(_speech(3, 3 * 24000, amp=1.5), -36.0, 0.0, 0.0, return_gain=True)[1]
    assert a.min() == L.WMIN and a.max() <= 1.0
    # segments under the gate do not move it: 2 s of silence in the middle of speech leave w where it was
    sp = _speech(4, 2 * 24000)
    gap = np.concatenate([sp, np.zeros(2 * 24000, dtype=np.float32), sp])
    a = L.leveller_ref(gap, -18.0, return_gain=True)[1]
    hold = a[2 * 24000 + 2 * L.S:4 * 24000]                                 # behind the ramp of the last counted segment
    assert (hold == hold[0]).all() and hold[0] != 1.0
    faint = np.concatenate([sp, sp[:24000] * np.float32(1e-3), sp])         # -60 dB: under the -50 LUFS segment gate
    a = L.leveller_ref(faint, -18.0, return_gain=True)[1]
    hold = a[2 * 24000 + 2 * L.S:3 * 24000]
    assert (hold == hold[0]).all()
    # a louder speaker brings the gain down within 400 ms (M4), the way back takes the slow mean
    step = np.concatenate([sp * np.float32(0.25), sp])
    a = L.leveller_ref(step, -18.0, return_gain=True)[1]
    before, after = a[2 * 24000 - 1], a[2 * 24000 + 6 * L.S]
    assert after < 0.4 * before


def test_the_worst_case_stays_inside_the_bound():
    """x = +-8 in the sign pattern of the reversed taps: at every T-th sample all 2400 products have one sign.  No product or sum of the
    definition passes 2^49 and E stays below 2^54; the float64 evaluation equals Python integers"""
    hq = L.taps().astype(np.int64)
    x = np.tile(np.where(hq[::-1] < 0, -8.0, 8.0).astype(np.float32), 3)
    xq = L.quantise(x)
    assert np.abs(xq).max() == 2 ** 23
    peak = sum(abs(int(h)) * 2 ** 23 for h in hq)
    assert 2 ** 48 < peak < 2 ** 49
    z = L._fir(np.concatenate([np.zeros(L.T - 1, dtype=np.int64), xq]))
    assert int(np.abs(z).max()) == peak == abs(int(z[L.T - 1]))
    for i in (0, 1, L.T - 1, L.T, 2 * L.T - 1, 3 * L.T - 1):                # exact: Python integers
        assert int(z[i]) == sum(int(hq[k]) * int(xq[i - k]) for k in range(min(i + 1, L.T)))
    partial = np.cumsum(hq * xq[L.T - 1::-1][:L.T])                         # the partial sums in tap order
    assert int(np.abs(partial).max()) < 2 ** 49
    E, F = L.segment_energies_ref(x), L.segment_energies_ref(x, fine=True)
    assert int(np.abs(z >> 28).max()) < 2 ** 21 and 0 < int(E.max()) < 2 ** 54
    assert int(np.abs(z >> 24).max()) < 2 ** 25 and 0 < int(F.max()) < 2 ** 62 and all(int(f) > 0 for f in F)      # no int64 wrap
    assert L.quantise(np.array([np.nan, np.inf, -np.inf, 9.0, -100.0, 2.0 ** -21, 3 * 2.0 ** -21], dtype=np.float32)).tolist() == \
        [0, 0, 0, 2 ** 23, -2 ** 23, 0, 2]                                  # non-finite: 0; clamp; ties to even


def test_host_loudness_is_cut_invariant():
    """a 2 s signal pushed in cuts of 1, 17, 2399, 2400, 2401 and 3200 samples and in 60 random cuts equals the one-shot bit for bit,
    output and gain; a push after the flush raises; reset restores"""
    x = _speech(5, 2 * 24000)
    x[1000], x[30000] = np.nan, np.inf
    want, gain = L.leveller_ref(x, -19.0, 2.0, 10.0, return_gain=True)
    assert gain[-1] != gain[0]
    assert _same(L.loudness_host(x, -19.0, 2.0, 10.0).numpy(), want)
    h = L.HostLoudness(-19.0, 2.0, 10.0)
    for cut in (1, 17, 2399, 2400, 2401, 3200):                             # 1: 48000 pushes, every segment closes on a push of its own
        h.reset()
        got, gg = zip(*[h.push(torch.from_numpy(x[a:a + cut]), return_gain=True) for a in range(0, x.shape[0], cut)])
        assert h.counts(5) == (x.shape[0], 5) and h.flush().shape == (0,)
        assert _same(torch.cat(got).numpy(), want) and _same(torch.cat(gg).numpy(), gain), cut
        assert h.energies == L.segment_energies_ref(x).tolist()
    rng = np.random.default_rng(11)
    for trial in range(2):
        edges = [0] + sorted(rng.integers(0, x.shape[0], 59).tolist()) + [x.shape[0]]
        h.reset()
        got, gg = zip(*[h.push(torch.from_numpy(x[a:b]), return_gain=True) for a, b in zip(edges[:-1], edges[1:])])
        assert len(got) == 60 and _same(torch.cat(got).numpy(), want) and _same(torch.cat(gg).numpy(), gain)
    h.flush()
    with pytest.raises(RuntimeError, match="flushed"):
        h.push(torch.zeros(10))
    h.reset()
    assert h.total_in == 0 and _same(h.push(torch.from_numpy(x), flush=True).numpy(), want)


@pytest.mark.parametrize("name,bad", [("target_lufs", -36.5), ("target_lufs", -9.9), ("target_lufs", float("nan")),
                                      ("start_db", -24.5), ("start_db", 24.1), ("start_db", float("nan")),
                                      ("max_boost_db", -0.1), ("max_boost_db", 24.5), ("max_boost_db", float("nan"))])
def test_parameters_out_of_range_are_refused_by_name(name, bad):
    kw = {"target_lufs": -16.0, "start_db": 0.0, "max_boost_db": 12.0, name: bad}
    skw = {"loudness_lufs": kw["target_lufs"], "loudness_start_db": kw["start_db"], "max_boost_db": kw["max_boost_db"]}
    for call in (lambda: L.leveller_ref(np.zeros(10), **kw), lambda: L.HostLoudness(**kw), lambda: L.loudness_host(np.zeros(10), **kw),
                 lambda: AudioStreamer(1, **skw)):
        with pytest.raises(ValueError, match=name):
            call()


def test_other_refusals():
    for call in (lambda: L.HostLoudness(-16.0, rate=48000), lambda: L.leveller_ref(np.zeros(10), -16.0, rate=16000),
                 lambda: L.loudness_host(np.zeros(10), -16.0, rate=44100)):
        with pytest.raises(ValueError, match="24000 Hz"):
            call()
    with pytest.raises(ValueError, match="loudness_start_db"):
        AudioStreamer(1, loudness_start_db=3.0)
    with pytest.raises(ValueError, match="max_boost_db"):
        AudioStreamer(1, max_boost_db=6.0)
    with pytest.raises(ValueError, match="one per sample index"):
        AudioStreamer(2, loudness_lufs=[-16.0, -20.0, -23.0])
    with pytest.raises(ValueError, match="one per sample index"):
        AudioStreamer(2, loudness_lufs=-16.0, max_boost_db=[6.0])


def _drain(st, idx):
    return list(st.get_stream(idx))


def _host_chain(x, target, start, boost, speed=None, rate=24000):
    y = L.loudness_host(x, target, start, boost).numpy()
    if speed is not None:
        y = T.stretch_ref(y, speed)
    if rate != 24000:
        y = R.resample_host(y, 24000, rate)
    return V.level_host(y, 0.0, -1.0, rate)


@pytest.mark.parametrize("mode", ["alone", "speed", "48k"])
def test_streamer_loudness_on_cpu_chunks(mode):
    """AudioStreamer(loudness_lufs=[-12, -20], loudness_start_db=[0, 6], max_boost_db=[24, 12]) on CPU chunks, alone, with speed=1.25 and
    with sample_rate=48000, sample 1 ending early: per sample index the delivered chunks, concatenated, are the composition of the host
    stages over the whole signal -- leveller, tempo, resampler, and the level stage the streamer adds at -1 dB -- bit for bit, and no
    sample exceeds that ceiling although the boosted signal does"""
    speed, rate = (1.25 if mode == "speed" else None), (48000 if mode == "48k" else 24000)
    n = 5 * 3200
    xs = np.stack([_speech(6, n, amp=0.12), _speech(7, n, amp=0.03)])
    x = torch.from_numpy(xs[:, None, :])
    tg, sd, mb = [-12.0, -20.0], [0.0, 6.0], [24.0, 12.0]
    st = AudioStreamer(2, loudness_lufs=tg, loudness_start_db=sd, max_boost_db=mb, speed=speed, sample_rate=rate, timeout=10)
    assert st._loud == (tg, sd, mb) and st._level == ([0.0, 0.0], -1.0) and st._stages == []
    st.put(x[:, :, :100], torch.tensor([0, 1]))
    for k in range(3):
        st.put(x[:, :, 100 + k * 3200:100 + (k + 1) * 3200], torch.tensor([0, 1]))
    st.end(torch.tensor([1]))
    st.put(x[:1, :, 100 + 3 * 3200:], torch.tensor([0]))
    st.end()
    c = float(V.ceiling_of(-1.0))
    for idx, m in ((0, n), (1, 100 + 3 * 3200)):
        got = torch.cat(_drain(st, idx), dim=-1)[0]
        want = _host_chain(xs[idx, :m], tg[idx], sd[idx], mb[idx], speed, rate)
        assert got.dtype == torch.float32 and _same(got.numpy(), want.numpy()), (mode, idx)
        assert float(got.abs().max()) <= c
    assert float(np.abs(L.leveller_ref(xs[0], tg[0], sd[0], mb[0])).max()) > c
    st._thread.join(timeout=10)


def test_streamer_ceiling_given_and_end_without_a_put():
    x = torch.from_numpy(_speech(8, 4 * 3200, amp=0.2)[None, None, :])
    st = AudioStreamer(2, loudness_lufs=-14.0, volume_db=2.0, ceiling_db=-6.0, timeout=10)
    assert st._level == ([2.0, 2.0], -6.0)
    for k in range(4):
        st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0]))
    st.end()
    want = V.level_host(L.loudness_host(x[0, 0], -14.0), 2.0, -6.0)
    got = torch.cat(_drain(st, 0), dim=-1)[0]
    assert _same(got.numpy(), want.numpy()) and float(got.abs().max()) <= float(V.ceiling_of(-6.0))
    assert _drain(st, 1) == []


@pytest.mark.parametrize("kw", [{}, dict(speed=1.25, sample_rate=16000, volume_db=4.0)])
def test_streamer_without_loudness_is_unchanged(kw):
    """without the new arguments: no loudness state anywhere, the very tensors the streamer delivers for a plain put, and with the other
    three stages the composition of their host forms as before"""
    x = torch.from_numpy(_speech(9, 7001, amp=1.2)[None, None, :])
    st = AudioStreamer(1, timeout=10, **kw)
    assert st._loud is None and st._ld is None and not st._ld_host and st._stages == []
    at = 0
    for c in (3200, 1, 3800):
        st.put(x[:, :, at:at + c], torch.tensor([0]))
        at += c
    st.end()
    got = _drain(st, 0)
    if not kw:
        assert st._level is None and len(got) == 3 and all(torch.equal(g, x[0, :, a:b]) for g, (a, b) in zip(got, ((0, 3200), (3200, 3201), (3201, 7001))))
    else:
        want = V.level_host(R.resample_host(T.stretch_ref(x[0, 0].numpy(), 1.25), 24000, 16000), 4.0, -1.0, 16000)
        assert _same(torch.cat(got, dim=-1)[0].numpy(), want.numpy())
    assert not st._ld_host


def test_streamer_arguments():
    import asyncio
    import inspect
    for name in ("loudness_lufs", "loudness_start_db", "max_boost_db"):
        assert name in inspect.signature(AsyncAudioStreamer.__init__).parameters
        assert name in inspect.signature(AudioStreamer.__init__).parameters

    async def run():
        st = AsyncAudioStreamer(1, loudness_lufs=-15.0, loudness_start_db=4.0)
        x = torch.from_numpy(_speech(10, 4 * 3200)[None, None, :])
        for k in range(4):
            st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0]))
        st.end()
        return [c async for c in st.get_stream(0)], x
    chunks, x = asyncio.run(run())
    want = V.level_host(L.loudness_host(x[0, 0], -15.0, 4.0), 0.0, -1.0)
    assert _same(torch.cat(chunks, dim=-1)[0].numpy(), want.numpy())
