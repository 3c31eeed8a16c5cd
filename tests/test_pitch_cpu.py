"""CPU tests of the pitch stage's definition (vibevoice_amd/pitch.py: ratio, pitch_ref, shift_ref, HostPitch, counts) and of
AudioStreamer(pitch=...) on CPU chunks.  The device kernels are held to the same definition in test_gpu_pitch.py.

The frequency-response thresholds are the issue's: passband gain within +-0.005 dB over 0.84 of the surviving band, a tone above the
folded Nyquist frequency at <= -78 dB, everything that is not the shifted tone at <= -85 dB; a prototype of this design measured
+-0.0006 dB, -79.8 dB and -90 dB.  The measured values are printed."""
import inspect
import math

import numpy as np
import pytest
import torch

from vibevoice_amd import level as V
from vibevoice_amd import pitch as P
from vibevoice_amd import resample as R
from vibevoice_amd import tempo as T
from vibevoice_amd.streamer import AsyncAudioStreamer, AudioStreamer

RATIOS = [(2, 1), (1, 2), (89, 84), (84, 89), (3, 2), (2, 3), (100, 51), (63, 50)]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _noise(seed, n):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- ratio and refusals
def test_ratio_is_reduced_within_100_and_within_8_71_cents():
    worst = 0.0
    for s in np.arange(-1200, 1201) / 100.0:
        p, q = P.ratio(float(s))
        assert 1 <= p <= 100 and 1 <= q <= 100 and math.gcd(p, q) == 1 and p <= 2 * q and q <= 2 * p
        assert T.ratio(q / p) == (q, p)                         # the tempo stage recovers Q / P exactly
        worst = max(worst, abs(P.cents_off(float(s))))
    whole = max(abs(P.cents_off(float(s))) for s in range(-12, 13))
    print(f"ratio(): worst error over -12..12 in 0.01 steps {worst:.3f} cents; over whole semitones {whole:.3f} cents")
    assert worst <= 8.71
    bound = 600.0 * math.log2(100.0 / 99.0)                      # half way from 1/1 to 100/99: reached next to unison, off the 0.01 grid
    assert bound - 0.01 < abs(P.cents_off(bound / 100.0 - 1e-9)) <= bound < 8.71 and abs(P.cents_off(-bound / 100.0 + 1e-9)) <= bound
    assert P.ratio(0) == P.ratio(0.0) == (1, 1)
    assert P.ratio(1) == (89, 84) and P.ratio(7) == (3, 2) and P.ratio(12) == (2, 1) and P.ratio(-12) == (1, 2)
    assert P.ratio(0.1) == (100, 99) and P.ratio(-0.1) == (99, 100) and P.ratio(6) == (99, 70)     # reduced: never 6 / 4 for 3 / 2


@pytest.mark.parametrize("bad", [float("nan"), -12.01, 12.5, float("inf"), 1000.0])
def test_semitones_outside_the_range_are_refused_by_name(bad):
    for call in (lambda: P.ratio(bad), lambda: P.pitch_ref(np.zeros(10), bad), lambda: P.HostPitch(bad), lambda: P.shift_ref(np.zeros(10), bad),
                 lambda: AudioStreamer(1, pitch=bad), lambda: AudioStreamer(2, pitch=[0.0, bad])):
        with pytest.raises(ValueError, match="nan" if bad != bad else str(bad).replace("-", r"\-").replace(".", r"\.")):
            call()
    with pytest.raises(ValueError, match="semitones"):
        P.ratio("high")


def test_a_combined_speed_outside_the_tempo_range_is_refused_naming_both():
    for speed, semis in ((2.0, -7.0), (0.5, 3.0), (0.9, 12.0)):
        for call in (lambda: P.tempo_speed(speed, semis), lambda: P.shift_ref(np.zeros(4000), semis, speed),
                     lambda: AudioStreamer(1, pitch=semis, speed=speed), lambda: AudioStreamer(2, pitch=[0.0, semis], speed=[1.0, speed])):
            with pytest.raises(ValueError, match=rf"speed={speed}.*semitones={semis}"):
                call()
    assert P.tempo_speed(1.0, 12.0) == 0.5 and P.tempo_speed(1.0, -12.0) == 2.0 and P.tempo_speed(1.5, 7.0) == 1.0


# ------------------------------------------------------------------------------------------------------------- frequency response
def _fit(y, freqs, trim=1500):
    """least-squares sines at `freqs` (cycles per sample) over y less `trim` samples at each end -> (amplitudes, what is left)"""
    m = np.arange(trim, y.shape[0] - trim, dtype=np.float64)
    cols = []
    for f in freqs:
        cols += [np.cos(2.0 * np.pi * f * m), np.sin(2.0 * np.pi * f * m)]
    A = np.stack(cols, axis=1)
    sol, *_ = np.linalg.lstsq(A, y[trim:y.shape[0] - trim], rcond=None)
    rest = y[trim:y.shape[0] - trim] - A @ sol
    return np.hypot(sol[0::2], sol[1::2]), rest


def _db(v):
    return 20.0 * math.log10(max(float(v), 1e-30))


@pytest.mark.parametrize("p,q", RATIOS)
def test_frequency_response_of_the_definition(p, q):
    """12000-sample tones through the definition in float64 over the float32 table, 1500 samples trimmed at each end, least-squares
    sines at the shifted frequencies"""
    n, m = 12000, np.arange(12000, dtype=np.float64)
    band = 0.5 * min(1.0, q / p)                             # input frequencies that survive, cycles per input sample
    assert (P.taps(2, 1), P.taps(1, 2), P.taps(89, 84)) == (64, 32, 34)                  # 129, 65 and 69 taps per output
    fin = [0.84 * band * u for u in (0.11, 0.53, 0.83, 1.0)]
    gain, residue = [], -400.0
    for i, f in enumerate(fin):                              # one tone at a time, as the thresholds were measured
        y = P.resample_ref(np.cos(2.0 * np.pi * f * m + 0.3 * i), p, q)
        assert y.shape == (P.total_out(n, p, q),) and y.dtype == np.float64
        amp, rest = _fit(y, [f * p / q])
        gain.append(_db(amp[0]))
        residue = max(residue, _db(math.sqrt(2.0) * np.sqrt(np.mean(rest * rest))))
    print(f"{p}/{q}: {2 * P.taps(p, q) + 1} taps, passband gain {min(gain):+.5f} .. {max(gain):+.5f} dB, residue {residue:.1f} dB", end="")
    assert max(abs(g) for g in gain) <= 0.005
    assert residue <= -85.0
    if p > q:                                                # the pitch goes up: what lies above the folded Nyquist must not fold back
        worst = -400.0
        for u in (1.0, 1.04, 1.25, 1.0 / (2.0 * band)):
            f = min(band * u, 0.5)
            z = P.resample_ref(np.cos(2.0 * np.pi * f * m + 0.7), p, q)[1500:-1500]
            worst = max(worst, _db(math.sqrt(2.0) * np.sqrt(np.mean(z * z))))
        print(f", above the folded Nyquist {worst:.1f} dB", end="")
        assert worst <= -78.0
    print()


def test_gain_of_the_taps_and_the_unison():
    """A1 = max_a sum_t |rho c| stays where the prototype measured it (2.15 .. 2.32), the table is the symmetric prototype's half, and
    1 / 1 is the identity, bit for bit"""
    H = P.table()
    assert H.shape == (P.Z * P.R + 1,) and H.dtype == np.float32 and not H.flags.writeable
    assert 0.9 < H[0] < 0.93 and abs(H[-1]) < 1e-4
    for p, q in RATIOS:
        den, tn = max(p, q), P.taps(p, q)
        a1 = 0.0
        for a in range(q):
            t = np.arange(-tn, tn + 1)
            pos = np.abs(a + t * q) * P.R / den
            c = np.where(pos < P.Z * P.R, np.interp(pos, np.arange(H.shape[0]), H.astype(np.float64)), 0.0)
            a1 = max(a1, float(np.abs(c).sum() * q / den))
        assert 2.1 <= a1 <= 2.35, (p, q, a1)
    x = _noise(1, 5000)
    assert _same(P.pitch_ref(x, 0.0, dtype=np.float32), x) and _same(P.pitch_host(torch.from_numpy(x), 0.0).numpy(), x)
    assert P.taps(1, 1) == 0 and P.emitted(77, 1, 1) == 77


# ---------------------------------------------------------------------------------------------------- shifted frequency and counts
def test_a_440_hz_sine_comes_out_at_440_p_over_q_and_keeps_its_length():
    n = 24000
    x = (0.5 * np.sin(2.0 * np.pi * 440.0 / 24000.0 * np.arange(n))).astype(np.float32)
    p, q = P.ratio(4)
    for speed in (1.0, 1.25):
        y = P.shift_ref(x, 4, speed)
        pt, qt = T.ratio(speed * q / p)
        assert y.shape == (P.total_out(T.total_out(n, pt, qt), p, q),) == (P.shift_len(n, 4, speed),)
        assert abs(y.shape[0] - n / speed) <= 1 + n * abs(qt / pt - p / (q * speed))
        spec = np.abs(np.fft.rfft(y[2400:-2400] * np.hanning(y.shape[0] - 4800)))
        peak = np.argmax(spec) * 24000.0 / (y.shape[0] - 4800)
        assert abs(peak - 440.0 * p / q) < 24000.0 / (y.shape[0] - 4800), (peak, 440.0 * p / q)
    assert abs(440.0 * p / q - 440.0 * 2 ** (4 / 12)) < 1.0
    # a combined speed of exactly 1: no tempo stage, plain resampling
    assert _same(P.shift_ref(x, 7, 1.5), P.resample_ref(x, 3, 2))
    assert _same(P.shift_ref(x, 0, 1.25, dtype=np.float32), T.stretch_ref(x, 1.25))


def test_counts_agree_with_brute_force_and_hold_beyond_2_pow_32():
    for p, q in RATIOS + [(1, 1), (100, 99), (99, 100)]:
        tn = P.taps(p, q)
        assert tn <= P.MAX_TN and P.delay_samples(p, q) == tn
        for total in list(range(0, 3 * tn + 40)) + [1000, 4097]:
            brute = sum(1 for m in range(0, 2 * total + 4) if (m * p) // q + tn < total)
            assert P.emitted(total, p, q) == brute, (p, q, total)
            assert P.total_out(total, p, q) == sum(1 for m in range(0, 2 * total + 4) if m * p < total * q)
            assert P.emitted(total, p, q) <= P.total_out(total, p, q)
        big = 2 ** 33 + 12345
        m0, k = P.counts(p, q, big, 3200)
        assert m0 == P.emitted(big, p, q) and m0 + k == P.emitted(big + 3200, p, q)
        assert (m0 * p) // q + tn >= big > ((m0 - 1) * p) // q + tn           # m0 is the first output that waits for more input
        assert abs(k - 3200 * q / p) <= 1
        m0f, kf = P.counts(p, q, big, 3200, flush=True)
        assert m0f == m0 and m0f + kf == P.total_out(big + 3200, p, q) == -((-(big + 3200) * q) // p)
    # the width of a push: whole where it fits the kernel, else a piece that does
    assert P.push_width([(2, 1)], [0], [3200]) == 3200
    w = P.push_width([(1, 2)], [0], [7000])
    assert 1 <= w <= P.MAX_IN and P.counts(1, 2, 10 ** 9, w, True)[1] <= P.MAX_OUT
    assert P.push_width([(2, 1)], [0], [9000]) <= P.MAX_IN


# -------------------------------------------------------------------------------------------------------------------- host streaming
@pytest.mark.parametrize("p,q", [(1, 2), (2, 1), (89, 84), (63, 50)])
def test_host_streaming_is_chunk_invariant(p, q):
    semis = 12.0 * math.log2(p / q)
    assert P.ratio(semis) == (p, q)
    tn = P.taps(p, q)
    x = _noise(p * 100 + q, 6000)
    want = P.pitch_host(torch.from_numpy(x), semis)
    assert want.shape == (P.total_out(6000, p, q),) and want.dtype == torch.float32
    ref = P.resample_ref(x, p, q)
    assert np.abs(want.numpy() - ref).max() < 2e-5            # the float32 form against the definition in float64
    rng = np.random.default_rng(7)
    for cuts in ([1, tn - 1, tn, tn + 1, 1, 1, 700], list(rng.integers(1, 900, 9)), [0, 3200, 0, 1]):
        h = P.HostPitch(semis)
        got, at, silent = [], 0, 0
        for c in list(cuts) + [6000]:
            c = min(int(c), 6000 - at)
            assert h.counts(c) == P.counts(p, q, at, c)
            y = h.push(torch.from_numpy(x[at:at + c]))
            assert y.shape == (h.counts(0)[0] - sum(g.shape[0] for g in got),)
            silent += y.shape[0] == 0
            got.append(y)
            at += c
        assert cuts[0] != 1 or silent >= 2                     # the first samples of a stream emit nothing: Tn of them wait
        got.append(h.flush())
        assert _same(torch.cat(got).numpy(), want.numpy())
        with pytest.raises(RuntimeError, match="flushed"):
            h.push(torch.zeros(4))


def _drain(st, idx):
    return list(st.get_stream(idx))


def test_streamer_pitch_on_cpu_chunks_is_the_composition_of_the_definitions():
    x = torch.from_numpy(np.stack([_noise(3, 3 * 3200), _noise(4, 3 * 3200)])[:, None, :] * 0.7)
    st = AudioStreamer(2, pitch=[3.0, 0.0], speed=[1.0, 1.25], sample_rate=16000, volume_db=-3.0, timeout=10)
    p, q = P.ratio(3.0)
    assert st._pitch == [3.0, 0.0] and st._speeds == [q / p, 1.25] and st._stages == []
    st.put(x[:, :, :30], torch.tensor([0, 1]))
    st.put(x[:, :, 30:3200], torch.tensor([0, 1]))
    st.put(x[[1, 0], :, 3200:6400], torch.tensor([1, 0]))
    st.end(torch.tensor([1]))
    st.put(x[:1, :, 6400:], torch.tensor([0]))
    st.end()
    for idx, n, semis, speed in ((0, 3 * 3200, 3.0, 1.0), (1, 2 * 3200, 0.0, 1.25)):
        got = torch.cat(_drain(st, idx), dim=-1)[0]
        y = T.stretch_host(x[idx, 0, :n], P.tempo_speed(speed, semis))
        y = P.pitch_host(y, semis)
        want = V.level_host(R.resample_host(y, 24000, 16000), -3.0, -1.0, 16000)
        assert _same(got.numpy(), want.numpy())
        assert abs(got.shape[0] - n / speed * 16000 / 24000) <= 2 + n * 2e-3
    assert isinstance(st._pt_host[0], P.HostPitch) and (st._pt_host[1].P, st._pt_host[1].Q) == (1, 1)
    st._thread.join(timeout=10)


def test_streamer_speed_and_pitch_that_cancel_build_no_tempo_object():
    x = torch.from_numpy(_noise(5, 7001)[None, None, :])
    st = AudioStreamer(1, speed=1.5, pitch=7.0, timeout=10)
    assert st._speeds is None and st._pitch == [7.0]
    at = 0
    for c in (3200, 1, 3800):
        st.put(x[:, :, at:at + c], torch.tensor([0]))
        at += c
    st.end()
    got = torch.cat(_drain(st, 0), dim=-1)[0]
    assert not st._tp_host and st._tp is None
    assert _same(got.numpy(), P.pitch_host(x[0, 0], 7.0).numpy()) and got.shape == (P.total_out(7001, 3, 2),)


@pytest.mark.parametrize("pitch", [None, 0, 0.0, [0.0, 0.0]])
def test_streamer_without_a_pitch_is_unchanged(pitch):
    x = torch.from_numpy(np.random.default_rng(3).uniform(-2, 2, (2, 1, 6400)).astype(np.float32)).to(torch.bfloat16)
    a, b = AudioStreamer(2, timeout=10), AudioStreamer(2, timeout=10, pitch=pitch)
    assert b._pitch is None and b._pt is None and b._speeds is None and b._stages == []
    for st in (a, b):
        st.put(x[:, :, :3200], torch.tensor([0, 1]))
        st.put(x[:, :, 3200:], torch.tensor([1, 0]))
        st.end()
    for idx in range(2):
        ca, cb = _drain(a, idx), _drain(b, idx)
        assert len(ca) == len(cb) == 2
        for u, v in zip(ca, cb):
            assert u.dtype == v.dtype == torch.bfloat16 and u.shape == v.shape == (1, 3200) and torch.equal(u, v)
    assert not b._pt_host


def test_streamer_arguments():
    import asyncio
    for cls in (AudioStreamer, AsyncAudioStreamer):
        assert "pitch" in inspect.signature(cls.__init__).parameters
    with pytest.raises(ValueError, match="one per sample index"):
        AudioStreamer(2, pitch=[1.0, 2.0, 3.0])

    async def run():
        st = AsyncAudioStreamer(1, pitch=-5.0)
        x = torch.from_numpy(_noise(6, 3200)[None, None, :])
        st.put(x, torch.tensor([0]))
        st.end()
        return [c async for c in st.get_stream(0)], x
    chunks, x = asyncio.run(run())
    y = P.pitch_host(T.stretch_host(x[0, 0], P.tempo_speed(1.0, -5.0)), -5.0)
    assert _same(torch.cat(chunks, dim=-1)[0].numpy(), y.numpy())


def test_the_module_and_the_readme_say_that_formants_move():
    import os
    assert "formants move with the pitch" in P.__doc__.lower()
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    assert "formants move with the pitch" in readme.lower()
