"""The formant warp's definition (vibevoice_amd/formant.py) on the CPU: the identity, silence, the counts, chunk invariance of the float32
host form, that the formants move by A / B while the pitch stays, that a warp by Q / P in front of the resampler at P / Q puts the
envelope back, and AudioStreamer(formant=...)'s arithmetic and CPU chunks.  The envelope read-out is formant_util.peaks."""
import numpy as np
import pytest
import torch

from formant_util import FORMANTS, peaks, pulses, vowel
from vibevoice_amd import formant as F
from vibevoice_amd import pitch as P
from vibevoice_amd.level import level_host
from vibevoice_amd.streamer import AudioStreamer, _formant_of
from vibevoice_amd.tempo import stretch_host

WARPS = [(5, 4), (4, 5), (3, 2), (2, 3)]
CUTS = [1, 255, 256, 257, 700, 3200]


def _noise(seed, n, scale=1.0):
    return (np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(np.float32)


def test_identity_and_the_window_sum():
    """1 / 1 returns the input bit for bit (non-finite samples included: nothing is computed); computed through the frames anyway,
    G = 1, float64 reproduces the input to 1e-15 (measured: 1.3e-15 peak at 5000 samples of unit noise, 2.8e-16 rms), so the window
    and the 2/3 scale are right"""
    x = _noise(1, 5000)
    x[17] = np.inf
    for y in (F.warp_host(x, 1, 1).numpy(), F.warp_ref(x, 7, 7)):
        assert np.array_equal(y[np.isfinite(x)], x[np.isfinite(x)]) and y[17] == np.inf
    x = np.random.default_rng(2).uniform(-1, 1, 5000)
    y = F.warp_ref(x, 1, 1, unit_gain=True)
    err = np.abs(y - x)
    print(f"[formant identity through the frames] max {err.max():.2e}, rms {np.sqrt((err ** 2).mean()):.2e}")
    assert y.shape == x.shape and np.sqrt((err ** 2).mean()) <= 1e-15 and err.max() <= 4e-15
    w = F.window(np.float64)
    assert np.abs(sum((w * w)[s * F.H:(s + 1) * F.H] for s in range(4)) - 1.5).max() < 1e-7
    t = F.twiddles()
    assert t.shape == (2, F.N) and t.dtype == np.float32 and not t.flags.writeable and F.twiddles() is t
    assert np.array_equal(t[0], np.cos(2 * np.pi * np.arange(F.N) / F.N).astype(np.float32))


def test_silence_gives_exact_zeros():
    for n in (1, 256, 1000):
        for a, b in WARPS:
            assert not F.warp_ref(np.zeros(n), a, b).any() and not F.warp_ref(np.zeros(n), a, b, table=True).any()
            y = F.warp_host(np.zeros(n, dtype=np.float32), a, b)
            assert y.shape == (n,) and not y.numpy().any()


def test_counts():
    """n samples in, n out; emitted / counts around multiples of 256 and beyond 2^32; a non-finite sample counts as 0"""
    for n in (1, 255, 256, 257, 1023, 1024, 1025, 5000):
        x = _noise(n, n)
        assert F.warp_host(x, 5, 4).shape == (n,) and F.warp_ref(x, 4, 5).shape == (n,)
    for base in (0, 256, 1024, 7 * 256, 2 ** 32, 2 ** 40 + 3 * 256):
        for d in (-1, 0, 1, 255, 256, 257):
            t = base + d
            if t < 0:
                continue
            lo = max(0, t // 256 - 8)                          # the blocks below lo are there; count the rest one by one
            want = 256 * (lo + sum(1 for b in range(lo, t // 256 + 1) if (b + 4) * 256 <= t))
            assert F.emitted(t) == 256 * max(0, t // 256 - 3) == want, t
            assert F.emitted(t, 3, 3) == t
            for n_in in (0, 1, 256, 3200):
                m0, k = F.counts(t, n_in)
                assert m0 == F.emitted(t) and m0 + k == F.emitted(t + n_in) and k % 256 == 0
                assert F.counts(t, n_in, True) == (m0, t + n_in - m0)
                assert F.counts(t, n_in, False, 1, 1) == (t, n_in)
    assert F.DELAY == 1023 and max(t - F.emitted(t) for t in range(0, 4096)) == 1023
    x = _noise(3, 3000)
    bad = x.copy()
    bad[[5, 1000, 2999]] = [np.nan, np.inf, -np.inf]
    zeroed = x.copy()
    zeroed[[5, 1000, 2999]] = 0.0
    assert np.array_equal(F.warp_host(bad, 5, 4).numpy(), F.warp_host(zeroed, 5, 4).numpy())
    assert np.array_equal(F.warp_ref(bad, 5, 4), F.warp_ref(zeroed, 5, 4))


def test_chunk_invariance_of_the_host_form():
    """HostFormant fed a signal cut at 1, 255, 256, 257, 700, 3200 samples (in every rotation) and flushed equals warp_host of the
    whole signal bit for bit, and its counts are formant.counts; a flushed stream refuses its next push"""
    x = np.concatenate([_noise(4, 2000), vowel()[:2669].astype(np.float32)])
    for a, b in WARPS + [(1, 1)]:
        whole = F.warp_host(x, a, b)
        for rot in range(6):
            h, at, got = F.HostFormant(a, b), 0, []
            for k in range(6):
                c = CUTS[(k + rot) % 6]
                want = F.counts(at, c, False, a, b)[1]
                got.append(h.push(torch.from_numpy(x[at:at + c])))
                assert got[-1].shape == (want,) and got[-1].dtype == torch.float32
                at += c
            assert at == x.shape[0] == h.total_in
            got.append(h.flush())
            assert torch.equal(torch.cat(got), whole), (a, b, rot)
            with pytest.raises(RuntimeError, match="flushed"):
                h.push(torch.zeros(1))


def _close(got, want, tol=0.06):
    return len(got) == len(want) and all(abs(g / w - 1.0) <= tol for g, w in zip(got, want))


def test_the_formants_move_and_the_pitch_does_not():
    """noise through resonators at 700 / 1500 / 2600 Hz: at 5/4, 4/5, 3/2 and 2/3 the read-out has exactly three maxima, each within
    6 % of A / B times the input's own read-out (measured: within 3.6 %; 656 / 1559 / 2695 Hz read 1008 / 2320 / 4031 at 3/2); a pulse
    train of period 218 through the same resonators keeps its autocorrelation peak at lag 218 +- 1"""
    own = peaks(vowel())
    assert _close(own, FORMANTS, 0.07)
    for a, b in WARPS:
        got = peaks(F.warp_ref(vowel(), a, b))
        print(f"[formant {a}/{b}] {[round(v) for v in own]} Hz read {[round(v) for v in got]}")
        assert _close(got, [v * a / b for v in own]), (a, b, got)
        y = F.warp_ref(pulses(), a, b)[4096:4096 + 8192]
        ac = np.correlate(y, y, "full")[y.shape[0] - 1:]
        lag = 100 + int(np.argmax(ac[100:400]))
        assert abs(lag - 218) <= 1, (a, b, lag)
    ac = np.correlate(pulses()[4096:4096 + 8192], pulses()[4096:4096 + 8192], "full")[8191:]
    assert 100 + int(np.argmax(ac[100:400])) == 218


def test_a_warp_by_q_over_p_in_front_of_the_resampler_keeps_the_formants():
    """the same excitation warped by Q / P, then pitch.resample_ref at P / Q: the three maxima read within 6 % of the input's at 89/84,
    5/4, 4/5 and 2/3; without the warp they read off by P / Q -- what the stage is for"""
    own = peaks(vowel())
    for p, q in [(89, 84), (5, 4), (4, 5), (2, 3)]:
        kept = peaks(P.resample_ref(F.warp_ref(vowel(), q, p), p, q))
        moved = peaks(P.resample_ref(vowel(), p, q))
        print(f"[formant then pitch {p}/{q}] {[round(v) for v in own]} Hz: kept {[round(v) for v in kept]}, without the warp {[round(v) for v in moved]}")
        assert _close(kept, own), (p, q, kept)
        assert _close(moved, [v * p / q for v in own]), (p, q, moved)
        if abs(p / q - 1.0) > 0.1:
            assert not _close(moved, own)


def test_the_streamers_arithmetic():
    """formant=0.0 with pitch=S is exactly the reduced Q / P of pitch.ratio(S); out-of-range values and a combined fraction outside
    [1/2, 2] are refused by name; formant=None builds no stage, and neither does a fraction of 1 / 1 everywhere"""
    for s in (-12.0, -7.0, -3.0, 1.0, 2.0, 4.0, 7.0, 12.0):
        p, q = P.ratio(s)
        assert F.fraction(0.0, s) == (q, p) and F.fraction(s) == F.warp_of(s) == (p, q) and F.fraction(s, s) == (1, 1)
        st = AudioStreamer(1, pitch=s, formant=0.0)
        assert st._formant == [(q, p)] and st._level == ([0.0], -1.0)
        st.close()
    assert P.ratio(2.0) == (55, 49) and P.ratio(4.0) == (63, 50) and F.fraction(2.0, 4.0) == (2750, 3087) and max(max(F.fraction(f, s)) for f in (5.0, -5.0) for s in (6.0, -6.0, 1.0)) <= 10 ** 4
    assert _formant_of([0.0, 2.0, None], [4.0, 0.0, -3.0], 3) == [(50, 63), P.ratio(2.0), (1, 1)]
    for kw, msg in ((dict(formant=13.0), r"formant: semitones must lie in \[-12, 12\], got 13.0"),
                    (dict(formant=float("nan")), "formant: semitones must lie in"),
                    (dict(formant=8.0, pitch=-8.0), r"formant=8.0 with pitch=-8.0 asks the stage for a warp of \d+ / \d+, outside \[1/2, 2\]"),
                    (dict(formant=[1.0, 2.0]), r"AudioStreamer\(formant=\.\.\.\): one value \(or None\), or one per sample index \(1\), got 2")):
        with pytest.raises(ValueError, match=msg):
            AudioStreamer(1, **kw)
    with pytest.raises(ValueError, match="must have both terms"):
        F.HostFormant(10001, 10000)
    for kw in (dict(), dict(pitch=3.0), dict(formant=None, pitch=3.0), dict(formant=0.0), dict(formant=3.0, pitch=3.0)):
        st = AudioStreamer(1, **kw)
        assert st._formant is None and st._fm is None and st._level is None and st._stages == []
        st.close()
    st = AudioStreamer(2, formant=[None, -2.0], ceiling_db=-3.0)
    assert st._formant == [(1, 1), P.ratio(-2.0)] and st._level == ([0.0, 0.0], -3.0) and st._pitch is None
    st.close()


def test_cpu_chunks_through_the_streamer():
    """AudioStreamer(3, formant=[0.0, +2.0, None], pitch=[+4, 0, -3], speed=1.25) on CPU chunks of 3200: per sample index the delivered
    chunks, concatenated, equal the host forms chained over the whole signal -- tempo, formant, pitch, level, the tails flushed in that
    order -- bit for bit; no delivered sample exceeds the ceiling; the None index equals the chain without the warp"""
    x = torch.from_numpy(np.stack([vowel()[i * 9000:i * 9000 + 3 * 3200].astype(np.float32) * 1.9 for i in range(3)]))
    pitch, formant = [4.0, 0.0, -3.0], [0.0, 2.0, None]
    st = AudioStreamer(3, formant=formant, pitch=pitch, speed=1.25, timeout=20)
    for k in range(3):
        st.put(x[:, k * 3200:(k + 1) * 3200], torch.tensor([0, 1, 2]))
    st.end()
    ceiling = np.float32(10.0 ** (-1.0 / 20.0))
    for idx in range(3):
        got = torch.cat(list(st.get_stream(idx)))
        y = x[idx]
        v = P.tempo_speed(1.25, pitch[idx])
        y = stretch_host(y, v)
        if formant[idx] is not None:
            y = F.warp_host(y, *F.fraction(formant[idx], pitch[idx]))
        if P.ratio(pitch[idx]) != (1, 1):
            y = P.pitch_host(y, pitch[idx])
        y = level_host(y, 0.0, -1.0, 24000)
        assert got.dtype == torch.float32 and torch.equal(got, y), idx
        assert float(got.abs().max()) <= ceiling
    st._thread.join(timeout=20)
