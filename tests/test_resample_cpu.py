"""CPU tests of vibevoice_amd/resample.py -- the filter design, the definition (resample_ref), the host's streaming bookkeeping --
and of AudioStreamer(sample_rate=...) on CPU chunks.  The device kernels are held to the same definition in test_gpu_resample.py.

Design bounds (atten_db = 80, zeros = 32): Kaiser's attenuation formula is approximate, so the stopband must reach atten_db - 1 dB;
the passband up to 0.5 / max(L, M) - dw (0.84 of the lower Nyquist frequency) must stay within +-0.005 dB and every phase's DC gain
within 1e-4 of 1.  Measured with the float64 design: stopband 79.3-79.9 dB, ripple +-0.0009 dB, DC gain error <= 4e-5 (float32 table).
Tone bound: a passband ripple of 1e-4 relative allows 80 dB; resample_ref measures 96-104 dB."""
import random

import numpy as np
import pytest
import torch

from vibevoice_amd import resample as R
from vibevoice_amd.streamer import AsyncAudioStreamer, AudioStreamer

OUT_OF_24K = [8000, 16000, 22050, 32000, 44100, 48000]
INTO_24K = [16000, 22050, 32000, 44100, 48000]
PAIRS = [(24000, d) for d in OUT_OF_24K] + [(s, 24000) for s in INTO_24K]
TONE_PAIRS = [(24000, 48000), (24000, 16000), (24000, 8000), (24000, 44100), (48000, 24000), (44100, 24000)]
ATTEN = 80.0


def _ids(pairs):
    return [f"{s}to{d}" for s, d in pairs]


@pytest.mark.parametrize("src,dst", PAIRS, ids=_ids(PAIRS))
def test_design(src, dst):
    L, M, T, coef = R.design(src, dst)
    g = np.gcd(src, dst)
    assert (L, M) == (dst // g, src // g)
    t_min = int(np.ceil(2 * 32 * max(1.0, M / L) - 1e-9))
    assert T % 2 == 0 and T in (t_min, t_min + 1)
    assert coef.shape == (L, T) and coef.dtype == np.float32
    h, dw = R.prototype(src, dst)
    assert h.shape == (L * T,) and h[-1] == 0.0
    assert np.array_equal(coef, h.reshape(T, L).T.astype(np.float32))            # coef[p][t] = h[p + t L]
    n0 = L * T - 1
    assert np.array_equal(h[:n0], h[:n0][::-1])
    flat = coef.T.reshape(-1)[:n0]
    assert np.array_equal(flat, flat[::-1])                                      # the float32 table is symmetric as a prototype
    H = np.abs(np.fft.rfft(h, 1 << 20)) / L
    f = np.arange(H.shape[0]) / float(1 << 20)                                   # cycles per sample at L * src
    edge = 0.5 / max(L, M)
    stop = -20.0 * np.log10(H[f >= edge].max())
    ripple = 20.0 * np.log10(H[f <= edge - dw])
    dc = np.abs(coef.astype(np.float64).sum(axis=1) - 1.0).max()
    print(f"[design {src}->{dst}] L={L} M={M} T={T} stopband {stop:.2f} dB, ripple {ripple.min():+.5f}..{ripple.max():+.5f} dB, "
          f"phase DC error {dc:.2e}, A1 {np.abs(coef).sum(axis=1).max():.3f}")
    assert stop >= ATTEN - 1.0, stop
    assert ripple.min() >= -0.005 and ripple.max() <= 0.005, (ripple.min(), ripple.max())
    assert dc <= 1e-4, dc


@pytest.mark.parametrize("src,dst", TONE_PAIRS, ids=_ids(TONE_PAIRS))
def test_tone_snr(src, dst):
    """a 1 kHz tone of 4000 samples against the ideal tone at the output rate, 3 T samples skipped at either end: >= 80 dB, and the
    length is ceil(n L / M) -- a prototype of even length (half a tap off centre) gives 24 dB here"""
    L, M, T, _ = R.design(src, dst)
    n = 4000
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / src)
    y = R.resample_ref(x, src, dst)
    assert y.dtype == np.float64 and y.shape == (-(-n * L // M),)
    ideal = np.sin(2.0 * np.pi * 1000.0 * np.arange(y.shape[0]) / dst)
    sl = slice(3 * T, y.shape[0] - 3 * T)
    assert sl.stop - sl.start > 100
    snr = 10.0 * np.log10((ideal[sl] ** 2).sum() / ((y[sl] - ideal[sl]) ** 2).sum())
    print(f"[tone {src}->{dst}] SNR {snr:.1f} dB over {sl.stop - sl.start} samples")
    assert snr >= 80.0, snr


def _splits(n, T):
    rng = random.Random(5)
    yield from ([c] for c in (1, 7, T // 2 - 1, T // 2, T // 2 + 1, 3200))
    for _ in range(3):
        yield [rng.choice([1, 2, 7, T // 2 - 1, T // 2, T // 2 + 1, 100, 700, 3200]) for _ in range(64)]


@pytest.mark.parametrize("src,dst", TONE_PAIRS, ids=_ids(TONE_PAIRS))
def test_host_class_is_chunk_invariant(src, dst):
    """the same signal in chunks of 1, 7, T/2 - 1, T/2, T/2 + 1, 3200 and in mixed random cuts: the concatenation equals the one-shot
    result exactly, totals ceil(n L / M), counts() says what push returns at every step, and what a push holds back is what
    delay_samples says"""
    L, M, T, coef = R.design(src, dst)
    n = 3 * 3200 + 17
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32))
    one = R.resample_host(x, src, dst)
    assert one.dtype == torch.float32 and one.shape[0] == R.total_out(n, L, M) == -(-n * L // M)
    ref = R.resample_ref(x.numpy(), src, dst)
    bound = (T + 3) * 2.0 ** -24 * float(np.abs(coef).sum(axis=1).max())
    assert float(np.abs(one.numpy().astype(np.float64) - ref).max()) <= bound
    short = 3 * T + 41                                   # the one-sample and seven-sample cuts run over a short signal: same paths
    one_short = R.resample_host(x[:short], src, dst)
    for cuts in _splits(n, T):
        xs, want = (x[:short], one_short) if max(cuts) <= 7 else (x, one)
        ns = xs.shape[0]
        h = R.HostResampler(src, dst)
        assert h.taps == T and h.delay_samples == T // 2
        got, at, k = [], 0, 0
        while at < ns:
            c = min(cuts[k % len(cuts)], ns - at)
            k += 1
            m0, cnt = R.counts(L, M, T, h.total_in, c)
            assert m0 == sum(g.shape[0] for g in got)
            y = h.push(xs[at:at + c])
            at += c
            assert y.shape[0] == cnt == h.counts(0)[0] - m0
            # everything whose newest input sample has arrived is out: the next output needs a sample at or beyond `at` ...
            assert (R.emitted(at, L, M, T) * M + (L * T - 2) // 2) // L >= at
            e = R.emitted(at, L, M, T)                   # ... and the last one that is out needed none: nothing is held that could go
            assert e == 0 or ((e - 1) * M + (L * T - 2) // 2) // L < at
            got.append(y)
        m0, cnt = R.counts(L, M, T, h.total_in, 0, flush=True)
        tail = h.flush()
        assert tail.shape[0] == cnt and m0 + cnt == R.total_out(ns, L, M)
        got.append(tail)
        with pytest.raises(RuntimeError, match="flushed"):
            h.push(xs[:4])
        assert torch.equal(torch.cat(got), want), cuts[:4]
        h.reset()
        assert torch.equal(h.push(xs, flush=True), want)


@pytest.mark.parametrize("src,dst", TONE_PAIRS, ids=_ids(TONE_PAIRS))
def test_push_width_fits_the_kernel(src, dst):
    """Resampler.take (resample.push_width): whatever the streams have taken and still hold, the width w it returns keeps every row of
    the next push within the kernel's 8192 outputs and the chunk within its LDS beside the filter table (the two refusals of
    vv_resample_rows, written out here as the C side has them), and it is all that remains wherever that fits"""
    from vibevoice_amd.engine import Resampler
    L, M, T, _ = R.design(src, dst)
    rs = Resampler.__new__(Resampler)                    # the host arithmetic alone: no engine, no configuration
    rs.L, rs.M, rs.T = L, M, T

    def fits(totals, widths, flush):
        return (all(R.counts(L, M, T, t, w, flush)[1] <= 8192 for t, w in zip(totals, widths))
                and 4 * (L * (T + 1) + T + max(widths) + T // 2) <= 65536 - 64)
    whole = 0
    for totals in ([0, 0, 0], [3200, 0, 4097], [2999, 3001, 3000]):
        rs.total = totals
        for most in (0, 1, T // 2, 3200, 4000, 4096, 4097, 6400, 8192, 12801, 16000, 20000, 70000):
            for flush in (False, True):
                rem = [most, most // 2, max(most - 1, 0)]
                w = rs.take([0, 1, 2], rem, flush)
                assert w == R.push_width(L, M, T, totals, rem, flush)
                assert 0 <= w <= most and (w > 0 or most == 0), (totals, most, flush, w)
                assert fits(totals, [min(r, w) for r in rem], flush), (totals, most, flush, w)
                if fits(totals, rem, flush):
                    assert w == most
                    whole += 1
    assert 0 < whole < 3 * 13 * 2                         # both answers occur for every pair


def _drain(st, idx):
    out = []
    while True:
        v = st.audio_queues[idx].get(timeout=10)
        if v is st.stop_signal:
            return out
        out.append(v)


def test_streamer_on_cpu_chunks_at_16k():
    """chunks of 3200 for two samples, ragged ends: order kept, every chunk trimmed to what the sample emitted, the tail in front of
    the stop signal, ceil(n * 2 / 3) samples in all and equal to the one-shot result; close() does not flush"""
    x = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, (2, 1, 4 * 3200)).astype(np.float32))
    st = AudioStreamer(2, sample_rate=16000, timeout=10)
    L, M, T, _ = R.design(24000, 16000)
    for k in range(4):
        if k < 2:
            st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
        else:
            st.put(x[:1, :, k * 3200:(k + 1) * 3200], torch.tensor([0]))
        if k == 1:
            st.end(torch.tensor([1]))
            st.put(x[1:, :, :3200], torch.tensor([1]))                   # an index that comes back after its end() is dropped
    st.end()
    for idx, n in ((0, 4 * 3200), (1, 2 * 3200)):
        chunks = _drain(st, idx)
        want = R.resample_host(x[idx, 0, :n], 24000, 16000)
        sizes = [c.shape[-1] for c in chunks]
        expect, h = [], R.HostResampler(24000, 16000)
        for _ in range(n // 3200):
            expect.append(R.counts(L, M, T, h.total_in, 3200)[1])
            h.push(torch.zeros(3200))
        expect.append(R.counts(L, M, T, h.total_in, 0, True)[1])
        assert sizes == expect and sizes[-1] > 0, (sizes, expect)
        assert all(c.shape == (1, s) and c.dtype == torch.float32 for c, s in zip(chunks, sizes))
        got = torch.cat(chunks, dim=-1)[0]
        assert got.shape[0] == -(-n * 2 // 3)
        assert torch.equal(got, want)
        assert st.audio_queues[idx].empty()
    st._thread.join(timeout=10)
    # a put that completes no output sample delivers nothing; close() ends without the tail
    st = AudioStreamer(1, sample_rate=16000, timeout=10)
    assert R.counts(L, M, T, 0, T // 2 - 1) == (0, 0) and R.counts(L, M, T, 0, T // 2) == (0, 1)
    st.put(x[:1, :, :T // 2 - 1], torch.tensor([0]))
    st.put(x[:1, :, T // 2 - 1:3200], torch.tensor([0]))
    st.close()
    chunks = _drain(st, 0)
    assert [c.shape[-1] for c in chunks] == [R.counts(L, M, T, T // 2 - 1, 3200 - T // 2 + 1)[1]]
    assert sum(c.shape[-1] for c in chunks) == R.emitted(3200, L, M, T) < -(-3200 * 2 // 3)
    st._thread.join(timeout=10)


@pytest.mark.parametrize("rate", [None, 24000])
def test_streamer_without_a_rate_is_unchanged(rate):
    """sample_rate None and 24000: the very tensors the streamer delivers without the keyword, and no resampler anywhere"""
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, 1, 6400)).astype(np.float32)).to(torch.bfloat16)
    a, b = AudioStreamer(2, timeout=10), AudioStreamer(2, timeout=10, sample_rate=rate)
    assert b._rs is None and b.sample_rate == 24000
    for st in (a, b):
        st.put(x[:, :, :3200], torch.tensor([0, 1]))
        st.put(x[:, :, 3200:], torch.tensor([1, 0]))
        st.end()
    for idx in range(2):
        ca, cb = _drain(a, idx), _drain(b, idx)
        assert len(ca) == len(cb) == 2
        for u, v in zip(ca, cb):
            assert u.dtype == v.dtype == torch.bfloat16 and u.shape == v.shape == (1, 3200) and torch.equal(u, v)
    assert not b._rs_host


def test_async_streamer_takes_the_keyword():
    import asyncio
    import inspect
    assert "sample_rate" in inspect.signature(AsyncAudioStreamer.__init__).parameters
    assert "engine" in inspect.signature(AudioStreamer.__init__).parameters

    async def run():
        st = AsyncAudioStreamer(1, sample_rate=8000)
        x = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (1, 1, 3200)).astype(np.float32))
        st.put(x, torch.tensor([0]))
        st.end()
        return [c async for c in st.get_stream(0)], x
    chunks, x = asyncio.run(run())
    assert torch.equal(torch.cat(chunks, dim=-1)[0], R.resample_host(x[0, 0], 24000, 8000))
    assert sum(c.shape[-1] for c in chunks) == -(-3200 // 3)
