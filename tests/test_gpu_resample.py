"""GPU tests of the streaming resampler (csrc/resample.hip: vv_resample_rows, vv_resample_once) against vibevoice_amd/resample.py,
of its chunk invariance and state handling, its 16-bit mode, its refusals, and of AudioStreamer(sample_rate=...) on device chunks
and through generate_continuous().  One engine serves the whole file: the small one of test_gpu_noise_rows.py.

The bound of the kernels against resample_ref (the definition in float64 over the float32 table) is derived, not measured:
    |y - y_ref| <= (T + 3) * 2^-24 * A1 * max|x|,     A1 = max_p sum_t |coef[p][t]|   (2.15 - 2.32 for these designs)
-- T roundings of the fp32 accumulation (every partial sum is at most A1 max|x|), one for the coefficient, one for the input and one
for the final store: 9e-6 at T = 64, 2.5e-5 at T = 192 for inputs in +-1.  A sequential fp32 emulation on the host stays near 5e-7; a
wrong tap, phase or offset is an O(0.1) error on uniform noise.  test_kernel_against_the_definition prints the measured maximum of
every case; on an MI355X: 3.9e-7 to 7.6e-7 over the streaming cases, 4.9e-7 to 7.2e-7 one-shot (12 to 40 times inside the bound)."""
import types

import numpy as np
import pytest
import torch

import synth
from gpu_util import build_small
from vibevoice_amd import resample as R
from vibevoice_amd.engine import EngineError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

PAIRS = [(24000, 48000), (24000, 16000), (24000, 8000), (24000, 44100), (48000, 24000), (44100, 24000)]
IDS = [f"{s}to{d}" for s, d in PAIRS]
GUARD, SENTINEL = 64, -77.25
N_STREAMS = 11
STREAMS = {1: [7], 3: [9, 2, 5], 8: [10, 0, 3, 8, 1, 6, 4, 2]}            # non-identity stream ids
S, E, D, X = 60, 61, 62, 63                  # control tokens inside the small vocabulary
TOK = types.SimpleNamespace(speech_start_id=S, speech_end_id=E, speech_diffusion_id=D, eos_token_id=X, bos_token_id=None, pad_token_id=59)


@pytest.fixture(scope="module")
def small():
    lm = synth.LMCfg(hidden=256, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
    s = build_small(lm, xsplit=3, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    yield s
    s.eng.close()


def _bound(src, dst, peak=1.0):
    L, M, T, coef = R.design(src, dst)
    return (T + 3) * 2.0 ** -24 * float(np.abs(coef).sum(axis=1).max()) * peak


def _noise(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).uniform(-1, 1, shape) * scale).astype(np.float32))


def _push(eng, rs, chunks, ids, flush=False, pcm16=False, cap=None):
    """One push of the rows `chunks` (1-D CPU tensors, lengths may differ: n_in per row) into guarded buffers: a sentinel row above
    and below the output rows and sentinel columns behind every row's count, a sentinel row above and below the input rows.  Checks
    the guards, that the input is unchanged and that the counts are what resample.counts says -> (per-row outputs, counts)."""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n + 2, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[1 + i, :c.shape[0]] = c
    fl = [flush] * n if isinstance(flush, bool) else list(flush)
    want = [R.counts(rs.L, rs.M, rs.T, rs.total[ids[i]], int(chunks[i].shape[0]), fl[i])[1] for i in range(n)]
    cap = max(want) + GUARD if cap is None else cap
    dt = torch.int16 if pcm16 else torch.float32
    sent = int(SENTINEL) if pcm16 else SENTINEL
    xd = xin.to(eng.device)
    out = torch.full((n + 2, cap), sent, dtype=dt, device=eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        _, cnts = rs.push(xd[1:n + 1], ids, flush=fl, out=out[1:n + 1], pcm16=pcm16, n_in=[int(c.shape[0]) for c in chunks])
    eng.sync()
    host = out.cpu()
    assert cnts == want, (cnts, want)
    assert bool((host[0] == sent).all()) and bool((host[n + 1] == sent).all()), "guard rows were written"
    for i in range(n):
        assert bool((host[1 + i, cnts[i]:] == sent).all()), f"row {i}: written beyond its {cnts[i]} samples"
    assert torch.equal(xd.cpu(), xin), "the input buffer was written"
    return [host[1 + i, :cnts[i]].clone() for i in range(n)], cnts


@pytest.fixture()
def make(small):
    made = []

    def _make(src, dst, n_streams=N_STREAMS):
        made.append(small.eng.resampler(src, dst, n_streams))
        return made[-1]
    yield _make
    for r in made:
        r.close()


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_kernel_against_the_definition(small, make, src, dst):
    """n = 1, 3 and 8 rows with non-identity stream ids; row i of step k brings chunk (k + i) % 6 of 1, T/2 - 1, T/2, T/2 + 1, 700
    and 3200 samples, so the rows of one launch stand at different input totals and bring different lengths; pushes that emit
    nothing occur (asserted); the last step flushes -- one row with its last chunk, the others with no samples at all.  Every
    stream's concatenated output against resample_ref in float64 of its concatenated input, within the derived bound, ceil(n L / M)
    samples; guards around every output row and the input stay untouched (_push)."""
    eng, rs = small.eng, make(src, dst)
    L, M, T = rs.L, rs.M, rs.T
    assert rs.taps == T and rs.delay_samples == T // 2
    lens = [1, T // 2 - 1, T // 2, T // 2 + 1, 700, 3200]
    bound = _bound(src, dst)
    saw_zero = False
    for n, ids in STREAMS.items():
        rs.reset()
        sig = [_noise(100 * n + i, sum(lens)) for i in range(n)]
        at, got = [0] * n, [[] for _ in range(n)]
        for k in range(6):
            chunks = []
            for i in range(n):
                c = lens[(k + i) % 6]
                chunks.append(sig[i][at[i]:at[i] + c])
                at[i] += c
            outs, cnts = _push(eng, rs, chunks, ids, flush=[k == 5 and i == 0 for i in range(n)])
            saw_zero |= 0 in cnts
            for i in range(n):
                got[i].append(outs[i])
        assert at == [sum(lens)] * n
        if n > 1:
            outs, _ = _push(eng, rs, [torch.zeros(0)] * (n - 1), ids[1:], flush=True)
            for i in range(1, n):
                got[i].append(outs[i - 1])
        worst = 0.0
        for i in range(n):
            y = torch.cat(got[i]).numpy().astype(np.float64)
            ref = R.resample_ref(sig[i].numpy(), src, dst)
            assert y.shape == ref.shape == (-(-sum(lens) * L // M),)
            worst = max(worst, float(np.abs(y - ref).max()))
        print(f"[resample {src}->{dst} n={n}] L={L} M={M} T={T}: max |gpu - ref| = {worst:.3e} (bound {bound:.2e})")
        assert worst <= bound, (worst, bound)
    assert saw_zero


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_chunk_invariance_on_the_device(small, make, src, dst):
    """the same 3000-sample signal in 1, 3 and 17 pushes (and a flush of no samples): bit-identical to Engine.resample, which is
    within the kernel bound of the definition"""
    eng, rs = small.eng, make(src, dst)
    x = _noise(7, 3000)
    with torch.cuda.stream(eng.stream):
        one = eng.resample(x, src, dst)
        two = eng.resample(torch.stack([x, -x]).to(eng.device), src, dst)
    eng.sync()
    one = one.cpu()
    assert one.shape == (-(-3000 * rs.L // rs.M),) and torch.equal(two[0].cpu(), one) and torch.equal(two[1].cpu(), -one)
    err = float(np.abs(one.numpy().astype(np.float64) - R.resample_ref(x.numpy(), src, dst)).max())
    print(f"[resample once {src}->{dst}] max |gpu - ref| = {err:.3e} (bound {_bound(src, dst):.2e})")
    assert err <= _bound(src, dst)
    for pushes in (1, 3, 17):
        rs.reset([4])
        cuts = np.linspace(0, 3000, pushes + 1).astype(int)
        got = [_push(eng, rs, [x[a:b]], [4])[0][0] for a, b in zip(cuts[:-1], cuts[1:])]
        got.append(_push(eng, rs, [torch.zeros(0)], [4], flush=True)[0][0])
        assert torch.equal(torch.cat(got), one), pushes


def test_reset_leaves_no_stale_state(small, make):
    """a loud signal through stream 0, reset([0]), then a quiet one: bit-equal to a fresh resampler; stream 1, in the middle of its
    own signal, does not notice its neighbour's reset"""
    eng = small.eng
    rs, fresh = make(24000, 16000, 2), make(24000, 16000, 2)
    loud, quiet, other = _noise(1, 1000, scale=100.0), _noise(2, 1000, scale=1e-3), _noise(3, 2000)
    _push(eng, rs, [loud, other[:1000]], [0, 1])
    _push(eng, fresh, [other[:1000]], [1])
    with torch.cuda.stream(eng.stream):
        rs.reset([0])
    a, _ = _push(eng, rs, [quiet, other[1000:]], [0, 1], flush=True)
    b, _ = _push(eng, fresh, [quiet, other[1000:]], [0, 1], flush=True)
    assert a[0].shape[0] == -(-1000 * 2 // 3) and torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    with torch.cuda.stream(eng.stream):
        want = eng.resample(other, 24000, 16000)
    eng.sync()
    assert torch.equal(a[1], want.cpu()[-a[1].shape[0]:])


def _pcm16_rule(rows):
    """the numpy rule of test_pcm16_reference_arithmetic (test_dropin_cpu.py), per chunk"""
    out = []
    for r in rows:
        data = r.numpy()
        peak = np.float32(np.abs(data).max()) if data.size else np.float32(0)
        mine = data / peak if peak > 1.0 else data
        out.append(torch.from_numpy(np.trunc(mine * np.float32(32767.0)).astype(np.int16)))
    return out


@pytest.mark.parametrize("src,dst", [(24000, 48000), (24000, 8000), (24000, 44100)], ids=["24000to48000", "24000to8000", "24000to44100"])
def test_int16_mode_is_the_pcm16_rule_on_the_float_rows(small, make, src, dst):
    """two resamplers in the same state; one push as float, one as int16 (the same single launch): the int16 rows equal the numpy rule
    applied to the float rows, bit for bit -- a row whose resampled peak exceeds 1 (normalised), one below, one of 5 samples"""
    eng = small.eng
    a, b = make(src, dst, 3), make(src, dst, 3)
    warm = [_noise(10, 500), _noise(11, 500, scale=0.3), _noise(12, 500)]      # the quiet row is quiet from its first sample on
    rows = [_noise(20, 3200, scale=2.5), _noise(21, 3200, scale=0.3), _noise(22, 5, scale=0.9)]
    for rs in (a, b):
        _push(eng, rs, warm, [2, 0, 1])
    f, cf = _push(eng, a, rows, [2, 0, 1])
    q, cq = _push(eng, b, rows, [2, 0, 1], pcm16=True)
    assert cf == cq and float(f[0].abs().max()) > 1.0 and float(f[1].abs().max()) < 1.0
    for got, want in zip(q, _pcm16_rule(f)):
        assert got.dtype == torch.int16 and torch.equal(got, want)
    f, _ = _push(eng, a, [torch.zeros(0)] * 3, [2, 0, 1], flush=True)
    q, _ = _push(eng, b, [torch.zeros(0)] * 3, [2, 0, 1], flush=True, pcm16=True)
    for got, want in zip(q, _pcm16_rule(f)):
        assert torch.equal(got, want)


def test_refusals_write_nothing(small, make):
    """every refusal raises with its message, leaves the sentinel-filled outputs untouched and the streams where they were"""
    eng = small.eng
    rs, twin = make(24000, 48000, 4), make(24000, 48000, 4)
    x = _noise(5, 2, 400).to(eng.device)
    out = torch.full((4, 1024), SENTINEL, dtype=torch.float32, device=eng.device)
    first = _noise(6, 300)
    _push(eng, rs, [first], [1])
    _push(eng, twin, [first], [1])
    _push(eng, rs, [first], [3], flush=True)
    cases = [
        (dict(stream_ids=[]), "n = 0 must be in"),
        (dict(stream_ids=[0, 4]), "stream id 4 out of range"),
        (dict(stream_ids=[-1, 0]), "stream id -1 out of range"),
        (dict(stream_ids=[1, 1]), "stream 1 is named twice"),
        (dict(stream_ids=[0, 1], n_in=[400, -1]), "n_in = -1 must be >= 0"),
        (dict(stream_ids=[0, 1], out=out[:, :700].contiguous().fill_(SENTINEL)), "the output rows hold 700"),
        (dict(stream_ids=[0, 3]), "stream 3 has been flushed"),
    ]
    for kw, msg in cases:
        o = kw.pop("out", out)
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                rs.push(x, out=o, **kw)
        eng.sync()
        assert bool((o == SENTINEL).all()), msg
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_resampler_reset(eng._ctx, eng._s, 9, 1, None), "vv_resampler_reset")
    # a pair whose table (147 x 140 taps, 83 KB) does not fit the kernel's LDS is refused when it is configured, by name: no other
    # rate is produced in its place, and the configuration it would have taken stays free
    used = list(eng._rs_used)
    with pytest.raises(EngineError, match="does not fit"):
        eng.resampler(24000, 11025, 1)
    assert eng._rs_used == used
    assert rs.total == [0, 300, 0, 300]
    # the refused calls changed no state: stream 1 goes on exactly like its twin, stream 3 pushes again after its reset
    nxt = _noise(8, 400)
    a, _ = _push(eng, rs, [nxt], [1], flush=True)
    b, _ = _push(eng, twin, [nxt], [1], flush=True)
    assert torch.equal(a[0], b[0])
    with torch.cuda.stream(eng.stream):
        rs.reset([3])
    a, _ = _push(eng, rs, [nxt], [3], flush=True)
    with torch.cuda.stream(eng.stream):
        want = eng.resample(nxt, 24000, 48000)
    eng.sync()
    assert torch.equal(a[0], want.cpu())


def _collect(st, idx):
    return list(st.get_stream(idx))


def test_streamer_at_48k_int16_end_to_end(small):
    """AudioStreamer(2, pcm16=eng, sample_rate=48000) on device chunks of 3200, sample 1 ending two puts before sample 0, then end():
    per sample, the delivered int16 chunks equal the pcm16 rule applied chunk by chunk to what the float streamer
    (engine=eng) delivers, whose concatenation is Engine.resample of the concatenated input bit for bit; 2 n samples each"""
    eng = small.eng
    x = _noise(9, 2, 1, 4 * 3200, scale=1.4).to(eng.device)
    sts = [AudioStreamer(2, pcm16=eng, sample_rate=48000, timeout=20), AudioStreamer(2, engine=eng, sample_rate=48000, timeout=20)]
    with torch.cuda.stream(eng.stream):
        for st in sts:
            for k in range(4):
                if k < 2:
                    st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
                else:
                    if k == 2:
                        st.end(torch.tensor([1]))
                    st.put(x[:1, :, k * 3200:(k + 1) * 3200], torch.tensor([0]))
            st.end()
        want = [eng.resample(x[0, 0], 24000, 48000), eng.resample(x[1, 0, :6400], 24000, 48000)]
    eng.sync()
    for idx, n in ((0, 4 * 3200), (1, 2 * 3200)):
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert len(q) == len(f) == n // 3200 + 1 and all(c.dtype == torch.int16 for c in q) and all(c.dtype == torch.float32 for c in f)
        assert [c.shape for c in q] == [c.shape for c in f] and all(c.dim() == 2 and c.shape[0] == 1 for c in f)
        assert f[-1].shape[-1] > 0                                        # the tail came, in front of the stop signal
        cat = torch.cat(f, dim=-1)[0]
        assert cat.shape[0] == 2 * n and torch.equal(cat, want[idx].cpu())
        for got, rule in zip(q, _pcm16_rule([c[0] for c in f])):
            assert torch.equal(got[0], rule)
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._rs_used == [None] * 4                                     # finished streamers gave their configurations back


def test_streamer_flushes_seventeen_samples_at_once(small):
    """AudioStreamer(17, engine=eng, sample_rate=16000), one put of [17, 1, 480] and end(): more rows than one launch takes, in the put
    and in the flush.  Every sample's chunks concatenate to Engine.resample of its row bit for bit and each gets its stop signal"""
    eng = small.eng
    x = _noise(12, 17, 1, 480).to(eng.device)
    st = AudioStreamer(17, engine=eng, sample_rate=16000, stop_signal="stop", timeout=20)
    with torch.cuda.stream(eng.stream):
        st.put(x, torch.arange(17))
        st.end()
        want = eng.resample(x[:, 0], 24000, 16000).cpu()
    eng.sync()
    counts = []
    for idx in range(17):
        items = [st.audio_queues[idx].get(timeout=20)]
        while not (isinstance(items[-1], str) and items[-1] == "stop"):
            items.append(st.audio_queues[idx].get(timeout=20))
        f = items[:-1]                                                    # the stop signal came, behind the sample's chunks
        counts.append(len(f))
        assert all(c.dtype == torch.float32 and c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        assert torch.equal(torch.cat(f, dim=-1)[0], want[idx]) and want[idx].shape[0] == 320, idx
    print(f"[17 samples, one put and the flush] chunks per sample: {counts}")
    assert counts == [2] * 17
    st._thread.join(timeout=20)
    assert st.audio_queues[0].empty() and eng._rs_used == [None] * 4


def test_requests_through_generate_continuous_at_16k(small):
    """two requests through ONE slot of generate_continuous with a 16 kHz float streamer (stream id = request index, whatever slot
    the request decodes in): per request, the streamed audio has the length of model.resample_audio(speech_outputs[0], 16000) and
    equals it within the kernel bound"""
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    eng = small.eng
    cfgd = {"decoder_config": {"max_position_embeddings": small.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
    m.set_speech_factors(small.scaling, small.bias)
    m.set_ddpm_inference_steps(5)
    g = synth.Gen(77)
    reqs = []
    for i, plan in enumerate([[D, D, D, X], [D, D, X]]):
        ids = torch.from_numpy(g.rng.integers(0, 59, (1, 9 + 3 * i)))
        ids[0, -1] = S
        reqs.append({"input_ids": ids, "attention_mask": torch.ones_like(ids), "_forced_tokens": plan, "seed": 11 + i})
    st = AudioStreamer(2, engine=eng, sample_rate=16000, timeout=30)
    outs = m.generate_continuous(reqs, max_concurrent=1, audio_streamer=st, tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=1.3)
    assert m.last_stats["max_in_flight"] == 1
    for i, frames in enumerate((3, 2)):
        wav = outs[i].speech_outputs[0].reshape(-1)
        assert wav.shape[0] == frames * 3200
        want = m.resample_audio(wav, 16000).cpu()
        torch.cuda.synchronize()
        got = torch.cat([c.reshape(-1) for c in _collect(st, i)]).float()
        assert got.shape == want.shape == (-(-frames * 3200 * 2 // 3),)
        peak = float(wav.abs().max())
        err = float((got.double() - want.double()).abs().max())
        print(f"[generate_continuous at 16 kHz, request {i}] max |streamed - resample_audio| = {err:.3e} (bound {_bound(24000, 16000, peak):.2e})")
        assert err <= _bound(24000, 16000, peak)
    assert eng.stat(5) == 0 and eng.stat(4) == 0
