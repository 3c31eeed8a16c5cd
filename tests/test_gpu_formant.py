"""GPU tests of the formant stage (csrc/formant.hip: vv_formant_rows, vv_formant_once, vv_formant_reset) against vibevoice_amd/formant.py,
of its chunk invariance and state handling, its refusals, and of AudioStreamer(formant=...) on device chunks and through generate().
One engine serves the whole file: the small one of test_gpu_pitch.py.

The bound of the kernels against the definition is the one the feature was specified with, relative to the float32 host form: a stream's
concatenated output is measured against warp_ref(table=True) -- float64 over the float32 twiddle table the device reads -- as relative
L2, and must not exceed 32 times the distance of warp_host, the float32 numpy form, from the same float64 result on the same input.
The margin allows a plain radix-2 transform a worse constant than numpy's, plus logf / expf rounding; a wrong bin, lifter edge, position
or frame offset is an error of 1e-2 or more.  The host form sits 1.0e-7 (noise) to 5.3e-7 (resonator signal) from float64, so the bound
lands near 3e-6 to 2e-5.  test_kernel_against_the_definition prints the measured figure of every row and the maximum per launch shape;
on an MI355X: relative L2 1.7e-7 to 4.1e-7 over the streaming rows against the host form's 1.0e-7 to 1.9e-7 on the same inputs, at
most 2.12 / 2.02 / 2.48 / 2.42 times the host form's distance at n = 1 / 3 / 8 / 17 (13 to 23 times inside the bound).
No bound was derived in the manner of test_gpu_pitch.py: the gain passes through a logarithm of the power, whose conditioning depends
on the signal."""
import types

import numpy as np
import pytest
import torch

import synth
from formant_util import rel_l2, vowel
from gpu_util import build_small
from vibevoice_amd import formant as F
from vibevoice_amd import pitch as P
from vibevoice_amd.engine import EngineError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

FRACS = [(1, 2), (2, 1), (89, 84), (84, 89), (5000, 9999), (5, 4), (1, 1)]
LENS = [1, 255, 256, 257, 700, 3200]
GUARD, SENTINEL = 64, -77.25
N_STREAMS = 19
STREAMS = {1: [7], 3: [9, 2, 5], 8: [10, 0, 3, 8, 1, 6, 4, 2], 17: [18, 3, 11, 0, 7, 16, 2, 9, 14, 5, 1, 12, 17, 6, 10, 4, 13]}
S, E, D, X = 60, 61, 62, 63                  # control tokens inside the small vocabulary
TOK = types.SimpleNamespace(speech_start_id=S, speech_end_id=E, speech_diffusion_id=D, eos_token_id=X, bos_token_id=None, pad_token_id=59)


@pytest.fixture(scope="module")
def small():
    lm = synth.LMCfg(hidden=256, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
    s = build_small(lm, xsplit=3, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    yield s
    s.eng.close()


def _noise(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).uniform(-1, 1, shape) * scale).astype(np.float32))


def _vowel(start, n):
    return torch.from_numpy(vowel()[start:start + n].astype(np.float32))


def _push(eng, fm, chunks, ids, fracs, flush=False, cap=None):
    """One push of the rows `chunks` (1-D CPU tensors, lengths may differ: n_in per row) into guarded buffers: a sentinel row above
    and below the output rows and sentinel columns behind every row's count, a sentinel row above and below the input rows.  Checks
    the guards, that the input is unchanged and that the counts are what formant.counts says -> (per-row outputs, counts)."""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n + 2, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[1 + i, :c.shape[0]] = c
    fl = [flush] * n if isinstance(flush, bool) else list(flush)
    want = [F.counts(fm.total[ids[i]], int(chunks[i].shape[0]), fl[i], *fracs[i])[1] for i in range(n)]
    assert want == [fm.counts(ids[i], int(chunks[i].shape[0]), flush=fl[i], fraction=fracs[i]) for i in range(n)]
    cap = max(want) + GUARD if cap is None else cap
    xd = xin.to(eng.device)
    out = torch.full((n + 2, cap), SENTINEL, dtype=torch.float32, device=eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        _, cnts = fm.push(xd[1:n + 1], ids, fractions=list(fracs), flush=fl, out=out[1:n + 1], n_in=[int(c.shape[0]) for c in chunks])
    eng.sync()
    host = out.cpu()
    assert cnts == want, (cnts, want)
    assert bool((host[0] == SENTINEL).all()) and bool((host[n + 1] == SENTINEL).all()), "guard rows were written"
    for i in range(n):
        assert bool((host[1 + i, cnts[i]:] == SENTINEL).all()), f"row {i}: written beyond its {cnts[i]} samples"
    assert torch.equal(xd.cpu(), xin), "the input buffer was written"
    return [host[1 + i, :cnts[i]].clone() for i in range(n)], cnts


@pytest.fixture()
def make(small):
    made = []

    def _make(n_streams=N_STREAMS):
        made.append(small.eng.formant(n_streams))
        return made[-1]
    yield _make
    for r in made:
        r.close()


@pytest.mark.parametrize("n", [1, 3, 8, 17])
def test_kernel_against_the_definition(small, make, n):
    """n rows with non-identity stream ids, row i at the warp FRACS[(i + n) % 7]: different fractions in the rows of one launch (17 rows:
    two launch groups).  Row i of step k brings chunk (k + i) % 6 of 1, 255, 256, 257, 700 and 3200 samples, so the rows of one launch
    stand at different input totals and bring different lengths; pushes that emit nothing occur (asserted); the last step flushes -- one
    row with its last chunk, the others with no samples at all.  Rows alternate between uniform noise in +-1 and the resonator signal.
    Every stream's concatenated output against the definition in float64 over the table, within 32 times the float32 host form's own
    distance from it, as many samples as went in, the 1/1 rows bit for bit; guards around every output row and the input stay
    untouched (_push).  Measured on an MI355X: the module's docstring."""
    eng, fm, ids = small.eng, make(), STREAMS[n]
    assert fm.delay_samples == 1023 and fm.max_in == F.MAX_IN == P.MAX_IN
    ab = [FRACS[(i + n) % 7] for i in range(n)]
    total = sum(LENS)
    sig = [_noise(100 * n + i, total) if (i + n) % 2 == 0 else _vowel(1000 * i + 37 * n, total) for i in range(n)]
    at, got, saw_zero = [0] * n, [[] for _ in range(n)], False
    for k in range(6):
        chunks = []
        for i in range(n):
            c = LENS[(k + i) % 6]
            chunks.append(sig[i][at[i]:at[i] + c])
            at[i] += c
        outs, cnts = _push(eng, fm, chunks, ids, ab, flush=[k == 5 and i == 0 for i in range(n)])
        saw_zero |= any(c == 0 and ch.shape[0] > 0 for c, ch in zip(cnts, chunks))
        for i in range(n):
            got[i].append(outs[i])
    assert at == [total] * n and [fm.ratio[i] for i in ids] == ab
    if n > 1:
        outs, _ = _push(eng, fm, [torch.zeros(0)] * (n - 1), ids[1:], ab[1:], flush=True)
        for i in range(1, n):
            got[i].append(outs[i - 1])
    assert saw_zero
    worst = 0.0
    for i, (a, b) in enumerate(ab):
        y = torch.cat(got[i])
        assert y.shape == (total,)
        if a == b:
            assert torch.equal(y, sig[i])
            continue
        ref = F.warp_ref(sig[i].numpy(), a, b, table=True)
        err, host = rel_l2(y.numpy(), ref), rel_l2(F.warp_host(sig[i], a, b).numpy(), ref)
        kind = "noise" if (i + n) % 2 == 0 else "vowel"
        print(f"[formant n={n} row {i} stream {ids[i]}] {a}/{b} {kind}: rel L2 gpu - ref = {err:.3e}, host - ref = {host:.3e} (bound {32 * host:.2e})")
        worst = max(worst, err / host)
        assert err <= 32.0 * host, (a, b, err, host)
    print(f"[formant n={n}] the kernel's largest distance: {worst:.2f} times the float32 host form's")


def test_streaming_equals_one_shot_on_the_device(small, make):
    """the same 3000-sample signal in 1, 3 and 17 pushes (and a flush of no samples), every fraction: bit-identical to
    Engine.formant_warp, alone and as one row of a call in which every signal has its own fraction -- device against device, the fixed
    summation order; a 1/1 row equals its input bit for bit, and semitones name pitch.ratio's fractions"""
    eng, fm = small.eng, make()
    x = _vowel(5000, 3000) + _noise(7, 3000, scale=0.01)
    with torch.cuda.stream(eng.stream):
        ones = [eng.formant_warp(x, fractions=ab) for ab in FRACS]
        many = eng.formant_warp(x[None, :].repeat(len(FRACS), 1), fractions=FRACS)
        semi = eng.formant_warp(x, 7.0)
    eng.sync()
    many = many.cpu()
    assert F.warp_of(7.0) == (3, 2) and torch.equal(semi.cpu(), eng.formant_warp(x, fractions=(3, 2)).cpu())
    for j, ab in enumerate(FRACS):
        one = ones[j].cpu()
        assert one.shape == (3000,) and torch.equal(many[j], one)
        if ab[0] == ab[1]:
            assert torch.equal(one, x)
        for pushes in (1, 3, 17):
            fm.reset([4])
            cuts = np.linspace(0, 3000, pushes + 1).astype(int)
            got = [_push(eng, fm, [x[a:b]], [4], [ab])[0][0] for a, b in zip(cuts[:-1], cuts[1:])]
            got.append(_push(eng, fm, [torch.zeros(0)], [4], [ab], flush=True)[0][0])
            assert torch.equal(torch.cat(got), one), (ab, pushes)


def test_reset_leaves_no_stale_state_or_fraction(small, make):
    """a loud signal through stream 0 at 2/1, reset([0]), then a quiet one at 84/89: bit-equal to a fresh stage; stream 1, in the
    middle of its own signal, does not notice its neighbour's reset; without the reset the new fraction is refused by name"""
    eng = small.eng
    fm, fresh = make(2), make(2)
    loud, quiet, other = _noise(1, 1000, scale=100.0), _noise(2, 1000, scale=1e-3), _noise(3, 2000)
    _push(eng, fm, [loud, other[:1000]], [0, 1], [(2, 1), (5, 4)])
    _push(eng, fresh, [other[:1000]], [1], [(5, 4)])
    with pytest.raises(EngineError, match=r"stream 0 runs at warp 2 / 1 since its first push; reset it before it changes to 84 / 89"):
        fm.push(quiet[None, :].to(eng.device), [0], fractions=(84, 89))
    with torch.cuda.stream(eng.stream):
        fm.reset([0])
    assert fm.ratio == [None, (5, 4)] and fm.total == [0, 1000]
    a, _ = _push(eng, fm, [quiet, other[1000:]], [0, 1], [(84, 89), (5, 4)], flush=True)
    b, _ = _push(eng, fresh, [quiet, other[1000:]], [0, 1], [(84, 89), (5, 4)], flush=True)
    assert a[0].shape[0] == 1000 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with torch.cuda.stream(eng.stream):
        want = eng.formant_warp(other, fractions=(5, 4))
    eng.sync()
    assert torch.equal(a[1], want.cpu()[-a[1].shape[0]:])


def test_refusals_write_nothing(small, make):
    """every refusal raises with its message, leaves the sentinel-filled outputs untouched and the streams where they were; the four
    configurations can be taken and a fifth is refused"""
    import ctypes as C
    from vibevoice_amd import _lib
    eng = small.eng
    fm, twin = make(4), make(4)
    x = _noise(5, 2, 400).to(eng.device)
    out = torch.full((4, 2048), SENTINEL, dtype=torch.float32, device=eng.device)
    first = _noise(6, 300)
    _push(eng, fm, [first], [1], [(5, 4)])
    _push(eng, twin, [first], [1], [(5, 4)])
    _push(eng, fm, [first], [3], [(5, 4)], flush=True)
    cases = [
        (dict(stream_ids=[]), "n = 0 must be in"),
        (dict(stream_ids=[0, 4]), "stream id 4 out of range"),
        (dict(stream_ids=[-1, 0]), "stream id -1 out of range"),
        (dict(stream_ids=[1, 1]), "stream 1 is named twice"),
        (dict(stream_ids=[0, 1], n_in=[400, -1]), "n_in = -1 must be >= 0"),
        (dict(stream_ids=[0, 1], flush=True, out=out[:, :300].contiguous().fill_(SENTINEL)), "the output rows hold 300"),
        (dict(stream_ids=[0, 3]), "stream 3 has been flushed"),
        (dict(stream_ids=[0, 1], fractions=[(5, 4), (4, 5)]), "stream 1 runs at warp 5 / 4 since its first push"),
    ]
    for kw, msg in cases:
        o = kw.pop("out", out)
        kw.setdefault("fractions", (5, 4))
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                fm.push(x, out=o, **kw)
        eng.sync()
        assert bool((o == SENTINEL).all()), msg
    # int16 is refused by name: a level stage follows this one
    o16 = torch.full((4, 2048), int(SENTINEL), dtype=torch.int16, device=eng.device)
    with pytest.raises(EngineError, match=r"out_fmt = 1 \(int16\) is not served"):
        fm.push(x, [0, 2], fractions=(5, 4), out=o16, pcm16=True)
    eng.sync()
    assert bool((o16 == int(SENTINEL)).all())
    # capacity: a row longer than one push takes, by name; take() cuts it
    long = torch.zeros((1, F.MAX_IN + 1), dtype=torch.float32, device=eng.device)
    big = torch.full((1, 20000), SENTINEL, dtype=torch.float32, device=eng.device)
    with torch.cuda.stream(eng.stream):
        with pytest.raises(EngineError, match=f"one push takes at most {F.MAX_IN} per row"):
            fm.push(long, [2], fractions=(5, 4), out=big)
    eng.sync()
    assert bool((big == SENTINEL).all()) and fm.ratio[2] is None and fm.take([2], [F.MAX_IN + 1]) == F.MAX_IN
    # A or B outside 1..10^4, or a fraction outside [1/2, 2]: only the C entry point can be asked for one
    for bad in ((10001, 10000), (0, 1), (3, -1), (100, 49), (49, 100)):
        with pytest.raises(ValueError, match="must have both terms"):
            F.check(*bad)
        rows = (_lib.VVFormantRow * 1)()
        rows[0].stream, rows[0].n_in, rows[0].flush, rows[0].A, rows[0].B = 0, 400, 0, bad[0], bad[1]
        cnt = (C.c_int * 1)()
        rc = eng.lib.vv_formant_rows(eng._ctx, eng._s, fm.slot, 1, rows, C.c_void_p(x.data_ptr()), 400, C.c_void_p(out.data_ptr()), 2048, 0, cnt)
        assert rc != 0 and f"warp {bad[0]} / {bad[1]} must have both terms in [1,10000]" in eng._err()
        ab = (C.c_int * 2)(*bad)
        rc = eng.lib.vv_formant_once(eng._ctx, eng._s, C.c_void_p(eng._formant_table().data_ptr()), 1, ab, 400, C.c_void_p(x.data_ptr()), 400,
                                     C.c_void_p(out.data_ptr()), 2048, C.c_void_p(big.data_ptr()), 20000)
        assert rc != 0 and f"warp {bad[0]} / {bad[1]} must have both terms in [1,10000]" in eng._err()
    eng.sync()
    assert bool((out == SENTINEL).all()) and bool((big == SENTINEL).all())
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_formant_reset(eng._ctx, eng._s, 9, 1, None), "vv_formant_reset")
    with pytest.raises(ValueError, match="13"):
        fm.push(x, [0, 2], [1.0, 13.0], out=out)
    assert fm.total == [0, 300, 0, 300] and fm.ratio == [None, (5, 4), None, (5, 4)]
    # the refused calls changed no state: stream 1 goes on exactly like its twin, stream 3 pushes again after its reset
    nxt = _noise(8, 900)
    a, _ = _push(eng, fm, [nxt], [1], [(5, 4)], flush=True)
    b, _ = _push(eng, twin, [nxt], [1], [(5, 4)], flush=True)
    assert a[0].shape[0] == 1200 and torch.equal(a[0], b[0])
    with torch.cuda.stream(eng.stream):
        fm.reset([3])
    a, _ = _push(eng, fm, [nxt], [3], [(2, 3)], flush=True)
    with torch.cuda.stream(eng.stream):
        want = eng.formant_warp(nxt, fractions=(2, 3))
    eng.sync()
    assert torch.equal(a[0], want.cpu())
    # four configurations, and no fifth
    more = [make(1), make(1)]
    assert sorted(s.slot for s in (fm, twin, *more)) == [0, 1, 2, 3]
    with pytest.raises(EngineError, match="all 4 formant configurations of this engine are in use"):
        eng.formant(1)


def _collect(st, idx):
    return list(st.get_stream(idx))


def _pcm16_rule(rows):
    """the numpy rule of test_pcm16_reference_arithmetic (test_dropin_cpu.py), per chunk"""
    out = []
    for r in rows:
        data = r.numpy()
        peak = np.float32(np.abs(data).max()) if data.size else np.float32(0)
        mine = data / peak if peak > 1.0 else data
        out.append(torch.from_numpy(np.trunc(mine * np.float32(32767.0)).astype(np.int16)))
    return out


CEILING = float(np.float32(10.0 ** (-1.0 / 20.0)))


@pytest.mark.parametrize("speed", [1.0, 1.25])
def test_streamer_formant_pitch_on_device_chunks(small, speed):
    """AudioStreamer(3, pitch=[+4, 0, -3], formant=[0.0, +2.0, None], speed) on device chunks of 3200, three puts and end(): per sample
    index the float streamer (engine=eng) delivers, concatenated, the whole-signal composition of the concatenated input -- time_stretch,
    formant_warp, pitch_resample, apply_level -- bit for bit, and the 16-bit streamer (pcm16=eng) the pcm16 rule of each of those chunks;
    no delivered sample exceeds the ceiling of the level stage the warp brings with it; the None index equals the chain without the
    warp (Engine.pitch_shift, what it delivered before, with the level stage added); the stages sit in the order tempo, formant, pitch,
    level and give their configurations back"""
    eng = small.eng
    x = (torch.stack([_vowel(9000 * i, 3 * 3200) for i in range(3)]) * 1.9 + _noise(40, 3, 3 * 3200, scale=0.05))[:, None, :].to(eng.device)
    pitch, formant = [4.0, 0.0, -3.0], [0.0, 2.0, None]
    kw = dict(pitch=pitch, formant=formant, speed=speed, timeout=20)
    sts = [AudioStreamer(3, pcm16=eng, **kw), AudioStreamer(3, engine=eng, **kw)]
    for st in sts:
        assert st._stages == [st._tp, st._fm, st._pt, st._lv] and None not in st._stages
        assert st._formant == [(50, 63), (55, 49), (1, 1)] and st._level == ([0.0] * 3, -1.0)
    with torch.cuda.stream(eng.stream):
        for st in sts:
            for k in range(3):
                st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1, 2]))
            st.end()
        want = []
        for idx in range(3):
            y = eng.time_stretch(x[idx, 0], sts[0]._speeds[idx])
            if sts[0]._formant[idx] != (1, 1):
                y = eng.formant_warp(y, fractions=sts[0]._formant[idx])
            if P.ratio(pitch[idx]) != (1, 1):
                y, cnt = eng.pitch_resample(y, pitch[idx])
                y = y[:cnt[0]]
            want.append(eng.apply_level(y, 0.0, -1.0, 24000))
        plain = eng.apply_level(eng.pitch_shift(x[2, 0], pitch[2], speed), 0.0, -1.0, 24000)
        kept = eng.apply_level(eng.pitch_shift(x[0, 0], pitch[0], speed, formant=0.0), 0.0, -1.0, 24000)
    eng.sync()
    assert torch.equal(plain, want[2]) and torch.equal(kept, want[0])
    for idx in range(3):
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert len(q) == len(f) >= 3 and all(c.dtype == torch.int16 for c in q) and all(c.dtype == torch.float32 for c in f)
        assert [c.shape for c in q] == [c.shape for c in f] and all(c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        cat = torch.cat(f, dim=-1)[0]
        assert cat.shape[0] == P.shift_len(3 * 3200, pitch[idx], speed) and torch.equal(cat, want[idx].cpu()), idx
        assert float(cat.abs().max()) <= CEILING
        for got, rule in zip(q, _pcm16_rule([c[0] for c in f])):
            assert torch.equal(got[0], rule)
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._fm_used == [None] * 4 and eng._pt_used == [None] * 4 and eng._tp_used == [None] * 4 and eng._lv_used == [None] * 4


def test_streamer_unwarped_index_passes_its_stage_and_device_chunks_need_an_engine(small):
    """formant=[+3, None] without pitch: index 1 runs through the formant stage at 1/1 and arrives as Engine.apply_level of what was put,
    bit for bit (the level stage the warp brings is all that touches it); index 0 is formant_warp then apply_level; without an engine
    device chunks are refused by name"""
    eng = small.eng
    x = (torch.stack([_vowel(3000, 2 * 3200), _vowel(20000, 2 * 3200)]) * 1.5)[:, None, :].to(eng.device)
    st = AudioStreamer(2, engine=eng, formant=[3.0, None], timeout=20)
    assert st._tp is None and st._pt is None and st._stages == [st._fm, st._lv] and st._formant == [P.ratio(3.0), (1, 1)]
    with torch.cuda.stream(eng.stream):
        for k in range(2):
            st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
        st.end()
        want = [eng.apply_level(eng.formant_warp(x[0, 0], 3.0), 0.0, -1.0, 24000), eng.apply_level(x[1, 0], 0.0, -1.0, 24000)]
    eng.sync()
    for idx in range(2):
        got = torch.cat(_collect(st, idx), dim=-1)[0]
        assert torch.equal(got, want[idx].cpu()) and float(got.abs().max()) <= CEILING
    st._thread.join(timeout=20)
    bare = AudioStreamer(1, formant=2.0, timeout=20)
    with pytest.raises(ValueError, match=r"AudioStreamer\(formant=\.\.\.\): device chunks are warped on the device and need an engine"):
        bare.put(x[:1], torch.tensor([0]))
    bare.close()


def test_generate_with_a_formant_kept_streamer_is_graph_safe(small):
    """generate() at toy shapes on the graph engine with AudioStreamer(1, engine=eng, formant=0.0, pitch=+2): the chunks arrive, their
    lengths add up to shift_len of the returned audio's (the warp and the level keep the count), they equal the one-shot calls chained
    over what generate() returns, the stages' launches on the producing stream leave the captured sequences kernel-only (vv_stat 5 = 0),
    and speech_outputs is what generate() returns without the streamer"""
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    eng = small.eng
    cfgd = {"decoder_config": {"max_position_embeddings": small.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
    m.set_speech_factors(small.scaling, small.bias)
    m.set_ddpm_inference_steps(5)
    ids = torch.from_numpy(synth.Gen(78).rng.integers(0, 59, (1, 11)))
    ids[0, -1] = S
    wavs = []
    for streamed in (False, True):
        st = AudioStreamer(1, engine=eng, formant=0.0, pitch=2.0, timeout=20) if streamed else None
        torch.manual_seed(7)
        out = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), cfg_scale=1.3, tokenizer=TOK, generation_config={"do_sample": False},
                         _forced_tokens=[[D, D, D, X]], show_progress_bar=False, audio_streamer=st)
        eng.sync()
        wavs.append(out.speech_outputs[0].detach().float().reshape(-1).cpu())
    assert eng.stat(5) == 0
    assert wavs[0].shape[0] == 3 * 3200 and torch.equal(wavs[0], wavs[1])
    chunks = _collect(st, 0)
    got = torch.cat([c.flatten() for c in chunks])
    assert len(chunks) >= 1 and got.shape == (P.shift_len(3 * 3200, 2.0),)
    want = m.apply_level(m.pitch_shift(wavs[1], 2.0, formant=0.0), 0.0, -1.0)
    torch.cuda.synchronize()
    assert torch.equal(got, want.cpu()) and float(got.abs().max()) <= CEILING
    kept = m.formant_shift(wavs[1], 0.0)
    torch.cuda.synchronize()
    assert torch.equal(kept.cpu(), wavs[1])
