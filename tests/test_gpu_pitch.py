"""GPU tests of the pitch stage (csrc/pitch.hip: vv_pitch_rows, vv_pitch_once, vv_pitch_reset) against vibevoice_amd/pitch.py, of its
chunk invariance and state handling, its 16-bit mode, its refusals, and of AudioStreamer(pitch=...) on device chunks and through
generate().  One engine serves the whole file: the small one of test_gpu_resample.py.

The bound of the kernels against the definition in float64 (resample_ref: the float32 table, f and rho widened) is derived, not measured.
With u = 2^-24, N = 2 Tn + 1 taps, w_t = rho c_t the coefficient of tap t, A1 = max_a sum_t |w_t| and dmax = max_i |H[i + 1] - H[i]|:
  - the coefficient: d = fl(H[i + 1] - H[i]) is off by at most u |d|, c = fma(f, d, H[i]) adds one rounding, u |c|, and w = fl(rho c)
    one more, u |w|: |w_t - w_t,ref| <= (2 |w_t| + rho dmax) u to first order, over a sum at most (2 A1 + N rho dmax) u max|x|;
  - the accumulation: N fma roundings, each of a partial sum of at most A1 max|x|: N A1 u max|x|;
    |y - y_ref| <= ((N + 2) A1 + N rho dmax) * 2^-24 * max|x|
-- 1.9e-5 at 2/1 (129 taps, A1 = 2.3, dmax = 5.6e-3) for inputs in +-1, 9e-6 at 65 taps; 1/1 is the identity and is compared bit for
bit.  A wrong tap, phase or offset is an O(0.1) error on uniform noise.  test_kernel_against_the_definition prints the measured
maximum of every launch shape; on an MI355X: 4.1e-7 to 7.2e-7 over the streaming rows, 3.9e-7 to 7.5e-7 one-shot (12 to 40 times
inside the bound)."""
import math
import types

import numpy as np
import pytest
import torch

import synth
from gpu_util import build_small
from vibevoice_amd import pitch as P
from vibevoice_amd import tempo as T
from vibevoice_amd.engine import EngineError
from vibevoice_amd.streamer import AudioStreamer

pytestmark = pytest.mark.gpu

RATIOS = [(1, 2), (2, 1), (89, 84), (84, 89), (63, 50), (100, 51), (1, 1)]
SEMIS = [12.0 * math.log2(p / q) for p, q in RATIOS]
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


def _bound(p, q, peak=1.0):
    if p == q:
        return 0.0
    H = P.table().astype(np.float64)
    den, tn = max(p, q), P.taps(p, q)
    t = np.arange(-tn, tn + 1)
    a1 = 0.0
    for a in range(q):
        pos = np.abs(a + t * q) * P.R / den
        c = np.where(pos < P.Z * P.R, np.interp(pos, np.arange(H.shape[0]), H), 0.0)
        a1 = max(a1, float(np.abs(c).sum() * q / den))
    n = 2 * tn + 1
    return ((n + 2) * a1 + n * (q / den) * float(np.abs(np.diff(H)).max())) * 2.0 ** -24 * peak


def _noise(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).uniform(-1, 1, shape) * scale).astype(np.float32))


def _push(eng, pt, chunks, ids, semis, flush=False, pcm16=False, cap=None):
    """One push of the rows `chunks` (1-D CPU tensors, lengths may differ: n_in per row) into guarded buffers: a sentinel row above
    and below the output rows and sentinel columns behind every row's count, a sentinel row above and below the input rows.  Checks
    the guards, that the input is unchanged and that the counts are what pitch.counts says -> (per-row outputs, counts)."""
    n, width = len(chunks), max([int(c.shape[0]) for c in chunks] + [1])
    xin = torch.full((n + 2, width), SENTINEL, dtype=torch.float32)
    for i, c in enumerate(chunks):
        xin[1 + i, :c.shape[0]] = c
    fl = [flush] * n if isinstance(flush, bool) else list(flush)
    want = [P.counts(*P.ratio(semis[i]), pt.total[ids[i]], int(chunks[i].shape[0]), fl[i])[1] for i in range(n)]
    assert want == [pt.counts(ids[i], int(chunks[i].shape[0]), semis[i], fl[i]) for i in range(n)]
    cap = max(want) + GUARD if cap is None else cap
    dt = torch.int16 if pcm16 else torch.float32
    sent = int(SENTINEL) if pcm16 else SENTINEL
    xd = xin.to(eng.device)
    out = torch.full((n + 2, cap), sent, dtype=dt, device=eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        _, cnts = pt.push(xd[1:n + 1], ids, semis, flush=fl, out=out[1:n + 1], pcm16=pcm16, n_in=[int(c.shape[0]) for c in chunks])
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

    def _make(n_streams=N_STREAMS):
        made.append(small.eng.pitch(n_streams))
        return made[-1]
    yield _make
    for r in made:
        r.close()


def test_the_semitones_name_the_ratios():
    assert [P.ratio(s) for s in SEMIS] == RATIOS


@pytest.mark.parametrize("n", [1, 3, 8, 17])
def test_kernel_against_the_definition(small, make, n):
    """n rows with non-identity stream ids, row i at ratio RATIOS[(i + n) % 7]: different ratios in the rows of one launch (17 rows: two
    launches).  Row i of step k brings chunk (k + i) % 6 of 1, Tn - 1, Tn, Tn + 1, 700 and 3200 samples of ITS Tn, so the rows of one
    launch stand at different input totals and bring different lengths; pushes that emit nothing occur (asserted); the last step
    flushes -- one row with its last chunk, the others with no samples at all.  Every stream's concatenated output against the
    definition in float64 of its concatenated input, within the derived bound, ceil(n Q / P) samples, the 1/1 rows bit for bit;
    guards around every output row and the input stay untouched (_push)."""
    eng, pt, ids = small.eng, make(), STREAMS[n]
    assert pt.delay_samples == 64 and pt.max_in == P.MAX_IN
    pq = [RATIOS[(i + n) % 7] for i in range(n)]
    semis = [SEMIS[(i + n) % 7] for i in range(n)]
    lens = [[1, max(P.taps(p, q) - 1, 0), P.taps(p, q), P.taps(p, q) + 1, 700, 3200] for p, q in pq]
    sig = [_noise(100 * n + i, sum(lens[i])) for i in range(n)]
    at, got, saw_zero = [0] * n, [[] for _ in range(n)], False
    for k in range(6):
        chunks = []
        for i in range(n):
            c = lens[i][(k + i) % 6]
            chunks.append(sig[i][at[i]:at[i] + c])
            at[i] += c
        outs, cnts = _push(eng, pt, chunks, ids, semis, flush=[k == 5 and i == 0 for i in range(n)])
        saw_zero |= any(c == 0 and ch.shape[0] > 0 for c, ch in zip(cnts, chunks))
        for i in range(n):
            got[i].append(outs[i])
    assert at == [sum(l) for l in lens] and [pt.ratio[i] for i in ids] == pq
    if n > 1:
        outs, _ = _push(eng, pt, [torch.zeros(0)] * (n - 1), ids[1:], semis[1:], flush=True)
        for i in range(1, n):
            got[i].append(outs[i - 1])
    assert saw_zero
    for i, (p, q) in enumerate(pq):
        y = torch.cat(got[i]).numpy()
        ref = P.resample_ref(sig[i].numpy(), p, q)
        assert y.shape == ref.shape == (-(-sum(lens[i]) * q // p),)
        err, bound = float(np.abs(y.astype(np.float64) - ref).max()), _bound(p, q)
        print(f"[pitch n={n} row {i} stream {ids[i]}] {p}/{q}, {2 * P.taps(p, q) + 1} taps: max |gpu - ref| = {err:.3e} (bound {bound:.2e})")
        assert err <= bound, (p, q, err, bound)
        if p == q:
            assert torch.equal(torch.cat(got[i]), sig[i])


def test_chunk_invariance_on_the_device(small, make):
    """the same 3000-sample signal in 1, 3 and 17 pushes (and a flush of no samples), every ratio: bit-identical to
    Engine.pitch_resample, alone and as one row of a launch in which every signal has its own ratio, which is within the kernel bound of
    the definition; a 1/1 row equals its input bit for bit"""
    eng, pt = small.eng, make()
    x = _noise(7, 3000)
    with torch.cuda.stream(eng.stream):
        ones = [eng.pitch_resample(x, s) for s in SEMIS]
        many, counts = eng.pitch_resample(x[None, :].repeat(len(SEMIS), 1), SEMIS)
    eng.sync()
    many = many.cpu()
    for j, ((p, q), s) in enumerate(zip(RATIOS, SEMIS)):
        one, cnt = ones[j][0].cpu(), ones[j][1]
        assert cnt == [counts[j]] == [-(-3000 * q // p)] and one.shape == (counts[j],) and torch.equal(many[j, :counts[j]], one)
        err = float(np.abs(one.numpy().astype(np.float64) - P.resample_ref(x.numpy(), p, q)).max())
        print(f"[pitch once {p}/{q}] max |gpu - ref| = {err:.3e} (bound {_bound(p, q):.2e})")
        assert err <= _bound(p, q)
        if p == q:
            assert torch.equal(one, x)
        for pushes in (1, 3, 17):
            pt.reset([4])
            cuts = np.linspace(0, 3000, pushes + 1).astype(int)
            got = [_push(eng, pt, [x[a:b]], [4], [s])[0][0] for a, b in zip(cuts[:-1], cuts[1:])]
            got.append(_push(eng, pt, [torch.zeros(0)], [4], [s], flush=True)[0][0])
            assert torch.equal(torch.cat(got), one), (p, q, pushes)


def test_pitch_shift_is_time_stretch_then_the_resampler(small):
    """Engine.pitch_shift / model.pitch_shift: shift_ref's length, the tempo stage's offsets are the definition's (so the stretched
    signal is, bit for bit) and the resampler on top is within its bound; no tempo stage where the speeds cancel, no stage at all at 0"""
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    eng = small.eng
    cfgd = {"decoder_config": {"max_position_embeddings": small.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
    x = _noise(31, 5000, scale=0.8)
    for semis, speed in ((4.0, 1.0), (-3.0, 1.25), (7.0, 1.5), (0.0, 1.0), (0.0, 0.8)):
        y = m.pitch_shift(x, semis, speed)
        torch.cuda.synchronize()
        p, q = P.ratio(semis)
        v = P.tempo_speed(speed, semis)
        mid = T.stretch_ref(x.numpy(), v) if T.ratio(v) != (1, 1) else x.numpy()
        assert y.shape == (P.shift_len(5000, semis, speed),) and y.dtype == torch.float32 and y.device == eng.device
        if p == q:
            assert np.array_equal(y.cpu().numpy(), mid)
            continue
        ref = P.resample_ref(mid, p, q)
        err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())
        print(f"[pitch_shift {semis:+g} semitones at speed {speed}] tempo {T.ratio(v)}, ratio {p}/{q}: max |gpu - shift_ref| = {err:.3e}")
        assert err <= _bound(p, q, float(np.abs(mid).max()))
        assert np.array_equal(P.shift_ref(x.numpy(), semis, speed), ref)
    two = eng.pitch_shift(torch.stack([x, -x]), 4.0)
    one = eng.pitch_shift(x, 4.0)
    torch.cuda.synchronize()
    assert torch.equal(two[0], one) and torch.equal(two[1], -one)
    with pytest.raises(ValueError, match="speed=2.0.*semitones=-7.0"):
        eng.pitch_shift(x, -7.0, 2.0)


def test_reset_leaves_no_stale_state_or_ratio(small, make):
    """a loud signal through stream 0 at 2/1, reset([0]), then a quiet one at 84/89: bit-equal to a fresh stage; stream 1, in the
    middle of its own signal, does not notice its neighbour's reset; without the reset the new ratio is refused by name"""
    eng = small.eng
    pt, fresh = make(2), make(2)
    loud, quiet, other = _noise(1, 1000, scale=100.0), _noise(2, 1000, scale=1e-3), _noise(3, 2000)
    _push(eng, pt, [loud, other[:1000]], [0, 1], [SEMIS[1], SEMIS[4]])
    _push(eng, fresh, [other[:1000]], [1], [SEMIS[4]])
    with pytest.raises(EngineError, match=r"stream 0 runs at ratio 2 / 1 since its first push; reset it before it changes to 84 / 89"):
        pt.push(quiet[None, :].to(eng.device), [0], [SEMIS[3]])
    with torch.cuda.stream(eng.stream):
        pt.reset([0])
    assert pt.ratio == [None, RATIOS[4]] and pt.total == [0, 1000]
    a, _ = _push(eng, pt, [quiet, other[1000:]], [0, 1], [SEMIS[3], SEMIS[4]], flush=True)
    b, _ = _push(eng, fresh, [quiet, other[1000:]], [0, 1], [SEMIS[3], SEMIS[4]], flush=True)
    assert a[0].shape[0] == -(-1000 * 89 // 84) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with torch.cuda.stream(eng.stream):
        want, _ = eng.pitch_resample(other, SEMIS[4])
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


def test_int16_mode_is_the_pcm16_rule_on_the_float_rows(small, make):
    """two stages in the same state; one push as float, one as int16 (the same single launch), the rows at three ratios: the int16 rows
    equal the numpy rule applied to the float rows, bit for bit -- a row whose resampled peak exceeds 1 (normalised), one below, one
    of 5 samples"""
    eng = small.eng
    a, b = make(3), make(3)
    semis = [SEMIS[0], SEMIS[2], SEMIS[5]]
    warm = [_noise(10, 500), _noise(11, 500, scale=0.3), _noise(12, 500)]      # the quiet row is quiet from its first sample on
    rows = [_noise(20, 3200, scale=2.5), _noise(21, 3200, scale=0.3), _noise(22, 5, scale=0.9)]
    for pt in (a, b):
        _push(eng, pt, warm, [2, 0, 1], semis)
    f, cf = _push(eng, a, rows, [2, 0, 1], semis)
    q, cq = _push(eng, b, rows, [2, 0, 1], semis, pcm16=True)
    assert cf == cq and float(f[0].abs().max()) > 1.0 and float(f[1].abs().max()) < 1.0
    for got, want in zip(q, _pcm16_rule(f)):
        assert got.dtype == torch.int16 and torch.equal(got, want)
    f, _ = _push(eng, a, [torch.zeros(0)] * 3, [2, 0, 1], semis, flush=True)
    q, _ = _push(eng, b, [torch.zeros(0)] * 3, [2, 0, 1], semis, flush=True, pcm16=True)
    for got, want in zip(q, _pcm16_rule(f)):
        assert torch.equal(got, want)


def test_refusals_write_nothing(small, make):
    """every refusal raises with its message, leaves the sentinel-filled outputs untouched and the streams where they were"""
    import ctypes as C
    from vibevoice_amd import _lib
    eng = small.eng
    pt, twin = make(4), make(4)
    x = _noise(5, 2, 400).to(eng.device)
    out = torch.full((4, 1024), SENTINEL, dtype=torch.float32, device=eng.device)
    first = _noise(6, 300)
    _push(eng, pt, [first], [1], [3.0])
    _push(eng, twin, [first], [1], [3.0])
    _push(eng, pt, [first], [3], [3.0], flush=True)
    cases = [
        (dict(stream_ids=[]), "n = 0 must be in"),
        (dict(stream_ids=[0, 4]), "stream id 4 out of range"),
        (dict(stream_ids=[-1, 0]), "stream id -1 out of range"),
        (dict(stream_ids=[1, 1]), "stream 1 is named twice"),
        (dict(stream_ids=[0, 1], n_in=[400, -1]), "n_in = -1 must be >= 0"),
        (dict(stream_ids=[0, 1], semitones=-12.0, out=out[:, :700].contiguous().fill_(SENTINEL)), "the output rows hold 700"),
        (dict(stream_ids=[0, 3]), "stream 3 has been flushed"),
        (dict(stream_ids=[0, 1], semitones=[3.0, 4.0]), "stream 1 runs at ratio 44 / 37 since its first push"),
    ]
    for kw, msg in cases:
        o = kw.pop("out", out)
        kw.setdefault("semitones", 3.0)
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                pt.push(x, out=o, **kw)
        eng.sync()
        assert bool((o == SENTINEL).all()), msg
    # capacity: a row longer than one push takes, and one whose outputs exceed a launch's, by name; take() cuts either
    long = torch.zeros((1, P.MAX_IN + 1), dtype=torch.float32, device=eng.device)
    big = torch.full((1, 20000), SENTINEL, dtype=torch.float32, device=eng.device)
    for semis, n_in, msg in ((3.0, P.MAX_IN + 1, f"one push takes at most {P.MAX_IN} per row"), (-12.0, 5000, "one push emits at most 8192 per row")):
        with torch.cuda.stream(eng.stream):
            with pytest.raises(EngineError, match=msg):
                pt.push(long, [2], semis, n_in=[n_in], out=big)
        eng.sync()
        assert bool((big == SENTINEL).all()) and pt.ratio[2] is None
        w = pt.take([2], [n_in], False, [semis])
        assert 1 <= w < n_in and P.counts(*P.ratio(semis), 0, w, True)[1] <= P.MAX_OUT
    # P or Q outside 1..100, or a ratio outside [1/2, 2]: only the C entry point can be asked for one
    for bad in ((101, 100), (0, 1), (3, -1), (100, 49), (49, 100)):
        rows = (_lib.VVPitchRow * 1)()
        rows[0].stream, rows[0].n_in, rows[0].flush, rows[0].P, rows[0].Q = 0, 400, 0, bad[0], bad[1]
        cnt = (C.c_int * 1)()
        rc = eng.lib.vv_pitch_rows(eng._ctx, eng._s, pt.slot, 1, rows, C.c_void_p(x.data_ptr()), 400, C.c_void_p(out.data_ptr()), 1024, 0, cnt)
        assert rc != 0 and f"ratio {bad[0]} / {bad[1]} must have both terms in [1,100]" in eng._err()
    eng.sync()
    assert bool((out == SENTINEL).all())
    with pytest.raises(EngineError, match="configuration 9 is not set"):
        eng._chk(eng.lib.vv_pitch_reset(eng._ctx, eng._s, 9, 1, None), "vv_pitch_reset")
    with pytest.raises(ValueError, match="13"):
        pt.push(x, [0, 2], [1.0, 13.0], out=out)
    assert pt.total == [0, 300, 0, 300] and pt.ratio == [None, (44, 37), None, (44, 37)]
    # the refused calls changed no state: stream 1 goes on exactly like its twin, stream 3 pushes again after its reset
    nxt = _noise(8, 400)
    a, _ = _push(eng, pt, [nxt], [1], [3.0], flush=True)
    b, _ = _push(eng, twin, [nxt], [1], [3.0], flush=True)
    assert torch.equal(a[0], b[0])
    with torch.cuda.stream(eng.stream):
        pt.reset([3])
    a, _ = _push(eng, pt, [nxt], [3], [-4.0], flush=True)
    with torch.cuda.stream(eng.stream):
        want, _ = eng.pitch_resample(nxt, -4.0)
    eng.sync()
    assert torch.equal(a[0], want.cpu())


def _collect(st, idx):
    return list(st.get_stream(idx))


def test_streamer_pitch_speed_48k_int16_end_to_end(small):
    """AudioStreamer(2, pcm16=eng, pitch=[+12, -5], speed=[1.0, 0.8], sample_rate=48000, ceiling_db=-1) on device chunks of 3200, three
    puts and end(): per sample index, the delivered int16 chunks equal the pcm16 rule applied chunk by chunk to what the float streamer
    (engine=eng) delivers, whose concatenation is the one-shot engine calls chained -- pitch_shift, resample, apply_level -- bit for bit;
    the stages sit in the order tempo, pitch, resampler, level and give their configurations back"""
    eng = small.eng
    x = _noise(9, 2, 1, 3 * 3200, scale=0.9).to(eng.device)
    kw = dict(pitch=[12.0, -5.0], speed=[1.0, 0.8], sample_rate=48000, ceiling_db=-1.0, timeout=20)
    sts = [AudioStreamer(2, pcm16=eng, **kw), AudioStreamer(2, engine=eng, **kw)]
    for st in sts:
        assert st._stages == [st._tp, st._pt, st._rs, st._lv] and None not in st._stages
        assert st._speeds == [0.5, P.tempo_speed(0.8, -5.0)]
    with torch.cuda.stream(eng.stream):
        for st in sts:
            for k in range(3):
                st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
            st.end()
        want = [eng.apply_level(eng.resample(eng.pitch_shift(x[i, 0], s, v), 24000, 48000), 0.0, -1.0, 48000) for i, (s, v) in enumerate(((12.0, 1.0), (-5.0, 0.8)))]
    eng.sync()
    for idx, (s, v) in enumerate(((12.0, 1.0), (-5.0, 0.8))):
        q, f = _collect(sts[0], idx), _collect(sts[1], idx)
        assert len(q) == len(f) >= 3 and all(c.dtype == torch.int16 for c in q) and all(c.dtype == torch.float32 for c in f)
        assert [c.shape for c in q] == [c.shape for c in f] and all(c.dim() == 2 and c.shape[0] == 1 and c.shape[1] > 0 for c in f)
        cat = torch.cat(f, dim=-1)[0]
        assert cat.shape[0] == 2 * P.shift_len(3 * 3200, s, v) and torch.equal(cat, want[idx].cpu())
        for got, rule in zip(q, _pcm16_rule([c[0] for c in f])):
            assert torch.equal(got[0], rule)
    for st in sts:
        st._thread.join(timeout=20)
    assert eng._pt_used == [None] * 4 and eng._tp_used == [None] * 4 and eng._rs_used == [None] * 4 and eng._lv_used == [None] * 4


def test_streamer_unshifted_index_passes_bit_for_bit_and_device_chunks_need_an_engine(small):
    """pitch=[+3, 0]: index 1 runs through the pitch stage at 1/1 (and through no tempo change worth the name: speed 1) and arrives as it
    was put; speed 1.5 with +7 semitones builds no tempo stage; without an engine device chunks are refused by name"""
    eng = small.eng
    x = _noise(14, 2, 1, 2 * 3200).to(eng.device)
    st = AudioStreamer(2, engine=eng, pitch=[7.0, 0.0], speed=[1.5, 1.0], timeout=20)
    assert st._tp is None and st._stages == [st._pt]
    with torch.cuda.stream(eng.stream):
        for k in range(2):
            st.put(x[:, :, k * 3200:(k + 1) * 3200], torch.tensor([0, 1]))
        st.end()
        want, _ = eng.pitch_resample(x[0, 0], 7.0)
    eng.sync()
    assert torch.equal(torch.cat(_collect(st, 1), dim=-1)[0], x[1, 0].cpu())
    assert torch.equal(torch.cat(_collect(st, 0), dim=-1)[0], want.cpu())
    st._thread.join(timeout=20)
    bare = AudioStreamer(1, pitch=2.0, timeout=20)
    with pytest.raises(ValueError, match=r"AudioStreamer\(pitch=\.\.\.\): device chunks are shifted on the device and need an engine"):
        bare.put(x[:1], torch.tensor([0]))
    bare.close()


def test_generate_with_a_shifted_streamer_is_graph_safe(small):
    """generate() at toy shapes on the graph engine with AudioStreamer(1, engine=eng, pitch=+2): the delivered audio has shift_ref's
    count, equals Engine.pitch_shift of what generate() returns, and the stages' launches on the producing stream leave the captured
    sequences kernel-only (vv_stat 5 = 0)"""
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    eng = small.eng
    cfgd = {"decoder_config": {"max_position_embeddings": small.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
    m.set_speech_factors(small.scaling, small.bias)
    m.set_ddpm_inference_steps(5)
    ids = torch.from_numpy(synth.Gen(78).rng.integers(0, 59, (1, 11)))
    ids[0, -1] = S
    st = AudioStreamer(1, engine=eng, pitch=2.0, timeout=20)
    torch.manual_seed(7)
    out = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), cfg_scale=1.3, tokenizer=TOK, generation_config={"do_sample": False},
                     _forced_tokens=[[D, D, D, X]], show_progress_bar=False, audio_streamer=st)
    eng.sync()
    assert eng.stat(5) == 0
    wav = out.speech_outputs[0].detach().float().reshape(-1)
    assert wav.shape[0] == 3 * 3200
    got = torch.cat([c.flatten() for c in _collect(st, 0)])
    assert got.shape == (P.shift_len(3 * 3200, 2.0),) == P.shift_ref(wav.cpu().numpy(), 2.0).shape
    want = m.pitch_shift(wav, 2.0)
    torch.cuda.synchronize()
    assert torch.equal(got, want.cpu())
