"""Prompt prefixes on the engine: vv_kv_export / vv_kv_snapshot / vv_kv_restore (csrc/kvspan.hip) against vv_kv_import_at and the
span prefill, and generate(prompt_prefix=...) against the oracle loop.

Bounds.  The copies are exact: torch.equal.  A suffix pass over a restored prefix runs the same kernels on the same data as the
in-place chunked pass: torch.equal.  Against the oracle LM (kv_round_bf16=True) the suffix rows are held to what the span prefill is
held to elsewhere: 3e-4 in the fp32-exact mode (test_gpu_kernels.py::test_lm_prefill_decode_and_logits, which runs xsplit = 3 only)
and 3e-2 in the bf16 mode (test_gpu_geometry.py::test_one_layer_at_real_widths, the suite's bound for xsplit = 1).  generate():
test_gpu_generate.py's own bounds (tokens identical, latents / negative hidden states 5e-3, waveforms 1e-2).
"""
import ctypes as C
import types

import pytest
import torch

import lm_shapes as ls
import synth
from gpu_util import build_small, rel_err
from oracle import generate as ogen
from test_gpu_generate import TOK, check, make_inputs
from test_gpu_geometry import GEOM, build_fast
from test_gpu_kernels import LM_CASES, _fill_past

pytestmark = pytest.mark.gpu

D, E, S, X = TOK.speech_diffusion_id, TOK.speech_end_id, TOK.speech_start_id, TOK.eos_token_id
NS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100]
SENT = 5.0                                   # a finite, bf16-exact sentinel


@pytest.fixture(scope="module")
def engs():
    """the small GQA model (3 layers, 2 kv heads x 64) per xsplit, built on first use: 2 slots = caches 0..3"""
    made = {}

    def get(xs):
        if xs not in made:
            made[xs] = build_small(LM_CASES[ls.SUFFIX_ENGINE[0]], xsplit=xs, n_slots=2, max_ctx=512, max_rows=ls.SUFFIX_ENGINE[1])
        return made[xs]
    yield get
    for s in made.values():
        s.eng.close()


def _bf16_rand(shape, seed, eng):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g).to(torch.bfloat16).to(torch.float32).to(eng.device)
    torch.cuda.synchronize()
    return t


def _fill(eng, cfg, cache, value):
    t = torch.full((cfg.kv_heads, eng.max_ctx, cfg.head_dim), float(value), device=eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        for layer in range(cfg.layers):
            eng.kv_import_at(cache, layer, 0, t, t)
    eng.sync()


def _export_all(eng, cfg, cache, pos0, n, dtype=torch.float32):
    with torch.cuda.stream(eng.stream):
        out = [eng.kv_export(cache, layer, pos0, n, dtype=dtype) for layer in range(cfg.layers)]
    eng.sync()
    return out


def _ceil32(n):
    return (n + 31) // 32 * 32


def _export_inverse(eng, cfg, cache, ns, pos0s):
    """case 1 on one engine: import at [pos0, pos0 + n), export the same span in both dtypes, the rest keeps the sentinel"""
    kvh, hd = cfg.kv_heads, cfg.head_dim
    _fill(eng, cfg, cache, SENT)
    sent = torch.full((kvh, eng.max_ctx, hd), SENT, device=eng.device)
    bad = []
    for pos0 in pos0s:
        for n in ns:
            k = [_bf16_rand((kvh, n, hd), 1000 * pos0 + 10 * n + layer, eng) for layer in range(cfg.layers)]
            v = [_bf16_rand((kvh, n, hd), 1000 * pos0 + 10 * n + layer + 5, eng) for layer in range(cfg.layers)]
            with torch.cuda.stream(eng.stream):
                for layer in range(cfg.layers):
                    eng.kv_import_at(cache, layer, pos0, k[layer], v[layer])
            f32 = _export_all(eng, cfg, cache, pos0, n, torch.float32)
            b16 = _export_all(eng, cfg, cache, pos0, n, torch.bfloat16)
            whole = _export_all(eng, cfg, cache, 0, eng.max_ctx, torch.float32)
            for layer in range(cfg.layers):
                ok = (torch.equal(f32[layer][0], k[layer]) and torch.equal(f32[layer][1], v[layer])
                      and b16[layer][0].dtype == torch.bfloat16 and torch.equal(b16[layer][0].float(), k[layer])
                      and torch.equal(b16[layer][1].float(), v[layer]))
                for t in whole[layer]:                      # outside the span: the sentinel, untouched
                    ok = ok and torch.equal(t[:, :pos0], sent[:, :pos0]) and torch.equal(t[:, pos0 + n:], sent[:, pos0 + n:])
                ok = ok and torch.equal(whole[layer][0][:, pos0:pos0 + n], k[layer]) and torch.equal(whole[layer][1][:, pos0:pos0 + n], v[layer])
                if not ok:
                    bad.append((pos0, n, layer))
            with torch.cuda.stream(eng.stream):             # back to the sentinel for the next case
                for layer in range(cfg.layers):
                    eng.kv_import_at(cache, layer, pos0, sent[:, :n], sent[:, :n])
            eng.sync()
    return bad


# ---------------------------------------------------------------- 1. export is the inverse of import
def test_export_is_the_inverse_of_import(engs):
    s = engs(3)
    bad = _export_inverse(s.eng, s.lmcfg, 1, NS, (0, 5, 16, 33))
    assert not bad, f"(pos0, n, layer) whose export differs from what was imported: {bad}"
    assert s.eng.stat(5) == 0


def _snapshot_restore(src, cfg, a, targets, ns, L):
    """case 2: cache `a` of engine `src` holds a real prefill of L positions; every (engine, cache) of `targets` is filled with the
    sentinel, takes the restore, and must hold A's n positions, zeros up to ceil32(n) and the sentinel beyond."""
    H = cfg.hidden
    x = synth.Gen(41).normal((L, H), 1.0, mat=False).to(src.device)
    torch.cuda.synchronize()
    hid = src.new(L, H)
    with torch.cuda.stream(src.stream):
        src.lm_forward_span(a, 0, L, x, hid)
    src.sync()
    ref = _export_all(src, cfg, a, 0, L)
    assert all(float(k.abs().sum()) > 0 and float(v.abs().sum()) > 0 for k, v in ref)
    bad = []
    for n in ns:
        with torch.cuda.stream(src.stream):
            ks, vs = src.kv_snapshot(a, n)
        src.sync()
        assert ks.dtype == torch.bfloat16 and ks.shape == (cfg.layers, cfg.kv_heads, _ceil32(n) * cfg.head_dim) and vs.shape == ks.shape
        for ti, (eng, b) in enumerate(targets):
            _fill(eng, cfg, b, SENT)
            with torch.cuda.stream(eng.stream):
                eng.kv_restore(b, n, ks, vs)
            got = _export_all(eng, cfg, b, 0, eng.max_ctx)
            c = _ceil32(n)
            for layer in range(cfg.layers):
                (k, v), (rk, rv) = got[layer], ref[layer]
                ok = torch.equal(k[:, :n], rk[:, :n]) and torch.equal(v[:, :n], rv[:, :n])
                ok = ok and bool((v[:, n:c] == 0).all()) and bool((k[:, n:c] == 0).all())
                ok = ok and bool((k[:, c:] == SENT).all()) and bool((v[:, c:] == SENT).all())
                if not ok:
                    bad.append((n, ti, layer))
    return bad


# ---------------------------------------------------------------- 2. snapshot and restore are exact and confined
def test_snapshot_restore_exact_and_confined(engs):
    s = engs(3)
    eng, cfg = s.eng, s.lmcfg
    child = eng.fork(max_ctx=256, n_slots=1)              # another max_ctx: other head / layer strides
    try:
        assert child.max_ctx != eng.max_ctx
        bad = _snapshot_restore(eng, cfg, 0, [(eng, 2), (child, 0)], NS, 128)
        assert not bad, f"(n, target, layer) where the restored cache is not the source's: {bad}"
        assert eng.stat(5) == 0 and child.stat(5) == 0
    finally:
        child.close()


def test_seven_b_attention_geometry():
    """one layer, 4 kv heads x 128 (test_gpu_geometry.py's 7B config): the d = 128 tile indexing of all three copy kernels"""
    c = GEOM["7b"]
    s = build_fast(c, xsplit=1, n_slots=2, max_ctx=256, max_rows=128, head_layers=1)
    eng = s.eng
    child = eng.fork(max_ctx=128, n_slots=1)
    try:
        bad = _export_inverse(eng, c, 1, [1, 17, 33, 100], (0, 5, 33))
        assert not bad, bad
        bad = _snapshot_restore(eng, c, 0, [(eng, 2), (child, 0)], [1, 16, 31, 33, 65, 100], 128)
        assert not bad, bad
    finally:
        child.close()
        eng.close()


# ---------------------------------------------------------------- 3. a snapshot is clean whatever lay behind it
@pytest.mark.parametrize("xs", [1, 3])
def test_snapshot_is_clean_whatever_lay_behind_it(engs, xs):
    s = engs(xs)
    eng, cfg = s.eng, s.lmcfg
    H = cfg.hidden
    bad = []
    for n, m in ((37, 20), (5, 3), (64, 70)):
        x = synth.Gen(900 + n).normal((n + m, H), 1.0, mat=False).to(eng.device)
        torch.cuda.synchronize()

        def run(poison):
            hid = eng.new(n, H)
            out = eng.new(m, H)
            _fill(eng, cfg, 2, 0.0)
            with torch.cuda.stream(eng.stream):
                eng.lm_forward_span(0, 0, n, x[:n], hid)
                _fill_past(eng, cfg, 0, n, poison)          # NaN / Inf (or zeros) in every slot behind the prefix
                ks, vs = eng.kv_snapshot(0, n)
                eng.kv_restore(2, n, ks, vs)
                eng.lm_forward_span(2, n, m, x[n:], out)
            eng.sync()
            return out.clone(), ks.float().clone(), vs.float().clone()
        (c_out, c_k, c_v), (d_out, d_k, d_v) = run(False), run(True)
        if not (bool(torch.isfinite(d_out).all()) and torch.equal(c_out, d_out) and torch.equal(c_k, d_k) and torch.equal(c_v, d_v)):
            bad.append((n, m))
    assert not bad, f"(n, m) where what lay behind the prefix reached the snapshot or the suffix pass: {bad}"


# ---------------------------------------------------------------- 4. suffix over a restored prefix == the in-place chunked pass
@pytest.mark.parametrize("xs,tol", [(1, 3e-2), (3, 3e-4)])
def test_suffix_over_a_restored_prefix_equals_the_chunked_pass(engs, xs, tol):
    """suffixes of 1 row (a decode row: fused attention), 2..7 rows (split + merge attention), 8..63 rows (vv_attn_prefill4 in the bf16
    mode) and >= 64 rows (the packed prefill), starting on and off the 16- / 32- / 64-position grids.  The spans: tests/lm_shapes.py;
    test_pass_plan_cpu.py asserts that each takes the route named here"""
    s = engs(xs)
    eng, cfg = s.eng, s.lmcfg
    H = cfg.hidden
    om = s.oracle_lm(kv_round_bf16=True)
    unequal, errs = [], {}
    for n, m in ls.SUFFIX_SPANS:
        xc = synth.Gen(300 + n + m).normal((n + m, H), 1.0, mat=False)
        x = xc.to(eng.device)
        torch.cuda.synchronize()
        hid_c, hid_a, hid_b = eng.new(n + m, H), eng.new(n, H), eng.new(m, H)
        with torch.cuda.stream(eng.stream):
            eng.lm_forward_span(0, 0, n, x[:n], hid_c[:n])
            eng.lm_forward_span(0, n, m, x[n:], hid_c[n:])
            eng.lm_forward_span(1, 0, n, x[:n], hid_a)
            ks, vs = eng.kv_snapshot(1, n)
            eng.kv_restore(2, n, ks, vs)
            eng.lm_forward_span(2, n, m, x[n:], hid_b)
        eng.sync()
        if not (torch.equal(hid_a, hid_c[:n]) and torch.equal(hid_b, hid_c[n:])):
            unequal.append((n, m))
        ref = om.forward(xc, om.new_cache())
        errs[(n, m)] = rel_err(hid_b, ref[n:])
    print("suffix rows vs the oracle LM, rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert not unequal, f"(n, m) where the suffix pass over a restored prefix differs from the in-place pass: {unequal}"
    assert all(v <= tol for v in errs.values()), errs


# ---------------------------------------------------------------- 5. generate() with a prefix vs the oracle loop
@pytest.fixture(scope="module")
def sm():
    s = build_small(synth.LMCfg(), xsplit=3, n_slots=2, max_ctx=512)
    yield s
    s.eng.close()


def _model(s, steps=5, eng=None):
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfgd = {"decoder_config": {"max_position_embeddings": s.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": steps},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, eng or s.eng, model_dtype=torch.float32)
    m.set_speech_factors(s.scaling, s.bias)
    m.set_ddpm_inference_steps(steps)
    return m


HTOK = types.SimpleNamespace(speech_start_id=S, speech_end_id=E, speech_diffusion_id=D, eos_token_id=X, bos_token_id=None,
                             pad_token_id=TOK.pad_token_id)


class _Case:
    """test_gpu_generate.run_both's recipe (forced plan, fixed noise, _prefill_noise, with_speech=True), the oracle side computed once"""

    def __init__(self, s, B, forced, seed):
        self.s, self.B, self.forced, self.seed = s, B, forced, seed
        self.ids, self.mask, self.sim, self.st, self.sm = make_inputs(s, B, True, seed)
        g = synth.Gen(seed + 1)
        self.bank = {}
        self.pre = (g.normal((B,), 1.0, mat=False), g.normal((B, 3, 64), 1.0, mat=False))
        self.otr = ogen.Trace()
        self.oracle = ogen.oracle_generate(s.oracle_model(kv_round_bf16=True), TOK, self.ids, self.mask, self.st, self.sm, self.sim, cfg_scale=1.3,
                                           num_steps=5, max_new_tokens=None, noise_fn=self.noise_fn, prefill_noise=self.pre,
                                           forced_tokens=forced, trace=self.otr)

    def noise_fn(self, step, n2):
        if (step, n2) not in self.bank:
            self.bank[(step, n2)] = synth.Gen(self.seed * 1000 + step).normal((n2, 64), 1.0, mat=False)
        return self.bank[(step, n2)]

    def row(self, b):
        return dict(input_ids=self.ids[b:b + 1], attention_mask=self.mask[b:b + 1], speech_input_mask=self.sim[b:b + 1],
                    speech_tensors=self.st[b:b + 1], speech_masks=self.sm[b:b + 1])

    def prefix(self, m, b):
        return m.build_prompt_prefix(**self.row(b), _prefill_noise=(self.pre[0][b:b + 1], self.pre[1][b:b + 1]))

    def generate(self, m, prompt_prefix):
        htr = ogen.Trace()
        out = m.generate(input_ids=self.ids, attention_mask=self.mask, speech_tensors=self.st, speech_masks=self.sm, speech_input_mask=self.sim,
                         cfg_scale=1.3, tokenizer=HTOK, max_new_tokens=None, generation_config={"do_sample": False},
                         _forced_tokens=self.forced, _noise_fn=self.noise_fn, _prefill_noise=self.pre, _trace=htr, show_progress_bar=False,
                         prompt_prefix=prompt_prefix)
        return out, htr

    def check(self, out, htr):
        oseq, oaud, omax = self.oracle
        check((oseq, oaud, omax, self.otr), (out, htr))


class _CountEncoder:
    def __init__(self, eng):
        self.eng, self.n, self.inner = eng, 0, eng.acoustic_encode

    def __enter__(self):
        def counted(*a, **k):
            self.n += 1
            return self.inner(*a, **k)
        self.eng.acoustic_encode = counted
        return self

    def __exit__(self, *a):
        del self.eng.acoustic_encode


@pytest.fixture(scope="module")
def case_b1(sm):
    return _Case(sm, 1, [[D, D, D, D, E, S, D, D, D, X]], 11)


@pytest.fixture(scope="module")
def case_b2(sm):
    return _Case(sm, 2, [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]], 23)       # rows desynchronise


def test_generate_with_a_prefix_single(sm, case_b1):
    m = _model(sm)
    p = case_b1.prefix(m, 0)
    assert (p.n_pos, p.speech_pos) == (5, [3, 4])
    with _CountEncoder(sm.eng) as enc:
        out, htr = case_b1.generate(m, p)
    assert enc.n == 0
    assert m.last_stats["prefix_rows_reused"] == 5 and m.last_stats["prompt_rows_computed"] == 16
    case_b1.check(out, htr)
    assert out.speech_outputs[0].shape[-1] == 7 * 3200


def test_generate_with_prefixes_batch2_desync(sm, case_b2):
    m = _model(sm)
    p = [case_b2.prefix(m, 0), case_b2.prefix(m, 1)]
    assert (p[1].n_pos, p[1].speech_pos) == (6, [3, 4, 5])
    with _CountEncoder(sm.eng) as enc:
        out, htr = case_b2.generate(m, p)
    assert enc.n == 0
    assert m.last_stats["prefix_rows_reused"] == 11 and m.last_stats["prompt_rows_computed"] == 16 + 11
    case_b2.check(out, htr)


def test_generate_batch2_one_row_without_a_prefix(sm, case_b2):
    m = _model(sm)
    p0 = case_b2.prefix(m, 0)
    with _CountEncoder(sm.eng) as enc:
        out, htr = case_b2.generate(m, [p0, None])
    assert enc.n == 1                                     # row 1's voice sample, and only it
    assert m.last_stats["prefix_rows_reused"] == 5 and m.last_stats["prompt_rows_computed"] == 16 + 17
    case_b2.check(out, htr)


def test_continuous_admission_restores_prefixes_into_reused_slots(sm, case_b2):
    """5 requests over 2 slots, each starting with its row's prefix: a restore lands in a slot another request has just left"""
    c = case_b2
    m = _model(sm)
    pf = [c.prefix(m, 0), c.prefix(m, 1)]
    plans = [[D, D, D, X], [D, E, S, D, D, X], [D, D, X], [D, D, D, D, E, X], [D, X]]
    reqs = []
    for i, plan in enumerate(plans):
        b = i % 2
        keep = c.mask[b].bool()
        bank = {st: synth.Gen(5000 + 100 * i + st).normal((2, 64), 1.0, mat=False) for st in range(16)}
        reqs.append(dict(input_ids=c.ids[b:b + 1][:, keep], attention_mask=c.mask[b:b + 1][:, keep], speech_input_mask=c.sim[b:b + 1][:, keep],
                         speech_tensors=c.st[b:b + 1], speech_masks=c.sm[b:b + 1], _prefill_noise=(c.pre[0][b:b + 1], c.pre[1][b:b + 1]),
                         _forced_tokens=plan, _noise_fn=(lambda nz: (lambda step, n2: nz[step]))(bank), prompt_prefix=pf[b]))
    with _CountEncoder(sm.eng) as enc:
        outs = m.generate_continuous(reqs, tokenizer=HTOK, generation_config={"do_sample": False}, cfg_scale=1.3)
    assert enc.n == 0
    assert m.last_stats["max_in_flight"] == 2 and len(m.last_stats["admissions"]) == 5
    assert m.last_stats["prefix_rows_reused"] == 5 + 6 + 5 + 6 + 5
    om = sm.oracle_model(kv_round_bf16=True)
    for r, o in zip(reqs, outs):
        oseq, oaud, omax = ogen.oracle_generate(om, TOK, r["input_ids"], r["attention_mask"], r["speech_tensors"], r["speech_masks"],
                                                r["speech_input_mask"], cfg_scale=1.3, num_steps=5, noise_fn=r["_noise_fn"],
                                                prefill_noise=r["_prefill_noise"], forced_tokens=[r["_forced_tokens"]])
        assert torch.equal(o.sequences.cpu(), oseq)
        assert rel_err(o.speech_outputs[0][0], oaud[0][0]) <= 1e-2, rel_err(o.speech_outputs[0][0], oaud[0][0])


def test_a_forked_lane_restores_the_parents_prefix(sm, case_b1):
    """a prefix is device resident and belongs to the weight copy: a fork() with another max_ctx uses the parent's"""
    m = _model(sm)
    p = case_b1.prefix(m, 0)
    lane = m.fork(max_ctx=256, n_slots=1)
    try:
        out, htr = case_b1.generate(lane, p)
        assert lane.last_stats["prefix_rows_reused"] == 5
        case_b1.check(out, htr)
    finally:
        lane.engine.close()


# ---------------------------------------------------------------- 6. save and load
def test_save_and_load(sm, case_b1, tmp_path):
    from vibevoice_amd import PromptPrefix
    m = _model(sm)
    p = case_b1.prefix(m, 0)
    out, _ = case_b1.generate(m, p)
    path = str(tmp_path / "voice.pt")
    p.save(path)
    q = PromptPrefix.load(path, m)
    assert (q.n_pos, q.ids, q.speech_pos, q.geometry) == (p.n_pos, p.ids, p.speech_pos, p.geometry)
    assert torch.equal(q.k, p.k) and torch.equal(q.v, p.v)
    out2, htr2 = case_b1.generate(m, q)
    assert torch.equal(out2.sequences, out.sequences)
    assert torch.equal(out2.speech_outputs[0], out.speech_outputs[0])
    case_b1.check(out2, htr2)


# ---------------------------------------------------------------- 7. refusals
def test_refusals(sm, case_b1):
    from vibevoice_amd.engine import EngineError
    c, eng = case_b1, sm.eng
    m = _model(sm)
    p = c.prefix(m, 0)
    ids = c.ids.clone()
    ids[0, 1] += 1
    with pytest.raises(ValueError, match="position 1"):
        m.generate(input_ids=ids, attention_mask=c.mask, speech_tensors=c.st, speech_masks=c.sm, speech_input_mask=c.sim, cfg_scale=1.3,
                   tokenizer=HTOK, generation_config={"do_sample": False}, _forced_tokens=c.forced, _noise_fn=c.noise_fn,
                   _prefill_noise=c.pre, show_progress_bar=False, prompt_prefix=p)
    eng.sync()
    # the same parameters uploaded again: the values do not change, the epoch does
    m.load_state_dict({"model.language_model.norm.weight": sm.lm_w["norm.weight"]}, strict=False)
    with pytest.raises(RuntimeError, match="stale"):
        c.generate(m, p)
    out, htr = c.generate(m, c.prefix(m, 0))              # rebuilt: accepted, and still the oracle's result
    c.check(out, htr)
    # the ABI refuses spans beyond max_ctx with a message and stays usable
    too_many = eng.max_ctx + 1
    assert eng.lib.vv_kv_snapshot_bytes(eng._ctx, too_many) < 0 and b"max_ctx" in eng.lib.vv_last_error(eng._ctx)
    buf = torch.zeros(1 << 20, dtype=torch.bfloat16, device=eng.device)
    torch.cuda.synchronize()
    for fn in (eng.lib.vv_kv_snapshot, eng.lib.vv_kv_restore):
        rc = fn(eng._ctx, eng._s, 0, too_many, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()))
        assert rc < 0 and b"max_ctx" in eng.lib.vv_last_error(eng._ctx)
    assert eng.lib.vv_kv_snapshot(eng._ctx, eng._s, 4, 8, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr())) < 0      # 2 slots: caches 0..3
    with pytest.raises(EngineError, match="max_ctx"):
        eng.kv_export(0, 0, eng.max_ctx - 4, 8)
    with pytest.raises(EngineError, match="layer"):
        eng.kv_export(0, sm.lmcfg.layers, 0, 8)
    with pytest.raises(EngineError):
        eng.kv_restore(0, 8, buf[:16], buf[:16])          # not a snapshot of 8 positions
    eng.sync()
    out, htr = c.generate(m, c.prefix(m, 0))
    c.check(out, htr)
    assert eng.stat(5) == 0
