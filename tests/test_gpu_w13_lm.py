"""W13 for the LM's decode launches and the per-tile-row fall-back inside every W13 form (csrc/gemv.hip: WF; csrc/gemv_plan.h:
vv_gemv_w13_forms; the twins of csrc/engine.hip).  Equality of bits is the whole oracle, as in test_gpu_w13.py: the bf16 route is held
to fp64 elsewhere.  Outputs are compared as int32 patterns, so that a planted infinity (inf and NaN outputs) is compared too.

  new forms    QKV (RMS + bias, 2 rows x 4 waves, N = 288), gate/up (RMS + SwiGLU, 2 x 4) and o / down (residual, 4 x 8) over the twins
               against the same form over the bf16 fragments, 2 rows: K = 256 (2 groups over 4 waves), K = 1152 (9 groups over 8 waves:
               ranges that start and end inside a group), K = 128 (waves without K)
  fall-back    every W13 form, one element the format cannot hold (a denormal, 31 binades under the row's largest, an infinity) in one
               tile row; SwiGLU: in gate, in up, in both in different tile rows.  The output is the bf16 form's; it does not change
               when that row's planes are overwritten with 0xFF, nor when every OTHER row's bf16 fragments are replaced: the row reads
               bf16, the others read planes.  All reads stay inside the allocations.  A matrix without one ok row equals bf16 too
  engine       an LM whose widths qualify (hidden 256 / 384, inter 1152), VVHIP_W13 = 1 / head / 0: LM decode of 1 and 2 rows, eager
               and graphed (first sight, capture, replay), equal across the arms; vv_stat 10 / 9 / 11; after re-uploading one down
               matrix, after planting a denormal in it, after set_adapter() on a q_proj and a down_proj target and after its reset.
               At these widths only the down projection takes a W13 form (the others get the default 8-wave form; o keeps bf16)
  wide engine  hidden 256 with 32 heads x 128 (QKV: 5120 features) and inter 4224: QKV and gate/up get the 2-row 4-wave forms, as at
               7B.  The profile window of one LM pass is smaller than with VVHIP_W13=0 by exactly 3/16 of the matrices that
               stream planes (gate and up of every layer, QKV of the first: later ones consume the split down projection's parts); the same upload / denormal / set_adapter steps on q_proj and gate_proj"""
import os

import numpy as np
import pytest
import torch

import synth
import w13_cases as WC
from gpu_util import build_small
from vibevoice_amd import w13

pytestmark = pytest.mark.gpu

NONE, RMS, RMS_MOD = 0, 1, 2
BIAS, SWIGLU, RESID, GATED = 1, 3, 4, 5
EPS = 1e-5
# every W13 form of gemv_plan.h: (prologue, epilogue, (rows, waves))
OLD_FORMS = {"head gate/up 2x4": (RMS_MOD, SWIGLU, (2, 4)), "head gate/up 4x8": (RMS_MOD, SWIGLU, (4, 8)), "head down": (NONE, GATED, (4, 8))}
NEW_FORMS = {"qkv": (RMS, BIAS, (2, 4)), "lm gate/up": (RMS, SWIGLU, (2, 4)), "o/down": (NONE, RESID, (4, 8))}
FORMS = {**OLD_FORMS, **NEW_FORMS}


@pytest.fixture(scope="module")
def eng():
    s = build_small(synth.LMCfg(), xsplit=1)
    yield s.eng
    s.eng.close()


def _pack(eng, w):
    packed = eng.pack_matrix(w.float())
    twin = eng.w13_pack(packed, *w.shape)
    eng.sync()
    return packed, twin


def _rows(eng, seed, T, width, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, width, generator=g) * scale).to(eng.device)


def _bits(y):
    return y.contiguous().view(torch.int32)


def _launch(eng, form, N, K, gate, up, twins):
    """one launch of the W13 form over (packed, twin) pairs gate [, up]: over the twins, or (twins False) over the bf16 fragments"""
    pro, epi, shape = FORMS[form]
    x = _rows(eng, 1, 2, K)
    y = _rows(eng, 7, 2, N).clone() if epi in (RESID, GATED) else torch.full((2, N), 7.0, device=eng.device)
    kw = dict(pro=pro, epi=epi, xsplit=1, w13_form=shape, twin=gate[1] if twins else None)
    if pro in (RMS, RMS_MOD):
        kw.update(nw=_rows(eng, 4, 1, K).reshape(-1) * 0.1 + 1.0, eps=EPS)
    if pro == RMS_MOD:
        kw.update(mod_scale=_rows(eng, 2, 2, K, 0.3), mod_shift=_rows(eng, 3, 2, K, 0.5), ld_mod=K)
    if epi == SWIGLU:
        kw.update(w2p=up[0], twin2=up[1] if twins else None)
    if epi == BIAS:
        kw.update(bias=_rows(eng, 8, 1, N).reshape(-1))
    if epi == RESID:
        kw.update(bias=_rows(eng, 8, 1, N).reshape(-1), nscale=_rows(eng, 9, 1, N).reshape(-1) * 0.1 + 1.0)
    if epi == GATED:
        kw.update(gate=_rows(eng, 6, 2, N, 0.5), ld_gate=N)
    assert eng.gemv_case(gate[0], x, y, 2, N, K, **kw) == (1, *shape, 0, 0)
    eng.sync()
    return y


@pytest.mark.parametrize("form,N,K", [("qkv", 288, 256), ("qkv", 288, 1152), ("qkv", 288, 128),
                                      ("lm gate/up", 768, 256), ("lm gate/up", 1152, 384), ("lm gate/up", 384, 128),
                                      ("o/down", 256, 1152), ("o/down", 256, 256), ("o/down", 384, 768), ("o/down", 384, 128)])
def test_new_form_gives_the_bits_of_bf16(eng, form, N, K):
    gate, up = _pack(eng, WC.weights(N, K, 500 + N + K)), _pack(eng, WC.weights(N, K, 600 + N + K))
    for m in (gate, up):          # no tile row falls back: the twins are what is read
        tail = m[1].cpu().numpy()[w13.plane_bytes(N, K):].view(np.uint32)
        assert tail[N // 16:2 * (N // 16) + 1].tolist() == [1] * (N // 16 + 1)
    y0 = _launch(eng, form, N, K, gate, up, twins=False)
    y1 = _launch(eng, form, N, K, gate, up, twins=True)
    assert bool(torch.isfinite(y0).all()) and float(y0.abs().max()) > 0 and not bool((y0 == 7.0).any())
    assert torch.equal(_bits(y0), _bits(y1))


# ---------------------------------------------------------------- the fall-back
FB_N, FB_K = 64, 384          # 4 tile rows; 3 groups: over 4 waves ranges start inside a group, over 8 waves some waves have no K


def _plant(b, tile_row, value):
    """one element of the tile row replaced by a pattern the format refuses ("under31": 31 binades under the row's largest)"""
    if value == "under31":
        row = b[16 * tile_row:16 * tile_row + 16].reshape(-1)
        value = WC.under(row[np.argmax((row >> 7) & 0xFF)], 31)
    b[16 * tile_row + 4, 70] = value


def _ok_words(twin, N, K):
    return twin.cpu().numpy()[w13.plane_bytes(N, K):].view(np.uint32)[N // 16:2 * (N // 16)].tolist()


def _planted(eng, seed, rows, value):
    """(packed, twin) of a normal matrix with `value` planted in the tile rows `rows`, and the matrix's bits"""
    b = WC.bits(WC.weights(FB_N, FB_K, seed))
    for r in rows:
        _plant(b, r, value)
    m = _pack(eng, WC.from_bits(b))
    assert _ok_words(m[1], FB_N, FB_K) == [0 if r in rows else 1 for r in range(FB_N // 16)]
    return m


def _ff_planes(m, rows):
    """the twin with the planes of the tile rows `rows` overwritten with 0xFF (scale and ok words stay)"""
    twin = m[1].clone()
    per_row = (FB_K // 128) * 3328
    for r in rows:
        twin[r * per_row:(r + 1) * per_row] = 0xFF
    return m[0], twin


def _other_fragments(eng, m, rows, seed):
    """the bf16 fragments of every tile row NOT in `rows` replaced by those of another finite matrix"""
    other = eng.pack_matrix(WC.weights(FB_N, FB_K, seed).float())
    per_row = (FB_K // 32) * 1024
    for r in rows:
        other[r * per_row:(r + 1) * per_row] = m[0][r * per_row:(r + 1) * per_row]
    return other, m[1]


ALL_ROWS = tuple(range(FB_N // 16))
# (case, tile rows planted in the matrix / in gate, tile rows planted in up): one matrix has the first and the last case
PLANTS = [("one row", (1,), ()), ("up", (), (2,)), ("both", (1,), (2,)), ("every row", ALL_ROWS, ALL_ROWS)]
FB_CASES = [(f, v, *p) for f, (_, epi, _) in FORMS.items() for v in (WC.DENORMAL, "under31", WC.INF) for p in PLANTS
            if epi == SWIGLU or p[0] in ("one row", "every row")]


@pytest.mark.parametrize("form,value,where,g_rows,u_rows", FB_CASES,
                         ids=[f"{c[0]}-{c[1] if isinstance(c[1], str) else hex(c[1])}-{c[2]}" for c in FB_CASES])
def test_a_tile_row_the_format_cannot_hold_streams_bf16(eng, form, value, where, g_rows, u_rows):
    if FORMS[form][1] != SWIGLU:
        u_rows = ()
    gate, up = _planted(eng, 900, g_rows, value), _planted(eng, 901, u_rows, value)
    want = _launch(eng, form, FB_N, FB_K, gate, up, twins=False)
    got = _launch(eng, form, FB_N, FB_K, gate, up, twins=True)
    assert float(torch.nan_to_num(want, 0.0, 0.0, 0.0).abs().max()) > 0
    assert torch.equal(_bits(got), _bits(want))
    # the rows that fall back read no planes (a SwiGLU workgroup falls back when either of its matrices asks for it) ...
    fb = tuple(sorted(set(g_rows) | set(u_rows)))
    got = _launch(eng, form, FB_N, FB_K, _ff_planes(gate, fb), _ff_planes(up, fb), twins=True)
    assert torch.equal(_bits(got), _bits(want))
    # ... and the others read no bf16 fragments
    got = _launch(eng, form, FB_N, FB_K, _other_fragments(eng, gate, fb, 910), _other_fragments(eng, up, fb, 911), twins=True)
    assert torch.equal(_bits(got), _bits(want))
    if len(fb) < FB_N // 16:          # the converse, so that the two checks above cannot pass on a kernel that reads one storage for every row
        ok_rows = tuple(r for r in range(FB_N // 16) if r not in fb)
        got = _launch(eng, form, FB_N, FB_K, _ff_planes(gate, ok_rows), _ff_planes(up, ok_rows), twins=True)
        assert not torch.equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- the engine
ARMS = ("1", "head", "0")
DOWN = "lm.layers.1.mlp.down_proj.weight"
QPROJ = "lm.layers.0.self_attn.q_proj.weight"


def _arm(arm, H, graph, heads=2, kv_heads=1, inter=1152):
    old = os.environ.get("VVHIP_W13")
    os.environ["VVHIP_W13"] = arm
    try:
        cfg = synth.LMCfg(hidden=H, heads=heads, kv_heads=kv_heads, inter=inter, head_dim_override=128)
        return build_small(cfg, xsplit=1, use_graph=graph, n_slots=1, max_ctx=512, head_layers=WC.HEAD_LAYERS)
    finally:
        if old is None:
            os.environ.pop("VVHIP_W13", None)
        else:
            os.environ["VVHIP_W13"] = old


def _decode(s, H, pos0):
    """three steps of 1 row and three of 2 rows from position pos0 (graphed: first sight, capture, replay of each key) -> hidden rows"""
    eng = s.eng
    if not hasattr(s, "io"):
        s.io = {n: (torch.zeros(n, H, device=eng.device), torch.zeros(n, H, device=eng.device)) for n in (1, 2)}
    outs = []
    for n in (1, 2):
        x, h = s.io[n]
        for step in range(3):
            x.copy_(_rows(eng, 50 + step + 10 * n, n, H))
            eng.lm_forward([(c, pos0 + 3 * (n - 1) + step) for c in range(n)], x, h)
            eng.sync()
            outs.append(h.clone())
    out = torch.cat(outs)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    return out


def _agree(arms, H, pos0):
    outs = [_decode(s, H, pos0) for s in arms]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    return outs[0]


@pytest.mark.parametrize("H", [256, 384])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_lm_decode_arms_agree(H, graph, tmp_path):
    import test_gpu_adapters as ta
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    arms = [_arm(a, H, graph) for a in ARMS]
    try:
        on, head, off = (s.eng for s in arms)
        layers = arms[0].lmcfg.layers
        assert [e.stat(10) for e in (on, head, off)] == [5 * layers, 0, 0]
        assert [e.stat(9) for e in (on, head, off)] == [12, 12, 0]
        assert [e.stat(11) for e in (on, head, off)] == [0, 0, 0]
        a = _agree(arms, H, 0)
        # one down matrix uploaded again with new values: its twin follows
        new = WC.weights(H, 1152, 8800 + H)
        for s in arms:
            s.eng.upload(DOWN, new)
        b = _agree(arms, H, 8)
        assert not torch.equal(a, b)
        base = _agree(arms, H, 0)          # positions 0.. again: what the adapter runs below are compared with
        assert not torch.equal(base, a)
        # one denormal: one tile row of that matrix streams bf16, inside the same launch
        bad = WC.bits(new)
        bad[5, 77] = WC.DENORMAL
        for s in arms:
            s.eng.upload(DOWN, WC.from_bits(bad))
        assert [e.stat(11) for e in (on, head, off)] == [1, 0, 0] and on.stat(10) == 5 * layers and on.stat(9) == 12
        _agree(arms, H, 16)
        for s in arms:
            s.eng.upload(DOWN, new)
        assert on.stat(11) == 0
        # a LoRA merge and its reset through the model: a q_proj (one part of the layer's QKV twin) and a down_proj target
        targets = {QPROJ: arms[0].lm_w["layers.0.self_attn.q_proj.weight"], DOWN: new.float()}
        ad = ta._small_factors(targets, 3, 4)
        path = ta._write_adapter(tmp_path / "x", ad, 4, 2)
        cfgd = {"decoder_config": {"max_position_embeddings": arms[0].lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
        models = [VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.float32) for s in arms]
        for m in models:
            assert m.load_adapter("x", path) == sorted(ad)
            m.set_adapter("x")
        merged = _agree(arms, H, 0)
        assert not torch.equal(merged, base)
        for m in models:
            m.set_adapter(None)
        assert torch.equal(_agree(arms, H, 0), base)
        assert on.stat(11) == 0 and on.stat(10) == 5 * layers
        if graph:
            for e in (on, head, off):
                assert e.stat(5) == 0 and e.stat(4) == 0 and e.stat(1) > 0
    finally:
        for s in arms:
            s.eng.close()


WIDE = dict(heads=32, kv_heads=4, inter=4224)          # QKV (32 + 2 x 4) x 128 = 5120 features, 320 tiles; gate/up 264 tiles: the 2 x 4 forms
GATE = "lm.layers.1.mlp.gate_proj.weight"


def _window_bytes(s, H):
    """bytes of the profile window of one 2-row LM pass (the launches run eagerly inside a window)"""
    eng = s.eng
    x, h = _rows(eng, 3, 2, H), torch.zeros(2, H, device=eng.device)
    eng.profile_begin()
    eng.lm_forward([(0, 30), (1, 30)], x, h)
    (_, _, total), _ = eng.profile_end()
    eng.sync()
    return total


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_wide_lm_streams_qkv_and_gate_up_twins(graph, tmp_path):
    import test_gpu_adapters as ta
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    H, I, QKV = 256, WIDE["inter"], (WIDE["heads"] + 2 * WIDE["kv_heads"]) * 128
    arms = [_arm(a, H, graph, **WIDE) for a in ARMS]
    try:
        on, head, off = (s.eng for s in arms)
        layers = arms[0].lmcfg.layers
        assert [e.stat(10) for e in (on, head, off)] == [5 * layers, 0, 0] and on.stat(11) == 0
        # what the launches stream: QKV, gate and up as planes (13/16 of 2 bytes per element), everything else as in the other arms
        # (gate and up of every layer; QKV of the first layer alone: a down projection of 16 tiles x 132 k-tiles splits K over three
        # workgroup columns, so the next layer's QKV consumes part tensors and has no W13 form, tests/test_w13_plan_cpu.py)
        saved = (QKV + layers * 2 * I) * H * 3 // 8
        by = [_window_bytes(s, H) for s in arms]
        assert by[1] == by[2] and by[2] - by[0] == saved
        base = _agree(arms, H, 0)
        # q_proj (one part of the layer's QKV twin) and gate_proj uploaded again with new values: their twins follow
        new_q, new_g = WC.weights(WIDE["heads"] * 128, H, 9100), WC.weights(I, H, 9101)
        for s in arms:
            s.eng.upload(QPROJ, new_q)
            s.eng.upload(GATE, new_g)
        base2 = _agree(arms, H, 0)
        assert not torch.equal(base2, base) and on.stat(11) == 0
        # a denormal in each: one tile row of the QKV twin and one of the gate twin stream bf16
        bad_q, bad_g = WC.bits(new_q), WC.bits(new_g)
        bad_q[37, 70] = WC.DENORMAL
        bad_g[5, 77] = WC.DENORMAL
        for s in arms:
            s.eng.upload(QPROJ, WC.from_bits(bad_q))
            s.eng.upload(GATE, WC.from_bits(bad_g))
        assert [e.stat(11) for e in (on, head, off)] == [2, 0, 0]
        _agree(arms, H, 0)
        for s in arms:
            s.eng.upload(QPROJ, new_q)
            s.eng.upload(GATE, new_g)
        assert on.stat(11) == 0 and torch.equal(_agree(arms, H, 0), base2)
        # set_adapter() and its reset on the same two targets
        targets = {QPROJ: new_q.float(), GATE: new_g.float()}
        ad = ta._small_factors(targets, 5, 4)
        path = ta._write_adapter(tmp_path / "x", ad, 4, 2)
        cfgd = {"decoder_config": {"max_position_embeddings": arms[0].lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
        models = [VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.float32) for s in arms]
        for m in models:
            assert m.load_adapter("x", path) == sorted(ad)
            m.set_adapter("x")
        assert not torch.equal(_agree(arms, H, 0), base2)
        for m in models:
            m.set_adapter(None)
        assert torch.equal(_agree(arms, H, 0), base2)
        by = [_window_bytes(s, H) for s in arms]
        assert by[2] - by[0] == saved
        if graph:
            for e in (on, head, off):
                assert e.stat(5) == 0 and e.stat(4) == 0 and e.stat(1) > 0
    finally:
        for s in arms:
            s.eng.close()
