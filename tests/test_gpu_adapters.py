"""Device-resident LoRA adapters on the GPU: the merge kernel (lora.hip) against lora.merge_lora bit for bit on exactly
representable inputs and against fp64 on Gaussian ones, the unpack kernel, the engine entries (base snapshots, reset, upload as
the new base, refusals) and model.set_adapter() through generate() with captured graphs.

Exact inputs (lora_ref.exact_case): a, b integers in [-16, 16] / 8, scale in {0.5, 2, 4}: every product and partial sum is
exact in fp32 in any order, so the kernel must equal merge_lora on the CPU in both merge modes -- compared as the BYTES of the
packed matrix, padding included."""
import json
import types

import pytest
import torch

import lora_ref
import synth
from gpu_util import build_small
from vibevoice_amd import lora
from vibevoice_amd.engine import EngineError

pytestmark = pytest.mark.gpu

MODES = ("float32", "bfloat16")
EXACT_CASES = [(16, 32, 1), (20, 40, 3), (48, 96, 8), (80, 160, 64), (16, 4096, 16), (1040, 32, 65), (32, 64, 256), (64, 18944, 8),
               (18944, 3584, 8)]
LM_TARGETS = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
HEAD_TARGETS = ["noisy_images_proj", "cond_proj", "layers.0.ffn.gate_proj", "layers.0.ffn.up_proj", "layers.0.ffn.down_proj",
                "layers.1.ffn.gate_proj", "layers.1.ffn.up_proj", "layers.1.ffn.down_proj", "final_layer.linear"]


@pytest.fixture(scope="module")
def sm():
    s = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=256)
    yield s
    s.eng.close()


def _dev(eng, t):
    return t.to(eng.device).contiguous()


# ---------------------------------------------------------------- raw kernel
@pytest.mark.parametrize("N,K,r", EXACT_CASES)
def test_merge_kernel_equals_merge_lora_bit_for_bit(sm, N, K, r):
    eng = sm.eng
    w, a, b, scale = lora_ref.exact_case(N, K, r, seed=N + K + r, scale_i=N + r)
    base = eng.pack_matrix(w.float())
    ad, bd = _dev(eng, a), _dev(eng, b)
    for mode in MODES:
        want = eng.pack_matrix(lora.merge_lora(w, a, b, scale, merge_dtype=mode).float())
        dst = torch.full_like(base, 0xFF)                              # NaN words: every byte of dst must be written
        eng.lora_merge_raw(base, dst, N, K, ad, bd, scale, mode)
        eng.sync()
        assert torch.equal(dst, want), (mode, int((dst != want).sum()))
        buf = base.clone()                                             # in place: dst == base
        eng.lora_merge_raw(buf, buf, N, K, ad, bd, scale, mode)
        eng.sync()
        assert torch.equal(buf, want), (mode, "in place", int((buf != want).sum()))
    assert torch.equal(base, eng.pack_matrix(w.float()))               # the out-of-place form left its base alone


@pytest.mark.parametrize("N,K,r", [(512, 512, 16), (512, 512, 64), (256, 1024, 8)])
def test_merge_kernel_gaussian_inputs_against_fp64(sm, N, K, r):
    """fp32-delta mode on Gaussian factors (lora_ref.gaussian_case: no deep cancellations, a property of the inputs): every element
    is the correctly rounded bf16 of the fp64 merge or its neighbour, and at most 1e-3 of them are not the correctly rounded one.
    merge_lora itself is held to the same two conditions on the same inputs, so the inputs are inside the cap on their own."""
    eng = sm.eng
    w, a, b, scale, _ = lora_ref.gaussian_case(N, K, r, seed=1000 + r)
    ref = lora_ref.rne_bf16(lora_ref.merge_fp64(w, a, b, scale))
    ok, share = lora_ref.equal_or_adjacent(lora.merge_lora(w, a, b, scale), ref)
    print(f"merge_lora (CPU) vs fp64: adjacent {ok}, not correctly rounded {share:.3e}")
    assert ok and share <= 1e-3
    base = eng.pack_matrix(w.float())
    dst = torch.full_like(base, 0xFF)
    eng.lora_merge_raw(base, dst, N, K, _dev(eng, a), _dev(eng, b), scale, "float32")
    got = eng.unpack_matrix(dst, N, K)
    eng.sync()
    ok, share = lora_ref.equal_or_adjacent(got.cpu().to(torch.bfloat16), ref)
    print(f"kernel vs fp64: adjacent {ok}, not correctly rounded {share:.3e}")
    assert torch.equal(got.cpu().to(torch.bfloat16).float(), got.cpu())      # the unpacked values are bf16 numbers
    assert ok and share <= 1e-3


@pytest.mark.parametrize("N,K", [(16, 32), (20, 40), (48, 96), (80, 160), (16, 4096), (1040, 32), (32, 64), (64, 18944)])
def test_unpack_is_the_inverse_of_pack(sm, N, K):
    eng = sm.eng
    w = lora_ref.exact_case(N, K, 1, seed=N * 3 + K)[0].float()
    packed = eng.pack_matrix(w)
    out = torch.full((N, K), float("nan"), device=eng.device)           # poisoned: every element must be written
    eng.unpack_matrix(packed, N, K, out=out)
    eng.sync()
    assert torch.equal(out.cpu(), w)


# ---------------------------------------------------------------- engine level
def _targets(s):
    """{engine parameter name: its synthetic base (bf16-representable fp32)} of every LoRA target of the small model"""
    t = {}
    for l in range(s.lmcfg.layers):
        for m in LM_TARGETS:
            t[f"lm.layers.{l}.{m}.weight"] = s.lm_w[f"layers.{l}.{m}.weight"]
    for m in HEAD_TARGETS:
        t[f"head.{m}.weight"] = s.head_w[m + ".weight"]
    return t


def _adapter(targets, seed, r=4, names=None):
    """{name: (a, b, scale)} of exact factors"""
    out = {}
    for i, (name, w) in enumerate(sorted(targets.items())):
        if names is not None and name not in names:
            continue
        _, a, b, scale = lora_ref.exact_case(w.shape[0], w.shape[1], r, seed=seed * 1000 + i, scale_i=seed + i)
        out[name] = (a, b, scale)
    return out


def _merge_all(eng, ad, mode="float32"):
    keep = []
    for name, (a, b, scale) in ad.items():
        a, b = _dev(eng, a), _dev(eng, b)
        keep.append((a, b))
        eng.lora_merge(name, a, b, scale, mode)
    eng.sync()


def _read_all(eng, targets):
    out = {k: eng.weight_read(k, w.shape) for k, w in targets.items()}
    eng.sync()
    return {k: v.cpu() for k, v in out.items()}


def _merged(w, abs_, mode="float32"):
    a, b, scale = abs_
    return lora.merge_lora(w.to(torch.bfloat16), a, b, scale, merge_dtype=mode).float()


@pytest.mark.parametrize("mode", MODES)
def test_engine_merge_reset_and_rebase(sm, mode):
    eng = sm.eng
    targets = _targets(sm)
    got = _read_all(eng, targets)
    for k, w in targets.items():
        assert torch.equal(got[k], w), k                                 # weight_read of the base: the synthetic tensor
    # k_proj alone: its neighbours in the shared q / k / v region keep their bits
    kname = "lm.layers.0.self_attn.k_proj.weight"
    x = _adapter(targets, seed=1)
    _merge_all(eng, {kname: x[kname]}, mode)
    got = _read_all(eng, targets)
    for k, w in targets.items():
        assert torch.equal(got[k], _merged(w, x[k], mode) if k == kname else w), k
    # every target
    _merge_all(eng, x, mode)
    got = _read_all(eng, targets)
    for k, w in targets.items():
        assert torch.equal(got[k], _merged(w, x[k], mode)), k
    assert eng.stat(7) == sum(int(eng.lib.vv_packed_bytes(*w.shape)) for w in targets.values())
    # X then Y: no trace of X (a fresh engine merged with Y alone holds the same bits)
    y = _adapter(targets, seed=2, r=7)
    _merge_all(eng, y, mode)
    got = _read_all(eng, targets)
    fresh = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=256)
    try:
        _merge_all(fresh.eng, y, mode)
        want = _read_all(fresh.eng, targets)
    finally:
        fresh.eng.close()
    for k, w in targets.items():
        assert torch.equal(got[k], want[k]) and torch.equal(got[k], _merged(w, y[k], mode)), k
    # upload onto a merged parameter: the upload is the new base
    up = "lm.layers.1.mlp.down_proj.weight"
    new_base = synth.Gen(77).linear(*targets[up].shape)
    eng.upload(up, new_base)
    assert torch.equal(_read_all(eng, {up: new_base})[up], new_base)
    eng.lora_reset(up)                                                   # no adapter is recorded for it: nothing to undo
    assert torch.equal(_read_all(eng, {up: new_base})[up], new_base)
    _merge_all(eng, {up: x[up]}, mode)
    assert torch.equal(_read_all(eng, {up: new_base})[up], _merged(new_base, x[up], mode))
    # reset: every parameter back to its base bits
    eng.lora_reset()
    got = _read_all(eng, targets)
    for k, w in targets.items():
        assert torch.equal(got[k], new_base if k == up else w), k
    eng.upload(up, targets[up])                                          # the module fixture goes back to its synthetic weights
    assert torch.equal(_read_all(eng, {up: targets[up]})[up], targets[up])


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(sm):
    eng = sm.eng
    H = sm.lmcfg.hidden
    name = "lm.layers.0.self_attn.q_proj.weight"
    N, K = sm.lm_w["layers.0.self_attn.q_proj.weight"].shape
    exp = eng.expected_weights()
    conv = next(k for k in exp if k.startswith("dec.upsample_layers.1.") and k.endswith("convtr.convtr.weight"))
    a = torch.zeros(4, K, device=eng.device)
    b = torch.zeros(N, 4, device=eng.device)
    out = torch.zeros(N, K, device=eng.device)
    eng.sync()
    n0 = eng.stat(0)

    def refused(text, fn, *args, **kw):
        with pytest.raises(EngineError, match=text):
            fn(*args, **kw)
        assert eng.stat(0) == n0, text

    # factors that hold the parameter's element count in another shape never reach the library
    dn = "lm.layers.0.mlp.down_proj.weight"
    dN, dK = sm.lm_w["layers.0.mlp.down_proj.weight"].shape
    with pytest.raises(ValueError, match="the parameter is"):
        eng.lora_merge(dn, torch.zeros(4, dN, device=eng.device), torch.zeros(dK, 4, device=eng.device), 1.0)
    with pytest.raises(ValueError, match="the parameter is"):
        eng.weight_read(dn, (dK, dN))
    assert eng.stat(0) == n0
    refused("unknown parameter", eng.lora_merge, "lm.layers.9.nope.weight", a, b, 1.0)
    refused("unknown parameter", eng.lora_reset, "lm.layers.9.nope.weight")
    refused("unknown parameter", eng.weight_read, "lm.layers.9.nope.weight", (N, K))
    # not a plain linear matrix: a table, a vector, a transposed-convolution weight
    V = sm.lmcfg.vocab
    for nm, (n_, k_) in (("lm.embed_tokens.weight", (V, H)), ("lm.norm.weight", (1, H)), (conv, (exp[conv] // 16, 16))):
        refused("not a plain linear matrix", eng.lora_merge, nm, torch.zeros(2, k_, device=eng.device), torch.zeros(n_, 2, device=eng.device), 1.0)
        refused("not a plain linear matrix", eng.weight_read, nm, (n_, k_))
        refused("not a plain linear matrix", eng.lora_reset, nm)
    refused("outside \\[1, 256\\]", eng.lora_merge, name, torch.zeros(257, K, device=eng.device), torch.zeros(N, 257, device=eng.device), 1.0)
    refused("outside \\[1, 256\\]", eng.lora_merge, name, torch.zeros(0, K, device=eng.device), torch.zeros(N, 0, device=eng.device), 1.0)
    for bad in (float("inf"), float("nan")):
        refused("scale is not finite", eng.lora_merge, name, a, b, bad)
    big = torch.zeros(4 * K + 8, device=eng.device)
    refused("16-byte aligned", eng.lora_merge, name, big[1:1 + 4 * K].view(4, K), b, 1.0, unaligned_ok=("a",))
    big = torch.zeros(4 * N + 8, device=eng.device)
    refused("16-byte aligned", eng.lora_merge, name, a, big[1:1 + 4 * N].view(N, 4), 1.0, unaligned_ok=("b",))
    assert eng.lib.vv_lora_merge(eng._ctx, eng._s, name.encode(), None, None, 4, 1.0, 0) < 0 and "null factor" in eng._err()
    assert eng.lib.vv_weight_read(eng._ctx, eng._s, name.encode(), None) < 0 and "out_dev is null" in eng._err()
    assert eng.stat(0) == n0
    # the raw entry refuses the same operands (no context: the text comes from the thread's last error)
    packed = eng.pack_matrix(torch.zeros(N, K))
    n0 = eng.stat(0)
    refused("scale is not finite", eng.lora_merge_raw, packed, packed, N, K, a, b, float("nan"))
    # a shared child, and a parent with a live child
    child = eng.fork()
    try:
        with pytest.raises(EngineError, match="shares its parent's weights"):
            child.lora_merge(name, a, b, 1.0)
        with pytest.raises(EngineError, match="shares its parent's weights"):
            child.lora_reset()
        with pytest.raises(EngineError, match="shares its parent's weights"):
            child.weight_read(name, (N, K))
        refused("shared context", eng.lora_merge, name, a, b, 1.0)
        refused("shared context", eng.lora_reset)
        refused("shared context", eng.weight_read, name, (N, K))
    finally:
        child.close()
    # the engine still works
    _, a2, b2, scale = lora_ref.exact_case(N, K, 4, seed=5)
    w = sm.lm_w["layers.0.self_attn.q_proj.weight"]
    _merge_all(eng, {name: (a2, b2, scale)})
    assert eng.stat(0) > n0
    assert torch.equal(_read_all(eng, {name: w})[name], _merged(w, (a2, b2, scale)))
    eng.lora_reset()
    assert torch.equal(_read_all(eng, {name: w})[name], w)


# ---------------------------------------------------------------- the whole path
def _write_adapter(root, ad, r, alpha):
    """the layout the reference's trainer writes: <root>/lora/adapter_* (language model) and <root>/lora/diffusion_head/adapter_*"""
    lm_sd, hd_sd = {}, {}
    for name, (a, b, _) in ad.items():
        mod = name[:-len(".weight")]
        if mod.startswith("lm."):
            lm_sd[f"base_model.model.{mod[3:]}.lora_A.weight"] = a
            lm_sd[f"base_model.model.{mod[3:]}.lora_B.weight"] = b
        else:
            hd_sd[f"base_model.model.base.{mod[5:]}.lora_A.default.weight"] = a
            hd_sd[f"base_model.model.base.{mod[5:]}.lora_B.default.weight"] = b
    (root / "lora" / "diffusion_head").mkdir(parents=True)
    for d, sd in ((root / "lora", lm_sd), (root / "lora" / "diffusion_head", hd_sd)):
        if sd:
            torch.save(sd, str(d / "adapter_model.bin"))
            (d / "adapter_config.json").write_text(json.dumps({"r": r, "lora_alpha": alpha}))
    return str(root)


def _small_factors(targets, seed, r, names=None):
    """exact factors small enough to leave a working model: integers in [-2, 2] / 8"""
    import numpy as np
    out = {}
    for i, (name, w) in enumerate(sorted(targets.items())):
        if names is not None and name not in names:
            continue
        g = np.random.default_rng(seed * 1000 + i)
        out[name] = (torch.from_numpy(g.integers(-2, 3, (r, w.shape[1])).astype(np.float32) / 8.0),
                     torch.from_numpy(g.integers(-2, 3, (w.shape[0], r)).astype(np.float32) / 8.0), None)
    return out


def test_set_adapter_through_generate_with_graphs(tmp_path):
    """model M switches base -> x -> y -> base on the device; model R receives the host-merged tensors of the same adapter through
    upload().  Every run: equal sequences, bit-equal audio, no foreign graph nodes -- with the graphs M captured before the first
    switch replayed after it, and the head's step table following the switch."""
    import test_gpu_generate as tg
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    sM = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=256, use_graph=True)
    sR = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=256, use_graph=True)
    try:
        targets = _targets(sM)
        r, alpha = 4, 2                                                    # scale = alpha / r = 0.5
        x = _small_factors(targets, 1, r)
        y = _small_factors(targets, 2, r, names=[k for k in targets if "q_proj" in k or "v_proj" in k or k.startswith("head.layers.1.") or "final" in k])
        cfgd = {"decoder_config": {"max_position_embeddings": sM.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
        tok = types.SimpleNamespace(speech_start_id=tg.TOK.speech_start_id, speech_end_id=tg.TOK.speech_end_id,
                                    speech_diffusion_id=tg.TOK.speech_diffusion_id, eos_token_id=tg.TOK.eos_token_id, bos_token_id=None,
                                    pad_token_id=tg.TOK.pad_token_id)
        models = []
        for s in (sM, sR):
            m = VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.float32)
            m.set_speech_factors(s.scaling, s.bias)
            m.set_ddpm_inference_steps(5)
            models.append(m)
        M, R = models
        assert M.load_adapter("x", _write_adapter(tmp_path / "x", x, r, alpha)) == sorted(x)
        M.load_adapter("y", _write_adapter(tmp_path / "y", y, r, alpha))
        ids, mask, sim, st, spm = tg.make_inputs(sM, 1, True, 11)
        g = synth.Gen(12)
        pre = (g.normal((1,), 1.0, mat=False), g.normal((1, 3, 64), 1.0, mat=False))
        bank = {}

        def noise_fn(step, n2):
            if (step, n2) not in bank:
                bank[(step, n2)] = synth.Gen(11000 + step).normal((n2, 64), 1.0, mat=False)
            return bank[(step, n2)]
        D, E, S, X = tg.D, tg.E, tg.S, tg.X
        forced = [[D, D, D, E, S, D, D, X]]

        def run(m):
            out = m.generate(input_ids=ids, attention_mask=mask, speech_tensors=st, speech_masks=spm, speech_input_mask=sim, cfg_scale=1.3,
                             tokenizer=tok, max_new_tokens=None, generation_config={"do_sample": False}, _forced_tokens=forced,
                             _noise_fn=noise_fn, _prefill_noise=pre, show_progress_bar=False)
            assert m.engine.stat(5) == 0
            return out

        def host(ad):
            for k, w in targets.items():                                    # R: the host path, every target re-uploaded
                R.upload(k, _merged(w, (ad[k][0], ad[k][1], alpha / r)) if k in ad else w)
        outs = {}
        for tag, ad in (("base", {}), ("x", x), ("y", y), ("none", {})):
            if tag != "base":
                M.set_adapter(None if tag == "none" else tag)
                host(ad)
            assert M.active_adapter == (tag if tag in ("x", "y") else None)
            oM, oR = run(M), run(R)
            assert torch.equal(oM.sequences.cpu(), oR.sequences.cpu()), tag
            assert len(oM.speech_outputs) == len(oR.speech_outputs) == 1
            assert torch.equal(oM.speech_outputs[0].cpu(), oR.speech_outputs[0].cpu()), tag
            outs[tag] = oM.speech_outputs[0].cpu()
        assert sM.eng.stat(1) > 0                                            # graphs were captured and kept across the switches
        assert not torch.equal(outs["x"], outs["base"]) and not torch.equal(outs["y"], outs["x"])      # the adapters change the output
        assert torch.equal(outs["none"], outs["base"])
    finally:
        sM.eng.close()
        sR.eng.close()
