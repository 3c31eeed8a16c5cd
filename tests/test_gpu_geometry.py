"""GPU parity at the REAL attention geometries and context lengths of the shipped models:

  * VibeVoice-7B widths, one layer: hidden 3584, 28 q / 4 kv heads x 128 (GQA group 7), MLP 18944, diffusion-head
    FFN 10752 (vibevoice/configs/qwen2.5_7b_32k.json) -- prefill (MFMA tile GEMM + prefill attention), decode steps,
    restricted logits, CFG sampler;
  * Streaming-0.5B widths, one layer: hidden 896, 14 / 2 heads x 64 (group 7), MLP 4864;
  * decode attention over a LONG cache: 32,768 positions at the 7B geometry, 65,536 at the 1.5B geometry (12 / 2 x 128),
    8,192 at the 0.5B geometry -- random bf16 K/V placed with vv_kv_import(_at), every flash-decoding split and the
    last-arriver ticket merge of vv_attn_fused_kernel, against the oracle's eager attention (oracle/lm.py);
  * prefill attention over >= 4K positions against the oracle in 512-row chunks: vv_attn_prefill4_kernel in the bf16 mode; in the
    exact modes the chunk's rows go through the split + merge attention pair, 64 rows per launch.

One layer keeps the CPU oracle to seconds; every kernel runs at its real per-layer shape.  Weights are bf16-representable
and the engine runs xsplit=3 unless stated, so bounds are fp32-class (bf16 KV cache mirrored by the oracle)."""
import numpy as np
import pytest
import torch

import lm_shapes as ls
import synth
from gpu_util import build_small, rel_err
from oracle import dpm, head
from oracle import lm as olm

pytestmark = pytest.mark.gpu

GEOM = {
    "7b": synth.LMCfg(hidden=3584, layers=1, heads=28, kv_heads=4, inter=18944, vocab=64, max_pos=32768),
    "1.5b": synth.LMCfg(hidden=1536, layers=1, heads=12, kv_heads=2, inter=8960, vocab=64, max_pos=65536),
    "0.5b": synth.LMCfg(hidden=896, layers=1, heads=14, kv_heads=2, inter=4864, vocab=64, max_pos=8192),
}


class _FastGen(synth.Gen):
    """synth.Gen with the big normal draws made on the GPU (numpy's PCG64 needs ~80 s for a 7B-width layer on the build box;
    these tests pin no golden file, any deterministic bf16-representable weights do)."""

    def __init__(self, seed):
        super().__init__(seed)
        self._dev = "cuda" if torch.cuda.is_available() else "cpu"
        self._tg = torch.Generator(device=self._dev).manual_seed(seed)

    def normal(self, shape, std=1.0, mat=True):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        a = torch.randn(shape, generator=self._tg, device=self._dev) * float(std)
        if mat:
            a = a.to(torch.bfloat16).to(torch.float32)
        return a.cpu()


def build_fast(*a, **k):
    old = synth.Gen
    synth.Gen = _FastGen
    try:
        return build_small(*a, **k)
    finally:
        synth.Gen = old


def dev(t, eng):
    out = t.to(eng.device, torch.float32).contiguous()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("xs,tol", [(3, 5e-4), (1, 3e-2)])
@pytest.mark.parametrize("tag", ["7b", "0.5b"])
def test_one_layer_at_real_widths(tag, xs, tol):
    """prefill 70 tokens (one 64-row pass + a 6-row remainder), 4 decode steps with a second cache in the same launch,
    restricted logits, and the CFG sampler at the model's diffusion-head width.  xs = 3: fp32-exact activations (general /
    tile kernels, 16-row prefill attention); xs = 1: the bf16 mode bench.py times -- packed activations, the LDS-staged
    128 x 128 GEMM and the 64-row prefill attention of prefill.hip at GQA group 7."""
    c = GEOM[tag]
    s = build_fast(c, xsplit=xs, max_ctx=256, max_rows=64, head_layers=1)
    eng = s.eng
    try:
        H = c.hidden
        m = s.oracle_lm(kv_round_bf16=True)
        g = synth.Gen(700)
        L0 = 70
        x = g.normal((L0, H), 1.0, mat=False)
        oc = m.new_cache()
        ref = m.forward(x, oc)
        hid = eng.new(L0, H)
        xd = dev(x, eng)
        with torch.cuda.stream(eng.stream):
            eng.lm_forward([(0, j) for j in range(64)], xd[:64], hid[:64])
            eng.lm_forward([(0, 64 + j) for j in range(L0 - 64)], xd[64:], hid[64:])
        eng.sync()
        assert rel_err(hid, ref) <= tol, rel_err(hid, ref)
        oc2 = m.new_cache()
        xdec = g.normal((4, 2, H), 1.0, mat=False)
        for i in range(4):
            r1 = m.forward(xdec[i, 0:1], oc)
            r2 = m.forward(xdec[i, 1:2], oc2)
            out = eng.new(2, H)
            with torch.cuda.stream(eng.stream):
                eng.lm_forward([(0, L0 + i), (1, i)], dev(xdec[i], eng), out)
            eng.sync()
            assert rel_err(out[0], r1[0]) <= tol, (i, rel_err(out[0], r1[0]))
            assert rel_err(out[1], r2[0]) <= tol, (i, rel_err(out[1], r2[0]))
        valid = [5, 17, 44, 2]
        eng.set_valid_tokens(valid)
        lg = eng.new(2 * len(valid))
        with torch.cuda.stream(eng.stream):
            eng.lm_logits(2, out, lg)
        eng.sync()
        ref_lg = torch.nn.functional.linear(torch.stack([r1[0], r2[0]]), s.lm_head)[:, valid]
        assert rel_err(lg.view(2, len(valid)), ref_lg) <= max(tol, 5e-4)
        # diffusion head at this width: 2 utterances -> 4 head rows
        pos = g.normal((2, H), 1.0, mat=False)
        neg = g.normal((2, H), 1.0, mat=False)
        noise = g.normal((4, 64), 1.0, mat=False)
        refl = dpm.sample_speech_tokens(lambda a, t, cnd: head.head_forward(s.head_w, a, t, cnd, s.hc.layers, s.hc.eps),
                                        pos, neg, 1.3, 5, noise)
        eng.set_num_steps(5)
        lat = eng.new(2, 64)
        with torch.cuda.stream(eng.stream):
            eng.diffusion_sample(2, dev(torch.cat([pos, neg]), eng), dev(noise[:2], eng), 1.3, lat)
        eng.sync()
        assert rel_err(lat, refl) <= (2e-3 if xs == 3 else 5e-2), rel_err(lat, refl)
    finally:
        eng.close()


@pytest.mark.parametrize("tag,L", [("7b", 32768 - 2), ("1.5b", 65536 - 2), ("0.5b", 8192 - 2)])
@pytest.mark.parametrize("xs,tol", [(3, 5e-4), (1, 3e-2)])
def test_decode_attention_over_the_full_context(tag, L, xs, tol):
    """One decode step whose query attends L cached positions (all 32 flash-decoding splits + the ticket merge), the new
    token's own K/V appended by the owner workgroup; a second, short cache rides in the same launch (its single-split
    path).  K/V: random bf16 values imported in two pieces (vv_kv_import for [0, L/3), vv_kv_import_at for the rest)."""
    import dataclasses
    c = dataclasses.replace(GEOM[tag], inter=256)          # the attention geometry is what matters here: a thin MLP and head
    s = build_fast(c, xsplit=xs, max_ctx=L + 2, max_rows=16, head_layers=1, head_ffn_ratio=0.25)
    eng = s.eng
    try:
        H, kvh, d = c.hidden, c.kv_heads, c.head_dim
        m = s.oracle_lm(kv_round_bf16=True)
        gk = torch.Generator().manual_seed(L)
        # keys with std 3: the scores have std ~3, so the softmax over tens of thousands of positions is peaked on a few dozen
        # of them and the attention output is O(0.2) instead of the O(0.005) mean of random values
        k = (torch.randn(kvh, L, d, generator=gk) * 3.0).to(torch.bfloat16)
        v = torch.randn(kvh, L, d, generator=gk).to(torch.bfloat16)
        cut = L // 3
        with torch.cuda.stream(eng.stream):
            eng.kv_import(0, 0, k[:, :cut].to(eng.device), v[:, :cut].to(eng.device))
            eng.kv_import_at(0, 0, cut, k[:, cut:].to(eng.device), v[:, cut:].to(eng.device))
        eng.sync()
        oc = m.new_cache()
        oc.k[0], oc.v[0], oc.length = k.float(), v.float(), L
        oc2 = m.new_cache()
        g = synth.Gen(900 + L)
        # a small input embedding: the residual stream after the layer is then dominated by o_proj(attention), so the compared
        # hidden state is essentially a function of the attention output (RMSNorm removes the scale on the way in)
        x = g.normal((2, 2, H), 0.02, mat=False)
        for i in range(2):                                   # two steps: the second one also reads the first one's append
            r1 = m.forward(x[i, 0:1], oc)
            r2 = m.forward(x[i, 1:2], oc2)
            out = eng.new(2, H)
            with torch.cuda.stream(eng.stream):
                eng.lm_forward([(0, L + i), (1, i)], dev(x[i], eng), out)
            eng.sync()
            assert rel_err(out[0], r1[0]) <= tol, (i, rel_err(out[0], r1[0]))
            assert rel_err(out[1], r2[0]) <= tol, (i, rel_err(out[1], r2[0]))
    finally:
        eng.close()


@pytest.mark.parametrize("xs,tol", [(3, 5e-4), (2, 1e-3), (1, 4e-2)])
def test_prefill_attention_over_4k_positions(xs, tol):
    """A 4,200-token prompt through one layer in 512-row chunks against the oracle's full causal attention: xs = 1 runs the
    packed-activation GEMMs + vv_attn_prefill4_kernel; xs = 2, 3 the tile / general GEMMs and, per chunk, eight 64-row launches of
    the split + merge attention pair (every row attends its own causal prefix).  Shapes: tests/lm_shapes.py; test_pass_plan_cpu.py
    asserts the routes."""
    c, chunk = ls.PREFILL_4K_ENGINE
    s = build_fast(c, xsplit=xs, max_ctx=4352, max_rows=chunk, head_layers=1)
    eng = s.eng
    try:
        H = c.hidden
        m = s.oracle_lm(kv_round_bf16=True)
        g = synth.Gen(4200)
        L0 = ls.PREFILL_4K_PROMPT
        x = g.normal((L0, H), 1.0, mat=False)
        ref = m.forward(x, m.new_cache())
        hid = eng.new(L0, H)
        xd = dev(x, eng)
        with torch.cuda.stream(eng.stream):
            for i0 in range(0, L0, chunk):
                n = min(chunk, L0 - i0)
                eng.lm_forward([(0, i0 + j) for j in range(n)], xd[i0:i0 + n], hid[i0:i0 + n])
        eng.sync()
        assert rel_err(hid[-64:], ref[-64:]) <= tol, rel_err(hid[-64:], ref[-64:])
        assert rel_err(hid, ref) <= tol, rel_err(hid, ref)
    finally:
        eng.close()


def _prefill_probe(L0, chunk, heads, kv_heads, hd):
    """One bf16-mode layer over an L0-token prompt in `chunk`-row passes; returns the hidden states [L0, H] (CPU)."""
    c = synth.LMCfg(hidden=heads * hd, layers=1, heads=heads, kv_heads=kv_heads, inter=512, vocab=64, max_pos=8192)
    s = build_fast(c, xsplit=1, max_ctx=(L0 + 255) // 128 * 128, max_rows=chunk, head_layers=1)
    eng = s.eng
    try:
        g = synth.Gen(L0 + chunk)
        x = g.normal((L0, c.hidden), 1.0, mat=False)
        hid = eng.new(L0, c.hidden)
        xd = dev(x, eng)
        with torch.cuda.stream(eng.stream):
            for i0 in range(0, L0, chunk):
                n = min(chunk, L0 - i0)
                eng.lm_forward([(0, i0 + j) for j in range(n)], xd[i0:i0 + n], hid[i0:i0 + n])
        eng.sync()
        return hid.float().cpu(), s, x
    finally:
        eng.close()
