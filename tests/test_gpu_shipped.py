"""GPU parity of the configurations that are SHIPPED and TIMED ("next round" item 1):

  (a) the voice-prompt encoder at the pass sizes the product uses (4, 5, 25, 75 frames per pass; the default is one
      75-frame pass per speaker) on a 75-frame prompt at the real tokenizer widths -- against the oracle's one-sequence
      encode (modular_vibevoice_tokenizer.py:384-418, 1081-1085) and against each other;
  (b) Streaming-0.5B generate() end to end in the timed mode (xsplit=1 + hipGraph) at the 0.5B attention geometry
      (hidden 896, 14 / 2 heads x 64 = GQA group 7, MLP 4864, 2 + 4 layers, head 4 layers): text windows of 5, speech windows
      of 6, EOS landing INSIDE a speech window (modeling_vibevoice_streaming_inference.py:568-694), teacher-forced per step and
      free-running;
  (c) one 7B-width layer prefilled in ONE pass of 10,922 rows (the pass bench.py times) against oracle/lm.py, row by row;
  (d) the bf16-mode-only kernels (vv_gemm3 / vv_gemm4, vv_attn_prefill4, vv_gemv16p, the 16-row sampler forms) against a
      reference whose matrix-unit INPUTS are rounded to bf16 (oracle mfma_in_bf16): what is left is summation order, so the
      bounds are ~1e-3, not the ~3e-2 the fp32 reference allows -- a wrong k-tile in a hundred fails;
  (e) SURVEY 8d's bf16-vs-bf16 tolerance: the HIP bf16 mode against the oracle loop run as PyTorch-ROCm eager ops in bf16 on
      the same GPU, teacher-forced per step: latent / hidden rel-L2 <= 2e-2, tokens identical.
"""
import copy
import dataclasses
import math
import types

import numpy as np
import pytest
import torch

import prefill_shapes
import synth
from gpu_util import build_small, rel_err
from oracle import codec, dpm, head
from oracle import generate as ogen
from oracle import generate_streaming as ogs
from test_gpu_geometry import GEOM, _FastGen, build_fast, dev

pytestmark = pytest.mark.gpu


def row_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float(((a - b).norm(dim=-1) / (b.norm(dim=-1) + 1e-30)).max())


class _Threads:
    """the GPU box advertises 256 logical CPUs; torch's default intra-op pool thrashes on it (bench.py caps it the same way)"""

    def __init__(self, n=32):
        self.n = n

    def __enter__(self):
        self.old = torch.get_num_threads()
        torch.set_num_threads(min(self.n, self.old))

    def __exit__(self, *a):
        torch.set_num_threads(self.old)


# ---------------------------------------------------------------------------------------------- (a) voice-prompt encoder
def _tokenizer_model(xsplit, enc_frames):
    from vibevoice_amd import synthetic
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg = copy.deepcopy(CONFIGS["1.5b"])
    cfg["decoder_config"]["num_hidden_layers"] = 1
    cfg["decoder_config"]["vocab_size"] = 2048
    cfg["decoder_config"]["max_position_embeddings"] = 64
    gen = torch.Generator().manual_seed(11)
    sd = {k: synthetic.random_tensor(k, shp, gen, "cpu", torch.bfloat16) for k, shp in synthetic.param_shapes(cfg).items()}
    model = VibeVoiceForConditionalGenerationInference.from_state_dict(cfg, sd, torch.float32, None, n_slots=1, max_ctx=64,
                                                                       xsplit=xsplit, use_graph=True, enc_frames=enc_frames)
    ac_w = {k[len("model.acoustic_tokenizer."):]: v.float() for k, v in sd.items() if k.startswith("model.acoustic_tokenizer.")}
    return model, ac_w


@pytest.mark.parametrize("xs,tol_ref,tol_pair", [(1, 1.5e-2, 1e-2), (3, 1e-5, 1e-5)])
def test_voice_prompt_encoder_at_the_shipped_pass_sizes(xs, tol_ref, tol_pair):
    """75-frame (10 s) voice prompt, real tokenizer widths (n_filters 32, depths 3-3-3-3-3-3-8, 3200x).  Pass sizes 2 (what
    rounds 1-2 tested), 4, 5, 25 and 75 frames per pass through vv_set_enc_pass_frames, in the bf16 mode bench.py times (xs = 1)
    and in the exact mode (xs = 3): each against the oracle's single non-streaming encode of the whole prompt, and all against
    pass size 2."""
    nfr = 75
    g = torch.Generator().manual_seed(75)
    wav = torch.rand(nfr * 3200, generator=g) * 0.2 - 0.1
    model, ac_w = _tokenizer_model(xs, nfr)
    eng = model.engine
    try:
        depths, ratios = [3, 3, 3, 3, 3, 3, 8], [8, 5, 5, 4, 2, 2]
        with _Threads(), torch.no_grad():
            ref = codec.encoder_forward(ac_w, wav[None, None], ratios, depths, None, 1e-5)[0].t()      # [75, 64]
        wd = wav.to(eng.device)
        outs = {}
        for F in (2, 4, 5, 25, 75):
            eng.set_enc_pass_frames(F)
            out = eng.new(nfr, 64)
            with torch.cuda.stream(eng.stream):
                eng.acoustic_encode(nfr, wd, out)
            eng.sync()
            outs[F] = out.cpu()
            e_ref, e_row = rel_err(out, ref), row_err(out, ref)
            e_pair = rel_err(out, outs[2])
            print(f"[encoder xsplit={xs}] {F:2d} frames/pass: vs oracle rel-L2 {e_ref:.3e} (worst frame {e_row:.3e}), vs 2 frames/pass {e_pair:.3e}")
            assert e_ref <= tol_ref, (xs, F, e_ref)
            assert e_row <= 2 * tol_ref, (xs, F, e_row)
            assert e_pair <= tol_pair, (xs, F, e_pair)
    finally:
        eng.close()


@pytest.mark.parametrize("xs,tol", [(1, 1.5e-2), (3, 1e-5)])
def test_voice_prompt_encoder_ragged_at_real_widths(xs, tol):
    """What every real wav hits: a 10-s voice prompt plus 1,234 stray samples (76 frames by the processor's ceil,
    vibevoice_processor.py:491) beside a shorter speaker (47 frames + 777 samples) that the processor zero-pads to the batch
    tensor's width.  The reference encodes the [2, 1, S] tensor non-streaming and right-pads PER strided conv layer
    (modular_vibevoice_tokenizer.py:127-134, 384-418); the product goes through _process_speech_inputs' path: whole frames of
    zero-padded waveform plus valid_samples = S for every row (vv_acoustic_encode_ragged).  Against the oracle's one-sequence
    non-streaming encode of the unpadded batch tensor, EVERY frame including the last, partial one; pass sizes 76 (one pass) and
    25 (the partial frame falls into a one-frame last pass)."""
    S = 75 * 3200 + 1234
    n_b = 47 * 3200 + 777
    nfr = -(-S // 3200)
    g = torch.Generator().manual_seed(76)
    wav = torch.zeros(2, S)
    wav[0] = torch.rand(S, generator=g) * 0.2 - 0.1
    wav[1, :n_b] = torch.rand(n_b, generator=g) * 0.2 - 0.1
    model, ac_w = _tokenizer_model(xs, nfr)
    eng = model.engine
    try:
        depths, ratios = [3, 3, 3, 3, 3, 3, 8], [8, 5, 5, 4, 2, 2]
        with _Threads(), torch.no_grad():
            ref = codec.encoder_forward(ac_w, wav[:, None], ratios, depths, None, 1e-5).permute(0, 2, 1)      # [2, 76, 64]
        assert ref.shape[1] == nfr
        padded = torch.zeros(2, nfr * 3200)
        padded[:, :S] = wav
        wd = padded.to(eng.device)
        for F in (nfr, 25):
            eng.set_enc_pass_frames(F)
            out, whole = eng.new(2, nfr, 64), eng.new(2, nfr, 64)
            with torch.cuda.stream(eng.stream):
                for i in range(2):
                    eng.acoustic_encode(nfr, wd[i], out[i], valid_samples=S)
                    eng.acoustic_encode(nfr, wd[i], whole[i])
            eng.sync()
            for i in range(2):
                e_ref, e_row, e_last = rel_err(out[i], ref[i]), row_err(out[i], ref[i]), rel_err(out[i, -1], ref[i, -1])
                e_whole_last = rel_err(whole[i, -1], ref[i, -1])
                print(f"[ragged encoder xsplit={xs}] speaker {i}, {F} frames/pass: rel-L2 {e_ref:.3e}, worst frame {e_row:.3e}, partial frame "
                      f"{e_last:.3e} (whole-frame padding: {e_whole_last:.3e})")
                assert e_ref <= tol and e_row <= 2 * tol and e_last <= 2 * tol, (xs, F, i, e_ref, e_row, e_last)
                assert rel_err(whole[i, :-1], ref[i, :-1]) <= tol            # causal: only the partial frame can tell the two paddings apart
            assert rel_err(whole[0, -1], ref[0, -1]) > 10 * rel_err(out[0, -1], ref[0, -1])   # ... and it does, where the signal ends in it
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- (b) Streaming-0.5B, timed mode
def _streaming_inputs(om, seed, n_text):
    g = synth.Gen(seed)
    prompt = torch.from_numpy(g.rng.integers(0, 300, (23,)))
    text = torch.from_numpy(g.rng.integers(0, 300, (n_text,)))
    bank = {}

    def noise_fn(frame, n2):
        if frame not in bank:
            bank[frame] = synth.Gen(seed * 100 + frame).normal((n2, 64), 1.0, mat=False)
        return bank[frame]
    return prompt, text, noise_fn


def test_streaming_generate_in_the_timed_mode_at_0p5b_widths():
    import test_gpu_streaming as tgs
    n_lm, n_tts = 2, 4
    lmcfg = dataclasses.replace(GEOM["0.5b"], layers=n_lm + n_tts, vocab=320, max_pos=512)
    old = synth.Gen
    synth.Gen = _FastGen
    try:
        om, model, cfg = tgs.build(n_lm, n_tts, use_graph=True, xsplit=1, lmcfg=lmcfg, head_layers=4, model_dtype=torch.bfloat16)
    finally:
        synth.Gen = old
    om.t_cast_dtype = torch.bfloat16
    eng = model.engine
    try:
        max_new = 11 + 24                                                      # 11 text tokens (windows of 5, 5, 1) + four speech windows
        # ---- place the EOS inside the second or third speech window: the classifier's bias is chosen from an oracle run that
        # never stops, so that exactly one frame (not the last of its window) crosses 0 with a margin on both sides; the first
        # seeded input set whose logit trace has such a frame is used
        om.eos["fc2.bias"] = torch.tensor([-100.0])
        pick = None
        for seed in range(21, 61):
            prompt, text, noise_fn = _streaming_inputs(om, seed, n_text=11)
            probe = []
            pre = ogs.make_preset(om, prompt, 305)
            with torch.no_grad():
                ogs.oracle_generate_streaming(om, pre, text, 1.5, 5, noise_fn, pre.tts_cache.length + max_new, probe)
            raw = [t["eos"] + 100.0 for t in probe]
            cands = [f for f in range(6, min(17, len(raw))) if f % 6 != 5]     # second / third window, not a window's last frame
            best = max(cands, key=lambda f: raw[f] - max(raw[:f]))
            gap = raw[best] - max(raw[:best])
            if gap > 0.1 * (max(raw) - min(raw)):
                pick = best
                break
        assert pick is not None, "no seeded input set puts a stand-out EOS logit inside a window"
        bias = -(raw[pick] + max(raw[:pick])) / 2.0
        om.eos["fc2.bias"] = torch.tensor([bias])
        eng.upload("eos.fc2.bias", torch.tensor([bias]))
        # ---- oracle run, then the engine teacher-forced with the oracle's latents
        otr = []
        pre_o = ogs.make_preset(om, prompt, 305)
        max_length = pre_o.tts_cache.length + max_new
        n_tok, audio, reach, fin = ogs.oracle_generate_streaming(om, pre_o, text, 1.5, 5, noise_fn, max_length, otr)
        assert fin and not reach
        assert len(otr) == (pick // 6 + 1) * 6, (len(otr), pick)               # the window that holds the EOS is completed
        htr = []
        pre_e = tgs.preset_for_engine(ogs.make_preset(om, prompt, 305), n_lm, 0)
        out = model.generate(tts_text_ids=text[None], all_prefilled_outputs=pre_e, cfg_scale=1.5, max_new_tokens=max_new,
                             _noise_fn=noise_fn, _trace=htr, _teacher_latents=lambda f: otr[f]["latent"] if f < len(otr) else None)
        assert len(htr) == len(otr)
        wl = wh = we = 0.0
        for a, b in zip(htr, otr):
            wl, wh = max(wl, rel_err(a["latent"], b["latent"])), max(wh, rel_err(a["tts_last"], b["tts_last"]))
            we = max(we, abs(a["eos"] - b["eos"]))
            assert (a["eos"] > 0) == (b["eos"] > 0)
        print(f"[streaming timed mode, teacher-forced] EOS at frame {pick} of {len(otr)}, worst latent rel-L2 {wl:.3e}, "
              f"TTS hidden {wh:.3e}, EOS logit |diff| {we:.3e} (decision margin {gap / 2:.3f})")
        assert wl <= 2e-2 and wh <= 2e-2, (wl, wh)          # measured 5.7e-3 / 3.9e-3 (SURVEY 8d allows 5e-2 against the fp32 oracle)
        assert bool(out.reach_max_step_sample[0]) == reach
        assert out.speech_outputs[0].shape[-1] == audio.shape[-1] == (pick + 1) * 3200      # chunks after the EOS are dropped
        wa, wb = out.speech_outputs[0][0].float().cpu(), audio[0]
        for f in range(pick + 1):
            fa, fb = wa[f * 3200:(f + 1) * 3200], wb[f * 3200:(f + 1) * 3200]
            assert abs(20 * math.log10(float(fa.norm()) / float(fb.norm()))) <= 0.5, f
            assert 20 * math.log10(float(fb.norm()) / max(1e-30, float((fa - fb).norm()))) >= 25.0, f
        assert eng.stat(1) > 0                                                  # hipGraphs captured and replayed
        # ---- free-running: nothing injected; the first window has no feedback from a previous bf16 frame beyond itself
        htr2 = []
        pre_e = tgs.preset_for_engine(ogs.make_preset(om, prompt, 305), n_lm, 0)
        out2 = model.generate(tts_text_ids=text[None], all_prefilled_outputs=pre_e, cfg_scale=1.5, max_new_tokens=max_new,
                              _noise_fn=noise_fn, _trace=htr2)
        first = rel_err(htr2[0]["latent"], otr[0]["latent"])
        assert first <= 5e-2, first
        n_cmp = min(6, out2.speech_outputs[0].shape[-1] // 3200)
        wa = out2.speech_outputs[0][0].float().cpu()
        worst = 0.0
        for f in range(n_cmp):
            fa, fb = wa[f * 3200:(f + 1) * 3200], wb[f * 3200:(f + 1) * 3200]
            worst = max(worst, abs(20 * math.log10(float(fa.norm()) / float(fb.norm()))))
        print(f"[streaming timed mode, free-running] first latent rel-L2 {first:.3e}, worst frame RMS over the first window {worst:.3f} dB, "
              f"{len(htr2)} frames (oracle {len(otr)})")
        assert worst <= 0.5, worst
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- (c) one-pass 10,922-row prefill
def test_one_pass_prefill_of_10922_rows_at_7b_widths():
    """The pass bench.py times: 10,922 prompt rows x (28 q / 4 kv heads x 128, hidden 3584, MLP 18944) through ONE call --
    vv_pack_rows, vv_gemm4 (QKV with RoPE + append in its epilogue / o / gate-up / down), vv_attn_prefill4 with 171 stages per workgroup -- then
    one decode step on top of the cache it wrote.  Row by row against oracle/lm.py: its fp32 form (bf16-mode bound) and its
    bf16-input form (what is left is summation order and the online-softmax rescaling)."""
    L0 = 10922
    c = GEOM["7b"]
    s = build_fast(c, xsplit=1, max_ctx=L0 + 128, max_rows=L0, head_layers=1)
    eng = s.eng
    try:
        H = c.hidden
        g = _FastGen(1092)
        x = g.normal((L0 + 1, H), 1.0, mat=False)
        hid = eng.new(L0, H)
        xd = dev(x, eng)
        with torch.cuda.stream(eng.stream):
            eng.lm_forward_span(0, 0, L0, xd[:L0], hid)
            out1 = eng.new(1, H)
            eng.lm_forward([(0, L0)], xd[L0:], out1)
        eng.sync()
        got, got1 = hid.float().cpu(), out1.float().cpu()
        del hid
        from oracle import lm as olm
        mk = lambda **k: olm.Qwen2Oracle(s.lm_w, c.layers, c.heads, c.kv_heads, c.head_dim, c.theta, c.eps, kv_round_bf16=True,
                                         attn_rows=512, **k)
        with _Threads():
            with torch.no_grad():
                m16 = mk(mfma_in_bf16=True)
                c16 = m16.new_cache()
                ref16 = m16.forward(x[:L0], c16)
                ref16_1 = m16.forward(x[L0:], c16)
                m32 = mk()
                c32 = m32.new_cache()
                ref32 = m32.forward(x[:L0], c32)
                ref32_1 = m32.forward(x[L0:], c32)
        e16, r16 = rel_err(got, ref16), row_err(got, ref16)
        e32, r32 = rel_err(got, ref32), row_err(got, ref32)
        d16, d32 = rel_err(got1, ref16_1), rel_err(got1, ref32_1)
        print(f"[one-pass prefill, 10922 rows, 7B widths] vs bf16-input oracle: rel-L2 {e16:.3e}, worst row {r16:.3e}; vs fp32 oracle: "
              f"{e32:.3e}, worst row {r32:.3e}; decode step on its cache: {d16:.3e} / {d32:.3e}")
        # measured: 1.2e-3 / 2.5e-3 (bf16-input form), 1.6e-3 / 2.8e-3 (fp32 form), decode step 2.1e-3 / 1.5e-3
        assert e32 <= 5e-3 and r32 <= 1e-2, (e32, r32)
        assert e16 <= 3e-3 and r16 <= 6e-3, (e16, r16)
        assert d32 <= 6e-3 and d16 <= 6e-3, (d32, d16)
    finally:
        eng.close()


def test_two_pass_prefill_with_the_fused_qkv_epilogue_at_a_position_offset():
    """Two consecutive 3,700-row passes of one 7B-width layer (vv_gemm4 shapes: QKV = 18 x 15 tiles -> bias + RoPE + KV append run
    in the GEMM's epilogue; the attention writes the o-projection's packed operand): the second pass starts at position 3,700, so the
    epilogue's rotation angles and cache addresses and the attention's causal prefix all depend on rows[0].pos.  Row by row against
    the oracle's single 7,400-row forward, then a decode step on top of the cache both passes wrote."""
    L1 = 3700
    c = GEOM["7b"]
    s = build_fast(c, xsplit=1, max_ctx=2 * L1 + 128, max_rows=L1, head_layers=1)
    eng = s.eng
    try:
        H = c.hidden
        g = _FastGen(3700)
        x = g.normal((2 * L1 + 1, H), 1.0, mat=False)
        xd = dev(x, eng)
        xin, hid, out1 = eng.new(L1, H), eng.new(L1, H), eng.new(1, H)
        with torch.cuda.stream(eng.stream):
            # the same buffers for both passes: the second one REPLAYS the first one's captured graph, only the row table differs
            xin.copy_(xd[:L1])
            eng.lm_forward_span(0, 0, L1, xin, hid)
            hid_a = hid.clone()
            xin.copy_(xd[L1:2 * L1])
            eng.lm_forward_span(0, L1, L1, xin, hid)
            hid_b = hid.clone()
            eng.lm_forward([(0, 2 * L1)], xd[2 * L1:], out1)
        eng.sync()
        got = torch.cat([hid_a.float().cpu(), hid_b.float().cpu()])
        got1 = out1.float().cpu()
        from oracle import lm as olm
        m16 = olm.Qwen2Oracle(s.lm_w, c.layers, c.heads, c.kv_heads, c.head_dim, c.theta, c.eps, kv_round_bf16=True, attn_rows=512,
                              mfma_in_bf16=True)
        with _Threads():
            with torch.no_grad():
                c16 = m16.new_cache()
                ref = m16.forward(x[:2 * L1], c16)
                ref1 = m16.forward(x[2 * L1:], c16)
        e_a, e_b = rel_err(got[:L1], ref[:L1]), rel_err(got[L1:], ref[L1:])
        r_a, r_b = row_err(got[:L1], ref[:L1]), row_err(got[L1:], ref[L1:])
        d1 = rel_err(got1, ref1)
        print(f"[two-pass prefill, fused QKV epilogue] pass 1: rel-L2 {e_a:.3e}, worst row {r_a:.3e}; pass 2 (pos 3700..): {e_b:.3e}, "
              f"worst row {r_b:.3e}; decode step: {d1:.3e}")
        assert e_a <= 3e-3 and r_a <= 6e-3, (e_a, r_a)
        assert e_b <= 3e-3 and r_b <= 6e-3, (e_b, r_b)
        assert d1 <= 6e-3, d1
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- (c2) the GEMM's K-split partial round
@pytest.mark.parametrize("epi", prefill_shapes.K_SPLIT_ROUND_EPIS)
@pytest.mark.parametrize("T,N,K", prefill_shapes.K_SPLIT_ROUND)
def test_prefill_gemm4_k_split_round(epi, T, N, K):
    """vv_gemm4_kernel with the tiles past its last whole round of 256 workgroups split along K (prefill.hip): the contributors'
    partial accumulators travel through the workspace (write-through + arrival word), the last part adds them in part order
    and runs the epilogue.  Shapes (tests/prefill_shapes.py; test_prefill_plan_cpu.py asserts that the plan splits every one of them
    under every epilogue): 17 x 17 = 289 tiles (SwiGLU: 33 x 17 = 561) with ragged T / N and an odd k-tile count, XCD 0 with one
    more remainder tile than the others (the early-exit path), split 4; 16 x 17 = 272 tiles (SwiGLU 544), 2 (4) remainder tiles
    on every XCD, split 4; 29 x 9 = 261 tiles (SwiGLU: 58 x 9 = 522), ragged T / N, 49 k-tiles: one remainder tile on XCDs 0-4
    and none on 5-7 (SwiGLU: two on XCDs 0-1, one on the others), split 3 = 25 steps / 8.  Against the
    bf16-rounded-activation reference at the bounds of test_prefill_gemm3, against the unsplit kernel (summation order only),
    and launched twice (the arrival words are reset by the consumer)."""
    geom, max_rows = prefill_shapes.K_SPLIT_ROUND_ENGINE
    s = build_fast(GEOM[geom], xsplit=1, max_ctx=128, max_rows=max_rows, head_layers=1)
    eng = s.eng
    try:
        g = _FastGen(7700 + T + N + K + epi)
        w = g.normal((N, K), 1.0 / np.sqrt(K))
        w2 = g.normal((N, K), 1.0 / np.sqrt(K))
        x = g.normal((T, K), 1.0, mat=False)
        nw = g.vec(K, 0.1, 1.0)
        bias = g.vec(N, 0.3)
        y0 = g.normal((T, N), 1.0, mat=False)
        norm = epi == 1
        xin = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * nw if norm else x
        x16 = synth.bf16_round(xin)
        mm = lambda a, b: (a.to(eng.device, torch.float64) @ b.to(eng.device, torch.float64).t()).float().cpu()   # reference only
        a16 = mm(x16, w)
        ref16 = {0: a16, 1: a16 + bias, 4: y0 + a16, 3: torch.nn.functional.silu(a16) * (mm(x16, w2) if epi == 3 else 0.0)}[epi]
        wp, w2p = eng.pack_matrix(w), (eng.pack_matrix(w2) if epi == 3 else None)
        xd = dev(x, eng)
        outs = []
        for ksplit in (True, True, False):
            y = dev(y0.clone(), eng)
            with torch.cuda.stream(eng.stream):
                eng.gemm3_raw(wp, xd, y, N, K, epi=epi, w2p=w2p, nw=dev(nw, eng) if norm else None, eps=1e-5,
                              bias=dev(bias, eng) if epi == 1 else None, ksplit=ksplit)
            eng.sync()
            outs.append(y.float().cpu())
        tight = 3e-3 if epi == 3 else 2e-4
        for y in outs:
            assert rel_err(y, ref16) <= tight, (rel_err(y, ref16), tight)
            assert float((y - ref16).abs().max()) <= 4 * tight * float(ref16.abs().max()), float((y - ref16).abs().max())
        assert torch.equal(outs[0], outs[1])                                   # deterministic: fixed part order
        assert rel_err(outs[0], outs[2]) <= (3e-3 if epi == 3 else 2e-6), rel_err(outs[0], outs[2])
    finally:
        eng.close()


@pytest.mark.parametrize("epi", prefill_shapes.SHORT_PROMPT_EPIS)
@pytest.mark.parametrize("T,N,K", prefill_shapes.SHORT_PROMPT)
def test_short_prompt_gemm3_k_split_and_reduce(epi, T, N, K):
    """Short prompts (round 4): vv_gemm3_kernel launches a few dozen 128 x 128 tiles for such shapes (36 for the 1.5B down projection
    of a 330-token prompt), so K is split over grid.y into dense fp32 partial tensors and vv_g3_reduce_kernel adds them in part order
    with the bias / residual -- with two LDS stage buffers, the next stage's copies issued before the current stage's MFMAs.
    Shapes: the 1.5B down / QKV projections at 330 rows, ragged T / N with an odd k-tile count (33), a 75-row voice prompt at 0.5B
    widths, a one-block problem.  Against the bf16-rounded-activation reference at test_prefill_gemm3's bounds, against the unsplit
    kernel (no workspace: summation order only), twice (bit-identical repeats)."""
    geom, max_rows = prefill_shapes.SHORT_PROMPT_ENGINE
    s = build_fast(GEOM[geom], xsplit=1, max_ctx=128, max_rows=max_rows, head_layers=1)
    eng = s.eng
    try:
        g = _FastGen(8800 + T + N + K + epi)
        w = g.normal((N, K), 1.0 / np.sqrt(K))
        x = g.normal((T, K), 1.0, mat=False)
        nw = g.vec(K, 0.1, 1.0)
        bias = g.vec(N, 0.3)
        y0 = g.normal((T, N), 1.0, mat=False)
        norm = epi == 1
        xin = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * nw if norm else x
        x16 = synth.bf16_round(xin)
        a16 = (x16.to(eng.device, torch.float64) @ w.to(eng.device, torch.float64).t()).float().cpu()
        ref16 = {0: a16, 1: a16 + bias, 4: y0 + a16}[epi]
        wp, xd = eng.pack_matrix(w), dev(x, eng)
        outs = []
        for ksplit in (True, True, False):
            y = dev(y0.clone(), eng)
            with torch.cuda.stream(eng.stream):
                eng.gemm3_raw(wp, xd, y, N, K, epi=epi, nw=dev(nw, eng) if norm else None, eps=1e-5,
                              bias=dev(bias, eng) if epi == 1 else None, ksplit=ksplit)
            eng.sync()
            outs.append(y.float().cpu())
        for y in outs:
            assert rel_err(y, ref16) <= 2e-4, rel_err(y, ref16)
            assert float((y - ref16).abs().max()) <= 8e-4 * float(ref16.abs().max()), float((y - ref16).abs().max())
        assert torch.equal(outs[0], outs[1])                                   # deterministic: fixed part order
        assert rel_err(outs[0], outs[2]) <= 2e-6, rel_err(outs[0], outs[2])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- (d) bf16-input references
@pytest.mark.parametrize("L0,chunk,heads,kv_heads,hd", [(4180, 512, 4, 2, 128), (1000, 1024, 7, 1, 128), (1555, 1024, 14, 2, 64), (90, 128, 4, 2, 128),
                                                        (1330, 1024, 12, 2, 128), (700, 512, 3, 1, 128), (333, 256, 2, 2, 128), (1100, 1024, 5, 1, 64)])
def test_prefill_attention_v3_against_the_bf16_input_oracle(L0, chunk, heads, kv_heads, hd):
    """vv_attn_prefill4 (+ the packed-activation GEMMs around it) ROW BY ROW against the oracle with bf16 matrix-unit inputs: one
    softmax update per 64-position stage, v_permlane16/32_swap row exchange (a clang quirk reads the wrong element of the builtin's
    result unless it goes through unsigned temporaries -- this test is what pins it), mask-free path below the diagonal.  A masking
    or tail-stage slip is an O(1) error in single rows, which a whole-tensor norm hides.  Shapes: ragged tails with 1..32 and
    33..64 live positions in the last stage, passes that start at a non-zero position, GQA groups 1 / 2 / 3 / 5 / 6 / 7 (a workgroup
    takes four (row tile, query head) units: groups that are not multiples of 4 make it straddle two row tiles, groups below 4 up to
    four, and the last workgroup is partly idle), both head widths, a prompt shorter than one pass."""
    from test_gpu_geometry import _prefill_probe
    got, s, x = _prefill_probe(L0, chunk, heads, kv_heads, hd)
    c = s.lmcfg
    from oracle import lm as olm
    m = olm.Qwen2Oracle(s.lm_w, c.layers, c.heads, c.kv_heads, c.head_dim, c.theta, c.eps, kv_round_bf16=True, mfma_in_bf16=True,
                        attn_rows=512)
    with _Threads(), torch.no_grad():
        ref = m.forward(x, m.new_cache())
    e, r = rel_err(got, ref), row_err(got, ref)
    print(f"[prefill attention vs bf16-input oracle] L0={L0} chunk={chunk} heads={heads}/{kv_heads}x{hd}: rel-L2 {e:.3e}, worst row {r:.3e}")
    assert e <= 3e-3 and r <= 5e-3, (e, r)


@pytest.mark.parametrize("tag", ["7b", "1.5b"])
def test_batch_decode_rows_against_the_bf16_input_oracle(tag):
    """16 decode rows (8 utterances, cond + uncond) of one layer at real widths: vv_pack16 + vv_gemv16p (QKV, o, gate/up with
    packed SwiGLU output, down) and the fused decode attention; then the 16-row sampler forms at the head's width.  Against the
    oracle with bf16 matrix-unit inputs: <= 5e-3 per row instead of the 5e-2 of the fp32 comparison."""
    c = GEOM[tag]
    s = build_fast(c, xsplit=1, max_ctx=256, max_rows=64, head_layers=2, n_slots=8)
    eng = s.eng
    try:
        from oracle import lm as olm
        H = c.hidden
        m = olm.Qwen2Oracle(s.lm_w, c.layers, c.heads, c.kv_heads, c.head_dim, c.theta, c.eps, kv_round_bf16=True, mfma_in_bf16=True)
        g = _FastGen(160)
        caches = [m.new_cache() for _ in range(16)]
        lens = [0] * 16
        worst = 0.0
        for step in range(3):
            rows = list(range(16)) if step != 1 else [0, 2, 3, 5, 8, 9, 11, 12, 14]       # 16 rows, then 9, then 16 again
            x = g.normal((len(rows), H), 1.0, mat=False)
            out = eng.new(len(rows), H)
            with torch.cuda.stream(eng.stream):
                eng.lm_forward([(r, lens[r]) for r in rows], dev(x, eng), out)
            eng.sync()
            with torch.no_grad():
                ref = torch.cat([m.forward(x[i:i + 1], caches[r]) for i, r in enumerate(rows)])
            for r in rows:
                lens[r] += 1
            worst = max(worst, row_err(out, ref))
        print(f"[gemv16p decode rows, {tag}] worst row rel-L2 vs bf16-input oracle {worst:.3e}")
        assert worst <= 5e-3, worst                 # measured 2.5e-3 (7B and 1.5B widths)
        n = 8
        pos = g.normal((n, H), 1.0, mat=False)
        neg = g.normal((n, H), 1.0, mat=False)
        noise = g.normal((2 * n, 64), 1.0, mat=False)
        with torch.no_grad():
            refl = dpm.sample_speech_tokens(lambda a, t, cnd: head.head_forward(s.head_w, a, t, cnd, s.hc.layers, s.hc.eps, mfma_in_bf16=True),
                                            pos, neg, 1.3, 10, noise)
        eng.set_num_steps(10)
        lat = eng.new(n, 64)
        with torch.cuda.stream(eng.stream):
            eng.diffusion_sample(n, dev(torch.cat([pos, neg]), eng), dev(noise[:n], eng), 1.3, lat)
        eng.sync()
        e = row_err(lat, refl)
        print(f"[16-row sampler forms, {tag}] worst latent rel-L2 vs bf16-input oracle {e:.3e}")
        assert e <= 1e-2, e
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- (e) bf16 HIP vs bf16 PyTorch-ROCm eager
def test_bf16_hip_against_bf16_pytorch_rocm_eager():
    """"bf16 HIP vs bf16 PyTorch-ROCm reference on identical inputs (teacher-forced, per step): latent rel-L2 <= 2e-2,
    hidden-state rel-L2 <= 2e-2, token decisions identical under the forced schedule".  The reference leg is the oracle loop with
    every weight and activation in bf16 on this GPU (plain eager torch ops = what the reference's generate() issues on a GPU);
    the HIP leg is xsplit=1 + hipGraph, fed per step with the eager run's next-step embeddings."""
    import test_gpu_timed_mode as tm
    from test_gpu_generate import make_inputs
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    s = build_small(synth.LMCfg(), xsplit=1, use_graph=True, n_slots=2, max_ctx=512)
    try:
        D, E, S, X = tm.D, tm.E, tm.S, tm.X
        forced = [[D, D, D, D, E, S, D, D, D, D, D, X], [D, E, S, D, D, D, D, D, X]]
        B, steps, seed = 2, 5, 5
        ids, mask, _, _, _ = make_inputs(s, B, False, seed)       # text-only prompts: the tokenizers' bf16 eager convolutions are
        bank = {}                                                 # exercised by the per-frame decode / re-encode of the loop

        def noise_fn(step, n2):
            return bank.setdefault((step, n2), synth.Gen(seed * 1000 + step).normal((n2, 64), 1.0, mat=False))
        devc = s.eng.device
        bf = lambda w: {k: v.to(devc, torch.bfloat16) for k, v in w.items()}
        from oracle import lm as olm
        with torch.device(devc):
            cL = s.lmcfg
            lm = olm.Qwen2Oracle(bf(s.lm_w), cL.layers, cL.heads, cL.kv_heads, cL.head_dim, cL.theta, cL.eps)
            om = ogen.OracleModel(lm=lm, lm_head=s.lm_head.to(devc, torch.bfloat16), head_w=bf(s.head_w), head_layers=s.hc.layers,
                                  ac_w=bf(s.ac_w), sem_w=bf(s.sem_w), ac_conn=bf(s.ac_conn), sem_conn=bf(s.sem_conn),
                                  ratios=s.cc.ratios, enc_depths=s.cc.enc_depths, dec_depths=s.cc.dec_depths,
                                  sem_depths=s.sc.enc_depths, scaling=s.scaling, bias=s.bias,
                                  max_position_embeddings=s.lmcfg.max_pos, head_eps=s.hc.eps, codec_eps=s.cc.eps)
            om.t_cast_dtype = torch.bfloat16
            otr = ogen.Trace()
            to = lambda t: t.to(devc) if t is not None else None
            with torch.no_grad():
                oseq, oaud, omax = ogen.oracle_generate(
                    om, tm.TOK, to(ids), to(mask), cfg_scale=1.3, num_steps=steps,
                    noise_fn=lambda step, n2: noise_fn(step, n2).to(devc, torch.bfloat16), forced_tokens=forced, trace=otr)
        torch.cuda.synchronize()
        cfgd = {"decoder_config": {"max_position_embeddings": s.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": steps},
                "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
        m = VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.bfloat16)
        m.set_speech_factors(s.scaling, s.bias)
        m.set_ddpm_inference_steps(steps)
        htr = ogen.Trace()
        out = m.generate(input_ids=ids, attention_mask=mask, cfg_scale=1.3,
                         tokenizer=tm.TOKNS, generation_config={"do_sample": False}, _forced_tokens=forced, _noise_fn=noise_fn,
                         _trace=htr, show_progress_bar=False,
                         _teacher_embeds=lambda step, rows: otr.next_embeds[step][rows].float())
        assert torch.equal(out.sequences.cpu(), oseq.cpu())
        assert len(htr.latents) == len(otr.latents) > 0
        wl = wh = wn = 0.0
        for a, b in zip(htr.latents, otr.latents):
            wl = max(wl, rel_err(a, b))
        for a, b in zip(htr.pos_hidden, otr.pos_hidden):
            if a.shape == b.shape:
                wh = max(wh, rel_err(a, b))
        for a, b in zip(htr.neg_hidden, otr.neg_hidden):
            wn = max(wn, rel_err(a, b))
        print(f"[bf16 HIP vs bf16 PyTorch-ROCm eager, teacher-forced] worst latent rel-L2 {wl:.3e}, positive hidden {wh:.3e}, negative hidden {wn:.3e}")
        assert wl <= 2e-2 and wh <= 2e-2 and wn <= 2e-2, (wl, wh, wn)
    finally:
        s.eng.close()


# ---------------------------------------------------------------------------------------------- from_pretrained on the GPU engine
def test_from_pretrained_checkpoint_directory_on_the_gpu_engine(tmp_path, monkeypatch):
    """demo/inference_from_file.py:297-317 on the real engine: from_pretrained(<dir with config.json + safetensors shards>) --
    including the warm-up it runs -- then generate() on the inputs, forced token plan and recorded noise draws of a golden the
    REFERENCE's own generate() produced (tests/golden/generate_forced_b1.npz): sequences identical, waveform rel-L2 <= 1e-3
    (xsplit = 3).  The same directory, placed under $VIBEVOICE_MODEL_DIR, is what bench.py's checkpoint hook picks up."""
    import importlib.util
    import json
    import os
    from safetensors.torch import save_file
    from test_dropin_cpu import TOK, tiny_reference_config, tiny_reference_state_dict
    from test_oracle_golden import G as GOLD
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    d = tmp_path / "VibeVoice-1.5B"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(tiny_reference_config()))
    sd = {k: v.contiguous() for k, v in tiny_reference_state_dict().items()}
    keys = sorted(sd)
    save_file({k: sd[k] for k in keys[::2]}, str(d / "model-00001-of-00002.safetensors"))
    save_file({k: sd[k] for k in keys[1::2]}, str(d / "model-00002-of-00002.safetensors"))
    model = VibeVoiceForConditionalGenerationInference.from_pretrained(str(d), torch_dtype=torch.float32, device_map="cuda",
                                                                       xsplit=3, use_graph=True, max_ctx=512, n_slots=2, max_rows=16)
    try:
        model.eval()
        model.set_ddpm_inference_steps(num_steps=5)
        model.speculate_sampling = False          # the recorded draws are consumed strictly in order (a discarded speculation would eat one)
        assert abs(float(model.speech_scaling_factor) - 0.2) < 1e-7
        z = np.load(os.path.join(GOLD, "generate_forced_b1.npz"))
        draws = [torch.from_numpy(z[f"draw_{i}"]) for i in range(int(z["n_draws"]))]
        pre = (draws[0].reshape(1), draws[1].reshape(1, 3, 64))
        it = iter(draws[2:])
        forced = [z["forced"][0][:int(z["forced_len"][0])].tolist()]
        out = model.generate(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
                             speech_tensors=torch.from_numpy(z["speech_tensors"]), speech_masks=torch.from_numpy(z["speech_masks"]),
                             speech_input_mask=torch.from_numpy(z["speech_input_mask"]), cfg_scale=1.3, tokenizer=TOK,
                             generation_config={"do_sample": False}, _forced_tokens=forced, _prefill_noise=pre,
                             _noise_fn=lambda step, n2: next(it).reshape(n2, 64), show_progress_bar=False)
        assert torch.equal(out.sequences.cpu(), torch.from_numpy(z["sequences"]))
        ref = torch.from_numpy(z["audio_0"])
        got = out.speech_outputs[0].reshape(-1).float().cpu()
        assert got.shape == ref.shape
        err = float((got - ref).norm() / ref.norm())
        print(f"[from_pretrained on the GPU engine] waveform rel-L2 vs the reference's own generate() golden {err:.3e}")
        assert err <= 1e-3, err
    finally:
        model.engine.close()
    # bench.py's $VIBEVOICE_MODEL_DIR hook finds this directory by the released model's name; a directory without shards is not one
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_hook", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setenv("VIBEVOICE_MODEL_DIR", str(tmp_path))
    assert bench.find_checkpoint("1.5b") == str(d)
    assert bench.find_checkpoint("7b") is None
    assert sorted(k for k, _ in bench.checkpoint_tensors(str(d))) == keys


def test_long_prompt_prefill_in_one_lane_while_another_lane_decodes_a_batch():
    """The one inter-workgroup hand-off of the path (the K split of vv_gemm4's partial round, prefill.hip) relies on dispatch order for
    forward progress and on a timeout + one repeat for recovery; with lanes (vv_create_shared) a second context's grids share the chip
    with it.  Lane A runs the 10,922-row 7B-width prompt pass 20 times while lane B, a forked context on its own stream and host thread,
    keeps decoding a batch of 8 rows (the 16-row packed-activation projections + batch attention): vv_check must never fire on either
    context, no stream capture may fall back, every repetition of the prompt pass must equal -- bit for bit -- the pass lane A ran
    alone, and lane B's rows must equal its own solo run."""
    import threading
    L0 = 10922
    c = GEOM["7b"]
    s = build_fast(c, xsplit=1, max_ctx=L0 + 128, max_rows=L0, head_layers=1)
    eng = s.eng
    lane = None
    try:
        H = c.hidden
        g = _FastGen(4242)
        x = dev(g.normal((L0, H), 1.0, mat=False), eng)
        xb = dev(g.normal((40, 16, H), 1.0, mat=False), eng)
        lane = eng.fork(n_slots=8, max_rows=16, max_ctx=512)

        def prompt_pass():
            hid = eng.new(L0, H)
            with torch.cuda.stream(eng.stream):
                eng.lm_forward_span(0, 0, L0, x, hid)
            eng.sync()                                   # stream wait + vv_check
            return hid

        def decode_batch(n_steps):
            outs = []
            with torch.cuda.stream(lane.stream):
                for t in range(n_steps):
                    out = lane.new(16, H)
                    lane.lm_forward([(r, t) for r in range(16)], xb[t % 40], out)
                    outs.append(out)
            lane.sync()
            return torch.stack(outs).float().cpu()
        alone = prompt_pass().clone()
        solo_b = decode_batch(40)
        errs, got_b, stop = [], [], threading.Event()

        def lane_b():
            try:
                torch.cuda.set_device(eng.device)
                while not stop.is_set():
                    got_b.append(decode_batch(40))
            except BaseException as ex:       # noqa: BLE001
                errs.append(ex)
        th = threading.Thread(target=lane_b, name="vv-lane-b")
        th.start()
        try:
            for rep in range(20):
                hid = prompt_pass()
                assert torch.equal(hid, alone), f"repetition {rep}: the prompt pass beside a decoding lane differs from the pass alone"
        finally:
            stop.set()
            th.join()
        assert not errs, errs
        assert len(got_b) >= 1
        for gb in got_b:
            assert torch.equal(gb, solo_b)
        assert eng.stat(4) == 0 and lane.stat(4) == 0          # no capture fell back to an eager run
        print(f"[lanes] 20 prompt passes of {L0} rows beside {len(got_b)} x 40 decode steps of a 16-row batch: bit-identical, no hand-off timeout")
    finally:
        if lane is not None:
            lane.close()
        eng.close()


# ---------------------------------------------------------------------------------------------- utterance sharding over RCCL
def test_generate_sharded_over_an_rccl_process_group():
    """parallel.generate_sharded on the real engine with torch.distributed's "nccl" backend (= RCCL; a one-rank group is what a
    1-GPU box offers): the finished utterances travel as padded device tensors through dist.gather -- token sequences as int64,
    waveforms in the model dtype -- and come back in request order, identical to generate_continuous() on the same queue.  The
    2-rank behaviour of the same code (unequal shards, both ranks contributing) is covered on CPU with gloo
    (tests/test_parallel_cpu.py)."""
    import socket
    import torch.distributed as dist
    from test_gpu_generate import _mk_requests, D, E, S, X
    from vibevoice_amd import parallel
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    sm = build_small(synth.LMCfg(), xsplit=3, n_slots=2, max_ctx=512, use_graph=True)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=sm.eng.device)
    try:
        reqs = _mk_requests(sm, 4, 13)
        cfgd = {"decoder_config": {"max_position_embeddings": sm.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
        m = VibeVoiceForConditionalGenerationInference(cfgd, sm.eng, model_dtype=torch.bfloat16)
        m.set_speech_factors(sm.scaling, sm.bias)
        m.set_ddpm_inference_steps(5)
        tok = types.SimpleNamespace(speech_start_id=S, speech_end_id=E, speech_diffusion_id=D, eos_token_id=X, bos_token_id=None, pad_token_id=305)
        kw = dict(tokenizer=tok, generation_config={"do_sample": False}, cfg_scale=1.3)
        solo = m.generate_continuous(reqs, **kw)
        st = {}
        calls = {"gather": [], "all_gather": []}
        o_gather, o_all = dist.gather, dist.all_gather

        def c_gather(t, gl=None, dst=0, **k):
            calls["gather"].append((t.dtype, t.device.type, t.numel()))
            return o_gather(t, gl, dst=dst, **k)

        def c_all(lst, t, **k):
            calls["all_gather"].append((t.dtype, t.device.type, t.numel()))
            return o_all(lst, t, **k)
        dist.gather, dist.all_gather = c_gather, c_all
        try:
            got = parallel.generate_sharded(m, reqs, gather_to=0, stats=st, **kw)
        finally:
            dist.gather, dist.all_gather = o_gather, o_all
        assert st["utterances_per_rank"] == [4] and st["imbalance_max_over_mean"] == 1.0
        # the one-rank group took the collective path: three payload gathers (sequences, flags, waveforms) of DEVICE tensors over RCCL,
        # the waveforms in the model dtype, plus the three length all_gathers
        assert [c[0] for c in calls["gather"]] == [torch.int64, torch.int64, torch.bfloat16], calls
        assert all(c[1] == "cuda" for c in calls["gather"] + calls["all_gather"]) and len(calls["all_gather"]) == 3, calls
        assert calls["gather"][2][2] == sum(o.speech_outputs[0].numel() for o in solo)
        assert st["gather"]["backend"] == "nccl" and st["gather"]["on_device"] and st["gather"]["audio_dtype"] == "bfloat16"
        assert st["gather"]["payload_bytes_this_rank"] > 0 and st["gather"]["seconds"] > 0
        print(f"[rccl gather] {st['gather']}")
        assert len(got) == 4
        for a, b in zip(got, solo):
            assert torch.equal(a.sequences.cpu(), b.sequences.cpu())
            assert bool(a.reach_max_step_sample[0]) == bool(b.reach_max_step_sample[0])
            assert a.speech_outputs[0].shape == b.speech_outputs[0].shape
            assert torch.equal(a.speech_outputs[0].float().cpu(), b.speech_outputs[0].float().cpu())     # bf16 waveforms travel unchanged
        st2 = {}
        every = parallel.generate_sharded(m, reqs, gather_to=None, stats=st2, **kw)                           # the all_gather form
        assert st2["gather"]["collective"] == "all_gather"
        assert all(torch.equal(a.sequences, b.sequences) for a, b in zip(every, got))
        assert all(torch.equal(a.speech_outputs[0], b.speech_outputs[0]) for a, b in zip(every, got))
    finally:
        dist.destroy_process_group()
        sm.eng.close()
