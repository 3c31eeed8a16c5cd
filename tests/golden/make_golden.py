"""Generate tests/golden/*.npz by running the REFERENCE's own classes.

Run only in the build container (needs /root/reference):
    python tests/golden/make_golden.py

What is executed is reference code, imported through oracle/refshim.py:
  vibevoice.schedule.dpm_solver.DPMSolverMultistepScheduler
  vibevoice.modular.modular_vibevoice_diffusion_head.VibeVoiceDiffusionHead
  vibevoice.modular.modular_vibevoice_tokenizer.{VibeVoiceAcousticTokenizerModel,
      VibeVoiceSemanticTokenizerModel, VibeVoiceTokenizerStreamingCache}
  vibevoice.modular.modeling_vibevoice.SpeechConnector
  vibevoice.modular.modeling_vibevoice_inference.VibeVoiceForConditionalGenerationInference.generate   (gen_generate:
      forced single / desynchronised batch of 2 + AudioStreamer call log / greedy / length cap / ragged voice sample /
      do_sample=True, every torch.randn draw recorded)
  vibevoice.modular.modeling_vibevoice_streaming_inference.VibeVoiceStreamingForConditionalGenerationInference.generate
      (gen_generate_streaming: text windows + length cap, EOS inside a window; prefilled branches from its own forwards)
  (both through oracle/refshim.install_*_shims: transformers 4.51.3 -> 5.x API adaptation, no arithmetic)
and, for the LM (third-party arithmetic, see oracle/lm.py), the installed
transformers Qwen2Model.  Weights come from tests/synth.py (seeded, small
shapes); only inputs/outputs + a weight checksum are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402

refshim.install()
import synth  # noqa: E402


OUT_DIR = HERE          # tools/fuzz_generate_vs_reference.py points this elsewhere


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    np.savez_compressed(os.path.join(OUT_DIR, name), **out)
    print("wrote", name, {k: tuple(np.shape(v)) for k, v in out.items()})


@torch.no_grad()
def gen_dpm_and_head():
    from vibevoice.schedule.dpm_solver import DPMSolverMultistepScheduler
    from vibevoice.modular.modular_vibevoice_diffusion_head import VibeVoiceDiffusionHead
    from vibevoice.modular.configuration_vibevoice import VibeVoiceDiffusionHeadConfig

    arrs = {}
    for n in (5, 10, 20):
        s = DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="cosine",
                                        prediction_type="v_prediction")
        s.set_timesteps(n)
        arrs[f"timesteps_{n}"] = s.timesteps
        arrs[f"sigmas_{n}"] = s.sigmas
    save("dpm_schedule.npz", **arrs)

    hc = synth.HeadCfg()
    w = synth.head_weights(hc)
    cfg = VibeVoiceDiffusionHeadConfig(hidden_size=hc.hidden, head_layers=hc.layers,
                                       head_ffn_ratio=hc.ffn_ratio, rms_norm_eps=hc.eps,
                                       latent_size=hc.latent)
    head = VibeVoiceDiffusionHead(cfg).eval()
    head.load_state_dict(w, strict=True)
    g = synth.Gen(100)
    noisy = g.normal((4, hc.latent), 1.0, mat=False)
    cond = g.normal((4, hc.hidden), 1.0, mat=False)
    outs = {}
    ts = [999, 500, 100, 3]
    for t in ts:
        tt = torch.full((4,), float(t))
        outs[f"out_{t}"] = head(noisy, tt, cond)
    save("head_forward.npz", noisy=noisy, cond=cond, ts=np.array(ts), wsum=synth.checksum(w), **outs)

    # full CFG sampler: the 10 lines of sample_speech_tokens
    # (modeling_vibevoice_inference.py:697-710) driven with the reference scheduler/head
    for n_steps in (5, 10):
        s = DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="cosine",
                                        prediction_type="v_prediction")
        g = synth.Gen(200 + n_steps)
        pos = g.normal((2, hc.hidden), 1.0, mat=False)
        neg = g.normal((2, hc.hidden), 1.0, mat=False)
        noise = g.normal((4, hc.latent), 1.0, mat=False)
        cfg_scale = 1.3
        s.set_timesteps(n_steps)
        condition = torch.cat([pos, neg], dim=0)
        speech = noise.clone()
        per_step = []
        for t in s.timesteps:
            half = speech[: len(speech) // 2]
            combined = torch.cat([half, half], dim=0)
            eps = head(combined, t.repeat(combined.shape[0]).to(combined), condition=condition)
            cond_eps, uncond_eps = torch.split(eps, len(eps) // 2, dim=0)
            half_eps = uncond_eps + cfg_scale * (cond_eps - uncond_eps)
            eps = torch.cat([half_eps, half_eps], dim=0)
            speech = s.step(eps, t, speech).prev_sample
            per_step.append(speech[:2].clone())
        save(f"sampler_{n_steps}.npz", pos=pos, neg=neg, noise=noise, cfg_scale=cfg_scale,
             latent=speech[:2], per_step=torch.stack(per_step), wsum=synth.checksum(w))

    # the same loop with the scheduler demo/gradio_demo.py:142-146 installs (`noise_scheduler.from_config(config,
    # algorithm_type='sde-dpmsolver++', beta_schedule='squaredcos_cap_v2')`): scheduler.step() draws its own variance noise
    # (randn_tensor, dpm_solver.py:994-997) -- recorded here through the module's randn_tensor
    import vibevoice.schedule.dpm_solver as ref_dpm
    for n_steps in (5, 10):
        base = DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="cosine", prediction_type="v_prediction")
        s = base.from_config(base.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")
        assert s.config.algorithm_type == "sde-dpmsolver++" and s.config.prediction_type == "v_prediction"
        g = synth.Gen(300 + n_steps)
        pos = g.normal((2, hc.hidden), 1.0, mat=False)
        neg = g.normal((2, hc.hidden), 1.0, mat=False)
        noise = g.normal((4, hc.latent), 1.0, mat=False)
        cfg_scale = 1.3
        s.set_timesteps(n_steps)
        condition = torch.cat([pos, neg], dim=0)
        speech = noise.clone()
        per_step, draws = [], []
        orig = ref_dpm.randn_tensor

        def rec(shape, generator=None, device=None, dtype=None):
            t = orig(shape, generator=generator, device=device, dtype=dtype)
            draws.append(t.clone())
            return t
        ref_dpm.randn_tensor = rec
        torch.manual_seed(4000 + n_steps)
        try:
            for t in s.timesteps:
                half = speech[: len(speech) // 2]
                combined = torch.cat([half, half], dim=0)
                eps = head(combined, t.repeat(combined.shape[0]).to(combined), condition=condition)
                cond_eps, uncond_eps = torch.split(eps, len(eps) // 2, dim=0)
                half_eps = uncond_eps + cfg_scale * (cond_eps - uncond_eps)
                eps = torch.cat([half_eps, half_eps], dim=0)
                speech = s.step(eps, t, speech).prev_sample
                per_step.append(speech[:2].clone())
        finally:
            ref_dpm.randn_tensor = orig
        assert len(draws) == n_steps and tuple(draws[0].shape) == (4, hc.latent) and draws[0].dtype == torch.float32
        torch.manual_seed(4000 + n_steps)            # the draws are plain torch.randn calls on the global generator
        assert all(torch.equal(d, torch.randn(4, hc.latent)) for d in draws)
        save(f"sampler_sde_{n_steps}.npz", pos=pos, neg=neg, noise=noise, cfg_scale=cfg_scale, seed=4000 + n_steps,
             step_noise=torch.stack(draws), latent=speech[:2], per_step=torch.stack(per_step), wsum=synth.checksum(w))


@torch.no_grad()
def gen_codec():
    from vibevoice.modular.configuration_vibevoice import (VibeVoiceAcousticTokenizerConfig,
                                                           VibeVoiceSemanticTokenizerConfig)
    from vibevoice.modular.modular_vibevoice_tokenizer import (VibeVoiceAcousticTokenizerModel,
                                                               VibeVoiceSemanticTokenizerModel,
                                                               VibeVoiceTokenizerStreamingCache)
    cc = synth.CodecCfg()
    acfg = VibeVoiceAcousticTokenizerConfig(encoder_n_filters=cc.n_filters, decoder_n_filters=cc.n_filters,
                                            vae_dim=cc.vae_dim, encoder_depths=cc.depth_str,
                                            layernorm_eps=cc.eps)
    ac = VibeVoiceAcousticTokenizerModel(acfg).eval()
    w = {}
    w.update(synth.encoder_weights(cc, seed=2))
    w.update(synth.decoder_weights(cc, seed=3))
    ac.load_state_dict(w, strict=True)

    g = synth.Gen(300)
    nfr = 7
    lat = g.normal((1, nfr, cc.vae_dim), 1.0, mat=False)           # [B, T, vae]
    cache = VibeVoiceTokenizerStreamingCache()
    idx = torch.tensor([0])
    chunks = []
    reset_after = 3
    for t in range(nfr):
        chunks.append(ac.decode(lat[:, t:t + 1], cache=cache, sample_indices=idx, use_cache=True))
        if t == reset_after:
            cache.set_to_zero(idx)
    stream = torch.cat(chunks, dim=-1)
    full_a = ac.decode(lat[:, :reset_after + 1])                  # non-streaming, first segment
    full_b = ac.decode(lat[:, reset_after + 1:])
    save("codec_decode.npz", latents=lat, stream=stream, reset_after=reset_after,
         nonstream_a=full_a, nonstream_b=full_b, wsum=synth.checksum(w))

    # acoustic encoder, non-streaming (voice-prompt path, _process_speech_inputs :154)
    wav = g.uniform((2, 3200 * 3), -0.5, 0.5)
    mean = ac.encode(wav.unsqueeze(1)).mean                        # [2, 3, vae]
    save("acoustic_encode.npz", wav=wav, mean=mean, wsum=synth.checksum(w))

    # semantic encoder, streaming, incl. mid-stream zeroing
    sc = synth.CodecCfg(vae_dim=128)
    scfg = VibeVoiceSemanticTokenizerConfig(encoder_n_filters=sc.n_filters, vae_dim=sc.vae_dim,
                                            encoder_depths=sc.depth_str, layernorm_eps=sc.eps)
    sem = VibeVoiceSemanticTokenizerModel(scfg).eval()
    sw = synth.encoder_weights(sc, seed=7)
    sem.load_state_dict(sw, strict=True)
    nfr = 6
    audio = g.uniform((1, 1, 3200 * nfr), -0.5, 0.5)
    cache = VibeVoiceTokenizerStreamingCache()
    outs = []
    for t in range(nfr):
        outs.append(sem.encode(audio[:, :, t * 3200:(t + 1) * 3200], cache=cache, sample_indices=idx,
                               use_cache=True).mean)
        if t == 2:
            cache.set_to_zero(idx)
    stream = torch.cat(outs, dim=1)                                # [1, nfr, 128]
    full_a = sem.encode(audio[:, :, :3 * 3200]).mean
    save("semantic_encode.npz", audio=audio, stream=stream, reset_after=2, nonstream_a=full_a,
         wsum=synth.checksum(sw))


@torch.no_grad()
def gen_connector():
    from vibevoice.modular.modeling_vibevoice import SpeechConnector
    for name, din in (("ac", 64), ("sem", 128)):
        H = 96
        w = synth.connector_weights(din, H, seed=4 if name == "ac" else 8)
        c = SpeechConnector(din, H).eval()
        c.load_state_dict(w, strict=True)
        x = synth.Gen(400).normal((3, din), 1.0, mat=False)
        save(f"connector_{name}.npz", x=x, y=c(x), wsum=synth.checksum(w))


@torch.no_grad()
def gen_lm():
    from transformers import Qwen2Config, Qwen2Model
    for tag, cfg in (("d64", synth.LMCfg()), ("d128", synth.LMCfg(hidden=256, heads=2, kv_heads=1, inter=384)),
                     ("gqa", synth.LMCfg(hidden=256, heads=4, kv_heads=2, inter=320, layers=3))):
        w = synth.lm_weights(cfg)
        hc = Qwen2Config(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.layers,
                         num_attention_heads=cfg.heads, num_key_value_heads=cfg.kv_heads,
                         vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos,
                         rope_theta=cfg.theta, rms_norm_eps=cfg.eps, tie_word_embeddings=True,
                         attn_implementation="eager")
        m = Qwen2Model(hc).eval()
        m.load_state_dict(w, strict=True)
        g = synth.Gen(500)
        L0, nd = 13, 5
        ids = torch.from_numpy(g.rng.integers(0, cfg.vocab, (1, L0)))
        out = m(input_ids=ids, use_cache=True)
        hs = [out.last_hidden_state[0]]
        past = out.past_key_values
        dec_in = g.normal((nd, cfg.hidden), 1.0, mat=False)
        for i in range(nd):
            out = m(inputs_embeds=dec_in[i][None, None], past_key_values=past, use_cache=True)
            past = out.past_key_values
            hs.append(out.last_hidden_state[0])
        save(f"lm_{tag}.npz", ids=ids, dec_in=dec_in, prefill_hidden=hs[0],
             decode_hidden=torch.cat(hs[1:], dim=0), wsum=synth.checksum(w))


def _tok_cfg(c):
    return dict(causal=True, channels=1, conv_bias=True, conv_norm="none", disable_last_norm=True,
                encoder_depths=c.depth_str, encoder_n_filters=c.n_filters, encoder_ratios=list(c.ratios),
                layer_scale_init_value=1e-6, layernorm="RMSNorm", layernorm_elementwise_affine=True, layernorm_eps=c.eps,
                mixer_layer="depthwise_conv", pad_mode="constant", weight_init_value=0.01, vae_dim=c.vae_dim,
                fix_std=0.5, std_dist_type="gaussian", decoder_n_filters=c.n_filters, decoder_ratios=list(c.ratios),
                decoder_depths=None)


class _Tok:
    speech_start_id, speech_end_id, speech_diffusion_id, eos_token_id = 301, 302, 303, 304
    bos_token_id, pad_token_id, pad_id = None, 305, 305


@torch.no_grad()
def gen_generate(custom=None):
    """custom: [(file name, batch, forced plans as lists of "D" / "E" / "S" / "X", seed, generate() keyword arguments)] -- record
    THOSE runs instead of the goldens (the fuzz tool); None: the goldens.
    Row G: the reference's OWN generate() loop (modeling_vibevoice_inference.py:326-710), tiny seeded weights, CPU
    fp32.  The token choice is forced through a LogitsProcessor (random weights would never emit <speech_diffusion>);
    every torch.randn / randn_like draw is recorded so the oracle can be fed the same noise."""
    from transformers import LogitsProcessor, LogitsProcessorList
    Ref = refshim.install_generate_shims()
    from vibevoice.modular.configuration_vibevoice import VibeVoiceConfig
    lc = synth.LMCfg()
    hc = synth.HeadCfg(hidden=lc.hidden, layers=2)
    cc, sc = synth.CodecCfg(), synth.CodecCfg(vae_dim=128)
    cfg = VibeVoiceConfig(
        acoustic_tokenizer_config=_tok_cfg(cc), semantic_tokenizer_config=dict(_tok_cfg(sc), fix_std=0, std_dist_type="none"),
        decoder_config=dict(model_type="qwen2", hidden_size=lc.hidden, intermediate_size=lc.inter, num_hidden_layers=lc.layers,
                            num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, vocab_size=lc.vocab,
                            rms_norm_eps=lc.eps, rope_theta=lc.theta, max_position_embeddings=lc.max_pos,
                            tie_word_embeddings=False, hidden_act="silu"),
        diffusion_head_config=dict(hidden_size=lc.hidden, head_layers=hc.layers, head_ffn_ratio=hc.ffn_ratio, rms_norm_eps=hc.eps,
                                   latent_size=64, speech_vae_dim=64, prediction_type="v_prediction", diffusion_type="ddpm",
                                   ddpm_num_steps=1000, ddpm_num_inference_steps=5, ddpm_beta_schedule="cosine", ddpm_batch_mul=4),
        acoustic_vae_dim=64, semantic_vae_dim=128,
        tie_word_embeddings=False)      # PretrainedConfig defaults to True; tie_weights() (:119-128) would alias lm_head to embed_tokens
    refshim.expose_text_config(cfg)
    m = Ref(cfg).eval()
    assert m.lm_head.weight.data_ptr() != m.model.language_model.embed_tokens.weight.data_ptr()
    sd = {}
    sd.update({"model.language_model." + k: v for k, v in synth.lm_weights(lc).items()})
    sd["lm_head.weight"] = synth.lm_head_weight(lc)
    sd.update({"model.prediction_head." + k: v for k, v in synth.head_weights(hc).items()})
    ac_w = {**synth.encoder_weights(cc, 2), **synth.decoder_weights(cc, 3)}
    sd.update({"model.acoustic_tokenizer." + k: v for k, v in ac_w.items()})
    sd.update({"model.semantic_tokenizer." + k: v for k, v in synth.encoder_weights(sc, 7).items()})
    sd.update({"model.acoustic_connector." + k: v for k, v in synth.connector_weights(64, lc.hidden, 4).items()})
    sd.update({"model.semantic_connector." + k: v for k, v in synth.connector_weights(128, lc.hidden, 8).items()})
    sd["model.speech_scaling_factor"] = torch.tensor(0.2)
    sd["model.speech_bias_factor"] = torch.tensor(-0.05)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("rotary" in k or "inv_freq" in k for k in missing), missing
    m.set_ddpm_inference_steps(5)
    T = _Tok
    D, E, S, X = T.speech_diffusion_id, T.speech_end_id, T.speech_start_id, T.eos_token_id

    class Force(LogitsProcessor):
        def __init__(self, plan):
            self.plan, self.step = plan, 0

        def __call__(self, input_ids, scores):
            out = torch.full_like(scores, -float("inf"))
            for b in range(scores.shape[0]):
                tok = self.plan[b][self.step] if self.step < len(self.plan[b]) else T.eos_token_id
                out[b, tok] = 0.0
            self.step += 1
            return out

    class RecStreamer:                      # what generate() tells an AudioStreamer (streamer.py:42-76), in order
        def __init__(self, batch):
            self.finished_flags = [False] * batch
            self.log = []

        def put(self, chunk, idx):
            self.log.append([0, int(chunk.shape[0])] + [int(i) for i in idx.tolist()])

        def end(self, idx=None):
            ids = list(range(len(self.finished_flags))) if idx is None else [int(i) for i in idx.tolist()]
            self.log.append([1, len(ids)] + ids)
            # NOTE: finished_flags deliberately left untouched -- the reference's own streamer sets them, which makes
            # generate() stop at the first finished sample (:443-447); here the whole batch is recorded.

    def run(name, B, plans, seed, max_new_tokens=None, do_sample=False, wav_len=3 * 3200, streamer=False, sde=False, gen_cfg=None,
            voices=None, dtype=None, **gen_kw):
        """voices: per row, the frame counts (1..3) of its voice samples -- several speakers in one prompt, as the processor builds a
        multi-speaker script (speech_tensors / speech_masks hold ALL samples of the batch, row after row; each sample's placeholder
        positions follow one another in its row, separated by a text token).  None: one sample per row (2, 3, 1, 2 frames)."""
        if dtype is not None:
            # the reference's GPU dtype (demo/inference_from_file.py:284-292 loads bf16) on the CPU: a copy of the model cast as
            # from_pretrained(torch_dtype=...) leaves it -- every parameter and buffer in `dtype`, the rotary inv_freq (a non-persistent
            # buffer the rotary module computes in fp32 whatever the default dtype) kept in fp32.  Also records every frame's latents.
            mm = Ref(cfg).eval()
            mm.load_state_dict(m.state_dict(), strict=False)
            mm.set_ddpm_inference_steps(5)
            mm = mm.to(dtype)
            ref_buf = dict(m.named_buffers())
            for nm, buf in mm.named_buffers():
                if "inv_freq" in nm:
                    buf.data = ref_buf[nm].detach().clone()
            lat_rec = []
            o_sst = mm.sample_speech_tokens

            def rec_sst(*a, **k):
                out = o_sst(*a, **k)
                lat_rec.append(out.detach().float().clone())
                return out
            mm.sample_speech_tokens = rec_sst
            arrs = _run(mm, None, B, plans, seed, max_new_tokens, do_sample, wav_len, streamer, sde, gen_cfg, voices, lat_rec, gen_kw)
            # ... and the fp32 model on the SAME draws (replayed in order): the distance between the two runs is the reference's own
            # rounding noise in `dtype` on this model -- free-running, as the reference runs
            lat32 = []
            o32 = m.sample_speech_tokens

            def rec32(*a, **k):
                out = o32(*a, **k)
                lat32.append(out.detach().float().clone())
                return out
            m.sample_speech_tokens = rec32
            try:
                replay = [arrs[f"draw_{i}"] for i in range(int(arrs["n_draws"]))]
                a32 = _run(m, None, B, plans, seed, max_new_tokens, do_sample, wav_len, streamer, sde, gen_cfg, voices, lat32, gen_kw, replay=replay)
            finally:
                m.sample_speech_tokens = o32
            assert torch.equal(a32["sequences"], arrs["sequences"])
            for k, v in a32.items():
                if k.startswith("latent_") or k.startswith("audio_"):
                    arrs["fp32_" + k] = v
            save(name, **arrs)
            return arrs
        return _run(m, name, B, plans, seed, max_new_tokens, do_sample, wav_len, streamer, sde, gen_cfg, voices, None, gen_kw)

    def _run(m, name, B, plans, seed, max_new_tokens, do_sample, wav_len, streamer, sde, gen_cfg, voices, lat_rec, gen_kw, replay=None):
        g = synth.Gen(seed)
        lens = [21, 17, 19, 14][:B]
        L0 = max(lens)
        ids = torch.full((B, L0), T.pad_token_id, dtype=torch.long)
        mask = torch.zeros((B, L0), dtype=torch.long)
        sim = torch.zeros((B, L0), dtype=torch.bool)
        n_fr = [2, 3, 1, 2]
        for b in range(B):
            n = lens[b]
            row = torch.from_numpy(g.rng.integers(0, 300, (n,)))
            row[-1] = T.speech_start_id
            ids[b, L0 - n:] = row
            mask[b, L0 - n:] = 1
            st0 = L0 - n + 3
            if voices is None:
                ids[b, st0:st0 + n_fr[b]] = T.speech_diffusion_id
                sim[b, st0:st0 + n_fr[b]] = True
            else:
                for f in voices[b]:
                    assert st0 + f < L0 - 1, "the row is too short for its voice samples"
                    ids[b, st0:st0 + f] = T.speech_diffusion_id
                    sim[b, st0:st0 + f] = True
                    st0 += f + 1
        if voices is None:
            speech = g.uniform((B, wav_len), -0.5, 0.5)
            smask = torch.zeros((B, 3), dtype=torch.bool)
            for b in range(B):
                smask[b, :n_fr[b]] = True
        else:
            fr = [f for v in voices for f in v]
            speech = g.uniform((len(fr), wav_len), -0.5, 0.5)
            smask = torch.zeros((len(fr), 3), dtype=torch.bool)
            for i, f in enumerate(fr):
                smask[i, :f] = True
        force = Force(plans) if plans is not None else None
        orig_glp = Ref._get_logits_processor

        def glp(self, *a, **k):
            lst = orig_glp(self, *a, **k)
            if force is not None:
                lst = LogitsProcessorList([force] + list(lst))
            return lst
        rec = RecStreamer(B) if streamer else None
        draws = []
        o_randn, o_like = torch.randn, torch.randn_like

        rp = iter(replay) if replay is not None else None

        def rec_randn(*a, **k):
            t = o_randn(*a, **k)
            if rp is not None:
                t = next(rp).reshape(t.shape).to(t.dtype)
            draws.append(t.detach().clone().reshape(-1))
            return t

        def rec_like(x, **k):
            t = o_like(x, **k)
            if rp is not None:
                t = next(rp).reshape(t.shape).to(t.dtype)
            draws.append(t.detach().clone().reshape(-1))
            return t
        Ref._get_logits_processor = glp
        torch.randn, torch.randn_like = rec_randn, rec_like
        base_sched = m.model.noise_scheduler
        if sde:     # demo/gradio_demo.py:142-146, verbatim
            m.model.noise_scheduler = m.model.noise_scheduler.from_config(
                m.model.noise_scheduler.config,
                algorithm_type='sde-dpmsolver++',
                beta_schedule='squaredcos_cap_v2'
            )
            m.set_ddpm_inference_steps(num_steps=5)
        try:
            torch.manual_seed(seed)
            out = m.generate(input_ids=ids, attention_mask=mask, tokenizer=T(), cfg_scale=1.3, max_new_tokens=max_new_tokens,
                             # top_k=0: HF's default top-50 warper runs BEFORE the reference's valid-token constraint; with random
                             # weights the 4 valid ids can all fall outside the top 50 (all -inf -> NaN probabilities)
                             generation_config=(gen_cfg if gen_cfg is not None else
                                                {"do_sample": True, "top_k": 0} if do_sample else {"do_sample": False}),
                             show_progress_bar=False, return_speech=True, audio_streamer=rec,
                             speech_tensors=speech, speech_masks=smask, speech_input_mask=sim, **gen_kw)
        finally:
            torch.randn, torch.randn_like = o_randn, o_like
            Ref._get_logits_processor = orig_glp
            m.model.noise_scheduler = base_sched
        arrs = dict(input_ids=ids, attention_mask=mask, speech_input_mask=sim, speech_tensors=speech, speech_masks=smask,
                    sequences=out.sequences, reach_max=out.reach_max_step_sample, n_draws=len(draws), seed=seed,
                    forced=np.array([p + [X] * (64 - len(p)) for p in plans]) if plans is not None else np.zeros((0,)),
                    forced_len=np.array([len(p) for p in plans]) if plans is not None else np.zeros((0,)))
        for i, d in enumerate(draws):
            arrs[f"draw_{i}"] = d.float()
        if lat_rec is not None:
            arrs["n_latents"] = len(lat_rec)
            for i, l in enumerate(lat_rec):
                arrs[f"latent_{i}"] = l
        if rec is not None:
            w = max(len(r) for r in rec.log)
            arrs["streamer_log"] = np.array([r + [-1] * (w - len(r)) for r in rec.log])
        for b in range(B):
            a = out.speech_outputs[b]
            arrs[f"audio_{b}"] = a.reshape(-1).float() if a is not None else torch.zeros(0)
        if name is not None:
            save(name, **arrs)
        return arrs

    if custom == "bf16":
        run("generate_forced_b1_bf16.npz", 1, [[D, D, D, D, E, S, D, D, D, X]], seed=11, dtype=torch.bfloat16)
        run("generate_forced_b2_bf16.npz", 2, [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]], seed=23, dtype=torch.bfloat16)
        return
    if custom is not None:
        sym = {"D": D, "E": E, "S": S, "X": X}
        for name, B, plans, seed, kw in custom:
            run(name, B, None if plans is None else [[sym[t] for t in p] for p in plans], seed=seed, **kw)
        return
    run("generate_forced_b1.npz", 1, [[D, D, D, D, E, S, D, D, D, X]], seed=11)
    run("generate_forced_b2.npz", 2, [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]], seed=23, streamer=True)
    run("generate_greedy_b1.npz", 1, None, seed=31, max_new_tokens=10)
    # multinomial token sampling from the CPU global RNG, interleaved with the noise draws: pins the RNG consumption order
    run("generate_sampled_b1.npz", 1, None, seed=47, max_new_tokens=14, do_sample=True)
    # the full-vocabulary logits processors in front of the valid-token constraint (HF's list, :310-319): repetition penalty,
    # temperature, top-k, top-p, min-p over all 320 ids of the toy vocabulary, then the constraint, then multinomial
    # (with random weights a step whose valid ids are ALL filtered makes the reference fail in torch.multinomial -- NaN
    # probabilities; the first seed of the list that runs through is used, and recorded in the file)
    def run_first_ok(name, seeds, *a, **k):
        for sd in seeds:
            try:
                run(name, *a, seed=sd, **k)
                return
            except RuntimeError as ex:
                if "probability tensor" not in str(ex):
                    raise
        raise RuntimeError(f"{name}: no seed in {list(seeds)} survives the filters")
    run_first_ok("generate_sampled_warped_b1.npz", range(59, 99), 1, None, max_new_tokens=14,
                 gen_cfg={"do_sample": True, "top_k": 300, "top_p": 0.995, "min_p": 0.0001, "temperature": 0.8, "repetition_penalty": 1.15})
    # the same processors in a batch of two (left-padded prompts: the pad id counts as seen for the repetition penalty)
    run_first_ok("generate_sampled_warped_b2.npz", range(161, 199), 2, None, max_new_tokens=12,
                 gen_cfg={"do_sample": True, "top_k": 310, "top_p": 0.998, "temperature": 1.3, "repetition_penalty": 1.05})
    # greedy decoding with a repetition penalty (a processor, not a warper: it also acts without sampling)
    run("generate_greedy_reppen_b1.npz", 1, None, seed=31, max_new_tokens=10, gen_cfg={"do_sample": False, "repetition_penalty": 4.0})
    # voice sample that is not a whole number of 3200-sample frames (2.5 frames; the prompt reserves ceil = 3 positions)
    run("generate_ragged_voice_b1.npz", 1, [[D, D, X]], seed=53, wav_len=8000)
    # length cap: the forced plan would go on, max_new_tokens stops it (reach_max_step_sample bookkeeping, :523-539)
    run("generate_cap_b1.npz", 1, [[D] * 50], seed=41, max_new_tokens=6)
    # the gradio demo's scheduler (stochastic sde-dpmsolver++): the solver's variance-noise draws join the recorded stream
    # (per frame: the initial randn(2n, 64), then one randn(2n, 64) per solver step inside scheduler.step())
    run("generate_sde_b1.npz", 1, [[D, D, D, E, S, D, D, X]], seed=67, sde=True)
    run("generate_sde_b2.npz", 2, [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]], seed=71, sde=True)
    # refresh_negative=False (:503-516, and the resets of :550-565 / the forward of :576-588 skipped): the negative branch consumes
    # every step's input and is never reset; in the batch of two the rows that do not diffuse while the other one does go through
    # the cache correction of :590-624
    run("generate_norefresh_b1.npz", 1, [[D, D, D, D, E, S, D, D, D, X]], seed=83, refresh_negative=False)
    run("generate_norefresh_b2.npz", 2, [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]], seed=89, refresh_negative=False)
    # max_length_times (:370, :421-422): the loop length follows the PADDED prompt width (int(0.4 * 21) = 8 steps), each row's own cap
    # its unpadded length (21 -> 8, 17 -> int(6.8) = 6): the shorter row is stopped by reach_max_step_sample while the other goes on
    run("generate_times_b2.npz", 2, [[D] * 50, [D] * 50], seed=101, max_length_times=0.4)
    # a row whose first frame comes LATER than the other row's: VibeVoiceTokenizerStreamingCache.get (modular_vibevoice_tokenizer.py:
    # 198-207) returns None for the whole call when one requested row has no entry yet, so the row that was already streaming loses its
    # conv history for that frame (both tokenizers) -- a cross-row coupling of the lock-step batch that processor-built prompts never
    # trigger (every row diffuses at step 0)
    run("generate_late_start_b2.npz", 2, [[D, D, D, X], [E, S, D, D, X]], seed=201)
    run("generate_late_start_b2r.npz", 2, [[S, D, D, X], [D, D, E, S, D, X]], seed=203)
    # the correction of a non-diffusing row (:594-624) when that row holds exactly ONE valid negative entry (a one-frame segment: D, then
    # <speech_end> while the other row diffuses): the mask shift is guarded by `start + 1 < seq_len - 1` (:603), the K/V shift by
    # `start + 1 < cache length - 1` (:613) -- the mask moves, the K/V does not, the entry appended at this step stays and the older
    # one is masked out
    run("generate_single_entry_b2.npz", 2, [[D, D, D, S, D, E, D, X], [D, E, D, D, D, D, D, D, E, X]], seed=207)
    # several voice samples in one prompt (a multi-speaker script: BASELINE configs[2] has two speakers, configs[3] four): row 0 carries
    # two samples (2 and 1 frames), row 1 one (3 frames); speech_tensors / speech_masks hold the three samples row after row
    run("generate_multivoice_b2.npz", 2, [[D, D, D, E, S, D, X], [D, D, E, X]], seed=602, voices=[[2, 1], [3]])
    # a voice sample that is not a whole number of frames AND whose partial last frame is used (row 1 takes all three frames of the
    # 2.5-frame batch tensor): SConv1d right-pads per strided conv layer (get_extra_padding_for_conv1d), so past the end of the signal
    # every strided conv reads zeros -- the partial frame's latent, and through it the whole prompt of that row, depends on it
    run("generate_ragged_voice_full_b2.npz", 2, [[D, D, D, X], [D, D, E, X]], seed=611, wav_len=8000)
    # the reference's own classes in bf16 (its GPU dtype) on the same model, plan and seed as generate_forced_b1 / _b2: what the oracle
    # run in bf16 is held to (tests/test_oracle_golden.py), so that "reference bf16 vs fp32" in bench.py's parity blocks is the
    # reference's rounding, not a restatement's
    run("generate_forced_b1_bf16.npz", 1, [[D, D, D, D, E, S, D, D, D, X]], seed=11, dtype=torch.bfloat16)
    run("generate_forced_b2_bf16.npz", 2, [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]], seed=23, dtype=torch.bfloat16)


@torch.no_grad()
def gen_generate_streaming(custom=None):
    """custom: [(file name, text tokens, max_new, seed, eos_bias or None)] -- record THOSE runs instead of the goldens (fuzzing).
    Row Z: the reference's Streaming-0.5B generate() (modeling_vibevoice_streaming_inference.py:412-751) on a tiny
    seeded model.  The four prefilled branches (what demo/voices/streaming_model/*.pt hold) are produced with the
    reference's own forward_lm / forward_tts_lm on a random prompt and stored, so the oracle starts from identical
    caches; every torch.randn draw is recorded."""
    RefS = refshim.install_streaming_shims()
    from vibevoice.modular.configuration_vibevoice_streaming import VibeVoiceStreamingConfig
    n_lm, n_tts = 1, 2
    lc = synth.LMCfg(hidden=128, layers=n_lm + n_tts, heads=2, kv_heads=1, inter=256, vocab=320)
    hc = synth.HeadCfg(hidden=lc.hidden, layers=2)
    cc = synth.CodecCfg()
    cfg = VibeVoiceStreamingConfig(
        acoustic_tokenizer_config=_tok_cfg(cc),
        decoder_config=dict(model_type="qwen2", hidden_size=lc.hidden, intermediate_size=lc.inter, num_hidden_layers=lc.layers,
                            num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, vocab_size=lc.vocab, rms_norm_eps=lc.eps,
                            rope_theta=lc.theta, max_position_embeddings=512, tie_word_embeddings=False, hidden_act="silu"),
        diffusion_head_config=dict(hidden_size=lc.hidden, head_layers=hc.layers, head_ffn_ratio=hc.ffn_ratio, rms_norm_eps=hc.eps,
                                   latent_size=64, speech_vae_dim=64, prediction_type="v_prediction", diffusion_type="ddpm",
                                   ddpm_num_steps=1000, ddpm_num_inference_steps=5, ddpm_beta_schedule="cosine", ddpm_batch_mul=4),
        tts_backbone_num_hidden_layers=n_tts, acoustic_vae_dim=64)
    refshim.expose_text_config(cfg)
    m = RefS(cfg).eval()
    # the same weights tests/test_gpu_streaming.py::build gives the oracle and the engine
    w = synth.lm_weights(lc)
    g = synth.Gen(900)
    tts_types = g.normal((2, lc.hidden), 0.5, mat=False)
    eos = {"fc1.weight": g.linear(lc.hidden, lc.hidden), "fc1.bias": g.vec(lc.hidden, 0.1),
           "fc2.weight": g.linear(1, lc.hidden, 0.3), "fc2.bias": g.vec(1, 0.1, -1.5)}
    sd = {"model.language_model.embed_tokens.weight": w["embed_tokens.weight"],
          "model.tts_language_model.embed_tokens.weight": w["embed_tokens.weight"],
          "model.tts_language_model.norm.weight": w["norm.weight"], "model.tts_input_types.weight": tts_types}
    for k, v in w.items():
        if k.startswith("layers."):
            li = int(k.split(".")[1])
            rest = k.split(".", 2)[2]
            if li < n_lm:
                sd[f"model.language_model.layers.{li}.{rest}"] = v
            else:
                sd[f"model.tts_language_model.layers.{li - n_lm}.{rest}"] = v
    sd.update({"tts_eos_classifier." + k: v for k, v in eos.items()})
    sd.update({"model.prediction_head." + k: v for k, v in synth.head_weights(hc).items()})
    sd.update({"model.acoustic_tokenizer." + k: v for k, v in synth.decoder_weights(cc, 3).items()})
    sd.update({"model.acoustic_connector." + k: v for k, v in synth.connector_weights(64, lc.hidden, 4).items()})
    sd["model.speech_scaling_factor"] = torch.tensor(0.2)
    sd["model.speech_bias_factor"] = torch.tensor(-0.05)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(("rotary" in k or "inv_freq" in k or "acoustic_tokenizer.encoder" in k) for k in missing), missing
    m.set_ddpm_inference_steps(5)

    class Tok:
        bos_token_id, eos_token_id, pad_token_id = None, 304, 305
        speech_start_id, speech_end_id, speech_diffusion_id = 301, 302, 303

        def convert_tokens_to_ids(self, t):
            return 305

    class RecStreamer:                      # what the streaming generate() tells an AudioStreamer, in order (flags left untouched)
        def __init__(self):
            self.finished_flags = [False]
            self.log = []

        def put(self, chunk, idx):
            self.log.append([0, int(chunk.shape[0]), int(chunk.shape[-1])] + [int(i) for i in idx.tolist()])

        def end(self, idx=None):
            ids = [0] if idx is None else [int(i) for i in idx.tolist()]
            self.log.append([1, len(ids), -1 if idx is None else 0] + ids)

    def run(name, n_text, max_new, seed, eos_bias=None):
        if eos_bias is not None:                       # make the binary EOS head fire (the seeded bias of -1.5 never does)
            m.tts_eos_classifier.fc2.bias.data.fill_(eos_bias)
        gg = synth.Gen(seed)
        prompt = torch.from_numpy(gg.rng.integers(0, 300, (23,)))[None]
        text = torch.from_numpy(gg.rng.integers(0, 300, (n_text,)))[None]
        ones = torch.ones_like(prompt)
        # prefilled branches with the reference's own forwards (text positions: type 1)
        lm_o = m.forward_lm(input_ids=prompt, attention_mask=ones, use_cache=True, return_dict=True)
        tts_o = m.forward_tts_lm(input_ids=prompt, attention_mask=ones, use_cache=True, return_dict=True,
                                 lm_last_hidden_state=lm_o.last_hidden_state, tts_text_masks=torch.ones_like(prompt))
        neg = torch.full((1, 1), 305, dtype=torch.long)
        nlm_o = m.forward_lm(input_ids=neg, attention_mask=torch.ones_like(neg), use_cache=True, return_dict=True)
        ntts_o = m.forward_tts_lm(input_ids=neg, attention_mask=torch.ones_like(neg), use_cache=True, return_dict=True,
                                  lm_last_hidden_state=nlm_o.last_hidden_state, tts_text_masks=torch.ones_like(neg))
        arrs = dict(prompt=prompt[0], text=text[0], max_new=max_new, eos_bias=float(m.tts_eos_classifier.fc2.bias.data[0]))
        for tag, o in (("lm", lm_o), ("tts", tts_o), ("neg_tts", ntts_o)):
            kc = [t for t in o.past_key_values.key_cache if t is not None]      # the cache object has a slot per decoder_config
            vc = [t for t in o.past_key_values.value_cache if t is not None]    # layer; each half of the split LM fills its own
            for li in range(len(kc)):
                arrs[f"{tag}_k{li}"] = kc[li][0].clone()
                arrs[f"{tag}_v{li}"] = vc[li][0].clone()
            arrs[f"{tag}_last"] = o.last_hidden_state[0, -1].clone()
            arrs[f"{tag}_layers"] = len(kc)
        draws = []
        o_randn = torch.randn
        rec = RecStreamer()

        def rec_randn(*a, **k):
            t = o_randn(*a, **k)
            draws.append(t.detach().clone().reshape(-1))
            return t
        torch.randn = rec_randn
        try:
            torch.manual_seed(seed)
            out = m.generate(input_ids=prompt, attention_mask=ones, tts_lm_input_ids=prompt.clone(), tts_lm_attention_mask=ones.clone(),
                             tts_text_ids=text, all_prefilled_outputs={"lm": lm_o, "tts_lm": tts_o, "neg_lm": nlm_o, "neg_tts_lm": ntts_o},
                             tokenizer=Tok(), cfg_scale=1.5, max_new_tokens=max_new, show_progress_bar=False, return_speech=True,
                             audio_streamer=rec)
        finally:
            torch.randn = o_randn
        arrs.update(sequences=out.sequences[0], streamer_log=np.array(rec.log))
        arrs.update(n_draws=len(draws), n_tokens=out.sequences.shape[1], reach_max=out.reach_max_step_sample,
                    audio=out.speech_outputs[0].reshape(-1) if out.speech_outputs[0] is not None else torch.zeros(0))
        for i, d in enumerate(draws):
            arrs[f"draw_{i}"] = d
        save(name, **arrs)

    if custom is not None:
        for name, n_text, max_new, seed, eos_bias in custom:
            run(name, n_text, max_new, seed=seed, eos_bias=eos_bias)
        return
    run("streaming_text12_cap40.npz", 12, 40, seed=5)
    run("streaming_text3_cap20.npz", 3, 20, seed=6)
    run("streaming_eos.npz", 12, 60, seed=7, eos_bias=0.35)
    # the length cap falls ON a text window (found by the fuzz tool, round 5): the reference concatenates the window's ids before it
    # checks the cap (:573-582), so `sequences` ends with those ids although the window is never fed to the model
    run("streaming_cap_on_text.npz", 23, 35, seed=191019, eos_bias=0.0)


def _no_init_tables(build):
    """{name: shape} of the model build() returns, instantiated in bf16 with every random initialisation skipped (only names and
    shapes are read; at real widths the initialisers alone take minutes of CPU)"""
    import torch.nn.init as init
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    saved = {n: getattr(init, n) for n in ("normal_", "uniform_", "trunc_normal_", "kaiming_uniform_", "kaiming_normal_", "xavier_uniform_",
                                           "xavier_normal_", "constant_", "zeros_", "ones_")}
    tsaved = {n: getattr(torch.Tensor, n) for n in ("normal_", "uniform_", "fill_", "zero_")}
    try:
        for n in saved:
            setattr(init, n, lambda t, *a, **k: t)
        for n in tsaved:
            setattr(torch.Tensor, n, lambda self, *a, **k: self)
        model = build()
        table = {k: list(v.shape) for k, v in model.state_dict().items()}
        del model
    finally:
        for n, f in saved.items():
            setattr(init, n, f)
        for n, f in tsaved.items():
            setattr(torch.Tensor, n, f)
        torch.set_default_dtype(old)
    return table


def gen_reference_contract():
    """reference_contract.json, what tests/test_reference_contract_cpu.py holds the loader to: the reference's shipped config files
    (vibevoice/configs/qwen2.5_1.5b_64k.json, qwen2.5_7b_32k.json) as they are, and the parameter table (name -> shape) of the
    reference's own model classes -- 1.5B / 7B from those files with the LM cut to two layers and a 1024-token vocabulary (per-layer
    names and shapes repeat), Streaming-0.5B at full depth from vibevoice_amd.configs (no config file ships for it)."""
    import copy
    import json
    from vibevoice_amd.configs import CONFIGS
    files = {"1.5b": "qwen2.5_1.5b_64k.json", "7b": "qwen2.5_7b_32k.json"}
    doc = {"config_files": {}, "param_tables": {}}
    Ref = refshim.install_generate_shims()
    from vibevoice.modular.configuration_vibevoice import VibeVoiceConfig
    for tag, fn in files.items():
        with open(os.path.join(refshim.REF_ROOT, "vibevoice", "configs", fn)) as f:
            raw = json.load(f)
        doc["config_files"][tag] = {"file": fn, "config": copy.deepcopy(raw)}
        raw["decoder_config"]["num_hidden_layers"] = 2
        raw["decoder_config"]["vocab_size"] = 1024

        def build(raw=raw):
            cfg = VibeVoiceConfig(**raw)
            refshim.expose_text_config(cfg)
            return Ref(cfg)
        doc["param_tables"][tag] = _no_init_tables(build)
    RefS = refshim.install_streaming_shims()
    from vibevoice.modular.configuration_vibevoice_streaming import VibeVoiceStreamingConfig

    def build_streaming():
        cfg = VibeVoiceStreamingConfig(**copy.deepcopy(CONFIGS["0.5b-streaming"]))
        refshim.expose_text_config(cfg)
        return RefS(cfg)
    doc["param_tables"]["0.5b-streaming"] = _no_init_tables(build_streaming)
    with open(os.path.join(OUT_DIR, "reference_contract.json"), "w") as f:
        json.dump(doc, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote reference_contract.json", {k: len(v) for k, v in doc["param_tables"].items()})


if __name__ == "__main__":
    if "--contract-only" in sys.argv:       # reference_contract.json alone
        gen_reference_contract()
        sys.exit(0)
    if "--streaming-cap-only" in sys.argv:
        gen_generate_streaming(custom=[("streaming_cap_on_text.npz", 23, 35, 191019, 0.0)])
        sys.exit(0)
    if "--bf16-only" in sys.argv:           # the two bf16 files alone (the full set takes ~4.5 minutes)
        gen_generate(custom="bf16")
        sys.exit(0)
    torch.manual_seed(0)
    gen_dpm_and_head()
    gen_codec()
    gen_connector()
    gen_lm()
    gen_generate()
    gen_generate_streaming()
    gen_reference_contract()
