#!/usr/bin/env python
"""First-audio latency at a host consumer with and without a prompt prefix (model.build_prompt_prefix, generate(prompt_prefix=...)).

Requests: the short-prompt shapes of the README tables with TWO voices -- 24 system tokens, 2 x (75-frame voice block), 220 text
tokens, N = 10 solver steps -- at VibeVoice-1.5B and at VibeVoice-7B widths, synthetic seeded weights (bench.py's generator).
One process, one build, one model per shape; the two arms alternate request by request (unprefixed, prefixed, unprefixed, ...)
after a warm-up of both, so drift on a shared host reaches both arms alike.  First audio = generate() entry -> the first
3200-sample chunk a consumer thread receives from an AudioStreamer (bench.py's first_audio_trials, the definition of the README
tables).  Reported per shape and arm: the median, the 10th / 90th percentile and every trial; `spread_ms` of an arm is p90 - p10
of its own trials.  The condition the prefix is held to: the prefixed median is not above the unprefixed median by more than the
unprefixed arm's spread.  The two arms must also SAY the same thing: the first chunks are compared (rel-L2).

    python tools/prefix_first_audio.py [--models 1.5b,7b] [--trials 15] [--warmup 3] [--out profiles/prompt_prefix_first_audio.json]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPE = dict(speakers=2, text_tokens=220, voice_frames=75, solver_steps=10)


def build_model(model_key, device, xsplit):
    from vibevoice_amd import synthetic
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd.engine import Engine, map_param_name
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference, engine_config_from_reference
    cfg = CONFIGS[model_key]
    inputs = synthetic.synthetic_inputs(cfg, n_speakers=SHAPE["speakers"], text_tokens=SHAPE["text_tokens"],
                                        voice_frames=SHAPE["voice_frames"], seed=100)
    L0 = inputs["input_ids"].shape[1]
    ecfg = engine_config_from_reference(cfg, n_slots=1, max_ctx=(L0 + 64 + 127) // 128 * 128, xsplit=xsplit, use_graph=True, max_rows=512)
    eng = Engine(ecfg, device)
    exp = eng.expected_weights()
    gen = torch.Generator(device=device)
    gen.manual_seed(0)
    for k, shape in synthetic.param_shapes(cfg).items():
        name = map_param_name(k)
        if name in exp:
            eng.upload(name, synthetic.random_tensor(k, shape, gen, device, torch.bfloat16))
    miss = eng.missing_weights()
    if miss:
        raise SystemExit(f"engine parameters not provided: {miss[:5]}")
    model = VibeVoiceForConditionalGenerationInference(cfg, eng, model_dtype=torch.bfloat16)
    model.set_speech_factors(0.2, -0.05)
    model.set_ddpm_inference_steps(SHAPE["solver_steps"])
    return model, cfg, inputs


def first_audio(model, call):
    """one request: (ms from generate() entry to the first chunk at a host consumer, that chunk)"""
    from vibevoice_amd.streamer import AudioStreamer
    st = AudioStreamer(batch_size=1)
    got = {}

    def consume():
        for chunk in st.get_stream(0):
            if "t" not in got:
                got["t"] = time.perf_counter()
                got["chunk"] = torch.as_tensor(chunk).detach().float().cpu().reshape(-1).clone()
    th = threading.Thread(target=consume, daemon=True)
    th.start()
    model.engine.sync()
    torch.cuda.current_stream(model.device).synchronize()
    t0 = time.perf_counter()
    call(st)
    th.join(timeout=60)
    st.close()
    if "t" not in got:
        raise RuntimeError("no audio chunk reached the consumer")
    return (got["t"] - t0) * 1e3, got["chunk"]


def summarise(ms):
    s = sorted(ms)
    p = lambda q: s[min(len(s) - 1, int(q * len(s)))]
    return {"median_ms": round(statistics.median(s), 3), "p10_ms": round(p(0.1), 3), "p90_ms": round(p(0.9), 3),
            "spread_ms": round(p(0.9) - p(0.1), 3), "trials_ms": [round(x, 3) for x in ms]}


def measure(model_key, device, trials, warmup, xsplit, frames=3):
    from vibevoice_amd import synthetic
    model, cfg, inputs = build_model(model_key, device, xsplit)
    try:
        T = synthetic.TOKENS
        import types
        tok = types.SimpleNamespace(speech_start_id=T.speech_start_id, speech_end_id=T.speech_end_id, speech_diffusion_id=T.speech_diffusion_id,
                                    eos_token_id=T.eos_token_id, bos_token_id=None)
        L = cfg["acoustic_vae_dim"]
        n_spk, vf = inputs["speech_masks"].shape
        g = torch.Generator().manual_seed(7)
        pre = (torch.randn(n_spk, generator=g), torch.randn(n_spk, vf, L, generator=g))     # one draw for both arms: same audio
        noise = torch.randn(frames + 1, 2, L, generator=g).to(device)
        forced = [[T.speech_diffusion_id] * frames + [T.eos_token_id]]
        model.warmup()
        prefix = model.build_prompt_prefix(**inputs, _prefill_noise=pre)
        common = dict(tokenizer=tok, cfg_scale=1.3, generation_config={"do_sample": False}, max_new_tokens=frames + 1, show_progress_bar=False,
                      _forced_tokens=forced, _noise_fn=lambda step, n2: noise[step][:n2])
        arms = {
            "unprefixed": lambda st: model.generate(**inputs, audio_streamer=st, _prefill_noise=pre, **common),
            "prefixed": lambda st: model.generate(input_ids=inputs["input_ids"], attention_mask=inputs["attention_mask"],
                                                  speech_input_mask=inputs["speech_input_mask"], audio_streamer=st, prompt_prefix=prefix, **common),
        }
        ms = {k: [] for k in arms}
        chunks = {}
        stats = {}
        for i in range(warmup + trials):
            for name, call in arms.items():               # alternate the arms
                t, chunk = first_audio(model, call)
                chunks[name] = chunk
                stats[name] = {k: model.last_stats.get(k) for k in ("prefix_rows_reused", "prompt_rows_computed")}
                if i >= warmup:
                    ms[name].append(t)
        res = {name: dict(summarise(v), **stats[name]) for name, v in ms.items()}
        a, b = chunks["prefixed"], chunks["unprefixed"]
        res["first_chunk_rel_l2_prefixed_vs_unprefixed"] = float((a - b).norm() / (b.norm() + 1e-30))
        res["prompt_tokens"] = int(inputs["input_ids"].shape[1])
        res["prefix_positions"] = prefix.n_pos
        res["gain_ms"] = round(res["unprefixed"]["median_ms"] - res["prefixed"]["median_ms"], 3)
        res["condition_prefixed_not_slower_beyond_spread"] = bool(
            res["prefixed"]["median_ms"] <= res["unprefixed"]["median_ms"] + res["unprefixed"]["spread_ms"])
        return res
    finally:
        model.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="1.5b,7b")
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--xsplit", type=int, default=int(os.environ.get("VVHIP_XSPLIT", "1")))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_prefix_first_audio.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    device = torch.device("cuda", 0)
    out = {"tool": "tools/prefix_first_audio.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "request": dict(SHAPE, frames_generated=3), "trials": args.trials, "warmup": args.warmup, "xsplit": args.xsplit,
           "first_audio_definition": "generate() entry -> first 3200-sample chunk delivered to an AudioStreamer consumer thread on the host",
           "spread_definition": "p90 - p10 of an arm's own trials; arms alternate request by request in one process", "shapes": {}}
    for key in [m for m in args.models.split(",") if m]:
        out["shapes"][key] = measure(key, device, args.trials, args.warmup, args.xsplit)
        print(json.dumps({key: {k: v for k, v in out["shapes"][key].items() if not isinstance(v, dict)},
                          "unprefixed_median_ms": out["shapes"][key]["unprefixed"]["median_ms"],
                          "prefixed_median_ms": out["shapes"][key]["prefixed"]["median_ms"],
                          "unprefixed_spread_ms": out["shapes"][key]["unprefixed"]["spread_ms"]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                    # after every shape: a later shape's trouble does not lose this one
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
