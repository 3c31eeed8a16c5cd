#!/usr/bin/env python
"""The noise stage of one frame with today's torch draws (no seed anywhere) and with vv_noise_rows (seeded requests): A/B on one
engine in one process.

Stage = what the host loop runs per sampler call to put the solver's start noise into the model's [n, latent] buffer and, under
sde-dpmsolver++, the N step-noise rows into its [N, n, latent] buffer:
  torch       torch.randn(2n, latent) on the CPU generator -> pinned ring -> async H2D (modeling.py::_stage_noise); under the
              stochastic solver N device randn(2n, latent) launches and N device copies on top (_sde_draws)
  noise_rows  one vv_noise_rows launch (_seeded_noise); under the stochastic solver a second one for streams 1 .. N
Shapes: the 7B configuration (latent 64; the stage touches no weight, so none is uploaded and the language model is cut to one
layer), n = 1 and n = 8 rows, the deterministic solver and sde-dpmsolver++ with N = 20 steps.

The arms alternate iteration by iteration after a warm-up of both; every iteration is bracketed by a pair of device events on the
engine's stream, and the host time the loop spends enqueueing the stage (until the call returns, before any wait) is taken with
perf_counter.  Reported per arm: median and p90 of both.  No threshold: the file records what was measured.

    python tools/seeded_noise_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/seeded_noise_ab.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

N_SDE = 20


def build_model(device, n_slots):
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd.engine import Engine
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference, engine_config_from_reference
    cfg = copy.deepcopy(CONFIGS["7b"])
    cfg["decoder_config"]["num_hidden_layers"] = 1
    ecfg = engine_config_from_reference(cfg, n_slots=n_slots, max_ctx=256, use_graph=False, max_rows=16)
    eng = Engine(ecfg, device)
    model = VibeVoiceForConditionalGenerationInference(cfg, eng, model_dtype=torch.bfloat16)
    model.set_ddpm_inference_steps(N_SDE)
    return model


def summarise(us):
    s = sorted(us)
    return {"median_us": round(statistics.median(s), 2), "p90_us": round(s[min(len(s) - 1, int(0.9 * len(s)))], 2), "iterations": len(s)}


def measure(model, n, sde, iters, warmup):
    from vibevoice_amd.modeling import _Session
    e = model.engine
    L = e.cfg.latent_dim
    utts = [types.SimpleNamespace(seed=0x9e3779b97f4a7c15 + i, n_lat=0) for i in range(n)]
    S_torch = _Session(seeds=None, sde_noise_fn=None, step=0, dev_gen=None, cpu_gen=None)
    S_seed = _Session(seeds=[u.seed for u in utts], sde_noise_fn=None, step=0)

    def arm_torch():
        model._stage_noise(torch.randn(2 * n, L), n)
        if sde:
            model._sde_draws(S_torch, n)

    def arm_rows():
        model._seeded_noise(utts)
        if sde:
            model._sde_draws(S_seed, n, utts)
    arms = {"torch": arm_torch, "noise_rows": arm_rows}
    dev_us = {k: [] for k in arms}
    host_us = {k: [] for k in arms}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(e.stream):
        for it in range(warmup + iters):
            for u in utts:
                u.n_lat = it
            for name, fn in arms.items():
                ev0.record(e.stream)
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                ev1.record(e.stream)
                ev1.synchronize()
                if it >= warmup:
                    dev_us[name].append(ev0.elapsed_time(ev1) * 1e3)
                    host_us[name].append((t1 - t0) * 1e6)
        # the last noise_rows iteration against the host definition
        from vibevoice_amd import noise
        arm_rows()
        got = model._noise[:n].cpu()
        ref = torch.stack([noise.normals(u.seed, u.n_lat, 1, 0, 1, 0, L)[0, 0] for u in utts])
    e.sync()
    return {"device_events": {k: summarise(v) for k, v in dev_us.items()}, "host_enqueue": {k: summarise(v) for k, v in host_us.items()},
            "max_abs_err_vs_host_definition": float((got.double() - ref.double()).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_noise_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/seeded_noise_ab.py measures on the GPU; none found")
    device = torch.device("cuda", 0)
    rows = [int(r) for r in args.rows.split(",") if r]
    model = build_model(device, max(rows))
    out = {"tool": "tools/seeded_noise_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "latent_dim": model.engine.cfg.latent_dim, "sde_steps": N_SDE,
           "stage": "start noise -> [n, latent] device buffer (+ N step-noise rows -> [N, n, latent] under sde-dpmsolver++)",
           "timing": "one device-event pair per iteration on the engine stream and perf_counter around the enqueueing calls; "
                     "arms alternate iteration by iteration in one process",
           "warmup": args.warmup, "cases": {}}
    try:
        for n in rows:
            for sde in (False, True):
                key = f"n{n}_{'sde-dpmsolver++' if sde else 'dpmsolver++'}"
                out["cases"][key] = measure(model, n, sde, args.iters, args.warmup)
                print(json.dumps({"case": key, **out["cases"][key]}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    finally:
        model.engine.close()


if __name__ == "__main__":
    main()
