#!/usr/bin/env python
"""Switching the merged LoRA adapter of the 7B language model: today's host path against model.set_adapter(), in one process.

Shapes: the 7B language model, 28 layers x seven matrices (q, k, v, o, gate, up, down; 6.5 G elements), synthetic seeded weights,
adapters of rank 8 and rank 64 on every one of the 196 matrices (the diffusion head is left out of both arms).

Arm "host" -- what load_lora_assets does per target: lora.merge_lora on the CPU (W' = W + scale * B @ A, fp32-delta mode), then
Engine.upload of the merged tensor (staging copy, re-pack, synchronize).  Measured with the wall clock for ONE layer's seven
matrices and SCALED by 28 (the file says so); the base tensors are held in host memory, so the checkpoint read load_lora_assets
does per target is not in the figure.
Arm "device" -- model.set_adapter(name) over the whole model, switching between two resident adapters x and y of the same rank:
196 merge launches from the base snapshots.  Device events on the engine stream around the call, plus the wall clock of the call.
Also timed: the first switch (it takes the base snapshots) and set_adapter(None) (196 copies back).

The arms alternate repetition by repetition; medians.  An upload of the host arm lands on parameters that hold a base snapshot
from the device arm and refreshes it (one device copy more in the host arm, under a thousandth of its time).

    python tools/adapter_switch_ab.py [--reps 5] [--ranks 8,64] [--out profiles/adapter_switch.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

MATS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
HBM_READ_CEILING_TBS = 6.3


def build_model(device, xsplit=1):
    """the 7B model with synthetic weights; returns (model, cfg, {engine name: shape} of the LM targets, host copies of layer 0's)"""
    from vibevoice_amd import synthetic
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd.engine import Engine, map_param_name
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference, engine_config_from_reference
    cfg = copy.deepcopy(CONFIGS["7b"])
    ecfg = engine_config_from_reference(cfg, n_slots=1, max_ctx=256, use_graph=False, max_rows=16, xsplit=xsplit)
    eng = Engine(ecfg, device)
    exp = eng.expected_weights()
    gen = torch.Generator(device=device)
    gen.manual_seed(0)
    shapes, host0 = {}, {}
    for k, shape in synthetic.param_shapes(cfg).items():
        name = map_param_name(k)
        if name not in exp:
            continue
        t = synthetic.random_tensor(k, shape, gen, device, torch.bfloat16)
        eng.upload(name, t)
        if name.startswith("lm.layers.") and name.endswith(".weight") and any(m in name for m in MATS):
            shapes[name] = tuple(shape)
            if name.startswith("lm.layers.0."):
                host0[name] = t.cpu()
    miss = eng.missing_weights()
    if miss:
        raise SystemExit(f"engine parameters not provided: {miss[:5]}")
    return VibeVoiceForConditionalGenerationInference(cfg, eng, model_dtype=torch.bfloat16), cfg, shapes, host0


def make_adapter(shapes, r, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return {name: (torch.randn(r, k, generator=g, device=device) * 0.02, torch.randn(n, r, generator=g, device=device) * 0.02, 32.0 / r)
            for name, (n, k) in shapes.items()}


def med(v):
    return round(statistics.median(v), 3)


def measure(model, shapes, host0, r, reps):
    from vibevoice_amd import lora
    e = model.engine
    x, y = make_adapter(shapes, r, 1, e.device), make_adapter(shapes, r, 2, e.device)
    model._register_adapter("x", x, "float32")
    model._register_adapter("y", y, "float32")
    host_pairs = {name: (x[name][0].cpu(), x[name][1].cpu(), x[name][2]) for name in host0}
    torch.cuda.current_stream(e.device).synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def switch(name):
        ev0.record(e.stream)
        t0 = time.perf_counter()
        model.set_adapter(name)                  # ends with a sync of the engine stream
        wall = (time.perf_counter() - t0) * 1e3
        ev1.record(e.stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1), wall
    snap0 = e.stat(7)
    first = switch("x")
    host_ms, dev_ms, wall_ms = [], [], []
    cur = "x"
    for _ in range(reps):
        t0 = time.perf_counter()
        for name, w in host0.items():
            a, b, sc = host_pairs[name]
            e.upload(name, lora.merge_lora(w, a, b, sc))
        host_ms.append((time.perf_counter() - t0) * 1e3)
        cur = "y" if cur == "x" else "x"
        d, wl = switch(cur)
        dev_ms.append(d)
        wall_ms.append(wl)
    reset = switch(None)
    elems = sum(int(e.lib.vv_packed_bytes(n, k)) // 2 for n, k in shapes.values())
    factor_bytes = sum((n + k) * r * 4 for n, k in shapes.values())
    moved = elems * 4 + factor_bytes              # snapshot read + active write, 2 bytes each, + the fp32 factors once
    res = {
        "rank": r, "matrices": len(shapes), "packed_elements": elems,
        "host": {"one_layer_ms_median": med(host_ms), "one_layer_ms": [round(v, 1) for v in host_ms],
                 "whole_model_ms_scaled_by_28": round(statistics.median(host_ms) * 28, 1),
                 "note": "merge_lora on the CPU + Engine.upload for layer 0's seven matrices, wall clock, SCALED by 28 layers; base tensors in host memory"},
        "device": {"set_adapter_device_ms_median": med(dev_ms), "set_adapter_wall_ms_median": med(wall_ms),
                   "device_ms": [round(v, 3) for v in dev_ms], "wall_ms": [round(v, 3) for v in wall_ms],
                   "first_switch_device_ms": round(first[0], 3), "first_switch_wall_ms": round(first[1], 3),
                   "set_adapter_none_device_ms": round(reset[0], 3), "set_adapter_none_wall_ms": round(reset[1], 3)},
        "base_snapshot_bytes": e.stat(7), "base_snapshot_bytes_before": snap0,
        "bytes_moved_per_switch": moved,
        # bf16 mode: every merge and reset also re-packs the written matrix's W13 twin on the same stream (read it, write 13/16 of it)
        "lm_matrices_with_a_w13_twin": e.stat(10),
        "twin_bytes_written_per_switch": (elems * 2 * 13 // 16) if e.stat(10) else 0,
        "tb_per_s": round(moved / (statistics.median(dev_ms) * 1e-3) / 1e12, 3),
        "hbm_read_ceiling_tb_per_s": HBM_READ_CEILING_TBS,
    }
    model.unload_adapter("x")
    model.unload_adapter("y")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", default="8,64")
    ap.add_argument("--xsplit", type=int, default=1, help="engine mode: 1 = bf16 activations (the bench default; the LM has W13 twins), 2 / 3 = the exact modes (none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapter_switch.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/adapter_switch_ab.py measures on the GPU; none found")
    device = torch.device("cuda", 0)
    model, cfg, shapes, host0 = build_model(device, args.xsplit)
    out = {"tool": "tools/adapter_switch_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "model": "7B language model, 28 layers x (q, k, v, o, gate, up, down), synthetic weights",
           "timing": "arms alternate repetition by repetition in one process; medians.  host: wall clock of one layer, scaled by 28; "
                     "device: device events on the engine stream around set_adapter() + the wall clock of the call",
           "repetitions": args.reps, "xsplit": args.xsplit, "ranks": {}}
    try:
        for r in [int(v) for v in args.ranks.split(",") if v]:
            out["ranks"][str(r)] = measure(model, shapes, host0, r, args.reps)
            print(json.dumps(out["ranks"][str(r)]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        model.engine.close()


if __name__ == "__main__":
    main()
