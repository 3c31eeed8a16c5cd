#!/usr/bin/env python
"""What the general solver path costs per frame, and what a shorter higher-order schedule saves: A/B of the sampler at the 7B head.

Arms, one engine context each over ONE weight copy (Engine.fork; a schedule table and its captured graphs are context state, so arms
that alternated on one context would re-install the table and drop the graphs every iteration):
  shipped_N20             vv_diffusion_sample on the shipped table (dpmsolver++, order 2, midpoint, linspace, final sigma 0), 20 steps
  general_same_N20        vv_diffusion_sample_general on make_general_table of the SAME settings, 20 steps: the price of the
                          general path (plain final layer + csrc/solver.hip's launch in place of the seam / the fused epilogues)
  general_order3_N10      vv_diffusion_sample_general at solver_order = 3, 10 steps
  general_same_N20_2launch   general_same_N20 in a context created under VVHIP_SOLVER_FUSE=0: update kernel + the existing
                          in-projection GEMM instead of the fused in-projection
The arms alternate iteration by iteration after a warm-up of all (the second call of a context captures its graph, later ones
replay it); every call is bracketed by a pair of device events on its context's stream.  Reported per arm: median and p90 in us,
the fused step ends / seam launches of the captured body, and vv_stat(0) (launches_per_call: 0 once a call is a graph replay).  Shapes: the 7B configuration's head (H = 3584, 4 layers, latent 64), bf16 mode, n = 1 and n = 8
utterances; the language model is cut to one layer; seeded random weights (vibevoice_amd/synthetic.py).  No threshold: the file
records what was measured.

    python tools/general_solver_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/general_solver_ab.json]
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG_SCALE = 1.3


def build_engine(device, n_slots):
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd import synthetic
    from vibevoice_amd.engine import Engine, map_param_name
    from vibevoice_amd.modeling import engine_config_from_reference
    cfg = copy.deepcopy(CONFIGS["7b"])
    cfg["decoder_config"]["num_hidden_layers"] = 1
    eng = Engine(engine_config_from_reference(cfg, n_slots=n_slots, max_ctx=256, use_graph=True, max_rows=16, xsplit=1), device)
    exp = eng.expected_weights()
    for k, v in synthetic.random_state_dict(cfg, device, seed=0):         # seeded random weights, one tensor at a time
        name = map_param_name(k)
        if name is not None and name in exp:
            eng.upload(name, v)
    return eng


def install_general_raw(eng, config, n_steps):
    """a general table through the C ABI: Engine.set_num_steps routes a shipped configuration to the shipped table"""
    from vibevoice_amd import schedule
    tv, coef = schedule.make_general_table(config, n_steps, True)
    fp = C.POINTER(C.c_float)
    eng._chk(eng.lib.vv_set_schedule_general(eng._ctx, len(tv), tv.ctypes.data_as(fp), np.ascontiguousarray(coef).ctypes.data_as(fp), 0, eng._s),
             "vv_set_schedule_general")
    eng._n_steps = None
    eng.general_solver = True


def summarise(us):
    s = sorted(us)
    return {"median_us": round(statistics.median(s), 2), "p90_us": round(s[min(len(s) - 1, int(0.9 * len(s)))], 2), "iterations": len(s)}


def measure(arms, n, iters, warmup):
    H, L = arms[0][1].cfg.lm_hidden, arms[0][1].cfg.latent_dim
    g = torch.Generator().manual_seed(5)
    cond_h, noise_h = torch.randn(2 * n, H, generator=g), torch.randn(n, L, generator=g)
    bufs = {}
    for name, e in arms:
        bufs[name] = (cond_h.to(e.device), noise_h.to(e.device), e.new(n, L))
    torch.cuda.synchronize()
    us = {name: [] for name, _ in arms}
    launches = {}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(warmup + iters):
        for name, e in arms:
            cd, nz, out = bufs[name]
            with torch.cuda.stream(e.stream):
                ev0.record(e.stream)
                e.diffusion_sample(n, cd, nz, CFG_SCALE, out)
                ev1.record(e.stream)
            ev1.synchronize()
            if it >= warmup:
                us[name].append(ev0.elapsed_time(ev1) * 1e3)
            launches[name] = e.stat(0)
    res = {name: dict(summarise(v), launches_per_call=launches[name], fused_step_ends=e.stat(8), seam_launches=e.stat(6),
                      non_kernel_graph_nodes=e.stat(5)) for (name, e), v in zip(arms, us.values())}
    outs = {name: bufs[name][2].cpu() for name, _ in arms}
    res["general_same_N20"]["rel_l2_vs_shipped_N20"] = float((outs["general_same_N20"] - outs["shipped_N20"]).norm()
                                                             / (outs["shipped_N20"].norm() + 1e-30))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_solver_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/general_solver_ab.py measures on the GPU; none found")
    device = torch.device("cuda", 0)
    rows = [int(r) for r in args.rows.split(",") if r]
    base = build_engine(device, max(rows))
    engines = [base]
    try:
        base.set_num_steps(20, t_cast_bf16=True)
        same = base.fork()
        engines.append(same)
        install_general_raw(same, {}, 20)
        o3 = base.fork()
        engines.append(o3)
        o3.set_num_steps(10, t_cast_bf16=True, solver={"solver_order": 3})
        os.environ["VVHIP_SOLVER_FUSE"] = "0"
        try:
            two = base.fork()
        finally:
            del os.environ["VVHIP_SOLVER_FUSE"]
        engines.append(two)
        install_general_raw(two, {}, 20)
        arms = [("shipped_N20", base), ("general_same_N20", same), ("general_order3_N10", o3), ("general_same_N20_2launch", two)]
        out = {"tool": "tools/general_solver_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
               "head": {"hidden": base.cfg.lm_hidden, "layers": base.cfg.head_layers, "latent_dim": base.cfg.latent_dim, "mode": "bf16 (xsplit 1)"},
               "timing": "one device-event pair per sampler call on the context's stream, graph replay; arms alternate iteration by "
                         "iteration in one process, one context per arm over one weight copy",
               "weights": "seeded random (vibevoice_amd/synthetic.py), language model cut to one layer", "warmup": args.warmup, "cases": {}}
        for n in rows:
            out["cases"][f"n{n}"] = measure(arms, n, args.iters, args.warmup)
            print(json.dumps({"case": f"n{n}", **out["cases"][f"n{n}"]}), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        for e in reversed(engines):
            e.close()


if __name__ == "__main__":
    main()
