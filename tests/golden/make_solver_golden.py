"""Generate tests/golden/solver_family.npz and tests/golden/solver_refused.json by running the REFERENCE's own scheduler,
vibevoice.schedule.dpm_solver.DPMSolverMultistepScheduler, loaded through oracle/refshim.py.

Run only where the reference tree exists (see oracle/refshim.py):
    python tests/golden/make_solver_golden.py

solver_family.npz: for every configuration of GRID and every N of STEP_COUNTS one run of set_timesteps(N) + step() over fixed
fp32 inputs (sample [2, 8], one model output and one variance-noise tensor per step index; the update is elementwise, so small
rows exercise everything).  A run is the reference's own trajectory: every step starts from the reference's previous state.
    configs      JSON list of the override dicts, in run order (a run = (config index, N))
    run_cfg / run_n / run_off      per run: config index, N asked for, offset of its first step in the step-major arrays
    run_len      steps the reference actually made (len(timesteps))
    timesteps [S] int64, sigmas_cur / sigmas_next [S] fp32 (sigmas[i], sigmas[i + 1]), prev_sample [S, 2, 8] fp32
    sample0 [2, 8], model_out [21, 2, 8], noise [21, 2, 8]      the inputs (step i of any run reads model_out[i], noise[i])
solver_refused.json: the configurations that stay refused, each with the exception class the reference raises on this model's
[2n, 64] latents, or the reason "deprecated" / "training-time".
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

STEP_COUNTS = (1, 2, 3, 5, 6, 14, 15, 20)
BASE = dict(num_train_timesteps=1000, beta_schedule="cosine", prediction_type="v_prediction")


def grid():
    """120 combinations of the sampling-time settings, then the edge cases: euler_at_final, (leading, steps_offset = 1), a
    lambda_min_clipped cut.  sde-dpmsolver++ has no third order (the reference fails on it: solver_refused.json)."""
    out = []
    pairs = [("dpmsolver++", 1), ("dpmsolver++", 2), ("dpmsolver++", 3), ("sde-dpmsolver++", 1), ("sde-dpmsolver++", 2)]
    for (algo, order), st, lof, fs, sp in itertools.product(pairs, ("midpoint", "heun"), (True, False), ("zero", "sigma_min"),
                                                            ("linspace", "leading", "trailing")):
        out.append(dict(algorithm_type=algo, solver_order=order, solver_type=st, lower_order_final=lof, final_sigmas_type=fs,
                        timestep_spacing=sp))
    for (algo, order), fs, lof in itertools.product(pairs, ("zero", "sigma_min"), (True, False)):
        out.append(dict(algorithm_type=algo, solver_order=order, euler_at_final=True, final_sigmas_type=fs, lower_order_final=lof))
    out.append(dict(solver_order=3, timestep_spacing="leading", steps_offset=1))
    out.append(dict(algorithm_type="sde-dpmsolver++", timestep_spacing="leading", steps_offset=1))
    out.append(dict(solver_order=3, lambda_min_clipped=-5.1))
    out.append(dict(solver_order=2, solver_type="heun", lambda_min_clipped=-5.1, timestep_spacing="trailing", final_sigmas_type="sigma_min"))
    return out


REFUSED = [
    # (overrides, key the refusal names, why): "reference" entries are run below and record the exception class
    (dict(use_karras_sigmas=True), "use_karras_sigmas", "reference"),
    (dict(thresholding=True), "thresholding", "reference"),
    (dict(algorithm_type="sde-dpmsolver++", solver_order=3), "solver_order", "reference"),
    (dict(use_lu_lambdas=True), "use_lu_lambdas", "reference"),
    (dict(algorithm_type="dpmsolver"), "algorithm_type", "deprecated"),
    (dict(algorithm_type="sde-dpmsolver"), "algorithm_type", "deprecated"),
    (dict(prediction_type="epsilon"), "prediction_type", "training-time"),
    (dict(prediction_type="sample"), "prediction_type", "training-time"),
    (dict(beta_schedule="linear"), "beta_schedule", "training-time"),
    (dict(beta_schedule="scaled_linear"), "beta_schedule", "training-time"),
    (dict(trained_betas=[0.0001, 0.02]), "trained_betas", "training-time"),
    (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr", "training-time"),
    (dict(variance_type="learned"), "variance_type", "training-time"),
    (dict(num_train_timesteps=500), "num_train_timesteps", "training-time"),
]


def reference_failure(cls, over):
    """the exception class the reference raises under `over` on [2n, 64] latents, at N = 6 and N = 20"""
    seen = {}
    for n in (6, 20):
        g = torch.Generator().manual_seed(7)
        try:
            s = cls(**dict(BASE, **over))
            s.set_timesteps(n)
            x = torch.randn(4, 64, generator=g)
            for t in s.timesteps:
                x = s.step(torch.randn(4, 64, generator=g), t, x, variance_noise=torch.randn(4, 64, generator=g)).prev_sample
            seen[str(n)] = None
        except Exception as e:      # noqa: BLE001 -- the class is the datum
            seen[str(n)] = type(e).__name__
    return seen


@torch.no_grad()
def main():
    from oracle import refshim
    if not os.path.isdir(refshim.REF_ROOT):
        raise SystemExit("tests/golden/make_solver_golden.py runs the reference's scheduler: no reference tree at " + refshim.REF_ROOT)
    refshim.install()
    from vibevoice.schedule.dpm_solver import DPMSolverMultistepScheduler as Sched

    g = torch.Generator().manual_seed(20260)
    sample0 = torch.randn(2, 8, generator=g)
    model_out = torch.randn(21, 2, 8, generator=g)
    noise = torch.randn(21, 2, 8, generator=g)
    cfgs = grid()
    run_cfg, run_n, run_off, run_len, ts_all, s0_all, s1_all, prev_all = [], [], [], [], [], [], [], []
    off = 0
    for ci, over in enumerate(cfgs):
        for n in STEP_COUNTS:
            s = Sched(**dict(BASE, **over))
            s.set_timesteps(n)
            assert len(set(s.timesteps.tolist())) == len(s.timesteps), (over, n, "duplicate timesteps")
            x = sample0.clone()
            run_cfg.append(ci); run_n.append(n); run_off.append(off); run_len.append(len(s.timesteps))
            for i, t in enumerate(s.timesteps):
                x = s.step(model_out[i], t, x, variance_noise=noise[i]).prev_sample
                ts_all.append(int(t)); s0_all.append(float(s.sigmas[i])); s1_all.append(float(s.sigmas[i + 1]))
                prev_all.append(x.clone())
                off += 1
    out = dict(configs=np.array(json.dumps(cfgs)), run_cfg=np.array(run_cfg, np.int32), run_n=np.array(run_n, np.int32),
               run_off=np.array(run_off, np.int32), run_len=np.array(run_len, np.int32), timesteps=np.array(ts_all, np.int64),
               sigmas_cur=np.array(s0_all, np.float32), sigmas_next=np.array(s1_all, np.float32),
               prev_sample=torch.stack(prev_all).numpy(), sample0=sample0.numpy(), model_out=model_out.numpy(), noise=noise.numpy())
    path = os.path.join(HERE, "solver_family.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cfgs), "configurations,", len(run_n), "runs,", off, "steps")
    assert os.path.getsize(path) < 1000 * 1000

    refused = []
    for over, key, why in REFUSED:
        rec = dict(overrides=over, key=key, reason=why)
        if why == "reference":
            rec["reference_raises"] = reference_failure(Sched, over)
            assert any(rec["reference_raises"].values()), (over, "the reference runs this configuration")
        refused.append(rec)
    with open(os.path.join(HERE, "solver_refused.json"), "w") as f:
        json.dump(refused, f, indent=1)
        f.write("\n")
    print("wrote solver_refused.json:", [(r["key"], r.get("reference_raises", r["reason"])) for r in refused])


if __name__ == "__main__":
    main()
