"""Host-side DPM-Solver++(2M) coefficient table for the HIP sampler.

The reference recomputes these scalars on the CPU for every generated frame
(`noise_scheduler.set_timesteps(N)` + ~30 0-dim tensor ops per solver step,
vibevoice/schedule/dpm_solver.py:321-423, 669-677, 738-764).  They depend only
on N, so they are computed once here -- in fp32 with the same formulas and
operation order -- and handed to `vv_set_schedule`; the device side
(vv_cfg_dpm_update, csrc/vv_device.h) then applies

    x0  = a_i * x - s_i * v                       (v-prediction, :581-584)
    x'  = cs_i * x + c0_i * x0 + c1_i * (x0 - x0_prev)

Configuration: the one the reference ships (cosine betas, v_prediction,
dpmsolver++, solver_order 2, midpoint, linspace spacing, final sigma 0;
modeling_vibevoice.py:138-142, configs/*.json:66-77), and the same with
sde-dpmsolver++: make_table.  Every other combination of the scheduler's
sampling-time settings: make_general_table, further down.
"""
import math

import numpy as np
import torch


def _alphas_cumprod(num_train=1000, max_beta=0.999):
    # betas_for_alpha_bar(cosine)  (dpm_solver.py:52-56, 79-83)
    f = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = [min(1 - f((i + 1) / num_train) / f(i / num_train), max_beta) for i in range(num_train)]
    return torch.cumprod(1.0 - torch.tensor(betas, dtype=torch.float32), dim=0)


def timesteps_and_sigmas(n_steps, num_train=1000):
    ac = _alphas_cumprod(num_train)
    ts = np.linspace(0, num_train - 1, n_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
    sig = (((1 - ac) / ac) ** 0.5).numpy()
    sig = np.interp(ts, np.arange(0, len(sig)), sig)
    sig = np.concatenate([sig, [0]]).astype(np.float32)
    return ts, torch.from_numpy(sig)


def _as(sigma):
    a = 1 / ((sigma ** 2 + 1) ** 0.5)
    return a, sigma * a


ALGORITHMS = ("dpmsolver++", "sde-dpmsolver++")


def make_table(n_steps, t_cast_bf16=False, algorithm_type="dpmsolver++"):
    """-> (t_values float32[n], coef float32[n,5]) for the deterministic solver the model classes build, or coef float32[n,6]
    = {a, s, cs, c0, c1, cn} for "sde-dpmsolver++" (what demo/gradio_demo.py:142-146 swaps in):
        x' = cs x + c0 x0 + c1 (x0 - x0_prev) + cn eps_i,  eps_i ~ N(0, 1) drawn once per solver step
    with cs = (sigma_t / sigma_s) e^{-h}, c0 = alpha_t (1 - e^{-2h}), c1 = c0 / (2 r0), cn = sigma_t sqrt(1 - e^{-2h})
    (dpm_solver.py:680-686, 785-793)."""
    if algorithm_type not in ALGORITHMS:
        raise NotImplementedError(f"noise scheduler algorithm_type={algorithm_type!r}: the HIP sampler implements {ALGORITHMS}")
    sde = algorithm_type == "sde-dpmsolver++"
    ts, sig = timesteps_and_sigmas(n_steps)
    coef = np.zeros((n_steps, 6 if sde else 5), dtype=np.float32)
    for i in range(n_steps):
        a_i, s_i = _as(sig[i])
        a_t, s_t = _as(sig[i + 1])
        lam_t = torch.log(a_t) - torch.log(s_t)
        lam_s = torch.log(a_i) - torch.log(s_i)
        h = lam_t - lam_s
        if sde:
            c0 = a_t * (1 - torch.exp(-2.0 * h))
            cs = s_t / s_i * torch.exp(-h)
            cn = s_t * torch.sqrt(1.0 - torch.exp(-2 * h))
        else:
            c0 = -(a_t * (torch.exp(-h) - 1.0))
            cs = s_t / s_i
        c1 = torch.zeros(())
        first_order = (i == 0) or (i == n_steps - 1)      # lower_order_nums<1 / final sigma == 0
        if not first_order:
            a_p, s_p = _as(sig[i - 1])
            lam_p = torch.log(a_p) - torch.log(s_p)
            r0 = (lam_s - lam_p) / h
            c1 = 0.5 * c0 * (1.0 / r0)
        coef[i, :5] = [float(a_i), float(s_i), float(cs), float(c0), float(c1)]
        if sde:
            coef[i, 5] = float(cn)
    tv = torch.from_numpy(ts).to(torch.float32)
    if t_cast_bf16:
        # the reference feeds `t.repeat(..).to(combined)` to the head
        # (modeling_vibevoice_inference.py:705): under bf16 weights the integer
        # timestep is rounded to bf16 (999 -> 1000, 949 -> 948, ...)
        tv = tv.to(torch.bfloat16).to(torch.float32)
    return tv.numpy().astype(np.float32), coef


# ---- the general table: the reference scheduler's other sampling-time settings ----
# What a caller can pass to noise_scheduler.from_config(config, **overrides) and have sampled on the device.  Every setting in
# SAMPLING_KEYS is a choice of how a trained checkpoint is sampled; one table row per solver step then drives
#     x0 = a z - s v
#     z' = cs z + c0 x0 + c1 (x0 - m1) + c2 (m1 - m2) + cn noise          (m1, m2: the two previous x0)
# (csrc/solver.hip).  The two configurations make_table serves are the special case c2 = 0 and keep their own path.
SHIPPED = dict(solver_order=2, solver_type="midpoint", lower_order_final=True, euler_at_final=False, final_sigmas_type="zero",
               timestep_spacing="linspace", steps_offset=0, lambda_min_clipped=-float("inf"))
SAMPLING_KEYS = ("algorithm_type",) + tuple(SHIPPED)
SOLVER_DEFAULTS = dict(SHIPPED, algorithm_type="dpmsolver++")
NUM_TRAIN = 1000


def solver_settings(config):
    """the sampling-time settings of a scheduler configuration (missing keys: the reference's defaults)"""
    return {k: config.get(k, v) if hasattr(config, "get") else getattr(config, k, v) for k, v in SOLVER_DEFAULTS.items()}


def is_shipped(config):
    """True when the configuration is one of the two make_table serves: it then keeps the shipped sampler, graphs and goldens"""
    s = solver_settings(config)
    return s["algorithm_type"] in ALGORITHMS and all(s[k] == v for k, v in SHIPPED.items())


def check_solver(config):
    """-> {key: (value, reason)} for every sampling-time setting of `config` the general table does not take"""
    s = solver_settings(config)
    bad = {}
    if s["algorithm_type"] in ("dpmsolver", "sde-dpmsolver"):
        bad["algorithm_type"] = (s["algorithm_type"], "deprecated by the reference and ill-conditioned in fp32 under the cosine schedule "
                                 "(alpha_t / alpha_s is of the order of 1e3 on the first step)")
    elif s["algorithm_type"] not in ALGORITHMS:
        bad["algorithm_type"] = (s["algorithm_type"], f"not a solver of the reference; the HIP sampler implements {ALGORITHMS}")
    if s["solver_order"] not in (1, 2, 3):
        bad["solver_order"] = (s["solver_order"], "the reference has orders 1, 2 and 3")
    elif s["solver_order"] == 3 and s["algorithm_type"] == "sde-dpmsolver++":
        bad["solver_order"] = (3, "the reference itself fails on it: sde-dpmsolver++ has no third-order update (UnboundLocalError)")
    for key, allowed in (("solver_type", ("midpoint", "heun")), ("final_sigmas_type", ("zero", "sigma_min")),
                         ("timestep_spacing", ("linspace", "leading", "trailing"))):
        if s[key] not in allowed:
            bad[key] = (s[key], f"the reference takes {allowed}")
    return bad


def general_timesteps_and_sigmas(config, n_steps):
    """set_timesteps(n_steps) of the reference (dpm_solver.py:321-423) for the settings in scope: int64 timesteps and the
    fp32 sigmas, one more than timesteps (sigma_last by final_sigmas_type)."""
    s = solver_settings(config)
    ac = _alphas_cumprod(NUM_TRAIN)
    lam = torch.log(torch.sqrt(ac)) - torch.log(torch.sqrt(1 - ac))
    # the lambda_min_clipped cut: train timesteps whose lambda lies below it are never visited
    last = NUM_TRAIN - int(torch.searchsorted(torch.flip(lam, [0]), float(s["lambda_min_clipped"])))
    n = int(n_steps)
    if s["timestep_spacing"] == "linspace":
        ts = np.linspace(0, last - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    elif s["timestep_spacing"] == "leading":
        ts = (np.arange(0, n + 1) * (last // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + int(s["steps_offset"])
    else:
        ts = np.arange(last, 0, -(NUM_TRAIN / n)).round().copy().astype(np.int64) - 1
    if len(ts) < 1 or ts.min() < 0 or ts.max() >= NUM_TRAIN:
        raise ValueError(f"noise scheduler: timestep_spacing={s['timestep_spacing']!r}, steps_offset={s['steps_offset']}, "
                         f"lambda_min_clipped={s['lambda_min_clipped']} at {n} steps leave [0, {NUM_TRAIN}) (timesteps {ts.tolist()})")
    sig = (((1 - ac) / ac) ** 0.5).numpy()
    sig = np.interp(ts, np.arange(0, len(sig)), sig)
    sig_last = ((1 - ac[0]) / ac[0]) ** 0.5 if s["final_sigmas_type"] == "sigma_min" else 0
    return ts, torch.from_numpy(np.concatenate([sig, [sig_last]]).astype(np.float32))


def step_orders(config, n):
    """the order scheduler.step() runs at each of n steps (dpm_solver.py:977-1011): the lower_order_nums ramp, the rules for
    the last and the second-to-last step"""
    s = solver_settings(config)
    order = int(s["solver_order"])
    out = []
    for i in range(n):
        lof = i == n - 1 and (s["euler_at_final"] or (s["lower_order_final"] and n < 15) or s["final_sigmas_type"] == "zero")
        los = i == n - 2 and s["lower_order_final"] and n < 15
        out.append(1 if (order == 1 or i < 1 or lof) else 2 if (order == 2 or i < 2 or los) else 3)
    return out


def make_general_table(config, n_steps, t_cast_bf16=False):
    """-> (t_values float32[N], coef float32[N, 8]) with row = {a, s, cs, c0, c1, c2, cn, 0}, fp32 scalars in the reference's
    operation order (the update functions of dpm_solver.py:669-686, 738-800, 861-893 with the model-output differences
    factored out).  N = len(timesteps): what the reference's set_timesteps(n_steps) yields, n_steps for every setting except
    where trailing spacing's float stride adds a step."""
    bad = check_solver(config)
    if bad:
        raise NotImplementedError("noise scheduler configuration not implemented by the HIP sampler: "
                                  + "; ".join(f"{k}={v!r}: {why}" for k, (v, why) in bad.items()))
    s = solver_settings(config)
    sde = s["algorithm_type"] == "sde-dpmsolver++"
    heun = s["solver_type"] == "heun"
    ts, sig = general_timesteps_and_sigmas(config, n_steps)
    n = len(ts)
    lam = lambda a, sg: torch.log(a) - torch.log(sg)
    coef = np.zeros((n, 8), dtype=np.float32)
    for i, order in enumerate(step_orders(config, n)):
        a_i, s_i = _as(sig[i])
        a_t, s_t = _as(sig[i + 1])
        lam_t, lam_s = lam(a_t, s_t), lam(a_i, s_i)
        h = lam_t - lam_s
        cn = torch.zeros(())
        if sde:
            c0 = a_t * (1 - torch.exp(-2.0 * h))
            cs = s_t / s_i * torch.exp(-h)
            cn = s_t * torch.sqrt(1.0 - torch.exp(-2 * h))
        else:
            c0 = -(a_t * (torch.exp(-h) - 1.0))
            cs = s_t / s_i
        c1 = c2 = torch.zeros(())
        if order >= 2:
            lam_p = lam(*_as(sig[i - 1]))
            r0 = (lam_s - lam_p) / h
        if order == 2:
            if not heun:
                d1 = 0.5 * c0
            elif sde:
                d1 = a_t * ((1.0 - torch.exp(-2.0 * h)) / (-2.0 * h) + 1.0)
            else:
                d1 = a_t * ((torch.exp(-h) - 1.0) / h + 1.0)
            c1 = d1 * (1.0 / r0)
        elif order == 3:
            r1 = (lam_p - lam(*_as(sig[i - 2]))) / h
            e1 = a_t * ((torch.exp(-h) - 1.0) / h + 1.0)
            e2 = -(a_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5))
            w = r0 / (r0 + r1)
            q = e2 * (1.0 / (r0 + r1))
            c1 = (e1 * (1.0 + w) + q) * (1.0 / r0)
            c2 = -((e1 * w + q) * (1.0 / r1))
        coef[i, :7] = [float(a_i), float(s_i), float(cs), float(c0), float(c1), float(c2), float(cn)]
    tv = torch.from_numpy(ts).to(torch.float32)
    if t_cast_bf16:
        tv = tv.to(torch.bfloat16).to(torch.float32)
    return tv.numpy().astype(np.float32), coef
