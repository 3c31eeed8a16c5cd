"""The reference scheduler's other DPM-Solver++ settings, on the CPU: vibevoice_amd.schedule.make_general_table against the
reference's own set_timesteps() / step() (tests/golden/solver_family.npz, written by tests/golden/make_solver_golden.py), the
refusals of tests/golden/solver_refused.json, and the host routing of a general configuration through generate()."""
import json
import os

import numpy as np
import pytest
import torch

import fake_engine
import solver_fake_engine
import solver_ref
from test_dropin_cpu import TOK, tiny_reference_config, tiny_reference_state_dict
from test_oracle_golden import G as GOLD
from vibevoice_amd import schedule

FAM = np.load(os.path.join(GOLD, "solver_family.npz"))
CONFIGS = json.loads(str(FAM["configs"]))
with open(os.path.join(GOLD, "solver_refused.json")) as _f:
    REFUSED = json.load(_f)
RUNS = {}
for _r in range(len(FAM["run_n"])):
    RUNS.setdefault(int(FAM["run_cfg"][_r]), []).append((int(FAM["run_n"][_r]), int(FAM["run_off"][_r]), int(FAM["run_len"][_r])))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_grid_is_the_issue_s():
    assert len(CONFIGS) >= 120 and sorted({n for runs in RUNS.values() for n, _, _ in runs}) == [1, 2, 3, 5, 6, 14, 15, 20]
    full = [schedule.solver_settings(c) for c in CONFIGS]
    for key, values in (("algorithm_type", schedule.ALGORITHMS), ("solver_order", (1, 2, 3)), ("solver_type", ("midpoint", "heun")),
                        ("lower_order_final", (True, False)), ("euler_at_final", (True, False)), ("final_sigmas_type", ("zero", "sigma_min")),
                        ("timestep_spacing", ("linspace", "leading", "trailing"))):
        assert {c[key] for c in full} == set(values), key
    assert any(c["timestep_spacing"] == "leading" and c["steps_offset"] == 1 for c in full)
    assert any(c["lambda_min_clipped"] == -5.1 for c in full)


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=lambda i: "-".join(f"{v}" for v in CONFIGS[i].values()))
def test_table_reproduces_the_reference_steps(ci):
    """Timesteps as integers, sigmas bit for bit; a first-order step bit-equal to the reference's prev_sample, every other step
    within 1e-6 of the trajectory's largest magnitude (the re-association of at most five fp32 terms; measured worst case over
    the grid: 2.2e-7).  Each step starts from the reference's own previous state."""
    cfg = CONFIGS[ci]
    sample0, vs, nz = (torch.from_numpy(FAM[k]) for k in ("sample0", "model_out", "noise"))
    for n, off, ln in RUNS[ci]:
        ts, sig = schedule.general_timesteps_and_sigmas(cfg, n)
        tv, coef = schedule.make_general_table(cfg, n)
        assert ts.dtype == np.int64 and np.array_equal(ts, FAM["timesteps"][off:off + ln]) and np.array_equal(tv, ts.astype(np.float32))
        assert np.array_equal(bits(sig[:-1].numpy()), bits(FAM["sigmas_cur"][off:off + ln]))
        assert np.array_equal(bits(sig[1:].numpy()), bits(FAM["sigmas_next"][off:off + ln]))
        assert coef.shape == (ln, 8) and np.isfinite(coef).all() and (coef[:, 7] == 0).all()
        orders = schedule.step_orders(cfg, ln)
        z, m1, m2 = sample0, None, None
        for i in range(ln):
            x0, zn = solver_ref.step(coef[i], z, vs[i], m1, m2, nz[i])
            ref = torch.from_numpy(FAM["prev_sample"][off + i])
            if orders[i] == 1:
                assert coef[i, 4] == 0 and coef[i, 5] == 0
                assert torch.equal(zn, ref), (cfg, n, i)
            else:
                d, top = float((zn - ref).abs().max()), float(ref.abs().max())
                assert d <= 1e-6 * top, (cfg, n, i, d / top)
            z, m1, m2 = ref, x0, m1


@pytest.mark.parametrize("algo", schedule.ALGORITHMS)
@pytest.mark.parametrize("n", [1, 2, 5, 10, 20])
def test_general_table_equals_make_table_on_the_shipped_configurations(algo, n):
    for cast in (False, True):
        tv, c = schedule.make_table(n, cast, algo)
        tg, g = schedule.make_general_table({"algorithm_type": algo}, n, cast)
        assert np.array_equal(bits(tv), bits(tg))
        assert np.array_equal(bits(c[:, :5]), bits(g[:, :5])) and (g[:, 5] == 0).all() and (g[:, 7] == 0).all()
        assert np.array_equal(bits(c[:, 5]), bits(g[:, 6])) if algo == "sde-dpmsolver++" else (g[:, 6] == 0).all()
    assert schedule.is_shipped({"algorithm_type": algo}) and schedule.is_shipped(dict(schedule.SHIPPED, algorithm_type=algo))
    assert not schedule.is_shipped({"algorithm_type": algo, "solver_order": 1})


@pytest.mark.parametrize("n", [5, 10, 20])
def test_make_table_is_unchanged(n):
    """against the reference's recorded timesteps and sigmas, as tests/test_oracle_golden.py reads them"""
    g = np.load(os.path.join(GOLD, "dpm_schedule.npz"))
    tv, coef = schedule.make_table(n)
    assert coef.shape == (n, 5) and np.array_equal(tv, g[f"timesteps_{n}"].astype(np.float32))
    sig = torch.from_numpy(g[f"sigmas_{n}"])
    a = 1 / ((sig[:-1] ** 2 + 1) ** 0.5)
    assert np.array_equal(bits(coef[:, 0]), bits(a.numpy())) and np.array_equal(bits(coef[:, 1]), bits((sig[:-1] * a).numpy()))
    assert coef[0, 4] == 0 and coef[-1, 4] == 0 and coef[-1, 2] == 0 and coef[-1, 3] == 1


# ---------------------------------------------------------------- the drop-in class
@pytest.fixture()
def model(monkeypatch):
    from vibevoice_amd import modeling
    with fake_engine.cpu_cuda_shims(monkeypatch):
        monkeypatch.setattr(modeling, "Engine", solver_fake_engine.SolverFakeEngine)
        m = modeling.VibeVoiceForConditionalGenerationInference.from_state_dict(
            tiny_reference_config(), tiny_reference_state_dict(), torch.float32, "cuda")
        m.set_ddpm_inference_steps(5)
        yield m


@pytest.mark.parametrize("rec", REFUSED, ids=lambda r: "-".join(f"{k}={v}" for k, v in r["overrides"].items()))
def test_refused_configurations_name_their_key_at_the_assignment(model, rec):
    sched = model.model.noise_scheduler
    with pytest.raises(NotImplementedError) as ei:
        model.model.noise_scheduler = sched.from_config(sched.config, **rec["overrides"])
    text = str(ei.value)
    assert rec["key"] + "=" in text
    want = {"reference": "the reference itself fails", "deprecated": "deprecated by the reference", "training-time": "how the checkpoint was trained"}
    assert want[rec["reason"]] in text
    if rec["reason"] == "reference":
        assert any(rec["reference_raises"].values())
    assert model.model.noise_scheduler.config.solver_order == 2         # a refused swap changes nothing


def test_every_grid_configuration_is_accepted(model):
    sched = model.model.noise_scheduler
    for ci, cfg in enumerate(CONFIGS):
        model.model.noise_scheduler = sched.from_config(sched.config, **cfg)
        view = model.model.noise_scheduler
        assert all(view.config[k] == v for k, v in cfg.items()), cfg
        n, off, ln = RUNS[ci][3]
        assert n == 5 and torch.equal(view.timesteps, torch.from_numpy(FAM["timesteps"][off:off + ln])), cfg


def test_a_steps_offset_that_leaves_the_train_range_is_refused(model):
    sched = model.model.noise_scheduler
    with pytest.raises(ValueError, match="steps_offset"):
        model.model.noise_scheduler = sched.from_config(sched.config, timestep_spacing="leading", steps_offset=400)


def _inputs():
    z = np.load(os.path.join(GOLD, "generate_forced_b2.npz"))
    B = z["input_ids"].shape[0]
    inputs = {k: torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "speech_tensors", "speech_masks", "speech_input_mask")}
    return inputs, [z["forced"][b][:int(z["forced_len"][b])].tolist() for b in range(B)]


def _generate(model, **kw):
    inputs, forced = _inputs()
    return model.generate(**inputs, max_new_tokens=None, cfg_scale=1.3, tokenizer=TOK, generation_config={"do_sample": False}, verbose=False,
                          is_prefill=True, _forced_tokens=forced, **kw)


def test_routing_shipped_configurations_pass_no_solver(model):
    sched = model.model.noise_scheduler
    for over in ({}, {"algorithm_type": "sde-dpmsolver++"}, dict(schedule.SHIPPED)):
        model.model.noise_scheduler = sched.from_config(sched.config, **over)
        model.engine.log.clear()
        torch.manual_seed(3)
        _generate(model)
        sets = [r for r in model.engine.log if r[0] == "set_num_steps"]
        assert sets and all("solver" not in r[2] for r in sets), sets


def test_routing_a_general_configuration_passes_its_settings_and_draws_per_step(model):
    sched = model.model.noise_scheduler
    model.model.noise_scheduler = sched.from_config(sched.config, algorithm_type="sde-dpmsolver++", solver_type="heun", timestep_spacing="trailing")
    draws = []
    real = torch.randn

    def counting(*shape, **kw):
        draws.append(tuple(shape[0]) if isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape))
        return real(*shape, **kw)
    torch.manual_seed(3)
    try:
        torch.randn = counting
        _generate(model)
    finally:
        torch.randn = real
    sets = [r for r in model.engine.log if r[0] == "set_num_steps"]
    assert sets and all(r[2] == {"algorithm_type": "sde-dpmsolver++", "solver": {"solver_type": "heun", "timestep_spacing": "trailing"}} for r in sets)
    samples = [r for r in model.engine.log if r[0] == "sample"]
    assert samples and all(r[2] == (5, r[1], 64) for r in samples)
    # per sampled frame: its initial noise, then one randn(2n, 64) per solver step (scheduler.step() draws the model output's shape)
    wide = [sh for sh in draws if len(sh) == 2 and sh[1] == 64]
    assert len(wide) == len(samples) * (1 + 5) and all(sh[0] == 2 * samples[0][1] for sh in wide)
    # a fork carries the configuration
    f = model.fork()
    assert f.noise_scheduler.config.solver_type == "heun" and f.noise_scheduler.config.timestep_spacing == "trailing"
    model.set_ddpm_inference_steps(7)
    assert model.noise_scheduler.timesteps.shape[0] == 7


def test_generate_under_third_order_is_the_table_sampler_run_by_hand(model):
    """generate() under solver_order=3: every frame's latent is tests/solver_ref's sampler on the same condition and noise, so the
    audio differs from the shipped configuration's and equals a second engine's that is handed the table's settings directly."""
    sched = model.model.noise_scheduler
    torch.manual_seed(11)
    base = _generate(model)
    model.model.noise_scheduler = sched.from_config(sched.config, solver_order=3)
    eng = model.engine
    seen = []
    real = eng.diffusion_sample

    def spy(n, cond, noise, cfg_scale, latent_out, step_noise=None):
        real(n, cond, noise, cfg_scale, latent_out, step_noise=step_noise)
        seen.append((n, cond[:2 * n].clone(), noise[:n].clone(), cfg_scale, latent_out[:n].clone()))
    eng.diffusion_sample = spy
    torch.manual_seed(11)
    out = _generate(model)
    assert seen and eng.solver == {"solver_order": 3}
    from oracle import head
    om = eng.om
    for n, cond, noise, cfg, lat in seen:
        by_hand = solver_ref.sample(lambda x, t, c: head.head_forward(om.head_w, x, t, c, om.head_layers, om.head_eps),
                                    {"solver_order": 3}, 5, cond[:n], cond[n:], cfg, noise)
        assert torch.equal(by_hand, lat)
    assert torch.equal(out.sequences, base.sequences)
    assert not torch.allclose(out.speech_outputs[0].float(), base.speech_outputs[0].float())


# ---------------------------------------------------------------- the head's route under a general table (csrc/pass_plan.h)
def test_head_plan_under_a_general_table(tmp_path):
    """vv_head_plan(..., solver_step): the modulations stay batched and the layers keep their route, as for the shipped samplers; no
    seam, no packed shift tiles (they serve the P16 CFG epilogue alone), and every step ends with the final layer's plain store."""
    import subprocess
    from vibevoice_amd import build as vvbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "probe")
    subprocess.run([vvbuild._hipcc(), "--offload-host-only", "-std=c++17", "-I", os.path.join(root, "vibevoice_amd", "csrc"),
                    os.path.join(root, "tests", "solver_plan_probe.hip"), "-o", exe], check=True)
    FINAL_GEMM = 3
    # rows, n_steps, HF, HL, MODW, p16_ok, p16_shift, ada_p, mod_all, head_tail: a bf16 context (everything offered) at 2 / 6 / 16
    # rows, 20 and 1 steps, and an exact-mode context (nothing but the batched modulations)
    cases = [(2, 20, 10752, 4, 50176, 1, 1, 1, 1, 1), (6, 20, 10752, 4, 50176, 1, 1, 1, 1, 1), (16, 5, 384, 2, 1024, 1, 1, 1, 1, 1),
             (2, 1, 384, 2, 1024, 1, 1, 1, 1, 1), (2, 5, 384, 2, 1024, 0, 0, 0, 1, 0), (16, 5, 384, 2, 1024, 0, 0, 0, 1, 0)]
    out = subprocess.run([exe], input="\n".join(" ".join(map(str, c)) for c in cases) + "\n", capture_output=True, text=True, check=True).stdout
    lines = [list(map(int, l.split())) for l in out.split("\n") if l.strip()]
    assert len(lines) == 2 * len(cases)
    seams = 0
    for c, shipped, general in zip(cases, lines[0::2], lines[1::2]):
        assert general[0] == shipped[0] and general[2] == shipped[2], (c, shipped, general)        # ada, layers
        assert general[1] == 0 and general[3] == 0 and general[4] == FINAL_GEMM, (c, general)
        assert general[5] == 1 and shipped[5] == 0, (c, shipped, general)                          # solver_step: solver.hip ends the step
        assert general[6:] == [FINAL_GEMM] * c[1], (c, general)
        seams += shipped[3]
    assert seams == 2          # the shipped plan of the two-row bf16 cases takes the seam: the probe distinguishes the two plans
