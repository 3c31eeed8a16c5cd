"""The general solver table on the engine: vv_set_schedule_general + vv_diffusion_sample_general (csrc/solver.hip ends every solver
step) against tests/solver_ref's table-driven sampler over the oracle's head -- solver_ref itself is held to the reference
scheduler's recorded steps by tests/test_solver_family_cpu.py.

Step counts: 1 (one first-order step from the initial state), 5 (the smallest count that reaches a third-order step under
lower_order_final), 15 (the first where the reference's `N < 15` rule is off).  Every case samples twice, so the second call replays
the captured graph; both calls must agree bit for bit and the graphs hold kernel nodes only."""
import pytest
import torch

import solver_ref
import synth
from gpu_util import build_small, rel_err
from oracle import head
from test_gpu_geometry import build_fast, dev
from test_gpu_head_seam import _lmcfg

pytestmark = pytest.mark.gpu

CFG_SCALE = 1.3
CONFIGS = {
    "order3": dict(solver_order=3),
    "order3-trailing-sigma_min-nolof": dict(solver_order=3, timestep_spacing="trailing", final_sigmas_type="sigma_min", lower_order_final=False),
    "order1": dict(solver_order=1),
    "order2-heun": dict(solver_type="heun"),
    "sde-heun": dict(algorithm_type="sde-dpmsolver++", solver_type="heun"),
    "sde-leading-offset1": dict(algorithm_type="sde-dpmsolver++", timestep_spacing="leading", steps_offset=1),
    "euler_at_final-sigma_min": dict(euler_at_final=True, final_sigmas_type="sigma_min", lower_order_final=False),
}
_engines = {}


def _engine(kind):
    """one engine per mode for the module: fp32 (xsplit 3), bf16 (xsplit 1, 8 slots), and a 256-wide bf16 head for the fused form"""
    if kind not in _engines:
        if kind == "fp32":
            _engines[kind] = build_small(synth.LMCfg(), xsplit=3, use_graph=True)
        elif kind == "bf16":
            _engines[kind] = build_small(synth.LMCfg(), xsplit=1, n_slots=8, use_graph=True)
        else:
            xs = {"wide": 1, "wide-fp32": 3, "wide-twolaunch": 1}[kind]
            _engines[kind] = build_fast(_lmcfg(256), xsplit=xs, use_graph=True, n_slots=2, max_ctx=128, max_rows=16, head_layers=2)
    return _engines[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for s in _engines.values():
        s.eng.close()
    _engines.clear()


def _inputs(seed, n, H, n_steps):
    g = synth.Gen(seed)
    return (g.normal((n, H), 1.0, mat=False), g.normal((n, H), 1.0, mat=False), g.normal((n, 64), 1.0, mat=False),
            g.normal((max(n_steps, 1), n, 64), 1.0, mat=False))


def _oracle(s, cfg, n_steps, pos, neg, noise, step_noise, cfg_scale=CFG_SCALE):
    hf = lambda a, t, c: head.head_forward(s.head_w, a, t, c, s.hc.layers, s.hc.eps)
    with torch.no_grad():
        return solver_ref.sample(hf, cfg, n_steps, pos, neg, cfg_scale, noise, step_noise=step_noise if solver_ref.stochastic(cfg) else None)


def _install(eng, cfg, n_steps):
    cfg = dict(cfg)
    eng.set_num_steps(n_steps, algorithm_type=cfg.pop("algorithm_type", "dpmsolver++"), solver=cfg)


def _sample(s, cfg, n_steps, pos, neg, noise, step_noise, cfg_scale=CFG_SCALE, out=None, bufs=None):
    eng = s.eng
    _install(eng, cfg, n_steps)
    n = noise.shape[0]
    if bufs is None:
        bufs = (dev(torch.cat([pos, neg]), eng), dev(noise, eng), dev(step_noise, eng) if solver_ref.stochastic(cfg) else None, eng.new(n, 64))
    cd, nz, sn, out = bufs
    with torch.cuda.stream(eng.stream):
        eng.diffusion_sample(n, cd, nz, cfg_scale, out, step_noise=sn)
    eng.sync()
    return out.cpu().clone(), bufs


def _twice(s, cfg, n_steps, inputs, bound, graph=True):
    pos, neg, noise, step_noise = inputs
    ref = _oracle(s, cfg, n_steps, pos, neg, noise, step_noise)
    a, bufs = _sample(s, cfg, n_steps, *inputs)
    b, _ = _sample(s, cfg, n_steps, *inputs, bufs=bufs)          # the same buffers: the captured graph replays
    err = rel_err(a, ref)
    print(f"[general solver] {cfg} N={n_steps} n={noise.shape[0]}: rel-L2 vs the table sampler {err:.3e}")
    assert bool(torch.isfinite(a).all()) and err <= bound, err
    assert torch.equal(a, b)
    if graph:
        assert s.eng.stat(5) == 0, s.eng.stat(5)
    return a


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("n_steps", [1, 5, 15])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fp32_mode_against_the_table_sampler(name, n_steps, n):
    """xsplit = 3: the bound tests/test_gpu_kernels.py::test_sampler holds the shipped sampler to"""
    s = _engine("fp32")
    _twice(s, CONFIGS[name], n_steps, _inputs(4000 + 31 * n_steps + n, n, s.hc.hidden, n_steps), 5e-4)
    assert s.eng.stat(8) == 0          # a 128-wide head: the update ran alone, head_eval did its own in-projection


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16_mode_against_the_table_sampler(name, n):
    """xsplit = 1, 2 / 6 / 16 head rows (GEMV rows, then the packed 16-row forms): test_bf16_mode_batched_sampler_rows' bound"""
    s = _engine("bf16")
    _twice(s, CONFIGS[name], 5, _inputs(4100 + n, n, s.hc.hidden, 5), 5e-2)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("kind,bound", [("wide", 5e-2), ("wide-fp32", 5e-4)])
def test_the_fused_in_projection_ran_on_a_wide_head(kind, bound, name):
    """H = 256: every step but the last carries the next step's in-projection (vv_stat 8 counts them, as vv_stat 6 counts seams)"""
    s = _engine(kind)
    _twice(s, CONFIGS[name], 5, _inputs(4200, 1, 256, 5), bound)
    assert s.eng.stat(8) == 4, s.eng.stat(8)
    assert s.eng.stat(6) == 0                     # the general path never takes the seam


@pytest.mark.parametrize("n", [1, 2])
def test_fused_in_projection_equals_the_in_projection_gemm(n, monkeypatch):
    """The fused form against "update kernel + the existing in-projection GEMM" (VVHIP_SOLVER_FUSE=0, read when the context is
    created) on the same weights and inputs.  Both quantise z' to the same bf16 operand and accumulate 64 products in fp32; they
    differ in the order of that sum only: <= 64 x 2^-24 = 4e-6 of a row's scale per step, 5 steps -> 2e-5; held to 1e-4."""
    fused = _engine("wide")
    monkeypatch.setenv("VVHIP_SOLVER_FUSE", "0")
    plain = _engine("wide-twolaunch")
    monkeypatch.delenv("VVHIP_SOLVER_FUSE")
    inputs = _inputs(4300 + n, n, 256, 5)
    a, _ = _sample(fused, CONFIGS["order3"], 5, *inputs)
    assert fused.eng.stat(8) == 4
    b, _ = _sample(plain, CONFIGS["order3"], 5, *inputs)
    assert plain.eng.stat(8) == 0
    err = rel_err(a, b)
    print(f"[general solver] fused vs two-launch in-projection, n={n}: rel-L2 {err:.3e}")
    assert err <= 1e-4, err


def test_cfg_rows_match_scalar_runs_and_replay():
    """cfg_rows = [1.0, 3.0] at n = 2 equals two n = 1 runs with scalar scales; rewriting the buffer replays the same graph"""
    s = _engine("fp32")
    eng = s.eng
    cfg = CONFIGS["order3"]
    pos, neg, noise, sn = _inputs(4400, 2, s.hc.hidden, 5)
    solo = [_sample(s, cfg, 5, pos[i:i + 1], neg[i:i + 1], noise[i:i + 1], sn[:, i:i + 1], cfg_scale=c)[0] for i, c in ((0, 1.0), (1, 3.0))]
    rows = dev(torch.tensor([1.0, 3.0]), eng)
    both, bufs = _sample(s, cfg, 5, pos, neg, noise, sn, cfg_scale=rows)
    for i in range(2):
        assert rel_err(both[i], solo[i][0]) <= 5e-4, (i, rel_err(both[i], solo[i][0]))
    _sample(s, cfg, 5, pos, neg, noise, sn, cfg_scale=rows, bufs=bufs)          # second sight: captured
    graphs = eng.stat(1)
    with torch.cuda.stream(eng.stream):
        rows.copy_(torch.tensor([3.0, 1.0]))
    swapped, _ = _sample(s, cfg, 5, pos, neg, noise, sn, cfg_scale=rows, bufs=bufs)
    assert eng.stat(1) == graphs and eng.stat(5) == 0
    ref = _oracle(s, cfg, 5, pos, neg, noise, sn, cfg_scale=torch.tensor([3.0, 1.0]))
    assert rel_err(swapped, ref) <= 5e-4 and rel_err(swapped, both) > 1e-2


@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_general_entry_point_on_the_shipped_settings(algo):
    """vv_set_schedule_general fed make_general_table of a shipped configuration (the engine wrapper would route it to the shipped
    path, so the table goes in through the C ABI) agrees with vv_diffusion_sample / _sde; switching general -> shipped returns
    the shipped sampler's earlier output bit for bit."""
    import ctypes as C
    import numpy as np
    from vibevoice_amd import schedule
    s = _engine("fp32")
    eng = s.eng
    pos, neg, noise, sn = _inputs(4500, 2, s.hc.hidden, 5)
    cd, nz, snd, out = dev(torch.cat([pos, neg]), eng), dev(noise, eng), dev(sn, eng), eng.new(2, 64)
    sde = algo == "sde-dpmsolver++"

    def shipped():
        eng.set_num_steps(5, algorithm_type=algo)
        with torch.cuda.stream(eng.stream):
            eng.diffusion_sample(2, cd, nz, CFG_SCALE, out, step_noise=snd if sde else None)
        eng.sync()
        return out.cpu().clone()
    before = shipped()
    tv, coef = schedule.make_general_table({"algorithm_type": algo}, 5)
    fp = C.POINTER(C.c_float)
    eng._chk(eng.lib.vv_set_schedule_general(eng._ctx, 5, tv.ctypes.data_as(fp), np.ascontiguousarray(coef).ctypes.data_as(fp), int(sde), eng._s),
             "vv_set_schedule_general")
    eng._n_steps = None
    eng._chk(eng.lib.vv_diffusion_sample_general(eng._ctx, eng._s, 2, eng._p(cd), eng._p(nz), eng._p(snd if sde else None), CFG_SCALE,
                                                 C.c_void_p(), eng._p(out)), "vv_diffusion_sample_general")
    eng.sync()
    assert rel_err(out.cpu(), before) <= 5e-4, rel_err(out.cpu(), before)
    assert torch.equal(shipped(), before)


def test_switching_to_a_shipped_table_and_back():
    s = _engine("fp32")
    inputs = _inputs(4600, 1, s.hc.hidden, 5)
    a, bufs = _sample(s, CONFIGS["order3"], 5, *inputs)
    _sample(s, CONFIGS["order3"], 5, *inputs, bufs=bufs)
    shipped, _ = _sample(s, {}, 5, *inputs, bufs=bufs)            # a shipped configuration: the shipped table and sampler
    assert s.eng.general_solver is False and rel_err(shipped, a) > 1e-3
    back, _ = _sample(s, CONFIGS["order3"], 5, *inputs, bufs=bufs)
    assert torch.equal(back, a) and s.eng.stat(5) == 0


def test_guard_rails():
    from vibevoice_amd.engine import EngineError
    import ctypes as C
    s = _engine("fp32")
    eng = s.eng
    pos, neg, noise, sn = _inputs(4700, 1, s.hc.hidden, 5)
    cd, nz, snd, out = dev(torch.cat([pos, neg]), eng), dev(noise, eng), dev(sn, eng), eng.new(1, 64)

    def general(step_noise=None, n=1):
        eng._chk(eng.lib.vv_diffusion_sample_general(eng._ctx, eng._s, n, eng._p(cd), eng._p(nz), eng._p(step_noise), CFG_SCALE, C.c_void_p(),
                                                     eng._p(out)), "vv_diffusion_sample_general")
    eng.set_num_steps(5)
    with pytest.raises(EngineError, match="shipped one"):
        general()
    _install(eng, CONFIGS["order3"], 5)
    with pytest.raises(EngineError, match="takes no step noise"):
        general(snd)
    with pytest.raises(EngineError, match=r"n must be in \[1,8\]"):
        general(n=9)
    for call, name in ((lambda: eng.lib.vv_diffusion_sample(eng._ctx, eng._s, 1, eng._p(cd), eng._p(nz), CFG_SCALE, eng._p(out)), "vv_diffusion_sample"),
                       (lambda: eng.lib.vv_diffusion_sample_sde(eng._ctx, eng._s, 1, eng._p(cd), eng._p(nz), eng._p(snd), CFG_SCALE, eng._p(out)),
                        "vv_diffusion_sample_sde"),
                       (lambda: eng.lib.vv_diffusion_sample_rows(eng._ctx, eng._s, 1, eng._p(cd), eng._p(nz), None, eng._p(nz), eng._p(out)),
                        "vv_diffusion_sample_rows")):
        with pytest.raises(EngineError, match="general one"):
            eng._chk(call(), name)
    _install(eng, CONFIGS["sde-heun"], 5)
    with pytest.raises(EngineError, match="needs its per-step noise"):
        general()
    general(snd)
    eng.sync()
    assert bool(torch.isfinite(out).all())
    with pytest.raises(NotImplementedError, match="solver_order"):
        eng.set_num_steps(5, algorithm_type="sde-dpmsolver++", solver={"solver_order": 3})
    with pytest.raises(ValueError, match="sampling-time"):
        eng.set_num_steps(5, solver={"use_karras_sigmas": True})
    eng.set_num_steps(5)


def test_generate_under_a_general_configuration():
    """generate() on the small model under solver_order = 3 / trailing spacing with a seeded request: finite, identical over two runs
    and between generate() and generate_continuous(), and not the shipped configuration's audio."""
    from test_gpu_noise_rows import TOK, _requests
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    s = _engine("wide-fp32")            # 64-token vocabulary, 2 slots, graphs on; H = 256, so the fused step end runs inside generate()
    cfgd = {"decoder_config": {"max_position_embeddings": s.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.float32)
    m.set_speech_factors(s.scaling, s.bias)
    m.set_ddpm_inference_steps(5)
    a = _requests()[0]
    kw = dict(tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=1.3)

    def solo():
        return m.generate(input_ids=a["input_ids"], attention_mask=a["attention_mask"], seed=a["seed"], _forced_tokens=[a["_forced_tokens"]],
                          show_progress_bar=False, **kw).speech_outputs[0].cpu()
    shipped = solo()
    sched = m.model.noise_scheduler
    m.model.noise_scheduler = sched.from_config(sched.config, solver_order=3, timestep_spacing="trailing")
    assert m.noise_scheduler.timesteps.tolist() == [999, 799, 599, 399, 199]
    w1, w2 = solo(), solo()
    assert s.eng.general_solver is True
    assert bool(torch.isfinite(w1).all()) and torch.equal(w1, w2)
    queued = m.generate_continuous([a], max_concurrent=1, **kw)[0].speech_outputs[0].cpu()
    assert torch.equal(queued, w1)
    assert rel_err(w1, shipped) > 1e-3
    assert s.eng.stat(5) == 0 and s.eng.stat(4) == 0
