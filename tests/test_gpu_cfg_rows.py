"""GPU tests of the per-utterance guidance scale: vv_diffusion_sample_rows (Engine.diffusion_sample with a tensor cfg_scale), the
cfg_rows operand of the CFG + DPM-Solver++ epilogues, and the request key / generate() form on the product class.

The sampler grid is n = 1, 2, 3, 8 utterances x both solvers x xsplit 1 and 3 on a head of width 256 (the smallest the solver-step
seam takes), 5 solver steps.  In xsplit 1 that reaches the seam (n = 1: headtail.hip, and the 2-row decode GEMV on the last step), the
4-row decode GEMV (n = 2) and the packed 16-row final layer (n = 3: 6 rows, n = 8: all 16).  In xsplit 3 the final layer of
n = 1 and n = 2 (2 and 4 rows) is still the decode GEMV, in its three-way-split instantiations, and only n = 3 and n = 8 (6 and 16
rows) reach the general kernel's epilogue (gemm.hip).  The wide 16-row GEMV form is reached one launch at a time
(Engine.gemv_case).

Bit-for-bit claims rest on two facts: a per-row scale runs the same kernels with the same arithmetic as the scalar (one operand of
one multiply comes from memory instead of an argument register), and the rows of a sampler pass do not interact.  Every path is
first shown to reproduce itself run to run (asserted in test 2: the kernels reduce in a fixed order), so no path is held to the
looser oracle tolerance a non-deterministic one would need."""
import ctypes as C
import types

import pytest
import torch

import gemv_ref as R
import synth
from gpu_util import build_small, rel_err
from oracle import dpm, head
from oracle import generate as ogen

pytestmark = pytest.mark.gpu

SCALES = [1.0, 3.0, 0.0, 1.3, 2.0, 0.5, 1.7, 2.5]
SOLVERS = ("dpmsolver++", "sde-dpmsolver++")
NS = (1, 2, 3, 8)
H, N_STEPS = 256, 5
TOL = {3: 5e-4, 1: 5e-2}          # test_sampler / test_sampler_sde; test_bf16_mode_batched_sampler_rows


def dev(t, eng):
    out = t.to(eng.device, torch.float32).contiguous()
    torch.cuda.synchronize()
    return out


_engines = {}


def _small(xsplit, use_graph=False):
    key = (xsplit, use_graph)
    if key not in _engines:
        lm = synth.LMCfg(hidden=H, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)
        _engines[key] = build_small(lm, xsplit=xsplit, use_graph=use_graph, n_slots=8, max_ctx=128, max_rows=16, head_layers=2)
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for s in _engines.values():
        s.eng.close()
    _engines.clear()


_cases = {}


def _case(n, solver):
    """inputs of one (n, solver) cell and the CPU oracle's latents for the mixed vector -- computed once, shared, never written.
    Asserts the precondition of every test on these inputs: row 0 under two of the scales differs by more than 1e-1 relative."""
    key = (n, solver)
    if key not in _cases:
        s = _small(3)
        g = synth.Gen(4100 + 10 * n + SOLVERS.index(solver))
        pos, neg = g.normal((n, H), 1.0, mat=False), g.normal((n, H), 1.0, mat=False)
        noise = g.normal((2 * n, 64), 1.0, mat=False)
        sn = g.normal((N_STEPS, 2 * n, 64), 1.0, mat=False)
        sde = solver == "sde-dpmsolver++"
        hf = lambda x, t, c: head.head_forward(s.head_w, x, t, c, s.hc.layers, s.hc.eps)
        orc = lambda cfg: dpm.sample_speech_tokens(hf, pos, neg, cfg, N_STEPS, noise, algorithm_type=solver, step_noise=sn if sde else None)
        c = torch.tensor(SCALES[:n])
        with torch.no_grad():
            a, b = orc(1.0), orc(3.0)
            assert rel_err(a[0], b[0]) > 1e-1, rel_err(a[0], b[0])
            ref = orc(c[:, None])
        _cases[key] = types.SimpleNamespace(n=n, solver=solver, cond=torch.cat([pos, neg]), noise=noise[:n].contiguous(),
                                            sn=sn[:, :n].contiguous() if sde else None, c=c, ref=ref)
    return _cases[key]


def _sample(s, k, cfg):
    """cfg: a float, or a host tensor of n scales (uploaded to a fresh device vector)"""
    eng = s.eng
    eng.set_num_steps(N_STEPS, algorithm_type=k.solver)
    out = eng.new(k.n, 64)
    cd, nz = dev(k.cond, eng), dev(k.noise, eng)
    sn = dev(k.sn, eng) if k.sn is not None else None
    cv = dev(cfg, eng) if isinstance(cfg, torch.Tensor) else cfg
    with torch.cuda.stream(eng.stream):
        eng.diffusion_sample(k.n, cd, nz, cv, out, step_noise=sn)
    eng.sync()
    return out.cpu()


GRID = [(n, so, xs) for xs in (1, 3) for so in SOLVERS for n in NS]
IDS = [f"n{n}-{so}-xs{xs}" for n, so, xs in GRID]


@pytest.mark.parametrize("n,solver,xs", GRID, ids=IDS)
def test_uniform_vector_equals_scalar(n, solver, xs):
    """1. n copies of c in the vector == the scalar c, bit for bit; at n = 1 in the bf16 mode the vector call runs the seam"""
    k, s = _case(n, solver), _small(xs)
    for c in (1.3, 0.0):
        a = _sample(s, k, c)
        b = _sample(s, k, torch.full((n,), c))
        if n == 1 and xs == 1:
            assert s.eng.stat(6) == N_STEPS - 1, s.eng.stat(6)
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, b), rel_err(b, a)


@pytest.mark.parametrize("n,solver,xs", GRID, ids=IDS)
def test_each_row_uses_its_own_scale(n, solver, xs):
    """2. row i of the mixed-vector call == row i of the scalar c[i] call on the same inputs, bit for bit (after the scalar call has
    been shown to reproduce itself run to run)."""
    k, s = _case(n, solver), _small(xs)
    one = _sample(s, k, float(k.c[0]))
    assert torch.equal(one, _sample(s, k, float(k.c[0]))), "this path does not reproduce itself run to run"
    mixed = _sample(s, k, k.c)
    for i in range(n):
        alone = one if i == 0 else _sample(s, k, float(k.c[i]))
        assert torch.equal(mixed[i], alone[i]), (i, rel_err(mixed[i], alone[i]))
    if n > 1:
        assert rel_err(mixed[1], one[1]) > 1e-2              # and the rows really saw different scales


@pytest.mark.parametrize("n,solver,xs", GRID, ids=IDS)
def test_mixed_vector_against_the_oracle(n, solver, xs):
    """3. the mixed vector against oracle.dpm.sample_speech_tokens(cfg_scale=c[:, None]) at the existing sampler tests' tolerances"""
    k, s = _case(n, solver), _small(xs)
    out = _sample(s, k, k.c)
    e = max(rel_err(out[i], k.ref[i]) for i in range(n))
    print(f"[cfg rows n={n} {solver} xsplit={xs}] worst row rel-L2 vs oracle {e:.3e} (bound {TOL[xs]:.0e})")
    assert e <= TOL[xs], e


# ------------------------------------------------------------------------------------------------ 4. one launch at a time
RMS_MOD, CFG_DPM = 2, 6
EPS = 1e-5


def _launch(eng, ops, n_cfg, N, K, cfg, cfg_rows, form):
    z = ops["z0"].to(eng.device).contiguous()
    x0p = ops["x00"].to(eng.device).contiguous()
    torch.cuda.synchronize()
    got = eng.gemv_case(ops["wp"], ops["x"], None, 2 * n_cfg, N, K, pro=RMS_MOD, epi=CFG_DPM, eps=EPS, xsplit=1, mod_scale=ops["sc"],
                        mod_shift=ops["sh"], ld_mod=K, z=z, x0p=x0p, coef=ops["coef"], cfg=cfg, n_cfg=n_cfg, sde_noise=ops["noise"],
                        cfg_rows=cfg_rows)
    torch.cuda.synchronize()
    assert got == form, (got, form)
    return z.cpu(), x0p.cpu()


@pytest.mark.parametrize("sde", [False, True], ids=["det", "sde"])
@pytest.mark.parametrize("n_cfg,form", [(1, (1, 4, 8, 0, 0)), (2, (1, 4, 8, 0, 0)), (3, (1, 16, 4, 0, 0)), (8, (1, 16, 4, 0, 0))],
                         ids=["decode-n1", "decode-n2", "wide-n3", "wide-n8"])
def test_one_gemv_launch_with_cfg_rows(n_cfg, form, sde):
    """Engine.gemv_case, RMS_MOD + CFG_DPM with cfg_rows set: the decode forms (2 and 4 rows) and the wide 16-row form, N = 20 (a
    partial 16-feature tile) and 64.  Row i of z (both halves) and of x0p equals the scalar launch with cfg = c[i], bit for bit; the
    scalar argument is ignored when the vector is present; rows of the other utterances are not those of the scalar launch.  Each row
    is also held to the fp64 reference of the launch (tests/gemv_ref.py, bf16-rounded operands) at 1e-4: fp32 accumulation over
    K = 100 products is ~K * 2^-24 = 6e-6 of the summed magnitudes, and z' subtracts near-equal terms (up to ~10 x) -- three orders
    below what a neighbour's scale would show (> 1e-1, the precondition)."""
    eng = _small(1).eng
    T = 2 * n_cfg
    for N, K in ((20, 100), (64, 100)):
        g = synth.Gen(4700 + N + n_cfg)
        w = g.normal((N, K), 1.0 / K ** 0.5)
        x, sc, sh = g.normal((T, K), 1.0, mat=False), g.normal((T, K), 0.3, mat=False), g.normal((T, K), 0.3, mat=False)
        z0 = g.normal((n_cfg, N), 1.0, mat=False)
        z0 = torch.cat([z0, z0])
        x00 = g.normal((n_cfg, N), 1.0, mat=False)
        noise = g.normal((n_cfg, N), 1.0, mat=False) if sde else None
        coef = torch.tensor([0.8, 0.6, 0.7, 0.45, -0.3, 0.25])
        c = torch.tensor(SCALES[:n_cfg])
        # precondition on the fp64 reference of this launch: row 0 under two of the scales differs by more than 1e-1
        acc = R.product(R.pro_rms_mod(x, None, sc, sh, EPS, 1), R.weights(w))
        za, _ = R.epi_cfg_dpm(acc, z0, x00, coef, 1.0, noise)
        zb, _ = R.epi_cfg_dpm(acc, z0, x00, coef, 3.0, noise)
        assert rel_err(za[0], zb[0]) > 1e-1, rel_err(za[0], zb[0])
        ops = dict(wp=eng.pack_matrix(w), x=dev(x, eng), sc=dev(sc, eng), sh=dev(sh, eng), z0=z0, x00=x00, coef=dev(coef, eng),
                   noise=dev(noise, eng) if sde else None)
        zm, xm = _launch(eng, ops, n_cfg, N, K, 77.0, dev(c, eng), form)         # 77: the scalar must not be read
        assert bool(torch.isfinite(zm).all() and torch.isfinite(xm).all())
        for i in range(n_cfg):
            zs, xs_ = _launch(eng, ops, n_cfg, N, K, float(c[i]), None, form)
            assert torch.equal(zm[i], zs[i]) and torch.equal(zm[n_cfg + i], zs[n_cfg + i]) and torch.equal(xm[i], xs_[i]), (N, i)
            assert rel_err(zm[i], R.epi_cfg_dpm(acc, z0, x00, coef, float(c[i]), noise)[0][i]) <= 1e-4
            for j in range(n_cfg):
                if j != i:
                    assert not torch.equal(zm[j], zs[j]), (N, i, j)


# ------------------------------------------------------------------------------------------------ 5. graph replay
def test_graph_replay_follows_the_buffer():
    """use_graph engine, n = 3, ONE vector tensor for every call.  The engine captures a key at its second sight (the first runs
    eagerly), so the buffer is overwritten after TWO calls -- by then the sampler graph is cached and vv_stat(1) has counted it;
    a third and a fourth call with new values in the same buffer must replay it (vv_stat(1) unchanged), hold no memset / memcpy node
    (vv_stat(5) == 0) and give, bit for bit, what an eager engine gives for the new values."""
    k = _case(3, "dpmsolver++")
    sg, se = _small(1, use_graph=True), _small(1)
    eng = sg.eng
    eng.set_num_steps(N_STEPS)
    cd, nz, out = dev(k.cond, eng), dev(k.noise, eng), eng.new(3, 64)
    vec = dev(k.c, eng)

    def call():
        with torch.cuda.stream(eng.stream):
            eng.diffusion_sample(3, cd, nz, vec, out)
        eng.sync()
        return out.cpu()
    g0 = eng.stat(1)
    first = call()
    assert torch.equal(call(), first)
    cached = eng.stat(1)
    assert cached == g0 + 1, (g0, cached)                      # the sampler graph, keyed by the vector's address
    assert torch.equal(first, _sample(se, k, k.c))
    for new in (torch.tensor([0.0, 1.3, 3.0]), torch.tensor([2.5, 2.5, 0.5])):
        with torch.cuda.stream(eng.stream):
            vec.copy_(new.to(eng.device), non_blocking=True)   # in place, on the engine stream
        got = call()
        assert eng.stat(1) == cached, (eng.stat(1), cached)
        assert eng.stat(5) == 0, eng.stat(5)
        assert torch.equal(got, _sample(se, k, new)), rel_err(got, _sample(se, k, new))
        assert rel_err(got[0], first[0]) > 1e-2                # the replay read the new values


def test_a_new_schedule_drops_the_cached_rows_graph():
    """use_graph engine, the same tensors throughout: two vector calls at 5 steps cache the sampler graph; a 10-step schedule (which
    also reallocates the per-step modulation buffers the captured launches point into) must drop it, so the next call samples 10 steps
    -- bit for bit what an eager engine gives at 10 steps -- and the call after that, captured anew, gives the same."""
    k = _case(3, "dpmsolver++")
    sg, se = _small(1, use_graph=True), _small(1)
    eng = sg.eng
    cd, nz, out, vec = dev(k.cond, eng), dev(k.noise, eng), eng.new(3, 64), dev(k.c, eng)

    def call():
        with torch.cuda.stream(eng.stream):
            eng.diffusion_sample(3, cd, nz, vec, out)
        eng.sync()
        return out.cpu()
    try:
        eng.set_num_steps(N_STEPS)
        five = call()
        assert torch.equal(call(), five)
        cached = eng.stat(1)
        eng.set_num_steps(2 * N_STEPS)
        dropped = eng.stat(1)
        assert dropped <= cached - 1, (dropped, cached)            # the rows graph went with the table it was captured against
        se.eng.set_num_steps(2 * N_STEPS)
        ecd, enz, eout, evec = dev(k.cond, se.eng), dev(k.noise, se.eng), se.eng.new(3, 64), dev(k.c, se.eng)
        with torch.cuda.stream(se.eng.stream):
            se.eng.diffusion_sample(3, ecd, enz, evec, eout)
        se.eng.sync()
        want = eout.cpu()
        # 10 steps and 5 steps are told apart: halving the step of a second-order solver moves the result by its discretisation
        # error, orders above fp32 rounding (~1e-6); a replay of the stale graph would return `five` exactly
        assert rel_err(want, five) > 1e-4, rel_err(want, five)
        ten = call()
        assert torch.equal(ten, want), rel_err(ten, want)
        assert torch.equal(call(), want) and eng.stat(1) == dropped + 1
        assert eng.stat(5) == 0, eng.stat(5)
    finally:
        eng.set_num_steps(N_STEPS)
        se.eng.set_num_steps(N_STEPS)


# ------------------------------------------------------------------------------------------------ 6. guard rails
def test_guard_rails_of_the_entry_point():
    """vv_diffusion_sample_rows refuses a null vector, n outside [1, 8], a stochastic table without step noise and a deterministic
    table with it: < 0, a message, nothing launched (the launch counter and the output buffer stay as they were)."""
    from vibevoice_amd.engine import EngineError
    s = _small(3)
    eng = s.eng
    k = _case(2, "sde-dpmsolver++")
    cd, nz, sn, vec = dev(k.cond, eng), dev(k.noise, eng), dev(k.sn, eng), dev(k.c, eng)
    big = eng.new(9)
    out = torch.full((9, 64), 12345.0, device=eng.device)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()

    def refused(n, step_noise, rows, word):
        before = eng.stat(0)
        rc = eng.lib.vv_diffusion_sample_rows(eng._ctx, eng._s, n, p(cd), p(nz), p(step_noise), p(rows), p(out))
        eng.sync()
        assert rc < 0 and word in eng._err(), (rc, eng._err())
        assert eng.stat(0) == before and bool((out == 12345.0).all())
    eng.set_num_steps(N_STEPS)
    good = eng.new(2, 64)
    with torch.cuda.stream(eng.stream):
        eng.diffusion_sample(2, cd, nz, vec, good)              # a valid call first: the launch counter is non-zero
    eng.sync()
    assert eng.stat(0) > 0
    refused(2, None, None, "null")
    refused(0, None, vec, "[1,8]")
    refused(9, None, big, "[1,8]")
    refused(2, sn, vec, "deterministic")
    with pytest.raises(EngineError, match="deterministic"):
        eng.diffusion_sample(2, cd, nz, vec, good, step_noise=sn)
    try:
        eng.set_num_steps(N_STEPS, algorithm_type="sde-dpmsolver++")
        refused(2, None, vec, "stochastic")
        refused(2, sn, None, "null")
    finally:
        eng.set_num_steps(N_STEPS)
    # the Python wrapper refuses a vector that is not n fp32 entries on the device before the library sees it
    for bad in (eng.new(3), eng.new(2, 1), torch.zeros(2), eng.new(2).double(), eng.new(4)[::2]):
        with pytest.raises(ValueError, match="cfg_scale"):
            eng.diffusion_sample(2, cd, nz, bad, good)


# ------------------------------------------------------------------------------------------------ 7. product
@pytest.fixture(scope="module")
def sm():
    s = build_small(synth.LMCfg(), xsplit=3, n_slots=2, max_ctx=512)
    yield s
    s.eng.close()


def _product(s):
    from test_gpu_generate import TOK
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfgd = {"decoder_config": {"max_position_embeddings": s.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, s.eng, model_dtype=torch.float32)
    m.set_speech_factors(s.scaling, s.bias)
    m.set_ddpm_inference_steps(5)
    tok = types.SimpleNamespace(speech_start_id=TOK.speech_start_id, speech_end_id=TOK.speech_end_id, speech_diffusion_id=TOK.speech_diffusion_id,
                                eos_token_id=TOK.eos_token_id, bos_token_id=None, pad_token_id=TOK.pad_token_id)
    return m, tok


def test_requests_carry_their_own_scale_through_the_queue(sm):
    """three forced-plan requests with cfg_scale 1.0, 1.3 and 3.0 through generate_continuous on 2 slots, each held to the oracle loop
    run on it alone under its own scale (sequences equal, waveform rel-L2 <= 1e-2: test_continuous_admission_on_the_engine's bound)"""
    from test_gpu_generate import TOK, _mk_requests
    scales = [1.0, 1.3, 3.0]
    reqs = [dict(r, cfg_scale=c) for r, c in zip(_mk_requests(sm, 3, 7), scales)]
    om = sm.oracle_model(kv_round_bf16=True)
    orc = lambda r, c: ogen.oracle_generate(om, TOK, r["input_ids"], r["attention_mask"], cfg_scale=c, num_steps=5,
                                            noise_fn=r["_noise_fn"], forced_tokens=[r["_forced_tokens"]])
    refs = [orc(r, c) for r, c in zip(reqs, scales)]
    other = orc(reqs[0], 3.0)
    assert rel_err(other[1][0][0], refs[0][1][0][0]) > 1e-1            # precondition: the scales are told apart at the waveform
    m, tok = _product(sm)
    outs = m.generate_continuous(reqs, tokenizer=tok, generation_config={"do_sample": False}, cfg_scale=7.0, max_concurrent=2)
    assert m.last_stats["max_in_flight"] == 2 and len(m.last_stats["admissions"]) == 3
    for o, (oseq, oaud, _) in zip(outs, refs):
        assert torch.equal(o.sequences.cpu(), oseq)
        assert rel_err(o.speech_outputs[0][0], oaud[0][0]) <= 1e-2, rel_err(o.speech_outputs[0][0], oaud[0][0])


def test_generate_takes_one_scale_per_row(sm):
    """generate() on a lock-step batch of 2 with cfg_scale=[1.0, 3.0]: row b against row b of the oracle's batch under c[b]"""
    from test_gpu_generate import D, E, S, TOK, X, make_inputs
    ids, mask, _, _, _ = make_inputs(sm, 2, False, 23)
    forced = [[D, D, D, E, S, D, D, X], [D, D, E, S, D, X]]
    bank = {}

    def noise_fn(step, n2):
        if (step, n2) not in bank:
            bank[(step, n2)] = synth.Gen(23000 + step).normal((n2, 64), 1.0, mat=False)
        return bank[(step, n2)]
    om = sm.oracle_model(kv_round_bf16=True)
    scales = [1.0, 3.0]
    refs = [ogen.oracle_generate(om, TOK, ids, mask, cfg_scale=c, num_steps=5, noise_fn=noise_fn, forced_tokens=forced) for c in scales]
    assert rel_err(refs[0][1][0][0], refs[1][1][0][0]) > 1e-1          # precondition: row 0 under the two scales
    m, tok = _product(sm)
    out = m.generate(input_ids=ids, attention_mask=mask, cfg_scale=scales, tokenizer=tok, generation_config={"do_sample": False},
                     _forced_tokens=forced, _noise_fn=noise_fn, show_progress_bar=False)
    for b in range(2):
        oseq, oaud, _ = refs[b]
        assert torch.equal(out.sequences.cpu()[b], oseq[b])
        assert out.speech_outputs[b].shape[-1] == oaud[b].shape[-1]
        assert rel_err(out.speech_outputs[b][0], oaud[b][0]) <= 1e-2, (b, rel_err(out.speech_outputs[b][0], oaud[b][0]))
