"""GPU parity of the solver-step seam (headtail.hip: vv_head_tail_kernel), the launch that ends every solver step but the last for
one utterance's two rows in the bf16 mode: final layer + CFG + DPM-Solver++ update + the next step's in-projection.

Every test proves that the seam ran: vv_stat(ctx, 6) counts the seam launches of the last recorded sampler body, n_steps - 1 here.
The widths reach the kernel's geometry (8 waves share the K = H range in kper = ceil(H / 256) k-tiles each; 4 feature tiles of 16 per
workgroup):

  H = 256   kper = 1
  H = 352   kper = 2, waves 6 and 7 have an empty K range (nk == 0), the last workgroup holds 2 of its 4 feature tiles
  H = 896   0.5B width: kper = 4, wave 7 idle
  H = 1536  1.5B width: the head's down projection is K-split (PARTS=1); also with 3 head layers, so that the other of the two
            part buffers (HL & 1) is the one the seam reads
  H = 3584  7B width: kper = 14
  H = 4096  kper == KMAX (16), the staging tile full

Both solvers (dpmsolver++ and sde-dpmsolver++ with its per-step noise) and 2, 3, 10 and 20 steps: an odd and an even number of seam
launches, so the final latent comes from either generation of the double-buffered state.  The FFN width of the head does not reach
the seam except through the K-split parts (1024 <= H <= 2048 with a down projection of >= 96 k-tiles), so 1536 keeps the 1.5B
ratio of 3 and the two widest heads use 0.5 to keep the CPU oracle to seconds.  The LM of these engines is one thin layer that no
test here runs."""
import itertools

import pytest
import torch

import synth
from oracle import dpm, head
from test_gpu_geometry import build_fast, dev
from test_gpu_shipped import row_err

pytestmark = pytest.mark.gpu

CFG_SCALE = 1.3
SOLVERS = ("dpmsolver++", "sde-dpmsolver++")
STEPS = (2, 3, 10, 20)
# (hidden, head layers, head FFN ratio)
GEOMS = [(256, 4, 3.0), (352, 4, 3.0), (896, 4, 3.0), (1536, 4, 3.0), (1536, 3, 3.0), (3584, 4, 0.5), (4096, 4, 0.5)]


def _lmcfg(H):
    # head_dim 64 x 2 heads: the LM geometry is free here, and 352 is no multiple of 64 (the engine takes heads * head_dim != hidden)
    return synth.LMCfg(hidden=H, layers=1, heads=2, kv_heads=1, inter=256, vocab=64, head_dim_override=64)


_cache = {}


def _small(geom, xsplit=1, use_graph=False):
    """one engine at a time: the previous one is closed when the geometry changes"""
    key = (geom, xsplit, use_graph)
    if key not in _cache:
        for s in _cache.values():
            s.eng.close()
        _cache.clear()
        H, hl, ratio = geom
        _cache[key] = build_fast(_lmcfg(H), xsplit=xsplit, use_graph=use_graph, n_slots=2, max_ctx=128, max_rows=16,
                                 head_layers=hl, head_ffn_ratio=ratio)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for s in _cache.values():
        s.eng.close()
    _cache.clear()


def _inputs(seed, H, n_steps):
    g = synth.Gen(seed)
    pos = g.normal((1, H), 1.0, mat=False)
    neg = g.normal((1, H), 1.0, mat=False)
    noise = g.normal((2, 64), 1.0, mat=False)
    step_noise = g.normal((n_steps, 2, 64), 1.0, mat=False)
    return pos, neg, noise, step_noise


def _oracle(s, pos, neg, noise, n_steps, solver, step_noise, bf16):
    hf = lambda a, t, c: head.head_forward(s.head_w, a, t, c, s.hc.layers, s.hc.eps, mfma_in_bf16=bf16)
    sde = solver == "sde-dpmsolver++"
    with torch.no_grad():
        return dpm.sample_speech_tokens(hf, pos, neg, CFG_SCALE, n_steps, noise, algorithm_type=solver,
                                        step_noise=step_noise if sde else None)


def _sample(s, n, cond, noise, n_steps, solver, step_noise):
    """cond [2n, H], noise [n, 64], step_noise [n_steps, n, 64] (used by the stochastic solver only), all on the host"""
    eng = s.eng
    eng.set_num_steps(n_steps, algorithm_type=solver)
    out = eng.new(n, 64)
    cd, nz = dev(cond, eng), dev(noise, eng)
    sn = dev(step_noise.contiguous(), eng) if solver == "sde-dpmsolver++" else None
    with torch.cuda.stream(eng.stream):
        eng.diffusion_sample(n, cd, nz, CFG_SCALE, out, step_noise=sn)
    eng.sync()
    return out.cpu()


CASES = [(g, so, n) for g, so, n in itertools.product(GEOMS, SOLVERS, STEPS)]


@pytest.mark.parametrize("geom,solver,n_steps", CASES, ids=[f"H{g[0]}-HL{g[1]}-{so}-{n}" for g, so, n in CASES])
def test_seam_against_the_bf16_input_oracle(geom, solver, n_steps):
    """One utterance through the sampler against the oracle sampler whose matrix-unit inputs are rounded to bf16 (what is left is
    summation order: the bound the 16-row sampler forms meet, 1e-2) and against the fp32 oracle (the bf16 mode's 5e-2).
    Measured worst row rel-L2 against the bf16-input oracle over both solvers and the four step counts: 2.7e-3 (256), 3.1e-3 (352),
    3.2e-3 (896), 3.0e-3 (1536, 4 and 3 layers), 4.4e-3 (3584), 3.4e-3 (4096); against the fp32 oracle at most 5.5e-3."""
    s = _small(geom)
    H = geom[0]
    pos, neg, noise, step_noise = _inputs(7000 + H + 10 * geom[1] + n_steps, H, n_steps)
    out = _sample(s, 1, torch.cat([pos, neg]), noise[:1], n_steps, solver, step_noise[:, :1])
    assert s.eng.stat(6) == n_steps - 1, (s.eng.stat(6), n_steps)
    e16 = row_err(out, _oracle(s, pos, neg, noise, n_steps, solver, step_noise, True))
    e32 = row_err(out, _oracle(s, pos, neg, noise, n_steps, solver, step_noise, False))
    print(f"[seam H={H} HL={geom[1]} {solver} n_steps={n_steps}] row rel-L2 vs bf16-input oracle {e16:.3e}, vs fp32 oracle {e32:.3e}")
    assert bool(torch.isfinite(out).all())
    assert e16 <= 1e-2, e16
    assert e32 <= 5e-2, e32


@pytest.mark.parametrize("geom", [(896, 4, 3.0), (1536, 4, 3.0)], ids=["H896", "H1536"])
def test_seam_against_the_two_launch_pair(geom):
    """The seam claims the arithmetic of the pair it replaces (the final layer as the folded-shift GEMV with the CFG + solver
    epilogue, then the in-projection): the same utterance twice (n = 2: 4 rows, no seam) against once (n = 1: the seam), on one
    engine, same cond, uncond, noise and step noise; both solvers, 4 input draws at 2 and 3 steps and one at 20.  The step counts
    keep the adaLN modulations in one launch form on both sides (the tile GEMM over all (step, row) pairs takes over above 32 of
    them: 2 / 3 steps = 4 / 6 pairs against 8 / 12, 20 steps = 40 against 80).
    The difference is summation order, and it comes in two sizes: 0 .. 6e-6 where no bf16 rounding point of the head (its operands
    are rounded at every matrix-unit input) lands on the other side of a rounding boundary, and 5e-4 .. 1.6e-3 where one does
    (measured over the 36 runs: 16 bit-identical, worst row rel-L2 1.6e-3).  The bf16-input oracle itself moves by 5e-4 .. 1e-3
    when only its in-projection output is perturbed by 1e-7 relative, so no two summation orders of this sampler agree closer than
    that at the latent.  Hence two bounds: every run within 4e-3 (2.5 x the measured worst), and at least one run per width closer
    than 1e-5 -- a systematic slip in the seam shows in EVERY run (measured smallest: 0 at both widths)."""
    s = _small(geom)
    H = geom[0]
    diffs = []
    for solver in SOLVERS:
        for n_steps in (2, 3, 20):
            for k in range(4 if n_steps < 20 else 1):
                pos, neg, noise, step_noise = _inputs(8000 + 100 * k + H + n_steps, H, n_steps)
                one = _sample(s, 1, torch.cat([pos, neg]), noise[:1], n_steps, solver, step_noise[:, :1])
                assert s.eng.stat(6) == n_steps - 1, (s.eng.stat(6), n_steps)
                two = _sample(s, 2, torch.cat([pos, pos, neg, neg]), noise[:1].repeat(2, 1), n_steps, solver,
                              step_noise[:, :1].repeat(1, 2, 1))
                assert s.eng.stat(6) == 0, s.eng.stat(6)                  # n = 2: the two-launch form
                d = max(row_err(two[0:1], one), row_err(two[1:2], one))
                print(f"[seam vs pair H={H} {solver} n_steps={n_steps} draw {k}] worst row rel-L2 {d:.3e}")
                diffs.append(d)
    assert max(diffs) <= 4e-3, max(diffs)
    assert min(diffs) <= 1e-5, min(diffs)


@pytest.mark.parametrize("solver", SOLVERS)
def test_seam_under_graph_replay(solver):
    """The timed mode replays the captured sampler graph, whose key holds the input pointers: sample (first sight: eager), sample
    again (captured), then overwrite cond, noise and step noise IN PLACE and replay -- the result must be the oracle's for the new
    inputs, and the replay keeps the seam count of its capture."""
    geom, n_steps = (1536, 4, 3.0), 10
    s = _small(geom, use_graph=True)
    eng, H = s.eng, geom[0]
    eng.set_num_steps(n_steps, algorithm_type=solver)
    sde = solver == "sde-dpmsolver++"
    a = _inputs(9100, H, n_steps)
    b = _inputs(9200, H, n_steps)
    cond, nz, sn = dev(torch.cat([a[0], a[1]]), eng), dev(a[2][:1], eng), dev(a[3][:, :1].contiguous(), eng)
    out = eng.new(1, 64)
    for _ in range(2):
        with torch.cuda.stream(eng.stream):
            eng.diffusion_sample(1, cond, nz, CFG_SCALE, out, step_noise=sn if sde else None)
        eng.sync()
    first = out.cpu()
    assert eng.stat(1) > 0 and eng.stat(6) == n_steps - 1, (eng.stat(1), eng.stat(6))
    assert row_err(first, _oracle(s, a[0], a[1], a[2], n_steps, solver, a[3], True)) <= 1e-2
    cond.copy_(torch.cat([b[0], b[1]]).to(eng.device))
    nz.copy_(b[2][:1].to(eng.device))
    sn.copy_(b[3][:, :1].to(eng.device))
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.stream):
        eng.diffusion_sample(1, cond, nz, CFG_SCALE, out, step_noise=sn if sde else None)
    eng.sync()
    second = out.cpu()
    assert eng.stat(6) == n_steps - 1, eng.stat(6)
    e = row_err(second, _oracle(s, b[0], b[1], b[2], n_steps, solver, b[3], True))
    print(f"[seam graph replay {solver}] new inputs: row rel-L2 vs bf16-input oracle {e:.3e}")
    assert e <= 1e-2, e
    assert row_err(second, first) > 1e-1                                 # the replay read the new inputs


@pytest.mark.parametrize("case", ["H128", "xsplit3", "n2", "n8"])
def test_seam_count_is_zero_where_the_two_launch_form_runs(case):
    """vv_stat(ctx, 6) counts seam launches only: none below H = 256 (vv_head_tail_ok), none in the exact modes, none for two or more
    utterances (the folded-shift GEMV and the 16-row forms) -- and the sampler still matches the oracle there."""
    n_steps = 10
    if case == "H128":
        from gpu_util import build_small
        for st in list(_cache.values()):
            st.eng.close()
        _cache.clear()
        s = build_small(synth.LMCfg(), xsplit=1, n_slots=2)
        _cache[("H128",)] = s
    else:
        s = _small((256, 4, 3.0), xsplit=3 if case == "xsplit3" else 1)
    H = s.hc.hidden
    n = {"n2": 2, "n8": 8}.get(case, 1)
    g = synth.Gen(9300 + n)
    pos = g.normal((n, H), 1.0, mat=False)
    neg = g.normal((n, H), 1.0, mat=False)
    noise = g.normal((2 * n, 64), 1.0, mat=False)
    out = _sample(s, n, torch.cat([pos, neg]), noise[:n], n_steps, "dpmsolver++", None)
    assert s.eng.stat(6) == 0, s.eng.stat(6)
    ref = _oracle(s, pos, neg, noise, n_steps, "dpmsolver++", None, False)
    assert row_err(out, ref) <= (2e-3 if case == "xsplit3" else 5e-2), row_err(out, ref)
