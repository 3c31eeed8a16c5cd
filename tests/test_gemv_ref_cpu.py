"""tests/gemv_ref.py (the fp64 reference the GPU form tests of the decode GEMV compare with) held to the oracle, on the CPU: with
every rounding off, its prologues and epilogues chained the way the engine chains its launches reproduce the oracle's own
computation -- so the reference cannot inherit a mistake from the kernel it judges.  Agreement is to fp32 rounding: the oracle
computes in fp32, the reference in fp64; 2e-6 relative to the largest value is a few fp32 ulps over these short chains."""
import pytest
import torch

import gemv_ref as R
import synth
from oracle import codec, dpm, head
from vibevoice_amd import schedule

TOL = 2e-6


def _close(got, want, tol=TOL):
    got, want = got.to(torch.float64), want.to(torch.float64)
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= tol, err


def test_head_layer_matches_oracle():
    """noisy / cond projections (NONE + STORE), adaLN (ADD_SILU + STORE: silu(cond_proj + t) . W), one layer
    (RMS_MOD + SWIGLU, then NONE + GATED_RESID) and the final layer (RMS_MOD + STORE without affine) = head_forward(n_layers=1)"""
    hc = synth.HeadCfg(hidden=64, layers=1)
    w = synth.head_weights(hc)
    g = synth.Gen(11)
    n, H = 4, hc.hidden
    noisy, cond = g.normal((n, hc.latent), 1.0, mat=False), g.normal((n, H), 1.0, mat=False)
    t = torch.tensor([999.0, 500.0, 37.0, 1.0])
    want = head.head_forward(w, noisy, t, cond, 1, eps=hc.eps)

    W = lambda k: R.weights(w[k], None)
    x = R.product(R.pro_none(noisy, None), W("noisy_images_proj.weight"))
    tf = head.timestep_embedding(t)
    t1 = R.product(R.pro_none(tf, None), W("t_embedder.mlp.0.weight"))
    temb = R.product(R.pro_add_silu(t1.float(), torch.zeros(1, H), n, None), W("t_embedder.mlp.2.weight"))
    c = R.product(R.pro_none(cond, None), W("cond_proj.weight"))
    # rows t of c, one add-vector per row: the batched adaLN mapping with x_row_mod = n, add_rows_per_vec = 1
    mod = R.product(R.pro_add_silu(c.float(), temb.float(), n, None, x_row_mod=n, add_rows_per_vec=1), W("layers.0.adaLN_modulation.1.weight"))
    shift, scale, gate = mod.float().chunk(3, -1)
    pro = R.pro_rms_mod(x.float(), w["layers.0.norm.weight"], scale, shift, hc.eps, None)
    u = R.epi_swiglu(R.product(pro, W("layers.0.ffn.gate_proj.weight")), R.product(pro, W("layers.0.ffn.up_proj.weight")))
    x = R.epi_gated_resid(R.product(R.pro_none(u.float(), None), W("layers.0.ffn.down_proj.weight")), x, gate)
    mod = R.product(R.pro_add_silu(c.float(), temb.float(), n, None, x_row_mod=n, add_rows_per_vec=1), W("final_layer.adaLN_modulation.1.weight"))
    shift, scale = mod.float().chunk(2, -1)
    got = R.epi_store(R.product(R.pro_rms_mod(x.float(), None, scale, shift, hc.eps, None), W("final_layer.linear.weight")))
    _close(got, want, 2e-5)      # five chained GEMMs whose intermediates pass through fp32 on both sides


@pytest.mark.parametrize("algo", schedule.ALGORITHMS)
def test_cfg_dpm_step_matches_oracle(algo):
    """every step of a 5-step trajectory (first-order first and last steps, second-order in between): CFG of the two halves of a
    model output + one scheduler.step() of oracle/dpm.py = epi_cfg_dpm with that step's row of schedule.make_table"""
    n_steps, n, N, cfg = 5, 3, 8, 1.3
    _, coef = schedule.make_table(n_steps, algorithm_type=algo)
    coef = torch.from_numpy(coef)
    if coef.shape[1] == 5:
        coef = torch.cat([coef, torch.zeros(n_steps, 1)], 1)
    g = synth.Gen(5)
    st = dpm.DPMState(dpm.Schedule(n_steps), algo)
    speech = g.normal((2 * n, N), 1.0, mat=False)
    speech[n:] = speech[:n]
    x0p = torch.zeros(n, N)
    for i in range(n_steps):
        eps = g.normal((2 * n, N), 1.0, mat=False)
        noise = g.normal((2 * n, N), 1.0, mat=False) if algo != "dpmsolver++" else None
        half = eps[n:] + cfg * (eps[:n] - eps[n:])
        want = st.step(torch.cat([half, half], 0), speech, noise)
        z, x0 = R.epi_cfg_dpm(eps.double(), speech, x0p, coef[i], cfg, noise)
        # the stochastic solver draws noise for both halves and only the first half reaches the next step (speech[:n]); the
        # oracle's fp32 update subtracts near-equal terms: 1e-5 of the largest value is ~100 ulps
        _close(z[:n], want[:n], 1e-5)
        _close(x0, st.model_outputs[1][:n], 1e-5)
        assert torch.equal(z[:n], z[n:])
        speech = torch.cat([want[:n], want[:n]], 0)
        x0p = st.model_outputs[1][:n].clone()


def test_block1d_streaming_step_matches_oracle():
    """NORMDW + BIAS_GELU (norm, causal depthwise conv over the six cached normed rows and the new one, layer scale, residual,
    FFN norm, linear1, GELU), then NONE + RESID (linear2, bias, layer scale, residual) = one streaming step of oracle block1d; the
    prologue's two side outputs are the block's mid residual and the conv cache's new column"""
    C, eps, p = 48, 1e-5, "b."
    w = {}
    synth._block_weights(synth.Gen(9), w, p, C)
    g = synth.Gen(10)
    state = {}
    for _ in range(7):                     # fill the conv cache with real history
        codec.block1d(g.normal((1, C, 1), 1.0, mat=False), w, p, state, eps)
    hist = state[p + "mixer"][0].t().contiguous()           # [6][C], oldest first
    x = g.normal((1, C, 1), 1.0, mat=False)
    want = codec.block1d(x, w, p, state, eps)[0, :, 0]
    taps = w[p + "mixer.conv.conv.conv.weight"][:, 0, :].t().contiguous()       # [7][C]
    pro, xo, h = R.pro_normdw(x[0, :, 0][None], w[p + "ffn_norm.weight"], eps, None, hist, taps, w[p + "mixer.conv.conv.conv.bias"],
                              w[p + "gamma"], w[p + "norm.weight"])
    u = R.epi_bias_gelu(R.product(pro, R.weights(w[p + "ffn.linear1.weight"], None)), w[p + "ffn.linear1.bias"])
    got = R.epi_resid(R.product(R.pro_none(u.float(), None), R.weights(w[p + "ffn.linear2.weight"], None)), xo,
                      w[p + "ffn.linear2.bias"], w[p + "ffn_gamma"])
    _close(got[0], want, 1e-5)
    _close(h[0], state[p + "mixer"][0, :, -1])
    assert state[p + "mixer"].shape[-1] == 6


def test_rounding_points_and_split():
    """xs = 1 rounds the staged operand, xs = 2 / 3 and None do not; the K-split columns tile K exactly and sum to the whole"""
    g = synth.Gen(3)
    x, nw = g.normal((2, 100), 1.0, mat=False), g.vec(100, 0.1, 1.0)
    a1, rs, _ = R.pro_rms(x, nw, 1e-5, 1)
    a3, rs3, _ = R.pro_rms(x, nw, 1e-5, 3)
    assert torch.equal(a1, R.bf16r(x * nw).double()) and torch.equal(a3, (x * nw).double()) and torch.equal(rs, rs3)
    _close(rs, torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + 1e-5), 1e-12)
    assert R.ksplit_ranges(64, 3) == [(0, 32), (32, 64), (64, 64)]
    assert R.ksplit_ranges(3076, 3) == [(0, 1056), (1056, 2112), (2112, 3076)]
    W = R.weights(g.linear(8, 100))
    pro = R.pro_none(x, 1)
    y = g.normal((2, 8), 1.0, mat=False)
    b, sc = g.vec(8), g.uniform((8,), 0.5, 1.5)
    out, parts = R.ksplit_producer(pro, W, 3, y, bias=b, nscale=sc)
    _close(out + parts[0] + parts[1], R.epi_resid(R.product(pro, W), y, b, sc), 1e-12)
    _close(parts[0], sc.double() * R.product(pro, W, 64, 100), 1e-12)
    assert float(parts[1].abs().max()) == 0.0          # 4 k-tiles in chunks of 2: the third column is empty
