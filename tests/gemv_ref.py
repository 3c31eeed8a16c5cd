"""Plain fp64 reference of the decode GEMV's operations (csrc/gemv.hip: vv_gemv_kernel), one function per prologue and one per
epilogue, written from the definitions in the VVGemm comments (csrc/vv_common.h) and the formulas of oracle/ -- not from the kernel.
tests/test_gemv_ref_cpu.py ties it to the oracle (head layer, solver step, Block1D streaming step) so that it cannot inherit a
kernel's mistake.

    Y[t][n] = epilogue( rs[t] * sum_k A[t][k] W[n][k]  +  sum_k S[t][k] W[n][k] )

A prologue returns (A, rs, S): the staged operand, the row scale 1/rms (None = 1) and the second, unscaled operand (None = absent).

Rounding points (`xs` is the activation precision of the launch: 1 = bf16 inside the matrix unit, 2 / 3 = split operands that carry
the fp32 value, None = nothing rounded, weights included -- the form the CPU test compares with the fp32 oracle):

  weights   rounded to bf16, as vv_pack_matrix stores them
  NONE      A = x; xs = 1: bf16(x)
  RMS       A = x * nw formed in fp32; xs = 1: bf16(x * nw).  rs = 1 / sqrt(mean(x^2) + eps) in fp64 from the UNROUNDED row; the
            product is scaled by rs afterwards
  RMS_MOD   A = (x * nw) * (1 + scale) formed in fp32; xs = 1: bf16 of it.  S = shift; xs = 1: bf16(shift); its product is added
            UNSCALED:  y = rs * W.A + W.S
  ADD_SILU  output row t reads activation row t % x_row_mod and add-vector t // add_rows_per_vec (0 = off: row t, vector 0):
            A = silu(x + addvec) (fp64, then fp32); xs = 1: bf16 of it
  NORMDW    one row, Block1D up to FFN1:  h = x / rms(x) * dw_nw;  xo = x + dw_gamma * (dw_b + sum_{j<6} dw_w[j] * dw_hist[j] +
            dw_w[6] * h);  A = xo * nw formed in fp32 (xs = 1: bf16), rs = 1 / rms(xo).  xo (dw_xout) and h (dw_hnew) are outputs
            too, in fp64.
  products, 1/rms and every epilogue: fp64.  Part tensors of a K split are added in fp32 in the order (base + part0) + part1.
"""
import math

import torch

F64 = torch.float64


def bf16r(t):
    """fp32 -> nearest bf16 -> fp32"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def weights(w, xs=1):
    """the matrix as the packed tiles hold it (bf16), in fp64; xs = None: unrounded"""
    return (w.to(torch.float32) if xs is None else bf16r(w)).to(F64)


def _stage(a32, xs):
    assert a32.dtype == torch.float32
    return (bf16r(a32) if xs == 1 else a32).to(F64)


def _rs(x, eps):
    x = x.to(F64)
    return 1.0 / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def add_parts(base, p0, p1):
    """a K-split tensor read back: (base + part0) + part1 in fp32, in that order"""
    return (base.to(torch.float32) + p0.to(torch.float32)) + p1.to(torch.float32)


# ---------------------------------------------------------------------------------------------- prologues -> (A, rs, S)
def pro_none(x, xs):
    return _stage(x.to(torch.float32), xs), None, None


def pro_rms(x, nw, eps, xs):
    x = x.to(torch.float32)
    a = x if nw is None else x * nw.to(torch.float32)
    return _stage(a, xs), _rs(x, eps), None


def pro_rms_mod(x, nw, scale, shift, eps, xs):
    x = x.to(torch.float32)
    a = x if nw is None else x * nw.to(torch.float32)
    a = a * (1.0 + scale.to(torch.float32))
    return _stage(a, xs), _rs(x, eps), _stage(shift.to(torch.float32), xs)


def pro_add_silu(x, addvec, T, xs, x_row_mod=0, add_rows_per_vec=0):
    """x [rows][K], addvec [vectors][K] -> staged [T][K]"""
    t = torch.arange(T)
    xi = t % x_row_mod if x_row_mod > 0 else t
    vi = t // add_rows_per_vec if add_rows_per_vec > 0 else torch.zeros_like(t)
    addvec = addvec.reshape(-1, x.shape[-1])
    u = x.to(F64)[xi] + addvec.to(F64)[vi]
    a = u / (1.0 + torch.exp(-u))
    return _stage(a.to(torch.float32), xs), None, None


def pro_normdw(x, nw, eps, xs, dw_hist, dw_w, dw_b, dw_gamma, dw_nw):
    """x [1][K]; dw_hist [6][K] oldest first; dw_w [7][K] taps, the last one on the new row.  -> (A, rs, S), xo [1][K], h [1][K]"""
    x64 = x.to(F64).reshape(1, -1)
    h = x64 * _rs(x64, eps) * dw_nw.to(F64)
    conv = dw_b.to(F64) + (dw_w.to(F64)[:6] * dw_hist.to(F64)).sum(0) + dw_w.to(F64)[6] * h
    xo = x64 + dw_gamma.to(F64) * conv
    a = xo.to(torch.float32)
    if nw is not None:
        a = a * nw.to(torch.float32)
    return (_stage(a, xs), _rs(xo, eps), None), xo, h


def product(pro, W, k0=0, k1=None):
    """rs * A.W^T + S.W^T over columns [k0, k1) of K, fp64.  W from weights()."""
    A, rs, S = pro
    k1 = A.shape[-1] if k1 is None else k1
    acc = A[:, k0:k1] @ W[:, k0:k1].t()
    if rs is not None:
        acc = rs * acc
    if S is not None:
        acc = acc + S[:, k0:k1] @ W[:, k0:k1].t()
    return acc


# ---------------------------------------------------------------------------------------------- epilogues (fp64)
def epi_store(acc):
    return acc


def epi_bias(acc, bias=None):
    return acc if bias is None else acc + bias.to(F64)


def epi_bias_gelu(acc, bias=None):
    u = epi_bias(acc, bias)
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def epi_swiglu(acc_gate, acc_up):
    return acc_gate / (1.0 + torch.exp(-acc_gate)) * acc_up


def epi_resid(acc, y, bias=None, nscale=None):
    """y + nscale * (acc + bias)"""
    u = epi_bias(acc, bias)
    return y.to(F64) + (u if nscale is None else nscale.to(F64) * u)


def epi_gated_resid(acc, y, gate):
    """y + gate * acc, gate per row and feature"""
    return y.to(F64) + gate.to(F64) * acc


def epi_cfg_dpm(acc, z, x0p, coef, cfg, sde_noise=None):
    """acc [2n][N]: rows [0, n) conditional, [n, 2n) unconditional model outputs.  z [2n][N] noisy latent, x0p [n][N] previous x0
    prediction, coef = {a, s, cs, c0, c1, cn}.  CFG, v-prediction -> x0, then the DPM-Solver++ update (vibevoice_amd/schedule.py):
        v = uncond + cfg * (cond - uncond);  x0 = a * z - s * v;  z' = cs * z + c0 * x0 + c1 * (x0 - x0p) [+ cn * noise]
    -> (z' written to both halves [2n][N], x0 [n][N])"""
    n = acc.shape[0] // 2
    a, s, cs, c0, c1, cn = (float(c) for c in coef.to(F64)[:6])
    cond, unc = acc[:n], acc[n:2 * n]
    v = unc + float(cfg) * (cond - unc)
    zo = z.to(F64)[:n]
    x0 = a * zo - s * v
    zn = cs * zo + c0 * x0 + c1 * (x0 - x0p.to(F64)[:n])
    if sde_noise is not None:
        zn = zn + cn * sde_noise.to(F64)[:n]
    return torch.cat([zn, zn], 0), x0


# ---------------------------------------------------------------------------------------------- K split over workgroup columns
def ksplit_ranges(K, kgrid):
    """column c of a kgrid-way split owns the 32-wide k-tiles [c * chunk, (c + 1) * chunk), chunk = ceil(k_tiles / kgrid); a column
    past the end is empty"""
    k_tiles = (K + 31) // 32
    chunk = (k_tiles + kgrid - 1) // kgrid
    return [(min(K, c * chunk * 32), min(K, (c + 1) * chunk * 32)) for c in range(kgrid)]


def ksplit_producer(pro, W, kgrid, y, bias=None, nscale=None, gate=None):
    """-> (Y, [part_1, ..]): column 0 writes the epilogue result of its own K range (residual, bias and scale), columns 1.. write
    scale * partial with no bias and no residual.  gate given: the gated residual, else the plain residual."""
    rng = ksplit_ranges(pro[0].shape[-1], kgrid)
    acc0 = product(pro, W, *rng[0])
    if gate is not None:
        out = epi_gated_resid(acc0, y, gate)
        scale = gate.to(F64)
    else:
        out = epi_resid(acc0, y, bias, nscale)
        scale = 1.0 if nscale is None else nscale.to(F64)
    return out, [scale * product(pro, W, *r) for r in rng[1:]]
