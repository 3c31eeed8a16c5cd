"""Plain fp64 reference of the batch-decode packed GEMV (csrc/gemv16p.hip: vv_gemv16p_kernel, vv_pack16_kernel,
vv_pack16_tiles_kernel), written from the definitions in the VVGemv16p comments (csrc/vv_common.h) -- not from the kernels.  The
products and epilogues are those of tests/gemv_ref.py (held to the oracle by tests/test_gemv_ref_cpu.py); this module adds only what
the packed kernel has of its own, and tests/test_gemv16p_ref_cpu.py ties each addition back to gemv_ref.

The packed 16-row activation tile.  Element (t, k) of a [16][K] tile is a bf16 at
    k-tile k >> 5 (1 KiB each),  lane (t & 15) + 16 * ((k & 31) >> 3) (16 bytes each),  slot k & 7 (2 bytes each)
-- the layout vv_common.h documents for a 16-row weight tile.  Rows >= T and columns >= K of the last k-tile are zero.

    Y[t][n] = epilogue( rs[t] * sum_k A[t][k] W[n][k]  +  sum_k S[t][k] W[n][k] )

  A, S     what the packed operands Xp / Xs hold (bf16, exact in fp64)
  RS       rs[t] = 1 / sqrt(sum_tiles ssq_in[tile][t] / K + eps) in fp64, from whatever partials the caller supplies; off: 1
  SH       the second operand's product is added UNSCALED: rs * W.A + W.S
  PK       besides Y: Yp = bf16((Y * pk_nw) * (1 + pk_sc)) formed in fp32, and ssq_out[tile][t] = sum of Y[t][n]^2 over the 16 features
           of the tile
"""
import torch

import gemv_ref as R

F64 = torch.float64


def tile_bytes(K):
    return ((K + 31) // 32) * 1024


def _index(K):
    """(k-tile, lane, slot) of every element (t, k) of a [16][K] tile"""
    t = torch.arange(16)[:, None]
    k = torch.arange(K)[None, :]
    return (k >> 5).expand(16, K), ((t & 15) + 16 * ((k & 31) >> 3)).expand(16, K), (k & 7).expand(16, K)


def pack16_tile(x16):
    """[T <= 16][K] floats -> the packed tile as uint8 [ceil(K / 32) * 1024]: every element rounded to the nearest bf16, rows >= T
    and the columns past K of the last k-tile zero"""
    T, K = x16.shape
    assert 1 <= T <= 16 and K >= 1
    full = torch.zeros(16, K, dtype=torch.bfloat16)
    full[:T] = x16.to(torch.float32).to(torch.bfloat16)
    out = torch.zeros((K + 31) // 32, 64, 8, dtype=torch.bfloat16)
    kt, lane, slot = _index(K)
    out[kt, lane, slot] = full
    return out.view(torch.uint8).reshape(-1).clone()


def unpack16_tile(raw, K):
    """the packed tile (uint8, at least ceil(K / 32) KiB) -> [16][K] fp32, exact"""
    n = tile_bytes(K)
    assert raw.dtype == torch.uint8 and raw.numel() >= n
    tiles = raw[:n].contiguous().view(torch.bfloat16).reshape(-1, 64, 8)
    kt, lane, slot = _index(K)
    return tiles[kt, lane, slot].to(torch.float32)


def unpack16_bits(raw, K):
    """the packed tile -> [16][K] int16: the bf16 bit patterns, for comparisons that must not go through a float"""
    n = tile_bytes(K)
    assert raw.dtype == torch.uint8 and raw.numel() >= n
    tiles = raw[:n].contiguous().view(torch.int16).reshape(-1, 64, 8)
    kt, lane, slot = _index(K)
    return tiles[kt, lane, slot]


def bf16_bits(v32):
    """fp32 -> nearest bf16 -> its bit pattern as int16"""
    return v32.to(torch.float32).to(torch.bfloat16).view(torch.int16)


def rs_from_partials(ssq_in, K, eps):
    """ssq_in [tiles][16] -> rs [16][1], fp64"""
    s = ssq_in.to(F64).reshape(-1, 16).sum(0)
    return (1.0 / torch.sqrt(s / K + eps))[:, None]


def operands(xp, K, T, ssq_in=None, eps=0.0, xs=None):
    """the (A, rs, S) triple of gemv_ref.product from the launch's packed operands: rows < T of Xp, the row scale (RS: ssq_in given)
    and rows < T of Xs (SH: xs given)"""
    A = unpack16_tile(xp, K)[:T].to(F64)
    rs = None if ssq_in is None else rs_from_partials(ssq_in, K, eps)[:T]
    S = None if xs is None else unpack16_tile(xs, K)[:T].to(F64)
    return A, rs, S


def ssq_partials(y):
    """y [T][N], N % 16 == 0 -> [N / 16][T]: each row's sum of squares over the 16 features of a tile, fp64"""
    T, N = y.shape
    assert N % 16 == 0
    return y.to(F64).pow(2).reshape(T, N // 16, 16).sum(-1).t().contiguous()


def pk_rows(y32, pk_nw=None, pk_sc=None):
    """PK's packed rows from the fp32 rows the launch stored: bf16((y * pk_nw) * (1 + pk_sc)), every step in fp32 (a missing factor
    is 1, which is exact) -> fp32 holding bf16 values"""
    assert y32.dtype == torch.float32
    v = y32 if pk_nw is None else y32 * pk_nw.to(torch.float32)
    if pk_sc is not None:
        v = v * (1.0 + pk_sc.to(torch.float32))
    return R.bf16r(v)


def pack16_value(x, nw, eps, sc=None, sh=None):
    """vv_pack16_kernel's value before the bf16 rounding, fp64: (main, shift) with v = main + shift, main = rs * x * nw * (1 + sc)"""
    x = x.to(F64)
    rs = 1.0 / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    main = rs * x
    if nw is not None:
        main = main * nw.to(F64)
    if sc is not None:
        main = main * (1.0 + sc.to(F64))
    shift = torch.zeros_like(main) if sh is None else sh.to(F64)
    return main, shift


def ulp_bf16(v):
    """the spacing of bf16 values at |v| (normal range)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().to(F64).clamp_min(2.0 ** -126))) - 7)
