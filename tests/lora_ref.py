"""fp64 references for the LoRA merge (tests only): W' = W + scale * B @ A in both of lora.merge_lora's modes, the correctly
rounded bf16 value of an fp64 tensor, and the comparison "the two bf16 values are equal or adjacent"."""
import numpy as np
import torch


def merge_fp64(w: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale: float, merge_dtype: str = "float32") -> torch.Tensor:
    """The merged matrix in fp64, before its final rounding to bf16.  "bfloat16": the factors and the delta are rounded to bf16
    first, as the mode defines them (the delta's rounding is the correctly rounded one of the fp64 product)."""
    if merge_dtype == "bfloat16":
        a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
        delta = rne_bf16(b.double() @ a.double() * float(scale)).double()
    else:
        delta = b.double() @ a.double() * float(scale)
    return w.double() + delta


def rne_bf16(x64: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16, round to nearest even in ONE step (through fp32 it would round twice).  Normal range only."""
    m, e = torch.frexp(x64.double())                     # x = m * 2^e, 0.5 <= |m| < 1: 8 significant bits = m * 256 an integer
    q = torch.round(m * 256.0) / 256.0                   # torch.round: half to even
    return torch.ldexp(q, e).to(torch.bfloat16)          # exact: the value is a bf16 number


def bf16_ordinal(t: torch.Tensor) -> torch.Tensor:
    """bf16 values as integers that count representable numbers in order (+0 and -0 share 0)"""
    assert t.dtype == torch.bfloat16
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def equal_or_adjacent(got: torch.Tensor, ref: torch.Tensor):
    """(all elements equal or adjacent bf16 values, share of elements that differ)"""
    d = (bf16_ordinal(got.cpu()) - bf16_ordinal(ref.cpu())).abs()
    return bool((d <= 1).all()), float((d != 0).double().mean())


def exact_case(N, K, r, seed, scale_i=0):
    """Inputs on which every product and partial sum of the merge is exact in fp32, in any order: a, b integers in [-16, 16] / 8,
    scale from {0.5, 2.0, 4.0}, W ~ N(0, 0.02^2) rounded to bf16."""
    g = np.random.default_rng(seed)
    w = torch.from_numpy((g.standard_normal((N, K), dtype=np.float32) * np.float32(0.02))).to(torch.bfloat16)
    a = torch.from_numpy(g.integers(-16, 17, (r, K)).astype(np.float32) / 8.0)
    b = torch.from_numpy(g.integers(-16, 17, (N, r)).astype(np.float32) / 8.0)
    return w, a, b, (0.5, 2.0, 4.0)[scale_i % 3]


def gaussian_case(N, K, r, seed):
    """W ~ N(0, 0.02^2) rounded to bf16, a and b ~ N(0, 0.02^2) fp32, scale 4 -- minus the deep cancellations.  Where W + delta
    nearly cancels, NO fp32 evaluation of the merge can promise the correctly rounded bf16 value or its neighbour: the fp32 error of
    the delta, at most E = (2r + 4) * 2^-24 * scale * sum_j |b_nj| |a_jk| for any summation order, fused or not, plus the add's
    2^-24 |W + delta|, has to stay below one bf16 step of the result, >= 2^-8 |W + delta|.  That holds wherever
    |W + delta| >= 2^8 * E; the few elements below it (a share of a few 1e-3 at r = 64) get W = +-0.02 with the delta's sign, so
    every element of the returned case satisfies it.  A property of the inputs alone, decided in fp64.
    Returns (w bf16, a, b, scale, share of elements replaced)."""
    g = np.random.default_rng(seed)
    w = torch.from_numpy((g.standard_normal((N, K), dtype=np.float32) * np.float32(0.02))).to(torch.bfloat16)
    a = torch.from_numpy(g.standard_normal((r, K), dtype=np.float32) * np.float32(0.02))
    b = torch.from_numpy(g.standard_normal((N, r), dtype=np.float32) * np.float32(0.02))
    scale = 4.0
    delta = b.double() @ a.double() * scale
    thr = (2 * r + 4) * 2.0 ** -16 * scale * (b.double().abs() @ a.double().abs())
    deep = (w.double() + delta).abs() < thr
    side = torch.where(delta >= 0, torch.tensor(0.02), torch.tensor(-0.02)).to(torch.bfloat16)
    w = torch.where(deep, side, w)
    assert bool(((w.double() + delta).abs() >= thr).all())
    return w, a, b, scale, float(deep.double().mean())
