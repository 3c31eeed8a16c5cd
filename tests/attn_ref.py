"""Plain fp64 reference of one attention launch of the LM pass (csrc/attn.hip, the attention of csrc/prefill.hip), per (row, head),
written from the definitions (oracle/lm.py: rotate-half RoPE, softmax(q k^T / sqrt(d)) v over a GQA cache) -- not from the kernels.
tests/test_attn_ref_cpu.py ties it to the oracle so that it cannot inherit a kernel's mistake.  CPU only, no engine import.

Rounding points (`xs` is the activation precision of the engine, `family` the kernel family of the launch):

  K, V      bf16 values, as the cache holds them (the GPU tests read them back with vv_kv_export: what a pass appended is an input)
  RoPE      the angle is the fp32 product float(pos) * inv_freq[i], as the kernels and the reference model form it; cos, sin and the
            rotation are fp64
  q         xs = 3: unrounded.  xs = 2: the two-term bf16 split of fp32(q / sqrt(D)).  xs = 1, "fused" and "split": bf16(fp32(q /
            sqrt(D))).  xs = 1, "prefill4": bf16(fp32(fp32(q / sqrt(D)) * log2(e))) -- the kernel works in the log2 domain; q_operand
            returns the operand back in natural units (times ln 2, in fp64)
  P         NOT rounded: its rounding (and that of the o-projection's operand) is what the GPU bounds measure
  scores, softmax, P.V: fp64

Errors are normalised by a[d] = sum_i p_i |v_id| / sum_i p_i, the scale of the terms the output is summed from: ||ref|| itself
cancels to about 1 / sqrt(L) of that under a flat softmax, and a correctly rounded bf16 P would look wrong against it."""
import math

import torch

F64 = torch.float64
LN2 = math.log(2.0)
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32)
STAGE = 64              # positions per stage of vv_attn_prefill4
REBASE_LOG2 = 8.0       # its lazy-rescale threshold, log2 units


def bf16r(t):
    """fp32 -> nearest bf16 -> fp32"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def inv_freq(D, theta):
    """HF Qwen2RotaryEmbedding's fp32 table"""
    return 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))


def rope(x, pos, invf):
    """x [T, heads, D] -> rotate-half RoPE at positions pos [T], fp64; the angle alone is formed in fp32"""
    ang = (torch.as_tensor(pos).to(torch.float32)[:, None] * invf.to(torch.float32)[None, :]).to(F64)
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos()[:, None, :], emb.sin()[:, None, :]
    x = x.to(F64)
    half = x.shape[-1] // 2
    rot = torch.cat([-x[..., half:], x[..., :half]], -1)
    return x * cos + rot * sin


def q_scaled32(q):
    """fp32(q / sqrt(D)) with the kernels' fp32 scale 1.0f / sqrtf(D): the operand before the mode's rounding"""
    scale = (1.0 / torch.sqrt(torch.tensor(float(q.shape[-1]), dtype=torch.float32))).to(F64)
    return (q.to(F64) * scale).to(torch.float32)


def q_prerounding(q, xs, family):
    """the fp32 value the mode rounds to bf16 (xs = 1), per element; what test (2d) measures the boundary distance of"""
    s = q_scaled32(q)
    return s * LOG2E_F32 if (xs == 1 and family == "prefill4") else s


def q_operand(q, xs, family):
    """rotated q [T, heads, D] -> the score operand in fp64, natural units, 1 / sqrt(D) included"""
    assert family in ("fused", "split", "prefill4") and xs in (1, 2, 3)
    if xs == 3:
        scale = (1.0 / torch.sqrt(torch.tensor(float(q.shape[-1]), dtype=torch.float32))).to(F64)
        return q.to(F64) * scale
    s = q_scaled32(q)
    if xs == 2:
        hi = bf16r(s)
        return hi.to(F64) + bf16r(s - hi).to(F64)
    if family == "prefill4":
        return bf16r(s * LOG2E_F32).to(F64) * LN2
    return bf16r(s).to(F64)


def scores(qop, k, limit, kv_of_head=None):
    """qop [T, Hq, D] (q_operand), k [Hkv, L, D], limit [T] = visible positions of each row ([0, limit)) -> [T, Hq, L] fp64,
    -inf at and past the limit.  kv_of_head: the kv head of every query head (default h // G)"""
    T, Hq, _ = qop.shape
    Hkv, L, _ = k.shape
    if kv_of_head is None:          # head h reads kv head h // G: one product per kv head, K is not copied once per query head
        s = torch.einsum("tkgd,kld->tkgl", qop.to(F64).reshape(T, Hkv, Hq // Hkv, -1), k.to(F64)).reshape(T, Hq, L)
    else:
        s = torch.einsum("thd,hld->thl", qop.to(F64), k.to(F64)[torch.as_tensor(kv_of_head)])
    hidden = torch.arange(L)[None, :] >= torch.as_tensor(limit)[:, None]
    return s.masked_fill(hidden[:, None, :], float("-inf"))


def softmax_v(s, v, kv_of_head=None):
    """s [T, Hq, L] (-inf = excluded), v [Hkv, L, D] -> (out, a, p): out = softmax(s) v, a = softmax(s) |v|, p the weights"""
    T, Hq, L = s.shape
    Hkv = v.shape[0]
    p = torch.softmax(s, -1)
    v = v.to(F64)
    if kv_of_head is None:
        pg = p.reshape(T, Hkv, Hq // Hkv, L)
        return (torch.einsum("tkgl,kld->tkgd", pg, v).reshape(T, Hq, -1), torch.einsum("tkgl,kld->tkgd", pg, v.abs()).reshape(T, Hq, -1), p)
    v = v[torch.as_tensor(kv_of_head)]
    return torch.einsum("thl,hld->thd", p, v), torch.einsum("thl,hld->thd", p, v.abs()), p


def attend(qop, k, v, limit, kv_of_head=None):
    """-> (out [T, Hq, D], a [T, Hq, D]) of rows that see positions [0, limit[t]) of the bf16-valued cache k, v [Hkv, L, D]"""
    n = int(torch.as_tensor(limit).max())                # slots at and past every limit may hold anything (NaN): never read
    out, a, _ = softmax_v(scores(qop, k[:, :n], limit, kv_of_head), v[:, :n], kv_of_head)
    return out, a


def row_head_errs(got, ref, a):
    """got, ref, a [T, Hq, D] -> (rel [T, Hq], mx [T, Hq]): ||got - ref||_2 / ||a||_2 and max |got - ref| / max a"""
    d = got.to(F64) - ref.to(F64)
    return d.norm(dim=-1) / a.norm(dim=-1).clamp_min(1e-300), d.abs().amax(-1) / a.amax(-1).clamp_min(1e-300)


def bf16_ulps(a, b):
    """bf16 tensors -> their distance in bf16 steps, per element (adjacent representable values are 1 apart, +0 and -0 are 0 apart)"""
    def order(t):
        i = t.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (order(a) - order(b)).abs()


CANCELLED = 2.0 ** -14


def rotated_k_steps(got, ref, src):
    """A rotated K against the fp64 rotation ref of src, both [.., D]: got bf16 (or fp32 about to be rounded), -> (steps, flat):
    steps = per-element distance in bf16 steps between bf16(got) and bf16(ref);  flat = the mask of CANCELLED elements, which are
    judged apart: where x cos - x' sin cancels to below 2^-14 of the pair's length |(x, x')| a bf16 step of the result is below
    2^-22 of the operands, which no fp32 rotation resolves (one fp32 rounding of a product is 2^-24 of it) -- there the distance
    is counted as 0 when |got - ref| <= 2^-22 |(x, x')| and as 99 otherwise.  2 * 2^-14 / pi = 3.9e-5 of all angles land there."""
    half = src.shape[-1] // 2
    s = src.to(F64)
    mag = torch.sqrt(s[..., :half] ** 2 + s[..., half:] ** 2)
    mag = torch.cat([mag, mag], -1)
    ref = ref.to(F64)
    flat = ref.abs() < CANCELLED * mag
    steps = bf16_ulps(got.to(torch.float32).to(torch.bfloat16), ref.to(torch.float32).to(torch.bfloat16))
    ok = (got.to(F64) - ref).abs() <= 2.0 ** -22 * mag
    return torch.where(flat, torch.where(ok, 0, 99), steps), flat


def bf16_boundary_distance(v32):
    """fp32 values -> the relative distance of each from the nearest bf16 rounding boundary (the midpoint of two adjacent bf16 values)"""
    bits = v32.to(torch.float32).contiguous().view(torch.int32).to(torch.int64)
    frac = (bits & 0xFFFF).to(F64) / 65536.0                       # position between the two neighbouring bf16 values
    ulp = torch.pow(2.0, torch.floor(torch.log2(v32.to(F64).abs())) - 7)
    return (frac - 0.5).abs() * ulp / v32.to(F64).abs()


# ---------------------------------------------------------------------------------------------- diagnostics
def rebase_stages(s_row):
    """The lazy-rescale rule of vv_attn_prefill4 replayed on one (row, head)'s fp64 scores s_row [L] (natural units, -inf = hidden):
    m = the maximum of stage 0 (positions [0, 64)), raised to a later stage's maximum when that exceeds m by more than 8 in log2
    units.  -> the list of stages (>= 1) at which m moves."""
    s2 = s_row.to(F64) / LN2
    L = s2.shape[0]
    m = float(s2[:STAGE].max())
    out = []
    for st in range(1, (L + STAGE - 1) // STAGE):
        mx = float(s2[st * STAGE:(st + 1) * STAGE].max())
        if mx - m > REBASE_LOG2:
            out.append(st)
            m = mx
    return out


def clip_never_rebased(s):
    """scores [.., L] as a kernel that never re-bases would effectively see them if its weights saturated at 2^8: clipped at the
    stage-0 maximum + 8 log2 units (the fault-sensitivity mutation of the lazy-rescale branch)"""
    m0 = s[..., :STAGE].amax(-1, keepdim=True)
    return torch.minimum(s, m0 + REBASE_LOG2 * LN2)


def weight_of(s_row, pos):
    """softmax weight of position pos in one (row, head)'s scores"""
    return float(torch.softmax(s_row.to(F64), -1)[pos])


# ---------------------------------------------------------------------------------------------- split geometry (for spike placement)
def fused_split_blocks(length, S):
    """vv_attn_fused_kernel: split s of S owns the 32-position blocks s, s + S, ..  -> per used split (first block, last block) of a
    row of `length` positions"""
    nb = (length + 31) // 32
    return [(s, s + (nb - 1 - s) // S * S) for s in range(min(S, nb))]


def split_chunk(length, S):
    """vv_attn_split_kernel: positions per split (at least 512, a multiple of 128)"""
    c = -(-length // S)
    c = -(-c // 128) * 128
    return max(c, 512)


def split_ranges(length, S):
    c = split_chunk(length, S)
    return [(s * c, min(length, (s + 1) * c)) for s in range(S) if s * c < length]
