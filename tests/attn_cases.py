"""Inputs of the attention tests (test_attn_ref_cpu.py, test_gpu_attn_paths.py): the readout layer, the prefix score designs and
the fp64 projection of the appended K / V.  CPU only, no engine import.

READOUT LAYER.  A one-layer LM whose weights are all exactly representable in bf16:
  o_proj = identity (heads * head_dim == hidden), down_proj = 0:  the layer returns x + attention, head h in columns [h D, (h + 1) D)
  q_proj.weight = 0:  q is q_proj.bias rotated to the row's position -- no projection rounding reaches q on any route
  k_proj:  the rows feeding dims D/2 - 1 and D - 1 (the lowest-frequency pair) are zero but for ONE column (SPIKE_COL) of the row
           feeding D/2 - 1: an x row with its energy in that channel appends a K that carries a planted logit (the "own" design)

PLANTED LOGITS ride on dim D/2 - 1 alone: q bias +-c there (even heads +c, odd heads -c), 0 on its partner D - 1; the rotation of
that pair is below 4e-3 rad over 2304 positions at theta = 1e6, so the q operand there stays c cos(phi) within 8e-6 of c.  c is
chosen per kernel family so that the operand the matrix unit sees is a bf16 value: 4 (natural units per unit of K) for the fused and
split kernels, 6 (log2 units) for vv_attn_prefill4, whose operand carries log2(e).  A flip of the device's fp32 value can then not
move a 40-nat logit (test_attn_ref_cpu.py, q rounding stability).  Over the 65K positions of test_gpu_attn_long.py the pair would
turn by 0.09 rad: those engines run on long_inv_freq, whose last entry is 0, and the weight dict carries that table (INV_FREQ)."""

import torch

import attn_ref as R
import synth

F64 = torch.float64
Q_STD = 2.0                 # random part of q: scores of std about 2 against K of std 1
SPIKE_COL = 5               # the hidden channel whose k_proj column feeds dim D/2 - 1
SPIKE_X = 2.0               # an "own" row's x in that channel (the others: std 0.02)
SPIKE_W = {256: 0.25, 896: 0.125}       # that column's weight: K[D/2 - 1] of an own row about 3.8 -> about 15 nats
X_STD = 0.02
SPIKE_NAT, SINK_NAT = 15.0, 40.0
RAMP_LOG2_PER_STAGE = 6.5


def plant_unit(family):
    """natural units of logit per unit of K[D/2 - 1] on a +c head"""
    return 6.0 * R.LN2 if family == "prefill4" else 4.0


def plant_c(D, family):
    """the q bias on dim D/2 - 1 (fp32): its scaled operand is 4 (fused, split) or, times log2(e), 6 (prefill4), to fp32 rounding"""
    scale = float(1.0 / torch.sqrt(torch.tensor(float(D), dtype=torch.float32)))
    target = 6.0 / float(R.LOG2E_F32) if family == "prefill4" else 4.0
    return float(torch.tensor(target / scale, dtype=torch.float32))


def q_bias(cfg, family, seed=41):
    """[Hq, D] fp32"""
    D = cfg.head_dim
    q = synth.Gen(seed + D).normal((cfg.heads, D), Q_STD, mat=False)
    c = plant_c(D, family)
    q[:, D // 2 - 1] = torch.tensor([c if h % 2 == 0 else -c for h in range(cfg.heads)])
    q[:, D - 1] = 0.0
    return q


def long_inv_freq(D, theta):
    """the model's fp32 RoPE table with its LAST entry at 0: the lowest-frequency pair (D/2 - 1, D - 1), which carries the planted
    logits, then does not rotate at all -- over 65K positions it would turn by 0.08 to 0.10 rad and c cos(phi) would no longer
    round to c.  Every other pair keeps the model's frequency.  Engines that run past a few thousand positions upload this table as
    lm.rope.inv_freq; a weight dict that holds it under INV_FREQ hands it to project_kv and reference"""
    t = R.inv_freq(D, theta).clone()
    t[-1] = 0.0
    return t


INV_FREQ = "rope.inv_freq"      # optional key of a readout weight dict: the RoPE table of the engine (default: the model's)


def rope_table(w, cfg):
    t = w.get(INV_FREQ)
    return R.inv_freq(cfg.head_dim, cfg.theta) if t is None else t


def readout_weights(cfg, family="fused", k_zero=False, layer=0, inv_freq=None):
    """the oracle-keyed weight dict of the readout layer (module docstring).  k_zero: k_proj.weight = 0 as well and a k bias on every
    dim -- the appended K is then a function of the bias and the position alone (test_append_exact).  layer: which layer of a deeper
    model is the readout layer (the others keep synth's weights; run that layer alone).  inv_freq: the engine's RoPE table when it
    is not the model's (long_inv_freq)"""
    H, D = cfg.hidden, cfg.head_dim
    assert 0 <= layer < cfg.layers and cfg.heads * D == H
    w = synth.lm_weights(cfg, seed=31)
    if inv_freq is not None:
        w[INV_FREQ] = inv_freq.to(torch.float32)
    p = f"layers.{layer}."
    w[p + "self_attn.o_proj.weight"] = torch.eye(H)
    w[p + "mlp.down_proj.weight"] = torch.zeros(H, cfg.inter)
    w[p + "self_attn.q_proj.weight"] = torch.zeros(H, H)
    w[p + "self_attn.q_proj.bias"] = q_bias(cfg, family).reshape(-1)
    kw, kb = w[p + "self_attn.k_proj.weight"].clone(), w[p + "self_attn.k_proj.bias"].clone()
    if k_zero:
        kw.zero_()
    else:
        for kvh in range(cfg.kv_heads):
            for d in (D // 2 - 1, D - 1):
                kw[kvh * D + d] = 0.0
                kb[kvh * D + d] = 0.0
            kw[kvh * D + D // 2 - 1, SPIKE_COL] = SPIKE_W[H]
    w[p + "self_attn.k_proj.weight"], w[p + "self_attn.k_proj.bias"] = kw, kb
    return w


def x_rows(cfg, T, seed, own=()):
    """[T, H] fp32 of std 0.02; rows in `own` carry SPIKE_X in channel SPIKE_COL"""
    x = synth.Gen(seed).normal((T, cfg.hidden), X_STD, mat=False)
    for j in own:
        x[j, SPIKE_COL] = SPIKE_X
    return x


LONG_SEED = 100000          # offset of the prefix seeds of the long decode cases (test_attn_ref_cpu.py holds their random design to a condition)
RAMP_TAIL = 1024            # positions of the "tail" ramp: |K| stays below 64 however long the prefix


def comb_fused(n, S):
    """one prefix position of every split of vv_attn_fused_kernel that holds one, for a decode row over a prefix of n positions (the
    row attends n + 1) in a launch of S splits; the block inside the split and the offset inside the block vary with the split"""
    out = []
    for s, (first, last) in enumerate(R.fused_split_blocks(n + 1, S)):
        nb = len([b for b in range(first, last + 1, S) if 32 * b < n])
        if nb:
            b = first + S * ((5 * s + 1) % nb)
            out.append(min(32 * b + (7 * s + 3) % 32, n - 1))
    return out


def comb_chunks(n, S):
    """the same for vv_attn_split_kernel's contiguous ranges (attn_ref.split_ranges) of a row at position n"""
    out = []
    for s, (a, b) in enumerate(R.split_ranges(n + 1, S)):
        b = min(b, n)
        if b > a:
            nb = (b - a + 31) // 32
            out.append(min(a + 32 * ((5 * s + 1) % nb) + (7 * s + 3) % 32, b - 1))
    return out


COMB_V = 4.0


def prefix(cfg, n, design, family, seed, spikes=None):
    """The imported prefix of one cache: (k, v) bf16 [Hkv, n, D], K as cached (rotated).  Random K / V of std 1 with the planted pair
    of K at zero, then on dim D/2 - 1:
      random  nothing
      spike   spikes[kvh] = one position per kv head about 15 nats above the rest, with a V of its own (mean 4)
      ramp    rising by about 6.5 log2 units per 64 positions (falling on the -c heads)
      tail    that ramp over the last RAMP_TAIL positions alone, flat (zero) before: a long prefix keeps |K| below 64
      sink    +40 nats on position 0
      comb    spikes = a list of positions, the same for every kv head (one per split of the launch: comb_fused, comb_chunks): the
              i-th is zero but for 15 nats on dim D/2 - 1 and carries a V that is zero but for 4.0 in dim i % D -- together they
              hold nearly all the weight of a +c head, and each split's share of the output sits in a dimension of its own"""
    D = cfg.head_dim
    g = synth.Gen(seed)
    k, v = g.normal((cfg.kv_heads, n, D), 1.0), g.normal((cfg.kv_heads, n, D), 1.0)
    k[:, :, D // 2 - 1] = 0.0
    k[:, :, D - 1] = 0.0
    unit = plant_unit(family)
    if n and design == "spike":
        for kvh, pos in enumerate(spikes):
            k[kvh, pos] = 0.0                   # the planted logit alone: exactly that far above the mean of the rest
            k[kvh, pos, D // 2 - 1] = SPIKE_NAT / unit
            v[kvh, pos] = v[kvh, pos] + 4.0 * (1 if kvh % 2 == 0 else -1)
    elif n and design == "ramp":
        k[:, :, D // 2 - 1] = (torch.arange(n, dtype=torch.float32) * (RAMP_LOG2_PER_STAGE * R.LN2 / 64.0 / unit))[None]
    elif n and design == "tail":
        up = (torch.arange(n, dtype=torch.float32) - (n - RAMP_TAIL)).clamp_min(0.0)
        k[:, :, D // 2 - 1] = (up * (RAMP_LOG2_PER_STAGE * R.LN2 / 64.0 / unit))[None]
    elif n and design == "comb":
        assert len(set(spikes)) == len(spikes)
        for i, pos in enumerate(spikes):
            k[:, pos] = 0.0
            k[:, pos, D // 2 - 1] = SPIKE_NAT / unit
            v[:, pos] = 0.0
            v[:, pos, i % D] = COMB_V
    elif n and design == "sink":
        k[:, 0] = 0.0
        k[:, 0, D // 2 - 1] = SINK_NAT / unit
    else:
        assert design in ("random", "spike", "ramp", "tail", "sink", "comb")
    return k.to(torch.bfloat16), v.to(torch.bfloat16)


def rmsnorm64(x, weight, eps):
    x = x.to(F64)
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight.to(F64)


def project_kv(w, cfg, x, pos, layer=0):
    """the K (rotated) and V a pass appends for rows x [T, H] at positions pos, fp64, unrounded: [Hkv, T, D] each"""
    p = f"layers.{layer}."
    n = rmsnorm64(x, w[p + "input_layernorm.weight"], cfg.eps)
    T, D = x.shape[0], cfg.head_dim
    k = n @ w[p + "self_attn.k_proj.weight"].to(F64).t() + w[p + "self_attn.k_proj.bias"].to(F64)
    v = n @ w[p + "self_attn.v_proj.weight"].to(F64).t() + w[p + "self_attn.v_proj.bias"].to(F64)
    k = R.rope(k.view(T, cfg.kv_heads, D), pos, rope_table(w, cfg))
    return k.transpose(0, 1), v.view(T, cfg.kv_heads, D).transpose(0, 1)


def v_term_norm(w, cfg, x, layer=0):
    """sqrt(sum_k (n_k W_v[d][k])^2) + |b_v[d]| of every appended V element, [Hkv, T, D]: the magnitude of the partial sums an fp32
    accumulation of the projection rounds (terms of random sign)"""
    p = f"layers.{layer}."
    n = rmsnorm64(x, w[p + "input_layernorm.weight"], cfg.eps)
    s = torch.sqrt((n ** 2) @ (w[p + "self_attn.v_proj.weight"].to(F64) ** 2).t()) + w[p + "self_attn.v_proj.bias"].to(F64).abs()
    return s.view(x.shape[0], cfg.kv_heads, cfg.head_dim).transpose(0, 1)


def reference(w, cfg, xs, family, rows, x, caches, layer=0):
    """What the readout layer returns for one launch: rows = (cache, pos) pairs, x [T, H], caches = {cache: (k, v) [Hkv, L, D] as the
    cache holds them AFTER the pass}.  -> (ref [T, Hq, D] = x + attention, a [T, Hq, D], scores {row: [Hq, L]} in natural units)"""
    Hq, D = cfg.heads, cfg.head_dim
    T = len(rows)
    pos = torch.tensor([p for _, p in rows])
    qb = w[f"layers.{layer}.self_attn.q_proj.bias"].view(1, Hq, D).expand(T, Hq, D)
    qop = R.q_operand(R.rope(qb, pos, rope_table(w, cfg)), xs, family)
    out, a, sc = torch.zeros(T, Hq, D, dtype=F64), torch.zeros(T, Hq, D, dtype=F64), {}
    for c in sorted({c for c, _ in rows}):
        idx = [i for i, (cc, _) in enumerate(rows) if cc == c]
        k, v = caches[c]
        lim = pos[idx] + 1
        n = int(lim.max())
        s = R.scores(qop[idx], k[:, :n], lim)
        o, aa, _ = R.softmax_v(s, v[:, :n])
        out[idx], a[idx] = o, aa
        for j, i in enumerate(idx):
            sc[i] = s[j]
    return x.to(F64).view(T, Hq, D) + out, a, sc


# ---------------------------------------------------------------------------------------------- spike placement
def spike_candidates(length, ranges):
    """positions of a prefix of `length` worth a spike: 0, 15, 16, 31, 32, length - 33, length - 32, length - 2, length - 1 (the
    diagonal neighbour of the row that follows the prefix) and the last position of every block listed in `ranges` -- one list of
    32-position block numbers per split: its first and last block (fused_ranges / chunk_ranges)"""
    c = [0, 15, 16, 31, 32, length - 33, length - 32, length - 2, length - 1]
    for blocks in ranges:
        c += [min(32 * b + 31, length - 1) for b in blocks]
    out = []
    for p in c:
        if 0 <= p < length and p not in out:
            out.append(p)
    return out


def fused_ranges(length, S):
    """first and last block of every split of vv_attn_fused_kernel"""
    return [list(fl) for fl in R.fused_split_blocks(length, S)]


def chunk_ranges(length, S):
    """first and last block of every split of vv_attn_split_kernel"""
    return [[a // 32, (b - 1) // 32] for a, b in R.split_ranges(length, S)]



def plus_head(cfg, kvh):
    """a query head of kv head kvh's group that carries +c (an even head): the head that sees that kv head's planted logits"""
    G = cfg.heads // cfg.kv_heads
    return next(h for h in range(kvh * G, (kvh + 1) * G) if h % 2 == 0)


def own_rows(n):
    """rows of an n-row chunk worth an own spike: the first row, the last row of every 64-row tile and the first of the next (63,
    64, 127, 128: where the tile values of a vv_attn_prefill4 workgroup change), two rows inside a 16-row tile, the last row"""
    out = []
    for j in (0, 63, 64, 127, 128, 5, 77, n - 1):
        if 0 <= j < n and j not in out:
            out.append(j)
    return out
