"""tests/attn_ref.py (the fp64 reference test_gpu_attn_paths.py compares every attention launch with) and the inputs of
tests/attn_cases.py, on the CPU:

  (a) the reference agrees with oracle/lm.py's Qwen2Oracle on the readout layer to fp32 class, rel-L2 <= 1e-5 per (row, head): both
      head dims, groups of 2 and 7, a chunk over a prefix, then decode steps -- it cannot inherit a kernel's mistake;
  (b) what the GPU bounds are worth: for every case family of the GPU file, a mutation of the reference -- the faults the kernels
      could have -- moves the targeted (row, head) by at least 10 x the loosest ceiling (2^-7, the bf16 mode's) in the metric the GPU
      tests use, or makes it non-finite (the GPU tests fill every unused slot with NaN);
  (c) the reference's fp32 form (the oracle's RoPE) against its fp64 form, both rounded to bf16: never more than one bf16 step
      apart, at most 0.25 % of the elements apart at all -- a quarter of the cap test_append_exact puts on the GPU.  Elements
      whose rotation cancels to below 2^-14 of the pair (3.9e-5 of all angles) are judged in absolute terms
      (attn_ref.rotated_k_steps): no fp32 rotation resolves a bf16 step of such a result -- one element of 294,912 sat 7 steps
      apart at a value of 1.4e-7 from operands of 0.36;
  (d) on the dimension that carries the planted logits the q operand of every row, before its bf16 rounding, lies at least 2^-12
      (relative) from a rounding boundary: a last-bit difference of the device's fp32 value cannot move a planted logit."""
import pytest
import torch

import attn_cases as AC
import attn_ref as R
import lm_shapes as ls
from oracle import lm as olm

F64 = torch.float64
CEILING = 2.0 ** -7
MOVE = 10 * CEILING


def _per_head(got, ref):
    d = got.to(F64) - ref.to(F64)
    return d.norm(dim=-1) / ref.to(F64).norm(dim=-1)


@pytest.mark.parametrize("geo", ["A", "B"])
@pytest.mark.parametrize("design", ["random", "spike"])
def test_reference_matches_oracle(geo, design):
    cfg = ls.ATTN_GEO[geo]
    w = AC.readout_weights(cfg)
    m = olm.Qwen2Oracle(w, 1, cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.theta, cfg.eps, kv_round_bf16=True)
    n0, T = 75, 20
    k, v = AC.prefix(cfg, n0, design, "fused", 7, spikes=[31, 40][:cfg.kv_heads])
    cache = m.new_cache()
    cache.k[0], cache.v[0], cache.length = k.float(), v.float(), n0
    worst = 0.0
    for step, (p0, rows) in enumerate([(n0, T), (n0 + T, 1), (n0 + T + 1, 1)]):       # prefix + chunk, then decode steps
        x = AC.x_rows(cfg, rows, 100 + step, own=(3,) if rows > 3 else ())
        with torch.no_grad():
            h = m.forward(x, cache, final_norm=False)
        rs = ls.span(0, p0, rows)
        ref, a, _ = AC.reference(w, cfg, 3, "fused", rs, x, {0: (cache.k[0], cache.v[0])})
        worst = max(worst, float(_per_head(h.view(rows, cfg.heads, cfg.head_dim), ref).max()))
    assert worst <= 1e-5, worst


# ---------------------------------------------------------------------------------------------- (b) fault sensitivity
def cpu_pass(w, cfg, rows, x, pre):
    """the caches after a pass, as the GPU test would export them: pre = {cache: (k, v) bf16 prefix}; the appended positions hold
    bf16(project_kv); every other slot up to one past the end is NaN (the GPU test's pre-fill) -> {cache: (k, v) fp64 [Hkv, L, D]}"""
    pos = torch.tensor([p for _, p in rows])
    kn, vn = AC.project_kv(w, cfg, x, pos)
    out = {}
    for c in sorted({c for c, _ in rows}):
        idx = [i for i, (cc, _) in enumerate(rows) if cc == c]
        L = int(pos[idx].max()) + 2
        k = torch.full((cfg.kv_heads, L, cfg.head_dim), float("nan"), dtype=F64)
        v = k.clone()
        n0 = pre[c][0].shape[1]
        k[:, :n0], v[:, :n0] = pre[c][0].to(F64), pre[c][1].to(F64)
        for i in idx:
            k[:, int(pos[i])] = R.bf16r(kn[:, i]).to(F64)
            v[:, int(pos[i])] = R.bf16r(vn[:, i]).to(F64)
        out[c] = (k, v)
    return out


def mutated(cfg, qop, k, v, limit, kind, arg=None):
    """attention of rows that share the cache k, v [Hkv, L, D] with one fault -> out [T, Hq, D]"""
    G = cfg.heads // cfg.kv_heads
    kv_of_head = None
    k, v = k.clone(), v.clone()
    limit = limit.clone()
    if kind == "admit_len":
        limit = limit + 1
    elif kind == "limit_minus_one":
        limit = limit - 1
    elif kind == "swap_v":
        v[:, [arg, arg ^ 1]] = v[:, [arg ^ 1, arg]]
    elif kind == "other_kv":
        kv_of_head = [(cfg.kv_heads - 1) - h // G for h in range(cfg.heads)]
    elif kind == "stale_slot":              # the slot of the new token as it was before the pass
        k[:, arg], v[:, arg] = float("nan"), float("nan")
    n = int(limit.max())
    s = R.scores(qop, k[:, :n], limit, kv_of_head)
    if kind == "drop":
        s[:, :, arg] = float("-inf")
    elif kind == "omit_positions":          # a split's partial left out of the merge
        s[:, :, arg] = float("-inf")
    elif kind == "never_rebase":
        s = R.clip_never_rebased(s)
    return R.softmax_v(s, v[:, :n], kv_of_head)[0]


def moved(cfg, xs, family, rows, x, caches, kind, arg=None, target_rows=None):
    """the smallest normalised move over the targeted rows and the +c heads (the heads that see a planted logit); inf = non-finite"""
    w = FAM_W[(cfg.hidden, family)]
    ref, a, _ = AC.reference(w, cfg, xs, family, rows, x, caches)
    T = len(rows)
    pos = torch.tensor([p for _, p in rows])
    qb = w["layers.0.self_attn.q_proj.bias"].view(1, cfg.heads, cfg.head_dim).expand(T, -1, -1)
    qop = R.q_operand(R.rope(qb, pos, R.inv_freq(cfg.head_dim, cfg.theta)), xs, family)
    c = rows[0][0]
    idx = [i for i, (cc, _) in enumerate(rows) if cc == c]
    k, v = caches[c]
    out = mutated(cfg, qop[idx], k, v, pos[idx] + 1, kind, arg)
    mut = x.to(F64).view(T, cfg.heads, -1)[idx] + out
    rel, _ = R.row_head_errs(mut, ref[idx], a[idx])
    rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
    tr = list(range(len(idx))) if target_rows is None else target_rows
    return float(rel[tr][:, 0::2].min())


FAM_W = {}
for _g in ("A", "B"):
    for _f in ("fused", "split", "prefill4"):
        FAM_W[(ls.ATTN_GEO[_g].hidden, _f)] = AC.readout_weights(ls.ATTN_GEO[_g], _f)


@pytest.mark.parametrize("xs", [1, 3])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_fused_decode_faults_are_visible(geo, xs):
    """one decode row over 2100 positions in three splits, one over 33 (two blocks) -- each on its own cache, judged alone"""
    cfg = ls.ATTN_GEO[geo]
    w = FAM_W[(cfg.hidden, "fused")]
    S = 3
    for n0 in (2100, 33):
        blocks = R.fused_split_blocks(n0, S)
        for sp, (first, last) in enumerate(blocks):
            spike = min(32 * last + 31, n0 - 1)
            spikes = [spike] * cfg.kv_heads
            pre = {0: AC.prefix(cfg, n0, "spike", "fused", 11 + sp, spikes=spikes)}
            rows, x = [(0, n0)], AC.x_rows(cfg, 1, 12)
            caches = cpu_pass(w, cfg, rows, x, pre)
            own = [p for p in range(n0) if (p // 32) % S == sp]
            assert moved(cfg, xs, "fused", rows, x, caches, "drop", spike) >= MOVE
            assert moved(cfg, xs, "fused", rows, x, caches, "swap_v", spike) >= MOVE
            assert moved(cfg, xs, "fused", rows, x, caches, "omit_positions", own) >= MOVE
            assert moved(cfg, xs, "fused", rows, x, caches, "admit_len") >= MOVE
            if cfg.kv_heads > 1:
                assert moved(cfg, xs, "fused", rows, x, caches, "other_kv") >= MOVE
        # the new token itself: an own row's K carries the planted logit
        pre = {0: AC.prefix(cfg, n0, "random", "fused", 13)}
        rows, x = [(0, n0)], AC.x_rows(cfg, 1, 14, own=(0,))
        caches = cpu_pass(w, cfg, rows, x, pre)
        assert moved(cfg, xs, "fused", rows, x, caches, "limit_minus_one") >= MOVE
        assert moved(cfg, xs, "fused", rows, x, caches, "stale_slot", n0) >= MOVE


@pytest.mark.parametrize("xs", [1, 3])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_split_merge_faults_are_visible(geo, xs):
    """a 5-row span at 1020 (two splits of 640 positions): a spike in the prefix, then on row 2's own position"""
    cfg = ls.ATTN_GEO[geo]
    w = FAM_W[(cfg.hidden, "split")]
    n, p0, S = 5, 1020, 2
    rows = ls.span(0, p0, n)
    for a0, b0 in R.split_ranges(p0 + 1, S):
        spike = min(b0, p0) - 1
        pre = {0: AC.prefix(cfg, p0, "spike", "split", 21, spikes=[spike] * cfg.kv_heads)}
        x = AC.x_rows(cfg, n, 22)
        caches = cpu_pass(w, cfg, rows, x, pre)
        assert moved(cfg, xs, "split", rows, x, caches, "drop", spike) >= MOVE
        assert moved(cfg, xs, "split", rows, x, caches, "swap_v", spike) >= MOVE
        assert moved(cfg, xs, "split", rows, x, caches, "omit_positions", list(range(a0, min(b0, p0)))) >= MOVE
        if cfg.kv_heads > 1:
            assert moved(cfg, xs, "split", rows, x, caches, "other_kv") >= MOVE
    pre = {0: AC.prefix(cfg, p0, "random", "split", 23)}
    x = AC.x_rows(cfg, n, 24, own=(2,))
    caches = cpu_pass(w, cfg, rows, x, pre)
    assert moved(cfg, xs, "split", rows, x, caches, "limit_minus_one", target_rows=[2]) >= MOVE
    assert moved(cfg, xs, "split", rows, x, caches, "stale_slot", p0 + 2, target_rows=[2, 3, 4]) >= MOVE
    # the last row's limit + 1 reads the NaN slot past the span
    assert moved(cfg, xs, "split", rows, x, caches, "admit_len", target_rows=[4]) >= MOVE


@pytest.mark.parametrize("geo", ["A", "B"])
def test_prefill4_faults_are_visible(geo):
    """a 150-row chunk at 1000 (bf16 mode, three 64-row tiles): spike, every own row of attn_cases.own_rows -- the rows the GPU test
    plants, the 64-row tile edges 63 | 64 and 127 | 128 among them -- and the up-ramp whose every row re-bases"""
    cfg = ls.ATTN_GEO[geo]
    w = FAM_W[(cfg.hidden, "prefill4")]
    n, p0 = 150, 1000
    rows = ls.span(0, p0, n)
    for spike in (p0 - 1, 63, 64, 959):
        pre = {0: AC.prefix(cfg, p0, "spike", "prefill4", 31, spikes=[spike] * cfg.kv_heads)}
        x = AC.x_rows(cfg, n, 32)
        caches = cpu_pass(w, cfg, rows, x, pre)
        assert moved(cfg, 1, "prefill4", rows, x, caches, "drop", spike) >= MOVE
        assert moved(cfg, 1, "prefill4", rows, x, caches, "swap_v", spike) >= MOVE
        if cfg.kv_heads > 1:
            assert moved(cfg, 1, "prefill4", rows, x, caches, "other_kv") >= MOVE
    pre = {0: AC.prefix(cfg, p0, "random", "prefill4", 33)}
    assert {63, 64, 127, 128} <= set(AC.own_rows(n))
    for j0 in AC.own_rows(n):
        x = AC.x_rows(cfg, n, 34, own=(j0,))
        caches = cpu_pass(w, cfg, rows, x, pre)
        assert moved(cfg, 1, "prefill4", rows, x, caches, "limit_minus_one", target_rows=[j0]) >= MOVE, j0
        assert moved(cfg, 1, "prefill4", rows, x, caches, "stale_slot", p0 + j0, target_rows=list(range(j0, n))) >= MOVE, j0
        if j0:          # the row before it admits one position too many: the own row's planted K (63 sees 64's, 127 sees 128's)
            assert moved(cfg, 1, "prefill4", rows, x, caches, "admit_len", target_rows=[j0 - 1]) >= MOVE, j0
        # the rows at and after the own row re-base in its stage, the 16 rows before it do not and give its position no weight
        _, _, sc = AC.reference(w, cfg, 1, "prefill4", rows, x, caches)
        st = (p0 + j0) // 64
        near = range(max(0, j0 - 16), min(n, 16 * (j0 // 16) + 16))
        assert all((st in R.rebase_stages(sc[j][0])) == (j >= j0) for j in near), j0
        assert all(R.weight_of(sc[j][0], p0 + j0) == 0.0 for j in near if j < j0), j0
    x = AC.x_rows(cfg, n, 34, own=(70,))
    caches = cpu_pass(w, cfg, rows, x, pre)
    assert moved(cfg, 1, "prefill4", rows, x, caches, "admit_len", target_rows=[n - 1]) >= MOVE      # the NaN slot past the chunk
    pre = {0: AC.prefix(cfg, p0, "ramp", "prefill4", 35)}
    x = AC.x_rows(cfg, n, 36)
    caches = cpu_pass(w, cfg, rows, x, pre)
    _, _, sc = AC.reference(w, cfg, 1, "prefill4", rows, x, caches)
    inside = lambda j, h: [s for s in R.rebase_stages(sc[j][h]) if s < p0 // 64]       # stages wholly inside the prefix
    assert min(len(inside(j, 0)) for j in range(n)) >= 4           # the up-ramp head
    assert max(len(inside(j, 1)) for j in range(n)) == 0           # the down-ramp head
    assert moved(cfg, 1, "prefill4", rows, x, caches, "never_rebase") >= MOVE


# ---------------------------------------------------------------------------------------------- (c), (d)
@pytest.mark.parametrize("geo", ["A", "B"])
def test_append_flip_cap(geo):
    cfg = ls.ATTN_GEO[geo]
    w = AC.readout_weights(cfg, k_zero=True)
    D = cfg.head_dim
    m = olm.Qwen2Oracle(w, 1, cfg.heads, cfg.kv_heads, D, cfg.theta, cfg.eps)
    pos = torch.arange(ls.ATTN_MAX_CTX)
    kb = w["layers.0.self_attn.k_proj.bias"].view(1, cfg.kv_heads, D).expand(len(pos), -1, -1)
    u, flat = R.rotated_k_steps(m._rope(kb.float(), pos), R.rope(kb, pos, R.inv_freq(D, cfg.theta)), kb)
    # a rotation lands below 2^-14 of its pair's length for 2 * 2^-14 / pi = 3.9e-5 of all angles
    assert float(flat.double().mean()) <= 1e-4 and int(u.max()) <= 1, (int(flat.sum()), int(u.max()))
    assert float((u > 0).double().mean()) <= 0.0025, float((u > 0).double().mean())


@pytest.mark.parametrize("family", ["fused", "prefill4"])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_planted_q_operand_is_far_from_a_rounding_boundary(geo, family):
    """every position a case of lm_shapes.ATTN_* can reach ([0, max_ctx)), every head; "split" rounds as "fused" does"""
    cfg = ls.ATTN_GEO[geo]
    D = cfg.head_dim
    pos = torch.arange(ls.ATTN_MAX_CTX)
    qb = AC.q_bias(cfg, family).view(1, cfg.heads, D).expand(len(pos), -1, -1)
    pre = R.q_prerounding(R.rope(qb, pos, R.inv_freq(D, cfg.theta)), 1, family)[:, :, D // 2 - 1]
    assert float(R.bf16_boundary_distance(pre).min()) >= 2.0 ** -12
    # ... and the operand is the planted value: 4 natural units, or 6 log2 units, per unit of K, within 1e-5
    want = 6.0 * R.LN2 if family == "prefill4" else 4.0
    op = R.q_operand(R.rope(qb, pos, R.inv_freq(D, cfg.theta)), 1, family)[:, :, D // 2 - 1]
    assert float((op.abs() / want - 1).abs().max()) <= 1e-5
    assert float(R.q_operand(R.rope(qb, pos, R.inv_freq(D, cfg.theta)), 3, family)[:, :, D - 1].abs().max()) <= 4.0 * 4.1e-3
