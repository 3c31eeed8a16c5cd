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
      (relative) from a rounding boundary: a last-bit difference of the device's fp32 value cannot move a planted logit;
  (e) the same at the contexts of test_gpu_attn_long.py (lm_shapes.ATTN_LONG_*: 64 and 67 splits over 65K positions), where the
      engines run on attn_cases.long_inv_freq: (d) at positions up to 69,631 and (c) at the positions that file appends at; the
      comb design holds >= 0.9 of the weight and the loss of ANY one split moves its row by >= 10 x the bf16 bound; the random
      design moves by more than 2 x the xs = 2 bound when any one split or any one 32-position block is lost; the tail ramp
      re-bases the up-ramp head in >= 4 of the last 16 prefix stages with |K| <= 64."""
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


def moved(cfg, xs, family, rows, x, caches, kind, arg=None, target_rows=None, w=None):
    """the smallest normalised move over the targeted rows and the +c heads (the heads that see a planted logit); inf = non-finite"""
    w = FAM_W[(cfg.hidden, family)] if w is None else w
    ref, a, _ = AC.reference(w, cfg, xs, family, rows, x, caches)
    T = len(rows)
    pos = torch.tensor([p for _, p in rows])
    qb = w["layers.0.self_attn.q_proj.bias"].view(1, cfg.heads, cfg.head_dim).expand(T, -1, -1)
    qop = R.q_operand(R.rope(qb, pos, AC.rope_table(w, cfg)), xs, family)
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


# ---------------------------------------------------------------------------------------------- (e) the long contexts
from test_gpu_attn_paths import ATTN_BOUND          # noqa: E402  (the bounds of the short file: what a fault has to exceed)


def long_w(cfg, family="fused", k_zero=False):
    return AC.readout_weights(cfg, family, k_zero, inv_freq=AC.long_inv_freq(cfg.head_dim, cfg.theta))


@pytest.mark.parametrize("case", ["L1", "L1x"])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_comb_shows_the_loss_of_any_split(geo, case):
    """the decode row of L1 / L1x with one planted position per split (attn_cases.comb_fused): from the reference alone"""
    cfg = ls.ATTN_GEO[geo]
    w = long_w(cfg)
    (n,), S = ls.ATTN_LONG_DECODE_LENS[case], ls.ATTN_LONG_DECODE_SPLITS[case][geo]
    comb = AC.comb_fused(n, S)
    assert len(comb) == S and sorted((p // 32) % S for p in comb) == list(range(S))
    assert len({p % 32 for p in comb}) >= 16 and len({(p // 32) // S for p in comb}) >= 5       # offsets and blocks vary
    pre = {0: AC.prefix(cfg, n, "comb", "fused", AC.LONG_SEED + n, spikes=comb)}
    rows, x = [(0, n)], AC.x_rows(cfg, 1, 50)
    caches = cpu_pass(w, cfg, rows, x, pre)
    _, _, sc = AC.reference(w, cfg, 1, "fused", rows, x, caches)
    for kvh in range(cfg.kv_heads):
        assert sum(R.weight_of(sc[0][AC.plus_head(cfg, kvh)], p) for p in comb) >= 0.9
    _, spl = losses(sc[0], *caches[0], cfg, S)
    plus = list(range(0, cfg.heads, 2))             # the +c heads
    # losses() against the mutation the other tests of this file use, on one split
    own = [p for p in range(n + 1) if (p // 32) % S == 5]
    assert abs(moved(cfg, 1, "fused", rows, x, caches, "omit_positions", own, w=w) - float(spl[plus, 5].min())) <= 1e-9
    print(f"comb {geo} {case}: least move of a +c head without one split {float(spl[plus].min()):.3f} (10 x the bf16 bound: {10 * ATTN_BOUND[('fused', 1)]:.3f})")
    assert float(spl[plus].min()) >= 10 * ATTN_BOUND[("fused", 1)], float(spl[plus].min())


def losses(sc_row, k, v, cfg, S):
    """one decode row's fp64 scores [Hq, L] over the cache v [Hkv, L, D]: the normalised move of every head when one 32-position
    block, and when one split of S (the blocks s, s + S, ..), is left out -> ([Hq, blocks], [Hq, S])"""
    Hq, L = sc_row.shape
    G, D = cfg.heads // cfg.kv_heads, cfg.head_dim
    nb = (L + 31) // 32
    p = torch.zeros(Hq, nb * 32, dtype=F64)
    p[:, :L] = torch.softmax(sc_row, -1)
    vv = torch.zeros(cfg.kv_heads, nb * 32, D, dtype=F64)
    vv[:, :L] = v[:, :L]
    vv = vv[torch.arange(Hq) // G].view(Hq, nb, 32, D)
    pb = p.view(Hq, nb, 32)
    ob = torch.einsum("hbi,hbid->hbd", pb, vv)              # every block's share of the output
    wb = pb.sum(-1)
    out, a = ob.sum(1), torch.einsum("hbi,hbid->hd", pb, vv.abs())

    def move(o_part, w_part):
        without = (out[:, None] - o_part) / (1.0 - w_part)[..., None]
        return (without - out[:, None]).norm(dim=-1) / a.norm(dim=-1)[:, None]
    split_of = torch.arange(nb) % S
    os_ = torch.stack([ob[:, split_of == s].sum(1) for s in range(S)], 1)
    ws_ = torch.stack([wb[:, split_of == s].sum(1) for s in range(S)], 1)
    return move(ob, wb), move(os_, ws_)


@pytest.mark.parametrize("case", ["L1", "L1x"])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_random_design_shows_the_loss_of_any_split_and_any_block(geo, case):
    """a condition on the INPUTS of test_fused_decode_long's random design (same seeds): in the exact modes no split and no single
    32-position block of the long row can go missing inside the bound.  A workgroup serves one kv head, so what it loses is lost to
    every query head of that group: the move of the group's worst head is what the GPU test sees"""
    cfg = ls.ATTN_GEO[geo]
    w = long_w(cfg)
    (n,), S = ls.ATTN_LONG_DECODE_LENS[case], ls.ATTN_LONG_DECODE_SPLITS[case][geo]
    pre = {0: AC.prefix(cfg, n, "random", "fused", AC.LONG_SEED + n)}
    rows, x = [(0, n)], AC.x_rows(cfg, 1, 50)
    caches = cpu_pass(w, cfg, rows, x, pre)
    _, _, sc = AC.reference(w, cfg, 2, "fused", rows, x, caches)
    blk, spl = losses(sc[0], *caches[0], cfg, S)
    group = lambda t: float(t.view(cfg.kv_heads, cfg.heads // cfg.kv_heads, -1).amax(1).min())
    print(f"random design {geo} {case}: least move without one split {group(spl):.2e}, without one block {group(blk):.2e} "
          f"(2 x the xs = 2 bound: {2 * ATTN_BOUND[('fused', 2)]:.2e})")
    assert group(spl) > 2 * ATTN_BOUND[("fused", 2)] and group(blk) > 2 * ATTN_BOUND[("fused", 2)], (group(spl), group(blk))


@pytest.mark.parametrize("geo", ["A", "B"])
def test_tail_ramp_rebases_late_and_stays_small(geo):
    cfg = ls.ATTN_GEO[geo]
    w = long_w(cfg, "prefill4")
    for n, p0 in ((8, 32760), (20, 65000)):
        k, v = AC.prefix(cfg, p0, "tail", "prefill4", 35)
        assert float(k.float().abs().max()) <= 64.0
        rows, x = ls.span(0, p0, n), AC.x_rows(cfg, n, 36)
        caches = cpu_pass(w, cfg, rows, x, {0: (k, v)})
        _, _, sc = AC.reference(w, cfg, 1, "prefill4", rows, x, caches)
        last16 = range(p0 // 64 - 16, p0 // 64)
        for j in (0, n - 1):
            assert len([s for s in R.rebase_stages(sc[j][0]) if s in last16]) >= 4
            assert not [s for s in R.rebase_stages(sc[j][1]) if s in last16]
        assert moved(cfg, 1, "prefill4", rows, x, caches, "never_rebase", w=w) >= MOVE


def rope32(x, pos, invf):
    """the reference model's fp32 form of attn_ref.rope: angle, cos, sin and the rotation all in fp32"""
    ang = pos.to(torch.float32)[:, None] * invf.to(torch.float32)[None, :]
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos()[:, None, :], emb.sin()[:, None, :]
    x = x.to(torch.float32)
    half = x.shape[-1] // 2
    return x * cos + torch.cat([-x[..., half:], x[..., :half]], -1) * sin


def long_append_positions():
    pos = list(ls.ATTN_LONG_APPEND_DECODE)
    for p0 in ls.ATTN_LONG_APPEND_SPANS:
        pos += range(p0, p0 + ls.ATTN_APPEND_SPAN)
    pos += range(ls.ATTN_LONG_APPEND_CHUNK_POS, ls.ATTN_LONG_APPEND_CHUNK_POS + max(ls.ATTN_LONG_APPEND_CHUNKS))
    pos += range(ls.QKV_ROPE_POS0, ls.QKV_ROPE_POS0 + ls.QKV_ROPE_ROWS, 7)
    return torch.tensor(sorted(set(pos)))


@pytest.mark.parametrize("geo", ["A", "B", "qkv"])
def test_append_flip_cap_long(geo):
    """(c) at the positions test_append_exact_long and test_qkv_rope_epilogue_append append at, on the table their engines hold"""
    cfg = ls.QKV_ROPE_CFG if geo == "qkv" else ls.ATTN_GEO[geo]
    D = cfg.head_dim
    invf = R.inv_freq(D, cfg.theta) if geo == "qkv" else AC.long_inv_freq(D, cfg.theta)
    kb = (synth_k_bias(cfg) if geo == "qkv" else long_w(cfg, k_zero=True)["layers.0.self_attn.k_proj.bias"]).view(1, cfg.kv_heads, D)
    pos = long_append_positions()
    kb = kb.expand(len(pos), -1, -1)
    u, flat = R.rotated_k_steps(rope32(kb, pos, invf), R.rope(kb, pos, invf), kb)
    assert float(flat.double().mean()) <= 1e-4 and int(u.max()) <= 1, (int(flat.sum()), int(u.max()))
    assert float((u > 0).double().mean()) <= 0.0025, float((u > 0).double().mean())


def synth_k_bias(cfg):
    import synth
    return synth.lm_weights(cfg, seed=31)["layers.0.self_attn.k_proj.bias"]


@pytest.mark.parametrize("family", ["fused", "prefill4"])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_planted_q_operand_stays_a_bf16_value_at_long_positions(geo, family):
    """(d) on the long engines' table: its last entry is 0, the planted pair does not rotate, and the operand is the planted value at
    every position -- 32,767, 65,535, 69,631 and a stride over the whole context.  On the model's own table it is not: the pair has
    turned by 0.09 rad at 65,535 and c cos(phi) sits 4e-3 below c"""
    cfg = ls.ATTN_GEO[geo]
    D = cfg.head_dim
    pos = torch.tensor(sorted({32767, 65535, 69631} | set(range(0, ls.ATTN_LONG_MAX_CTX, 997))))
    qb = AC.q_bias(cfg, family).view(1, cfg.heads, D).expand(len(pos), -1, -1)
    invf = AC.long_inv_freq(D, cfg.theta)
    assert float(invf[-1]) == 0.0 and torch.equal(invf[:-1], R.inv_freq(D, cfg.theta)[:-1])
    pre = R.q_prerounding(R.rope(qb, pos, invf), 1, family)[:, :, D // 2 - 1]
    assert float(R.bf16_boundary_distance(pre).min()) >= 2.0 ** -12
    want = 6.0 * R.LN2 if family == "prefill4" else 4.0
    op = R.q_operand(R.rope(qb, pos, invf), 1, family)[:, :, D // 2 - 1]
    assert float((op.abs() / want - 1).abs().max()) <= 1e-5
    assert float(R.q_operand(R.rope(qb, pos, invf), 3, family)[:, :, D - 1].abs().max()) == 0.0
    model = R.q_operand(R.rope(qb, torch.tensor([65535]), R.inv_freq(D, cfg.theta)), 3, family)[:, :, D // 2 - 1]
    assert float((model.abs() / want - 1).abs().max()) >= 1e-3
