"""Every attention path of the LM pass -- vv_attn_fused_kernel (+ vv_attn_merge2_kernel), vv_rope_append_kernel + vv_attn_split_kernel +
vv_attn_merge_kernel, vv_attn_prefill4_kernel -- ONE launch at a time against the fp64 reference of tests/attn_ref.py (itself held to
the oracle by tests/test_attn_ref_cpu.py), per (row, head).

No new entry point: the READOUT LAYER of tests/attn_cases.py (identity o-projection, zero down projection, zero q projection) makes
vv_lm_forward_range(.., 0, 1, final_norm = 0) return x + attention, head h in columns [h D, (h + 1) D), with q = the q bias rotated
to the row's position.  The prefix K / V are placed with vv_kv_import (bf16, exact) and the whole cache is read back with
vv_kv_export after the pass: the reference attends over what the cache holds, so the K / V a pass appended are inputs, not a source
of error (test_append_exact holds them on their own).  Which kernels a row set runs is asserted on the CPU, from the same row sets
(tests/lm_shapes.py ATTN_*), by test_pass_plan_cpu.py -- this file never asserts a route it cannot see.

Every pass
  * compares per (row, head):  ||got - ref||_2 / ||a||_2  and  max |got - ref| / max a,  a = softmax-weighted mean of |V| (attn_ref);
  * gives the kernel an output buffer with a guard row before and after and an input with a NaN row before and after (the pass takes
    no strides): results finite, guards bit-unchanged;
  * exports every touched cache before and after: only the appended positions may differ -- and, on the routes that reach
    vv_attn_prefill4, the V slots between the chunk's end and the end of its 64-position stage, which the pass zeroes by design
    (vv_kv_zero_v_tail_kernel) and which must then be exactly zero.  Every slot past a cache's prefix was filled with NaN words
    through vv_kv_import, so a read past the end shows;
  * runs twice from the same state: outputs and caches bit-identical (the merges claim a fixed order).

Score designs on the imported prefix (attn_cases.prefix): random (std about 2), spike (one position per kv head 15 nats above the
rest with a V of its own, walked over the tile, block and split edges), ramp (6.5 log2 units per 64 positions up on the even heads,
down on the odd ones), sink (+40 nats on position 0), and own: a row whose OWN appended K carries the planted logit.

Branch-reach assertions, all read off the reference: test_prefill4 asserts from attn_ref.rebase_stages that the up-ramp head of every
row re-bases in at least four stages after stage 0 (chunks at position 1000) and the down-ramp head in none -- counted over the
stages that lie wholly inside the prefix, where the design sets the scores --, and that the rows of an own row's 16-row tile
re-base in its stage exactly from that row on; the spike and own designs assert the softmax weight the
planted position carries (>= 0.5 on the heads that see it), so a dropped position cannot hide.

Bounds.  ATTN_MEASURED: the worst normalised per-(row, head) rel-L2 over every case of a kernel family and mode of this file on an
MI355X, rounded up in the third digit; the bound is 4 x that (room for other summation orders), the max-error bound 4 x the rel-L2
bound.  Every test prints its worst value beside the bound (run with -s).  The ceilings are conditions, not measurements: xs = 3
below 2e-5 (the exact mode's per-row bound), xs = 2 below 2^-15 (three 16-bit-class roundings), xs = 1 below 2^-7 (P and the
o-projection's operand: one bf16 rounding each, 2^-9 against a; q is rounded identically in the reference).  No bound comes from
another attention launch."""
import pytest
import torch

import attn_cases as AC
import attn_ref as R
import gemv_ref
import lm_shapes as ls
from gpu_util import build_small

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = 12345.0
CEILING = {1: 2.0 ** -7, 2: 2.0 ** -15, 3: 2e-5}
# Worst per-(row, head) rel-L2 / ||a|| over every case of this file, per kernel family and mode, on an MI355X (2026-10-20, libvvhip
# build 899c487a2952f1d8; both geometries; two runs gave the same digits), rounded up in the third digit:
#   fused (+ merge2)   xs 1: 2.713e-03   xs 2: 4.124e-06   xs 3: 8.290e-07
#   split + merge      xs 1: 2.700e-03   xs 2: 4.374e-06   xs 3: 9.957e-07
#   prefill4           xs 1: 2.752e-03
# all under their ceilings (7.81e-03, 3.05e-05, 2e-05).  The bf16 mode sits where two bf16 roundings of 2^-9 each put it; the
# worst max-error seen is 4.4e-03 / 7.9e-06 / 1.5e-06.
ATTN_MEASURED = {("fused", 1): 2.72e-3, ("fused", 2): 4.13e-6, ("fused", 3): 8.30e-7,
                 ("split", 1): 2.71e-3, ("split", 2): 4.38e-6, ("split", 3): 9.96e-7,
                 ("prefill4", 1): 2.76e-3}
assert all(v < CEILING[xs] for (_, xs), v in ATTN_MEASURED.items())
ATTN_BOUND = {k: 4 * v for k, v in ATTN_MEASURED.items()}
P = "lm.layers.0.self_attn."


class Eng:
    def __init__(self, geo, xs):
        self.geo, self.xs, self.cfg = geo, xs, ls.ATTN_GEO[geo]
        self.w = AC.readout_weights(self.cfg, "fused")
        self.loaded = ("fused", False)
        self.s = build_small(self.cfg, xsplit=xs, n_slots=ls.ATTN_SLOTS, max_ctx=ls.ATTN_MAX_CTX, max_rows=ls.ATTN_MAX_ROWS, lm_w=self.w)
        self.eng = self.s.eng
        assert self.eng.max_ctx == ls.ATTN_MAX_CTX

    def load(self, family, k_zero=False):
        """the q bias of the kernel family (its planted operand is a bf16 value in that family's units) and the k projection"""
        key = ("prefill4" if family == "prefill4" else "fused", k_zero)
        if key != self.loaded:
            self.w = AC.readout_weights(self.cfg, key[0], k_zero)
            for n in ("q_proj.bias", "k_proj.weight", "k_proj.bias"):
                self.eng.upload(P + n, self.w["layers.0.self_attn." + n])
            torch.cuda.synchronize()
            self.loaded = key


_engines = {}


@pytest.fixture(scope="module")
def engines():
    def get(geo, xs):
        if (geo, xs) not in _engines:
            _engines[(geo, xs)] = Eng(geo, xs)
        return _engines[(geo, xs)]
    yield get
    for e in _engines.values():
        e.eng.close()
    _engines.clear()


def dev(t, eng):
    out = t.to(eng.device).contiguous()
    torch.cuda.synchronize()
    return out


def export(eng, c):
    k, v = eng.kv_export(c, 0, 0, eng.max_ctx)
    eng.sync()
    return k.cpu(), v.cpu()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def place(E, eng, c, k, v):
    """cache c: NaN words in every slot, then the prefix k, v bf16 [Hkv, n, D]"""
    cfg = E.cfg
    nan = torch.full((cfg.kv_heads, eng.max_ctx, cfg.head_dim), float("nan"), dtype=torch.bfloat16)
    nan[:, :k.shape[1]] = k
    nv = nan.clone()
    nv[:, :v.shape[1]] = v
    with torch.cuda.stream(eng.stream):
        eng.kv_import(c, 0, dev(nan, eng), dev(nv, eng))
    eng.sync()


def run_pass(E, rows, x, eng=None, v_tail=False):
    """one launch, twice from the same state, with every check of the module docstring -> (got [T, H] fp32, {cache: (k, v) fp64})"""
    eng = eng or E.eng
    cfg = E.cfg
    H, T = cfg.hidden, len(rows)
    caches = sorted({c for c, _ in rows})
    before = {c: export(eng, c) for c in caches}
    xin = torch.full((T + 2, H), float("nan"))
    xin[1:T + 1] = x
    xin_d = dev(xin, eng)
    out0 = torch.full((T + 2, H), SENT)
    out_d = dev(out0, eng)
    snaps = []
    for rep in range(2):
        if rep:
            with torch.cuda.stream(eng.stream):
                for c in caches:
                    eng.kv_import(c, 0, dev(before[c][0], eng), dev(before[c][1], eng))
            eng.sync()
            out_d.copy_(out0)
            torch.cuda.synchronize()
        with torch.cuda.stream(eng.stream):
            eng.lm_forward_range(rows, xin_d[1:], out_d[1:], 0, 1, False)
        eng.sync()
        torch.cuda.synchronize()
        snaps.append((out_d.cpu(), {c: export(eng, c) for c in caches}))
    (o, after), (o2, after2) = snaps
    assert torch.equal(bits(o), bits(o2)), "two launches from one state differ"
    for c in caches:
        assert torch.equal(bits(after[c][0]), bits(after2[c][0])) and torch.equal(bits(after[c][1]), bits(after2[c][1])), "caches of two launches differ"
    assert torch.equal(bits(o[0]), bits(out0[0])) and torch.equal(bits(o[T + 1]), bits(out0[T + 1])), "guard rows changed"
    got = o[1:T + 1]
    assert bool(torch.isfinite(got).all()), "non-finite output"
    for c in caches:
        app = torch.tensor([p for cc, p in rows if cc == c])
        for which, (b, a) in enumerate(zip(before[c], after[c])):
            changed = (bits(a) != bits(b)).any(0).any(-1)
            allowed = torch.zeros_like(changed)
            allowed[app] = True
            if which == 1 and v_tail:
                end = int(app.max()) + 1
                tail = slice(end, min(eng.max_ctx, (end + 63) & ~63))
                allowed[tail] = True
                assert bool((a[:, tail].float() == 0).all()), "V slots between the chunk and the end of its stage are not zero"
            assert not bool((changed & ~allowed).any()), ("KV"[which], c, (changed & ~allowed).nonzero().flatten().tolist()[:8])
            assert bool(torch.isfinite(a[:, app].float()).all()), "non-finite appended K / V"
    return got, {c: (k.to(F64), v.to(F64)) for c, (k, v) in after.items()}


class Worst:
    def __init__(self, E, family):
        self.E, self.family, self.rel, self.mx, self.fails = E, family, 0.0, 0.0, []
        self.bound = ATTN_BOUND[(family, E.xs)]

    def judge(self, tag, rows, x, got, after):
        E = self.E
        ref, a, sc = AC.reference(E.w, E.cfg, E.xs, self.family, rows, x, after)
        rel, mx = R.row_head_errs(got.view(len(rows), E.cfg.heads, E.cfg.head_dim), ref, a)
        r, m = float(rel.max()), float(mx.max())
        self.rel, self.mx = max(self.rel, r), max(self.mx, m)
        if not (r <= self.bound and m <= 4 * self.bound):
            self.fails.append((tag, r, m))
        return sc

    def done(self):
        E = self.E
        print(f"ATTN {self.family} geo={E.geo} xs={E.xs}: worst per-(row, head) rel-L2 / a = {self.rel:.3e}, max / a = {self.mx:.3e} "
              f"(bounds {self.bound:.2e}, {4 * self.bound:.2e}; ceiling {CEILING[E.xs]:.2e})")
        assert not self.fails, self.fails[:10]


def planted_weight(sc, row, head, pos):
    return R.weight_of(sc[row][head], pos)


GEO_XS = [(g, xs) for g in ("A", "B") for xs in (1, 2, 3)]


# ---------------------------------------------------------------------------------------------- decode rows, one cache each
def decode_candidates(n, splits):
    """spike positions of a prefix of n positions: the prefix is placed once and the steps of a case may run with different split
    counts (a row crossing 1024 or 2048), so the block edges of EVERY split count the case's steps use are walked"""
    return AC.spike_candidates(n, [b for S in sorted(set(splits)) for b in AC.fused_ranges(n, S)]) if n else []


def decode_case(E, W, lens, eng, tag, design, variant, splits):
    cfg = E.cfg
    spikes = {}
    for c, n in enumerate(lens):
        cand = decode_candidates(n, splits)
        sp = [cand[(c + kvh + variant) % len(cand)] for kvh in range(cfg.kv_heads)] if cand else None
        spikes[c] = sp
        k, v = AC.prefix(cfg, n, design if design != "own" else "random", "fused", 1000 * variant + 17 * c + n, spikes=sp)
        place(E, eng, c, k, v)
    for step in range(ls.ATTN_DECODE_STEPS):
        rows = [(c, n + step) for c, n in enumerate(lens)]
        x = AC.x_rows(cfg, len(rows), 50 + step + variant, own=range(len(rows)) if design == "own" else ())
        got, after = run_pass(E, rows, x, eng)
        sc = W.judge((tag, design, variant, step), rows, x, got, after)
        for c, n in enumerate(lens):
            for kvh in range(cfg.kv_heads):
                h = AC.plus_head(cfg, kvh)
                if design == "spike" and spikes[c]:
                    assert planted_weight(sc, c, h, spikes[c][kvh]) >= 0.5, (tag, c, kvh, spikes[c])
                if design == "own":
                    assert sum(planted_weight(sc, c, h, n + s) for s in range(step + 1)) >= 0.5, (tag, c, kvh)
            if n + step == 0:
                # a row with nothing but its own token: the output is x + the exported V of that token
                vnew = torch.cat([after[c][1][h // (cfg.heads // cfg.kv_heads), 0] for h in range(cfg.heads)])
                want = x[c].float() + vnew.float()
                if E.xs == 3:
                    assert torch.equal(got[c], want), (tag, "length 0")
                else:
                    assert bool(((got[c].double() - x[c].double() - vnew).abs() <= 2.0 ** -9 * vnew.abs() + 1e-6).all()), (tag, "length 0")


@pytest.mark.parametrize("case", list(ls.ATTN_DECODE_LENS) + ["cap"])
@pytest.mark.parametrize("geo,xs", GEO_XS)
def test_fused_decode(engines, geo, xs, case):
    """Rows on distinct caches, three steps each: 1, 2, 6, 16 rows and a mix of one- and two-block rows beside a three-split row
    (lm_shapes.ATTN_DECODE_LENS); "cap": attn_splits = 2 capping the split count of a 2100-position row."""
    E = engines(geo, xs)
    E.load("fused")
    W = Worst(E, "fused")
    eng, lens, splits = E.eng, ls.ATTN_DECODE_LENS.get(case), None
    try:
        if case == "cap":
            eng, lens, splits = E.eng.fork(attn_splits=2), ls.ATTN_DECODE_CAPPED, [2]
        else:
            splits = ls.ATTN_DECODE_SPLITS[case]
        n_var = max(len(decode_candidates(n, splits)) for n in lens)
        for design, variants in (("random", 1), ("sink", 1), ("own", 1), ("spike", n_var)):
            for v in range(variants):
                decode_case(E, W, lens, eng, case, design, v, splits)
    finally:
        if eng is not E.eng:
            eng.close()
    W.done()


# ---------------------------------------------------------------------------------------------- rows that share a cache: split + merge
def span_case(E, W, rows, tag, design, variant, own=()):
    cfg = E.cfg
    first = {}
    for c, p in rows:
        first.setdefault(c, p)
    S = max(p for _, p in rows) // 1024 + 1
    spikes = {}
    for c, n in first.items():
        cand = AC.spike_candidates(n, AC.chunk_ranges(n + 1, S)) if n else []
        sp = [cand[(kvh + variant) % len(cand)] for kvh in range(cfg.kv_heads)] if cand else None
        spikes[c] = sp
        k, v = AC.prefix(cfg, n, design if design != "own" else "random", "split", 2000 * variant + 13 * c + n, spikes=sp)
        place(E, E.eng, c, k, v)
    x = AC.x_rows(cfg, len(rows), 70 + variant, own=own)
    got, after = run_pass(E, rows, x)
    sc = W.judge((tag, design, variant), rows, x, got, after)
    for kvh in range(cfg.kv_heads):
        h = AC.plus_head(cfg, kvh)
        for i, (c, p) in enumerate(rows):
            if design == "spike" and spikes[c]:
                assert planted_weight(sc, i, h, spikes[c][kvh]) >= 0.5, (tag, i, kvh, spikes[c])
        if design == "own":
            pos = {i: p for i, (c, p) in enumerate(rows)}
            for i in own:       # the own rows a row sees (itself included) hold most of its weight
                seen = [pos[j] for j in own if rows[j][0] == rows[i][0] and pos[j] <= pos[i]]
                assert sum(planted_weight(sc, i, h, p) for p in seen) >= 0.5, (tag, i, kvh)


def n_variants(n, S):
    return len(AC.spike_candidates(n, AC.chunk_ranges(n + 1, S))) if n else 0


@pytest.mark.parametrize("geo,xs", GEO_XS)
def test_split_merge(engines, geo, xs):
    """Rows sharing a cache through vv_rope_append + vv_attn_split + vv_attn_merge: spans of 2, 5 and 7 rows at 0, 30, 510, 1020 and
    2046 (one, two and three splits; the spans at 1020 and 2046 cross a split count); a 5-row span at 6 beside a row at 1500 on
    another cache (a one-split row inside a two-split launch at the 512-position floor); exact modes: a 70-row chunk at 1000 (two
    launches of the pair).  own: every row's own K carries the planted logit, so each row's diagonal neighbour does too."""
    E = engines(geo, xs)
    E.load("split")
    W = Worst(E, "split")
    for n, p0 in ls.ATTN_SPANS:
        rows = ls.span(0, p0, n)
        S = (p0 + n - 1) // 1024 + 1
        for design, variants in (("random", 1), ("sink", 1 if p0 else 0), ("own", 1), ("spike", n_variants(p0, S) if n == 5 else min(2, n_variants(p0, S)))):
            for v in range(variants):
                span_case(E, W, rows, (n, p0), design, v + n, own=range(n) if design == "own" else ())
    for design, variants in (("random", 1), ("own", 1), ("spike", n_variants(1500, 2))):
        for v in range(variants):
            span_case(E, W, ls.ATTN_SHORT_LONG, "short+long", design, v, own=range(len(ls.ATTN_SHORT_LONG)) if design == "own" else ())
    if xs != 1:
        n, p0 = ls.ATTN_EXACT_CHUNK
        for design, variants in (("random", 1), ("own", 1), ("spike", 4)):
            for v in range(variants):
                span_case(E, W, ls.span(0, p0, n), "chunk", design, v, own=(0, 33, 63, 64, n - 1) if design == "own" else ())
    W.done()


# ---------------------------------------------------------------------------------------------- vv_attn_prefill4 (bf16 mode)
def prefill_spikes(p0):
    """prefix positions worth a spike: pos0 - 1 (the first row's diagonal neighbour), 0, and both sides of the first and last 64-position
    stage edge below the chunk"""
    last = (p0 // 64) * 64
    out = []
    for p in (p0 - 1, 0, 63, 64, last - 1, last, p0 - 2):
        if 0 <= p < p0 and p not in out:
            out.append(p)
    return out


@pytest.mark.parametrize("p0", sorted({p for _, p in ls.ATTN_CHUNKS}))
@pytest.mark.parametrize("geo", ["A", "B"])
def test_prefill4(engines, geo, p0):
    """Chunks of 8, 20, 63, 64, 100 and 150 consecutive rows at one position, bf16 mode (lm_shapes.ATTN_CHUNKS).  Every row of
    attn_cases.own_rows is an own row once per chunk: 0, 63 | 64, 127 | 128 (the 64-row tile edges, where qt_lo / qt_hi /
    first_masked / pend of a workgroup change and, in geometry B, one workgroup straddles both tiles), 5, 77 and the last row."""
    E = engines(geo, 1)
    E.load("prefill4")
    W = Worst(E, "prefill4")
    cfg = E.cfg
    heads = [AC.plus_head(cfg, kvh) for kvh in range(cfg.kv_heads)]
    for ci, (n, _) in enumerate([c for c in ls.ATTN_CHUNKS if c[1] == p0]):
        rows = ls.span(0, p0, n)
        cand = prefill_spikes(p0)
        runs = [("random", None, ()), ("sink", None, ())] if p0 else [("random", None, ())]
        runs += [("spike", cand[(ci + i) % len(cand)], ()) for i in range(min(3, len(cand)))]
        runs += [("own", None, (j0,)) for j0 in AC.own_rows(n)]          # every one of them, one own row per pass
        if p0:
            runs += [("ramp", None, ())]
        for design, spike, own in runs:
            sp = [spike] * cfg.kv_heads if spike is not None else None
            k, v = AC.prefix(cfg, p0, design if design != "own" else "random", "prefill4", 3000 + 7 * n + p0, spikes=sp)
            place(E, E.eng, 0, k, v)
            x = AC.x_rows(cfg, n, 90 + n, own=own)
            got, after = run_pass(E, rows, x, v_tail=True)
            # branch reach, from the reference alone, before the comparison
            _, _, sc = AC.reference(E.w, cfg, 1, "prefill4", rows, x, after)
            if design == "ramp":
                # counted over the stages that lie wholly inside the prefix, where the design sets the scores (the chunk's own
                # K carries no ramp: its stages are random-score territory for both heads)
                up = [len([s for s in R.rebase_stages(sc[j][0]) if s < p0 // 64]) for j in range(n)]
                down = [len([s for s in R.rebase_stages(sc[j][1]) if s < p0 // 64]) for j in range(n)]
                assert max(down) == 0, (n, p0, down)
                if p0 >= 1000:
                    assert min(up) >= 4, (n, p0, up)
            if design == "own":
                j0 = own[0]
                st = (p0 + j0) // 64
                for h in heads:
                    assert planted_weight(sc, j0, h, p0 + j0) >= 0.5, (n, p0, j0, h)
                # the causal edge at the own row, across a 16-row (and, for 64 and 128, a 64-row) tile edge as well: the 16 rows
                # before it do not see its K and do not re-base in its stage, the rows of its own 16-row tile from it on do
                near = range(max(0, j0 - 16), min(n, 16 * (j0 // 16) + 16))
                assert all(planted_weight(sc, j, 0, p0 + j0) == 0.0 for j in near if j < j0), (n, p0, j0)
                if st > 0:
                    assert all((st in R.rebase_stages(sc[j][0])) == (j >= j0) for j in near), (n, p0, j0)
            if design == "spike":
                for h in heads:
                    assert planted_weight(sc, 0, h, spike) >= 0.5, (n, p0, spike, h)
            W.judge((n, p0, design, spike, own), rows, x, got, after)
    W.done()


# ---------------------------------------------------------------------------------------------- the three K-append paths
def check_append(E, tag, rows, x, after, v_mode, fails, stats):
    """exported K / V of the appended positions against the fp64 projection rounded to bf16"""
    cfg = E.cfg
    pos = torch.tensor([p for _, p in rows])
    kref, vref = AC.project_kv(E.w, cfg, x, pos)                           # [Hkv, T, D]
    kb = E.w["layers.0.self_attn.k_proj.bias"].view(1, cfg.kv_heads, cfg.head_dim).expand(len(rows), -1, -1).transpose(0, 1)
    kgot = torch.stack([after[c][0][:, p] for c, p in rows], 1)            # [Hkv, T, D]
    vgot = torch.stack([after[c][1][:, p] for c, p in rows], 1)
    steps, flat = R.rotated_k_steps(kgot, kref, kb)
    off = float((steps > 0).double().mean())
    if int(steps.max()) > 1 or off > 0.01:
        fails.append((tag, "K", int(steps.max()), off))
    if v_mode == "exact":
        # bit-exact wherever the projection's fp32 accumulation cannot reach a rounding boundary: the exact mode's operand terms carry
        # all 24 bits, so what separates the device's V from the fp64 one is the accumulation of H <= 896 fp32 terms of random sign:
        # each partial sum (of the size of the terms' 2-norm, or of the result) is rounded to 2^-24 of itself and the roundings add
        # like a random walk, sqrt(H) 2^-24 <= 2^-19.  An element whose fp64 value lies nearer than 2^-19 (|v| + ||terms||_2) to the
        # midpoint of two bf16 values may land on either side (one step); every other element must match bit for bit
        u = R.bf16_ulps(vgot, vref.float())
        # 2^-19 is this MODEL of the accumulation (a random walk over at most 1024 roundings), not a measured figure
        reach = 2.0 ** -19 * (vref.abs() + AC.v_term_norm(E.w, cfg, x))
        near = R.bf16_boundary_distance(vref.float()) * vref.abs() <= reach
        # ... and no element is farther from the fp64 value than that reach plus the rounding of the store (half a bf16 step of the
        # stored value, a little over half a step of the reference: 0.51): where the projection cancels to a small value the reach is
        # several of ITS bf16 steps, so the near elements are held in absolute terms, not in steps
        step = torch.pow(2.0, torch.floor(torch.log2(vref.abs().clamp_min(1e-300))) - 7)
        far = (vgot - vref).abs() > reach + 0.51 * step
        if int(u[~near].max()) > 0 or bool(far.any()):
            fails.append((tag, "V", int(u[~near].max()), int(far.sum()), int(u.max()), float((u > 0).double().mean()), float(near.double().mean())))
        stats["v_off"] = max(stats.get("v_off", 0.0), float((u > 0).double().mean()))
        stats["v_near"] = max(stats.get("v_near", 0.0), float(near.double().mean()))
    elif v_mode == "gemv":
        # the GEMV's own operand rounding (tests/gemv_ref.py: RMS prologue, bf16 weights), then one bf16 rounding of the result
        p = "layers.0."
        pro = gemv_ref.pro_rms(x, E.w[p + "input_layernorm.weight"], cfg.eps, E.xs)
        vr = gemv_ref.epi_bias(gemv_ref.product(pro, gemv_ref.weights(E.w[p + "self_attn.v_proj.weight"])), E.w[p + "self_attn.v_proj.bias"])
        vr = vr.view(len(rows), cfg.kv_heads, cfg.head_dim).transpose(0, 1)
        u = R.bf16_ulps(vgot, vr.float())
        if int(u.max()) > 1 or float((u > 0).double().mean()) > 0.01:
            fails.append((tag, "V", int(u.max()), float((u > 0).double().mean())))
    return off


@pytest.mark.parametrize("geo,xs", GEO_XS)
def test_append_exact(engines, geo, xs):
    """k_proj.weight = 0: the appended K is RoPE(k_proj.bias) at the row's position and nothing else.  One decode step per position
    class (six rows in one launch -- the packed batch route in the bf16 mode -- and each alone: vv_attn_fused_kernel's table RoPE and
    knew / vnew), a 5-row span (vv_rope_append_kernel, trigonometric) and chunks of 64 and 150 rows (the packed prefill's QKV GEMM +
    vv_rope_append in the bf16 mode), at 0, 37 and 2040.  The RoPE epilogue of vv_gemm4 needs a QKV width that is a multiple of 256
    and 256 workgroups of 256 x 256 tiles -- about 8000 rows at a 2048-wide QKV -- out of reach of this file's geometries:
    test_gpu_attn_long.py::test_qkv_rope_epilogue_append reaches it with a thin layer whose QKV is 4608 wide (3600 rows).
    Exported K: never more than one bf16 step from the fp64 rotation rounded to bf16 and at most 1 % of the elements off at all
    (attn_ref.rotated_k_steps; the reference's own fp32 form stays under a quarter of that, test_attn_ref_cpu.py).
    Exported V at xs = 3: bit-exact against the fp64 projection rounded to bf16, but for the elements whose fp64 value lies within
    the projection's own fp32 accumulation error of a rounding boundary (check_append), which may land on the other side and are held
    to that error in absolute terms -- measured: 2 of 8192 elements of the 64-row chunk of geometry A, 6 of 19,200 of the 150-row
    chunk of B, all among the 0.6 % that near; no append path can do better over an fp32 projection.
    At xs = 1 on the GEMV routes (single rows, the 5-row span): within one bf16 step of gemv_ref's form of the projection (bf16
    operands, the same on both sides), 1 % off at most.  The packed routes (16-row batch, packed prefill) round the normalised row at
    another point, and the xs = 2 GEMV carries 16 bits of the operand where gemv_ref carries all 24 (a 5-row span of geometry B: 5
    of 640 elements off, by up to two steps) -- neither is gemv_ref's form, so there the check is K only."""
    E = engines(geo, xs)
    E.load("fused", k_zero=True)
    cfg, eng = E.cfg, E.eng
    fails, worst, stats = [], 0.0, {}
    vm = {1: "gemv", 2: None, 3: "exact"}[xs]          # the V check of the GEMV routes
    sets = [("decode6", list(enumerate(ls.ATTN_APPEND_DECODE)), "exact" if xs == 3 else None)]
    sets += [(f"decode@{p}", [(0, p)], vm) for p in ls.ATTN_APPEND_DECODE]
    sets += [(f"span@{p0}", ls.span(0, p0, ls.ATTN_APPEND_SPAN), vm) for p0 in ls.ATTN_APPEND_POS0]
    sets += [(f"chunk{n}@{p0}", ls.span(0, p0, n), "exact" if xs == 3 else None) for n in ls.ATTN_APPEND_CHUNKS for p0 in ls.ATTN_APPEND_POS0]
    for tag, rows, v_mode in sets:
        first = {}
        for c, p in rows:
            first.setdefault(c, p)
        for c, n in first.items():
            place(E, eng, c, *AC.prefix(cfg, n, "random", "fused", 4000 + n))
        x = AC.x_rows(cfg, len(rows), 95 + len(rows))
        chunk = xs == 1 and len(rows) >= 8 and len(first) == 1
        got, after = run_pass(E, rows, x, v_tail=chunk)
        worst = max(worst, check_append(E, tag, rows, x, after, v_mode, fails, stats))
    print(f"ATTN append geo={geo} xs={xs}: worst share of K elements one bf16 step off = {worst:.4%} (cap 1 %)" +
          (f"; V: {stats['v_off']:.4%} off, all among the {stats['v_near']:.4%} within 2^-19 of a rounding boundary" if stats else ""))
    assert not fails, fails
