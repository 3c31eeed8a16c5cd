"""The attention paths of test_gpu_attn_paths.py at the contexts the product decodes at -- 32K positions in 32 splits, 64K in 64 --
against the same fp64 reference (tests/attn_ref.py), per (row, head), with every check of that file's run_pass (guard rows, NaN
slots past every prefix, only the appended positions changed, two launches bit-identical).  The short file stops at 2304 positions
and three splits; what runs only beyond that:

  vv_attn_merge2_kernel   eight partials per thread group at once: the live mask, the redirect of dead slots, the second and third
                          outer iteration and their rescale (64, 67, 15 and 29 splits: lm_shapes.ATTN_LONG_DECODE_SPLITS)
  vv_attn_fused_kernel    a workgroup stride of 8K-16K positions, the owner split among 64, rows with used < S beside used == S
  vv_attn_split / merge   positions per split far above the 512 floor (2560 to 30,080)
  vv_attn_prefill4        500 to 1000 stages before the chunk
  RoPE at large angles    cosf in vv_rope_append_kernel, the table of vv_rope_table_kernel, and that table as the VV_EPI_QKV_ROPE
                          epilogue of vv_gemm4 reads it (test_qkv_rope_epilogue_append: a thin layer whose QKV GEMM has 270 tiles)
  cache offsets >= 2^31   test_far_cache_offsets: caches that start at element 2^31 of the K and V arrays

Which kernels and how many splits every row set runs is asserted on the CPU (test_pass_plan_cpu.py, test_prefill_plan_cpu.py) from
the same data (lm_shapes.ATTN_LONG_*, QKV_ROPE_*, FAR_*); what the designs are worth -- the loss of any one split or block moves the
reference beyond the bound -- in test_attn_ref_cpu.py (e).

The long engines are engines of their own (never a fork of a short one) and hold attn_cases.long_inv_freq: the model's RoPE table
with its last entry at 0, so that the pair carrying the planted logits does not rotate and the planted operand stays a bf16 value at
every position; the reference reads the same table from the weight dict.  Designs beyond the short file's: comb (one planted
position per split of the launch, each with a V dimension of its own) and the tail ramp (the last 1024 prefix positions).

Bounds.  ATTN_MEASURED_LONG: the worst normalised per-(row, head) rel-L2 against the fp64 reference over every case of a kernel
family and mode of THIS file on an MI355X, rounded up in the third digit; bound = 4 x that, max-error bound = 4 x the rel-L2 bound
(the short file's rule).  Every test prints its worst value beside the bound (run with -s).  The ceilings are the short file's
conditions, not measurements.  No bound comes from another attention launch or from the short-context figures."""
import types

import pytest
import torch

import attn_cases as AC
import attn_ref as R
import lm_shapes as ls
import synth
from gpu_util import build_small
from test_gpu_attn_paths import CEILING, Eng, Worst, check_append, export, bits, dev, place, planted_weight, run_pass

pytestmark = pytest.mark.gpu

F64 = torch.float64
# Worst per-(row, head) rel-L2 / ||a|| against the fp64 reference over every case of this file, per kernel family and mode, on an
# MI355X (2026-10-21, libvvhip build 4a93b26e79c81a21; both geometries, test_far_cache_offsets included), rounded up in the third digit:
#   fused (+ merge2)   xs 1: 3.562e-03   xs 2: 4.996e-06   xs 3: 1.222e-06
#   split + merge      xs 1: 2.286e-03   xs 2: 4.454e-06   xs 3: 2.418e-06
#   prefill4           xs 1: 2.458e-03
# all under their ceilings (7.81e-03, 3.05e-05, 2e-05); the worst max-error seen is 3.9e-03 / 7.3e-06 / 3.6e-06.  The exact mode's fp32
# accumulation over 2000 blocks stays at 1.2e-06 (fused, 64 splits) and 2.4e-06 (split + merge, 30,080 positions per split) of a.
# The fused bf16 figure is L16's (geometry A), with max / a = 3.65e-03 beside it: the error sits in ONE dimension.  That is what a
# short row of the comb design gives -- its V lives in one dimension, so the packed route's bf16 rounding of the output (up to 2^-8
# of a value just above a power of two) is the whole row's error; which row it was has not been read out.  The sets of long rows
# alone sit at 1.9e-03 to 2.7e-03, where two bf16 roundings of 2^-9 put them.  The caches past element 2^31 (test_far_cache_offsets)
# measured 1.0e-03 / 1.4e-06 / 3.9e-07 (fused) and 1.2e-03 / 1.9e-06 / 4.1e-07 (split + merge), 3.2e-04 (prefill4).
ATTN_MEASURED_LONG = {("fused", 1): 3.57e-3, ("fused", 2): 5.00e-6, ("fused", 3): 1.23e-6,
                      ("split", 1): 2.29e-3, ("split", 2): 4.46e-6, ("split", 3): 2.42e-6,
                      ("prefill4", 1): 2.46e-3}
assert all(v < CEILING[xs] for (_, xs), v in ATTN_MEASURED_LONG.items())
ATTN_BOUND_LONG = {k: 4 * v for k, v in ATTN_MEASURED_LONG.items()}
GEO_XS = [(g, xs) for g in ("A", "B") for xs in (1, 2, 3)]


class LongEng(Eng):
    """a fresh engine of a geometry and mode over the readout layer (layer `layer` of cfg) on attn_cases.long_inv_freq"""

    def __init__(self, geo, xs, cfg=None, layer=0, n_slots=ls.ATTN_LONG_SLOTS, max_ctx=ls.ATTN_LONG_MAX_CTX, max_rows=ls.ATTN_LONG_MAX_ROWS):
        self.geo, self.xs, self.cfg, self.layer = geo, xs, cfg or ls.ATTN_GEO[geo], layer
        self.invf = AC.long_inv_freq(self.cfg.head_dim, self.cfg.theta)
        self.w = AC.readout_weights(self.cfg, "fused", layer=layer, inv_freq=self.invf)
        self.loaded = ("fused", False)
        self.s = build_small(self.cfg, xsplit=xs, n_slots=n_slots, max_ctx=max_ctx, max_rows=max_rows, lm_w=self.w)
        self.eng = self.s.eng
        assert self.eng.max_ctx == max_ctx
        self.eng.upload("lm.rope.inv_freq", self.invf)
        torch.cuda.synchronize()

    def load(self, family, k_zero=False):
        """as Eng.load, and the RoPE table again: the table of every position is rebuilt from it before the next decode step"""
        key = ("prefill4" if family == "prefill4" else "fused", k_zero)
        if key != self.loaded:
            self.w = AC.readout_weights(self.cfg, key[0], k_zero, layer=self.layer, inv_freq=self.invf)
            for n in ("q_proj.bias", "k_proj.weight", "k_proj.bias"):
                self.eng.upload(f"lm.layers.{self.layer}.self_attn.{n}", self.w[f"layers.{self.layer}.self_attn.{n}"])
            self.eng.upload("lm.rope.inv_freq", self.invf)
            torch.cuda.synchronize()
            self.loaded = key


_engines = {}


@pytest.fixture(scope="module")
def engines():
    def get(geo, xs):
        if (geo, xs) not in _engines:
            _engines[(geo, xs)] = LongEng(geo, xs)
        return _engines[(geo, xs)]
    yield get
    for e in _engines.values():
        e.eng.close()
    _engines.clear()


class LongWorst(Worst):
    def __init__(self, E, family):
        self.E, self.family, self.rel, self.mx, self.fails = E, family, 0.0, 0.0, []
        self.bound = ATTN_BOUND_LONG[(family, E.xs)]

    def judge(self, tag, rows, x, got, after):
        E = self.E
        ref, a, sc = AC.reference(E.w, E.cfg, E.xs, self.family, rows, x, after, layer=E.layer)
        rel, mx = R.row_head_errs(got.view(len(rows), E.cfg.heads, E.cfg.head_dim), ref, a)
        r, m = float(rel.max()), float(mx.max())
        self.rel, self.mx = max(self.rel, r), max(self.mx, m)
        if not (r <= self.bound and m <= 4 * self.bound):
            self.fails.append((tag, r, m))
        return sc


def plus_heads(cfg):
    return [AC.plus_head(cfg, kvh) for kvh in range(cfg.kv_heads)]


# ---------------------------------------------------------------------------------------------- decode rows, one cache each
def decode_spikes(n, S, D):
    """the six spike placements of a decode row over a prefix of n positions in a launch of S splits (None: no prefix): the first and
    the last block of split 0, the last block of the last used split, a block of a split that vv_attn_merge2 reads in its second
    outer iteration (the last used split where there is none), the block before the owner's, position n - 1"""
    if n == 0:
        return [None] * 6
    blocks = R.fused_split_blocks(n + 1, S)
    used = len(blocks)
    s2 = min(8 * (512 // D) + 1, used - 1)
    first2, last2 = blocks[s2]
    mid2 = first2 + S * (((last2 - first2) // S) // 2)
    cand = [31, 32 * blocks[0][1] + 31, 32 * blocks[-1][1] + 31, 32 * mid2 + 9, 32 * ((n >> 5) - 1) + 17, n - 1]
    return [min(max(p, 0), n - 1) for p in cand]


DECODE_SPIKES = {"L1": (0, 1, 2, 3, 4, 5), "L1x": (0, 1, 2, 3, 4, 5), "L2": (0, 2, 5), "L6": (3, 4), "Lcap": (1, 3, 5)}


def long_decode_case(E, W, lens, eng, tag, design, variant, S, steps=1):
    cfg = E.cfg
    planted = {}
    for c, n in enumerate(lens):
        sp = None
        if design == "comb":
            sp = AC.comb_fused(n, S)
        elif design == "spike" and n:
            sp = [decode_spikes(n, S, cfg.head_dim)[variant]] * cfg.kv_heads
        planted[c] = sp
        k, v = AC.prefix(cfg, n, design if design != "own" else "random", "fused", AC.LONG_SEED + 1000 * variant + 17 * c + n, spikes=sp)
        place(E, eng, c, k, v)
    for step in range(steps):
        rows = [(c, n + step) for c, n in enumerate(lens)]
        x = AC.x_rows(cfg, len(rows), 50 + step + variant, own=range(len(rows)) if design == "own" else ())
        got, after = run_pass(E, rows, x, eng)
        sc = W.judge((tag, design, variant, step), rows, x, got, after)
        for c, n in enumerate(lens):
            for h in plus_heads(cfg):
                if design == "spike" and planted[c]:
                    assert planted_weight(sc, c, h, planted[c][0]) >= 0.5, (tag, c, h, planted[c])
                if design == "comb" and planted[c]:
                    assert sum(planted_weight(sc, c, h, p) for p in planted[c]) >= 0.5, (tag, c, h)
                if design == "own":
                    assert sum(planted_weight(sc, c, h, n + s) for s in range(step + 1)) >= 0.5, (tag, c, h)


@pytest.mark.parametrize("case", list(ls.ATTN_LONG_DECODE_LENS) + ["Lcap"])
@pytest.mark.parametrize("geo,xs", GEO_XS)
def test_fused_decode_long(engines, geo, xs, case):
    """Decode rows on distinct caches at 64 and 67 splits, long rows beside short ones, and attn_splits = 8 capping a 65,000-position
    row (lm_shapes.ATTN_LONG_DECODE_LENS).  random, sink, comb: one step; own: two steps, the second reads the first's append; spike:
    decode_spikes, up to six placements (DECODE_SPIKES); L16: random and comb only."""
    E = engines(geo, xs)
    E.load("fused")
    W = LongWorst(E, "fused")
    eng = E.eng
    try:
        if case == "Lcap":
            eng, lens, S = E.eng.fork(attn_splits=ls.ATTN_LONG_CAP), ls.ATTN_LONG_DECODE_CAPPED, ls.ATTN_LONG_CAP
        else:
            lens, S = ls.ATTN_LONG_DECODE_LENS[case], ls.ATTN_LONG_DECODE_SPLITS[case][geo]
        runs = [("random", 0, 1), ("comb", 0, 1)]
        if case != "L16":
            runs += [("sink", 0, 1), ("own", 0, 2)] + [("spike", v, 1) for v in DECODE_SPIKES[case]]
        for design, variant, steps in runs:
            long_decode_case(E, W, lens, eng, case, design, variant, S, steps)
    finally:
        if eng is not E.eng:
            eng.close()
    W.done()


# ---------------------------------------------------------------------------------------------- rows that share a cache: split + merge
def long_span_case(E, W, rows, S, tag, design, variant, own=()):
    cfg = E.cfg
    first = {}
    for c, p in rows:
        first.setdefault(c, p)
    planted = {}
    for c, n in first.items():
        sp = None
        if design == "comb":
            sp = AC.comb_chunks(n, S)
        elif design == "spike":
            # both sides of a split edge of the first row: the last position of split 0, the first of the last split
            rng = R.split_ranges(n + 1, S)
            sp = [min((rng[0][1] - 1, rng[-1][0])[variant], n - 1)] * cfg.kv_heads
        planted[c] = sp
        k, v = AC.prefix(cfg, n, design if design != "own" else "random", "split", AC.LONG_SEED + 2000 * variant + 13 * c + n, spikes=sp)
        place(E, E.eng, c, k, v)
    x = AC.x_rows(cfg, len(rows), 70 + variant, own=own)
    got, after = run_pass(E, rows, x)
    sc = W.judge((tag, design, variant), rows, x, got, after)
    pos = {i: p for i, (c, p) in enumerate(rows)}
    for h in plus_heads(cfg):
        for i, (c, p) in enumerate(rows):
            if design == "spike":
                assert planted_weight(sc, i, h, planted[c][0]) >= 0.5, (tag, i, h, planted[c])
            if design == "comb":
                assert sum(planted_weight(sc, i, h, q) for q in planted[c]) >= 0.5, (tag, i, h)
        if design == "own":
            for i in own:       # the own rows a row sees (itself included) hold most of its weight
                seen = [pos[j] for j in own if rows[j][0] == rows[i][0] and pos[j] <= pos[i]]
                assert sum(planted_weight(sc, i, h, q) for q in seen) >= 0.5, (tag, i, h)


@pytest.mark.parametrize("geo,xs", GEO_XS)
def test_split_merge_long(engines, geo, xs):
    """Spans of 5, 2 and 7 rows of one cache at 64,990, 32,767 and 65,530 (19 to 52 splits of 1280 to 3456 positions), a 5-row span at
    6 beside a row at 65,000 of another cache (one-split rows in a 64-split launch), and in the exact modes a 70-row chunk at 60,000
    (two launches of the pair, 30,080 and 15,104 positions per split).  random, own, comb and a spike on either side of a split edge."""
    E = engines(geo, xs)
    E.load("split")
    W = LongWorst(E, "split")
    sets = [((n, p0), ls.span(0, p0, n), ls.ATTN_LONG_SPAN_SPLITS[(n, p0)][geo], range(n)) for n, p0 in ls.ATTN_LONG_SPANS]
    sets.append(("short+long", list(ls.ATTN_LONG_SHORT_LONG), ls.ATTN_LONG_SHORT_LONG_SPLITS[geo], range(len(ls.ATTN_LONG_SHORT_LONG))))
    if xs != 1:
        n, p0 = ls.ATTN_LONG_EXACT_CHUNK
        sets.append(("chunk", ls.span(0, p0, n), ls.ATTN_LONG_EXACT_CHUNK_SPLITS[geo], (0, 33, 63, 64, n - 1)))
    for tag, rows, S, own in sets:
        for design, variant in (("random", 0), ("own", 0), ("comb", 0), ("spike", 0), ("spike", 1)):
            long_span_case(E, W, rows, S, tag, design, variant, own=own if design == "own" else ())
    W.done()


# ---------------------------------------------------------------------------------------------- vv_attn_prefill4 (bf16 mode)
def long_prefill_spikes(p0):
    """p0 - 1 (the first row's diagonal neighbour), 0, and both sides of the last 64-position stage edge below the chunk"""
    edge = ((p0 - 1) // 64) * 64
    return [p0 - 1, 0, edge - 1, edge]


@pytest.mark.parametrize("chunk", ls.ATTN_LONG_CHUNKS, ids=lambda c: f"{c[0]}@{c[1]}")
@pytest.mark.parametrize("geo", ["A", "B"])
def test_prefill4_long(engines, geo, chunk):
    """Chunks of 8, 20, 64 and 150 rows behind 500 to 1000 stages of prefix, bf16 mode.  random, sink, the tail ramp (the up-ramp head
    re-bases in at least four of the last 16 prefix stages, the down-ramp head in none of them), four spikes, own rows 0, 63 and the last;
    the 150-row chunk (its fp64 reference costs seconds) runs random, the ramp and own row 64 alone."""
    E = engines(geo, 1)
    E.load("prefill4")
    W = LongWorst(E, "prefill4")
    cfg = E.cfg
    n, p0 = chunk
    rows = ls.span(0, p0, n)
    if n >= 128:
        runs = [("random", None, ()), ("tail", None, ()), ("own", None, (64,))]
    else:
        runs = [("random", None, ()), ("sink", None, ()), ("tail", None, ())] + [("spike", p, ()) for p in long_prefill_spikes(p0)]
        runs += [("own", None, (j,)) for j in sorted({0, 63, n - 1}) if j < n]
    for design, spike, own in runs:
        sp = [spike] * cfg.kv_heads if spike is not None else None
        k, v = AC.prefix(cfg, p0, design if design != "own" else "random", "prefill4", AC.LONG_SEED + 3000 + 7 * n + p0, spikes=sp)
        place(E, E.eng, 0, k, v)
        x = AC.x_rows(cfg, n, 90 + n, own=own)
        got, after = run_pass(E, rows, x, v_tail=True)
        sc = W.judge((n, p0, design, spike, own), rows, x, got, after)
        # branch reach, from the reference alone
        if design == "tail":
            assert float(k.float().abs().max()) <= 64.0
            last16 = range(p0 // 64 - 16, p0 // 64)
            for j in sorted({0, n // 2, n - 1}):
                assert len([s for s in R.rebase_stages(sc[j][0]) if s in last16]) >= 4, (n, p0, j)
                assert not [s for s in R.rebase_stages(sc[j][1]) if s in last16], (n, p0, j)
        if design == "own":
            j0 = own[0]
            for h in plus_heads(cfg):
                assert planted_weight(sc, j0, h, p0 + j0) >= 0.5, (n, p0, j0, h)
            assert all(planted_weight(sc, j, 0, p0 + j0) == 0.0 for j in range(max(0, j0 - 16), j0)), (n, p0, j0)
        if design == "spike":
            for h in plus_heads(cfg):
                assert planted_weight(sc, 0, h, spike) >= 0.5, (n, p0, spike, h)
    W.done()


# ---------------------------------------------------------------------------------------------- the K-append paths at large angles
@pytest.mark.parametrize("geo,xs", GEO_XS)
def test_append_exact_long(engines, geo, xs):
    """test_append_exact at 4095, 4096, 32,767, 32,768, 65,535 and 69,631 (the last position of the context): k_proj.weight = 0, the
    appended K is RoPE(k_proj.bias) alone.  All six decode steps in one launch and each alone (vv_rope_table_kernel's table as
    vv_attn_fused_kernel reads it), 5-row spans at 32,766 and 65,534 (vv_rope_append_kernel's cosf of an angle of up to 65,538 rad),
    chunks of 64 and 150 rows at 65,000 (the packed prefill in the bf16 mode).  Same criteria as test_append_exact: exported K never
    more than one bf16 step from the fp64 rotation of the fp32 angle and at most 1 % of the elements off (the reference's own fp32
    form stays under a quarter of that at these positions: test_attn_ref_cpu.py::test_append_flip_cap_long); the V checks per mode."""
    E = engines(geo, xs)
    E.load("fused", k_zero=True)
    cfg, eng = E.cfg, E.eng
    fails, worst, stats = [], 0.0, {}
    vm = {1: "gemv", 2: None, 3: "exact"}[xs]
    sets = [("decode6", list(enumerate(ls.ATTN_LONG_APPEND_DECODE)), "exact" if xs == 3 else None)]
    sets += [(f"decode@{p}", [(0, p)], vm) for p in ls.ATTN_LONG_APPEND_DECODE]
    sets += [(f"span@{p0}", ls.span(0, p0, ls.ATTN_APPEND_SPAN), vm) for p0 in ls.ATTN_LONG_APPEND_SPANS]
    sets += [(f"chunk{n}@{ls.ATTN_LONG_APPEND_CHUNK_POS}", ls.span(0, ls.ATTN_LONG_APPEND_CHUNK_POS, n), "exact" if xs == 3 else None)
             for n in ls.ATTN_LONG_APPEND_CHUNKS]
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
    print(f"ATTN long append geo={geo} xs={xs}: worst share of K elements one bf16 step off = {worst:.4%} (cap 1 %)" +
          (f"; V: {stats['v_off']:.4%} off, all among the {stats['v_near']:.4%} within 2^-19 of a rounding boundary" if stats else ""))
    assert not fails, fails


def test_qkv_rope_epilogue_append():
    """The RoPE + cache-append epilogue of the prefill QKV GEMM (VV_EPI_QKV_ROPE of vv_gemm4_kernel), which reads the table of
    vv_rope_table_kernel: a thin 7B-shaped layer (lm_shapes.QKV_ROPE_CFG: 28 query and 4 kv heads of 128 on a hidden size of 64) and
    one 3600-row pass at position 61,000 make the 4608-wide QKV GEMM 18 x 15 = 270 workgroups, the shape vv_qkv_rope_plan takes
    (asserted in test_prefill_plan_cpu.py).  k_proj.weight = 0: all 3600 x 4 x 128 appended K elements are RoPE(k_proj.bias) at
    positions 61,000 to 64,599, held to check_append's K criterion; nothing but the appended positions (and the V tail) changes."""
    cfg = ls.QKV_ROPE_CFG
    T, p0 = ls.QKV_ROPE_ROWS, ls.QKV_ROPE_POS0
    w = synth.lm_weights(cfg, seed=31)
    w["layers.0.self_attn.k_proj.weight"] = torch.zeros_like(w["layers.0.self_attn.k_proj.weight"])
    s = build_small(cfg, xsplit=1, n_slots=1, max_ctx=ls.QKV_ROPE_MAX_CTX, max_rows=T, lm_w=w)
    try:
        E = types.SimpleNamespace(cfg=cfg, eng=s.eng, xs=1, w=w)
        g = synth.Gen(77)
        shape = (cfg.kv_heads, p0, cfg.head_dim)
        place(E, s.eng, 0, g.normal(shape, 1.0).to(torch.bfloat16), g.normal(shape, 1.0).to(torch.bfloat16))
        rows = ls.span(0, p0, T)
        x = AC.x_rows(cfg, T, 96)
        got, after = run_pass(E, rows, x, v_tail=True)
        pos = torch.arange(p0, p0 + T)
        kb = w["layers.0.self_attn.k_proj.bias"].view(1, cfg.kv_heads, cfg.head_dim).expand(T, -1, -1)
        kref = R.rope(kb, pos, R.inv_freq(cfg.head_dim, cfg.theta)).transpose(0, 1)
        steps, flat = R.rotated_k_steps(after[0][0][:, p0:p0 + T], kref, kb.transpose(0, 1))
        off = float((steps > 0).double().mean())
        print(f"ATTN QKV-RoPE epilogue: {steps.numel()} K elements, {off:.4%} one bf16 step off (cap 1 %), worst {int(steps.max())} step(s)")
        assert int(steps.max()) <= 1 and off <= 0.01, (int(steps.max()), off)
    finally:
        s.eng.close()


# ---------------------------------------------------------------------------------------------- cache offsets of 2^31 elements and more
class LayerView:
    """an engine seen through one layer: run_pass and place address layer 0 and run layers [0, 1); this sends them to `layer`"""

    def __init__(self, eng, layer):
        self._eng, self._layer = eng, layer

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def kv_import(self, cache, layer, k, v):
        return self._eng.kv_import(cache, self._layer, k, v)

    def kv_export(self, cache, layer, pos0, n_pos, **kw):
        return self._eng.kv_export(cache, self._layer, pos0, n_pos, **kw)

    def lm_forward_range(self, rows, x_in, hidden_out, l0, l1, final_norm):
        return self._eng.lm_forward_range(rows, x_in, hidden_out, self._layer, self._layer + 1, final_norm)


@pytest.mark.parametrize("xs", [1, 2, 3])
def test_far_cache_offsets(xs):
    """Geometry A sixteen layers deep with 65,536 positions and 9 slots: a cache is 2^27 elements, caches 16 and 17 start at element
    2^31 and 2^31 + 2^27 of the K and V arrays (4.83 GB each, 9.7 GB for the engine), and layer 15 -- the readout layer here, run
    alone -- lies another 15 x 2^23 elements in.  A fused decode step over caches 0, 16 and 17 (65,000, 40 and 3000 positions), a
    5-row span on each, and in the bf16 mode a 64-row chunk on cache 17, prefixes placed with vv_kv_import and read back with
    vv_kv_export at layer 15, against the fp64 reference at this file's bounds; layers 0 and 15 of cache 0 are bit-unchanged by the
    passes on caches 16 and 17 (a 32-bit offset would wrap onto cache 0)."""
    from vibevoice_amd.engine import EngineError
    try:
        E = LongEng("A", xs, cfg=ls.FAR_CFG, layer=ls.FAR_LAYER, n_slots=ls.FAR_SLOTS, max_ctx=ls.FAR_MAX_CTX, max_rows=ls.FAR_MAX_ROWS)
    except EngineError as e:
        if "hipMalloc" in str(e):
            pytest.skip(f"the engine cannot allocate its caches: {e}")
        raise
    try:
        cfg, eng = E.cfg, E.eng
        view = LayerView(eng, ls.FAR_LAYER)
        g = synth.Gen(5)
        shape = (cfg.kv_heads, eng.max_ctx, cfg.head_dim)
        with torch.cuda.stream(eng.stream):
            eng.kv_import(0, 0, dev(g.normal(shape, 1.0).to(torch.bfloat16), eng), dev(g.normal(shape, 1.0).to(torch.bfloat16), eng))
        eng.sync()

        def cache0():
            out = []
            for layer in (0, ls.FAR_LAYER):
                k, v = eng.kv_export(0, layer, 0, eng.max_ctx)
                eng.sync()
                out += [bits(k.cpu()), bits(v.cpu())]
            return out

        def prefixes(rows, family, seed):
            first = {}
            for c, p in rows:
                first.setdefault(c, p)
            for c, n in first.items():
                place(E, view, c, *AC.prefix(cfg, n, "random", family, AC.LONG_SEED + seed + 13 * c + n))

        Wf, Ws, Wp = LongWorst(E, "fused"), LongWorst(E, "split"), LongWorst(E, "prefill4") if xs == 1 else None
        E.load("fused")
        rows = list(ls.FAR_DECODE)
        prefixes(rows, "fused", 5000)
        x = AC.x_rows(cfg, len(rows), 60, own=(1,))
        got, after = run_pass(E, rows, x, view)
        sc = Wf.judge(("far", "decode"), rows, x, got, after)
        for h in plus_heads(cfg):
            assert planted_weight(sc, 1, h, rows[1][1]) >= 0.5
        before = cache0()
        for c, p0 in ls.FAR_SPANS[1:]:
            rows = ls.span(c, p0, 5)
            prefixes(rows, "split", 6000)
            x = AC.x_rows(cfg, 5, 61 + c)
            got, after = run_pass(E, rows, x, view)
            Ws.judge(("far", "span", c), rows, x, got, after)
        if xs == 1:
            E.load("prefill4")
            c, p0, n = ls.FAR_CHUNK
            rows = ls.span(c, p0, n)
            prefixes(rows, "prefill4", 7000)
            x = AC.x_rows(cfg, n, 62)
            got, after = run_pass(E, rows, x, view, v_tail=True)
            Wp.judge(("far", "chunk"), rows, x, got, after)
            E.load("split")
        assert all(torch.equal(a, b) for a, b in zip(before, cache0())), "passes on caches 16 and 17 changed cache 0"
        c, p0 = ls.FAR_SPANS[0]
        rows = ls.span(c, p0, 5)
        prefixes(rows, "split", 6000)
        x = AC.x_rows(cfg, 5, 61)
        got, after = run_pass(E, rows, x, view)
        Ws.judge(("far", "span", c), rows, x, got, after)
    finally:
        E.eng.close()
    for W in (Wf, Ws, Wp):
        if W is not None:
            W.done()
