"""Every compiled form of the decode GEMV (csrc/gemv.hip: vv_gemv_kernel), ONE launch at a time through vv_gemv_case, against the
fp64 reference of tests/gemv_ref.py (itself held to the oracle by tests/test_gemv_ref_cpu.py).

vv_gemv_case launches the GEMV or refuses -- no other kernel can stand in -- and reports the form (XS, MR, WPB, PARTS, SL) that the
launcher itself chose; every case asserts the form it was written for.  Every case also
  * pads every input stride (ldx, ld_mod, ld_gate > width) with NaN and every output stride (ldy > N) with a finite sentinel, puts one
    guard row before and after every output, and requires finite results with pads, guards and rows of unnamed slots bit-unchanged;
  * launches twice from identical inputs and requires bit-identical buffers (the kernel's sums are fixed-order);
  * compares PER ROW: rel-L2 of each output row and max |err| / max |ref| of each row -- one bad tile or row cannot hide in a norm.

Forms and the cases that reach them (n_tiles = ceil(N / 16), k_tiles = ceil(K / 32)):

  <XS, 4, 8>           test_decode_default   xs 1, 2, 3 x all 14 pairs x T 1..4 (NORMDW: T = 1; CFG_DPM: T = 2 n_cfg = 2, 4) x
                                             K 32 (one k-tile, seven idle waves), 36, 100 (masked tail), 160, 288 (9 tiles), 544 (17 tiles:
                                             two 8-step batches and a tail) x N 4, 20 (last tile of 4 features), 96
  <1, 2, 4> <1, 4, 4>  test_four_wave        the eight W4 pairs, N 4112, 4100 (257 tiles; 4-feature last tile), K 64, 100, T 1, 2 -> MR 2,
                                             T 3, 4 -> MR 4
  <1, 4, 16>           test_sixteen_wave     the four W16 pairs, K 3072 (96 k-tiles), 3076 (97: waves 14, 15 empty), N 20, 2048, T 1, 4
  <XS, 4, 8> grid.y 3  test_ksplit_producer  NONE + RESID (bias, nscale) and NONE + GATED_RESID, xs 1, 2, 3, k_tiles 2 (empty third column),
                                             96, 97, 98; Y and each part against their own K range, (Y + p0) + p1 against the whole
  <XS, 4, 8, 1>        test_parts_x          the four PARTS_X pairs, xs 1, 2, 3
  <1, 2, 4, 1> <1, 4, 4, 1>  test_parts_x_wide   RMS_MOD + SWIGLU at N 4112: T 1, 2 -> the 2-row consumer, T 3, 4 -> the 4-wave one
  <XS, 4, 8, 2>        test_parts_y          both PARTS_Y pairs, xs 1, 2, 3
  producer -> consumer test_ksplit_chain     a kgrid = 3 launch feeds a PARTS = 1 launch; against the two products unsplit
  <XS, 16, 8>          test_wide             the eight WIDE pairs, xs 1, 2, T 5, 16, 17, 33
  <1, 16, 4>           test_wide4            the four WIDE4 pairs, n_tiles * grid.y > 128
  <1, 16, 4> (MOD)     test_wide_mod         the three WIDE_MOD pairs; CFG_DPM with n_cfg 3, 8 (T = 2 n_cfg), with and without sde noise
  <XS, 16, 8> ADD_SILU test_wide_add_silu_row_map   x_row_mod = 2, add_rows_per_vec = 2, T = 20
  CFG_DPM decode       test_cfg_dpm_decode   n_cfg 1, 2; a mid-trajectory row of vibevoice_amd/schedule.py and a synthetic all-non-zero row
  <XS, 16, WPB, 0, 1>  test_slots            the three SL pairs, xs 1, 2; (sl_n, sl_T) (1, 5), (3, 7) (a slot straddles a 16-row tile),
                                             (8, 2), (2, 16); ids out of order; slot buffers on the X side or the Y side; one 4-wave shape
  refusals             test_refusals         host side only: nothing launches

Bounds.  xs = 3: rel-L2 <= 2e-5 per row (the stated bound of one exact-mode GEMM, test_gpu_kernels.py).  xs = 1, 2 against the reference
with the SAME operand rounding: rel-L2 <= 2e-4 per row (what test_prefill_gemm3 holds bf16 operands + fp32 accumulation to), normalised
max error <= 4 x the rel-L2 bound.  CFG_DPM's z / x0p: see CFG_BOUND below.  No bound comes from another GEMV launch."""
import numpy as np
import pytest
import torch

import gemv_ref as R
import synth
from gpu_util import build_small
from vibevoice_amd import schedule

pytestmark = pytest.mark.gpu

NONE, RMS, RMS_MOD, ADD_SILU, NORMDW = 0, 1, 2, 3, 4
STORE, BIAS, BIAS_GELU, SWIGLU, RESID, GATED, CFG_DPM = 0, 1, 2, 3, 4, 5, 6
COMBOS = [(NONE, STORE), (NONE, BIAS), (NONE, RESID), (NONE, GATED), (RMS, BIAS), (RMS, BIAS_GELU), (RMS, SWIGLU), (RMS, RESID),
          (RMS, STORE), (RMS_MOD, SWIGLU), (RMS_MOD, CFG_DPM), (RMS_MOD, STORE), (ADD_SILU, STORE), (NORMDW, BIAS_GELU)]
W4 = [(RMS, SWIGLU), (RMS_MOD, SWIGLU), (RMS, BIAS_GELU), (RMS, BIAS), (NONE, STORE), (NONE, BIAS), (ADD_SILU, STORE), (NORMDW, BIAS_GELU)]
W16 = [(NONE, RESID), (NONE, GATED), (NONE, BIAS), (NONE, STORE)]
WIDE = [(NONE, STORE), (NONE, BIAS), (NONE, RESID), (RMS, BIAS), (RMS, BIAS_GELU), (RMS, SWIGLU), (ADD_SILU, STORE), (NONE, GATED)]
WIDE4 = [(NONE, STORE), (NONE, BIAS), (NONE, RESID), (RMS, BIAS_GELU)]
WIDE_MOD = [(RMS_MOD, SWIGLU), (RMS_MOD, CFG_DPM), (RMS_MOD, STORE)]
PARTS_X = [(RMS, BIAS), (RMS_MOD, SWIGLU), (RMS_MOD, CFG_DPM), (RMS_MOD, STORE)]
PARTS_Y = [(NONE, RESID), (NONE, GATED)]
SL_PAIRS = [(NONE, BIAS), (NONE, RESID), (RMS, BIAS_GELU)]

REL = {1: 2e-4, 2: 2e-4, 3: 2e-5}
# CFG_DPM's outputs.  z' = cs z + c0 x0 + c1 (x0 - x0p) and x0 = a z - s v subtract near-equal terms, so the bound is MEASURED, not taken
# in advance: CFG_MEASURED is the worst per-row rel-L2 of z / x0p against the fp64 reference over every CFG_DPM case of this file on an
# MI355X (xs = 1: 1.687e-07, xs = 2: 1.515e-05 -- the two-term split carries 16 mantissa bits of the activation, the reference all 24
# --, xs = 3: 2.109e-07), rounded up in the third digit; the bound is 4 x that, room for the other forms' summation orders.  Every
# CFG_DPM test prints its own worst value next to the bound (run with -s).
CFG_MEASURED = {1: 1.69e-7, 2: 1.52e-5, 3: 2.11e-7}
CFG_BOUND = {xs: 4 * v for xs, v in CFG_MEASURED.items()}
EPS = 1e-5
SENT = 12345.0
PAD = 4            # extra floats per padded row: keeps every row 16-byte aligned


@pytest.fixture(scope="module")
def eng():
    s = build_small(synth.LMCfg(), xsplit=1)
    yield s.eng
    s.eng.close()


_wcache = {}


def _weights(eng, N, K, which=0):
    """(the matrix as the tiles hold it, fp64; packed device tiles), one per shape for the whole module"""
    key = (N, K, which)
    if key not in _wcache:
        w = synth.Gen(900 + 7 * N + 13 * K + which).normal((N, K), 1.0 / np.sqrt(K))
        _wcache[key] = (R.weights(w), eng.pack_matrix(w))
    return _wcache[key]


def _in(eng, t, ld=None):
    """rows of t at stride ld, the pad columns NaN"""
    t = t.reshape(-1, t.shape[-1]).float()
    ld = t.shape[-1] if ld is None else ld
    buf = torch.full((t.shape[0], ld), float("nan"))
    buf[:, :t.shape[-1]] = t
    return buf.to(eng.device)


class Out:
    """an output region: a flat buffer of `total` floats filled with the sentinel, the kernel's pointer `base` floats in, logical row r
    at base + offs[r], `width` floats wide (initial contents `init`, e.g. the residual), everything else must stay bit-unchanged"""

    def __init__(self, eng, total, base, offs, width, init=None):
        self.base, self.width = base, width
        self.idx = (base + torch.as_tensor(offs, dtype=torch.long)[:, None] + torch.arange(width)[None]).reshape(len(offs), width)
        assert int(self.idx.min()) >= 0 and int(self.idx.max()) < total and self.idx.unique().numel() == self.idx.numel()
        buf = torch.full((total,), SENT)
        if init is not None:
            buf[self.idx] = init.float()
        self.init = buf
        self.dev = buf.to(eng.device)
        self.ptr = self.dev[base:]
        self.keep = torch.ones(total, dtype=torch.bool)
        self.keep[self.idx.reshape(-1)] = False

    @classmethod
    def rows(cls, eng, T, width, ld, init=None):
        """[T][ld] with one guard row before and one after"""
        return cls(eng, (T + 2) * ld, ld, [r * ld for r in range(T)], width, init)

    def reset(self):
        self.dev.copy_(self.init)

    def read(self):
        after = self.dev.cpu()
        assert torch.equal(after.view(torch.int32)[self.keep], self.init.view(torch.int32)[self.keep]), "pad / guard / unnamed rows changed"
        got = after[self.idx]
        assert bool(torch.isfinite(got).all()), "non-finite output"
        return after, got


def row_errs(got, ref):
    """worst row: (rel-L2, max |err| / max |ref|); a row whose reference is exactly zero must be exactly zero"""
    d = got.double() - ref
    nrm, mx = ref.norm(dim=-1), ref.abs().amax(-1)
    zero = nrm == 0
    rel = torch.where(zero, torch.where(d.norm(dim=-1) == 0, 0.0, float("inf")), d.norm(dim=-1) / nrm.clamp_min(1e-300))
    mxe = torch.where(zero, rel, d.abs().amax(-1) / mx.clamp_min(1e-300))
    return float(rel.max()), float(mxe.max())


def run_case(eng, pro, epi, T, N, K, xs, form, seed, *, n_cfg=0, coef=None, sde=False, x_row_mod=0, arpv=0, kgrid=0, parts=None, sl=None,
             cfg_scale=1.3):
    """build, launch twice, check form / guards / determinism; -> {output name: (got fp32, ref fp64)}"""
    g = synth.Gen(seed)
    ldx, ldy = K + PAD, N + PAD
    W, wp = _weights(eng, N, K)
    kw = dict(pro=pro, epi=epi, ldx=ldx, ldy=ldy, eps=EPS, xsplit=xs)
    x_rows = x_row_mod if x_row_mod > 0 else T
    x = g.normal((x_rows, K), 1.0, mat=False)
    x_eff = x
    if parts == "x":
        xa = g.normal((2, T, K), 0.5, mat=False)
        x_eff = R.add_parts(x, xa[0], xa[1])
        kw.update(xa=_in(eng, xa, ldx).reshape(-1), n_xa=2, part_stride=T * ldx)
    # ---- activation side
    if sl is not None:
        sl_n, sl_T, ids, x_slots, y_slots = sl
        assert T == sl_n * sl_T
        nbuf = max(ids) + 2
        kw.update(sl_n=sl_n, sl_T=sl_T, sl_id=ids)
        if x_slots:
            sl_x = sl_T * ldx + 8
            xb = torch.full((nbuf, sl_x), float("nan"))
            for rg in range(T):
                xb[ids[rg // sl_T], (rg % sl_T) * ldx:(rg % sl_T) * ldx + K] = x[rg]
            xd = xb.to(eng.device).reshape(-1)
            kw.update(sl_x=sl_x)
        else:
            xd = _in(eng, x, ldx).reshape(-1)
    else:
        xd = _in(eng, x, ldx).reshape(-1)
    nw = None
    if pro in (RMS, NORMDW) or (pro == RMS_MOD and epi == SWIGLU):
        nw = g.vec(K, 0.1, 1.0)
        kw.update(nw=nw.to(eng.device))
    outs = {}
    if pro == NONE:
        P = R.pro_none(x_eff, xs)
    elif pro == RMS:
        P = R.pro_rms(x_eff, nw, EPS, xs)
    elif pro == RMS_MOD:
        sc, sh = g.normal((T, K), 0.3, mat=False), g.normal((T, K), 0.3, mat=False)
        P = R.pro_rms_mod(x_eff, nw, sc, sh, EPS, xs)
        kw.update(mod_scale=_in(eng, sc, ldx + PAD).reshape(-1), mod_shift=_in(eng, sh, ldx + PAD).reshape(-1), ld_mod=ldx + PAD)
    elif pro == ADD_SILU:
        n_vec = (T - 1) // arpv + 1 if arpv > 0 else 1
        av = g.normal((n_vec, K), 1.0, mat=False)
        P = R.pro_add_silu(x, av, T, xs, x_row_mod, arpv)
        kw.update(addvec=av.to(eng.device).reshape(-1), x_row_mod=x_row_mod, add_rows_per_vec=arpv)
    else:
        hist, taps = g.normal((6, K), 1.0, mat=False), g.normal((7, K), 1.0 / np.sqrt(7.0), mat=False)
        db, dg, dn = g.vec(K, 0.1), g.uniform((K,), 0.3, 0.9), g.vec(K, 0.1, 1.0)
        P, xo, hn = R.pro_normdw(x, nw, EPS, xs, hist, taps, db, dg, dn)
        outs["dw_xout"] = (Out.rows(eng, 1, K, K), xo)
        outs["dw_hnew"] = (Out.rows(eng, 1, K, K), hn)
        kw.update(dw_hist=hist.to(eng.device).reshape(-1), dw_w=taps.to(eng.device).reshape(-1), dw_b=db.to(eng.device),
                  dw_gamma=dg.to(eng.device), dw_nw=dn.to(eng.device), dw_xout=outs["dw_xout"][0].ptr, dw_hnew=outs["dw_hnew"][0].ptr)
    acc = R.product(P, W)
    # ---- output side
    y0 = g.normal((T, N), 1.0, mat=False) if epi in (RESID, GATED) else None
    y_eff = y0
    if parts == "y":
        ya = g.normal((2, T, N), 0.5, mat=False)
        y_eff = R.add_parts(y0, ya[0], ya[1])
        kw.update(ya=_in(eng, ya, ldy).reshape(-1), n_ya=2, part_stride=T * ldy)
    bias = nscale = gate = None
    if epi in (BIAS, BIAS_GELU, RESID):
        bias = g.vec(N, 0.3)
        kw.update(bias=bias.to(eng.device))
    if epi == RESID:
        nscale = g.uniform((N,), 0.5, 1.5)
        kw.update(nscale=nscale.to(eng.device))
    if epi == GATED:
        gate = g.normal((T, N), 1.0, mat=False)
        kw.update(gate=_in(eng, gate, ldy + PAD).reshape(-1), ld_gate=ldy + PAD)
    if epi == SWIGLU:
        w2, w2p = _weights(eng, N, K, 1)
        kw.update(w2p=w2p)
    if epi == CFG_DPM:
        z0 = g.normal((n_cfg, N), 1.0, mat=False)
        z0 = torch.cat([z0, z0], 0)
        x00 = g.normal((n_cfg, N), 1.0, mat=False)
        noise = g.normal((n_cfg, N), 1.0, mat=False) if sde else None
        zr, x0r = R.epi_cfg_dpm(acc, z0, x00, coef, cfg_scale, noise)
        outs["z"] = (Out.rows(eng, 2 * n_cfg, N, N, z0), zr)
        outs["x0p"] = (Out.rows(eng, n_cfg, N, N, x00), x0r)
        kw.update(z=outs["z"][0].ptr, x0p=outs["x0p"][0].ptr, coef=coef.float().to(eng.device), cfg=cfg_scale, n_cfg=n_cfg,
                  sde_noise=None if noise is None else noise.to(eng.device).reshape(-1))
        yptr = None
    else:
        if kgrid > 1:
            ref, pref = R.ksplit_producer(P, W, kgrid, y_eff, bias, nscale, gate)
            pt = Out(eng, 2 * (T + 2) * ldy, ldy, [p * (T + 2) * ldy + r * ldy for p in range(2) for r in range(T)], N)
            outs["parts"] = (pt, torch.cat(pref, 0))
            kw.update(kgrid=kgrid, yparts=pt.ptr, part_stride=(T + 2) * ldy)
        else:
            ref = {STORE: lambda: R.epi_store(acc), BIAS: lambda: R.epi_bias(acc, bias), BIAS_GELU: lambda: R.epi_bias_gelu(acc, bias),
                   SWIGLU: lambda: R.epi_swiglu(acc, R.product(P, w2)),
                   RESID: lambda: R.epi_resid(acc, y_eff, bias, nscale), GATED: lambda: R.epi_gated_resid(acc, y_eff, gate)}[epi]()
        if sl is not None and sl[4]:
            sl_y = sl_T * ldy + 8
            offs = [ids[rg // sl_T] * sl_y + (rg % sl_T) * ldy for rg in range(T)]
            yo = Out(eng, ldy + nbuf * sl_y + ldy, ldy, offs, N, y0)
            kw.update(sl_y=sl_y)
        else:
            yo = Out.rows(eng, T, N, ldy, y0)
        outs["y"] = (yo, ref)
        yptr = yo.ptr
    snaps = []
    for _ in range(2):
        for o, _r in outs.values():
            o.reset()
        torch.cuda.synchronize()
        got_form = eng.gemv_case(wp, xd, yptr, T, N, K, **kw)
        torch.cuda.synchronize()
        assert got_form == form, f"form {got_form}, the case was written for {form}"
        snaps.append({k: o.read() for k, (o, _r) in outs.items()})
    for k in outs:
        assert torch.equal(snaps[0][k][0].view(torch.int32), snaps[1][k][0].view(torch.int32)), f"{k}: two launches differ"
    res = {k: (snaps[0][k][1], outs[k][1]) for k in outs}
    if kgrid > 1:       # the parts read back in the consumer's order against the unsplit product
        whole = R.epi_gated_resid(acc, y_eff, gate) if epi == GATED else R.epi_resid(acc, y_eff, bias, nscale)
        p = res["parts"][0]
        res["sum"] = (R.add_parts(res["y"][0], p[:T], p[T:]), whole)
    return res


def check(res, xs, tag, fails, worst=None):
    for k, (got, ref) in res.items():
        rel, mxe = row_errs(got, ref)
        if k in ("z", "x0p"):
            if worst is not None:
                worst[0] = max(worst[0], rel)
            if rel > CFG_BOUND[xs]:
                fails.append((tag, k, rel, mxe))
        elif rel > REL[xs] or mxe > 4 * REL[xs]:
            fails.append((tag, k, rel, mxe))


_sched_rows = {}


def coef_rows():
    """a mid-trajectory (second-order, stochastic: six non-zero entries but for rounding) row of the shipped 10-step table, and a
    synthetic row with all six entries far from zero"""
    if not _sched_rows:
        _, c = schedule.make_table(10, algorithm_type="sde-dpmsolver++")
        _sched_rows["mid"] = torch.from_numpy(c[5].copy())
        _sched_rows["syn"] = torch.tensor([0.8, 0.6, 0.7, 0.45, -0.3, 0.25])
    return _sched_rows


def _t_list(pro, epi, ts):
    if pro == NORMDW:
        return [t for t in ts if t == 1]
    if epi == CFG_DPM:
        return [t for t in ts if t % 2 == 0]
    return list(ts)


def _sweep(eng, pro, epi, xs, ts, ns, ks, form_of, seed, **kw):
    fails, worst = [], [0.0]
    for T in _t_list(pro, epi, ts):
        for N in ns:
            for K in ks:
                extra = dict(kw)
                if epi == CFG_DPM:
                    extra.update(n_cfg=T // 2, coef=coef_rows()["mid"], sde=(N + K) % 8 == 0)
                res = run_case(eng, pro, epi, T, N, K, xs, form_of(T, N, K), seed + 131 * T + 17 * N + K, **extra)
                check(res, xs, (T, N, K), fails, worst)
    if epi == CFG_DPM:
        print(f"CFG_DPM pro={pro} xs={xs}: worst per-row rel-L2 of z / x0p = {worst[0]:.3e} (bound {CFG_BOUND[xs]:.1e})")
    assert not fails, fails


@pytest.mark.parametrize("xs", [1, 2, 3])
@pytest.mark.parametrize("pro,epi", COMBOS)
def test_decode_default(eng, pro, epi, xs):
    _sweep(eng, pro, epi, xs, (1, 2, 3, 4), (4, 20, 96), (32, 36, 100, 160, 288, 544), lambda T, N, K: (xs, 4, 8, 0, 0), 1000 * pro + 100 * epi + xs)


@pytest.mark.parametrize("pro,epi", W4)
def test_four_wave(eng, pro, epi):
    _sweep(eng, pro, epi, 1, (1, 2, 3, 4), (4112, 4100), (64, 100), lambda T, N, K: (1, 2 if T <= 2 else 4, 4, 0, 0), 2000 + 10 * pro + epi)


@pytest.mark.parametrize("pro,epi", W16)
def test_sixteen_wave(eng, pro, epi):
    _sweep(eng, pro, epi, 1, (1, 4), (20, 2048), (3072, 3076), lambda T, N, K: (1, 4, 16, 0, 0), 3000 + 10 * pro + epi)


@pytest.mark.parametrize("xs", [1, 2, 3])
@pytest.mark.parametrize("epi", [RESID, GATED])
def test_ksplit_producer(eng, epi, xs):
    # k_tiles 2 (third column empty), 96, 97, 98; N = 20: a last tile of 4 features
    _sweep(eng, NONE, epi, xs, (1, 2, 4), (20, 96), (64, 3072, 3076, 3136), lambda T, N, K: (xs, 4, 8, 0, 0), 4000 + 10 * epi + xs, kgrid=3)


@pytest.mark.parametrize("xs", [1, 2, 3])
@pytest.mark.parametrize("pro,epi", PARTS_X)
def test_parts_x(eng, pro, epi, xs):
    _sweep(eng, pro, epi, xs, (1, 2, 3, 4), (20, 96), (100, 544), lambda T, N, K: (xs, 4, 8, 1, 0), 5000 + 10 * epi + xs, parts="x")


def test_parts_x_wide(eng):
    _sweep(eng, RMS_MOD, SWIGLU, 1, (1, 2, 3, 4), (4112,), (100,), lambda T, N, K: (1, 2 if T <= 2 else 4, 4, 1, 0), 5500, parts="x")


@pytest.mark.parametrize("xs", [1, 2, 3])
@pytest.mark.parametrize("pro,epi", PARTS_Y)
def test_parts_y(eng, pro, epi, xs):
    _sweep(eng, pro, epi, xs, (1, 2, 3, 4), (20, 96), (100, 544), lambda T, N, K: (xs, 4, 8, 2, 0), 6000 + 10 * epi + xs, parts="y")


@pytest.mark.parametrize("xs", [1, 2, 3])
def test_ksplit_chain(eng, xs):
    """x1 = y0 + nscale * (x . W1^T + b) leaves a kgrid = 3 launch as Y + 2 parts; RMS + BIAS reads it back as (Y + p0) + p1.  Reference:
    the same two products with K unsplit (fp64, the first result rounded to fp32 where the tensor is fp32)."""
    T, K1, H, N2 = 2, 3076, 100, 20
    g = synth.Gen(7700 + xs)
    ld = H + PAD
    w1, w1p = _weights(eng, H, K1)
    w2, w2p = _weights(eng, N2, H)
    x, y0 = g.normal((T, K1), 1.0, mat=False), g.normal((T, H), 1.0, mat=False)
    b1, ns, nw, b2 = g.vec(H, 0.3), g.uniform((H,), 0.5, 1.5), g.vec(H, 0.1, 1.0), g.vec(N2, 0.3)
    x1 = R.epi_resid(R.product(R.pro_none(x, xs), w1), y0, b1, ns)
    ref = R.epi_bias(R.product(R.pro_rms(x1.float(), nw, EPS, xs), w2), b2)
    yo = Out.rows(eng, T, H, ld, y0)
    pt = Out(eng, 2 * (T + 2) * ld, ld, [p * (T + 2) * ld + r * ld for p in range(2) for r in range(T)], H)
    out = Out.rows(eng, T, N2, N2 + PAD)
    torch.cuda.synchronize()
    f1 = eng.gemv_case(w1p, x.to(eng.device).reshape(-1), yo.ptr, T, H, K1, epi=RESID, ldy=ld, bias=b1.to(eng.device), nscale=ns.to(eng.device),
                       kgrid=3, yparts=pt.ptr, part_stride=(T + 2) * ld, xsplit=xs)
    f2 = eng.gemv_case(w2p, yo.ptr, out.ptr, T, N2, H, pro=RMS, epi=BIAS, ldx=ld, ldy=N2 + PAD, nw=nw.to(eng.device), eps=EPS,
                       bias=b2.to(eng.device), xa=pt.ptr, n_xa=2, part_stride=(T + 2) * ld, xsplit=xs)
    torch.cuda.synchronize()
    assert f1 == (xs, 4, 8, 0, 0) and f2 == (xs, 4, 8, 1, 0), (f1, f2)
    fails = []
    p = pt.read()[1]
    check({"x1": (R.add_parts(yo.read()[1], p[:T], p[T:]), x1), "y": (out.read()[1], ref)}, xs, "chain", fails)
    assert not fails, fails


@pytest.mark.parametrize("xs", [1, 2])
@pytest.mark.parametrize("pro,epi", WIDE)
def test_wide(eng, pro, epi, xs):
    kw = dict(arpv=0) if pro != ADD_SILU else dict(arpv=4)
    _sweep(eng, pro, epi, xs, (5, 16, 17, 33), (20, 96), (36, 288), lambda T, N, K: (xs, 16, 8, 0, 0), 7000 + 100 * pro + 10 * epi + xs, **kw)


@pytest.mark.parametrize("pro,epi", WIDE4)
def test_wide4(eng, pro, epi):
    # n_tiles * grid.y: 129 * 1, 65 * 2 and 65 * 3 > 128 -- and 64 * 2 = 128 stays on 8 waves
    form = lambda T, N, K: (1, 16, 4 if ((N + 15) // 16) * ((T + 15) // 16) > 128 else 8, 0, 0)
    _sweep(eng, pro, epi, 1, (5, 16), (2052,), (36, 288), form, 7500 + 10 * pro + epi)
    _sweep(eng, pro, epi, 1, (17, 33), (1028, 1024), (100,), form, 7600 + 10 * pro + epi)


@pytest.mark.parametrize("sde", [False, True])
@pytest.mark.parametrize("n_cfg", [3, 8])
def test_wide_mod_cfg_dpm(eng, n_cfg, sde):
    fails, worst = [], [0.0]
    for N in (20, 64):
        for K in (100, 288):
            for name, coef in coef_rows().items():
                res = run_case(eng, RMS_MOD, CFG_DPM, 2 * n_cfg, N, K, 1, (1, 16, 4, 0, 0), 8000 + N + K + n_cfg, n_cfg=n_cfg, coef=coef, sde=sde)
                check(res, 1, (n_cfg, N, K, name), fails, worst)
    print(f"CFG_DPM 16-row n_cfg={n_cfg} sde={sde}: worst per-row rel-L2 of z / x0p = {worst[0]:.3e} (bound {CFG_BOUND[1]:.1e})")
    assert not fails, fails


@pytest.mark.parametrize("epi", [SWIGLU, STORE])
def test_wide_mod(eng, epi):
    _sweep(eng, RMS_MOD, epi, 1, (5, 16, 17, 33), (20, 96), (36, 288), lambda T, N, K: (1, 16, 4, 0, 0), 8500 + epi)


@pytest.mark.parametrize("xs", [1, 2])
def test_wide_add_silu_row_map(eng, xs):
    """the batched adaLN mapping: 20 output rows = 10 add-vectors x 2 activation rows"""
    fails = []
    for N, K in ((20, 100), (96, 288)):
        check(run_case(eng, ADD_SILU, STORE, 20, N, K, xs, (xs, 16, 8, 0, 0), 8800 + N + xs, x_row_mod=2, arpv=2), xs, (N, K), fails)
    assert not fails, fails


@pytest.mark.parametrize("xs", [1, 2, 3])
@pytest.mark.parametrize("n_cfg", [1, 2])
def test_cfg_dpm_decode(eng, n_cfg, xs):
    fails, worst = [], [0.0]
    for N in (20, 64):
        for K in (100, 544):
            for name, coef in coef_rows().items():
                for sde in (False, True):
                    res = run_case(eng, RMS_MOD, CFG_DPM, 2 * n_cfg, N, K, xs, (xs, 4, 8, 0, 0), 9000 + N + K + n_cfg, n_cfg=n_cfg, coef=coef, sde=sde)
                    check(res, xs, (n_cfg, N, K, name, sde), fails, worst)
    print(f"CFG_DPM decode n_cfg={n_cfg} xs={xs}: worst per-row rel-L2 of z / x0p = {worst[0]:.3e} (bound {CFG_BOUND[xs]:.1e})")
    assert not fails, fails


SLOTS = [(1, 5, [3]), (3, 7, [5, 0, 3]), (8, 2, [7, 2, 5, 0, 3, 6, 1, 4]), (2, 16, [4, 1])]


@pytest.mark.parametrize("xs", [1, 2])
@pytest.mark.parametrize("pro,epi", SL_PAIRS)
def test_slots(eng, pro, epi, xs):
    fails = []
    for sl_n, sl_T, ids in SLOTS:
        for x_slots, y_slots in ((True, False), (False, True)):
            for N, K in ((20, 36), (96, 288)):
                res = run_case(eng, pro, epi, sl_n * sl_T, N, K, xs, (xs, 16, 8, 0, 1), 9500 + 10 * sl_n + sl_T + N, sl=(sl_n, sl_T, ids, x_slots, y_slots))
                check(res, xs, (sl_n, sl_T, x_slots, N, K), fails)
    if xs == 1:         # 65 feature tiles x 2 row tiles > 128 workgroups: the 4-wave form
        res = run_case(eng, pro, epi, 21, 1028, 100, 1, (1, 16, 4, 0, 1), 9600, sl=(3, 7, [5, 0, 3], True, False))
        check(res, 1, "4-wave", fails)
    assert not fails, fails


def test_refusals(eng):
    """host side only: vv_gemv_ok or the launcher says no, vv_gemv_case returns VV_GEMV_REFUSED (None here) and nothing is launched.
    The two `assert not refused` lines launch a legal all-zero case: they show that it is the one changed argument that is refused."""
    d = eng.device
    f = lambda *s: torch.zeros(*s, device=d)
    wp = lambda N, K: torch.zeros(int(eng.lib.vv_packed_bytes(N, K)), dtype=torch.uint8, device=d)
    T, N, K = 2, 32, 64
    base = dict(wp=wp(N, K), x=f(T * K), y=f(T * N), T=T, N=N, K=K, xsplit=1)

    def refused(**over):
        a = dict(base)
        a.update(over)
        return eng.gemv_case(a.pop("wp"), a.pop("x"), a.pop("y"), a.pop("T"), a.pop("N"), a.pop("K"), **a) is None
    assert not refused()                                                                    # the base case itself launches
    assert refused(K=62, wp=wp(N, 62))                                                      # K % 4 != 0
    assert refused(K=16, wp=wp(N, 16))                                                      # K < 32
    assert refused(N=30, wp=wp(30, K))                                                      # N % 4 != 0
    assert refused(x=f(T * K + 4)[1:], unaligned_ok=("x",))                                 # misaligned X
    assert refused(epi=RESID, kgrid=2, yparts=f(T * N), part_stride=T * N)                  # kgrid = 2
    assert refused(pro=RMS, epi=BIAS, n_xa=1, xa=f(2 * T * K), part_stride=T * K)           # n_xa = 1
    assert refused(T=5, x=f(5 * K), y=f(5 * N), epi=RESID, n_ya=2, ya=f(10 * N), part_stride=5 * N)   # parts with T > 4
    assert refused(pro=RMS, epi=BIAS, x_row_mod=1)                                          # x_row_mod without ADD_SILU
    dw = dict(dw_hist=f(6 * K), dw_w=f(7 * K), dw_b=f(K), dw_gamma=f(K), dw_nw=f(K), dw_xout=f(K), dw_hnew=f(K))
    assert refused(pro=NORMDW, epi=BIAS_GELU, **dw)                                         # NORMDW with T = 2
    assert refused(T=5, x=f(5 * K), y=f(5 * N), xsplit=3)                                   # xs = 3 with T > 4
    # CFG_DPM pairs row r with row r + n_cfg by a lane shuffle inside one 16-row tile and indexes z / x0p by the tile-local row:
    # T must be 2 * n_cfg and fit one tile
    mod = dict(pro=RMS_MOD, epi=CFG_DPM, ld_mod=K, coef=f(6), cfg=1.3)
    cfg = lambda T_, n: dict(T=T_, x=f(T_ * K), y=None, mod_scale=f(T_ * K), mod_shift=f(T_ * K), z=f(max(T_, 2 * n) * N), x0p=f(max(T_, 2 * n) * N),
                             n_cfg=n, **mod)
    assert not refused(**cfg(2, 1))
    assert refused(**cfg(3, 1))                                                             # T != 2 * n_cfg
    assert refused(**cfg(3, 2))
    assert refused(**cfg(18, 9))                                                            # two 16-row tiles
    assert refused(**cfg(16, 7))
    torch.cuda.synchronize()


def test_wrapper_rejects_bad_arguments(eng):
    """a typo in a test fails in Python, before anything reaches the GPU"""
    d = eng.device
    T, N, K = 2, 32, 64
    wp = torch.zeros(int(eng.lib.vv_packed_bytes(N, K)), dtype=torch.uint8, device=d)
    x, y = torch.zeros(T * K, device=d), torch.zeros(T * N, device=d)
    with pytest.raises(ValueError):
        eng.gemv_case(wp, x[:-1], y, T, N, K)                       # short X
    with pytest.raises(ValueError):
        eng.gemv_case(wp, x, y, T, N, K, ldy=N + 4)                 # Y does not cover the stride
    with pytest.raises(ValueError):
        eng.gemv_case(wp, x.double(), y, T, N, K)                   # dtype
    with pytest.raises(ValueError):
        eng.gemv_case(wp, x.cpu(), y, T, N, K)                      # device
    with pytest.raises(ValueError):
        eng.gemv_case(wp, torch.zeros(T * K + 4, device=d)[1:], y, T, N, K)      # alignment
    with pytest.raises(ValueError):
        eng.gemv_case(wp[:-16], x, y, T, N, K)                      # packed weights of another shape
    with pytest.raises(ValueError):
        eng.gemv_case(wp, x, y, T, N, K, epi=BIAS, bias=torch.zeros(N - 4, device=d))
    with pytest.raises(ValueError):
        eng.gemv_case(wp, x, y, T, N, K, pro=RMS_MOD)               # missing operands
    with pytest.raises(ValueError):
        eng.gemv_case(wp, torch.zeros(T, 2 * K, device=d)[:, :K], y, T, N, K)    # not contiguous
