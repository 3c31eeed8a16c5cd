"""The batch-decode packed GEMV (csrc/gemv16p.hip: vv_gemv16p_kernel, vv_pack16_kernel, vv_pack16_tiles_kernel), ONE launch at a time
through vv_gemv16p_case / vv_pack16_case / vv_pack16_tiles_case, against the fp64 reference of tests/gemv16p_ref.py + tests/gemv_ref.py
(held to their definitions and to the oracle by test_gemv16p_ref_cpu.py and test_gemv_ref_cpu.py).

vv_gemv16p_case launches the kernel through its own launcher or refuses, and reports the waves per workgroup (WPB) the launcher chose;
every case asserts the WPB it was written for.  Every GEMV case also
  * builds its packed operands on the host (gemv16p_ref.pack16_tile): no GEMV case depends on vv_pack16_kernel;
  * pads every input stride (ld_gate, ld_pk > N; bias / pk_nw past N) with NaN and every output stride (ldy > N) with a finite
    sentinel, puts one guard row (1 KiB for a packed output) before and after every output and requires pads and guards bit-unchanged;
  * launches twice from identical inputs and requires bit-identical buffers (the kernel's sums are fixed-order);
  * compares PER ROW: rel-L2 of each output row and max |err| / max |ref| of each row.

Forms (epilogue, flags; flags 1 = RS, 2 = SH, 4 = PK) and the cases that reach them; n_tiles = ceil(N / 16) <= 256 -> WPB 8, else 4:

  BIAS / STORE 0, 1, 3   test_fp32_forms    with and without a bias pointer (STORE: epi 0 on the same kernel)
  RESID 0, GATED 0       test_fp32_forms    in place on Y, ldy > N
  RESID 4, GATED 4       test_pk_forms      Y, Yp and ssq_out; pk_nw / pk_sc present or null
  SWIGLU 0, 1, 3         test_swiglu_forms  packed output
  CFG_DPM 0, 3           test_cfg_dpm_forms n_cfg 1, 3, 8 (T = 2 n_cfg); cfg_rows / sde_noise given and null; a mid-trajectory row of
                                            vibevoice_amd/schedule.py and a synthetic all-non-zero row
  each form, WPB 8:      K 32 (one k-tile, seven empty waves), 160 (5 k-tiles < 8 waves), 288 (9: kper 2, the last busy wave holds 1,
                         three empty), 544 (17), 2080 (65: kper 9, a full 8-step batch + a tail of 1, the second buffer), 4640 (145:
                         kper 19, buffers A, B, A with a tail of 3);  N 4, 20 (fp32 out), 8, 40, 96 (SwiGLU), 16, 48, 96 (PK);
                         T 1, 5, 15, 16;  ssq_tiles 1, 3, 130 (520 float4s > 512 threads)
  each form, WPB 4:      N 4112 (257 tiles) x K 64, 96 (3 k-tiles, one empty wave), 2208 (69: kper 18); N 4100 / 4104 (SwiGLU) x K 64;
                         ssq_tiles 96 (384 float4s > 256 threads)
  every form             test_idle_rows     rows >= T of Xp / Xs / ssq_in NaN: every output buffer bit-identical to the run with zeros
  o -> gate/up -> down   test_chain         three launches on device buffers, each link against the reference of that link fed with
                                            what the previous launch stored; end to end at 5e-3 (test_gpu_shipped.py's bound)
  refusals               test_refusals, test_pack16_refusals    host side only: nothing launches
  vv_pack16_kernel       test_pack16        modes 1 (with / without nw), 2; K 32, 1056, 8192; T 1, 5, 16
  vv_pack16_tiles_kernel test_pack16_tiles  7 tiles, n_inner 3, strides that differ, tile_bytes > a tile
  layout                 test_pack_matrix_is_the_tile_layout    eng.pack_matrix of a 16 x K matrix = pack16_tile, byte for byte

Bounds -- from the project or derived, none from this kernel's own output.  fp32 outputs: rel-L2 <= 2e-4 per row, normalised max error
<= 8e-4 (REL[1] of test_gpu_gemv_forms.py, test_prefill_gemm3's bound: the same bf16 operands, fp32 accumulation).  SwiGLU's packed
output, per element: |got - ref| <= ulp_bf16(ref) / 2 + 8e-4 max |ref_row|.  CFG_DPM: the epilogue is affine in the two accumulators, so
the GEMV bound is propagated through it plus 16 fp32 roundings of the terms' magnitudes (cfg_limits below).  PK: Yp is bit for bit
bf16((Y_got * pk_nw) * (1 + pk_sc)) formed in fp32 from the Y of the same launch; ssq_out agrees with the fp64 sum of Y_got^2 over the
tile to 2e-6 (4 squares in a lane, then a 2-step lane tree: at most 20 fp32 roundings of a positive sum, 1.2e-6).  vv_pack16_kernel:
|got - v| <= ulp_bf16(v) / 2 + 2e-6 (|rs x nw (1 + sc)| + |sh|) (at most 41 sequential fp32 roundings of a positive sum, halved by
the square root, rsqrtf and four more operations: 1.6e-6).  Run with -s for the measured figure of every form beside its bound."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gemv16p_ref as P
import gemv_ref as R
import synth
from gpu_util import build_small
from test_gpu_gemv_forms import PAD, Out, _in, coef_rows, row_errs

pytestmark = pytest.mark.gpu

STORE, BIAS, SWIGLU, RESID, GATED, CFG_DPM = 0, 1, 3, 4, 5, 6
RS, SH, PK = 1, 2, 4
REL_L2, REL_MAX = 2e-4, 8e-4
SSQ_REL = 2e-6
EPS = 1e-5
NAN = float("nan")
SENT_BYTE = 0x5A                     # a packed output's sentinel: bf16 0x5A5A is finite
SENT_BITS = 0x5A5A
GUARD = 1024
K8 = (32, 160, 288, 544, 2080, 4640)
K4 = (64, 96, 2208)
TS = (1, 5, 15, 16)


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
        w = synth.Gen(1700 + 7 * N + 13 * K + which).normal((N, K), 1.0 / np.sqrt(K))
        _wcache[key] = (R.weights(w), eng.pack_matrix(w))
    return _wcache[key]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class PackedOut:
    """a packed 16-row output tile of n features, one guard KiB before and after, every byte the sentinel (or `fill`)"""

    def __init__(self, eng, n, fill=SENT_BYTE):
        self.n, self.n32, self.nb = n, 32 * ((n + 31) // 32), P.tile_bytes(n)
        self.init = torch.full((self.nb + 2 * GUARD,), SENT_BYTE, dtype=torch.uint8)
        self.init[GUARD:GUARD + self.nb] = fill
        self.dev = self.init.to(eng.device).clone()
        self.ptr = self.dev[GUARD:]

    def reset(self):
        self.dev.copy_(self.init)

    def read(self):
        """-> (the whole buffer, the tile's bf16 bit patterns [16][n32] with every byte of the tile in them)"""
        after = self.dev.cpu()
        assert torch.equal(after[:GUARD], self.init[:GUARD]) and torch.equal(after[GUARD + self.nb:], self.init[GUARD + self.nb:]), "guard bytes changed"
        return after, P.unpack16_bits(after[GUARD:GUARD + self.nb], self.n32)


def _vals(bits):
    return bits.contiguous().view(torch.bfloat16).to(torch.float32)


def _nan_tail(v):
    """a per-feature vector in a buffer one float4 longer than N, the tail NaN"""
    return torch.cat([v.float(), torch.full((4,), NAN)])


def cfg_limits(acc, z0, x00, coef, cfgs):
    """per row: the limits of ||z' - z'_ref|| and ||x0 - x0_ref||.  With v = uncond + cfg (cond - uncond), x0 = a z - s v and
    z' = cs z + c0 x0 + c1 (x0 - x0p) = (cs + (c0 + c1) a) z - (c0 + c1) s v - c1 x0p (+ cn noise): an error e of the two accumulator rows
    (||e_row|| <= 2e-4 ||row||, the GEMV bound) reaches x0 as s (cfg e_c + (1 - cfg) e_u) and z' as (c0 + c1) times that; the fp32
    evaluation adds a few roundings of each term's magnitude, bounded by 16 of them."""
    n = acc.shape[0] // 2
    a, s, cs, c0, c1, _cn = (abs(float(c)) for c in coef.double()[:6])
    c01 = abs(float(coef[3].double() + coef[4].double()))
    cfg = cfgs.double()
    cond, unc = acc[:n], acc[n:2 * n]
    v = unc + cfg[:, None] * (cond - unc)
    nz, nv, nx = z0[:n].double().norm(dim=-1), v.norm(dim=-1), x00.double().norm(dim=-1)
    gemv = REL_L2 * (cfg.abs() * cond.norm(dim=-1) + (1.0 - cfg).abs() * unc.norm(dim=-1))
    u = 16 * 2.0 ** -24
    lim_z = c01 * s * gemv + u * (cs * nz + c01 * (a * nz + s * nv) + c1 * nx)
    lim_x0 = s * gemv + u * (a * nz + s * nv)
    return lim_z, lim_x0


def build(eng, epi, flags, T, N, K, seed, *, with_bias=True, pk_mode="nw+sc", ssq_tiles=1, n_cfg=0, coef=None, sde=False, cfg_rows=False,
          idle_nan=False):
    """one launch's operands, outputs and references; idle_nan: rows >= T of Xp / Xs / ssq_in are NaN instead of zero (same live data)"""
    g = synth.Gen(seed)
    d = eng.device
    idle = NAN if idle_nan else 0.0
    W, wp = _weights(eng, N, K)

    def operand(std):
        full = torch.full((16, K), idle)
        full[:T] = g.normal((T, K), std, mat=False)
        return P.pack16_tile(full)
    xp = operand(1.0)
    kw = dict(epi=epi, flags=flags, eps=EPS)
    part = xs = None
    if flags & RS:                    # arbitrary positive partials: the consumer is held to its definition, not to the operand
        part = torch.full((ssq_tiles, 16), idle)
        part[:, :T] = g.uniform((ssq_tiles, T), 0.5, 2.0) * (K / ssq_tiles)
        kw.update(ssq_in=part.to(d).reshape(-1), ssq_tiles=ssq_tiles)
    if flags & SH:
        xs = operand(0.3)
        kw.update(xs=xs.to(d))
    ops = P.operands(xp, K, T, ssq_in=part, eps=EPS, xs=xs)
    acc = R.product(ops, W)
    c = SimpleNamespace(epi=epi, flags=flags, T=T, N=N, K=K, kw=kw, wp=wp, xp=xp.to(d), outs={}, ref={}, aux={})
    if epi in (STORE, BIAS, RESID, GATED):
        ldy = N + PAD
        y0 = g.normal((T, N), 1.0, mat=False) if epi in (RESID, GATED) else None
        b = g.vec(N, 0.3) if (with_bias and epi in (BIAS, RESID)) else None
        if b is not None:
            kw["bias"] = _nan_tail(b).to(d)
        if epi == GATED:
            gate = g.normal((T, N), 1.0, mat=False)
            kw.update(gate=_in(eng, gate, N + 2 * PAD).reshape(-1), ld_gate=N + 2 * PAD)
            c.ref["y"] = R.epi_gated_resid(acc, y0, gate)
        elif epi == RESID:
            c.ref["y"] = R.epi_resid(acc, y0, b)
        else:
            c.ref["y"] = R.epi_bias(acc, b)
        c.outs["y"] = Out.rows(eng, T, N, ldy, y0)
        kw.update(y=c.outs["y"].ptr, ldy=ldy)
    if flags & PK:
        nt = (N + 15) // 16
        nwv = g.vec(N, 0.1, 1.0) if "nw" in pk_mode else None
        scv = g.normal((T, N), 0.3, mat=False) if "sc" in pk_mode else None
        if nwv is not None:
            kw["pk_nw"] = _nan_tail(nwv).to(d)
        if scv is not None:
            kw.update(pk_sc=_in(eng, scv, N + PAD).reshape(-1), ld_pk=N + PAD)
        c.outs["yp"] = PackedOut(eng, N)
        c.outs["ssq"] = Out.rows(eng, 1, nt * 16, nt * 16)
        kw.update(yp=c.outs["yp"].ptr, ssq_out=c.outs["ssq"].ptr)
        c.aux.update(pk_nw=nwv, pk_sc=scv)
    if epi == SWIGLU:
        W2, w2p = _weights(eng, N, K, 1)
        c.ref["yp"] = R.epi_swiglu(acc, R.product(ops, W2))
        c.outs["yp"] = PackedOut(eng, N)
        kw.update(w2p=w2p, yp=c.outs["yp"].ptr)
    if epi == CFG_DPM:
        n = n_cfg
        coef = coef.float()
        z0 = g.normal((n, N), 1.0, mat=False)
        z0 = torch.cat([z0, z0], 0)
        x00 = g.normal((n, N), 1.0, mat=False)
        noise = g.normal((n, N), 1.0, mat=False) if sde else None
        cfgs = g.uniform((n,), 1.0, 3.0) if cfg_rows else torch.full((n,), 1.25)
        zr, x0r = [], []
        for r in range(n):              # one guidance scale per utterance row
            pair = [r, n + r]
            zz, xx = R.epi_cfg_dpm(acc[pair], z0[pair], x00[r:r + 1], coef, float(cfgs[r]), None if noise is None else noise[r:r + 1])
            zr.append(zz[0])
            x0r.append(xx[0])
        c.ref["z"] = torch.stack(zr + zr, 0)
        c.ref["x0p"] = torch.stack(x0r, 0)
        c.outs["z"] = Out.rows(eng, 2 * n, N, N, z0)
        c.outs["x0p"] = Out.rows(eng, n, N, N, x00)
        # with cfg_rows the scalar is a value no row uses: a launch that read it would miss every bound
        kw.update(z=c.outs["z"].ptr, x0p=c.outs["x0p"].ptr, coef=coef.to(d), cfg=-7.0 if cfg_rows else 1.25, n_cfg=n,
                  sde_noise=None if noise is None else noise.to(d).reshape(-1), cfg_rows=cfgs.to(d) if cfg_rows else None)
        c.aux.update(acc=acc, z0=z0, x00=x00, cfgs=cfgs, coef=coef)
    return c


def launch(eng, c, wpb):
    """twice from identical inputs: the reported WPB, pads / guards, bit-identical outputs -> {name: (whole buffer, logical result)}"""
    snaps = []
    for _ in range(2):
        for o in c.outs.values():
            o.reset()
        torch.cuda.synchronize()
        got = eng.gemv16p_case(c.wp, c.xp, c.T, c.N, c.K, **c.kw)
        torch.cuda.synchronize()
        assert got == wpb, f"WPB {got}, the case was written for {wpb}"
        snaps.append({k: o.read() for k, o in c.outs.items()})
    for k in c.outs:
        assert torch.equal(_bits(snaps[0][k][0]), _bits(snaps[1][k][0])), f"{k}: two launches differ"
    return snaps[0]


def swiglu_excess(vals, ref):
    """worst (|got - ref| - ulp / 2) / max |ref_row| of the packed SwiGLU rows: the bound is REL_MAX"""
    err = (vals.double() - ref).abs() - P.ulp_bf16(ref) / 2
    return float((err / ref.abs().amax(-1, keepdim=True).clamp_min(1e-300)).max())


def verify(c, snap, tag, fails, worst):
    """every assertion on one launch's outputs; figures into worst {name: value}"""
    T, N = c.T, c.N

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    if "y" in c.ref:
        y_got = snap["y"][1]
        rel, mxe = row_errs(y_got, c.ref["y"])
        note("rel-L2", rel)
        note("max", mxe)
        if rel > REL_L2 or mxe > REL_MAX:
            fails.append((tag, "y", rel, mxe))
    if c.flags & PK:
        y_got = snap["y"][1]
        bits = snap["yp"][1]
        want = P.bf16_bits(P.pk_rows(y_got, c.aux["pk_nw"], c.aux["pk_sc"]))
        if not torch.equal(bits[:T, :N], want):
            fails.append((tag, "Yp is not bf16((Y * pk_nw) * (1 + pk_sc)) of the stored Y", int((bits[:T, :N] != want).sum())))
        if bool((bits[T:, :N] != 0).any()):
            fails.append((tag, "Yp rows >= T are not zero"))
        if bool((bits[:, N:] != SENT_BITS).any()):
            fails.append((tag, "Yp features >= N were written"))
        ssq = snap["ssq"][1].reshape(-1, 16)
        if bool((ssq[:, T:] != 0).any()):
            fails.append((tag, "ssq_out rows >= T are not zero"))
        want = P.ssq_partials(y_got)
        rel = float(((ssq[:, :T].double() - want).abs() / want.clamp_min(1e-300)).max())
        note("ssq", rel)
        if rel > SSQ_REL:
            fails.append((tag, "ssq_out", rel))
    if c.epi == SWIGLU:
        bits = snap["yp"][1]
        ex = swiglu_excess(_vals(bits[:T, :N]), c.ref["yp"])
        note("packed", ex)
        if not ex <= REL_MAX:
            fails.append((tag, "Yp", ex))
        if bool((bits[T:] != SENT_BITS).any()) or bool((bits[:, N:] != SENT_BITS).any()):
            fails.append((tag, "Yp rows >= T or features >= N were written"))
    if c.epi == CFG_DPM:
        n = T // 2
        z_got, x_got = snap["z"][1], snap["x0p"][1]
        if not torch.equal(_bits(z_got[:n]), _bits(z_got[n:])):
            fails.append((tag, "the two copies of z' differ"))
        lim_z, lim_x = cfg_limits(c.aux["acc"], c.aux["z0"], c.aux["x00"], c.aux["coef"], c.aux["cfgs"])
        ez = (z_got[:n].double() - c.ref["z"][:n]).norm(dim=-1)
        ex = (x_got.double() - c.ref["x0p"]).norm(dim=-1)
        rz, rx = float((ez / lim_z).max()), float((ex / lim_x).max())
        note("z err / limit", rz)
        note("x0 err / limit", rx)
        print(f"  CFG_DPM {tag}: worst row ||z' err|| = {float(ez.max()):.3e} (limit {float(lim_z[ez.argmax()]):.3e}), "
              f"||x0 err|| = {float(ex.max()):.3e} (limit {float(lim_x[ex.argmax()]):.3e})")
        if not (rz <= 1.0 and rx <= 1.0):
            fails.append((tag, "z / x0p", rz, rx))


def _report(name, worst, bounds):
    print(f"[gemv16p {name}] " + ", ".join(f"{k} {v:.3e} (bound {bounds[k]:.1e})" for k, v in worst.items()))


BOUNDS = {"rel-L2": REL_L2, "max": REL_MAX, "ssq": SSQ_REL, "packed": REL_MAX, "z err / limit": 1.0, "x0 err / limit": 1.0}


def _thin(rot, *lists):
    """a thin cross product: case i takes element (i + rot) of every list, cyclically, until the longest is exhausted -- every value
    of every list appears at least once"""
    n = max(len(l) for l in lists)
    return [tuple(l[(i + rot * j) % len(l)] for j, l in enumerate(lists)) for i in range(n)]


def _sweep(eng, name, epi, flags, seed, ns8, ns4_tail, **opts):
    """the shape classes of the module docstring for one form; opts: lists to rotate through (one entry per case)"""
    fails, worst = [], {}
    rot = (epi + flags) % 3
    names = list(opts)
    cases = [(8,) + t for t in _thin(rot, K8, ns8, TS, (1, 3, 130), *[opts[k] for k in names])]
    wide = [(K, 4112) for K in K4] + [(64, ns4_tail)]
    cases += [(4,) + c[0] + c[1:] for c in _thin(rot, wide, TS, (96,), *[opts[k] for k in names])]
    for i, (wpb, K, N, T, tiles, *rest) in enumerate(cases):
        o = dict(zip(names, rest))
        if epi == CFG_DPM:
            T = 2 * o["n_cfg"]
        c = build(eng, epi, flags, T, N, K, seed + 31 * i, ssq_tiles=tiles, **o)
        tag = (wpb, T, N, K) + ((tiles,) if flags & RS else ()) + tuple(str(v)[:12] for k, v in o.items() if k != "coef")
        verify(c, launch(eng, c, wpb), tag, fails, worst)
    _report(name, worst, BOUNDS)
    assert not fails, fails


@pytest.mark.parametrize("epi,flags,with_bias", [(BIAS, 0, True), (BIAS, 0, False), (STORE, 0, False), (BIAS, RS, True), (BIAS, RS, False),
                                                 (BIAS, RS | SH, True), (BIAS, RS | SH, False), (RESID, 0, True), (RESID, 0, False), (GATED, 0, False)])
def test_fp32_forms(eng, epi, flags, with_bias):
    _sweep(eng, f"epi {epi} flags {flags} bias {int(with_bias)}", epi, flags, 100 * epi + 10 * flags + with_bias, (4, 20, 96), 4100, with_bias=[with_bias])


@pytest.mark.parametrize("epi", [RESID, GATED])
def test_pk_forms(eng, epi):
    _sweep(eng, f"epi {epi} flags 4", epi, PK, 2000 + epi, (16, 48, 96), 4112, with_bias=[True, False], pk_mode=["nw", "nw+sc", "sc", ""])


@pytest.mark.parametrize("flags", [0, RS, RS | SH])
def test_swiglu_forms(eng, flags):
    _sweep(eng, f"SWIGLU flags {flags}", SWIGLU, flags, 3000 + flags, (8, 40, 96), 4104)


@pytest.mark.parametrize("flags", [0, RS | SH])
def test_cfg_dpm_forms(eng, flags):
    rows = coef_rows()
    _sweep(eng, f"CFG_DPM flags {flags}", CFG_DPM, flags, 4000 + flags, (4, 20, 96), 4100, n_cfg=[1, 3, 8], coef=[rows["mid"], rows["syn"]],
           sde=[False, True, True, False], cfg_rows=[False, True, True, False, True])


ALL_FORMS = [(BIAS, 0), (BIAS, RS), (BIAS, RS | SH), (SWIGLU, 0), (SWIGLU, RS), (SWIGLU, RS | SH), (RESID, 0), (RESID, PK), (GATED, 0), (GATED, PK),
             (CFG_DPM, 0), (CFG_DPM, RS | SH)]


@pytest.mark.parametrize("epi,flags", ALL_FORMS)
def test_idle_rows(eng, epi, flags):
    """NaN in rows >= T of the packed operands and of ssq_in reaches no output: MFMA output columns are independent and the epilogues
    mask by row, so every output buffer is bit-identical to the run with zeros there -- an invariant, not a tolerance"""
    T, N, K = (6 if epi == CFG_DPM else 5), 96, 288
    o = dict(ssq_tiles=3)
    if epi == CFG_DPM:
        o.update(n_cfg=3, coef=coef_rows()["syn"], sde=True, cfg_rows=True)
    snaps = []
    for idle_nan in (False, True):
        c = build(eng, epi, flags, T, N, K, 5000 + 10 * epi + flags, idle_nan=idle_nan, **o)
        snaps.append(launch(eng, c, 8))
    for k in snaps[0]:
        assert torch.equal(_bits(snaps[0][k][0]), _bits(snaps[1][k][0])), f"{k}: NaN in idle rows changed the output"
    fails = []
    verify(c, snaps[1], "idle", fails, {})
    assert not fails, fails


@pytest.mark.parametrize("H,I,T", [(64, 96, 5), (96, 160, 16)])
def test_chain(eng, H, I, T):
    """o-proj (RESID + PK) -> gate/up (SWIGLU + RS) -> down (RESID), device buffers only.  Each link against the fp64 reference of that
    link fed with what the previous launch actually stored (Y, the Yp bytes, ssq_out): a rounding flip of a bf16 hand-off cannot enter
    a bound; the producer's own checks (test_pk_forms) close the chain.  End to end against the unbroken fp64 layer: printed, and
    asserted only at 5e-3, the bound test_gpu_shipped.py holds this path to."""
    g = synth.Gen(6000 + H + T)
    d = eng.device
    Wo, wop = _weights(eng, H, H, 2)
    Wg, wgp = _weights(eng, I, H, 0)
    Wu, wup = _weights(eng, I, H, 1)
    Wd, wdp = _weights(eng, H, I, 0)
    a, y0, nw = g.normal((T, H), 1.0, mat=False), g.normal((T, H), 1.0, mat=False), g.vec(H, 0.1, 1.0)
    xp = P.pack16_tile(a)
    ld = H + PAD
    y, yp1, ssq, yp2 = Out.rows(eng, T, H, ld, y0), PackedOut(eng, H), Out.rows(eng, 1, H, H), PackedOut(eng, I, fill=0)
    xp_d, nw_d = xp.to(d), nw.to(d)
    torch.cuda.synchronize()
    w1 = eng.gemv16p_case(wop, xp_d, T, H, H, epi=RESID, flags=PK, y=y.ptr, ldy=ld, yp=yp1.ptr, ssq_out=ssq.ptr, pk_nw=nw_d)
    torch.cuda.synchronize()
    y1 = y.read()[1]
    w2 = eng.gemv16p_case(wgp, yp1.ptr, T, I, H, epi=SWIGLU, flags=RS, w2p=wup, yp=yp2.ptr, ssq_in=ssq.ptr, ssq_tiles=H // 16, eps=EPS)
    w3 = eng.gemv16p_case(wdp, yp2.ptr, T, H, I, epi=RESID, flags=0, y=y.ptr, ldy=ld)
    torch.cuda.synchronize()
    assert (w1, w2, w3) == (8, 8, 8)
    raw1, ssq_got, raw2, y3 = yp1.read()[0][GUARD:], ssq.read()[1].reshape(-1, 16), yp2.read()[0][GUARD:], y.read()[1]
    fails = []
    # link 1
    x1 = R.epi_resid(R.product(P.operands(xp, H, T), Wo), y0)
    rel, mxe = row_errs(y1, x1)
    print(f"[gemv16p chain H {H} I {I} T {T}] o-proj rel-L2 {rel:.3e} max {mxe:.3e} (bounds {REL_L2:.1e}, {REL_MAX:.1e})")
    if rel > REL_L2 or mxe > REL_MAX:
        fails.append(("o-proj", rel, mxe))
    # link 2, from the bytes and partials link 1 stored
    ops = P.operands(raw1, H, T, ssq_in=ssq_got, eps=EPS)
    u = R.epi_swiglu(R.product(ops, Wg), R.product(ops, Wu))
    ex = swiglu_excess(_vals(P.unpack16_bits(raw2, I)[:T]), u)
    print(f"    gate/up packed excess {ex:.3e} (bound {REL_MAX:.1e})")
    if not ex <= REL_MAX:
        fails.append(("gate/up", ex))
    # link 3, from the bytes link 2 stored and the Y link 1 stored
    ref3 = R.epi_resid(R.product(P.operands(raw2, I, T), Wd), y1)
    rel, mxe = row_errs(y3, ref3)
    print(f"    down rel-L2 {rel:.3e} max {mxe:.3e}")
    if rel > REL_L2 or mxe > REL_MAX:
        fails.append(("down", rel, mxe))
    # the unbroken layer: only the o-proj operand and the weights are bf16
    h = x1 * (1.0 / torch.sqrt(x1.pow(2).mean(-1, keepdim=True) + EPS)) * nw.double()
    want = x1 + R.epi_swiglu(h @ Wg.t(), h @ Wu.t()) @ Wd.t()
    rel, mxe = row_errs(y3, want)
    print(f"    end to end rel-L2 {rel:.3e} (bound 5.0e-03)")
    if rel > 5e-3:
        fails.append(("end to end", rel))
    assert not fails, fails


def test_pack_matrix_is_the_tile_layout(eng):
    """two independent statements of one layout: the host's pack16_tile (from the index formula) and the device's weight packer"""
    for K in (96, 40):
        w = synth.Gen(70 + K).normal((16, K), 1.0, mat=False)
        got = eng.pack_matrix(w).cpu()
        assert got.numel() == P.tile_bytes(K)
        assert torch.equal(got, P.pack16_tile(w)), K


@pytest.mark.parametrize("mode", ["rms", "rms_nw", "mod"])
def test_pack16(eng, mode):
    fails, worst_share = [], 0.0
    for K in (32, 1056, 8192):          # 1056: 264 float4s, the second chunk of a thread is partly live; 8192: the limit
        for T in (1, 5, 16):
            g = synth.Gen(7000 + K + T)
            x = g.normal((T, K), 2.0, mat=False)
            nw = g.vec(K, 0.1, 1.0) if mode != "rms" else None
            sc = g.normal((T, K), 0.3, mat=False) if mode == "mod" else None
            sh = g.normal((T, K), 0.3, mat=False) if mode == "mod" else None
            ldx, ld_mod = K + PAD, K + 2 * PAD
            out = PackedOut(eng, K)
            kw = dict(mode=2 if mode == "mod" else 1, ldx=ldx, eps=EPS, nw=None if nw is None else nw.to(eng.device))
            if mode == "mod":
                kw.update(sc=_in(eng, sc, ld_mod).reshape(-1), sh=_in(eng, sh, ld_mod).reshape(-1), ld_mod=ld_mod)
            x_d = _in(eng, x, ldx).reshape(-1)
            torch.cuda.synchronize()
            assert eng.pack16_case(x_d, out.ptr, T, K, **kw) == 4
            torch.cuda.synchronize()
            bits = out.read()[1]
            assert not bool((bits[T:] != 0).any()), "rows >= T are not zero"
            got = _vals(bits[:T])
            assert bool(torch.isfinite(got).all())
            main, shift = P.pack16_value(x, nw, EPS, sc, sh)
            v = main + shift
            lim = P.ulp_bf16(v) / 2 + 2e-6 * (main.abs() + shift.abs())
            over = (got.double() - v).abs() - lim
            if bool((over > 0).any()):
                fails.append((K, T, int((over > 0).sum()), float(over.max())))
            worst_share = max(worst_share, float((got != R.bf16r(v.float())).double().mean()))
    print(f"[pack16 {mode}] worst share of elements that differ from bf16(fp64 value): {worst_share:.3e}")
    assert not fails, fails


def test_pack16_tiles(eng):
    """7 row blocks [6][64] at (outer, inner) strides that differ -> 7 tiles tile_bytes apart: exact bf16 roundings, zero rows >= T,
    the bytes between tiles and around them untouched; the rows and gaps no tile names are NaN"""
    T, K, n_inner, n_tiles = 6, 64, 3, 7
    g = synth.Gen(7100)
    ldx = K + PAD
    s_in = T * ldx + 8
    s_out = n_inner * s_in + 16
    tb, step = P.tile_bytes(K), P.tile_bytes(K) + 512
    offs = [(j // n_inner) * s_out + (j % n_inner) * s_in for j in range(n_tiles)]
    xbuf = torch.full((max(offs) + T * ldx,), NAN)
    blocks = []
    for o in offs:
        b = g.normal((T, K), 1.0, mat=False)
        blocks.append(b)
        for t in range(T):
            xbuf[o + t * ldx:o + t * ldx + K] = b[t]
    init = torch.full((2 * GUARD + n_tiles * step,), SENT_BYTE, dtype=torch.uint8)
    dev, x_d = init.to(eng.device).clone(), xbuf.to(eng.device)
    torch.cuda.synchronize()
    rc = eng.pack16_tiles_case(x_d, dev[GUARD:], T, K, n_tiles, ldx=ldx, stride_outer=s_out, n_inner=n_inner, stride_inner=s_in,
                               tile_bytes=step)
    torch.cuda.synchronize()
    assert rc == 4
    after = dev.cpu()
    keep = torch.ones(after.numel(), dtype=torch.bool)
    for j in range(n_tiles):
        lo = GUARD + j * step
        keep[lo:lo + tb] = False
        bits = P.unpack16_bits(after[lo:lo + tb], K)
        assert torch.equal(bits[:T], P.bf16_bits(blocks[j])), j
        assert not bool((bits[T:] != 0).any()), j
    assert torch.equal(after[keep], init[keep]), "bytes outside the tiles changed"
    # refusals: a stride that is no multiple of 4 floats, a tile distance that is no multiple of 16 bytes
    big = torch.zeros(4 * xbuf.numel(), device=eng.device)
    assert eng.pack16_tiles_case(big, dev[GUARD:], T, K, n_tiles, ldx=ldx, stride_outer=s_out, n_inner=n_inner, stride_inner=s_in + 2, tile_bytes=step) is None
    assert eng.pack16_tiles_case(big, dev[GUARD:], T, K, n_tiles, ldx=ldx, stride_outer=s_out, n_inner=n_inner, stride_inner=s_in, tile_bytes=tb + 8) is None
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), after)


def test_pack16_refusals(eng):
    """host side only: vv_pack16_launch says no and nothing is launched"""
    d = eng.device
    f = lambda n: torch.zeros(n, device=d)
    xp = torch.zeros(260 * 1024, dtype=torch.uint8, device=d)
    T = 4
    assert eng.pack16_case(f(T * 64), xp, T, 64) == 4                                   # the base case itself launches
    assert eng.pack16_case(f(T * 48), xp, T, 48) is None                                # K % 32 != 0
    assert eng.pack16_case(f(T * 8224), xp, T, 8224) is None                            # K > 8192
    assert eng.pack16_case(f(T * 66), xp, T, 64, ldx=66, unaligned_ld_ok=True) is None  # rows that are not 16-byte aligned
    assert eng.pack16_case(f(T * 64), xp, T, 64, mode=3) is None                        # no such mode
    assert eng.pack16_case(f(T * 64), xp, T, 64, mode=2) is None                        # mode 2 without scale / shift rows
    assert eng.pack16_case(f(17 * 64), xp, 17, 64) is None and eng.pack16_case(f(64), xp, 0, 64) is None
    torch.cuda.synchronize()


def test_refusals(eng):
    """host side only: vv_gemv16p_launch2 says no, vv_gemv16p_case returns VV_GEMV_REFUSED (None here) and nothing is launched.  The
    `assert not refused` lines launch a legal all-zero case: they show that it is the one changed argument that is refused."""
    d = eng.device
    f = lambda n: torch.zeros(n, device=d)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=d)
    wp = lambda N, K: u8(int(eng.lib.vv_packed_bytes(N, K)))
    T, N, K = 4, 32, 64
    base = dict(wp=wp(N, K), xp=u8(4096), T=T, N=N, K=K, epi=BIAS, y=f(17 * 64))

    def refused(**over):
        a = dict(base)
        a.update(over)
        return eng.gemv16p_case(a.pop("wp"), a.pop("xp"), a.pop("T"), a.pop("N"), a.pop("K"), **a) is None
    assert not refused()
    assert refused(T=0) and refused(T=17)
    assert refused(K=16, wp=wp(N, 16)) and refused(K=48, wp=wp(N, 48))
    assert refused(N=6, ldy=8, wp=wp(6, K))                                               # N % 4 != 0
    sw = dict(epi=SWIGLU, y=None, w2p=wp(N, K), yp=u8(4096))
    assert not refused(**sw)
    assert refused(**dict(sw, N=12, wp=wp(12, K), w2p=wp(12, K)))                         # SwiGLU stores 8 bytes at a 16-byte slot: N % 8
    pk = dict(epi=RESID, flags=PK, yp=u8(4096), ssq_out=f(64))
    assert not refused(**pk)
    assert refused(**dict(pk, N=24, wp=wp(24, K)))                                        # PK writes whole 16-feature tiles
    assert not refused(flags=RS, ssq_in=f(16), ssq_tiles=1)
    assert refused(flags=RS)                                                              # RS without partials
    assert refused(flags=RS, ssq_tiles=1)
    assert not refused(flags=RS | SH, ssq_in=f(16), ssq_tiles=1, xs=u8(4096))
    assert refused(flags=RS | SH, ssq_in=f(16), ssq_tiles=1)                              # SH without the second operand
    cfg = dict(epi=CFG_DPM, y=None, z=f(16 * N), x0p=f(8 * N), coef=f(6), cfg=1.25)
    assert not refused(**dict(cfg, n_cfg=2))
    assert refused(**dict(cfg, n_cfg=1)) and refused(**dict(cfg, n_cfg=3)) and refused(**dict(cfg, n_cfg=0))   # T != 2 n_cfg
    assert refused(**dict(cfg, n_cfg=2, coef=None))
    rs = dict(ssq_in=f(16), ssq_tiles=1)
    assert refused(epi=RESID, flags=RS, **rs)                                             # pairs without an instantiation
    assert refused(epi=GATED, flags=RS, gate=f(T * N), ld_gate=N, **rs)
    assert refused(flags=SH, xs=u8(4096)) and refused(flags=PK, yp=u8(4096), ssq_out=f(64))
    assert refused(**dict(sw, flags=PK, ssq_out=f(64))) and refused(**dict(cfg, n_cfg=2, flags=RS, **rs))
    assert refused(epi=2) and refused(epi=GATED)                                          # no such epilogue here; gated without a gate
    torch.cuda.synchronize()


def test_wrapper_rejects_bad_arguments(eng):
    """a typo in a test fails in Python, before anything reaches the GPU"""
    d = eng.device
    f = lambda n: torch.zeros(n, device=d)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=d)
    T, N, K = 4, 48, 96
    wp, xp, y = u8(int(eng.lib.vv_packed_bytes(N, K))), u8(3072), f(T * N)
    bad = [
        dict(xp=xp[:-16]),                                             # packed operand: ceil(K / 32) KiB
        dict(wp=wp[:-16]),                                             # packed weights of another shape
        dict(y=y[:-4]),                                                # Y does not cover (T - 1) * ldy + N
        dict(ldy=N + 4),
        dict(ldy=N - 4),
        dict(y=y.double()), dict(y=y.cpu()), dict(y=f(T * N + 4)[1:]), dict(y=f(2 * T * N).reshape(-1, 2)[:, 0]),
        dict(bias=f(N - 4)),
        dict(epi=SWIGLU, w2p=wp, yp=u8(1024)),                         # Yp: ceil(N / 32) KiB
        dict(epi=SWIGLU, yp=u8(2048)),                                 # SwiGLU without the second matrix
        dict(flags=RS, ssq_in=f(16 * 3 - 4), ssq_tiles=3),
        dict(flags=RS, ssq_in=f(16), ssq_tiles=0),
        dict(flags=RS | SH, ssq_in=f(16), ssq_tiles=1, xs=u8(2048)),
        dict(epi=RESID, flags=PK, yp=u8(2048), ssq_out=f(32)),         # ssq_out: ceil(N / 16) * 16
        dict(epi=RESID, flags=PK, yp=u8(2048), ssq_out=f(48), pk_nw=f(N - 4)),
        dict(epi=RESID, flags=PK, yp=u8(2048), ssq_out=f(48), pk_sc=f(T * N), ld_pk=N + 4),
        dict(epi=GATED, gate=f(T * N - 4), ld_gate=N),
        dict(epi=CFG_DPM, y=None, n_cfg=2, z=f(4 * N - 4), x0p=f(2 * N), coef=f(6)),
        dict(epi=CFG_DPM, y=None, n_cfg=2, z=f(4 * N), x0p=f(2 * N - 4), coef=f(6)),
        dict(epi=CFG_DPM, y=None, n_cfg=2, z=f(4 * N), x0p=f(2 * N), coef=f(6), sde_noise=f(N)),
        dict(epi=CFG_DPM, y=None, n_cfg=2, z=f(4 * N), x0p=f(2 * N), coef=f(4)),
        dict(epi=7), dict(flags=8), dict(T=-1), dict(N=0),
    ]
    for over in bad:
        a = dict(wp=wp, xp=xp, T=T, N=N, K=K, epi=BIAS, y=y)
        a.update(over)
        with pytest.raises(ValueError):
            eng.gemv16p_case(a.pop("wp"), a.pop("xp"), a.pop("T"), a.pop("N"), a.pop("K"), **a)
    with pytest.raises(ValueError):
        eng.pack16_case(f(T * K - 4), xp, T, K)
    with pytest.raises(ValueError):
        eng.pack16_case(f(T * K), xp[:-16], T, K)
    with pytest.raises(ValueError):
        eng.pack16_case(f(T * K), xp, T, K, nw=f(K - 4))
    with pytest.raises(ValueError):
        eng.pack16_case(f(T * K), xp, T, K, mode=2, sc=f(T * K), sh=f(T * K - 4), ld_mod=K)
    with pytest.raises(ValueError):
        eng.pack16_tiles_case(f(2 * T * K - 4), u8(6144), T, K, 2, n_inner=2, stride_inner=T * K)
    with pytest.raises(ValueError):
        eng.pack16_tiles_case(f(2 * T * K), u8(6144 - 16), T, K, 2, n_inner=2, stride_inner=T * K)
