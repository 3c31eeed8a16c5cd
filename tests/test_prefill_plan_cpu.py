"""The host-side dispatch of the prefill GEMM (csrc/prefill_plan.h: vv_gemm3_plan, vv_qkv_rope_plan) and of the general kernel
(vv_gemm_general_plan in csrc/gemv_plan.h) on a machine without a GPU.  tests/prefill_plan_probe.hip includes the two headers alone
and is compiled for the host only; the expected plans were read off the launchers the plans replaced, one case per threshold and
per fall-through.  The last part asks the plan what the GPU tests of tests/prefill_shapes.py claim to run."""
import os
import subprocess

import pytest

import prefill_shapes as ps
from vibevoice_amd import build as vvbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, RMS, RMS_MOD, ADD_SILU = range(4)
STORE, BIAS, BIAS_GELU, SWIGLU, RESID, GATED, CFG_DPM, QKV_ROPE = range(8)
G4, G3, G3_DB = range(3)                            # VV_PF_*
TILE, GEMV, GENERAL, NO_KERNEL = range(4)           # VV_ROUTE_*
NO_FORM = -3                                        # VV_RC_NO_FORM
BIG = 1 << 30
PLAN_FIELDS = ("form", "epi", "n_blocks", "t_blocks", "grid_x", "grid_y", "block", "lds", "full_idx", "split", "ks")
GEN_FIELDS = ("vec", "dual", "wpb", "maxr", "nt", "ks", "t_pad", "grid_x", "grid_y", "lds")


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prefill_plan") / "probe")
    subprocess.run([vvbuild._hipcc(), "--offload-host-only", "-std=c++17", "-I", os.path.join(ROOT, "vibevoice_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "prefill_plan_probe.hip"), "-o", exe], check=True)

    def run(lines):
        """lines: probe input lines -> one list of ints per line"""
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        res = [list(map(int, l.split())) for l in out if l.strip()]
        assert len(res) == len(lines)
        return res
    return run


def g3(T, N, K, epi=STORE, ldy=None, w2=True, y=True, yp=True, ws=True, g3_bytes=None):
    """ws: the partial-round workspace and (unless g3_bytes says otherwise) ample short-prompt partial tensors"""
    g3_bytes = (BIG if ws else 0) if g3_bytes is None else g3_bytes
    return f"g3 {T} {N} {K} {N if ldy is None else ldy} {epi} {int(w2)} {int(y)} {int(yp)} {int(ws)} {g3_bytes}"


def plans(probe, lines):
    """-> (rc, dict over PLAN_FIELDS or None) per line"""
    return [(r[0], dict(zip(PLAN_FIELDS, r[1:])) if len(r) > 1 else None) for r in probe(lines)]


def check(probe, cases):
    """cases: (probe line, expected subset of the plan) -- every plan also has rc 0 and the block / LDS size of its form"""
    fails = []
    for (line, want), (rc, p) in zip(cases, plans(probe, [c for c, _ in cases])):
        ok = rc == 0 and p is not None and all(p[k] == v for k, v in want.items())
        ok = ok and (p["block"], p["lds"]) == ((512, 128 * 1024) if p["form"] == G4 else (256, 0))
        ok = ok and (p["form"] != G4 or (p["grid_y"] == 1 and p["ks"] == 1)) and (p["form"] == G4 or (p["split"] == 1 and p["grid_y"] == p["ks"]))
        if not ok:
            fails.append((line, want, rc, p))
    assert not fails, fails


def g4_whole(nb, tb, epi):
    return dict(form=G4, epi=epi, n_blocks=nb, t_blocks=tb, grid_x=nb * tb, full_idx=0, split=1)


def test_chip_fill_boundary(probe):
    """the 256 x 256 kernel from 256 workgroups on (16 feature tiles per workgroup, 8 per matrix for SwiGLU); STORE runs the BIAS kernel"""
    check(probe, [
        (g3(4096, 4096, 64, STORE), g4_whole(16, 16, BIAS)),
        (g3(4096, 3840, 64, STORE), dict(form=G3, epi=BIAS, n_blocks=30, t_blocks=32, grid_x=960, ks=1)),
        (g3(4096, 2048, 64, SWIGLU), g4_whole(16, 16, SWIGLU)),
        (g3(4096, 1920, 64, SWIGLU), dict(form=G3, epi=SWIGLU, n_blocks=30, t_blocks=32, grid_x=960, ks=1)),
        (g3(4096, 4096, 64, RESID), g4_whole(16, 16, RESID)),
        (g3(4096, 4096, 64, BIAS), g4_whole(16, 16, BIAS)),
    ])


def test_partial_round_split(probe):
    """the K-split of the tiles past the last whole round of 256 workgroups: the 7B projections at T = 10,922, then one case per cap"""
    check(probe, [
        (g3(10922, 4608, 3584, BIAS), dict(form=G4, n_blocks=18, t_blocks=43, full_idx=96, split=7, grid_x=824)),      # QKV: 774 tiles
        (g3(10922, 3584, 3584, RESID), g4_whole(14, 43, RESID)),                        # o: halves of K = 3584 do not pay
        (g3(10922, 18944, 3584, SWIGLU), g4_whole(148, 43, SWIGLU)),                    # gate/up: 6364 tiles, whole
        (g3(10922, 3584, 18944, RESID), dict(form=G4, full_idx=64, split=2, grid_x=704)),   # down: halves of a long K do
        (g3(4100, 4112, 2080, STORE), dict(form=G4, n_blocks=17, t_blocks=17, full_idx=32, split=4, grid_x=416)),
        (g3(4100, 4112, 2080, SWIGLU), dict(form=G4, n_blocks=33, t_blocks=17, full_idx=64, split=4, grid_x=736)),
        (g3(4100, 4112, 16384, STORE), dict(form=G4, split=6, grid_x=496)),             # 32 / 5 remainder tiles
        (g3(4352, 8192, 16384, STORE), dict(form=G4, split=8, grid_x=768)),             # capped at 8
        (g3(1100, 8200, 1024, SWIGLU), g4_whole(65, 5, SWIGLU)),                        # 3 -> 2 (parts of >= 8 steps) -> 1 (halves of a short K)
        (g3(2100, 7420, 1568, STORE), dict(form=G4, n_blocks=29, t_blocks=9, full_idx=32, split=3, grid_x=280)),       # 25 steps / 8
        (g3(2100, 7420, 1568, SWIGLU), dict(form=G4, n_blocks=58, t_blocks=9, full_idx=64, split=3, grid_x=560)),
    ])
    # without the workspace every one of them is computed whole
    shapes = [(10922, 4608, 3584, BIAS), (10922, 3584, 18944, RESID), (4100, 4112, 2080, STORE), (4100, 4112, 2080, SWIGLU),
              (4100, 4112, 16384, STORE), (4352, 8192, 16384, STORE), (1100, 8200, 1024, SWIGLU), (2100, 7420, 1568, STORE)]
    lines = [g3(T, N, K, e, ws=False) for T, N, K, e in shapes]
    for line, (rc, p) in zip(lines, plans(probe, lines)):
        assert rc == 0 and p["form"] == G4 and p["split"] == 1 and p["full_idx"] == 0 and p["grid_x"] == p["n_blocks"] * p["t_blocks"], (line, p)


def test_short_prompt_split(probe):
    """K over grid.y below 128 workgroups, up to ~192, parts of >= 4 steps, at most 8; two stage buffers up to 512 workgroups"""
    check(probe, [
        (g3(330, 1536, 8960), dict(form=G3_DB, n_blocks=12, t_blocks=3, grid_x=36, ks=6)),
        (g3(330, 2048, 1536), dict(form=G3_DB, grid_x=48, ks=4)),
        (g3(75, 896, 4864), dict(form=G3_DB, grid_x=7, ks=8)),
        (g3(500, 36, 3584), dict(form=G3_DB, grid_x=4, ks=8)),
        (g3(384, 2048, 1024, SWIGLU), dict(form=G3_DB, epi=SWIGLU, ks=1)),              # SwiGLU never splits
        (g3(128, 16256, 1024), dict(form=G3_DB, grid_x=127, ks=2)),
        (g3(128, 16384, 1024), dict(form=G3_DB, grid_x=128, ks=1)),
        (g3(512, 16384, 64), dict(form=G3_DB, grid_x=512, ks=1)),
        (g3(512, 16400, 64), dict(form=G3, grid_x=516, ks=1)),
        (g3(330, 1536, 8960, ws=False), dict(form=G3_DB, grid_x=36, ks=1)),
        # the partial tensors are all or nothing
        (g3(330, 1536, 8960, g3_bytes=6 * 330 * 1536 * 4), dict(form=G3_DB, ks=6)),
        (g3(330, 1536, 8960, g3_bytes=6 * 330 * 1536 * 4 - 1), dict(form=G3_DB, ks=1)),
    ])


def test_refusals(probe):
    base = dict(T=128, N=128, K=64)
    bad = [g3(0, 128, 64), g3(128, 128, 16), g3(128, 30, 64), g3(**base, epi=SWIGLU, w2=False), g3(**base, epi=SWIGLU, yp=False),
           g3(**base, epi=RESID, y=False), g3(**base, epi=RESID, ldy=6), g3(**base, epi=STORE, y=False), g3(**base, epi=BIAS, ldy=6),
           g3(4096, 4096, 64, epi=SWIGLU, w2=False), g3(4096, 4096, 64, epi=RESID, ldy=6)]
    no_form = [g3(**base, epi=e) for e in (BIAS_GELU, GATED, CFG_DPM, QKV_ROPE)] + [g3(4096, 4096, 64, epi=BIAS_GELU)]
    ok = [g3(**base, epi=e) for e in (STORE, BIAS, RESID, SWIGLU)] + [g3(**base, epi=SWIGLU, y=False), g3(**base, epi=RESID, w2=False, yp=False)]
    got = plans(probe, bad + no_form + ok)
    assert [rc for rc, _ in got] == [-1] * len(bad) + [NO_FORM] * len(no_form) + [0] * len(ok), got


def test_qkv_rope(probe):
    q = lambda T, K=3584, D=128, Hq=28, Hkv=4, ops=1, ws=1: f"qkv {T} {K} {D} {Hq} {Hkv} {ops} {ws}"
    got = plans(probe, [q(3584), q(3585), q(3585, D=64), q(3585, Hq=27), q(3585, ops=0), q(10922), q(10922, ws=0), q(3585, K=16), q(0)])
    assert [rc for rc, _ in got] == [0, 1, 0, 0, 0, 1, 1, 0, 0], got      # 18 x 14 = 252 tiles; 270; D = 64; N = 4480; an operand missing
    want = dict(form=G4, epi=QKV_ROPE, n_blocks=18, t_blocks=15, full_idx=32, split=7, grid_x=368, grid_y=1, block=512, lds=128 * 1024, ks=1)
    assert all(got[1][1][k] == v for k, v in want.items()), got[1]              # 14 tiles past the round: two on an XCD at most
    assert (got[5][1]["full_idx"], got[5][1]["split"], got[5][1]["grid_x"]) == (96, 7, 824), got[5]      # the plain QKV GEMM's split
    assert (got[6][1]["full_idx"], got[6][1]["split"], got[6][1]["grid_x"]) == (0, 1, 774), got[6]


def test_the_thin_layer_reaches_the_qkv_rope_epilogue(probe):
    """test_gpu_attn_long.py::test_qkv_rope_epilogue_append: lm_shapes.QKV_ROPE_* is a shape vv_qkv_rope_plan takes -- 18 x 15 = 270
    workgroups of the 256 x 256 kernel with the VV_EPI_QKV_ROPE epilogue -- on an engine that has the partial-round workspace"""
    import lm_shapes as ls
    c, T = ls.QKV_ROPE_CFG, ls.QKV_ROPE_ROWS
    assert (c.heads + 2 * c.kv_heads) * c.head_dim == 4608 and T >= 1024 and c.hidden % 8 == 0 and c.inter % 8 == 0
    (rc, p), (rc1, _) = plans(probe, [f"qkv {T} {c.hidden} {c.head_dim} {c.heads} {c.kv_heads} 1 1",
                                      f"qkv {T - 272} {c.hidden} {c.head_dim} {c.heads} {c.kv_heads} 1 1"])
    assert rc == 1 and rc1 == 0, (rc, rc1)          # 3328 rows are 13 row blocks: 234 workgroups, the plain GEMM + vv_rope_append
    want = dict(form=G4, epi=QKV_ROPE, n_blocks=18, t_blocks=15, grid_y=1, block=512, lds=128 * 1024, ks=1)
    assert all(p[k] == v for k, v in want.items()), p
    assert p["grid_x"] >= 270


def engine_ws(geometry, max_rows, xsplit=1):
    """what vv_create's workspace offers an engine of that geometry: (partial round?, bytes of the short-prompt partial tensors)"""
    from test_gpu_geometry import GEOM
    c = GEOM[geometry]
    qkv, attn = (c.heads + 2 * c.kv_heads) * c.head_dim, c.heads * c.head_dim
    if xsplit != 1 or max_rows < 64 or c.hidden % 8 or attn % 8 or c.inter % 8:
        return False, 0
    return max_rows >= 1024, 8 * min(max_rows, 1024) * max(qkv, c.hidden) * 4


def test_the_gpu_tests_run_the_kernels_they_name(probe):
    rnd, g3b = engine_ws(*ps.K_SPLIT_ROUND_ENGINE)
    assert rnd
    lines = [g3(T, N, K, e, ws=True, g3_bytes=g3b) for T, N, K in ps.K_SPLIT_ROUND for e in ps.K_SPLIT_ROUND_EPIS]
    got = plans(probe, lines)
    for line, (rc, p) in zip(lines, got):
        assert rc == 0 and p["form"] == G4 and p["split"] > 1, (line, rc, p)
    assert len({p["split"] for _, p in got}) >= 2, sorted({p["split"] for _, p in got})
    unsplit = plans(probe, [g3(T, N, K, e, ws=False) for T, N, K in ps.K_SPLIT_ROUND for e in ps.K_SPLIT_ROUND_EPIS])     # gemm3_raw(ksplit=False)
    assert all(rc == 0 and p["form"] == G4 and p["split"] == 1 for rc, p in unsplit), unsplit

    rnd, g3b = engine_ws(*ps.SHORT_PROMPT_ENGINE)
    assert not rnd and g3b > 0
    for ws_bytes, split in ((g3b, True), (0, False)):
        lines = [g3(T, N, K, e, ws=False, g3_bytes=ws_bytes) for T, N, K in ps.SHORT_PROMPT for e in ps.SHORT_PROMPT_EPIS]
        for line, (rc, p) in zip(lines, plans(probe, lines)):
            assert rc == 0 and p["form"] == G3_DB and (p["ks"] > 1) == split, (line, rc, p)

    n4 = ps.PREFILL_GEMM3_ON_G4                     # test_prefill_gemm3's engine runs the exact mode: no K-split workspace
    for k, (T, N, K) in enumerate(ps.PREFILL_GEMM3):
        for (rc, p) in plans(probe, [g3(T, N, K, e, ws=False) for e in ps.PREFILL_GEMM3_EPIS]):
            assert rc == 0 and (p["form"] == G4) == (k >= len(ps.PREFILL_GEMM3) - n4), (T, N, K, p)


# ---- the general kernel of gemm.hip ----
def gen(xs, pro, epi, T, N, K, ksplit=0, x_mis=0, w2=1):
    return f"gen {xs} {pro} {epi} {T} {N} {K} {ksplit} {x_mis} {w2}"


def test_general_kernel_plan(probe):
    """one case per rule of vv_gemm_general_plan, each on a shape vv_gemm_route sends to the general kernel: (NONE, BIAS_GELU) has no
    GEMV form; at xs 3 nothing above four rows has one and the tile GEMM is out"""
    P = lambda vec, dual, wpb, maxr, nt, ks, t_pad, gx, gy, lds: dict(zip(GEN_FIELDS, (vec, dual, wpb, maxr, nt, ks, t_pad, gx, gy, lds)))
    cases = [
        (gen(1, NONE, BIAS_GELU, 4, 64, 64), P(1, 0, 8, 4, 1, 1, 4, 1, 1, 16384)),          # up to 4 rows: 8 waves
        (gen(1, NONE, BIAS_GELU, 5, 64, 64), P(1, 0, 4, 16, 1, 1, 5, 1, 1, 10240)),         # 5 rows: 4 waves
        (gen(3, NONE, BIAS, 16, 65536, 64), P(1, 0, 4, 16, 2, 1, 16, 512, 1, 98304)),       # 4096 tile pairs: two tiles per wave
        (gen(3, NONE, BIAS, 16, 65520, 64), P(1, 0, 4, 16, 1, 1, 16, 1024, 1, 98304)),      # 4095
        (gen(3, NONE, BIAS, 17, 32768, 64), P(1, 0, 4, 16, 2, 1, 16, 256, 2, 98304)),       # 2048 x 2 row tiles
        (gen(1, NONE, BIAS_GELU, 4, 8192, 4096), P(1, 0, 8, 4, 1, 4, 4, 256, 1, 16384)),    # ks = 2048 / 512 waves
        (gen(1, NONE, BIAS_GELU, 5, 1024, 1024), P(1, 0, 4, 16, 1, 4, 5, 64, 1, 10240)),    # ks capped by 32 k-tiles / 8
        (gen(1, NONE, BIAS_GELU, 5, 64, 4096), P(1, 0, 4, 16, 1, 4, 5, 4, 1, 10240)),       # ks capped by the waves of a block
        (gen(1, NONE, BIAS_GELU, 4, 1024, 1024), P(1, 0, 8, 4, 1, 8, 4, 64, 1, 16384)),     # few tiles: widened from 4 to one tile per workgroup
        (gen(1, NONE, BIAS_GELU, 4, 8176, 4096), P(1, 0, 8, 4, 1, 8, 4, 511, 1, 16384)),    # 511 tiles: still few
        (gen(1, RMS, SWIGLU, 2, 4096, 64, ksplit=2), P(1, 1, 8, 4, 1, 2, 2, 64, 1, 18432)),  # explicit K split
        (gen(1, NONE, BIAS_GELU, 4, 1024, 1024, ksplit=1), P(1, 0, 8, 4, 1, 1, 4, 8, 1, 16384)),     # ... is not widened
        (gen(3, NONE, STORE, 5, 20, 7), P(0, 0, 4, 16, 1, 1, 5, 1, 1, 30720)),              # unaligned K: the generic form
        (gen(1, NONE, STORE, 2, 64, 64, x_mis=1), P(0, 0, 4, 16, 1, 1, 2, 1, 1, 5120)),     # unaligned rows
    ]
    got = probe([c for c, _ in cases])
    fails = [(c, want, r) for (c, want), r in zip(cases, got) if r[:2] != [0, GENERAL] or dict(zip(GEN_FIELDS, r[2:])) != want]
    assert not fails, fails
    refused = probe([gen(1, RMS, SWIGLU, 2, 64, 62), gen(1, RMS, SWIGLU, 2, 64, 64, x_mis=1), gen(1, RMS, SWIGLU, 2, 64, 62, w2=0)])
    assert refused == [[NO_FORM, GENERAL], [NO_FORM, GENERAL], [-1, GENERAL]], refused
