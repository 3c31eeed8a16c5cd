"""The host-side GEMM dispatch (csrc/gemv_plan.h) on a machine without a GPU: which compiled form of the decode GEMV a launch takes
(vv_gemv_plan) and which kernel vv_gemm_launch routes a call to (vv_gemm_route).  tests/gemv_plan_probe.hip includes that header
alone and is compiled for the host only; the expected forms were read off the launcher the plan replaced, one case per threshold
and per fall-through of its cascade."""
import os
import subprocess

import pytest

from vibevoice_amd import build as vvbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, RMS, RMS_MOD, ADD_SILU, NORMDW = range(5)
STORE, BIAS, BIAS_GELU, SWIGLU, RESID, GATED, CFG_DPM = range(7)
TILE, GEMV, GENERAL, NO_KERNEL = range(4)          # VV_ROUTE_*
FIELDS = ("xs", "pro", "epi", "T", "N", "K", "kgrid", "n_xa", "n_ya", "sl_n", "sl_T", "ksplit", "n_cfg", "x_row_mod", "x_misaligned")


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemv_plan") / "probe")
    subprocess.run([vvbuild._hipcc(), "--offload-host-only", "-std=c++17", "-I", os.path.join(ROOT, "vibevoice_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "gemv_plan_probe.hip"), "-o", exe], check=True)

    def run(cases):
        """cases: dicts over FIELDS (missing = 0; n_cfg defaults to T / 2 for CFG_DPM) -> one dict of the probe's answers per case"""
        lines = []
        for c in cases:
            c = dict(c)
            if c.get("epi") == CFG_DPM:
                c.setdefault("n_cfg", c["T"] // 2)
            assert not set(c) - set(FIELDS), c
            lines.append(" ".join(str(int(c.get(f, 0))) for f in FIELDS))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        res = [list(map(int, l.split())) for l in out if l.strip()]
        assert len(res) == len(cases)
        return [dict(eligible=bool(r[0]), has_form=bool(r[1]), form=tuple(r[2:7]), grid=(r[7], r[8]), route=r[9]) for r in res]
    return run


def case(xs, pro, epi, T, N, K, **kw):
    return dict(xs=xs, pro=pro, epi=epi, T=T, N=N, K=K, **kw)


XA, YA, K3 = dict(n_xa=2), dict(n_ya=2), dict(kgrid=3)
S25, S21 = dict(sl_n=2, sl_T=5), dict(sl_n=2, sl_T=1)
NOT_ELIGIBLE, NO_FORM = "not eligible", "eligible, no form"
# (case, expected form | NO_FORM | NOT_ELIGIBLE, expected grid.y or None = ceil(T / 16) for 16-row forms, else 1)
PLAN = [
    (case(1, RMS, SWIGLU, 2, 4096, 64), (1, 4, 8, 0, 0), None),                 # 256 tiles: default
    (case(1, RMS, SWIGLU, 2, 4112, 64), (1, 2, 4, 0, 0), None),                 # 257 tiles, T <= 2
    (case(1, RMS, SWIGLU, 3, 4112, 64), (1, 4, 4, 0, 0), None),                 # 257 tiles, T = 3
    (case(1, NONE, RESID, 2, 4112, 64), (1, 4, 8, 0, 0), None),                 # 257 tiles, pair without a 4-wave form: falls through
    (case(2, RMS, SWIGLU, 2, 4112, 64), (2, 4, 8, 0, 0), None),                 # 4-wave forms are xs 1 only
    (case(1, NONE, RESID, 4, 2048, 3072), (1, 4, 16, 0, 0), None),              # 128 tiles, 96 k-tiles
    (case(1, NONE, RESID, 4, 2064, 3072), (1, 4, 8, 0, 0), None),               # 129 tiles
    (case(1, NONE, RESID, 4, 2048, 3040), (1, 4, 8, 0, 0), None),               # 95 k-tiles
    (case(1, RMS, BIAS, 4, 2048, 3072), (1, 4, 8, 0, 0), None),                 # pair without a 16-wave form
    (case(2, NONE, RESID, 4, 2048, 3072), (2, 4, 8, 0, 0), None),
    (case(1, NONE, RESID, 2, 2048, 3072, **K3), (1, 4, 8, 0, 0), 3),            # kgrid disables the 16-wave form
    (case(1, NONE, BIAS, 5, 2048, 64), (1, 16, 8, 0, 0), None),                 # 128 workgroups
    (case(1, NONE, BIAS, 5, 2064, 64), (1, 16, 4, 0, 0), None),                 # 129
    (case(1, NONE, BIAS, 17, 1040, 64), (1, 16, 4, 0, 0), 2),                   # 2 x 65
    (case(1, NONE, BIAS, 17, 1024, 64), (1, 16, 8, 0, 0), 2),                   # 2 x 64
    (case(1, RMS, SWIGLU, 5, 2064, 64), (1, 16, 8, 0, 0), None),                # pair without a 4-wave 16-row form
    (case(2, NONE, BIAS, 5, 2064, 64), (2, 16, 8, 0, 0), None),
    (case(3, NONE, BIAS, 5, 2064, 64), NO_FORM, None),
    (case(1, RMS_MOD, SWIGLU, 16, 64, 64), (1, 16, 4, 0, 0), None),             # 16-row RMS_MOD
    (case(2, RMS_MOD, SWIGLU, 16, 64, 64), NO_FORM, None),
    (case(1, RMS, RESID, 5, 64, 64), NOT_ELIGIBLE, None),                       # (RMS, RESID) has no 16-row form
    (case(1, RMS_MOD, SWIGLU, 2, 4112, 64, **XA), (1, 2, 4, 1, 0), None),
    (case(1, RMS_MOD, SWIGLU, 3, 4112, 64, **XA), (1, 4, 4, 1, 0), None),
    (case(1, RMS_MOD, SWIGLU, 2, 4096, 64, **XA), (1, 4, 8, 1, 0), None),
    (case(2, RMS_MOD, SWIGLU, 2, 4112, 64, **XA), (2, 4, 8, 1, 0), None),
    (case(1, RMS, BIAS, 2, 4112, 64, **XA), (1, 4, 8, 1, 0), None),             # wide consumer is SWIGLU only
    (case(1, RMS, SWIGLU, 2, 64, 64, **XA), NOT_ELIGIBLE, None),
    (case(3, NONE, GATED, 4, 64, 64, **YA), (3, 4, 8, 2, 0), None),
    (case(1, NONE, RESID, 2, 64, 3072, **K3, **YA), (1, 4, 8, 2, 0), 3),
    (case(1, NONE, BIAS, 10, 64, 64, **S25), (1, 16, 8, 0, 1), None),
    (case(1, NONE, BIAS, 10, 2064, 64, **S25), (1, 16, 4, 0, 1), None),
    (case(2, NONE, BIAS, 10, 2064, 64, **S25), (2, 16, 8, 0, 1), None),
    (case(3, NONE, BIAS, 10, 64, 64, **S25), NO_FORM, None),
    (case(1, NONE, BIAS, 2, 64, 64, **S21), (1, 16, 8, 0, 1), None),            # slots use the 16-row form at any T
    (case(1, NONE, STORE, 10, 64, 64, **S25), NOT_ELIGIBLE, None),
]


def test_plan_forms(probe):
    got = probe([c for c, _, _ in PLAN])
    fails = []
    for (c, want, gy), g in zip(PLAN, got):
        if want == NOT_ELIGIBLE:
            ok = not g["eligible"] and not g["has_form"]
        elif want == NO_FORM:
            ok = g["eligible"] and not g["has_form"]
        else:
            grid = ((c["N"] + 15) // 16, gy if gy is not None else ((c["T"] + 15) // 16 if want[1] == 16 else 1))
            ok = g["eligible"] and g["has_form"] and g["form"] == want and g["grid"] == grid
        if not ok:
            fails.append((c, want, g))
    assert not fails, fails


def test_plan_refusals(probe):
    """the host-side refusals of test_gpu_gemv_forms.py::test_refusals that need no device memory"""
    base = case(1, NONE, STORE, 2, 32, 64)
    cfg = lambda T, n: dict(base, pro=RMS_MOD, epi=CFG_DPM, T=T, n_cfg=n)
    refused = [dict(base, K=62), dict(base, K=16), dict(base, N=30), dict(base, x_misaligned=1),
               dict(base, epi=RESID, kgrid=2), dict(base, pro=RMS, epi=BIAS, n_xa=1), dict(base, T=5, epi=RESID, n_ya=2),
               dict(base, pro=RMS, epi=BIAS, x_row_mod=1), cfg(3, 1), cfg(3, 2), cfg(18, 9), cfg(16, 7)]
    got = probe([base, cfg(2, 1)] + refused)
    assert got[0]["eligible"] and got[0]["has_form"] and got[1]["eligible"] and got[1]["has_form"]      # one changed argument is what is refused
    fails = [(c, g) for c, g in zip(refused, got[2:]) if g["eligible"] or g["has_form"] or g["route"] == GEMV]
    assert not fails, fails


def test_route(probe):
    cases = [
        (case(1, NONE, BIAS, 10, 64, 64, **S25), GEMV),
        (case(1, NONE, BIAS, 10, 2064, 64, **S25), GEMV),
        (case(2, NONE, BIAS, 10, 2064, 64, **S25), GEMV),
        (case(3, NONE, BIAS, 10, 64, 64, **S25), NO_KERNEL),                    # slot batches have no general form
        (case(1, NONE, BIAS, 2, 64, 64, **S21), GEMV),
        (case(1, NONE, STORE, 10, 64, 64, **S25), NO_KERNEL),
        (case(1, RMS, SWIGLU, 64, 4096, 256), TILE),                            # tall: 64 workgroups of the tile GEMM
        (case(1, RMS, SWIGLU, 2, 4096, 64), GEMV),
        (case(1, RMS, SWIGLU, 2, 4096, 64, ksplit=2), GENERAL),                 # an explicit K split asks for the general kernel
        (case(3, NONE, BIAS, 5, 2064, 64), GENERAL),                            # eligible, no form at xs 3
        (case(2, RMS_MOD, SWIGLU, 16, 64, 64), GENERAL),
        (case(1, NONE, RESID, 5, 64, 64, **K3), NO_KERNEL),                     # part tensors exist only on the GEMV path
    ]
    got = probe([c for c, _ in cases])
    fails = [(c, want, g["route"]) for (c, want), g in zip(cases, got) if g["route"] != want]
    assert not fails, fails
