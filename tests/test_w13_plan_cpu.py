"""Which launches stream W13 twins, decided on the host (csrc/gemv_plan.h: vv_gemv_w13_form; csrc/pass_plan.h: the LM plan's w13 flag),
on a machine without a GPU.  tests/w13_plan_probe.hip includes the two headers alone and is compiled for the host only.

  the four launches of a 7B LM layer (QKV 4608 x 3584, o 3584 x 3584, gate/up 18944 x 3584, down 3584 x 18944) have a W13 form at
  T = 1 and T = 2, in the forms vv_gemv_plan gives them: QKV and gate/up 2 rows x 4 waves, o and down the default 4 rows x 8 waves
  no form: K split over three workgroup columns (the 1.5B down projection), a part-consuming QKV, T = 5, the exact modes (xs = 2)
  the LM plan's flag: set on the GEMV route of one utterance (<= 2 rows) where the context has twins, and nowhere else"""
import os
import subprocess

import pytest

from vibevoice_amd import build as vvbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, RMS = 0, 1
BIAS, SWIGLU, RESID = 1, 3, 4
PREFILL, P16, GEMV = range(3)                       # VV_LM_*
H, QKV, I = 3584, 4608, 18944                       # 7B widths


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("w13_plan") / "probe")
    subprocess.run([vvbuild._hipcc(), "--offload-host-only", "-std=c++17", "-I", os.path.join(ROOT, "vibevoice_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "w13_plan_probe.hip"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        res = [tuple(map(int, l.split())) for l in out if l.strip()]
        assert len(res) == len(lines)
        return res
    return run


def form(pro, epi, T, N, K, xs=1, kgrid=0, n_xa=0):
    return f"form {xs} {pro} {epi} {T} {N} {K} {kgrid} {n_xa}"


LAYER = {"qkv": (RMS, BIAS, QKV, H, (2, 4)), "o": (NONE, RESID, H, H, (4, 8)), "gate_up": (RMS, SWIGLU, I, H, (2, 4)),
         "down": (NONE, RESID, H, I, (4, 8))}


@pytest.mark.parametrize("T", [1, 2])
def test_the_7b_layer_launches_have_a_form(probe, T):
    got = probe([form(pro, epi, T, N, K) for pro, epi, N, K, _ in LAYER.values()])
    for (name, spec), (idx, mr, wpb) in zip(LAYER.items(), got):
        assert idx >= 0 and (mr, wpb) == spec[4], (name, idx, mr, wpb)
    assert len({g[0] for g in got}) == 3          # o and down share the residual form


def test_launches_without_a_form(probe):
    cases = {
        "1.5B down, K over three columns": form(NONE, RESID, 2, 1536, 8960, kgrid=3),
        "the same shape unsplit: the 16-wave form": form(NONE, RESID, 2, 1536, 8960),
        "7B down, K over three columns": form(NONE, RESID, 2, H, I, kgrid=3),
        "part-consuming QKV": form(RMS, BIAS, 2, QKV, H, n_xa=2),
        "T = 5": form(RMS, SWIGLU, 5, I, H),
        "T = 5, down": form(NONE, RESID, 5, H, I),
        "xs = 2": form(RMS, SWIGLU, 2, I, H, xs=2),
        "xs = 2, down": form(NONE, RESID, 2, H, I, xs=2),
        "K without whole groups": form(NONE, RESID, 2, H, I + 32),
        "the default form of a narrow QKV": form(RMS, BIAS, 2, 2048, 1536),
    }
    got = dict(zip(cases, probe(list(cases.values()))))
    for name, (idx, mr, wpb) in got.items():
        assert idx == -1, (name, idx)


def lm(rows, w13=True, tile3=True, attn2=True, p16=True):
    return f"lm {int(w13)} {int(tile3)} {int(attn2)} {int(p16)} {len(rows)} " + " ".join(f"{c} {p}" for c, p in rows)


def test_the_lm_flag_is_set_on_the_gemv_route_alone(probe):
    distinct = lambda n: [(i, 40 + i) for i in range(n)]
    span = lambda n: [(0, 10 + i) for i in range(n)]
    cases = [
        (lm(distinct(1)), GEMV, 1), (lm(distinct(2)), GEMV, 1),                   # one utterance: cond, cond + uncond
        (lm(distinct(2), w13=False), GEMV, 0),                                    # a context without twins
        (lm(distinct(3)), GEMV, 0), (lm(distinct(4)), GEMV, 0),                   # more rows: the bf16 launches
        (lm(distinct(5)), P16, 0), (lm(distinct(16)), P16, 0),                    # batch decode
        (lm(distinct(5), p16=False), GEMV, 0),
        (lm(span(64)), PREFILL, 0), (lm(span(256)), PREFILL, 0),                  # prompt chunks
        (lm(span(8)), GEMV, 0), (lm(span(63)), GEMV, 0),
        (lm([(0, 5), (0, 9)]), GEMV, 1),                                          # two rows of one cache: still the decode GEMV
    ]
    got = probe([c for c, _, _ in cases])
    for (line, route, flag), (rc, r, f) in zip(cases, got):
        assert rc == 0 and (r, f) == (route, flag), (line, rc, r, f)
