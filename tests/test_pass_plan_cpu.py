"""The routing of one LM pass and of the diffusion head (csrc/pass_plan.h: vv_lm_pass_plan, vv_head_plan) on a machine without a
GPU.  tests/pass_plan_probe.hip includes the header alone and is compiled for the host only; the expected plans were read off the
launch code the plans replaced (vv_lm_forward_range / lm_body / lm_gemv_layer, head_eval / sample_body), one case per threshold and
per fall-through.  The last part asks the plan what the GPU tests of tests/lm_shapes.py claim to run."""
import os
import subprocess

import pytest

import lm_shapes as ls
from vibevoice_amd import build as vvbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILL, P16, GEMV = range(3)                       # VV_LM_*
FUSED, PREFILL4, SPLIT_MERGE = range(3)             # VV_ATTN_*
ADA_PER_STEP, ADA_TILE, ADA_ROWS16 = range(3)       # VV_ADA_*
HEAD_P16, HEAD_GEMV = range(2)                      # VV_HEAD_*
FINAL_P16_CFG, FINAL_SEAM, FINAL_GEMM_CFG, FINAL_GEMM = range(4)     # VV_FINAL_*
LM_FIELDS = ("fused", "contiguous", "route", "attn", "attn_S", "attn_groups", "zero_v_tail", "key_mode", "key_split", "kv_positions")


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass_plan") / "probe")
    subprocess.run([vvbuild._hipcc(), "--offload-host-only", "-std=c++17", "-I", os.path.join(ROOT, "vibevoice_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pass_plan_probe.hip"), "-o", exe], check=True)

    def run(lines):
        """lines: probe input lines -> one list of ints per line"""
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        res = [list(map(int, l.split())) for l in out if l.strip()]
        assert len(res) == len(lines)
        return res
    return run


def lm(rows, ws=64, splits=128, hkv=2, tile3=True, attn2=True, p16=True):
    return f"lm {ws} {splits} {hkv} {int(tile3)} {int(attn2)} {int(p16)} {len(rows)} " + " ".join(f"{c} {p}" for c, p in rows)


EXACT = dict(tile3=False, attn2=False, p16=False)   # what an engine of the exact modes (xsplit 2, 3) offers


def lm_plans(probe, lines):
    """-> (rc, dict over LM_FIELDS; a refused launch has fused and contiguous only) per line"""
    return [(r[0], dict(zip(LM_FIELDS, r[1:]))) for r in probe(lines)]


def check_lm(probe, cases):
    """cases: (probe line, expected subset of the plan); every plan has rc 0"""
    got = lm_plans(probe, [c for c, _ in cases])
    fails = [(line, want, rc, p) for (line, want), (rc, p) in zip(cases, got) if rc != 0 or any(p[k] != v for k, v in want.items())]
    assert not fails, fails


def distinct(n, pos=10):
    return [(i, pos + i) for i in range(n)]


def test_split_counts(probe):
    """one split per 1024 positions of the longest row, at most attn_splits, and no more than puts ~256 workgroups (splits x kv heads x
    long rows) on the chip"""
    check_lm(probe, [
        (lm([(0, 0)]), dict(attn_S=1, kv_positions=1)),
        (lm([(0, 1023)]), dict(attn_S=1, kv_positions=1024)),
        (lm([(0, 1024)]), dict(attn_S=2, key_split=2, kv_positions=1025)),
        (lm([(0, 32767)]), dict(attn_S=32)),
        (lm([(0, 32767)], splits=4), dict(attn_S=4)),                   # attn_splits below both other bounds
        (lm([(i, 32767) for i in range(8)], hkv=2), dict(attn_S=16, key_split=16, route=P16)),      # 256 / (8 x 2)
        (lm([(i, 32767) for i in range(8)], hkv=4), dict(attn_S=8)),    # 256 / (8 x 4)
        (lm([(0, 32767), (1, 5)], hkv=2), dict(attn_S=32)),             # only rows past 1024 positions count as long
        (lm([(i, 32767) for i in range(16)], hkv=8, splits=1), dict(attn_S=1)),
        (lm([(i, 32767) for i in range(64)], hkv=8), dict(attn_S=1, route=GEMV)),          # 256 / 512 rounds up to one
    ])


def test_decode_rows_on_distinct_caches(probe):
    """fused attention; the packed-activation projections for 5..16 rows when the context has their buffers"""
    fused = dict(fused=1, contiguous=0, attn=FUSED, attn_S=1, attn_groups=0, zero_v_tail=0, key_mode=1, key_split=1)
    check_lm(probe, [
        (lm(distinct(1)), dict(fused, route=GEMV)),
        (lm(distinct(4)), dict(fused, route=GEMV)),
        (lm(distinct(5)), dict(fused, route=P16)),
        (lm(distinct(16)), dict(fused, route=P16)),
        (lm(distinct(17)), dict(fused, route=GEMV)),
        (lm(distinct(5), p16=False), dict(fused, route=GEMV)),
        (lm(distinct(8)), dict(fused, route=P16)),                      # fused wins over contiguous
        (lm([(i, 7) for i in range(8)], **EXACT), dict(fused, route=GEMV)),
    ])


def test_ragged_and_small_row_sets(probe):
    """rows that share a cache without being a chunk of >= 8 consecutive positions: rope/append, then the split + merge pair"""
    ragged = dict(fused=0, contiguous=0, route=GEMV, attn=SPLIT_MERGE, attn_groups=1, zero_v_tail=0, key_mode=0, key_split=1)
    gap = ls.span(0, 5, 4) + ls.span(0, 10, 4)
    check_lm(probe, [
        (lm([(0, 5), (0, 6)]), ragged),
        (lm(ls.span(0, 5, 7)), dict(ragged, kv_positions=63)),          # 7 consecutive rows are not a chunk
        (lm(gap), ragged),
        (lm(ls.span(0, 0, 7) + [(1, 7)]), ragged),                      # consecutive positions, two caches
        (lm(ls.span(0, 0, 8) + [(1, 3)]), ragged),                      # 5..16 rows that share caches: never the batch-decode route
        (lm(gap, ws=8), ragged),                                        # exactly ws_rows rows: one launch of the pair
        (lm(ls.span(0, 1020, 7)), dict(ragged, attn_S=2, key_split=2)),
    ])


def test_contiguous_chunks(probe):
    chunk = dict(fused=0, contiguous=1, key_mode=2)
    p4 = dict(chunk, route=GEMV, attn=PREFILL4, attn_groups=0, zero_v_tail=1, key_split=0)
    check_lm(probe, [
        # bf16 mode: vv_attn_prefill4 from 8 rows on (the V tail zeroed, no split count in the key), the packed pass from 64
        (lm(ls.span(0, 0, 8)), p4),
        (lm(ls.span(0, 100, 63)), p4),
        (lm(ls.span(0, 2000, 8)), dict(p4, attn_S=2)),                  # the split count exists, the key does not carry it
        (lm(ls.span(0, 0, 64)), dict(chunk, route=PREFILL, attn=PREFILL4, attn_groups=0, zero_v_tail=1, key_split=0)),
        (lm(ls.span(0, 0, 64), tile3=False), p4),                       # no packed-activation buffers: GEMV layers + vv_attn_prefill4
        (lm(ls.span(0, 0, 65), ws=64), dict(chunk, route=PREFILL)),     # a chunk may exceed ws_rows
        # exact modes: every chunk through the split + merge pair, ws_rows rows per launch; the key carries the split count
        (lm(ls.span(0, 0, 512), **EXACT), dict(chunk, route=GEMV, attn=SPLIT_MERGE, attn_groups=8, zero_v_tail=0, attn_S=1, key_split=1)),
        (lm(ls.span(0, 600, 512), **EXACT), dict(chunk, route=GEMV, attn=SPLIT_MERGE, attn_groups=8, attn_S=2, key_split=2)),   # 88 long rows x 2 kv heads
        (lm(ls.span(0, 0, 8), **EXACT), dict(chunk, route=GEMV, attn=SPLIT_MERGE, attn_groups=1, zero_v_tail=0)),
        (lm(ls.span(0, 0, 65), **EXACT), dict(chunk, attn=SPLIT_MERGE, attn_groups=2)),
        # the packed pass without vv_attn_prefill4 elsewhere (no engine offers this): the pass still zeroes its V tail, the key says attn_S
        (lm(ls.span(0, 0, 64), attn2=False), dict(chunk, route=PREFILL, attn=PREFILL4, zero_v_tail=1, key_split=1)),
    ])


def test_refusal(probe):
    """a launch that is not one chunk takes at most ws_rows rows"""
    two = ls.span(0, 0, 33) + ls.span(1, 0, 32)
    got = lm_plans(probe, [lm(two, ws=64), lm(two[:64], ws=64), lm(ls.span(0, 0, 32) + ls.span(0, 33, 33), ws=64), lm(distinct(65), ws=64),
                           lm(ls.span(0, 0, 65), ws=64), lm(distinct(17), ws=16)])
    assert [rc for rc, _ in got] == [-1, 0, -1, -1, 0, -1], got
    assert (got[0][1]["fused"], got[0][1]["contiguous"]) == (0, 0) and got[3][1]["fused"] == 1


# ---- the diffusion head ----
def head(rows, n_steps=5, HF=384, HL=2, MODW=1024, p16=True, shift=True, ada_p=True, mod_all=True, tail=True, coef=True):
    return f"head {rows} {n_steps} {HF} {HL} {MODW} {int(p16)} {int(shift)} {int(ada_p)} {int(mod_all)} {int(tail)} {int(coef)}"


def check_head(probe, cases):
    """cases: (probe line, (ada, sh_tiles, layers, [final stage per step])); solver_step is false for every plan of a shipped table and
    for vv_head_forward's -- all this probe asks for (the general table's plans: test_solver_family_cpu.py)"""
    got = probe([c for c, _ in cases])
    fails = [(line, want, r) for (line, want), r in zip(cases, got) if (r[0], r[1], r[2], r[4:]) != want or r[3] != 0]
    assert not fails, fails


def test_head_layer_and_final_routes(probe):
    check_head(probe, [
        (head(2), (ADA_ROWS16, 0, HEAD_GEMV, [FINAL_SEAM] * 4 + [FINAL_GEMM_CFG])),        # the seam on every step but the last
        (head(2, n_steps=1), (ADA_ROWS16, 0, HEAD_GEMV, [FINAL_GEMM_CFG])),
        (head(2, tail=False), (ADA_ROWS16, 0, HEAD_GEMV, [FINAL_GEMM_CFG] * 5)),
        (head(4), (ADA_ROWS16, 0, HEAD_GEMV, [FINAL_GEMM_CFG] * 5)),                       # only decode rows (one utterance) take the seam
        (head(6), (ADA_ROWS16, 1, HEAD_P16, [FINAL_P16_CFG] * 5)),
        (head(16, n_steps=2), (ADA_ROWS16, 1, HEAD_P16, [FINAL_P16_CFG] * 2)),
        (head(6, shift=False), (ADA_ROWS16, 0, HEAD_P16, [FINAL_GEMM_CFG] * 5)),           # without the shift tiles: P16 layers, the GEMM's final layer
        (head(16, n_steps=2, shift=False), (ADA_ROWS16, 0, HEAD_P16, [FINAL_GEMM_CFG] * 2)),
        (head(6, HF=400), (ADA_ROWS16, 1, HEAD_GEMV, [FINAL_GEMM_CFG] * 5)),               # HF % 32 != 0; the tiles are still packed
        (head(6, p16=False, shift=False), (ADA_ROWS16, 0, HEAD_GEMV, [FINAL_GEMM_CFG] * 5)),
        (head(6, HL=0, MODW=256), (ADA_ROWS16, 1, HEAD_P16, [FINAL_GEMM_CFG] * 5)),        # no layer whose down projection could pack the operand
        (head(6, mod_all=False), (ADA_PER_STEP, 0, HEAD_P16, [FINAL_GEMM_CFG] * 5)),       # no batched modulations: no tiles of them either
        # vv_head_forward: one evaluation without solver coefficients
        (head(8, n_steps=1, coef=False), (ADA_PER_STEP, 0, HEAD_P16, [FINAL_GEMM])),
        (head(4, n_steps=1, coef=False), (ADA_PER_STEP, 0, HEAD_GEMV, [FINAL_GEMM])),
        (head(5, n_steps=1, coef=False), (ADA_PER_STEP, 0, HEAD_P16, [FINAL_GEMM])),
        (head(16, n_steps=1, coef=False), (ADA_PER_STEP, 0, HEAD_P16, [FINAL_GEMM])),
        (head(2, n_steps=1, coef=False), (ADA_PER_STEP, 0, HEAD_GEMV, [FINAL_GEMM])),
    ])


def test_head_adaln_route(probe):
    """the tile GEMM above 32 (step, row) pairs, when the packed operand exists and MODW is a multiple of 4"""
    ada = lambda r: r[0]
    got = probe([head(2, n_steps=16), head(2, n_steps=17), head(16, n_steps=2), head(16, n_steps=3), head(8, MODW=1022),
                 head(8, ada_p=False), head(8, mod_all=False), head(8)])
    assert [ada(r) for r in got] == [ADA_ROWS16, ADA_TILE, ADA_ROWS16, ADA_TILE, ADA_ROWS16, ADA_ROWS16, ADA_PER_STEP, ADA_TILE], got
    assert not any(r[3] for r in got), got         # solver_step: none of these is a general table's plan


# ---- what the GPU tests say they run ----
def engine_caps(engine, xsplit, attn_splits=128):
    """what vv_create's context offers the LM pass of an engine (LM_CASES key or LMCfg, max_rows): the arguments of lm()"""
    from test_gpu_kernels import LM_CASES
    c, R = engine
    c = LM_CASES[c] if isinstance(c, str) else c
    A = c.heads * c.head_dim
    return dict(ws=min(R, 64), splits=attn_splits, hkv=c.kv_heads, attn2=xsplit == 1,
                tile3=xsplit == 1 and R >= 64 and c.hidden % 8 == 0 and A % 8 == 0 and c.inter % 8 == 0,
                p16=xsplit == 1 and R > 4 and c.hidden % 32 == 0 and A % 32 == 0 and c.inter % 32 == 0)


def span_claim(n, xs, ws=64):
    """what the docstrings say n consecutive rows of one cache run"""
    if n == 1:
        return dict(route=GEMV, attn=FUSED)
    if n < 8 or xs != 1:
        return dict(route=GEMV, attn=SPLIT_MERGE, attn_groups=-(-n // ws), zero_v_tail=0)
    if n < 64:
        return dict(route=GEMV, attn=PREFILL4, zero_v_tail=1)
    return dict(route=PREFILL, attn=PREFILL4, zero_v_tail=1)


def test_the_gpu_tests_run_the_launches_they_name(probe):
    for xs in (1, 3):                               # test_suffix_over_a_restored_prefix_equals_the_chunked_pass
        caps = engine_caps(ls.SUFFIX_ENGINE, xs)
        assert caps["tile3"] == caps["p16"] == (xs == 1)
        spans = [s for n, m in ls.SUFFIX_SPANS for s in ((0, n), (n, m))]
        check_lm(probe, [(lm(ls.span(0, p0, k), **caps), span_claim(k, xs)) for p0, k in spans])
    ms = [m for _, m in ls.SUFFIX_SPANS]
    assert 1 in ms and any(2 <= m < 8 for m in ms) and any(8 <= m < 64 for m in ms) and any(m >= 64 for m in ms)

    for xs in (1, 3):                               # test_short_prompt_spans_ignore_cache_slots_past_their_end
        caps = engine_caps(ls.SHORT_SPANS_ENGINE, xs)
        check_lm(probe, [(lm(ls.span(0, 0, k), **caps), span_claim(k, xs)) for k in ls.SHORT_SPANS] +
                        [(lm(ls.span(0, p0, k), **caps), span_claim(k, xs)) for p0, k in ls.SHORT_SPANS_CHUNKED])
    assert any(2 <= k < 8 for k in ls.SHORT_SPANS) and {8, 63} <= set(ls.SHORT_SPANS) and all(k < 64 for k in ls.SHORT_SPANS)
    assert [k >= 64 for _, k in ls.SHORT_SPANS_CHUNKED] == [True, False]

    caps = engine_caps(ls.RAGGED_ENGINE, 3)         # test_lm_prefill_one_pass_and_ragged_chunks_match_the_oracle
    n = min(ls.RAGGED_PROMPT, ls.RAGGED_ENGINE[1])
    assert ls.RAGGED_CHUNK < 8
    check_lm(probe, [(lm(ls.span(0, 0, n), **caps), dict(contiguous=1, route=GEMV, attn=SPLIT_MERGE, attn_groups=3))] +
                    [(lm(ls.span(1, i0, min(ls.RAGGED_CHUNK, n - i0)), **caps), dict(contiguous=0, route=GEMV, attn=SPLIT_MERGE, attn_groups=1))
                     for i0 in range(0, n, ls.RAGGED_CHUNK)])

    for xs in (1, 3):                               # test_decode_batches_ignore_cache_slots_past_each_row
        caps = engine_caps(ls.DECODE_ENGINE, xs)
        for case, lens in ls.DECODE_LENS.items():
            want = dict(fused=1, attn=FUSED, route=P16 if xs == 1 and case in ("6", "16") else GEMV, attn_S=2 if case == "long" else 1)
            check_lm(probe, [(lm([(c, n + step) for c, n in enumerate(lens)], **caps), want) for step in range(ls.DECODE_STEPS)])
    assert (len(ls.DECODE_LENS["6"]), len(ls.DECODE_LENS["16"]), ls.DECODE_LENS["long"]) == (6, 16, [1100])

    for xs in (1, 3):                               # test_gpu_graph_replay.py::test_lm_replays_follow_the_row_table
        caps = engine_caps(ls.REPLAY_ENGINE, xs)
        assert set(ls.REPLAY_ROWS) == set(ls.REPLAY_SPLITS) == {"one", "short+long", "block-edge", "6", "16"}
        for case, steps in ls.REPLAY_ROWS.items():
            splits = ls.REPLAY_SPLITS[case]
            assert len(splits) == len(steps)
            packed = xs == 1 and case in ("6", "16")
            check_lm(probe, [(lm(rows, **caps), dict(fused=1, attn=FUSED, key_mode=1, route=P16 if packed else GEMV, attn_S=S, key_split=S))
                             for rows, S in zip(steps, splits)])
        # the claims of the docstring: the boundary sits between positions 1023 and 1024, both split counts come back often enough
        # to be replayed (three sights), and the one-row case ends on the one-split key it began with
        one = [(rows[0], S) for rows, S in zip(ls.REPLAY_ROWS["one"], ls.REPLAY_SPLITS["one"])]
        assert ((0, 1023), 1) in one and ((0, 1024), 2) in one and one[-3:] == [((1, 0), 1), ((1, 1), 1), ((1, 2), 1)]
        for case in ("one", "short+long"):
            assert ls.REPLAY_SPLITS[case].count(1) >= 3 and ls.REPLAY_SPLITS[case].count(2) >= 3
        assert [rows[1] for rows in ls.REPLAY_ROWS["short+long"][:4]] == [(1, 5), (1, 6), (1, 7), (1, 8)]
        assert ls.REPLAY_SPLITS["short+long"][:4] == [1, 1, 1, 2]
        edge = ls.REPLAY_ROWS["block-edge"]
        assert edge[0] == [(0, 30), (1, 62)] and edge[-1] == [(0, 34), (1, 66)]
        assert [len(ls.REPLAY_ROWS[c][0]) for c in ("6", "16")] == [6, 16]
        # test_replays_after_an_upload: the 3-row span of one cache is the rope/append + split + merge route in both modes
        check_lm(probe, [(lm(ls.span(2, p0, ls.REPLAY_SPAN), **caps), dict(fused=0, contiguous=0, route=GEMV, attn=SPLIT_MERGE, key_mode=0, key_split=1))
                         for p0 in range(0, 6 * ls.REPLAY_SPAN, ls.REPLAY_SPAN)])

    for xs in (1, 2, 3):                            # test_prefill_attention_over_4k_positions
        caps = engine_caps(ls.PREFILL_4K_ENGINE, xs)
        chunks = [(i0, min(ls.PREFILL_4K_CHUNK, ls.PREFILL_4K_PROMPT - i0)) for i0 in range(0, ls.PREFILL_4K_PROMPT, ls.PREFILL_4K_CHUNK)]
        assert caps["ws"] == 64 and chunks[0][1] == 512 and chunks[-1][0] >= 4096
        check_lm(probe, [(lm(ls.span(0, i0, k), **caps), span_claim(k, xs)) for i0, k in chunks])
        if xs != 1:                                 # "eight 64-row launches" per whole chunk
            whole = lm_plans(probe, [lm(ls.span(0, i0, k), **caps) for i0, k in chunks if k == 512])
            assert all(p["attn_groups"] == 8 for _, p in whole), whole


def test_the_attention_path_tests_run_the_launches_they_name(probe):
    """test_gpu_attn_paths.py: the kernel family, the split count and the projection route of every row set of lm_shapes.ATTN_*"""
    for geo, cfg in ls.ATTN_GEO.items():
        eng = (cfg, ls.ATTN_MAX_ROWS)
        for xs in (1, 2, 3):
            caps = engine_caps(eng, xs)
            assert caps["ws"] == 64 and caps["hkv"] == cfg.kv_heads and caps["tile3"] == caps["p16"] == caps["attn2"] == (xs == 1)
            # test_fused_decode: fused attention, the split count of every step, the packed batch route for 5..16 rows in the bf16 mode
            assert set(ls.ATTN_DECODE_LENS) == set(ls.ATTN_DECODE_SPLITS)
            for case, lens in ls.ATTN_DECODE_LENS.items():
                steps = ls.decode_steps(list(enumerate(lens)), ls.ATTN_DECODE_STEPS)
                route = P16 if xs == 1 and 5 <= len(lens) <= 16 else GEMV
                check_lm(probe, [(lm(rows, **caps), dict(fused=1, attn=FUSED, route=route, attn_S=S))
                                 for rows, S in zip(steps, ls.ATTN_DECODE_SPLITS[case])])
            capped = engine_caps(eng, xs, attn_splits=2)
            check_lm(probe, [(lm(rows, **capped), dict(fused=1, attn=FUSED, route=GEMV, attn_S=2))
                             for rows in ls.decode_steps(list(enumerate(ls.ATTN_DECODE_CAPPED)), ls.ATTN_DECODE_STEPS)])
            check_lm(probe, [(lm(ls.decode_steps(list(enumerate(ls.ATTN_DECODE_CAPPED)), 1)[0], **caps), dict(attn_S=3))])
            # test_split_merge: rope/append + the split + merge pair in every mode
            ragged = dict(fused=0, contiguous=0, route=GEMV, attn=SPLIT_MERGE, attn_groups=1, zero_v_tail=0)
            check_lm(probe, [(lm(ls.span(0, p0, n), **caps), dict(ragged, attn_S=(p0 + n - 1) // 1024 + 1)) for n, p0 in ls.ATTN_SPANS])
            check_lm(probe, [(lm(ls.ATTN_SHORT_LONG, **caps), dict(ragged, attn_S=2))])
            n, p0 = ls.ATTN_EXACT_CHUNK
            if xs != 1:
                check_lm(probe, [(lm(ls.span(0, p0, n), **caps), dict(contiguous=1, route=GEMV, attn=SPLIT_MERGE, attn_groups=2, attn_S=2))])
            # test_prefill4 and the chunks of test_append_exact
            chunks = list(ls.ATTN_CHUNKS) + [(n, p0) for n in ls.ATTN_APPEND_CHUNKS for p0 in ls.ATTN_APPEND_POS0]
            check_lm(probe, [(lm(ls.span(0, p0, n), **caps), span_claim(n, xs)) for n, p0 in chunks])
            # test_append_exact: one decode step of six rows, the 5-row spans
            check_lm(probe, [(lm(list(enumerate(ls.ATTN_APPEND_DECODE)), **caps), dict(fused=1, attn=FUSED, route=P16 if xs == 1 else GEMV))] +
                            [(lm([(0, p)], **caps), dict(fused=1, attn=FUSED, route=GEMV)) for p in ls.ATTN_APPEND_DECODE] +
                            [(lm(ls.span(0, p0, ls.ATTN_APPEND_SPAN), **caps), ragged) for p0 in ls.ATTN_APPEND_POS0])
    # what the docstrings of the GPU file say about the row sets
    lens = sorted({n for v in ls.ATTN_DECODE_LENS.values() for n in v})
    assert set(lens) >= {0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, 129, 1022, 1023, 1024, 2047, 2048, 2100}
    assert [len(ls.ATTN_DECODE_LENS[c]) for c in ("1", "2", "6", "16")] == [1, 2, 6, 16]
    assert set(ls.ATTN_DECODE_LENS["mix"][1:]) == {1, 32, 33, 40, 96, 97} and ls.ATTN_DECODE_LENS["mix"][0] == 2100
    # the owner split (pos >> 5) % S takes every residue for S = 2 and S = 3
    owners = {2: set(), 3: set()}
    for case, lens in ls.ATTN_DECODE_LENS.items():
        for step, S in enumerate(ls.ATTN_DECODE_SPLITS[case]):
            if S in owners:
                owners[S] |= {((n + step) >> 5) % S for n in lens}
    assert owners == {2: {0, 1}, 3: {0, 1, 2}}, owners
    assert any(n < 64 for n, _ in ls.ATTN_CHUNKS) and any(n >= 64 for n, _ in ls.ATTN_CHUNKS)


def merge2_walk(used, D):
    """vv_attn_merge2_kernel over `used` partials: per outer iteration (live groups, groups with a dead slot, live slots of group 0)"""
    NG = 512 // D
    out = []
    for it in range(-(-used // (8 * NG))):
        live = [sum(1 for u in range(8) if it * 8 * NG + g + u * NG < used) for g in range(NG)]
        out.append((sum(1 for n in live if n), sum(1 for n in live if 0 < n < 8), live[0]))
    return out


def test_the_long_attention_tests_run_the_launches_they_name(probe):
    """test_gpu_attn_long.py: route and split count of every row set of lm_shapes.ATTN_LONG_*, QKV_ROPE_* and FAR_*, and the state of
    vv_attn_merge2's outer loop those split counts reach"""
    ragged = dict(fused=0, contiguous=0, route=GEMV, attn=SPLIT_MERGE, attn_groups=1, zero_v_tail=0)
    for geo, cfg in ls.ATTN_GEO.items():
        eng = (cfg, ls.ATTN_LONG_MAX_ROWS)
        for xs in (1, 2, 3):
            caps = engine_caps(eng, xs)
            assert caps["ws"] == 64 and caps["tile3"] == caps["p16"] == caps["attn2"] == (xs == 1)
            assert set(ls.ATTN_LONG_DECODE_LENS) == set(ls.ATTN_LONG_DECODE_SPLITS)
            for case, lens in ls.ATTN_LONG_DECODE_LENS.items():
                assert len(lens) <= 2 * ls.ATTN_LONG_SLOTS and max(lens) + 2 <= ls.ATTN_LONG_MAX_CTX
                route = P16 if xs == 1 and 5 <= len(lens) <= 16 else GEMV
                S = ls.ATTN_LONG_DECODE_SPLITS[case][geo]
                check_lm(probe, [(lm(rows, **caps), dict(fused=1, attn=FUSED, route=route, attn_S=S, key_split=S))
                                 for rows in ls.decode_steps(list(enumerate(lens)), 1 if case == "L16" else 2)])     # "own": two steps; L16 has no own
            capped = engine_caps(eng, xs, attn_splits=ls.ATTN_LONG_CAP)
            cap_rows = ls.decode_steps(list(enumerate(ls.ATTN_LONG_DECODE_CAPPED)), 2)
            check_lm(probe, [(lm(rows, **capped), dict(fused=1, attn=FUSED, route=GEMV, attn_S=ls.ATTN_LONG_CAP)) for rows in cap_rows])
            check_lm(probe, [(lm(cap_rows[0], **caps), dict(attn_S=64))])
            check_lm(probe, [(lm(ls.span(0, p0, n), **caps), dict(ragged, attn_S=ls.ATTN_LONG_SPAN_SPLITS[(n, p0)][geo]))
                             for n, p0 in ls.ATTN_LONG_SPANS])
            check_lm(probe, [(lm(list(ls.ATTN_LONG_SHORT_LONG), **caps), dict(ragged, attn_S=ls.ATTN_LONG_SHORT_LONG_SPLITS[geo]))])
            n, p0 = ls.ATTN_LONG_EXACT_CHUNK
            if xs != 1:
                check_lm(probe, [(lm(ls.span(0, p0, n), **caps), dict(contiguous=1, route=GEMV, attn=SPLIT_MERGE, attn_groups=2,
                                                                      attn_S=ls.ATTN_LONG_EXACT_CHUNK_SPLITS[geo]))])
            chunks = list(ls.ATTN_LONG_CHUNKS) + [(n, ls.ATTN_LONG_APPEND_CHUNK_POS) for n in ls.ATTN_LONG_APPEND_CHUNKS]
            check_lm(probe, [(lm(ls.span(0, p0, n), **caps), span_claim(n, xs)) for n, p0 in chunks])
            assert all(p0 + n <= ls.ATTN_LONG_MAX_CTX for n, p0 in chunks + list(ls.ATTN_LONG_SPANS) + [ls.ATTN_LONG_EXACT_CHUNK])
            check_lm(probe, [(lm(list(enumerate(ls.ATTN_LONG_APPEND_DECODE)), **caps), dict(fused=1, attn=FUSED, route=P16 if xs == 1 else GEMV))] +
                            [(lm([(0, p)], **caps), dict(fused=1, attn=FUSED, route=GEMV)) for p in ls.ATTN_LONG_APPEND_DECODE] +
                            [(lm(ls.span(0, p0, ls.ATTN_APPEND_SPAN), **caps), ragged) for p0 in ls.ATTN_LONG_APPEND_SPANS])
    assert max(ls.ATTN_LONG_APPEND_DECODE) == ls.ATTN_LONG_MAX_CTX - 1
    # what the comments of lm_shapes.py say the split counts do to vv_attn_merge2 (a row of `used` = S partials)
    S = ls.ATTN_LONG_DECODE_SPLITS
    assert merge2_walk(S["L1"]["A"], 64) == [(8, 0, 8)]                             # one full iteration, all eight slots of every group
    assert merge2_walk(S["L1"]["B"], 128) == [(4, 0, 8), (4, 0, 8)]                 # two outer iterations
    assert merge2_walk(S["L1x"]["A"], 64) == [(8, 0, 8), (3, 3, 1)]                 # a second one: three live groups, dead slots
    assert len(merge2_walk(S["L1x"]["B"], 128)) == 3 and merge2_walk(S["L1x"]["B"], 128)[2] == (3, 3, 1)
    assert merge2_walk(S["L16"]["A"], 64) == [(8, 8, 2)] and merge2_walk(S["L16"]["B"], 128) == [(4, 3, 8)]
    assert (S["L6"]["A"], S["L6"]["B"]) == (32, 64)
    blocks = [(n + 32) // 32 for n in ls.ATTN_LONG_DECODE_LENS["L6"]]               # 32-position blocks of each row with its new token
    for g in ("A", "B"):
        assert any(b >= S["L6"][g] for b in blocks) and any(1 < b < S["L6"][g] for b in blocks) and 5 in blocks
    assert [(n + 32) // 32 for n in ls.ATTN_LONG_DECODE_LENS["L2"]] == [2032, 1]
    # test_qkv_rope_epilogue_append: a contiguous chunk on the packed prefill; test_far_cache_offsets: layer 15 of a 16-layer engine
    caps = engine_caps((ls.QKV_ROPE_CFG, ls.QKV_ROPE_ROWS), 1)
    assert caps["tile3"]
    check_lm(probe, [(lm(ls.span(0, ls.QKV_ROPE_POS0, ls.QKV_ROPE_ROWS), **caps), dict(contiguous=1, route=PREFILL, attn=PREFILL4, zero_v_tail=1))])
    assert ls.QKV_ROPE_POS0 + ls.QKV_ROPE_ROWS <= ls.QKV_ROPE_MAX_CTX
    c = ls.FAR_CFG
    stride = c.layers * c.kv_heads * ls.FAR_MAX_CTX * c.head_dim
    assert stride == 2 ** 27 and 16 * stride == 2 ** 31 and 2 * ls.FAR_SLOTS == 18
    for xs in (1, 2, 3):
        caps = engine_caps((c, ls.FAR_MAX_ROWS), xs)
        check_lm(probe, [(lm(list(ls.FAR_DECODE), **caps), dict(fused=1, attn=FUSED, route=GEMV, attn_S=64))] +
                        [(lm(ls.span(cc, p0, 5), **caps), ragged) for cc, p0 in ls.FAR_SPANS])
        if xs == 1:
            cc, p0, n = ls.FAR_CHUNK
            check_lm(probe, [(lm(ls.span(cc, p0, n), **caps), span_claim(n, 1))])
    assert {cc for cc, _ in ls.FAR_DECODE} == {cc for cc, _ in ls.FAR_SPANS} == {0, 16, 17} and ls.FAR_CHUNK[0] >= 16
