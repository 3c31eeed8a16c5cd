"""The row sets behind the route claims of the LM pass's GPU tests, and the engine settings that decide what their context offers, as
plain data: the GPU tests take their shapes from here, and test_pass_plan_cpu.py asks the routing (csrc/pass_plan.h), on a machine
without a GPU, whether every row set runs the launches its test's docstring says it does.  Engines: (key of LM_CASES in
test_gpu_kernels.py or an LMCfg, max_rows); the tests build them at the xsplit values of their parametrisation."""
import synth


def span(cache, pos0, n):
    """n consecutive positions of one cache, as Engine.lm_forward_span issues them"""
    return [(cache, pos0 + j) for j in range(n)]


# test_gpu_prompt_prefix.py::test_suffix_over_a_restored_prefix_equals_the_chunked_pass: (prefix rows n, suffix rows m); the suffix
# starts at position n.  A 1-row suffix is a decode row (fused attention), 2..7 rows split + merge, 8..63 vv_attn_prefill4 in the
# bf16 mode, >= 64 the packed prefill
SUFFIX_SPANS = ((8, 1), (37, 5), (37, 20), (100, 64), (100, 150), (128, 20), (64, 7))
SUFFIX_ENGINE = ("gqa", 256)

# test_gpu_kernels.py::test_short_prompt_spans_ignore_cache_slots_past_their_end: spans at position 0, then a chunked prompt (pos0, rows)
SHORT_SPANS = (2, 5, 7, 8, 20, 48, 63)
SHORT_SPANS_CHUNKED = ((0, 128), (128, 20))
SHORT_SPANS_ENGINE = ("gqa", 256)

# test_gpu_kernels.py::test_lm_prefill_one_pass_and_ragged_chunks_match_the_oracle: the prompt in one pass, then in ragged chunks
# (below the 8 rows of a contiguous chunk: rope/append + split + merge, one launch of the pair per layer); exact mode
RAGGED_PROMPT, RAGGED_CHUNK = 150, 7
RAGGED_ENGINE = (synth.LMCfg(), 160)

# test_gpu_kernels.py::test_decode_batches_ignore_cache_slots_past_each_row: cache lengths of the rows of one launch (row i on cache i),
# DECODE_STEPS steps each.  6 and 16 rows: the batch-decode route in the bf16 mode; 1100: two splits, the merge kernel runs
DECODE_LENS = {"1": [37], "6": [1, 31, 32, 33, 64, 90], "16": [1, 2, 7, 16, 31, 32, 33, 40, 63, 64, 65, 70, 95, 96, 97, 127],
               "long": [1100]}
DECODE_STEPS = 3
DECODE_ENGINE = ("gqa", 16)

# test_gpu_geometry.py::test_prefill_attention_over_4k_positions: the prompt in chunks of max_rows rows; bf16 mode: the packed prefill;
# exact modes: per whole chunk, eight 64-row launches of the split + merge pair
PREFILL_4K_PROMPT, PREFILL_4K_CHUNK = 4200, 512
PREFILL_4K_ENGINE = (synth.LMCfg(hidden=512, layers=1, heads=4, kv_heads=2, inter=512, vocab=64, max_pos=8192), 512)


def decode_steps(starts, n):
    """n decode steps of the rows starting at (cache, position) `starts`: one row set per step"""
    return [[(c, p + s) for c, p in starts] for s in range(n)]


# test_gpu_graph_replay.py::test_lm_replays_follow_the_row_table: decode row sets a use_graph engine replays with ONE x / hidden
# buffer per row count, so the row table (device memory) and the split count (a key field) are all that tells two steps apart.
# Per case: the row set of every step, and the split count each step's key carries (key_split; the merge kernel joins the launches at 2).
#   one         cache 0 over the 1024-position boundary, then cache 1 from position 0: back to the one-split graph
#   short+long  a row at 5 beside a row crossing 1024: the short row rides in a two-split launch, the merge kernel skips it (the first
#               four steps reach the boundary; three more let the two-split key come back and be replayed)
#   block-edge  two rows crossing position 32 / 64: the 32-position block edge of the V layout and of the owner split
#   6, 16       DECODE_LENS as starting lengths: the packed batch route in the bf16 mode
REPLAY_ROWS = {"one": decode_steps([(0, 1021)], 7) + decode_steps([(1, 0)], 3),
               "short+long": decode_steps([(0, 1021), (1, 5)], 7),
               "block-edge": decode_steps([(0, 30), (1, 62)], 5),
               "6": decode_steps(list(enumerate(DECODE_LENS["6"])), 4),
               "16": decode_steps(list(enumerate(DECODE_LENS["16"])), 4)}
REPLAY_SPLITS = {"one": [1, 1, 1, 2, 2, 2, 2, 1, 1, 1], "short+long": [1, 1, 1, 2, 2, 2, 2], "block-edge": [1] * 5, "6": [1] * 4, "16": [1] * 4}
REPLAY_ENGINE = ("gqa", 16)
# test_gpu_graph_replay.py::test_replays_after_an_upload: a 3-row span of one cache (rope/append reads inv_freq itself, then split + merge)
REPLAY_SPAN = 3

# ---- test_gpu_attn_paths.py: one attention launch at a time through the readout layer (tests/attn_cases.py) ----
# geometries: A head_dim 64, 4 query / 2 kv heads; B head_dim 128, 7 query heads on 1 kv head (the 7B group: a vv_attn_prefill4
# workgroup of four units straddles two 64-row tiles).  heads * head_dim == hidden: the identity o-projection reads attention out
ATTN_GEO = {"A": synth.LMCfg(hidden=256, layers=1, heads=4, kv_heads=2, inter=256, vocab=64),
            "B": synth.LMCfg(hidden=896, layers=1, heads=7, kv_heads=1, inter=256, vocab=64)}
ATTN_MAX_CTX, ATTN_SLOTS, ATTN_MAX_ROWS = 2304, 8, 160
# test_fused_decode: cache lengths before the first step (row i on cache i), ATTN_DECODE_STEPS steps each.  Between them the sets hold
# every length of 0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, 129, 1022, 1023, 1024, 2047, 2048, 2100; "6", "16" and "mix" take the
# batch-decode route in the bf16 mode; "mix": rows of one block (used = 1) and of two (used < S) beside a row of three splits
ATTN_DECODE_LENS = {"1": [1023], "2": [1055, 31], "6": [2048, 2100, 2030, 33, 1022, 129],
                    "16": [0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, 129, 1022, 1023, 1024, 2047],
                    "mix": [2100, 1, 32, 33, 40, 96, 97]}
ATTN_DECODE_STEPS = 3
# the split count of every step of a case (one per 1024 positions of the longest row), and with attn_splits = 2 capping it
ATTN_DECODE_SPLITS = {"1": [1, 2, 2], "2": [2, 2, 2], "6": [3, 3, 3], "16": [2, 3, 3], "mix": [3, 3, 3]}
ATTN_DECODE_CAPPED = [2100, 40]
# test_split_merge: (rows, pos0) spans of one cache; a 5-row span at 6 beside a row at 1500 of another cache (a short row in a
# two-split launch whose positions per split sit at the 512 floor); exact modes: a 70-row chunk (two launches of the pair)
ATTN_SPANS = tuple((n, p0) for n in (2, 5, 7) for p0 in (0, 30, 510, 1020, 2046))
ATTN_SHORT_LONG = span(0, 6, 5) + [(1, 1500)]
ATTN_EXACT_CHUNK = (70, 1000)
# test_prefill4 (bf16 mode): (rows, pos0) chunks; below 64 rows through the per-layer GEMMs, from 64 the packed prefill
ATTN_CHUNKS = tuple((n, p0) for n in (8, 20, 63, 64, 100, 150) for p0 in (0, 37, 64, 100, 1000))
# test_append_exact: one decode step per position class, a 5-row span and two chunks at each pos0
ATTN_APPEND_DECODE = [0, 15, 16, 31, 32, 2040]
ATTN_APPEND_POS0 = (0, 37, 2040)
ATTN_APPEND_SPAN, ATTN_APPEND_CHUNKS = 5, (64, 150)
