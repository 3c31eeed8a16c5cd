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

# ---- test_gpu_attn_long.py: the same launches at the contexts the product decodes at (32K: 32 splits, 64K: 64) ----
# The split counts are vv_lm_pass_plan's: one per 1024 positions of the longest row, at most 256 / (long rows x kv heads), rows past
# 1024 positions counting as long; geometry A has 2 kv heads, B has 1.  vv_attn_merge2 reads eight partials per thread group at
# once, slots b0 + u NG with NG = 512 / head_dim groups (A: 8, B: 4): 8 NG splits per outer iteration.
ATTN_LONG_MAX_CTX, ATTN_LONG_SLOTS, ATTN_LONG_MAX_ROWS = 69632, 8, 160          # 68 x 1024 positions
# test_fused_decode_long: cache lengths before the step (row i on cache i); per set the split count in A and in B
#   L1    64 splits: B two outer iterations of merge2, A one full iteration with all eight slots of every group live
#   L1x   67 splits: A a second iteration with three live groups and dead slots, B three iterations
#   L2    a 64-split row beside a one-block row the attention kernel finishes itself
#   L6    four rows past 1024 positions: rows with used == S, used < S (1022: 32 blocks, B) and used = 5 (129) in one launch; the
#         packed batch route and out_packed in the bf16 mode
#   L16   eight long rows from 2000 to 64,000 and eight short ones; 1024 is past 1024 positions once its token is appended, so nine
#         rows count as long: ceil(256 / 18) = 15 and ceil(256 / 9) = 29 splits -- odd counts, dead slots in every group but one
#   Lcap  attn_splits = 8 capping a 65,000-position row: 8 splits of about 8125 positions
ATTN_LONG_DECODE_LENS = {"L1": (64999,), "L1x": (67900,), "L2": (65000, 31), "L6": (64990, 40000, 33000, 5000, 1022, 129),
                         "L16": (2000, 9000, 17000, 25000, 33000, 41000, 52000, 64000, 0, 1, 31, 32, 63, 64, 1023, 1024)}
ATTN_LONG_DECODE_SPLITS = {"L1": {"A": 64, "B": 64}, "L1x": {"A": 67, "B": 67}, "L2": {"A": 64, "B": 64}, "L6": {"A": 32, "B": 64},
                           "L16": {"A": 15, "B": 29}}
ATTN_LONG_DECODE_CAPPED, ATTN_LONG_CAP = (65000, 40), 8
# test_split_merge_long: (rows, pos0) spans of one cache -- every row of a span is long, so the split count is ceil(256 / (rows x kv
# heads)) unless one per 1024 positions is fewer --, a 5-row span at 6 beside a row at 65,000 of another cache (one-split rows in a
# 64-split launch), and in the exact modes a 70-row chunk at 60,000 (two launches of the pair, 30,080 and 15,104 positions per split)
ATTN_LONG_SPANS = ((5, 64990), (2, 32767), (7, 65530))
ATTN_LONG_SPAN_SPLITS = {(5, 64990): {"A": 26, "B": 52}, (2, 32767): {"A": 33, "B": 33}, (7, 65530): {"A": 19, "B": 37}}
ATTN_LONG_SHORT_LONG = tuple(span(0, 6, 5) + [(1, 65000)])
ATTN_LONG_SHORT_LONG_SPLITS = {"A": 64, "B": 64}
ATTN_LONG_EXACT_CHUNK = (70, 60000)
ATTN_LONG_EXACT_CHUNK_SPLITS = {"A": 2, "B": 4}
# test_prefill4_long (bf16 mode): (rows, pos0) chunks, about 500 to 1000 stages of 64 positions before the chunk
ATTN_LONG_CHUNKS = ((8, 32760), (20, 65000), (64, 64960), (150, 60001))
# test_append_exact_long: decode steps (all six in one launch, then each alone), 5-row spans, chunks of 64 and 150 rows
ATTN_LONG_APPEND_DECODE = (4095, 4096, 32767, 32768, 65535, 69631)
ATTN_LONG_APPEND_SPANS = (32766, 65534)
ATTN_LONG_APPEND_CHUNKS, ATTN_LONG_APPEND_CHUNK_POS = (64, 150), 65000
# test_qkv_rope_epilogue_append: a thin 7B-shaped layer (hidden 64, 28 query / 4 kv heads of 128) whose 3600-row chunk at 61,000 puts
# 18 x 15 = 270 workgroups of 256 x 256 on the 4608-wide QKV GEMM: vv_qkv_rope_plan takes it (test_prefill_plan_cpu.py)
QKV_ROPE_CFG = synth.LMCfg(hidden=64, layers=1, heads=28, kv_heads=4, inter=256, vocab=64, head_dim_override=128)
QKV_ROPE_ROWS, QKV_ROPE_POS0, QKV_ROPE_MAX_CTX = 3600, 61000, 65536
# test_far_cache_offsets: geometry A sixteen layers deep, 65,536 positions, 9 slots: 2^27 elements per cache, caches 16 and 17 start
# at element 2^31 and 2^31 + 2^27 of the K and V arrays (18 x 2^27 x 2 bytes = 4.83 GB each)
FAR_CFG = synth.LMCfg(hidden=256, layers=16, heads=4, kv_heads=2, inter=256, vocab=64)
FAR_MAX_CTX, FAR_SLOTS, FAR_LAYER, FAR_MAX_ROWS = 65536, 9, 15, 64
FAR_DECODE = ((0, 65000), (16, 40), (17, 3000))
FAR_SPANS = ((0, 64990), (16, 37), (17, 3000))          # (cache, pos0) of a 5-row span each
FAR_CHUNK = (17, 30000, 64)                             # (cache, pos0, rows), bf16 mode
