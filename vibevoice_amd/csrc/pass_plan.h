// pass_plan.h -- which sequence of launches a row set gets, one level above the GEMM plans (gemv_plan.h, prefill_plan.h): the route of
// one LM pass (engine_lm.hip) and of the diffusion head's sampler (engine_head.hip), decided on the host before anything is launched.
// Plain host C++: no kernel, no HIP call, no device pointer is dereferenced (a test drives it on a machine without a GPU).
#pragma once
#include "vv_common.h"

// batch decode (5..16 rows, bf16 mode): activations as one 16-row packed fragment tile (gemv16p.hip).  One window for the LM's
// projections and the head's layers
constexpr int VV_P16_MIN_ROWS = 5, VV_P16_MAX_ROWS = 16;
inline bool vv_p16_rows(int rows) { return rows >= VV_P16_MIN_ROWS && rows <= VV_P16_MAX_ROWS; }

// ---- the LM pass ----
// decode attention geometry: one split (workgroup column) per 1024 positions of the longest row, at most attn_splits.  A grid
// choice, so it is part of the graph key: a growing context re-captures the step graph when the split count changes.
constexpr int VV_ATTN_SPLIT_POS = 1024;
// ... and no more splits than it takes to put ~256 workgroups on the chip: with eight 32K-context utterances in flight the
// rows themselves are the parallelism (8 splits of 4096 positions: 122 us per layer against 162 us with 32 splits).
// Measured and left alone: 512 / 256 positions per split (no gain once the merge is its own launch), 8-wave workgroups (three
// times, slower than 4 waves: round 4, 8.90 vs 8.28 us per unit at 400 positions, 1.5B; 5.84 vs 5.78 at 250, 0.5B).
constexpr int VV_ATTN_TARGET_WGS = 256;        // workgroups a launch of long rows aims for
constexpr int VV_CHUNK_MIN_ROWS = 8;           // a contiguous chunk (one cache, consecutive positions) has at least this many rows
// prompt prefill, bf16-activation mode (a contiguous chunk of >= 64 rows): packed activations + LDS-staged MFMA GEMMs + 64-row prefill attention
constexpr int VV_PREFILL_MIN_ROWS = 64;

enum { VV_LM_PREFILL, VV_LM_P16, VV_LM_GEMV };                       // the layer path (lm_prefill_layers / lm_p16_layer / lm_gemv_layer)
enum { VV_ATTN_FUSED, VV_ATTN_PREFILL4, VV_ATTN_SPLIT_MERGE };       // the attention inside it

// what the context offers a pass
struct VVLmCaps { int ws_rows, attn_splits, Hkv; bool tile3_ok, attn2_ok, p16_ok; bool w13 = false; };      // w13: the layers' matrices have W13 twins (vv_w13.h)

struct VVLmPlan {
    bool fused;                 // every row a different cache: RoPE + append + attention in one launch
    bool contiguous;            // one cache, consecutive positions, >= VV_CHUNK_MIN_ROWS rows
    int route, attn;            // VV_LM_*, VV_ATTN_*
    int attn_S;                 // splits of the fused / split attention
    int attn_groups;            // VV_ATTN_SPLIT_MERGE: launches of the pair per layer, at most ws_rows rows each (else 0)
    bool zero_v_tail;           // the pass reaches vv_attn_prefill4: the V tail past the chunk is zeroed once for every layer
    int key_mode, key_split;    // the graph key's last two fields
    int64_t kv_positions;       // cached positions the rows attend, summed (the profile window's byte count)
    bool w13 = false;           // one utterance (<= 2 rows) on the GEMV route: a layer's projections stream their W13 twins where a form exists
};

// rows: n_rows validated (cache, pos) pairs.  0: *p is the pass;  -1: a ragged launch of more than ws_rows rows (fused and
// contiguous are set, nothing else)
inline int vv_lm_pass_plan(const VVRow* rows, int n_rows, const VVLmCaps& c, VVLmPlan* p) {
    bool fused = true;
    for (int i = 0; i < n_rows && fused; ++i)
        for (int j = 0; j < i; ++j) if (rows[i].cache == rows[j].cache) { fused = false; break; }
    bool contiguous = !fused && n_rows >= VV_CHUNK_MIN_ROWS;      // one cache, consecutive positions
    for (int i = 1; i < n_rows && contiguous; ++i)
        if (rows[i].cache != rows[0].cache || rows[i].pos != rows[0].pos + i) contiguous = false;
    p->fused = fused; p->contiguous = contiguous;
    if (!contiguous && n_rows > c.ws_rows) return -1;
    int max_len = 1, n_long = 0;
    int64_t kv_positions = 0;
    for (int i = 0; i < n_rows; ++i) {
        const int len = rows[i].pos + 1;
        if (len > max_len) max_len = len;
        if (len > VV_ATTN_SPLIT_POS) ++n_long;
        kv_positions += len;
    }
    const int long_wgs = (n_long > 1 ? n_long : 1) * c.Hkv;
    int S = (VV_ATTN_TARGET_WGS + long_wgs - 1) / long_wgs;
    if (S < 1) S = 1;
    if (S > c.attn_splits) S = c.attn_splits;
    const int by_len = (max_len + VV_ATTN_SPLIT_POS - 1) / VV_ATTN_SPLIT_POS;       // >= 1
    if (S > by_len) S = by_len;
    p->attn_S = S;
    p->kv_positions = kv_positions;
    // short prompt chunks reach vv_attn_prefill4 as well: the same V tail past the chunk
    const bool chunk_attn = contiguous && c.attn2_ok;
    if (contiguous && c.tile3_ok && n_rows >= VV_PREFILL_MIN_ROWS) { p->route = VV_LM_PREFILL; p->attn = VV_ATTN_PREFILL4; }
    else {
        // batch decode rows: packed-activation projections
        p->route = vv_p16_rows(n_rows) && c.p16_ok && fused ? VV_LM_P16 : VV_LM_GEMV;
        p->attn = fused ? VV_ATTN_FUSED : chunk_attn ? VV_ATTN_PREFILL4 : VV_ATTN_SPLIT_MERGE;
    }
    p->attn_groups = p->attn == VV_ATTN_SPLIT_MERGE ? (n_rows + c.ws_rows - 1) / c.ws_rows : 0;
    p->zero_v_tail = p->route == VV_LM_PREFILL || chunk_attn;
    p->key_mode = fused ? 1 : (contiguous ? 2 : 0);
    p->key_split = chunk_attn ? 0 : S;
    p->w13 = c.w13 && p->route == VV_LM_GEMV && n_rows <= 2;
    return 0;
}

// ---- the diffusion head ----
// bf16 mode, three or more 16-row passes: ONE MFMA tile GEMM over all (step, row) pairs instead -- the modulation
// matrix (360 MB for the 7B head) is streamed once, not once per 16 rows (8 utterances x 20 steps: 20 passes)
constexpr int VV_ADA_TILE_ABOVE_ROWS = 32;

enum { VV_ADA_PER_STEP, VV_ADA_TILE, VV_ADA_ROWS16 };     // adaLN modulations: inside every head evaluation / one tile GEMM / 16-row passes, both up front
enum { VV_HEAD_P16, VV_HEAD_GEMV };                       // the layers' projections
enum { VV_FINAL_P16_CFG,        // final layer over the packed operand the last down projection left, CFG + solver update in the epilogue
       VV_FINAL_SEAM,           // the fused seam (headtail.hip), when the launcher accepts its operands; else VV_FINAL_GEMM_CFG
       VV_FINAL_GEMM_CFG,       // the GEMM dispatcher's kernel with the CFG-DPM epilogue
       VV_FINAL_GEMM };         // ... with a plain store (no solver coefficients: vv_head_forward)

// what the context offers: the batch-decode buffers, the packed shift tiles, the packed adaLN operand, the batched modulations, the seam
// ... and W13 twins of the layers' matrices (vv_w13.h)
struct VVHeadCaps { bool p16_ok, p16_shift, ada_p, mod_all, head_tail, w13; };

struct VVHeadPlan {
    int rows, n_steps;
    int ada;                    // VV_ADA_*
    bool sh_tiles;              // the shift rows of every (solver step, layer) as packed bf16 tiles, one launch per frame
    int layers;                 // VV_HEAD_*
    bool seam;                  // decode rows, bf16 mode: every step but the last ends with the fused seam
    int final_stage;            // VV_FINAL_* of a step that does not
    bool solver_step;           // the general solver table: a step ends with solver.hip's launch behind the final layer's plain store
    bool w13;                   // one utterance on the GEMV route: a layer's projections stream their W13 twins
};

// has_coef: the call has solver coefficients (the samplers; vv_head_forward has none and evaluates the head once)
// solver_step: the general solver table (vv_diffusion_sample_general): the modulations stay batched and the layers are chosen as for
// has_coef, but every step ends with the final layer's plain store -- the update is solver.hip's launch, never an epilogue or the seam
inline VVHeadPlan vv_head_plan(int rows, int n_steps, int HF, int HL, int MODW, const VVHeadCaps& c, bool has_coef, bool solver_step = false) {
    VVHeadPlan p;
    p.rows = rows; p.n_steps = n_steps;
    const bool batch_ada = has_coef && c.mod_all;
    p.ada = !batch_ada ? VV_ADA_PER_STEP : (c.ada_p && rows * n_steps > VV_ADA_TILE_ABOVE_ROWS && (MODW & 3) == 0) ? VV_ADA_TILE : VV_ADA_ROWS16;
    p.sh_tiles = batch_ada && vv_p16_rows(rows) && c.p16_shift;
    // batch rows: normalise + modulate + pack ONCE, then both projections stream weights against packed fragments
    p.layers = vv_p16_rows(rows) && c.p16_ok && (HF % 32) == 0 ? VV_HEAD_P16 : VV_HEAD_GEMV;
    p.seam = has_coef && rows == 2 && c.head_tail;
    p.w13 = c.w13 && p.layers == VV_HEAD_GEMV && rows <= 2;
    p.final_stage = p.layers == VV_HEAD_P16 && p.sh_tiles && has_coef && HL > 0 ? VV_FINAL_P16_CFG : has_coef ? VV_FINAL_GEMM_CFG : VV_FINAL_GEMM;
    p.solver_step = solver_step;
    if (solver_step) { p.sh_tiles = false; p.seam = false; p.final_stage = VV_FINAL_GEMM; }      // the packed shift tiles serve VV_FINAL_P16_CFG alone
    return p;
}
inline int vv_head_final(const VVHeadPlan& p, int step) { return p.seam && step + 1 < p.n_steps ? VV_FINAL_SEAM : p.final_stage; }
