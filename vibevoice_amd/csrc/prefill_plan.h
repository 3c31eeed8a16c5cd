// prefill_plan.h -- what the prefill GEMM launchers of prefill.hip (vv_gemm3_launch, vv_gemm_qkv_rope_launch) run a call on: the kernel
// form, the compiled epilogue, the grid, and the two K-splits, decided on the host before anything is launched.
// Plain host C++: no kernel, no HIP call, no operand pointer is dereferenced (a test drives it on a machine without a GPU).
#pragma once
#include "vv_common.h"

// the three kernel forms: vv_gemm4_kernel (256 x 256 tiles) and vv_gemm3_kernel (128 x 128) with one or two stage buffers
enum { VV_PF_G4, VV_PF_G3, VV_PF_G3_DB, VV_PF_FORMS };

// What the caller's workspace (VVGemmWs) offers: round = partials, flags and err of the 256 x 256 kernel's partial round all exist;
// g3_bytes = the size of the short-prompt partial tensors (0: none).
struct VVPrefillWs { bool round; size_t g3_bytes; };
inline VVPrefillWs vv_prefill_ws(const VVGemmWs* ws) {
    return {ws && ws->partials && ws->flags && ws->err, ws && ws->g3_partials ? ws->g3_bytes : (size_t)0};
}

struct VVGemm3Plan {
    int form;                   // VV_PF_*
    int epi;                    // the compiled epilogue (VV_EPI_STORE runs the BIAS kernel: bias == null is a plain store)
    int n_blocks, t_blocks;     // feature blocks x row blocks of the form's tile
    dim3 grid;
    int block;                  // threads per workgroup
    size_t lds;                 // dynamic LDS bytes
    int full_idx, split;        // G4, the partial round: per XCD, tiles [0, full_idx) are computed whole, the rest in `split` k-parts (1: none)
    int ks;                     // G3, short prompts: K parts over grid.y; > 1: vv_g3_reduce_kernel follows
};

constexpr int VV_G4_BLOCK = 512, VV_G3_BLOCK = 256;
constexpr size_t VV_G4_LDS = 4 * 32 * 1024;      // 4-slot ring of 32-wide K stages
// long prompts: the 256 x 256 kernel whenever its grid fills the chip at least once; smaller problems keep the 128-feature
// kernel, whose tiles quantise better.  Per launch at T = 10,922 (7B layer), 128-feature kernel -> round-2 256 x 256 ->
// round-3 schedule + strip order + K-split: gate/up 3188 -> 2650 -> 2350 us, down 1751 -> 1470 -> 1390, qkv 518 -> 404 -> 315,
// o 432 -> 340 -> 271.
constexpr int VV_G4_MIN_WGS = 256;
// One workgroup per CU (128 KiB of LDS): the grid runs in rounds of 256 and the tiles past the last whole round (T =
// 10,922 at 7B widths: 602 tiles for down / o = 2.35 rounds, 774 for QKV = 3.02) cost most of a round however few they
// are.  Each XCD's share of that remainder (<= 32 tiles) is split along K by the largest factor that still fits one
// round (g4_map / g4_finish).  Measured (tools/experiments/gemm_pingpong): it pays when the remainder is a handful of
// tiles (QKV: split 7, -6 %) or the parts stay long (down: K = 18,944 halved, -3.5 %); halving K = 3584 tiles does not
// (o: +6 %; gate/up: neutral) -- a partial round is not a lost round on this chip: the package is at its power limit
// under these kernels and the clock rises when fewer CUs compute -- so those launches stay whole.
constexpr int VV_G4_ROUND = 256, VV_G4_XCD_ROUND = VV_G4_ROUND / 8;      // workgroups per round: on the chip, on one XCD
constexpr int VV_G4_MAX_SPLIT = 8;
constexpr int VV_G4_MIN_PART_STEPS = 8;          // a part keeps >= 8 of the 64-wide steps
constexpr int VV_G4_HALVES_MIN_STEPS = 256;      // halves of a K shorter than this many steps do not pay (above: o / gate/up against down)
// Short prompts (a 330-token request: 36 tiles for the o / down projections of a 1.5B layer, 48 for QKV): a few dozen workgroups
// stream the whole matrix -- 170 us for the 27.5 MB down projection.  K is split over grid.y (each part >= 4 of the 64-wide
// steps) until ~192 workgroups pull on HBM; the parts go to dense fp32 tensors and vv_g3_reduce_kernel sums them in part order
// with the bias / residual: deterministic, no hand-off inside a launch.
constexpr int VV_G3_SPLIT_BELOW_WGS = 128, VV_G3_SPLIT_TARGET_WGS = 192, VV_G3_MAX_SPLIT = 8, VV_G3_MIN_PART_STEPS = 4;
constexpr int VV_G3_DB_MAX_WGS = 512;            // at most ~2 workgroups per CU: nothing else hides a stage's latency -> two stage buffers

inline int vv_pf_k_steps(int K) { return ((K + 31) / 32 + 1) / 2; }       // 64-wide K steps of both kernels

// The K-split of the 256 x 256 kernel's partial last round (see VV_G4_ROUND): sets p->full_idx / split and the grid of a plan whose
// n_blocks / t_blocks are set.  Without the workspace every tile is computed whole.
inline void vv_g4_split_plan(int n_blocks, int t_blocks, int K, bool ws_round, VVGemm3Plan* p) {
    const int total = n_blocks * t_blocks, q = total >> 3, r = total & 7;
    p->full_idx = 0; p->split = 1;
    p->grid = dim3((unsigned)total);
    if (!ws_round) return;
    const int full_idx = (total / VV_G4_ROUND) * VV_G4_XCD_ROUND;
    const int max_rem = q + (r ? 1 : 0) - full_idx;           // 0..32 tiles per XCD in the partial round
    const int n_steps = vv_pf_k_steps(K);
    int split = max_rem > 0 ? VV_G4_XCD_ROUND / max_rem : 1;
    if (split > VV_G4_MAX_SPLIT) split = VV_G4_MAX_SPLIT;
    if (split > n_steps / VV_G4_MIN_PART_STEPS) split = n_steps / VV_G4_MIN_PART_STEPS;
    if (split == 2 && n_steps < VV_G4_HALVES_MIN_STEPS) split = 1;
    if (split > 1) {
        p->full_idx = full_idx; p->split = split;
        p->grid = dim3((unsigned)(8 * full_idx + 8 * max_rem * split));
    }
}

inline void vv_g4_plan(int n_blocks, int t_blocks, int K, int epi, bool ws_round, VVGemm3Plan* p) {
    p->form = VV_PF_G4; p->epi = epi; p->n_blocks = n_blocks; p->t_blocks = t_blocks;
    p->block = VV_G4_BLOCK; p->lds = VV_G4_LDS; p->ks = 1;
    vv_g4_split_plan(n_blocks, t_blocks, K, ws_round, p);
}

// Y (op)= Xp . W^T.  epi: VV_EPI_STORE / BIAS / RESID -> fp32 Y[T][ldy];  VV_EPI_SWIGLU -> packed bf16 Yp [T][N] (W = gate, W2 = up).
// -1: bad shape or operands;  VV_RC_NO_FORM: an epilogue without a prefill form;  0: *p is the launch.
inline int vv_gemm3_plan(int T, int N, int K, int ldy, int epi, bool has_w2, bool has_y, bool has_yp, VVPrefillWs ws, VVGemm3Plan* p) {
    if (T < 1 || N < 1 || K < 32 || (N & 3)) return -1;
    const bool dual = epi == VV_EPI_SWIGLU;
    if (!dual && epi != VV_EPI_RESID && epi != VV_EPI_BIAS && epi != VV_EPI_STORE) return VV_RC_NO_FORM;
    if (dual ? (!has_w2 || !has_yp) : (!has_y || (ldy & 3))) return -1;
    const int c_epi = epi == VV_EPI_STORE ? VV_EPI_BIAS : epi;
    const int n_tiles = (N + 15) / 16;
    const int ft4 = dual ? 8 : 16, t_blocks4 = (T + 255) / 256;       // feature tiles (per matrix) / row blocks of a 256 x 256 workgroup
    if ((int64_t)((n_tiles + ft4 - 1) / ft4) * t_blocks4 >= VV_G4_MIN_WGS) {
        vv_g4_plan((n_tiles + ft4 - 1) / ft4, t_blocks4, K, c_epi, ws.round, p);
        return 0;
    }
    const int ft = dual ? 4 : 8;
    p->epi = c_epi; p->n_blocks = (n_tiles + ft - 1) / ft; p->t_blocks = (T + 127) / 128;
    p->block = VV_G3_BLOCK; p->lds = 0; p->full_idx = 0; p->split = 1;
    const unsigned wgs = (unsigned)(p->n_blocks * p->t_blocks);
    int ks = 1;
    if (!dual && ws.g3_bytes && wgs < (unsigned)VV_G3_SPLIT_BELOW_WGS) {
        ks = (int)((VV_G3_SPLIT_TARGET_WGS + wgs - 1) / wgs);
        if (ks > VV_G3_MAX_SPLIT) ks = VV_G3_MAX_SPLIT;
        if (ks > vv_pf_k_steps(K) / VV_G3_MIN_PART_STEPS) ks = vv_pf_k_steps(K) / VV_G3_MIN_PART_STEPS;
        if (ks < 2 || (size_t)ks * T * N * 4 > ws.g3_bytes) ks = 1;        // all or nothing: the parts are dense [ks][T][N] tensors
    }
    p->ks = ks;
    p->grid = dim3(wgs, (unsigned)ks);
    p->form = (int64_t)wgs * ks <= VV_G3_DB_MAX_WGS ? VV_PF_G3_DB : VV_PF_G3;
    return 0;
}

// The QKV projection of a prompt pass with RoPE + KV-cache append in the epilogue: head_dim 128, whole 256-feature blocks, every
// operand present (rows, rope table, q_out, K and V caches), and a grid that fills the chip (the 256 x 256 kernel is the only one
// with that epilogue).  1: *p is the launch;  0: not this shape -- the caller runs the plain GEMM + vv_rope_append.
inline int vv_qkv_rope_plan(int T, int K, int D, int Hq, int Hkv, bool operands, bool ws_round, VVGemm3Plan* p) {
    const int N = (Hq + 2 * Hkv) * D;
    if (D != 128 || T < 1 || K < 32 || !operands) return 0;
    const int n_blocks = N / 256, t_blocks = (T + 255) / 256;
    if ((N & 255) || (int64_t)n_blocks * t_blocks < VV_G4_MIN_WGS) return 0;
    vv_g4_plan(n_blocks, t_blocks, K, VV_EPI_QKV_ROPE, ws_round, p);
    return 1;
}
