// gemv_plan.h -- which compiled form of vv_gemv_kernel (gemv.hip) a launch takes, decided on the host before anything is launched;
// at the end, the question one level up: which of the three GEMM kernels vv_gemm_launch runs a call on (vv_gemm_route), and the
// form and decomposition of the general kernel of gemm.hip where the route ends there (vv_gemm_general_plan).
// Plain host C++: no kernel, no HIP call, no operand pointer is dereferenced (a test drives it on a machine without a GPU).
#pragma once
#include "vv_common.h"

struct VVGemvForm { int xs, mr, wpb, parts, sl; };      // template arguments of the instantiation: <XS, pro, epi, MR, WPB, PARTS, SL>
struct VVGemvPlan { VVGemvForm form; dim3 grid; };      // block size = form.wpb * 64

// A family = one (MR, WPB, PARTS, SL) of vv_gemv_kernel, compiled for xs = 1..xs_max and for each (prologue, epilogue) pair of
// its list: exactly these instantiations exist (gemv.hip builds its table of kernels from this declaration and nothing else).
struct VVGemvPair { int pro, epi; };
struct VVGemvFamily {
    int mr, wpb, parts, sl, xs_max, n;
    const VVGemvPair* pair;
    template <int N>
    constexpr VVGemvFamily(int mr_, int wpb_, int parts_, int sl_, int xs_max_, const VVGemvPair (&p)[N])
        : mr(mr_), wpb(wpb_), parts(parts_), sl(sl_), xs_max(xs_max_), n(N), pair(p) {}
    constexpr bool has(int pro, int epi) const {
        for (int i = 0; i < n; ++i) if (pair[i].pro == pro && pair[i].epi == epi) return true;
        return false;
    }
};
// The (prologue, epilogue) pairs the engine actually issues; anything else runs on the general kernel.
inline constexpr VVGemvPair vv_gemv_pairs[] = {
    {VV_PRO_NONE, VV_EPI_STORE}, {VV_PRO_NONE, VV_EPI_BIAS}, {VV_PRO_NONE, VV_EPI_RESID}, {VV_PRO_NONE, VV_EPI_GATED_RESID},
    {VV_PRO_RMS, VV_EPI_BIAS}, {VV_PRO_RMS, VV_EPI_BIAS_GELU}, {VV_PRO_RMS, VV_EPI_SWIGLU}, {VV_PRO_RMS, VV_EPI_RESID}, {VV_PRO_RMS, VV_EPI_STORE},
    {VV_PRO_RMS_MOD, VV_EPI_SWIGLU}, {VV_PRO_RMS_MOD, VV_EPI_CFG_DPM}, {VV_PRO_RMS_MOD, VV_EPI_STORE},
    {VV_PRO_ADD_SILU, VV_EPI_STORE}, {VV_PRO_NORMDW, VV_EPI_BIAS_GELU}};
// pairs with a 4-wave form (wide outputs) and a 16-wave form (few tiles, long K); bench mode (xs == 1) only
inline constexpr VVGemvPair vv_gemv_pairs_w4[] = {
    {VV_PRO_RMS, VV_EPI_SWIGLU}, {VV_PRO_RMS_MOD, VV_EPI_SWIGLU}, {VV_PRO_RMS, VV_EPI_BIAS_GELU}, {VV_PRO_RMS, VV_EPI_BIAS},
    {VV_PRO_NONE, VV_EPI_STORE}, {VV_PRO_NONE, VV_EPI_BIAS}, {VV_PRO_ADD_SILU, VV_EPI_STORE}, {VV_PRO_NORMDW, VV_EPI_BIAS_GELU}};
inline constexpr VVGemvPair vv_gemv_pairs_w16[] = {
    {VV_PRO_NONE, VV_EPI_RESID}, {VV_PRO_NONE, VV_EPI_GATED_RESID}, {VV_PRO_NONE, VV_EPI_BIAS}, {VV_PRO_NONE, VV_EPI_STORE}};
// pairs that also exist in the 16-row form (prefill chunks, batched adaLN, T = 8 codec stage, connectors)
inline constexpr VVGemvPair vv_gemv_pairs_wide[] = {
    {VV_PRO_NONE, VV_EPI_STORE}, {VV_PRO_NONE, VV_EPI_BIAS}, {VV_PRO_NONE, VV_EPI_RESID}, {VV_PRO_RMS, VV_EPI_BIAS},
    {VV_PRO_RMS, VV_EPI_BIAS_GELU}, {VV_PRO_RMS, VV_EPI_SWIGLU}, {VV_PRO_ADD_SILU, VV_EPI_STORE}, {VV_PRO_NONE, VV_EPI_GATED_RESID}};
// 16-row pairs that also have a 4-wave form (tall tokenizer stages, batched adaLN)
inline constexpr VVGemvPair vv_gemv_pairs_wide4[] = {
    {VV_PRO_NONE, VV_EPI_STORE}, {VV_PRO_NONE, VV_EPI_BIAS}, {VV_PRO_NONE, VV_EPI_RESID}, {VV_PRO_RMS, VV_EPI_BIAS_GELU}};
// 16-row diffusion-head pairs (8 utterances x {cond, uncond} rows): two B operands -> 4-wave workgroups only (LDS)
inline constexpr VVGemvPair vv_gemv_pairs_wide_mod[] = {
    {VV_PRO_RMS_MOD, VV_EPI_SWIGLU}, {VV_PRO_RMS_MOD, VV_EPI_CFG_DPM}, {VV_PRO_RMS_MOD, VV_EPI_STORE}};
// pairs that can consume a K-split tensor: on the activation side (x) or on the residual side (y)
inline constexpr VVGemvPair vv_gemv_pairs_parts_x[] = {
    {VV_PRO_RMS, VV_EPI_BIAS}, {VV_PRO_RMS_MOD, VV_EPI_SWIGLU}, {VV_PRO_RMS_MOD, VV_EPI_CFG_DPM}, {VV_PRO_RMS_MOD, VV_EPI_STORE}};
inline constexpr VVGemvPair vv_gemv_pairs_parts_x_wide[] = {{VV_PRO_RMS_MOD, VV_EPI_SWIGLU}};   // wide outputs: only the gate/up projection has them
inline constexpr VVGemvPair vv_gemv_pairs_parts_y[] = {{VV_PRO_NONE, VV_EPI_RESID}, {VV_PRO_NONE, VV_EPI_GATED_RESID}};
// pairs with a slot-batched form: strided conv / transposed conv (bias), FFN1 (RMSNorm + bias + GELU), FFN2 (layer scale + residual)
inline constexpr VVGemvPair vv_gemv_pairs_slots[] = {{VV_PRO_NONE, VV_EPI_BIAS}, {VV_PRO_NONE, VV_EPI_RESID}, {VV_PRO_RMS, VV_EPI_BIAS_GELU}};

enum { VV_GF_DEFAULT, VV_GF_ROWS2_W4, VV_GF_ROWS4_W4, VV_GF_W16, VV_GF_WIDE, VV_GF_WIDE4, VV_GF_WIDE_MOD, VV_GF_PARTS_X, VV_GF_PARTS_X_ROWS2_W4,
       VV_GF_PARTS_X_W4, VV_GF_PARTS_Y, VV_GF_SLOTS, VV_GF_SLOTS4, VV_GF_COUNT };
constexpr int VV_GEMV_MAX_PAIRS = sizeof(vv_gemv_pairs) / sizeof(vv_gemv_pairs[0]), VV_GEMV_MAX_XS = 3;
inline constexpr VVGemvFamily vv_gemv_families[VV_GF_COUNT] = {      // in the order of the enum: {MR, WPB, PARTS, SL, xs_max, pairs}
    {4, 8, 0, 0, 3, vv_gemv_pairs},                   // DEFAULT
    {2, 4, 0, 0, 1, vv_gemv_pairs_w4},                // ROWS2_W4
    {4, 4, 0, 0, 1, vv_gemv_pairs_w4},                // ROWS4_W4
    {4, 16, 0, 0, 1, vv_gemv_pairs_w16},              // W16
    {16, 8, 0, 0, 2, vv_gemv_pairs_wide},             // WIDE: 16-row staging tiles of the exact mode (xs = 3) exceed the LDS: general kernel
    {16, 4, 0, 0, 1, vv_gemv_pairs_wide4},            // WIDE4
    {16, 4, 0, 0, 1, vv_gemv_pairs_wide_mod},         // WIDE_MOD
    {4, 8, 1, 0, 3, vv_gemv_pairs_parts_x},           // PARTS_X
    {2, 4, 1, 0, 1, vv_gemv_pairs_parts_x_wide},      // PARTS_X_ROWS2_W4: the 2-row form of the K-split consumer (7B-width A/B of the column split, round 6)
    {4, 4, 1, 0, 1, vv_gemv_pairs_parts_x_wide},      // PARTS_X_W4
    {4, 8, 2, 0, 3, vv_gemv_pairs_parts_y},           // PARTS_Y
    {16, 8, 0, 1, 2, vv_gemv_pairs_slots},            // SLOTS
    {16, 4, 0, 1, 1, vv_gemv_pairs_slots}};           // SLOTS4

// Eligibility, independent of xs: decode rows, aligned operands, 32-bit offsets, a specialised (prologue, epilogue) pair.
inline bool vv_gemv_eligible(const VVGemm* a) {
    const VVGemvFamily* const fam = vv_gemv_families;
    if (a->T < 1) return false;
    if (a->T > 4 || a->sl_n > 0) { if (!fam[VV_GF_WIDE].has(a->pro, a->epi) && !fam[VV_GF_WIDE_MOD].has(a->pro, a->epi)) return false; }
    else if (!fam[VV_GF_DEFAULT].has(a->pro, a->epi)) return false;
    if (a->sl_n > 0) {      // slot-batched rows: the three tokenizer pairs, plain operands, 32-bit offsets inside every slot buffer
        if (a->sl_n > 8 || a->sl_T < 1 || a->T != a->sl_n * a->sl_T || a->sl_x < 0 || a->sl_y < 0 || (a->sl_x & 3) || (a->sl_y & 3)) return false;
        if (a->kgrid > 1 || a->n_xa || a->n_ya || a->x_row_mod > 0 || a->add_rows_per_vec > 0) return false;
        if (!fam[VV_GF_SLOTS].has(a->pro, a->epi)) return false;
        for (int j = 0; j < a->sl_n; ++j)
            if (a->sl_id[j] < 0 || (int64_t)a->sl_id[j] * a->sl_x + (int64_t)a->sl_T * a->ldx >= (1LL << 30) ||
                (int64_t)a->sl_id[j] * a->sl_y + (int64_t)a->sl_T * a->ldy >= (1LL << 30)) return false;
    }
    if ((a->x_row_mod > 0 || a->add_rows_per_vec > 0) && a->pro != VV_PRO_ADD_SILU) return false;
    // CFG + solver epilogue: row r (cond) meets row r + n_cfg (uncond) by a lane shuffle inside ONE 16-row tile, and z / x0p are
    // indexed by the tile-local row -- so the launch is exactly the 2 * n_cfg rows of one tile (decode forms: n_cfg <= 2)
    if (a->epi == VV_EPI_CFG_DPM && (a->n_cfg < 1 || a->T != 2 * a->n_cfg || a->T > 16 || !a->z || !a->x0p || !a->coef)) return false;
    if (a->pro == VV_PRO_NORMDW) {     // one row, whole K inside every workgroup, every operand present and 16-B aligned
        if (a->T != 1 || a->sl_n > 0 || a->kgrid > 1 || a->n_xa || a->n_ya || !a->dw_hist || !a->dw_w || !a->dw_b || !a->dw_gamma ||
            !a->dw_nw || !a->dw_xout || !a->dw_hnew || a->dw_xout == a->X) return false;
        if ((((uintptr_t)a->dw_hist) | ((uintptr_t)a->dw_w) | ((uintptr_t)a->dw_b) | ((uintptr_t)a->dw_gamma) | ((uintptr_t)a->dw_nw) |
             ((uintptr_t)a->dw_xout) | ((uintptr_t)a->dw_hnew)) & 15) return false;
        if ((int64_t)7 * a->K >= (1LL << 30)) return false;
    }
    if ((a->K & 3) || (a->ldx & 3) || (((uintptr_t)a->X) & 15)) return false;
    if (a->pro == VV_PRO_RMS_MOD && (a->ld_mod & 3)) return false;
    if (a->nw && (((uintptr_t)a->nw) & 15)) return false;
    if (a->K < 32) return false;
    if ((int64_t)a->T * a->ldy >= (1LL << 30) || (int64_t)a->T * a->ldx >= (1LL << 30)) return false;
    if ((a->N & 3) || (a->ldy & 3)) return false;
    if ((((uintptr_t)a->Y) & 15) || (a->bias && (((uintptr_t)a->bias) & 15))) return false;
    if (a->nscale && (((uintptr_t)a->nscale) & 15)) return false;
    if (a->epi == VV_EPI_GATED_RESID && ((a->ld_gate & 3) || (((uintptr_t)a->gate) & 15))) return false;
    if (a->pro == VV_PRO_RMS_MOD && ((((uintptr_t)a->mod_scale) & 15) || (((uintptr_t)a->mod_shift) & 15))) return false;
    if (a->pro == VV_PRO_ADD_SILU && (((uintptr_t)a->addvec) & 15)) return false;
    if (a->kgrid > 1 && (a->T > 4 || a->kgrid != 3 || a->pro != VV_PRO_NONE || !a->yparts || (a->part_stride & 3) ||
                         (a->epi != VV_EPI_RESID && a->epi != VV_EPI_GATED_RESID) || (((uintptr_t)a->yparts) & 15))) return false;
    if ((a->n_xa > 0 && (!a->xa || (((uintptr_t)a->xa) & 15))) || (a->n_ya > 0 && (!a->ya || (((uintptr_t)a->ya) & 15)))) return false;
    if ((a->n_xa != 0 && a->n_xa != 2) || (a->n_ya != 0 && a->n_ya != 2) || (a->n_xa && a->n_ya)) return false;
    if ((a->n_xa || a->n_ya) && ((a->part_stride & 3) || a->T > 4 || !fam[a->n_xa > 0 ? VV_GF_PARTS_X : VV_GF_PARTS_Y].has(a->pro, a->epi))) return false;
    return true;
}

// The launcher picks WPB so that EVERY workgroup of the launch is resident at once (a second dispatch round costs a full
// load-latency chain): 4 waves for wide outputs, 16 for few tiles x long K, 8 otherwise.
constexpr int VV_GEMV_WIDE_TILES = 256;          // more output tiles than this: the 4-wave forms
constexpr int VV_GEMV_W16_MAX_TILES = 128, VV_GEMV_W16_MIN_KTILES = 96;     // at most / at least this many output / k-tiles: the 16-wave form
// The 16-row tiles are used by the codec (T = 5..16 rows): above ~half a workgroup per CU the 4-wave form
// (2x the resident workgroups per CU) wins; measured 3.117 -> 3.053 ms/frame on the 1.5B config for
// thresholds 64..128 vs 512 (DESIGN.md section 8 lists the sweep).
constexpr int VV_GEMV_WIDE4_WGS = 128;

// True when a compiled form exists for this launch at this xs; *out then holds the form and the grid.
inline bool vv_gemv_plan(const VVGemm* a, int xs, VVGemvPlan* out) {
    if (!vv_gemv_eligible(a)) return false;
    const VVGemvFamily* const fam = vv_gemv_families;
    const int n_tiles = (a->N + 15) / 16, k_tiles = (a->K + 31) / 32;
    const bool rows16 = a->T > 4 || a->sl_n > 0;                     // slots use the 16-row form at any T
    const int grid_y = rows16 ? (a->T + 15) / 16 : a->kgrid > 1 ? a->kgrid : 1;
    const auto fits = [&](int f) { return xs >= 1 && xs <= fam[f].xs_max && fam[f].has(a->pro, a->epi); };
    const bool wide = n_tiles > VV_GEMV_WIDE_TILES, wide4 = (int64_t)n_tiles * grid_y > VV_GEMV_WIDE4_WGS;
    int f = VV_GF_DEFAULT;          // the first rule that holds decides; a family that lacks this pair or this xs never holds
    if (a->sl_n > 0) f = wide4 && fits(VV_GF_SLOTS4) ? VV_GF_SLOTS4 : VV_GF_SLOTS;
    else if (rows16 && wide4 && fits(VV_GF_WIDE4)) f = VV_GF_WIDE4;
    else if (rows16) f = fits(VV_GF_WIDE) ? VV_GF_WIDE : VV_GF_WIDE_MOD;
    // consumers of a K-split tensor (decode rows only); wide outputs: only the gate/up projection (SwiGLU) has them
    else if (a->n_xa > 0 && wide && a->T <= 2 && fits(VV_GF_PARTS_X_ROWS2_W4)) f = VV_GF_PARTS_X_ROWS2_W4;
    else if (a->n_xa > 0) f = wide && fits(VV_GF_PARTS_X_W4) ? VV_GF_PARTS_X_W4 : VV_GF_PARTS_X;
    else if (a->n_ya > 0) f = VV_GF_PARTS_Y;
    else if (a->kgrid > 1) f = VV_GF_DEFAULT;                        // K split over workgroup columns (grid.y): the default form only
    // one utterance = two rows (cond + uncond): the 2-row form halves the activation registers and the staging tile, so
    // one more workgroup fits per SIMD (RMS_MOD + SwiGLU: 160 -> <= 128 VGPRs) and a 672-tile launch is resident at once
    else if (wide && a->T <= 2 && fits(VV_GF_ROWS2_W4)) f = VV_GF_ROWS2_W4;
    else if (wide && fits(VV_GF_ROWS4_W4)) f = VV_GF_ROWS4_W4;
    else if (n_tiles <= VV_GEMV_W16_MAX_TILES && k_tiles >= VV_GEMV_W16_MIN_KTILES && fits(VV_GF_W16)) f = VV_GF_W16;
    if (!fits(f)) return false;
    out->form = {xs, fam[f].mr, fam[f].wpb, fam[f].parts, fam[f].sl};
    out->grid = dim3(n_tiles, grid_y);
    return true;
}

// ---- W13 forms (vv_w13.h): the instantiations of vv_gemv_kernel that stream a matrix's 13-bit twin -- the diffusion head's gate/up and
// down projections of one utterance, in the forms the plan above gives them (wide outputs, and the default form of narrow models), and
// the four projections of an LM layer at 7B widths (QKV and gate/up: wide outputs, 2 rows; o and down: the default form).
// A W13 form keeps the wave K ranges, the staging, the MFMA order and the reduce of its bf16 form: same bits, 13/16 of the bytes.
// A tile row the format cannot hold streams bf16 inside the same launch (gemv.hip: WF), so a twin serves its matrix whatever it holds.
struct VVGemvW13Form { int pro, epi, mr, wpb; };
inline constexpr VVGemvW13Form vv_gemv_w13_forms[] = {
    {VV_PRO_RMS_MOD, VV_EPI_SWIGLU, 2, 4}, {VV_PRO_RMS_MOD, VV_EPI_SWIGLU, 4, 8}, {VV_PRO_NONE, VV_EPI_GATED_RESID, 4, 8},
    {VV_PRO_RMS, VV_EPI_BIAS, 2, 4}, {VV_PRO_RMS, VV_EPI_SWIGLU, 2, 4}, {VV_PRO_NONE, VV_EPI_RESID, 4, 8}};
constexpr int VV_GEMV_W13_FORMS = sizeof(vv_gemv_w13_forms) / sizeof(vv_gemv_w13_forms[0]);
inline int vv_gemv_w13_find(int pro, int epi, int mr, int wpb) {
    for (int i = 0; i < VV_GEMV_W13_FORMS; ++i) {
        const VVGemvW13Form& f = vv_gemv_w13_forms[i];
        if (f.pro == pro && f.epi == epi && f.mr == mr && f.wpb == wpb) return i;
    }
    return -1;
}
// what a W13 form asks of a launch beyond its bf16 form: bf16 mode, whole 4-k-tile groups and 16-feature tiles, no part tensors
inline bool vv_gemv_w13_shape(const VVGemm* a, int xs) {
    return xs == 1 && (a->K & 127) == 0 && (a->N & 15) == 0 && a->T <= 4 && a->kgrid <= 1 && a->n_xa == 0 && a->n_ya == 0 && a->sl_n == 0;
}
// index of the W13 form of this launch (the form vv_gemv_plan picks for it, streaming twins), or -1: the launch stays bf16
inline int vv_gemv_w13_form(const VVGemm* a, int xs) {
    VVGemvPlan p;
    if (!vv_gemv_w13_shape(a, xs) || !vv_gemv_plan(a, xs, &p) || p.form.parts || p.form.sl) return -1;
    return vv_gemv_w13_find(a->pro, a->epi, p.form.mr, p.form.wpb);
}

// ---- the MFMA tile GEMM (tile.hip): its pairs and its eligibility ----
constexpr int VV_TILE_BM = 64;          // rows per workgroup
#define VV_TILE_COMBOS(X)                                                                      \
    X(VV_PRO_NONE, VV_EPI_STORE) X(VV_PRO_NONE, VV_EPI_BIAS) X(VV_PRO_NONE, VV_EPI_RESID)      \
    X(VV_PRO_RMS, VV_EPI_BIAS) X(VV_PRO_RMS, VV_EPI_BIAS_GELU) X(VV_PRO_RMS, VV_EPI_SWIGLU)    \
    X(VV_PRO_RMS, VV_EPI_STORE)

// Eligibility: tall, aligned, enough workgroups (>= 48), one of the pairs above, bench / two-term activation modes, no row re-mapping or part tensors.
inline bool vv_tile_eligible(const VVGemm* a, int xs) {
    if (a->T < 32 || xs > 2) return false;
    {   // enough workgroups to occupy the chip; smaller problems (tokenizer stages at decode) stay on the row-tiled GEMV
        const int per_wg = 4 * (a->epi == VV_EPI_SWIGLU ? 1 : 2);
        const int64_t wgs = (int64_t)(((a->N + 15) / 16 + per_wg - 1) / per_wg) * ((a->T + VV_TILE_BM - 1) / VV_TILE_BM);
        // slot-batched tokenizer stages (several utterances' frames in one launch): the 16-row GEMV form re-normalises and
        // re-stages its 16 rows in every one of its (feature tiles x row tiles) workgroups -- 87 us for the C = 256 FFN1 of eight
        // utterances (1600 rows x 1024 features x 256: 0.8 GFLOP) -- so the tile form takes over much earlier there
        const int min_wgs = a->sl_n > 0 ? 40 : 48;
        if (wgs < min_wgs) return false;
    }
    if (a->sl_n > 0) {
        if (a->sl_n > 8 || a->sl_T < 1 || a->T != a->sl_n * a->sl_T || a->sl_x < 0 || a->sl_y < 0 || (a->sl_x & 3) || (a->sl_y & 3)) return false;
    }
    if ((a->K & 3) || (a->ldx & 3) || (a->N & 3) || (a->ldy & 3)) return false;
    if ((((uintptr_t)a->X) | ((uintptr_t)a->Y)) & 15) return false;
    if ((a->nw && (((uintptr_t)a->nw) & 15)) || (a->bias && (((uintptr_t)a->bias) & 15)) || (a->nscale && (((uintptr_t)a->nscale) & 15))) return false;
    if (a->x_row_mod > 0 || a->add_rows_per_vec > 0 || a->kgrid > 1 || a->n_xa > 0 || a->n_ya > 0 || a->ksplit > 0) return false;
    if (a->K < 32) return false;
    if (a->epi == VV_EPI_SWIGLU && !a->W2) return false;
#define X(P, E) if (a->pro == P && a->epi == E) return true;
    VV_TILE_COMBOS(X)
#undef X
    return false;
}

// ---- which kernel vv_gemm_launch (gemm.hip) runs a call on: the tile GEMM, the decode GEMV, the general kernel of gemm.hip, or none ----
enum { VV_ROUTE_TILE, VV_ROUTE_GEMV, VV_ROUTE_GENERAL, VV_ROUTE_NONE };
inline int vv_gemm_route(const VVGemm* a, int xs) {
    VVGemvPlan p;
    if (vv_tile_eligible(a, xs)) return VV_ROUTE_TILE;              // tall activations, slot-batched or not
    if (a->sl_n > 0) return xs <= 2 && vv_gemv_plan(a, xs, &p) ? VV_ROUTE_GEMV : VV_ROUTE_NONE;      // slot-batched rows: no general form
    if (a->ksplit <= 0 && vv_gemv_plan(a, xs, &p)) return VV_ROUTE_GEMV;
    if (a->kgrid > 1 || a->n_xa > 0 || a->n_ya > 0) return VV_ROUTE_NONE;      // part tensors exist only on the decode GEMV path
    return VV_ROUTE_GENERAL;
}

// ---- the general kernel (gemm.hip): the form vv_gemm_kernel<NT, XS, DUAL, WPB, MAXR, VEC> and the decomposition of a call ----
struct VVGemmGeneralPlan {
    bool vec, dual;             // aligned operands (float4 staging); two matrices (SwiGLU)
    int wpb, maxr, nt;          // waves per block, the staging tile's row capacity, tiles per wave
    int ks, t_pad;              // waves of a block that split K; LDS row stride of the staging tile (both go into the VVGemm argument)
    dim3 grid;
    size_t lds;                 // dynamic LDS bytes
};
constexpr int VV_GG_NT2_TILE_PAIRS = 4096;       // two tiles per wave once there are plenty of tiles (halves staging work per weight byte)
constexpr int VV_GG_WAVES = 2048, VV_GG_MIN_KSTEPS = 8;      // enough waves to cover 256 CUs x ~8, at least 8 k-steps (one batch) per wave
constexpr int VV_GG_FEW_TILES = 512;             // few tiles: give every tile its own workgroup (more CUs pulling on HBM) rather than packing tiles into one
inline int vv_pow2_floor(int v) { int p = 1; while (p * 2 <= v) p *= 2; return p; }

// -1: SwiGLU without its second matrix;  VV_RC_NO_FORM: unaligned SwiGLU;  0: *p is the launch.  `xs` in {1,2,3}.
inline int vv_gemm_general_plan(const VVGemm* a, int xs, VVGemmGeneralPlan* p) {
    const int n_tiles = (a->N + 15) / 16, k_tiles = (a->K + 31) / 32, t_tiles = (a->T + 15) / 16;
    p->dual = a->epi == VV_EPI_SWIGLU;
    if (p->dual && !a->W2) return -1;
    p->vec = ((a->K & 3) == 0) && ((a->ldx & 3) == 0) && ((((uintptr_t)a->X) & 15) == 0) && (a->pro != VV_PRO_RMS_MOD || (a->ld_mod & 3) == 0);
    if (!p->vec && p->dual) return VV_RC_NO_FORM;                  // SwiGLU operands are always aligned on this path
    p->t_pad = a->T < 16 ? a->T : 16;       // odd multiples avoid bank conflicts on the 8-byte writes
    // waves per block: 8 for decode-sized row counts (small staging tiles, deep K split), 4 otherwise -- and for the generic
    // form (odd K / unaligned rows): encoder stem, tiny test shapes
    p->wpb = (p->t_pad <= 4 && p->vec) ? 8 : 4;
    p->maxr = p->wpb == 8 ? 4 : 16;
    p->nt = (!p->dual && p->vec && (long)n_tiles * t_tiles >= VV_GG_NT2_TILE_PAIRS) ? 2 : 1;
    const long work = ((long)n_tiles + p->nt - 1) / p->nt * t_tiles;     // waves if K is not split
    int ks = 1;
    if (a->ksplit > 0) ks = a->ksplit;
    else {
        const int want = (int)((VV_GG_WAVES + work - 1) / work);
        ks = vv_pow2_floor(want < 1 ? 1 : want);
        const int kmax = vv_pow2_floor(k_tiles / VV_GG_MIN_KSTEPS < 1 ? 1 : k_tiles / VV_GG_MIN_KSTEPS);
        if (ks > kmax) ks = kmax;
    }
    if (ks > p->wpb) ks = p->wpb;
    if (a->ksplit <= 0 && p->wpb == 8 && work < VV_GG_FEW_TILES) { while (ks < p->wpb && (k_tiles / (ks * 2)) >= 2) ks *= 2; }
    p->ks = ks;
    const int per_block = p->wpb / ks * p->nt;
    p->grid = dim3((n_tiles + per_block - 1) / per_block, t_tiles);
    const size_t stage_b = (size_t)p->wpb * xs * 8 * 4 * p->t_pad * 16;
    const size_t red_b = (size_t)p->wpb * (p->dual ? 2 : p->nt) * 64 * 16 + (size_t)p->wpb * 64 * 4;
    p->lds = stage_b > red_b ? stage_b : red_b;
    return 0;
}
