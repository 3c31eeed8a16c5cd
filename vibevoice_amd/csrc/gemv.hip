// gemv.hip -- latency-lean decode variant of the weight-streaming GEMM (T <= 4 rows).
//
// At decode every dense op of the hot path is a chain of DEPENDENT small launches
// (~450 per frame), so a launch's fixed cost matters as much as its bandwidth.  An
// s_memtime trace of the general kernel (gemm.hip) showed ~7000 of ~8500 cycles of a
// small launch outside the weight stream: 64-bit address arithmetic and guarded-load
// branches in the prologue, a ds_bpermute reduction chain for RMSNorm's sum(x^2), two
// barriers around the split-K reduction, and an epilogue that only then starts loading
// its residual / bias / gate operands.  This kernel keeps the same data path
//   packed bf16 weight tiles --global_load_dwordx4 nt--> VGPR --MFMA 16x16x32--> fp32 acc
//   fp32 activations --float4--> prologue --bf16 split--> wave-private LDS B-fragments
// and restructures everything around it:
//   * one workgroup = one 16-feature tile (two for SwiGLU), its 8 waves split K evenly;
//   * 32-bit offsets from uniform bases (no 64-bit multiplies), k-range handled with
//     clamped loads + one uniform branch per batch instead of a branch per load;
//   * the epilogue wave issues its residual / bias / gate loads at kernel entry;
//   * sum(x^2) by DPP row reductions + readlane (no LDS permutes: vv_wave_sum_dpp);
//   * split-K partials go to a dedicated LDS region: a single barrier.
#include <array>
#include <utility>
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"
#include "vv_w13.h"

#ifdef VV_GEMM_TIMING
#define VV_STAMP(i) do { if (a.dbg && blockIdx.x == 0 && threadIdx.x == 0) a.dbg[i] = __builtin_amdgcn_s_memtime(); } while (0)
// per-workgroup wall-clock (100 MHz, chip-wide) entry/exit stamps: the launch's occupancy timeline (tools/gemv_timeline.py)
#define VV_BSTAMP(i) do { if (a.dbg && threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < 3200) a.dbg[16 + 2 * (blockIdx.y * gridDim.x + blockIdx.x) + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define VV_BSTAMP(i) do { } while (0)
#define VV_STAMP(i) do { } while (0)
#endif

namespace {

constexpr int U = 8;       // k-steps per batch (256 k = one float4 per lane per row)

// adaLN-modulated norm, decode rows (MR <= 4): the shift rows ride in the SAME B tile as the modulated activation rows, as columns
// MR..2MR-1 of the MFMA's 16 (a decode launch uses 2..4 of them) -- one operand, one accumulator set, half the ds_reads and MFMAs
// per k-step; the epilogue adds column r + MR to column r with one DPP row shift (A/B against the two-operand form:
// profiles/r06_mod_fold_ab.json); the 16-row batch form has no spare columns and keeps two operands.

// PRO / EPI are compile-time: a launch executes only the code of its own prologue/epilogue (the runtime-
// switched version spent a third of a small launch fetching and skipping code it never needed).
// MR = activation rows a launch can carry: 4 for decode steps, 16 for prefill chunks / batched adaLN / the T = 8 codec
// stage (same weight stream, 4x the staging work and LDS).
// WPB = waves per workgroup = K split inside the workgroup.  The launcher picks it so that EVERY workgroup of the launch
// is resident at once (a second dispatch round costs a full load-latency chain): 4 for wide outputs (> 256 tiles),
// 16 for few tiles x long K (the streaming rate of a CU is set by its waves' loads in flight), 8 otherwise.
// PARTS: the activation (prologue side) or residual (epilogue side) tensor arrives as base + 2 part tensors (the producer
// split K over 3 workgroup columns): the three loads are issued together and summed in a fixed order.
// SL: slot-batched rows (VVGemm::sl_*): the rows of one launch are gathered from / scattered to the streaming buffers of up
// to 8 utterances -- one weight pass for the tokenizer stages of a whole batch.  16-row form only.
// WF: weight format.  0: packed bf16 fragments.  1, 2: W13 planes (vv_w13.h; pW / pW2 are the twins, a.W / a.W2 the bf16 fragments): only
// the weight loads and the fragment handed to the MFMA change -- the wave K ranges, the staging batches, the order of MFMAs over k, the
// reduce and the epilogue are those of WF = 0, so the outputs are the same bits.  A wave's K range need not start or end on a 4-k-tile
// group: the groups at its ends are loaded whole and the k-tiles outside the range skipped (a neighbour wave of the same workgroup
// streams them too).  A tile row whose ok word is 0 (an element outside the format's span; a twin never packed) is one workgroup: it
// drops the groups it loaded and runs the bf16 loop of WF = 0 over a.W / a.W2 -- a workgroup-uniform branch only such rows pay for.
// That is WF = 2.  WF = 1 is the same stream without the ok word, the branch and the bf16 loop, for twins the host knows to be exact in
// every tile row (VVGemm::w13_exact; the diffusion head's matrices, re-read 20 times per step): the fall-back's presence alone costs
// the head's gate/up launch 0.4 us (profiles/w13_lm_ab.json), which an exact twin need not pay.
template <int XS, int PRO, int EPI, int MR, int WPB, int PARTS = 0, int SL = 0, int WF = 0>      // PARTS: 0 none, 1 activation side, 2 residual side
// The operands every wave needs before its first load (weight / activation bases, shape, strides) are separate leading
// scalar parameters: with -mllvm -amdgpu-kernarg-preload-count=16 the dispatcher delivers them in SGPRs at wave launch,
// so the first addresses do not wait for a scalar-cache round trip; the rest of VVGemm is fetched by one s_load batch.
__global__ __launch_bounds__(WPB * 64) void vv_gemv_kernel(const u32x4* __restrict__ pW, const u32x4* __restrict__ pW2,
                                                           const float* __restrict__ pX, float* __restrict__ pY,
                                                           const float* __restrict__ pnw, int pT, int pN, int pK, int pldx,
                                                           int pldy, const VVGemm a) {
    constexpr bool DUAL = (EPI == VV_EPI_SWIGLU);
    constexpr int NM = DUAL ? 2 : 1;
    // LDS: [wave][XS][U][4][MR] x 16 B staging tiles, then [wave][NM][64] f32x4 partials, then [wave][MR] ssq
    // adaLN-modulated norm: y = rs * W.(x*nw*(1+scale)) + W.shift -- two B operands and two accumulator sets, so the
    // 1/rms of the row is only needed in the epilogue (as for plain RMSNorm) and no pre-pass over x exists
    constexpr bool FOLD = (PRO == VV_PRO_RMS_MOD) && MR <= 4;
    constexpr int NOP = (PRO == VV_PRO_RMS_MOD && !FOLD) ? 2 : 1;
    constexpr int MRS = FOLD ? 2 * MR : MR;         // staged B columns: activation rows, then (folded form) their shift rows
    static_assert(WF == 0 || (XS == 1 && NOP == 1 && MR <= 4 && PARTS == 0 && SL == 0), "W13 forms: bf16 mode, decode rows, one operand");
    // one (k-step, k-group) plane of the staging tile = MR rows x 16 B; the 16-row form pads it by 16 B so that the planes
    // one staging store touches fall into different bank groups (unpadded: 256-B stride = the same 4 banks, 16-way conflict)
    constexpr int GSB = MRS * 16 + (MR == 16 ? 16 : 0);
    __shared__ __attribute__((aligned(16))) unsigned char stg_all[WPB * NOP * XS * U * 4 * GSB];
    __shared__ f32x4 red[WPB][NM * NOP][64];
    __shared__ float ssq_sh[WPB][MR];
    __shared__ float ssq1_sh[PRO == VV_PRO_NORMDW ? WPB : 1];
    // Pull every kernel argument into SGPRs with ONE batch of s_loads: left alone the compiler fetches
    // them lazily behind branches, i.e. 3-4 dependent ~600-cycle round trips on a launch's critical path.
    asm volatile("" ::"s"(a.mod_scale), "s"(a.mod_shift), "s"(a.addvec), "s"(a.bias), "s"(a.nscale), "s"(a.gate));
    asm volatile("" ::"s"(a.ld_mod), "s"(a.ld_gate), "s"(a.x_row_mod), "s"(a.add_rows_per_vec),
                 "s"(a.eps), "s"(a.z), "s"(a.x0p), "s"(a.coef), "s"(a.cfg), "s"(a.n_cfg));
    asm volatile("" ::"s"(a.yparts), "s"(a.xa), "s"(a.ya), "s"(a.n_xa), "s"(a.n_ya), "s"(a.part_stride));
    if constexpr (EPI == VV_EPI_CFG_DPM) asm volatile("" ::"s"(a.sde_noise), "s"(a.cfg_rows));
    VV_STAMP(0);
    VV_BSTAMP(0);
    int lane = threadIdx.x & 63;      // WF = 1: re-derived, with frow / fq / kk / st_off, in a tile row that falls back (see there)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // 16-row form: grid.y walks 16-row tiles of a tall activation (tokenizer stages, prefill chunks)
    const int t_base = (MR == 16) ? (int)blockIdx.y * 16 : 0;
    const int T = min(MR, pT - t_base);
    const unsigned tile = blockIdx.x;
    const unsigned k_tiles = (unsigned)(pK + 31) >> 5;
    // K range of this workgroup (grid.y splits K for few-tile x long-K shapes so that all CUs stream), then of this wave
    const unsigned KSB = (MR <= 4) ? gridDim.y : 1u;
    const unsigned ksb = (MR <= 4) ? blockIdx.y : 0u;
    const unsigned kchunk = (k_tiles + KSB - 1) / KSB;
    const unsigned kb0 = min(k_tiles, ksb * kchunk), kb1 = min(k_tiles, kb0 + kchunk);
    const unsigned kper = (kb1 - kb0 + WPB - 1) / WPB;
    const unsigned kt0 = kb0 + wave * kper;
    const unsigned kt1 = min(kb1, kt0 + kper);
    const bool has_k = kt0 < kt1;
    int frow = lane & 15, fq = lane >> 4;
    unsigned char* stg = stg_all + (size_t)wave * (NOP * XS * U * 4 * GSB);
    unsigned kk = lane * 4;
    unsigned st_off = ((kk >> 5) * 4 + ((kk & 31) >> 3)) * GSB + (kk & 7) * 2;

    // WF = 1: the bf16 fragments are a.W / a.W2, and only a tile row that falls back forms these addresses
    const u32x4* wbase = WF ? nullptr : pW + (size_t)tile * k_tiles * 64 + lane;
    const u32x4* wbase2 = DUAL && !WF ? pW2 + (size_t)tile * k_tiles * 64 + lane : nullptr;
    // W13: this tile row's groups in the twin's planes, and its scale word behind them (gridDim.x = the matrix's tile rows)
    const unsigned char* gbase = reinterpret_cast<const unsigned char*>(pW) + (size_t)tile * (k_tiles >> 2) * VV_W13_GROUP;
    const unsigned char* gbase2 = reinterpret_cast<const unsigned char*>(pW2) + (size_t)tile * (k_tiles >> 2) * VV_W13_GROUP;
    // groups in flight per stream: one weight batch (two streams: see the single-buffered bf16 form below), one and a half for one
    // stream (a fourth slot costs the 8-wave form its second resident workgroup per CU: 134 VGPRs)
    constexpr int RG = WF ? (DUAL ? 2 : 3) : 1;
    const unsigned g_lo = kt0 >> 2, g_hi = (kt1 + 3) >> 2, ph = kt0 & 3;
    VVW13Raw raw[RG][NM];
    auto g_load = [&](unsigned g, VVW13Raw (&dst)[NM]) {
        g = min(g, g_hi - 1);                              // clamped: a group past the range re-reads the last one, MFMAs skipped
        dst[0] = vv_w13_load(gbase + g * VV_W13_GROUP, lane);
        if constexpr (DUAL) dst[1] = vv_w13_load(gbase2 + g * VV_W13_GROUP, lane);
    };

    // slot-batched rows: per-row activation offsets (wave-uniform), computed once
    unsigned xoff_sl[SL ? MR : 1];
    if constexpr (SL) {
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            const int rg = t_base + r;
            const int j = rg / a.sl_T, tt = rg - j * a.sl_T;
            xoff_sl[r] = (r < T) ? (a.sl_x ? (unsigned)(vv_slot_id(a.sl_id, j) * a.sl_x + tt * pldx) : (unsigned)(rg * pldx)) : 0u;
        }
    }
    constexpr int MODR = (PRO == VV_PRO_RMS_MOD) ? MR : 1;
    constexpr int ADDR = (PRO == VV_PRO_ADD_SILU) ? MR : 1;
    constexpr int PR = (PARTS == 1) ? MR : 1;
    constexpr int DWH = (PRO == VV_PRO_NORMDW) ? 6 : 1, DWT = (PRO == VV_PRO_NORMDW) ? 7 : 1;
    struct XR { float4 x[MR]; float4 p0[PR]; float4 p1[PR]; float4 sc[MODR]; float4 sh[MODR]; float4 addv[ADDR]; float4 nwv;
                float4 dh[DWH]; float4 dt[DWT]; float4 db, dg, dn; };
    auto x_load = [&](unsigned ktb, XR& R) {
        unsigned k = ktb * 32 + kk;
        const bool kin = k < min(kt1 * 32, (unsigned)pK);
        if (!kin) k = 0;                                   // clamped: always a legal address, masked later
        R.nwv = pnw ? *reinterpret_cast<const float4*>(pnw + k) : float4{1.f, 1.f, 1.f, 1.f};
        if constexpr (PRO == VV_PRO_NORMDW) {          // one row: history rows, taps, bias, layer scale, first norm's weight
#pragma unroll
            for (int j = 0; j < 6; ++j) R.dh[j] = *reinterpret_cast<const float4*>(a.dw_hist + (unsigned)(j * pK) + k);
#pragma unroll
            for (int j = 0; j < 7; ++j) R.dt[j] = *reinterpret_cast<const float4*>(a.dw_w + (unsigned)(j * pK) + k);
            R.db = *reinterpret_cast<const float4*>(a.dw_b + k);
            R.dg = *reinterpret_cast<const float4*>(a.dw_gamma + k);
            R.dn = *reinterpret_cast<const float4*>(a.dw_nw + k);
        }
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            if (r < T) {
                const int rg = t_base + r;
                const int xr_idx = a.x_row_mod > 0 ? rg % a.x_row_mod : rg;
                if constexpr (SL) R.x[r] = *reinterpret_cast<const float4*>(pX + xoff_sl[r] + k);
                else R.x[r] = *reinterpret_cast<const float4*>(pX + (unsigned)(xr_idx * pldx) + k);
                if constexpr (PARTS == 1) {
                    R.p0[r] = *reinterpret_cast<const float4*>(a.xa + (unsigned)(xr_idx * pldx) + k);
                    R.p1[r] = *reinterpret_cast<const float4*>(a.xa + (unsigned)(a.part_stride + xr_idx * pldx) + k);
                }
                if constexpr (PRO == VV_PRO_ADD_SILU) {
                    const int av = a.add_rows_per_vec > 0 ? rg / a.add_rows_per_vec : 0;
                    R.addv[r] = *reinterpret_cast<const float4*>(a.addvec + (unsigned)(av * pK) + k);
                }
                if constexpr (PRO == VV_PRO_RMS_MOD) {
                    R.sc[r] = *reinterpret_cast<const float4*>(a.mod_scale + (unsigned)(rg * a.ld_mod) + k);
                    R.sh[r] = *reinterpret_cast<const float4*>(a.mod_shift + (unsigned)(rg * a.ld_mod) + k);
                }
            }
        }
    };
    auto w_load = [&](unsigned ktb, u32x4 (&dst)[U][NM]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned kt = min(ktb + u, kt1 - 1);      // clamped: tail k-steps re-read the last tile, MFMA skipped
            dst[u][0] = __builtin_nontemporal_load(wbase + kt * 64);
            if constexpr (DUAL) dst[u][1] = __builtin_nontemporal_load(wbase2 + kt * 64);
        }
    };
    // ---- first activation batch and first weight batch go out before anything else ----
    XR R;
    u32x4 wA[U][NM], wB[U][NM];      // WF = 1: live in a tile row that falls back alone
    if constexpr (WF) {
        if (has_k) {
            x_load(kt0, R);
#pragma unroll
            for (int q = 0; q < RG; ++q) g_load(g_lo + q, raw[q]);
        }
    } else
    if (has_k) { x_load(kt0, R); w_load(kt0, wA); }      // x first: its wait must not drag the weight stream along
    __builtin_amdgcn_sched_barrier(0);
    VV_STAMP(1);
    // PRO_NORMDW: 1/rms of the INPUT row is needed before anything can be staged (it sits inside the conv's newest tap): every
    // wave sums its own k-range of x (L2-resident, two loads per lane at C = 2048), one barrier -- under the first weight batch
    float rs1 = 1.0f;
    if constexpr (PRO == VV_PRO_NORMDW) {
        float s1 = 0.f;
        for (unsigned ktb = kt0; ktb < kt1; ktb += U) {
            const unsigned k = ktb * 32 + kk;
            if (k < min(kt1 * 32, (unsigned)pK)) {
                const float4 v = *reinterpret_cast<const float4*>(pX + k);
                s1 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
            }
        }
        s1 = vv_wave_sum_dpp(s1);
        if (lane == 0) ssq1_sh[wave] = s1;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < WPB; ++w) tot += ssq1_sh[w];
        rs1 = rsqrtf(tot / (float)pK + a.eps);
    }

    // ---- epilogue operands: requested now, consumed ~one weight stream later (wave 0 only) ----
    const int n0 = tile * 16 + fq * 4;
    const bool epi_lane = (wave == 0) && frow < T && n0 < pN;
    float4 pre_y = {0.f, 0.f, 0.f, 0.f}, pre_b = {0.f, 0.f, 0.f, 0.f}, pre_g = {1.f, 1.f, 1.f, 1.f};
    float4 pre_y0 = {0.f, 0.f, 0.f, 0.f}, pre_y1 = {0.f, 0.f, 0.f, 0.f};
    unsigned yrow_off = (unsigned)((t_base + frow) * pldy);
    if constexpr (SL) {
        const int rg = min(t_base + frow, pT - 1);
        const int j = rg / a.sl_T, tt = rg - j * a.sl_T;
        yrow_off = a.sl_y ? (unsigned)(vv_slot_id(a.sl_id, j) * a.sl_y + tt * pldy) : (unsigned)(rg * pldy);
    }
    if (epi_lane) {            // N % 4 == 0 and 16-B aligned operands are launch preconditions (vv_gemv_ok)
        if constexpr (EPI == VV_EPI_BIAS || EPI == VV_EPI_BIAS_GELU || EPI == VV_EPI_RESID) {
            if (a.bias) pre_b = *reinterpret_cast<const float4*>(a.bias + n0);
        }
        if constexpr (EPI == VV_EPI_RESID || EPI == VV_EPI_GATED_RESID) {
            pre_y = *reinterpret_cast<const float4*>(pY + (yrow_off + (unsigned)n0));
            if constexpr (PARTS == 2) {
                const float* yp0 = a.ya + (unsigned)((t_base + frow) * pldy + n0);
                pre_y0 = *reinterpret_cast<const float4*>(yp0);
                pre_y1 = *reinterpret_cast<const float4*>(yp0 + a.part_stride);
            }
            if constexpr (EPI == VV_EPI_GATED_RESID) pre_g = *reinterpret_cast<const float4*>(a.gate + (unsigned)((t_base + frow) * a.ld_gate + n0));
            else if (a.nscale) pre_g = *reinterpret_cast<const float4*>(a.nscale + n0);
        }
    }

    f32x4 acc[NM * NOP];            // [NM, 2NM): the shift operand's products (RMS_MOD)
#pragma unroll
    for (int i = 0; i < NM * NOP; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ssq[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) ssq[r] = 0.f;

    auto x_stage = [&](unsigned ktb, const XR& R) {
        const unsigned k = ktb * 32 + kk;
        const float msk = (k < min(kt1 * 32, (unsigned)pK)) ? 1.f : 0.f;
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            if (r < T) {
                float v[4] = {R.x[r].x, R.x[r].y, R.x[r].z, R.x[r].w};
                if constexpr (PARTS == 1) {
                    v[0] = (v[0] + R.p0[r].x) + R.p1[r].x; v[1] = (v[1] + R.p0[r].y) + R.p1[r].y;
                    v[2] = (v[2] + R.p0[r].z) + R.p1[r].z; v[3] = (v[3] + R.p0[r].w) + R.p1[r].w;
                }
                v[0] *= msk; v[1] *= msk; v[2] *= msk; v[3] *= msk;
                if constexpr (PRO == VV_PRO_RMS) {
                    ssq[r] += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
                    v[0] *= R.nwv.x; v[1] *= R.nwv.y; v[2] *= R.nwv.z; v[3] *= R.nwv.w;
                } else if constexpr (PRO == VV_PRO_NORMDW) {
                    if (r == 0) {
                        const float xn[4] = {R.dn.x, R.dn.y, R.dn.z, R.dn.w}, bb[4] = {R.db.x, R.db.y, R.db.z, R.db.w};
                        const float gg[4] = {R.dg.x, R.dg.y, R.dg.z, R.dg.w}, n2[4] = {R.nwv.x, R.nwv.y, R.nwv.z, R.nwv.w};
                        float hn[4], xo[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            hn[e] = v[e] * rs1 * xn[e];                    // the new normed row (the conv's newest input)
                            float acc = bb[e];
#pragma unroll
                            for (int j = 0; j < 6; ++j) acc += reinterpret_cast<const float*>(&R.dt[j])[e] * reinterpret_cast<const float*>(&R.dh[j])[e];
                            acc += reinterpret_cast<const float*>(&R.dt[6])[e] * hn[e];
                            xo[e] = (v[e] + gg[e] * acc) * msk;
                        }
                        if (tile == 0 && msk != 0.f) {                     // one workgroup publishes the block's intermediate rows
                            *reinterpret_cast<float4*>(a.dw_xout + k) = float4{xo[0], xo[1], xo[2], xo[3]};
                            *reinterpret_cast<float4*>(a.dw_hnew + k) = float4{hn[0], hn[1], hn[2], hn[3]};
                        }
                        ssq[r] += xo[0] * xo[0] + xo[1] * xo[1] + xo[2] * xo[2] + xo[3] * xo[3];
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = xo[e] * n2[e];
                    }
                } else if constexpr (PRO == VV_PRO_RMS_MOD) {
                    ssq[r] += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
                    v[0] = (v[0] * R.nwv.x) * (1.f + R.sc[r].x); v[1] = (v[1] * R.nwv.y) * (1.f + R.sc[r].y);
                    v[2] = (v[2] * R.nwv.z) * (1.f + R.sc[r].z); v[3] = (v[3] * R.nwv.w) * (1.f + R.sc[r].w);
                    float sh4[4] = {R.sh[r].x * msk, R.sh[r].y * msk, R.sh[r].z * msk, R.sh[r].w * msk};
                    uint2 sparts[XS];
                    vv_split_bf16<XS>(sh4, sparts);
#pragma unroll
                    for (int p = 0; p < XS; ++p) {
                        if constexpr (FOLD) *reinterpret_cast<uint2*>(stg + p * (U * 4 * GSB) + st_off + (MR + r) * 16) = sparts[p];
                        else *reinterpret_cast<uint2*>(stg + (XS + p) * (U * 4 * GSB) + st_off + r * 16) = sparts[p];
                    }
                } else if constexpr (PRO == VV_PRO_ADD_SILU) {
                    v[0] = vv_silu(v[0] + R.addv[r].x) * msk; v[1] = vv_silu(v[1] + R.addv[r].y) * msk;
                    v[2] = vv_silu(v[2] + R.addv[r].z) * msk; v[3] = vv_silu(v[3] + R.addv[r].w) * msk;
                }
                uint2 parts[XS];
                vv_split_bf16<XS>(v, parts);
#pragma unroll
                for (int p = 0; p < XS; ++p)
                    *reinterpret_cast<uint2*>(stg + p * (U * 4 * GSB) + st_off + r * 16) = parts[p];
            }
        }
    };
    auto mma = [&](unsigned ktb, const u32x4 (&wb)[U][NM]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ktb + u < kt1) {
#pragma unroll
                for (int p = 0; p < XS; ++p) {
                    u32x4 f = u32x4{0u, 0u, 0u, 0u};
                    if (frow < MRS) f = *reinterpret_cast<const u32x4*>(stg + (size_t)((p * U + u) * 4 + fq) * GSB + frow * 16);
                    const bf16x8 xb = __builtin_bit_cast(bf16x8, f);
#pragma unroll
                    for (int i = 0; i < NM; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wb[u][i]), xb, acc[i], 0, 0, 0);
                    if constexpr (NOP == 2) {
                        u32x4 f2 = u32x4{0u, 0u, 0u, 0u};
                        if (frow < MR) f2 = *reinterpret_cast<const u32x4*>(stg + (size_t)(((XS + p) * U + u) * 4 + fq) * GSB + frow * 16);
                        const bf16x8 sb = __builtin_bit_cast(bf16x8, f2);
#pragma unroll
                        for (int i = 0; i < NM; ++i)
                            acc[NM + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wb[u][i]), sb, acc[NM + i], 0, 0, 0);
                    }
                }
            }
        }
    };

    if constexpr (WF) {
        float wscale[NM];
        // the W13 weight stream of a wave with K: the raw slots hold its first groups, the activations of its first batch are staged;
        // Rx: the registers of the batches that follow
        auto w13_loop = [&](XR& Rx) {
        const unsigned klen = kt1 - kt0;
        // k-tile j of the wave (0 = kt0) sits in staging slot j & 7 of activation batch j >> 3, exactly as in the bf16 form
        auto mma1 = [&](const u32x4 (&f)[NM][4], int t, unsigned slot) {
            u32x4 xf = u32x4{0u, 0u, 0u, 0u};
            if (frow < MRS) xf = *reinterpret_cast<const u32x4*>(stg + (size_t)(slot * 4 + fq) * GSB + frow * 16);
            const bf16x8 xb = __builtin_bit_cast(bf16x8, xf);
#pragma unroll
            for (int i = 0; i < NM; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f[i][t]), xb, acc[i], 0, 0, 0);
        };
        // weight batch i = groups g_lo + 2i, + 1 = k-tiles 8i - ph .. 8i + 7 - ph of the wave: the first ph of them belong to the
        // activation batch i - 1 still staged, the others to batch i, staged between the two
        auto wstep = [&](unsigned i, auto s0c, auto s1c) {      // s0, s1: the raw slots of the batch's two groups
            constexpr int sl[2] = {decltype(s0c)::value, decltype(s1c)::value};
#pragma unroll
            for (int gi = 0; gi < 2; ++gi) {
                u32x4 f[NM][4];
                if (gi == 0) {
                    if (ph > 0 && i > 0) {      // a range that starts inside a group (narrow models): decoded for these k-tiles alone
#pragma unroll
                        for (int m = 0; m < NM; ++m) vv_w13_unpack(raw[sl[0]][m], wscale[m], f[m]);
#pragma unroll
                        for (int t = 0; t < 3; ++t)
                            if ((unsigned)t < ph && 8 * i + t - ph < klen) mma1(f, t, 8 + t - ph);
                    }
                    if (i > 0 && 8 * i < klen) x_stage(kt0 + 8 * i, Rx);
                    if (8 * (i + 1) < klen) x_load(kt0 + 8 * (i + 1), Rx);
                }
#pragma unroll
                for (int m = 0; m < NM; ++m) vv_w13_unpack(raw[sl[gi]][m], wscale[m], f[m]);
                const unsigned gn = g_lo + 2 * i + gi + RG;
                if (gn < g_hi) g_load(gn, raw[sl[gi]]);      // the slot's next group goes out before this one's MFMAs
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if ((unsigned)t >= (gi == 0 ? ph : 0u) && 8 * i + 4 * gi + t - ph < klen) mma1(f, t, 4 * gi + t - ph);
            }
        };
        const unsigned n_wb = (ph + klen + 7) >> 3;
        using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>; using S2 = std::integral_constant<int, 2>;
        if constexpr (RG == 2) {
#pragma unroll 1
            for (unsigned i = 0; i < n_wb; ++i) wstep(i, S0{}, S1{});
        } else {
#pragma unroll 1
            for (unsigned i = 0; i < n_wb; i += 3) {
                wstep(i, S0{}, S1{});
                if (i + 1 < n_wb) wstep(i + 1, S2{}, S0{});
                if (i + 2 < n_wb) wstep(i + 2, S1{}, S2{});
            }
        }
        };
        if constexpr (WF == 1) {        // every tile row of the twin(s) is known to be exact: no ok word is read, no bf16 loop exists
            {
                const size_t tail = (size_t)gridDim.x * (k_tiles >> 2) * VV_W13_GROUP;
                wscale[0] = vv_w13_scale(reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(pW) + tail)[tile]);
                if constexpr (DUAL) wscale[1] = vv_w13_scale(reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(pW2) + tail)[tile]);
            }
            if (has_k) {
                x_stage(kt0, R);
                VV_STAMP(2);
                w13_loop(R);
            }
        } else {
            unsigned w13_ok;            // the tile row's ok word(s), fetched with its scale word(s): one scalar batch
            {
                const unsigned n_tiles = (unsigned)pN >> 4;      // = gridDim.x, from a preloaded argument: no round trip in front of the batch
                const size_t tail = (size_t)n_tiles * (k_tiles >> 2) * VV_W13_GROUP;
                const unsigned* t1 = reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(pW) + tail);
                unsigned sw[NM];
                sw[0] = t1[tile];
                w13_ok = t1[n_tiles + tile];
                if constexpr (DUAL) {
                    const unsigned* t2 = reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(pW2) + tail);
                    sw[1] = t2[tile];
                    w13_ok &= t2[n_tiles + tile];
                    asm volatile("" ::"s"(sw[1]));
                }
                // all of them in SGPRs here, under the first activation batch still in flight: left alone the compiler sinks the scale
                // load behind the branch on the ok word, a scalar round trip in front of the weight loop of every launch
                asm volatile("" ::"s"(sw[0]), "s"(w13_ok));
#pragma unroll
                for (int m = 0; m < NM; ++m) wscale[m] = vv_w13_scale(sw[m]);
            }
            if (has_k) x_stage(kt0, R);
            VV_STAMP(2);
            // a tile row that falls back: the bf16 weight stream of WF = 0 below, statement for statement (wA holds the batch at kt0, the
            // activations of that batch are staged; Rx: the registers of the batches that follow).  Kept textually apart from it: with the
            // WF = 0 loop routed through this lambda the register allocation of 44 bf16 forms moved by 1-8 VGPRs and one of them lost a wave.
            auto w_stream = [&](XR& Rx) {
                if constexpr (DUAL) {
#pragma unroll 1
                    for (unsigned ktb = kt0; ktb < kt1; ktb += U) {
                        const bool n1 = ktb + U < kt1;
                        if (n1) x_load(ktb + U, Rx);
                        mma(ktb, wA);
                        if (n1) { w_load(ktb + U, wA); x_stage(ktb + U, Rx); }
                    }
                } else
#pragma unroll 1
                for (unsigned ktb = kt0; ktb < kt1; ktb += 2 * U) {
                    const bool n1 = ktb + U < kt1, n2 = ktb + 2 * U < kt1;
                    if (n1) { x_load(ktb + U, Rx); w_load(ktb + U, wB); }
                    mma(ktb, wA);
                    if (n1) x_stage(ktb + U, Rx);
                    if (n2) { x_load(ktb + 2 * U, Rx); w_load(ktb + 2 * U, wA); }
                    if (n1) mma(ktb + U, wB);
                    if (n2) x_stage(ktb + 2 * U, Rx);
                }
            };
            // Registers: both arms below keep the activations of their later batches in registers of their own (Rf; Rw, a copy of R), and the
            // fall-back arm derives its lane constants afresh behind an opaque copy.  With R or those constants shared between the arms the
            // compiler holds them across the W13 loop as well: +18 VGPRs on the 8-wave forms, one resident workgroup per CU less.  Rw starts
            // as a copy of R rather than undefined: with nothing in it the next batch's activation loads were scheduled behind the weight
            // groups of the trip, and the wait for them (vmcnt 16 -> 4) drained the weight stream once per batch: +0.35 us on a head gate/up
            // launch.  The fall-back arm is marked unlikely so that block placement and allocation favour the W13 loop.
            if (__builtin_expect(w13_ok == 0, 0)) {          // this tile row streams bf16: the groups in flight are dropped, the weight stream starts over
                if (has_k) {
                    asm volatile("" : "+v"(lane));
                    frow = lane & 15; fq = lane >> 4; kk = lane * 4;
                    st_off = ((kk >> 5) * 4 + ((kk & 31) >> 3)) * GSB + (kk & 7) * 2;
                    wbase = a.W + (size_t)tile * k_tiles * 64 + lane;
                    if constexpr (DUAL) wbase2 = a.W2 + (size_t)tile * k_tiles * 64 + lane;
                    w_load(kt0, wA);
                    XR Rf;
                    w_stream(Rf);
                }
            } else if (has_k) {
                XR Rw = R;      // a copy, not R itself: see above
                w13_loop(Rw);
            }
        }
    } else
    if (has_k) {
        x_stage(kt0, R);
        VV_STAMP(2);
        // two batches per trip, ping-ponging the weight buffers: no register copies, so the prefetched batch
        // stays in flight across the MFMAs of the current one
        if constexpr (DUAL) {
            // two weight streams: a second weight buffer costs 64 VGPRs and halves the resident workgroups per CU
            // (1 instead of 2); run single-buffered and let the other resident waves cover the load latency
#pragma unroll 1
            for (unsigned ktb = kt0; ktb < kt1; ktb += U) {
                const bool n1 = ktb + U < kt1;
                if (n1) x_load(ktb + U, R);
                mma(ktb, wA);
                if (n1) { w_load(ktb + U, wA); x_stage(ktb + U, R); }
            }
        } else
#pragma unroll 1
        for (unsigned ktb = kt0; ktb < kt1; ktb += 2 * U) {
            const bool n1 = ktb + U < kt1, n2 = ktb + 2 * U < kt1;
            if (n1) { x_load(ktb + U, R); w_load(ktb + U, wB); }
            mma(ktb, wA);
            if (n1) x_stage(ktb + U, R);
            if (n2) { x_load(ktb + 2 * U, R); w_load(ktb + 2 * U, wA); }
            if (n1) mma(ktb + U, wB);
            if (n2) x_stage(ktb + 2 * U, R);
        }
    }
    // rows beyond T were never staged: their fragment slots hold stale LDS -> D columns >= T are garbage, never stored.

    VV_STAMP(3);
    // ---- split-K partials -> LDS, one barrier, wave 0 finishes ----
#pragma unroll
    for (int i = 0; i < NM * NOP; ++i) red[wave][i][lane] = acc[i];
    if constexpr (PRO == VV_PRO_RMS || PRO == VV_PRO_RMS_MOD || PRO == VV_PRO_NORMDW) {
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            const float s = (r < T) ? vv_wave_sum_dpp(ssq[r]) : 0.f;
            if (lane == 0) ssq_sh[wave][r] = s;
        }
    }
    VV_STAMP(4);
    __syncthreads();
    VV_STAMP(5);
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < WPB; ++w)
#pragma unroll
        for (int i = 0; i < NM * NOP; ++i) acc[i] += red[w][i][lane];
    f32x4 shf[FOLD ? NM : 1];                      // folded form: W.shift of row r sits in column r + MR -> row_shl:MR brings it to lane r
    if constexpr (FOLD) {
#pragma unroll
        for (int i = 0; i < NM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float av = acc[i][r];        // through a scalar temporary: bit_cast applied to a vector ELEMENT reads element 0 under this clang
                const int sv = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, av), 0x100 + MR, 0xF, 0xF, true);
                shf[i][r] = __builtin_bit_cast(float, sv);
            }
    }
    if (!epi_lane) return;
    float rs = 1.0f;
    if constexpr (PRO == VV_PRO_RMS || PRO == VV_PRO_RMS_MOD || PRO == VV_PRO_NORMDW) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WPB; ++w) s += ssq_sh[w][frow];
        rs = rsqrtf(s / (float)pK + a.eps);
    }
    float o[4] = {acc[0][0] * rs, acc[0][1] * rs, acc[0][2] * rs, acc[0][3] * rs};
    float up[4] = {0.f, 0.f, 0.f, 0.f};            // SwiGLU: the "up" half
    if constexpr (DUAL) { up[0] = acc[1][0] * rs; up[1] = acc[1][1] * rs; up[2] = acc[1][2] * rs; up[3] = acc[1][3] * rs; }
    if constexpr (NOP == 2) {                      // + W.shift
#pragma unroll
        for (int r = 0; r < 4; ++r) { o[r] += acc[NM][r]; if constexpr (DUAL) up[r] += acc[NM + 1][r]; }
    }
    if constexpr (FOLD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { o[r] += shf[0][r]; if constexpr (DUAL) up[r] += shf[1][r]; }
    }
    const float pb[4] = {pre_b.x, pre_b.y, pre_b.z, pre_b.w};
    const float py[4] = {(pre_y.x + pre_y0.x) + pre_y1.x, (pre_y.y + pre_y0.y) + pre_y1.y, (pre_y.z + pre_y0.z) + pre_y1.z, (pre_y.w + pre_y0.w) + pre_y1.w};
    const float pg[4] = {pre_g.x, pre_g.y, pre_g.z, pre_g.w};
    if constexpr (EPI == VV_EPI_BIAS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += pb[r];
    } else if constexpr (EPI == VV_EPI_BIAS_GELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = vv_gelu_erf(o[r] + pb[r]);
    } else if constexpr (EPI == VV_EPI_SWIGLU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = vv_silu(o[r]) * up[r];
    } else if constexpr (EPI == VV_EPI_RESID) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (ksb == 0) ? py[r] + pg[r] * (o[r] + pb[r]) : pg[r] * o[r];
    } else if constexpr (EPI == VV_EPI_GATED_RESID) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (ksb == 0) ? py[r] + pg[r] * o[r] : pg[r] * o[r];
    }
    if constexpr (EPI == VV_EPI_CFG_DPM) {
        const int nc = a.n_cfg;
        const VVSolverCoef cf = vv_solver_coef(a.coef, a.sde_noise != nullptr);
        float cfg = a.cfg;
        if (a.cfg_rows && frow < nc) cfg = a.cfg_rows[frow];     // one guidance scale per utterance row
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float vu = __shfl(o[r], lane + nc);
            const int n = n0 + r;
            if (frow < nc && n < pN) {
                const unsigned zi = (unsigned)(frow * pN + n);
                float x0, zn;
                vv_cfg_dpm_update(o[r], vu, cfg, a.z[zi], a.x0p[zi], cf, a.sde_noise != nullptr, [&] { return a.sde_noise[zi]; }, x0, zn);
                a.x0p[zi] = x0;
                a.z[zi] = zn;
                a.z[zi + (unsigned)(nc * pN)] = zn;
            }
        }
        return;
    }
    float* yp = (ksb == 0 ? pY : a.yparts + (unsigned)((ksb - 1) * a.part_stride)) + (yrow_off + (unsigned)n0);
    *reinterpret_cast<float4*>(yp) = float4{o[0], o[1], o[2], o[3]};
    VV_STAMP(6);
    VV_BSTAMP(1);
}

}  // namespace

extern "C" int vv_gemv_ok(const VVGemm* a) { return vv_gemv_eligible(a); }

// One kernel per (family, pair of the family, xs <= the family's xs_max) of gemv_plan.h -- the whole set of instantiations.
using GemvKernel = void (*)(const u32x4*, const u32x4*, const float*, float*, const float*, int, int, int, int, int, const VVGemm);
template <int F, int I, int XS>
static constexpr GemvKernel gemv_kernel_at() {
    constexpr const VVGemvFamily& f = vv_gemv_families[F];
    if constexpr (I < f.n && XS <= f.xs_max) return vv_gemv_kernel<XS, f.pair[I].pro, f.pair[I].epi, f.mr, f.wpb, f.parts, f.sl>;
    else return nullptr;
}
template <size_t... J>      // J = (family * VV_GEMV_MAX_PAIRS + pair) * VV_GEMV_MAX_XS + xs - 1
static constexpr std::array<GemvKernel, sizeof...(J)> gemv_kernel_table(std::index_sequence<J...>) {
    return {gemv_kernel_at<J / (VV_GEMV_MAX_PAIRS * VV_GEMV_MAX_XS), J / VV_GEMV_MAX_XS % VV_GEMV_MAX_PAIRS, J % VV_GEMV_MAX_XS + 1>()...};
}
static const auto gemv_kernels = gemv_kernel_table(std::make_index_sequence<VV_GF_COUNT * VV_GEMV_MAX_PAIRS * VV_GEMV_MAX_XS>{});

// the W13 forms of gemv_plan.h: [form][0] its bf16 instantiation (one of the table above), [form][1] the one that streams twins known
// to be exact, [form][2] the one that streams twins and falls back to bf16 per tile row
template <size_t... J>
static constexpr std::array<std::array<GemvKernel, 3>, sizeof...(J)> gemv_w13_table(std::index_sequence<J...>) {
    return {{{vv_gemv_kernel<1, vv_gemv_w13_forms[J].pro, vv_gemv_w13_forms[J].epi, vv_gemv_w13_forms[J].mr, vv_gemv_w13_forms[J].wpb, 0, 0, 0>,
              vv_gemv_kernel<1, vv_gemv_w13_forms[J].pro, vv_gemv_w13_forms[J].epi, vv_gemv_w13_forms[J].mr, vv_gemv_w13_forms[J].wpb, 0, 0, 1>,
              vv_gemv_kernel<1, vv_gemv_w13_forms[J].pro, vv_gemv_w13_forms[J].epi, vv_gemv_w13_forms[J].mr, vv_gemv_w13_forms[J].wpb, 0, 0, 2>}...}};
}
static const auto gemv_w13_kernels = gemv_w13_table(std::make_index_sequence<VV_GEMV_W13_FORMS>{});

static GemvKernel gemv_kernel(const VVGemvForm& form, int pro, int epi) {
    for (int f = 0; f < VV_GF_COUNT; ++f) {
        const VVGemvFamily& fam = vv_gemv_families[f];
        if (fam.mr != form.mr || fam.wpb != form.wpb || fam.parts != form.parts || fam.sl != form.sl || form.xs > fam.xs_max) continue;
        for (int i = 0; i < fam.n; ++i)
            if (fam.pair[i].pro == pro && fam.pair[i].epi == epi) return gemv_kernels[(f * VV_GEMV_MAX_PAIRS + i) * VV_GEMV_MAX_XS + form.xs - 1];
    }
    return nullptr;
}

// form (optional, tests): receives {XS, MR, WPB, PARTS, SL} of the plan this call launches -- the kernel is looked up from
// these very numbers, so it IS the dispatch decision, not a restatement of it.  The engine passes nullptr.
extern "C" int vv_gemv_launch(VVGemm a, int xs, hipStream_t s, int* form) {
    if (a.epi == VV_EPI_SWIGLU && !a.W2) return -1;
    VVGemvPlan p;
    if (!vv_gemv_plan(&a, xs, &p)) return VV_RC_NO_FORM;
    GemvKernel k = gemv_kernel(p.form, a.pro, a.epi);      // never null: the plan and the table read the same declaration
    if (a.w13) {            // the caller asked for the twins: a W13 form of this very plan exists (vv_gemv_w13_form), or the call is refused
        const int wi = vv_gemv_w13_form(&a, xs);
        if (wi < 0 || (a.epi == VV_EPI_SWIGLU && !a.w13_2)) return VV_RC_NO_FORM;
        k = gemv_w13_kernels[wi][a.w13_exact ? 1 : 2];
    }
    if (form) { form[0] = p.form.xs; form[1] = p.form.mr; form[2] = p.form.wpb; form[3] = p.form.parts; form[4] = p.form.sl; }
    // a W13 form takes the twins as its leading (preloaded) pointers; a.W / a.W2 stay the bf16 fragments of tile rows that fall back
    hipLaunchKernelGGL(k, p.grid, dim3(p.form.wpb * 64), 0, s, a.w13 ? (const u32x4*)a.w13 : a.W, a.w13 ? (const u32x4*)a.w13_2 : a.W2, a.X, a.Y, a.nw,
                       a.T, a.N, a.K, a.ldx, a.ldy, a);
    return vv_launch_rc(0);
}

// tests: the named W13 form (mr, wpb) on this launch, streaming the twins (a.w13) or, without them, the bf16 fragments: the two
// instantiations that must agree bit for bit, whatever form the plan would give the shape
extern "C" int vv_gemv_w13_form_launch(VVGemm a, int mr, int wpb, hipStream_t s) {
    if (a.epi == VV_EPI_SWIGLU && (!a.W2 || (a.w13 && !a.w13_2))) return -1;
    const int wi = vv_gemv_w13_find(a.pro, a.epi, mr, wpb);
    if (wi < 0 || !vv_gemv_eligible(&a) || !vv_gemv_w13_shape(&a, 1) || a.T > mr) return VV_RC_NO_FORM;
    const GemvKernel k = gemv_w13_kernels[wi][a.w13 ? (a.w13_exact ? 1 : 2) : 0];
    hipLaunchKernelGGL(k, dim3(a.N / 16, 1), dim3(wpb * 64), 0, s, a.w13 ? (const u32x4*)a.w13 : a.W, a.w13 ? (const u32x4*)a.w13_2 : a.W2, a.X, a.Y, a.nw,
                       a.T, a.N, a.K, a.ldx, a.ldy, a);
    return vv_launch_rc(0);
}
