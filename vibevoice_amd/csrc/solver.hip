// solver.hip -- the end of a solver step on the general path (the reference scheduler's other DPM-Solver++ settings: orders 1..3,
// midpoint / Heun, the three timestep spacings, sigma_min endings; vibevoice_amd/schedule.py: make_general_table).
//
// The step's final layer has stored eps [2n][L] plainly (conditional rows, then the negative ones).  One table row
// {a, s, cs, c0, c1, c2, cn, 0} then gives
//
//   v   = eps_u + cfg (eps_c - eps_u)
//   x0  = a z - s v                                                  (v-prediction, schedule/dpm_solver.py:581-584)
//   z'  = cs z + c0 x0 + c1 (x0 - m1) + c2 (m1 - m2) + cn noise      (m1, m2: the two previous x0; :669-686, 738-800, 861-893)
//
// and, on every step but the last, the NEXT step's in-projection xh'[t][f] = sum_j Win[f][j] z'[t][j] (noisy_images_proj,
// modular_vibevoice_diffusion_head.py:254-262): every workgroup recomputes the at most 8 x 64 update from the read-only state of
// generation g (2.5 KB of loads, L2-resident after the first workgroup) and multiplies its own 4 sixteen-feature tiles of W_in with
// it; workgroup 0 alone stores generation g ^ 1 (z' on both CFG halves, m1' = x0, m2' = m1).  No workgroup reads what another writes
// in the same launch: the caller double-buffers z / m1 / m2 / xh, as the seam of headtail.hip does.  The in-projection's operand is
// quantised as vv_gemm_launch quantises it: XS bf16 terms per element (vv_split_bf16), fp32 accumulation, bf16 weights.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int SV_WAVES = 4;            // waves per workgroup = in-projection feature tiles per workgroup
constexpr int SV_L = 64;               // latent width of the fused form (2 k-tiles)

// XS = 0: the update alone (one workgroup)
template <int XS>
__global__ __launch_bounds__(SV_WAVES * 64) void vv_solver_step_kernel(const VVSolverStep a) {
    constexpr int XT = XS > 0 ? XS : 1;
    __shared__ __attribute__((aligned(16))) unsigned char zfr[XT * 2 * 1024];      // z' as B fragments: [term][k-tile][lane][8] bf16
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int frow = lane & 15, fq = lane >> 4;
    const int n = a.n, L = a.L;
    // this wave's W_in tile: requested first, consumed last
    const int tile = blockIdx.x * SV_WAVES + wave;
    const bool has_in = XS > 0 && tile * 16 < a.H;
    u32x4 win[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
    if constexpr (XS > 0) {
        if (has_in) {
            win[0] = a.Win[((size_t)tile * 2 + 0) * 64 + lane];
            win[1] = a.Win[((size_t)tile * 2 + 1) * 64 + lane];
        }
    }
    // ---- the update: thread g owns 4 consecutive latents of one utterance row ----
    const int g = threadIdx.x;
    if (g * 4 < n * L) {
        const int r = (g * 4) / L, d0 = (g * 4) % L;
        const unsigned zi = (unsigned)(r * L + d0);
        const float4 ec = *reinterpret_cast<const float4*>(a.eps + zi);
        const float4 eu = *reinterpret_cast<const float4*>(a.eps + (unsigned)(n * L) + zi);
        const float4 z4 = *reinterpret_cast<const float4*>(a.z_in + zi);
        const float4 p1 = *reinterpret_cast<const float4*>(a.m1_in + zi);
        const float4 p2 = *reinterpret_cast<const float4*>(a.m2_in + zi);
        float4 nz = {0.f, 0.f, 0.f, 0.f};
        if (a.noise) nz = *reinterpret_cast<const float4*>(a.noise + zi);
        const float cfg = a.cfg_rows ? a.cfg_rows[r] : a.cfg;
        const float ca = a.coef[0], cs_ = a.coef[1], csx = a.coef[2], c0 = a.coef[3], c1 = a.coef[4], c2 = a.coef[5], cn = a.coef[6];
        float x0[4], zn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float vc = reinterpret_cast<const float*>(&ec)[j], vu = reinterpret_cast<const float*>(&eu)[j];
            const float zo = reinterpret_cast<const float*>(&z4)[j];
            const float m1 = reinterpret_cast<const float*>(&p1)[j], m2 = reinterpret_cast<const float*>(&p2)[j];
            const float v = vu + cfg * (vc - vu);
            x0[j] = ca * zo - cs_ * v;
            float zz = csx * zo + c0 * x0[j];
            // a zero coefficient skips its term: the history rows of the first steps hold whatever the last frame left
            if (c1 != 0.f) zz += c1 * (x0[j] - m1);
            if (c2 != 0.f) zz += c2 * (m1 - m2);
            if (a.noise) zz += cn * reinterpret_cast<const float*>(&nz)[j];
            zn[j] = zz;
        }
        if (blockIdx.x == 0) {              // one workgroup publishes the step's state, into the OTHER generation
            const float4 zo4 = {zn[0], zn[1], zn[2], zn[3]};
            *reinterpret_cast<float4*>(a.z_out + zi) = zo4;
            *reinterpret_cast<float4*>(a.z_out + (unsigned)(n * L) + zi) = zo4;
            *reinterpret_cast<float4*>(a.m1_out + zi) = float4{x0[0], x0[1], x0[2], x0[3]};
            *reinterpret_cast<float4*>(a.m2_out + zi) = p1;
        }
        if constexpr (XS > 0) {
            // B fragments of the in-projection: element (k = d, column t) of k-tile d >> 5; both CFG halves (columns r and r + n) carry z'
            uint2 terms[XT];
            vv_split_bf16<XT>(zn, terms);
#pragma unroll
            for (int x = 0; x < XT; ++x) {
                unsigned char* const base = zfr + x * 2048;
                *reinterpret_cast<uint2*>(base + vv_packed_index<int>(d0 >> 5, r, d0) * 2) = terms[x];
                *reinterpret_cast<uint2*>(base + vv_packed_index<int>(d0 >> 5, r + n, d0) * 2) = terms[x];
            }
        }
    }
    if constexpr (XS > 0) {
        __syncthreads();
        if (!has_in) return;
        f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int x = 0; x < XT; ++x) {
                u32x4 f = u32x4{0u, 0u, 0u, 0u};
                if (frow < 2 * n) f = *reinterpret_cast<const u32x4*>(zfr + x * 2048 + ((size_t)kt * 64 + lane) * 16);
                y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(win[kt]), as_bf16x8(f), y, 0, 0, 0);
            }
        if (frow < 2 * n)
            *reinterpret_cast<float4*>(a.Xout + (size_t)frow * a.H + tile * 16 + fq * 4) = float4{y[0], y[1], y[2], y[3]};
    }
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

// the update itself: 1..8 utterances, whole float4 groups, one workgroup's threads cover the n x L update, state double buffered
extern "C" int vv_solver_step_ok(const VVSolverStep* a) {
    if (a->n < 1 || a->n > 8 || a->L < 4 || (a->L & 3) || a->n * a->L > SV_WAVES * 64 * 4) return 0;
    if (!a->eps || !a->z_in || !a->m1_in || !a->m2_in || !a->z_out || !a->m1_out || !a->m2_out || !a->coef) return 0;
    if (a->z_in == a->z_out || a->m1_in == a->m1_out || a->m2_in == a->m2_out) return 0;
    if (!aligned16(a->eps) || !aligned16(a->z_in) || !aligned16(a->m1_in) || !aligned16(a->m2_in) || !aligned16(a->z_out) ||
        !aligned16(a->m1_out) || !aligned16(a->m2_out) || (a->noise && !aligned16(a->noise))) return 0;
    return 1;
}

// The fused in-projection's rule: asked for (Win and Xout given), L = 64 (two k-tiles), H a multiple of 16 (whole feature tiles, whole
// float4 stores) and H >= 256 -- the seam's own lower bound (headtail.hip), so a context takes its fused step ends together and
// narrow heads keep the two-launch form -- and 1..3 operand terms.  Anything else: the update alone.
extern "C" int vv_solver_step_fused_ok(const VVSolverStep* a) {
    return vv_solver_step_ok(a) && a->Win && a->Xout && aligned16(a->Win) && aligned16(a->Xout) && a->L == SV_L && (a->H & 15) == 0 &&
           a->H >= 256 && (int64_t)16 * a->H < (1LL << 30) && a->xs >= 1 && a->xs <= 3;
}

// 1: the fused form ran (the next step's in-projection is in Xout);  0: the update alone;  < 0: refused / launch error
extern "C" int vv_solver_step_launch(const VVSolverStep* ap, hipStream_t s) {
    if (!vv_solver_step_ok(ap)) return VV_RC_NO_FORM;
    const VVSolverStep& a = *ap;
    if (!vv_solver_step_fused_ok(ap)) {
        hipLaunchKernelGGL((vv_solver_step_kernel<0>), dim3(1), dim3(SV_WAVES * 64), 0, s, a);
        return vv_launch_rc(0);
    }
    const dim3 grid((a.H / 16 + SV_WAVES - 1) / SV_WAVES);
    if (a.xs == 1) hipLaunchKernelGGL((vv_solver_step_kernel<1>), grid, dim3(SV_WAVES * 64), 0, s, a);
    else if (a.xs == 2) hipLaunchKernelGGL((vv_solver_step_kernel<2>), grid, dim3(SV_WAVES * 64), 0, s, a);
    else hipLaunchKernelGGL((vv_solver_step_kernel<3>), grid, dim3(SV_WAVES * 64), 0, s, a);
    return vv_launch_rc(1);
}
