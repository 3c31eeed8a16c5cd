// vv_device.h -- the device arithmetic every kernel file shares (gfx950 only): wave reductions, the 16-bit PCM rule, activations, the fp32 -> bf16
// term split, the packed-tile element index and the sampler's guidance + solver update.  Include it after vv_common.h.
// Everything here is __device__ __forceinline__: a kernel compiles to the same instructions as with the expression written out.
#pragma once
#include "vv_common.h"

// ---- wave reductions -----------------------------------------------------------
// full-wave sum by an xor butterfly: every lane gets the sum
template <class T>
__device__ __forceinline__ T vv_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// full-wave sum, result uniform (returned from SGPRs): 4 DPP steps inside each row of 16 + 4 readlanes (no LDS permutes).
// NOT the same rounding order as vv_wave_sum: a call site keeps the one it has.
__device__ __forceinline__ float vv_wave_sum_dpp(float v) {
    int x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true));  // row_half_mirror
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true));  // row_mirror
    x = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 48));
    return (r0 + r1) + (r2 + r3);
}

// ---- 16-bit PCM of one chunk per workgroup ------------------------------------------
// The arithmetic of the reference's convert_to_16_bit_wav (demo/gradio_demo.py:1058-1073): peak = max|x| over the chunk; where
// peak > 1, x / peak (fp32, IEEE division); (x * 32767) truncated toward zero.  vv_block_peak: the largest of the threads' own maxima
// (each >= 0) in a workgroup of WAVES full waves, through wmx, WAVES words of the caller's LDS; one barrier, every thread gets the peak.
// fmaxf is exact, so the order of the reduction is free; the division, the product and the truncation below are the rule.
template <int WAVES>
__device__ __forceinline__ float vv_block_peak(float mx, float* wmx) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = mx;
    __syncthreads();
    float peak = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) peak = fmaxf(peak, wmx[w]);
    return peak;
}
__device__ __forceinline__ short vv_pcm16_of(float v, float peak) {
    if (peak > 1.0f) v = __fdiv_rn(v, peak);
    return (short)(int)__fmul_rn(v, 32767.0f);
}

// ---- activations ---------------------------------------------------------------
// SiLU in two precisions that do NOT give the same bits: vv_silu uses the accurate expf, vv_silu_fast the hardware __expf
// (prefill GEMM epilogues only).  Moving a call from one to the other changes results.
__device__ __forceinline__ float vv_silu(float u) { return u / (1.0f + expf(-u)); }
__device__ __forceinline__ float vv_silu_fast(float u) { return u / (1.0f + __expf(-u)); }
// exact (erf) GELU
__device__ __forceinline__ float vv_gelu_erf(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752440f)); }

// ---- fp32 -> bf16 terms ----------------------------------------------------------
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 u) { return __builtin_bit_cast(bf16x8, u); }

// 4 fp32 -> XS packed bf16x4 terms (8 bytes each): hi [, mid = bf16(v - hi) [, lo = bf16((v - hi) - mid)]]
template <int XS>
__device__ __forceinline__ void vv_split_bf16(const float (&v)[4], uint2 (&out)[XS]) {
    bf16x4 h, m, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[j] = (__bf16)v[j];
        if constexpr (XS > 1) {
            const float r = v[j] - (float)h[j];
            m[j] = (__bf16)r;
            if constexpr (XS > 2) l[j] = (__bf16)(r - (float)m[j]);
        }
    }
    out[0] = __builtin_bit_cast(uint2, h);
    if constexpr (XS > 1) out[1] = __builtin_bit_cast(uint2, m);
    if constexpr (XS > 2) out[2] = __builtin_bit_cast(uint2, l);
}

// ---- packed 16 x 32 tile (layout: vv_common.h, "packed weight tile") ---------------
// Index, in bf16 elements, of element (r16, k) of tile number `tile`: lane r16 + 16 * ((k & 31) >> 3), slot k & 7, where r16 is
// the row INSIDE the tile (row & 15).  The caller numbers the tiles ([row / 16][k / 32] for weights, activations and the K
// cache) and picks the index type I with it: a 32-bit tile number keeps 32-bit address arithmetic, an int64_t one 64-bit.
// Sites that form the lane as an int of its own first, or a byte offset, associate the sum differently and keep their text.
template <class I>
__device__ __forceinline__ I vv_packed_index(I tile, int r16, int k) {
    return (tile * 64 + r16 + 16 * ((k & 31) >> 3)) * 8 + (k & 7);
}

// ---- classifier-free guidance + one DPM-Solver++(2M) update of ONE latent element ---
//   v  = v_u + cfg (v_c - v_u)                      (v_c / v_u: the conditional / unconditional prediction)
//   x0 = a z - s v
//   z' = cs z + c0 x0 + c1 (x0 - x0_prev)           (c1 = 0 on first-order steps)
//   z' += cn noise                                  (sde-dpmsolver++ only: dpm_solver.py:680-686, 785-793)
// One row {a, s, cs, c0, c1, cn} of the schedule table per solver step.  How a row finds its unconditional partner, where the
// state lives and who stores x0 / z' differ between the kernels and stay with them.  The expression tree is the contract: the
// compiler forms its FMAs from this shape, and every copy of the update must round the same way.  `noise` is a callable that
// returns this element's noise: it is only evaluated under `sde`, so a null noise tensor is never read and the load stays
// inside the branch (fetched ahead of the arithmetic, the compiler pairs and fuses the products differently).
struct VVSolverCoef { float a, s, cs, c0, c1, cn; };
__device__ __forceinline__ VVSolverCoef vv_solver_coef(const float* row, bool sde) {
    return VVSolverCoef{row[0], row[1], row[2], row[3], row[4], sde ? row[5] : 0.f};
}
template <class Noise>
__device__ __forceinline__ void vv_cfg_dpm_update(float vc, float vu, float cfg, float z, float x0_prev, const VVSolverCoef& c,
                                                  bool sde, Noise&& noise, float& x0, float& zn) {
    const float v = vu + cfg * (vc - vu);
    x0 = c.a * z - c.s * v;
    zn = c.cs * z + c.c0 * x0 + c.c1 * (x0 - x0_prev);
    if (sde) zn += c.cn * noise();
}
