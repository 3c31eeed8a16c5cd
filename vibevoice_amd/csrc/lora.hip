// lora.hip -- device-resident LoRA adapters (gfx950): a rank-r update of a packed bf16 matrix in the MFMA tile layout, in place,
// and the inverse of the weight pack.
//
//   vv_lora_merge_kernel   dst_packed = bf16(base_packed + scale * B.A), one streaming pass over the tiles vv_pack_launch wrote
//                          ([(N+15)/16][(K+31)/32][512], element index vv_packed_index): 2 bytes read + 2 written per element.
//   vv_unpack_kernel       packed bf16 of a linear [N][K] matrix -> row-major fp32 (exact).
//
// The merge's arithmetic is a contract (the tests hold it to lora.merge_lora on the CPU bit for bit on exactly representable
// inputs, and to the fp64 result within one bf16 step otherwise):
//   d = 0; for j = 0 .. r-1 ascending: d = fmaf(b[n][j], a[j][k], d)
//   fp32-delta mode:  delta = scale * d (one rounding);                 w' = bf16(f32(base) + delta)          (a second rounding)
//   bf16-delta mode:  a, b rounded to bf16 as they are staged;  delta = bf16(scale * d);  w' = bf16(f32(base) + f32(delta))
// The multiply by scale and the add onto the base are NOT contracted into one FMA (the host path rounds twice), and nothing is
// accumulated through MFMA: its internal summation order is not ours to fix.
//
// Shape: a workgroup of 4 waves owns a k-span of 4 k-tiles (one per wave) and up to 8 n-tiles.  Per chunk of 64 ranks the a
// columns of the k-span ([64][128] fp32) and the b rows of the n-tiles ([64][128 rows], transposed, xor-swizzled) are staged in
// LDS once: 64 KiB static, no attribute call.  A wave keeps the 8 tiles' accumulators in registers across the chunks, so the j
// order stays ascending for every r; one a fragment read from LDS feeds 8 tiles.  Each lane loads its 16-byte fragment of every
// tile before the first chunk (the loads fly under the arithmetic) and stores it once: dst == base is allowed.  Offsets are
// 32-bit from uniform bases (the launcher refuses matrices whose packed size or factor sizes pass 2^31).
#include <algorithm>
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

constexpr int LORA_JC = 64;        // ranks per LDS chunk
constexpr int LORA_KS = 128;       // k-span of a workgroup: 4 waves x one 32-wide k-tile
constexpr int LORA_NT = 8;         // n-tiles of a workgroup (accumulators held in registers)

template <bool BF>
__global__ __launch_bounds__(256) void vv_lora_merge_kernel(const u32x4* base, u32x4* dst, const float* __restrict__ a,
                                                            const float* __restrict__ b, int N, int K, int r, float scale, int ntw) {
    __shared__ __attribute__((aligned(16))) float a_s[LORA_JC * LORA_KS];
    __shared__ __attribute__((aligned(16))) float b_s[LORA_JC * LORA_NT * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k_tiles = (K + 31) >> 5, n_tiles = (N + 15) >> 4;
    const int kb = blockIdx.x * LORA_KS;
    const int kt = blockIdx.x * 4 + wave;
    const int nt0 = blockIdx.y * ntw;
    const bool kt_ok = kt < k_tiles;
    const int n16 = lane & 15, kq = (lane >> 4) * 8;

    u32x4 w[LORA_NT];
    float acc[LORA_NT][8];
#pragma unroll
    for (int t = 0; t < LORA_NT; ++t) {
        w[t] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[t][i] = 0.f;
        if (t < ntw && nt0 + t < n_tiles && kt_ok) w[t] = base[((unsigned)(nt0 + t) * k_tiles + kt) * 64u + lane];
    }

    for (int jc = 0; jc < r; jc += LORA_JC) {
        const int rc = min(LORA_JC, r - jc);
        if (jc) __syncthreads();
        // both factors go through registers 8 loads at a time: the loads of a batch are in flight together
        for (int i0 = tid; i0 < rc * LORA_KS; i0 += 8 * 256) {          // a[jc + j][kb + kk], zero past K
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256, k = kb + (i & (LORA_KS - 1));
                v[u] = (i < rc * LORA_KS && k < K) ? a[(unsigned)(jc + (i >> 7)) * K + k] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256;
                if constexpr (BF) v[u] = (float)(__bf16)v[u];
                if (i < rc * LORA_KS) a_s[i] = v[u];
            }
        }
        const int nb = ntw * 16 * rc;
        for (int i0 = tid; i0 < nb; i0 += 8 * 256) {                     // b[nt0 * 16 + row][jc + j] -> [j][row ^ (j & 31)], zero past N
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256, row = i / rc, n = nt0 * 16 + row;
                v[u] = (i < nb && n < N) ? b[(unsigned)n * r + jc + (i - row * rc)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256, row = i / rc, j = i - row * rc;
                if constexpr (BF) v[u] = (float)(__bf16)v[u];
                if (i < nb) b_s[j * (LORA_NT * 16) + (row ^ (j & 31))] = v[u];
            }
        }
        __syncthreads();
        if (kt_ok) {
            // the operands of rank j + 1 are read from LDS while rank j is accumulated (two waves per SIMD hide little latency)
            const float* ap = &a_s[wave * 32 + kq];
            f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
            float bv[LORA_NT];
#pragma unroll
            for (int t = 0; t < LORA_NT; ++t) bv[t] = b_s[t * 16 + n16];
            for (int j = 0; j < rc; ++j) {
                const f32x4 c0 = a0, c1 = a1;
                float cb[LORA_NT];
#pragma unroll
                for (int t = 0; t < LORA_NT; ++t) cb[t] = bv[t];
                const int jn = min(j + 1, rc - 1);
                a0 = *reinterpret_cast<const f32x4*>(ap + jn * LORA_KS);
                a1 = *reinterpret_cast<const f32x4*>(ap + jn * LORA_KS + 4);
#pragma unroll
                for (int t = 0; t < LORA_NT; ++t) bv[t] = b_s[jn * (LORA_NT * 16) + ((t * 16 + n16) ^ (jn & 31))];
#pragma unroll
                for (int t = 0; t < LORA_NT; ++t) {
                    if (t < ntw) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[t][i] = __builtin_fmaf(cb[t], c0[i], acc[t][i]);
                            acc[t][4 + i] = __builtin_fmaf(cb[t], c1[i], acc[t][4 + i]);
                        }
                    }
                }
            }
        }
    }

    if (!kt_ok) return;
#pragma unroll
    for (int t = 0; t < LORA_NT; ++t) {
        if (t < ntw && nt0 + t < n_tiles) {
#pragma clang fp contract(off)
            const bf16x8 wb = as_bf16x8(w[t]);
            const u16x8 keep = __builtin_bit_cast(u16x8, w[t]);
            const bool row_ok = (nt0 + t) * 16 + n16 < N;
            u16x8 out;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float delta = scale * acc[t][i];
                if constexpr (BF) delta = (float)(__bf16)delta;
                const float s = (float)wb[i] + delta;
                const __bf16 o = (__bf16)s;
                // padding of the edge tiles (row >= N, k >= K) is copied from the base unchanged
                out[i] = (row_ok && kt * 32 + kq + i < K) ? __builtin_bit_cast(unsigned short, o) : keep[i];
            }
            dst[((unsigned)(nt0 + t) * k_tiles + kt) * 64u + lane] = __builtin_bit_cast(u32x4, out);
        }
    }
}

// one thread per 16-byte fragment: 8 consecutive k of one row
__global__ __launch_bounds__(256) void vv_unpack_kernel(const u32x4* __restrict__ src, float* __restrict__ dst, int N, int K) {
    const int k_tiles = (K + 31) >> 5;
    const unsigned total = (unsigned)((N + 15) >> 4) * k_tiles * 64u;
    for (unsigned f = blockIdx.x * 256u + threadIdx.x; f < total; f += gridDim.x * 256u) {
        const unsigned tile = f >> 6;
        const int lane = f & 63;
        const int n = (int)(tile / k_tiles) * 16 + (lane & 15);
        const int k0 = (int)(tile % k_tiles) * 32 + (lane >> 4) * 8;
        if (n >= N || k0 >= K) continue;
        const bf16x8 v = as_bf16x8(src[f]);
        float* o = dst + (int64_t)n * K + k0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (k0 + i < K) o[i] = (float)v[i];
    }
}

}  // namespace

extern "C" int vv_lora_merge_launch(const void* base, void* dst, int N, int K, const float* a, const float* b, int r, float scale,
                                    int delta_bf16, hipStream_t s) {
    const int n_tiles = (N + 15) / 16, k_tiles = (K + 31) / 32;
    const int kch = (k_tiles + 3) / 4;
    // enough workgroups for every CU (two resident per CU at 64 KiB of LDS each) before a workgroup takes more n-tiles
    int ntw = (int)std::min<int64_t>(LORA_NT, std::max<int64_t>(1, (int64_t)n_tiles * kch / 512));
    const dim3 grid(kch, (n_tiles + ntw - 1) / ntw);
    if (delta_bf16)
        hipLaunchKernelGGL((vv_lora_merge_kernel<true>), grid, dim3(256), 0, s, (const u32x4*)base, (u32x4*)dst, a, b, N, K, r, scale, ntw);
    else
        hipLaunchKernelGGL((vv_lora_merge_kernel<false>), grid, dim3(256), 0, s, (const u32x4*)base, (u32x4*)dst, a, b, N, K, r, scale, ntw);
    return vv_launch_rc(0);
}

extern "C" int vv_unpack_launch(const void* packed, float* dst, int N, int K, hipStream_t s) {
    const int64_t frags = vv_packed_elems(N, K) / 8;
    const unsigned blocks = (unsigned)std::min<int64_t>((frags + 255) / 256, 8192);
    hipLaunchKernelGGL(vv_unpack_kernel, dim3(blocks), dim3(256), 0, s, (const u32x4*)packed, dst, N, K);
    return vv_launch_rc(0);
}
