// noise.hip -- the normals of seeded requests (vibevoice_amd/noise.py is the definition): Philox4x32-10 keyed by the request's seed,
// counter (quad, t, stream id, aux), Box-Muller on the four output words.
//
// One thread per Philox block: four normals, one 16-byte store.  The row (= the key) and the stream id are workgroup-uniform
// (blockIdx.y / .z), the keys travel by value in the kernel arguments (16 x 16 B); the kernel reads no global memory, uses no LDS and
// keeps no state: out[s][r][f][j] depends on (keys[r], stream0 + s, f, j) alone, whatever else the launch computes beside it.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int NZ_THREADS = 256;

struct VVNoiseKey { uint32_t seed_lo, seed_hi, t0, aux; };      // vv_noise_key (include/vvhip.h)
struct VVNoiseKeys { VVNoiseKey k[16]; };

__device__ __forceinline__ void nz_philox(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// ((x >> 9) + 0.5) * 2^-23: 24 significant bits, exact
__device__ __forceinline__ float nz_u(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

__device__ __forceinline__ void nz_pair(uint32_t xa, uint32_t xb, float& za, float& zb) {
    const float r = sqrtf(-2.0f * logf(nz_u(xa)));
    float s, c;
    sincospif(2.0f * nz_u(xb), &s, &c);
    za = r * c;
    zb = r * s;
}

__global__ __launch_bounds__(NZ_THREADS) void vv_noise_rows_kernel(float* __restrict__ out, VVNoiseKeys keys, uint32_t stream0, int n_t,
                                                                   int quads) {
    const int idx = blockIdx.x * NZ_THREADS + threadIdx.x;      // (frame, quad) of this row
    const int per = n_t * quads;
    if (idx >= per) return;
    const int row = blockIdx.y, s = blockIdx.z;
    const VVNoiseKey k = keys.k[row];                            // uniform index into the kernel arguments
    const int f = idx / quads, q = idx - f * quads;
    uint32_t c0 = (uint32_t)q, c1 = k.t0 + (uint32_t)f, c2 = stream0 + (uint32_t)s, c3 = k.aux;
    nz_philox(c0, c1, c2, c3, k.seed_lo, k.seed_hi);
    float4 z;
    nz_pair(c0, c1, z.x, z.y);
    nz_pair(c2, c3, z.z, z.w);
    const int64_t at = ((int64_t)s * gridDim.y + row) * per + idx;
    reinterpret_cast<float4*>(out)[at] = z;
}

}  // namespace

// keys: n x {seed_lo, seed_hi, t0, aux} in host memory.  The caller has checked 1 <= n <= 16, n_t >= 1, 1 <= n_streams <= 65,
// width % 4 == 0, n_streams * n * n_t * width < 2^31 and that out is 16-byte aligned; checked again here: -1, nothing launched.
extern "C" int vv_noise_rows_launch(float* out, int n, const uint32_t* keys, uint32_t stream0, int n_streams, int n_t, int width,
                                    hipStream_t s) {
    if (!out || !keys || n < 1 || n > 16 || n_t < 1 || n_streams < 1 || n_streams > 65 || width < 4 || (width & 3)) return -1;
    if (((uintptr_t)out & 15u) != 0) return -1;
    if ((int64_t)n_streams * n * n_t * width >= ((int64_t)1 << 31)) return -1;
    VVNoiseKeys kk;
    for (int i = 0; i < 16; ++i) {
        const int j = i < n ? i : 0;
        kk.k[i].seed_lo = keys[4 * j + 0];
        kk.k[i].seed_hi = keys[4 * j + 1];
        kk.k[i].t0 = keys[4 * j + 2];
        kk.k[i].aux = keys[4 * j + 3];
    }
    const int quads = width / 4;
    const int64_t per = (int64_t)n_t * quads;
    const int64_t gx = (per + NZ_THREADS - 1) / NZ_THREADS;
    if (gx > 0x7fffffff) return -1;
    hipLaunchKernelGGL(vv_noise_rows_kernel, dim3((unsigned)gx, n, n_streams), dim3(NZ_THREADS), 0, s, out, kk, stream0, n_t, quads);
    return vv_launch_rc(0);
}
