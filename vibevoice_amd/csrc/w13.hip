// w13.hip -- W13 twins of packed bf16 matrices (vv_w13.h): the pack kernel with its own device round trip, the fold of its per-tile
// ok words, and the expansion back to fragments (tests).  The decoder is vv_w13_unpack of the header, the one the GEMV runs.
#include "vv_common.h"
#include "vv_w13.h"
#include "vv_launch.h"

namespace {

constexpr int PACK_WAVES = 4;

// One workgroup per 16-feature tile row: Emax over the row, then wave w packs groups w, w + 4, ...; every packed group is decoded
// again with vv_w13_unpack and compared with the source bit for bit -- the answer is ok[tile], whatever the host thinks of the rule.
__global__ __launch_bounds__(PACK_WAVES * 64) void vv_w13_pack_kernel(const u32x4* __restrict__ W, unsigned char* __restrict__ out, int n_tiles, int k_tiles, int tile0) {
    __shared__ unsigned red[PACK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tile = blockIdx.x + tile0;      // the launch covers the tile rows tile0 .. tile0 + gridDim.x - 1 of the matrix
    const int groups = k_tiles >> 2;
    const u32x4* src = W + (size_t)tile * k_tiles * 64;
    unsigned emax = 0;
    for (int i = threadIdx.x; i < k_tiles * 64; i += PACK_WAVES * 64) {
        const u32x4 v = src[i];
#pragma unroll
        for (int d = 0; d < 4; ++d) emax = max(emax, max((v[d] >> 7) & 0xffu, (v[d] >> 23) & 0xffu));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) emax = max(emax, (unsigned)__shfl_xor((int)emax, o));
    if (lane == 0) red[wave] = emax;
    __syncthreads();
    emax = red[0];
#pragma unroll
    for (int w = 1; w < PACK_WAVES; ++w) emax = max(emax, red[w]);
    __syncthreads();
    const float scale = vv_w13_scale(emax);
    unsigned char* planes = out + (size_t)tile * groups * VV_W13_GROUP;
    unsigned ok = 1;
    for (int g = wave; g < groups; g += PACK_WAVES) {
        u32x4 f[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) f[t] = src[(g * 4 + t) * 64 + lane];
        unsigned hi[8] = {0, 0, 0, 0, 0, 0, 0, 0}, lo[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {          // the output pair j: elements 2j, 2j + 1 of the lane's 32
            const unsigned pair = f[j >> 2][j & 3];
            unsigned x = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned b = (pair >> (16 * h)) & 0xffffu, s = b >> 15, E = (b >> 7) & 0xffu, m = b & 0x7fu;
                const bool zero = (b & 0x7fffu) == 0;
                const bool rep = zero || (E >= 1 && E + 29 >= emax && emax <= 254);
                const unsigned c = (rep && !zero) ? E + 30 - emax : 0u;
                const unsigned hb = (s << 7) | (c << 2) | ((rep && !zero) ? m >> 5 : 0u);
                const unsigned l5 = (rep && !zero) ? m & 31u : 0u;
                hi[j >> 1] |= hb << (8 * (2 * (j & 1) + h));
                x |= l5 << (5 * h);
            }
            const int d = (10 * j) >> 5, s10 = (10 * j) & 31;
            lo[d] |= x << s10;
            if (s10 + 10 > 32) lo[d + 1] |= x >> (32 - s10);
        }
        VVW13Raw r;
        r.h0 = u32x4{hi[0], hi[1], hi[2], hi[3]}; r.h1 = u32x4{hi[4], hi[5], hi[6], hi[7]};
        r.lo = u32x4{lo[0], lo[1], lo[2], lo[3]}; r.l4 = lo[4];
        vv_w13_store(planes + (size_t)g * VV_W13_GROUP, lane, r);
        u32x4 back[4];
        vv_w13_unpack(r, scale, back);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int d = 0; d < 4; ++d) if (back[t][d] != f[t][d]) ok = 0;
    }
    ok = __all((int)ok) ? 1u : 0u;
    if (lane == 0) red[wave] = ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned all = 1;
#pragma unroll
        for (int w = 0; w < PACK_WAVES; ++w) all &= red[w];
        unsigned* tail = reinterpret_cast<unsigned*>(out + (size_t)n_tiles * groups * VV_W13_GROUP);
        tail[tile] = emax;
        tail[n_tiles + tile] = all;
    }
}

// ok[n_tiles] -> one word per matrix, the one the host reads
__global__ __launch_bounds__(256) void vv_w13_fold_kernel(unsigned* __restrict__ tail, int n_tiles) {
    __shared__ unsigned red[4];
    unsigned ok = 1;
    for (int i = threadIdx.x; i < n_tiles; i += 256) ok &= tail[n_tiles + i];
    ok = __all((int)ok) ? 1u : 0u;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ok;
    __syncthreads();
    if (threadIdx.x == 0) tail[2 * n_tiles] = red[0] & red[1] & red[2] & red[3];
}

// tests: planes -> packed bf16 fragments
__global__ __launch_bounds__(PACK_WAVES * 64) void vv_w13_unpack_kernel(const unsigned char* __restrict__ in, u32x4* __restrict__ W, int n_tiles, int k_tiles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tile = blockIdx.x;
    const int groups = k_tiles >> 2;
    const unsigned* tail = reinterpret_cast<const unsigned*>(in + (size_t)n_tiles * groups * VV_W13_GROUP);
    const float scale = vv_w13_scale(tail[tile]);
    const unsigned char* planes = in + (size_t)tile * groups * VV_W13_GROUP;
    u32x4* dst = W + (size_t)tile * k_tiles * 64;
    for (int g = wave; g < groups; g += PACK_WAVES) {
        const VVW13Raw r = vv_w13_load(planes + (size_t)g * VV_W13_GROUP, lane);
        u32x4 f[4];
        vv_w13_unpack(r, scale, f);
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[(g * 4 + t) * 64 + lane] = f[t];
    }
}

}  // namespace

// packed: the matrix's bf16 fragments (vv_pack_launch's output); twin: vv_w13_bytes(N, K) bytes.  The folded ok word is the twin's last
// word but three: vv_w13_ok_offset
// tile0, tiles: the tile rows to pack (a parameter that is one part of the matrix: q, k or v of a QKV matrix); the fold covers all rows
extern "C" int vv_w13_pack_rows_launch(const void* packed, void* twin, int N, int K, int tile0, int tiles, hipStream_t s) {
    if (!vv_w13_shape_ok(N, K) || tile0 < 0 || tiles < 1 || tile0 + tiles > N / 16) return VV_RC_NO_FORM;
    const int n_tiles = N / 16, k_tiles = K / 32;
    hipLaunchKernelGGL(vv_w13_pack_kernel, dim3(tiles), dim3(PACK_WAVES * 64), 0, s, (const u32x4*)packed, (unsigned char*)twin, n_tiles, k_tiles, tile0);
    hipLaunchKernelGGL(vv_w13_fold_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned*>((unsigned char*)twin + vv_w13_plane_bytes(N, K)), n_tiles);
    return vv_launch_rc(0);
}
extern "C" int vv_w13_pack_launch(const void* packed, void* twin, int N, int K, hipStream_t s) {
    return vv_w13_pack_rows_launch(packed, twin, N, K, 0, N / 16, s);
}
extern "C" int vv_w13_unpack_launch(const void* twin, void* packed, int N, int K, hipStream_t s) {
    if (!vv_w13_shape_ok(N, K)) return VV_RC_NO_FORM;
    const int n_tiles = N / 16, k_tiles = K / 32;
    hipLaunchKernelGGL(vv_w13_unpack_kernel, dim3(n_tiles), dim3(PACK_WAVES * 64), 0, s, (const unsigned char*)twin, (u32x4*)packed, n_tiles, k_tiles);
    return vv_launch_rc(0);
}
