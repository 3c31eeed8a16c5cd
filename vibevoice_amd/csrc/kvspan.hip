// kvspan.hip -- a prompt prefix's K/V as data: snapshot of the first n positions of a cache into a compact buffer, its restore into
// another cache (of any max_ctx), and the export of a span back to HF layout (the inverse of vv_kv_import_kernel, misc.hip).
//
// All three are copies: one 16-byte chunk per lane, consecutive lanes on consecutive chunks, no LDS, grids of
// (chunk blocks, kv heads, layers).  A chunk is one `[lane][8]` entry of the cache's tile layouts (attn.hip header):
//   K tile  [pos/16][d/32][lane][8]:  lane = (pos & 15) + 16 * ((d & 31) >> 3), element d & 7      -> one position, 8 channels
//   V block [pos/32][d/16][lane][8]:  lane = (d & 15) + 16 * ((pos & 15) >> 2), element 4 * ((pos & 31) >> 4) + (pos & 3)
//                                                                                                   -> one channel, 8 positions
// Both layouts put positions [0, 32 m) of one (layer, kv head) in the first 32 m * D elements of that head's region, so a span that
// starts at 0 and ends on a 32-position boundary is ONE contiguous run per head whatever max_ctx is: the snapshot buffer is
// [layer][kv head][ceil32(n) * D] bf16 and a restore needs no re-tiling.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

// position of the K chunk `c` of a head's region / first position and stride pattern of the V chunk `c`
__device__ __forceinline__ int kchunk_pos(int c, int D) { return ((c >> 6) / (D >> 5)) * 16 + (c & 15); }
// element j of V chunk c belongs to position vchunk_pos0(c) + 16 * (j >> 2) + (j & 3)
__device__ __forceinline__ int vchunk_pos0(int c, int D) { return ((c >> 6) / (D >> 4)) * 32 + ((c & 63) >> 4) * 4; }

// bf16 elements of a chunk whose position is >= n_pos become +0
__device__ __forceinline__ u32x4 vmask_chunk(u32x4 w, int p0, int n_pos) {
    unsigned r[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int pos = p0 + 16 * (j >> 2) + (j & 3);
        if (pos >= n_pos) r[j >> 1] &= (j & 1) ? 0x0000ffffu : 0xffff0000u;
    }
    u32x4 o; o.x = r[0]; o.y = r[1]; o.z = r[2]; o.w = r[3];
    return o;
}

// TO_CACHE = false: cache -> snapshot; true: snapshot -> cache.  The cache side of head (layer, h) starts at
// layer * layer_stride + h * head_stride elements, the snapshot side at (layer * Hkv + h) * span elements, span = ceil32(n_pos) * D.
// Slots of positions >= n_pos are written as zero in both directions (K: whole chunks, V: per element).
// grid (ceil(span / 8 / 256), Hkv, layers), block 256.
template <bool TO_CACHE>
__global__ __launch_bounds__(256) void vv_kv_span_copy_kernel(__bf16* __restrict__ kc, __bf16* __restrict__ vc, __bf16* __restrict__ ks,
                                                              __bf16* __restrict__ vs, int D, int64_t layer_stride, int64_t head_stride,
                                                              int n_pos) {
    const int span_chunks = ((n_pos + 31) & ~31) * (D >> 3);
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= span_chunks) return;
    const int64_t co = ((int64_t)blockIdx.z * layer_stride + (int64_t)blockIdx.y * head_stride) / 8 + c;
    const int64_t so = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * span_chunks + c;
    u32x4* kcp = reinterpret_cast<u32x4*>(kc) + co;
    u32x4* vcp = reinterpret_cast<u32x4*>(vc) + co;
    u32x4* ksp = reinterpret_cast<u32x4*>(ks) + so;
    u32x4* vsp = reinterpret_cast<u32x4*>(vs) + so;
    u32x4 kw = TO_CACHE ? *ksp : *kcp;
    u32x4 vw = TO_CACHE ? *vsp : *vcp;
    if (kchunk_pos(c, D) >= n_pos) kw = u32x4{0u, 0u, 0u, 0u};
    const int p0 = vchunk_pos0(c, D);
    if (p0 + 20 > n_pos) vw = vmask_chunk(vw, p0, n_pos);      // p0 + 19 is the chunk's last position
    if (TO_CACHE) { *kcp = kw; *vcp = vw; }
    else { *ksp = kw; *vsp = vw; }
}

template <typename OT> __device__ __forceinline__ void store8(OT* dst, const unsigned short (&e)[8]);
template <> __device__ __forceinline__ void store8<__bf16>(__bf16* dst, const unsigned short (&e)[8]) {
    u32x4 o;
    o.x = e[0] | ((unsigned)e[1] << 16); o.y = e[2] | ((unsigned)e[3] << 16);
    o.z = e[4] | ((unsigned)e[5] << 16); o.w = e[6] | ((unsigned)e[7] << 16);
    *reinterpret_cast<u32x4*>(dst) = o;
}
template <> __device__ __forceinline__ void store8<float>(float* dst, const unsigned short (&e)[8]) {
    u32x4 a, b;                                     // bf16 -> fp32 is the bit pattern shifted up: exact, NaN payloads included
    a.x = (unsigned)e[0] << 16; a.y = (unsigned)e[1] << 16; a.z = (unsigned)e[2] << 16; a.w = (unsigned)e[3] << 16;
    b.x = (unsigned)e[4] << 16; b.y = (unsigned)e[5] << 16; b.z = (unsigned)e[6] << 16; b.w = (unsigned)e[7] << 16;
    reinterpret_cast<u32x4*>(dst)[0] = a;
    reinterpret_cast<u32x4*>(dst)[1] = b;
}

// tiled cache layout -> HF layout [kvh][L][D], one layer, positions [pos0, pos0 + L): the inverse of vv_kv_import_kernel.  A lane
// owns 8 consecutive channels of one position: the K side is one 16-byte chunk of the cache, the V side gathers its 8 elements
// from 8 neighbouring chunks (V keeps positions, not channels, together); both sides store 16 (bf16) or 32 (fp32) contiguous bytes.
// grid (ceil(L * D / 8 / 256), kvh), block 256.
template <typename OT>
__global__ __launch_bounds__(256) void vv_kv_export_kernel(const __bf16* __restrict__ kc, const __bf16* __restrict__ vc, OT* __restrict__ k,
                                                           OT* __restrict__ v, int L, int D, int64_t head_stride, int pos0) {
    const int g = blockIdx.x * 256 + threadIdx.x;            // (row i, channel group d8)
    const int dg = D >> 3;
    if (g >= L * dg) return;
    const int i = g / dg, d = (g - i * dg) * 8;
    const int h = blockIdx.y, pos = pos0 + i;
    const unsigned short* kb = reinterpret_cast<const unsigned short*>(kc) + (int64_t)h * head_stride;
    const unsigned short* vb = reinterpret_cast<const unsigned short*>(vc) + (int64_t)h * head_stride;
    const int64_t oi = ((int64_t)h * L + i) * D + d;
    unsigned short e[8];
    {
        const int64_t tile = (int64_t)(pos >> 4) * (D / 32) + (d >> 5);
        const int ln = (pos & 15) + 16 * ((d & 31) >> 3);
        const u32x4 w = *reinterpret_cast<const u32x4*>(kb + (tile * 64 + ln) * 8);
        e[0] = w.x & 0xffffu; e[1] = w.x >> 16; e[2] = w.y & 0xffffu; e[3] = w.y >> 16;
        e[4] = w.z & 0xffffu; e[5] = w.z >> 16; e[6] = w.w & 0xffffu; e[7] = w.w >> 16;
        store8<OT>(k + oi, e);
    }
    {
        const int p = pos & 31, half = p >> 4, pp = p & 15, q4 = pp >> 2, rr = pp & 3;
        const int64_t tile = (int64_t)(pos >> 5) * (D / 16) + (d >> 4);
        const int ln = (d & 15) + 16 * q4;                   // d & 15 is 0 or 8: the 8 channels stay inside one 16-lane group
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = vb[(tile * 64 + ln + j) * 8 + half * 4 + rr];
        store8<OT>(v + oi, e);
    }
}

}  // namespace

extern "C" {

// kc / vc: the cache's first layer; ks / vs: the snapshot buffers.  to_cache = 0 snapshot, 1 restore.
int vv_kv_span_copy_launch(void* kc, void* vc, void* ks, void* vs, int to_cache, int layers, int Hkv, int D, int64_t layer_stride,
                           int64_t head_stride, int n_pos, hipStream_t s) {
    if ((D & 31) || n_pos < 1 || (head_stride & 7) || (layer_stride & 7)) return -1;
    const int span_chunks = ((n_pos + 31) & ~31) * (D >> 3);
    const dim3 grid((span_chunks + 255) / 256, Hkv, layers);
    if (to_cache) hipLaunchKernelGGL((vv_kv_span_copy_kernel<true>), grid, dim3(256), 0, s, (__bf16*)kc, (__bf16*)vc, (__bf16*)ks, (__bf16*)vs, D, layer_stride, head_stride, n_pos);
    else hipLaunchKernelGGL((vv_kv_span_copy_kernel<false>), grid, dim3(256), 0, s, (__bf16*)kc, (__bf16*)vc, (__bf16*)ks, (__bf16*)vs, D, layer_stride, head_stride, n_pos);
    return vv_launch_rc(0);
}
// kc / vc: the layer's region of the cache; k / v: HF layout [Hkv][L][D] in fp32 (dst_bf16 = 0) or bf16
int vv_kv_export_launch(const void* kc, const void* vc, void* k, void* v, int dst_bf16, int L, int Hkv, int D, int64_t head_stride, int pos0,
                        hipStream_t s) {
    if ((D & 31) || L < 1) return -1;
    const dim3 grid((L * (D >> 3) + 255) / 256, Hkv);
    if (dst_bf16) hipLaunchKernelGGL((vv_kv_export_kernel<__bf16>), grid, dim3(256), 0, s, (const __bf16*)kc, (const __bf16*)vc, (__bf16*)k, (__bf16*)v, L, D, head_stride, pos0);
    else hipLaunchKernelGGL((vv_kv_export_kernel<float>), grid, dim3(256), 0, s, (const __bf16*)kc, (const __bf16*)vc, (float*)k, (float*)v, L, D, head_stride, pos0);
    return vv_launch_rc(0);
}

}  // extern "C"
