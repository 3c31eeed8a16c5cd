// vv_w13.h -- "W13": a lossless 13-bit storage of packed bf16 weight tiles (definition by bits: vibevoice_amd/w13.py).
//
// Per 16-feature x K tile row, Emax = the largest bf16 exponent field.  An element is representable if it is +-0, or if its exponent
// field E has Emax - 29 <= E <= Emax (Emax <= 254).  Its code c = E - Emax + 30 (1..30; 0 = zero) is the exponent field of an e5m2
// byte, so the high byte  sign | c | mantissa[6:5]  decodes with v_cvt_scalef32_pk_bf16_bf8 and the scale 2^(Emax - 142); the low
// field mantissa[4:0] is or-ed under it.
//
// Layout: the packed fragment order (tile, k-tile, 64 lanes, 8 elements per lane) with k-tiles grouped in fours.  One (tile, group) is
// VV_W13_GROUP contiguous bytes, plane by plane so that every load of a wave is one contiguous run:
//   [0, 1024)     lane * 16: high bytes of the lane's elements  0..15  (k-tiles 0, 1 of the group; element = k-tile * 8 + e)
//   [1024, 2048)  lane * 16: high bytes of elements 16..31            (k-tiles 2, 3)
//   [2048, 3072)  lane * 16: bits 0..127 of the lane's low string
//   [3072, 3328)  lane * 4:  bits 128..159 of it
// The low string holds, for the output pair j = 0..15 (elements 2j, 2j + 1), the 10 bits  lo[2j] | lo[2j + 1] << 5  at bit 10 j.
// A matrix = n_tiles x (K / 128) groups, then n_tiles scale words (Emax), n_tiles ok words, one folded ok word (vv_w13_bytes).
#pragma once
#include "vv_common.h"

constexpr int VV_W13_GROUP = 3328;          // bytes of one (tile, group): 64 lanes x 52 B, where bf16 takes 64 lanes x 64 B
static inline __host__ __device__ bool vv_w13_shape_ok(int N, int K) { return N > 0 && K > 0 && (N & 15) == 0 && (K & 127) == 0; }
static inline __host__ __device__ int64_t vv_w13_plane_bytes(int N, int K) { return (int64_t)(N / 16) * (K / 128) * VV_W13_GROUP; }
static inline __host__ __device__ int64_t vv_w13_bytes(int N, int K) { return vv_w13_plane_bytes(N, K) + (int64_t)(2 * (N / 16) + 4) * 4; }

#ifdef __HIPCC__
struct VVW13Raw { u32x4 h0, h1, lo; unsigned l4; };      // one lane's share of a group: 52 B

// g: the (tile, group)'s first byte
__device__ __forceinline__ VVW13Raw vv_w13_load(const unsigned char* __restrict__ g, int lane) {
    VVW13Raw r;
    r.h0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g) + lane);
    r.h1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + 1024) + lane);
    r.lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + 2048) + lane);
    r.l4 = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(g + 3072) + lane);
    return r;
}
__device__ __forceinline__ void vv_w13_store(unsigned char* __restrict__ g, int lane, const VVW13Raw& r) {
    reinterpret_cast<u32x4*>(g)[lane] = r.h0;
    reinterpret_cast<u32x4*>(g + 1024)[lane] = r.h1;
    reinterpret_cast<u32x4*>(g + 2048)[lane] = r.lo;
    reinterpret_cast<unsigned*>(g + 3072)[lane] = r.l4;
}
// the conversion's scale 2^(Emax - 142) (a denormal float below Emax = 16: the pack kernel's round trip decides whether it holds)
__device__ __forceinline__ float vv_w13_scale(unsigned emax) {
    return __builtin_bit_cast(float, emax >= 16u ? (emax - 15u) << 23 : 1u << ((emax + 7u) & 31u));
}

// The only decoder: one lane's group -> the four bf16 fragments (k-tiles 0..3 of the group) the MFMA consumes.
__device__ __forceinline__ void vv_w13_unpack(const VVW13Raw& r, float scale, u32x4 (&f)[4]) {
    const unsigned hi[8] = {r.h0[0], r.h0[1], r.h0[2], r.h0[3], r.h1[0], r.h1[1], r.h1[2], r.h1[3]};
    const unsigned lo[5] = {r.lo[0], r.lo[1], r.lo[2], r.lo[3], r.l4};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int d = (10 * j) >> 5, s = (10 * j) & 31;
        unsigned x = lo[d] >> s;
        if (s + 10 > 32) x |= lo[d + 1] << (32 - s);
        x &= 0x3ffu;
        const unsigned low = (x * 0x801u) & 0x001f001fu;      // lo[2j] at bit 0, lo[2j + 1] at bit 16
        const bf16x2 v = (j & 1) ? __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(hi[j >> 1], scale, true)
                                 : __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(hi[j >> 1], scale, false);
        f[j >> 2][j & 3] = __builtin_bit_cast(unsigned, v) | low;
    }
}
#endif
