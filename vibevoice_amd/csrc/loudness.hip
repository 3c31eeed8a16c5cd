// loudness.hip -- BS.1770 segment energies and the adaptive leveller (vibevoice_amd/loudness.py is the definition).  At 24 kHz, with S = 2400
// samples a segment and T = 2400 taps hq (int32, the K-weighting impulse response times 2^24):
//   xq = rint(fl(clamp(x, -8, 8) 2^20)), a non-finite x counts as 0;   z[i] = sum_k hq[k] xq[i - k];   zs = z >> 28;   E[m] = sum zs^2
//   a segment counts if E >= VV_LD_GATE; M30 / c30: sum and number of the last <= 30 counted segments, M4: sum of the last 4; while
//   c30 < 4 w[m] = w[m-1], else p = max(fl(float(M30 >> 8) / float(c30 S 2^24)), fl(float(M4 >> 8) / float(4 S 2^24))) and
//   w[m] = clamp(fl(sqrt(fl(t / p))), wmin, wmax);   sample k of segment m: a = fl(w[m-2] + fl(fl(w[m-1] - w[m-2]) fl(k / S))), y = fl(a x)
// |z| < 2^49, so z is an exact integer in fp64 whatever the order of its 2400 fused multiply-adds: the FIR runs on the fp64 pipe in
// parallel and is held to the definition with no tolerance.  Everything behind z is integer or a single correctly rounded fp32 operation.
//
// ld_tile, 256 threads, is the work: 320 outputs of the FIR from a stretch of 320 + T - 1 quantised inputs staged in LDS as fp64.  Lane l
// of each wave owns outputs 5 l .. 5 l + 4 (a stride of 5 doubles: its LDS reads hit distinct banks), the four waves split the taps, 600
// each; a step of 5 taps reads 5 new inputs and 5 taps (a broadcast) for 25 fma.  The waves' partial sums meet in LDS (exact, any order),
// then zs^2 is summed per wave and added to one of two 64-bit LDS words: the segment the tile starts in, and the next one.
//
// Streaming (vv_loud_rows_launch), two kernel launches per push:
//   vv_loud_fir_rows_kernel, grid (tiles of 320 samples, rows): the stretch comes from the stream's ring of quantised inputs (slot =
//     position % T, zero after a reset) and the chunk; the tile's two sums go to part[stream][tile][2].
//   vv_loud_apply_rows_kernel, ONE workgroup per row, orders its phases inside the launch: thread 0 adds the tiles' sums to the open
//     segment's (1), closes the at most two segments the push completes -- ring of counted energies, wanted gain (2), barrier, then all
//     threads apply the gains and store the chunk's quantised samples to the ring (3).  State goes back with ordinary vector stores.
// One-shot: vv_loud_energy_kernel, one workgroup per segment (8 tiles of 300), writes E[row][m] and, for the meter, the same sum at 16
// times the resolution, F[row][m] = sum (z >> 24)^2 < 2^62 (at -60 LUFS zs is a few dozen units and its floor shows in a reading; the
// leveller never looks that far down, the meter does); vv_loud_once_kernel, one workgroup per row, walks the segments with the leveller's
// state in LDS and registers only.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int LD_S = VV_LD_S, LD_T = VV_LD_T, LD_TILE = VV_LD_TILE, LD_RING = VV_LD_RING;
constexpr int LD_B = LD_TILE + LD_T - 1;                    // staged inputs of a tile
constexpr int LD_FIR_THREADS = 256, LD_FIR_WAVES = LD_FIR_THREADS / 64, LD_PER = 5, LD_WAVE_TAPS = LD_T / LD_FIR_WAVES;
constexpr int LD_ONCE_TILE = 300;                           // the one-shot's tiles: 8 to a segment
constexpr int LD_APPLY_THREADS = 1024;
constexpr float LD_WMIN = 0x1.0270acp-4f;                   // float32(10^(-24 / 20)) (loudness.py: WMIN)
static_assert(64 * LD_PER == LD_TILE && LD_WAVE_TAPS * LD_FIR_WAVES == LD_T && LD_WAVE_TAPS % LD_PER == 0, "lanes x outputs, waves x taps");
static_assert(LD_S % LD_ONCE_TILE == 0 && LD_ONCE_TILE <= LD_TILE && LD_TILE < LD_S, "a tile touches at most two segments");
static_assert((VV_LD_S - 1 + VV_LD_MAX_IN) / VV_LD_S <= 2 && VV_LD_MAX_TILES * VV_LD_TILE == VV_LD_MAX_IN, "a push closes at most 2 segments");

struct LdFirLds {
    double xs[LD_B + 1];                // xq at output index b - (T - 1) of the tile
    double hs[LD_T];
    double zp[LD_FIR_WAVES][LD_TILE];   // each wave's share of z
    unsigned long long e[3];            // the segment the tile starts in, the next one; FINE: sum (z >> 24)^2 of the whole tile
};
static_assert(sizeof(LdFirLds) <= 65536, "static LDS");

__device__ __forceinline__ float ld_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 0.f : x; }
__device__ __forceinline__ int ld_quant(float x) {
    return __float2int_rn(__fmul_rn(fminf(fmaxf(ld_finite(x), -8.0f), 8.0f), 1048576.0f));
}

// The caller has staged lds.xs[0 .. LD_B) and lds.hs, set lds.e and published them with a barrier.  Adds zs^2 of the tile's outputs
// o < min(split, cnt) to lds.e[0] and of split <= o < cnt to lds.e[1] (FINE: and (z >> 24)^2 of every o < cnt to lds.e[2]); returns
// behind a barrier: lds.e is complete, lds.xs is free.
template <bool FINE>
__device__ void ld_tile(LdFirLds& lds, int cnt, int split) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kb = wv * LD_WAVE_TAPS;
    double acc[LD_PER], w[2 * LD_PER - 1];
#pragma unroll
    for (int r = 0; r < LD_PER; ++r) acc[r] = 0.0;
    // w[j] = xs[base - 4 + j], base = T - 1 + 5 lane - k0 the index of output 5 lane's input at tap k0: output r at tap k0 + u reads
    // w[4 + r - u].  base - 4 >= T - 1 - (T - 5) - 4 = 0 and base + 4 <= T - 1 + 315 + 4 = LD_B - 1.
    int base = LD_T - 1 + LD_PER * lane - kb;
#pragma unroll
    for (int j = LD_PER; j < 2 * LD_PER - 1; ++j) w[j] = lds.xs[base - (LD_PER - 1) + j];
    for (int k0 = kb; k0 < kb + LD_WAVE_TAPS; k0 += LD_PER, base -= LD_PER) {
#pragma unroll
        for (int j = 0; j < LD_PER; ++j) w[j] = lds.xs[base - (LD_PER - 1) + j];
#pragma unroll
        for (int u = 0; u < LD_PER; ++u) {
            const double h = lds.hs[k0 + u];
#pragma unroll
            for (int r = 0; r < LD_PER; ++r) acc[r] = fma(h, w[LD_PER - 1 + r - u], acc[r]);
        }
#pragma unroll
        for (int j = 0; j < LD_PER - 1; ++j) w[LD_PER + j] = w[j];
    }
#pragma unroll
    for (int r = 0; r < LD_PER; ++r) lds.zp[wv][LD_PER * lane + r] = acc[r];
    __syncthreads();
    long long e0 = 0, e1 = 0, f = 0;
    for (int o = tid; o < cnt; o += LD_FIR_THREADS) {
        const double z = (lds.zp[0][o] + lds.zp[1][o]) + (lds.zp[2][o] + lds.zp[3][o]);      // integers below 2^49: exact
        const long long zi = (long long)z, zs = zi >> 28;
        if (o < split) e0 += zs * zs; else e1 += zs * zs;
        if (FINE) { const long long zf = zi >> 24; f += zf * zf; }      // |zf| < 2^25: a segment's sum stays below 2400 2^50 < 2^62
    }
    e0 = vv_wave_sum(e0);
    e1 = vv_wave_sum(e1);
    if (FINE) f = vv_wave_sum(f);
    if (lane == 0) {
        atomicAdd(&lds.e[0], (unsigned long long)e0);
        atomicAdd(&lds.e[1], (unsigned long long)e1);
        if (FINE) atomicAdd(&lds.e[2], (unsigned long long)f);
    }
    __syncthreads();
}

__global__ __launch_bounds__(LD_FIR_THREADS) void vv_loud_fir_rows_kernel(VVLdRows rows, const double* __restrict__ taps, const int* __restrict__ hist,
                                                                         const float* __restrict__ x, int ld_in, long long* __restrict__ part) {
    __shared__ LdFirLds lds;
    const VVLdRow r = rows.r[blockIdx.y];                       // uniform index into the kernel arguments
    const int tid = threadIdx.x, o0 = blockIdx.x * LD_TILE;
    if (o0 >= r.n_in) return;                                   // the apply kernel reads the tiles below ceil(n_in / 320) only
    const int cnt = min(LD_TILE, r.n_in - o0);
    const int* hrow = hist + (size_t)r.stream * LD_T;
    const float* xr = x + (size_t)blockIdx.y * ld_in;
    for (int b = tid; b < LD_B; b += LD_FIR_THREADS) {
        const int c = o0 - (LD_T - 1) + b;                      // the sample's index in the chunk, >= -(T - 1)
        int q = 0;
        if (c < 0) { int sl = r.h0 + c; if (sl < 0) sl += LD_T; q = hrow[sl]; }
        else if (c < r.n_in) q = ld_quant(xr[c]);
        lds.xs[b] = (double)q;
    }
    for (int k = tid; k < LD_T; k += LD_FIR_THREADS) lds.hs[k] = taps[k];
    if (tid < 2) lds.e[tid] = 0;
    __syncthreads();
    ld_tile<false>(lds, cnt, LD_S - (r.k0 + o0) % LD_S);
    if (tid < 2) part[((size_t)r.stream * VV_LD_MAX_TILES + blockIdx.x) * 2 + tid] = (long long)lds.e[tid];
}

// segment blockIdx.x of signal blockIdx.y: x is zero before the signal.  E and F may each be null.
__global__ __launch_bounds__(LD_FIR_THREADS) void vv_loud_energy_kernel(const double* __restrict__ taps, int n_in, const float* __restrict__ x, int ld_in,
                                                                       long long* __restrict__ E, int ld_e, long long* __restrict__ F, int ld_f) {
    __shared__ LdFirLds lds;
    const int tid = threadIdx.x;
    const float* xr = x + (size_t)blockIdx.y * ld_in;
    for (int k = tid; k < LD_T; k += LD_FIR_THREADS) lds.hs[k] = taps[k];
    if (tid < 3) lds.e[tid] = 0;
    for (int sub = 0; sub < LD_S / LD_ONCE_TILE; ++sub) {
        const long long o0 = (long long)blockIdx.x * LD_S + sub * LD_ONCE_TILE;
        for (int b = tid; b < LD_B; b += LD_FIR_THREADS) {
            const long long c = o0 - (LD_T - 1) + b;
            lds.xs[b] = (c >= 0 && c < n_in) ? (double)ld_quant(xr[c]) : 0.0;
        }
        __syncthreads();
        ld_tile<true>(lds, LD_ONCE_TILE, LD_ONCE_TILE);
    }
    if (tid == 0 && E) E[(size_t)blockIdx.y * ld_e + blockIdx.x] = (long long)lds.e[0];
    if (tid == 0 && F) F[(size_t)blockIdx.y * ld_f + blockIdx.x] = (long long)lds.e[2];
}

struct LdGainLds { long long ring[LD_RING]; long long E[4]; float G[4]; int head, count; };

// Segment m is complete with energy E (one thread): the ring of counted energies moves on, -> w[m] from w[m-1]
__device__ float ld_close(LdGainLds& l, long long E, float w1, float t, float wmax) {
    if (E >= VV_LD_GATE) {
        l.ring[l.head] = E;
        l.head = l.head + 1 == LD_RING ? 0 : l.head + 1;
        if (l.count < LD_RING) ++l.count;
    }
    if (l.count < 4) return w1;
    long long m30 = 0, m4 = 0;
    int at = l.head;
    for (int i = 0; i < l.count; ++i) {
        at = at == 0 ? LD_RING - 1 : at - 1;
        m30 += l.ring[at];
        if (i < 4) m4 += l.ring[at];
    }
    // M >> 8 < 2^51 is exact in fp64 and rounds once to fp32; c30 S 2^24 = (75 c30) 2^29 and 4 S 2^24 = 75 2^31 are fp32 values
    const float p30 = __fdiv_rn(__double2float_rn(__ll2double_rn(m30 >> 8)), __fmul_rn((float)(75 * l.count), 536870912.0f));
    const float p4 = __fdiv_rn(__double2float_rn(__ll2double_rn(m4 >> 8)), 161061273600.0f);
    // the fp64 square root of an fp32 value, rounded to fp32, is the correctly rounded fp32 square root (53 >= 2 * 24 + 2)
    const float w = __double2float_rn(sqrt((double)__fdiv_rn(t, fmaxf(p30, p4))));
    return fminf(fmaxf(w, LD_WMIN), wmax);
}

// three roundings: the product must not fuse with the sum (the compiler contracts a * b + c by default, also through __fmul_rn / __fadd_rn)
__device__ __forceinline__ float ld_gain(float w2, float w1, int k) {
#pragma clang fp contract(off)
    const float f = __fdiv_rn((float)k, (float)LD_S), d = w1 - w2;
    const float step = d * f;
    return w2 + step;
}

__global__ __launch_bounds__(LD_APPLY_THREADS) void vv_loud_apply_rows_kernel(VVLdRows rows, int* __restrict__ hist, VVLdState* __restrict__ state,
                                                                             const long long* __restrict__ part, const float* __restrict__ x, int ld_in,
                                                                             float* __restrict__ out, int ld_out) {
    __shared__ LdGainLds l;
    const VVLdRow r = rows.r[blockIdx.x];
    const int tid = threadIdx.x;
    VVLdState* st = state + r.stream;
    if (tid < LD_RING) l.ring[tid] = r.first ? 0 : st->e[tid];
    if (tid >= 32 && tid < 36) l.E[tid - 32] = 0;
    __syncthreads();
    if (tid == 0) {
        const int h = r.first ? 0 : st->head, c = r.first ? 0 : st->count;
        l.head = (unsigned)h < (unsigned)LD_RING ? h : 0;
        l.count = c < 0 ? 0 : (c > LD_RING ? LD_RING : c);
        float w1 = r.first ? r.g0 : st->w1, w2 = r.first ? r.g0 : st->w2;
        // 1. the tiles' sums into the segments they belong to; segment 0 is the one that was open
        const long long* p = part + (size_t)r.stream * VV_LD_MAX_TILES * 2;
        const int ntiles = (r.n_in + LD_TILE - 1) / LD_TILE;
        for (int t = 0; t < ntiles; ++t) {
            const int s0 = (r.k0 + t * LD_TILE) / LD_S;           // <= 2
            l.E[s0] += p[2 * t];
            l.E[s0 + 1] += p[2 * t + 1];
        }
        l.E[0] += r.first ? 0 : st->acc;
        // 2. the segments this push completes, in order
        const int nseg = (r.k0 + r.n_in) / LD_S;                  // <= 2
        l.G[0] = w2; l.G[1] = w1; l.G[2] = w1; l.G[3] = w1;
        for (int j = 0; j < nseg; ++j) {
            const float wn = ld_close(l, l.E[j], w1, r.t, r.wmax);
            w2 = w1; w1 = wn;
            l.G[j + 2] = wn;
        }
        st->acc = l.E[nseg]; st->head = l.head; st->count = l.count; st->w1 = w1; st->w2 = w2;
    }
    __syncthreads();
    if (tid < LD_RING) st->e[tid] = l.ring[tid];
    // 3. sample j sits at position k0 + j of the segment that was open: segment rel <= 2 of this push, gains G[rel], G[rel + 1]
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    float* orow = out + (size_t)blockIdx.x * ld_out;
    int* hrow = hist + (size_t)r.stream * LD_T;
    for (int j = tid; j < r.n_in; j += LD_APPLY_THREADS) {
        const float xv = xr[j];
        const int pos = r.k0 + j, rel = pos / LD_S;
        orow[j] = __fmul_rn(ld_gain(l.G[rel], l.G[rel + 1], pos - rel * LD_S), ld_finite(xv));
        if (j >= r.n_in - LD_T) hrow[(r.h0 + j) % LD_T] = ld_quant(xv);      // each slot once: the chunk's last T samples
    }
}

__global__ __launch_bounds__(LD_APPLY_THREADS) void vv_loud_once_kernel(float t, float g0, float wmax, int n_in, const long long* __restrict__ E, int ld_e,
                                                                       const float* __restrict__ x, int ld_in, float* __restrict__ out, int ld_out,
                                                                       float* __restrict__ gain, int ld_g) {
    __shared__ LdGainLds l;
    const int tid = threadIdx.x;
    if (tid < LD_RING) l.ring[tid] = 0;
    if (tid == 0) { l.head = 0; l.count = 0; l.G[0] = g0; l.G[1] = g0; }
    __syncthreads();
    const long long* Er = E + (size_t)blockIdx.x * ld_e;
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    float* orow = out + (size_t)blockIdx.x * ld_out;
    float* grow = gain ? gain + (size_t)blockIdx.x * ld_g : nullptr;
    const int n_seg = n_in / LD_S, n_all = (int)(((long long)n_in + LD_S - 1) / LD_S);
    for (int m = 0; m < n_all; ++m) {
        const float w2 = l.G[0], w1 = l.G[1];
        const long long b = (long long)m * LD_S;
        for (int k = tid; k < LD_S && b + k < n_in; k += LD_APPLY_THREADS) {
            const float a = ld_gain(w2, w1, k);
            orow[b + k] = __fmul_rn(a, ld_finite(xr[b + k]));
            if (grow) grow[b + k] = a;
        }
        __syncthreads();                                        // every thread has read this segment's gains
        if (tid == 0 && m < n_seg) {
            const float wn = ld_close(l, Er[m], w1, t, wmax);
            l.G[0] = w1; l.G[1] = wn;
        }
        __syncthreads();
    }
}

// the ring of inputs and the state of up to 16 streams to zero (a kernel, not a memset node: DESIGN.md section 8)
struct LdIds { int id[16]; };
__global__ void vv_loud_reset_kernel(int* __restrict__ hist, VVLdState* __restrict__ state, LdIds ids) {
    const int id = ids.id[blockIdx.x];
    int* hrow = hist + (size_t)id * LD_T;
    int* st = (int*)(state + id);
    for (int i = threadIdx.x; i < LD_T; i += blockDim.x) hrow[i] = 0;
    for (int i = threadIdx.x; i < (int)(sizeof(VVLdState) / 4); i += blockDim.x) st[i] = 0;
}

}  // namespace

// The caller (vv_loud_rows, engine_codec.hip) has derived every row from its stream's counter; what the kernels index with is checked
// again here: -1, nothing launched.
extern "C" int vv_loud_rows_launch(const VVLdRows* rows, int n, const double* taps, int* hist, VVLdState* state, long long* part, int n_streams,
                                   const float* x, int ld_in, float* out, int ld_out, hipStream_t s) {
    if (!rows || !taps || !hist || !state || !part || !out || n < 1 || n > 16) return -1;
    int max_in = 0;
    for (int i = 0; i < n; ++i) {
        const VVLdRow& r = rows->r[i];
        for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
        if (r.stream < 0 || r.stream >= n_streams || r.n_in < 0 || r.n_in > VV_LD_MAX_IN || r.n_in > ld_in || r.n_in > ld_out || (r.n_in > 0 && !x)) return -1;
        if (r.k0 < 0 || r.k0 >= VV_LD_S || r.h0 < 0 || r.h0 >= VV_LD_T || !vv_ld_params_ok(r.t, r.g0, r.wmax)) return -1;
        max_in = r.n_in > max_in ? r.n_in : max_in;
    }
    if (max_in > 0) {
        hipLaunchKernelGGL(vv_loud_fir_rows_kernel, dim3((max_in + VV_LD_TILE - 1) / VV_LD_TILE, n), dim3(LD_FIR_THREADS), 0, s, *rows, taps, hist, x, ld_in,
                           part);
        if (vv_launch_rc(0)) return -2;
    }
    hipLaunchKernelGGL(vv_loud_apply_rows_kernel, dim3(n), dim3(LD_APPLY_THREADS), 0, s, *rows, hist, state, part, x, ld_in, out, ld_out);
    return vv_launch_rc(0);
}

// E[i][m] and / or F[i][m], m < n_in / S, of n signals of n_in samples; a signal shorter than a segment has none: nothing is launched
extern "C" int vv_loud_energy_launch(const double* taps, int n, int n_in, const float* x, int ld_in, long long* E, int ld_e, long long* F, int ld_f,
                                     hipStream_t s) {
    if (!taps || !x || n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return -1;
    const int n_seg = n_in / VV_LD_S;
    if (n_seg == 0) return 0;
    if ((!E && !F) || (E && n_seg > ld_e) || (F && n_seg > ld_f)) return -1;
    hipLaunchKernelGGL(vv_loud_energy_kernel, dim3(n_seg, n), dim3(LD_FIR_THREADS), 0, s, taps, n_in, x, ld_in, E, ld_e, F, ld_f);
    return vv_launch_rc(0);
}

// n signals of n_in samples -> n_in outputs each (and their gains where gain is not null); E [n][ld_e]: room for the energies
extern "C" int vv_loud_once_launch(const double* taps, float t, float g0, float wmax, int n, int n_in, const float* x, int ld_in, float* out, int ld_out,
                                   float* gain, int ld_gain, long long* E, int ld_e, hipStream_t s) {
    if (!out || n_in > ld_out || (gain && n_in > ld_gain) || !vv_ld_params_ok(t, g0, wmax)) return -1;
    const int rc = vv_loud_energy_launch(taps, n, n_in, x, ld_in, E, ld_e, nullptr, 0, s);
    if (rc) return rc;
    hipLaunchKernelGGL(vv_loud_once_kernel, dim3(n), dim3(LD_APPLY_THREADS), 0, s, t, g0, wmax, n_in, E, ld_e, x, ld_in, out, ld_out, gain, ld_gain);
    return vv_launch_rc(0);
}

extern "C" int vv_loud_reset_launch(int* hist, VVLdState* state, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!hist || !state || !ids || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    LdIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_loud_reset_kernel, dim3(n), dim3(256), 0, s, hist, state, a);
    return vv_launch_rc(0);
}
