// level.hip -- output level: a gain and a look-ahead peak limiter (vibevoice_amd/level.py is the definition).  With A the look-ahead and
// ramp, H the hold (samples), g the gain, c the ceiling, x zero outside the signal:
//   u = fl(g x), a non-finite u counts as 0;   r = 1 where |u| <= c, fl(c / |u|) elsewhere;   q = floor(r 2^20)
//   h[j] = min q[j - H .. j + A - 1];   S[i] = sum h[i - A + 1 .. i];   a = fl(float(S) / float(A 2^20));   y = clamp(fl(a u), -c, c)
// q, h and S are integers: minima and sums in any order give the same bits, so the kernels are held to the definition with no tolerance.
//
// Both kernels run lv_solve over a stretch of B <= VV_LV_BUF samples staged in LDS, 1024 threads:
//   1. u and q of every staged sample (u replaces x in place);
//   2. the sliding minimum over W = H + A by doubling, in place: after the pass of stride s, m[b] = min q[b .. b + 2 s - 1] (each thread
//      reads its up to 8 elements and their partners into registers, barrier, writes them back, barrier); with s the largest power of
//      two <= W, min(m[b], m[b + W - s]) is the minimum over q[b .. b + W - 1] = h[b + H].  Reads past the stretch count as r = 1;
//   3. an inclusive prefix sum of those minima, in place, modulo 2^32: each thread scans its 8 consecutive words, the waves scan their
//      threads' totals by shuffles, the 16 wave totals go through LDS.  S <= A 2^20 < 2^31, so the difference of two prefixes is S.
// lv_sample then forms one output from u and two prefixes.  log2(W) + 3 passes over the stretch, no thread walks the row.
//
// vv_level_rows_kernel (streaming, chunk-continuous): ONE workgroup per row of the push, the rows by value in the kernel arguments
// (VVLvRows, vv_common.h).  The stretch is [the stream's H + 2 A - 2 history samples | the chunk | A - 1 zeros]; the new history (the
// last H + 2 A - 2 samples that have arrived) goes back while step 1 walks the stretch.  Float rows are stored as they are; 16-bit rows
// with the rule of vv_device.h (vv_block_peak, vv_pcm16_of) over the row's own output in the same launch: the peak is <= c <= 1.
// vv_level_once_kernel (stateless, whole signals): outputs tiled over workgroups, each tile's stretch read from global memory.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int LV_THREADS = 1024, LV_WAVES = LV_THREADS / 64, LV_PER = 8, LV_ONE = 1 << 20;
static_assert(VV_LV_BUF <= LV_THREADS * LV_PER && VV_LV_BUF % 4 == 0, "eight staged samples per thread");

struct LvLds {
    float u[VV_LV_BUF];                 // the staged stretch: x, then u
    unsigned m[VV_LV_BUF];              // q, the running minima, then their prefix sums
    unsigned part[LV_WAVES];
    float wmx[LV_WAVES];
};
static_assert(sizeof(LvLds) <= 65536, "static LDS");

// Steps 1 to 3 over lds.u[0 .. B), which the caller has staged and published with a barrier.  hrow (may be null): where samples
// [n_in, n_in + hist) of the stretch go, the stream's new history.  On return (behind a barrier) lds.u holds u and lds.m the prefixes.
__device__ void lv_solve(LvLds& lds, int B, int A, int H, float g, float c, float* __restrict__ hrow, int n_in, int hist) {
    const int tid = threadIdx.x;
    for (int b = tid; b < B; b += LV_THREADS) {
        const float xv = lds.u[b];
        if (hrow && b >= n_in && b < n_in + hist) hrow[b - n_in] = xv;       // every read of the old row is done: the caller's barrier
        float u = __fmul_rn(g, xv);
        if ((__float_as_uint(u) & 0x7f800000u) == 0x7f800000u) u = 0.f;      // inf or NaN
        const float au = fabsf(u);
        unsigned q = LV_ONE;
        if (!(au <= c)) q = (unsigned)(int)floorf(__fmul_rn(__fdiv_rn(c, au), 1048576.0f));
        lds.u[b] = u;
        lds.m[b] = q;
    }
    __syncthreads();
    const int W = H + A;
    unsigned v[LV_PER];
    int s = 1;
    for (; 2 * s <= W; s <<= 1) {
#pragma unroll
        for (int i = 0; i < LV_PER; ++i) {
            const int b = tid + i * LV_THREADS;
            if (b < B) { const unsigned p = b + s < B ? lds.m[b + s] : (unsigned)LV_ONE; v[i] = min(lds.m[b], p); }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < LV_PER; ++i) { const int b = tid + i * LV_THREADS; if (b < B) lds.m[b] = v[i]; }
        __syncthreads();
    }
    // the window minimum of thread tid's eight consecutive words, then their prefix sum
    const int d = W - s, b8 = tid * LV_PER;
    unsigned run = 0;
#pragma unroll
    for (int i = 0; i < LV_PER; ++i) {
        const int b = b8 + i;
        unsigned w = 0;
        if (b < B) { const unsigned p = b + d < B ? lds.m[b + d] : (unsigned)LV_ONE; w = min(lds.m[b], p); }
        run += w;
        v[i] = run;
    }
    unsigned inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o); if ((tid & 63) >= o) inc += t; }
    if ((tid & 63) == 63) lds.part[tid >> 6] = inc;
    __syncthreads();                                        // the partners above have been read, the wave totals are in
    unsigned base = inc - run;
    for (int wv = 0; wv < (tid >> 6); ++wv) base += lds.part[wv];
#pragma unroll
    for (int i = 0; i < LV_PER; ++i) { const int b = b8 + i; if (b < B) lds.m[b] = base + v[i]; }
    __syncthreads();
}

// the output at index b of the stretch: S = sum_{j = b - A + 1 .. b} h[j] = P[b - H] - P[b - H - A], P the prefixes (P[-1] = 0)
__device__ __forceinline__ float lv_sample(const LvLds& lds, int b, int A, int H, float c, float denom) {
    const int e = b - H;
    const unsigned S = lds.m[e] - (e - A >= 0 ? lds.m[e - A] : 0u);
    const float a = __fdiv_rn(__int2float_rn((int)S), denom);
    return fminf(fmaxf(__fmul_rn(a, lds.u[b]), -c), c);
}

__global__ __launch_bounds__(LV_THREADS) void vv_level_rows_kernel(VVLvRows rows, int A, int H, float c, float* __restrict__ hist,
                                                                  const float* __restrict__ x, int ld_in, void* __restrict__ out, int ld_out,
                                                                  int pcm16) {
    __shared__ LvLds lds;
    const VVLvRow r = rows.r[blockIdx.x];                       // uniform index into the kernel arguments
    const int tid = threadIdx.x, nh = H + 2 * A - 2, B = nh + r.n_in + A - 1;
    float* hrow = hist + (size_t)r.stream * nh;
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    for (int b = tid; b < B; b += LV_THREADS) lds.u[b] = b < nh ? hrow[b] : (b < nh + r.n_in ? xr[b - nh] : 0.f);
    __syncthreads();
    lv_solve(lds, B, A, H, r.gain, c, hrow, r.n_in, nh);
    const float denom = (float)(A * LV_ONE);
    float y[LV_PER];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < LV_PER; ++i) {
        const int j = tid + i * LV_THREADS;
        y[i] = j < r.n_out ? lv_sample(lds, r.b0 + j, A, H, c, denom) : 0.f;
        mx = fmaxf(mx, fabsf(y[i]));
    }
    if (!pcm16) {
        float* orow = (float*)out + (size_t)blockIdx.x * ld_out;
#pragma unroll
        for (int i = 0; i < LV_PER; ++i) { const int j = tid + i * LV_THREADS; if (j < r.n_out) orow[j] = y[i]; }
        return;
    }
    const float peak = vv_block_peak<LV_WAVES>(mx, lds.wmx);
    short* orow = (short*)out + (size_t)blockIdx.x * ld_out;
#pragma unroll
    for (int i = 0; i < LV_PER; ++i) { const int j = tid + i * LV_THREADS; if (j < r.n_out) orow[j] = vv_pcm16_of(y[i], peak); }
}

// Tile t of a signal holds outputs [t * tile, min(n_in, (t + 1) * tile)); its stretch starts H + A - 1 samples before the first of them
// and ends A - 1 samples behind the last, zeros where the signal has none.
__global__ __launch_bounds__(LV_THREADS) void vv_level_once_kernel(int A, int H, float g, float c, int tile, int n_in, const float* __restrict__ x,
                                                                  int ld_in, float* __restrict__ out, int ld_out) {
    __shared__ LvLds lds;
    const int tid = threadIdx.x, b0 = H + A - 1;
    const long long o0 = (long long)blockIdx.x * tile, left = (long long)n_in - o0;
    const int n_out = (int)(left < tile ? left : tile), B = b0 + n_out + A - 1;
    const float* xr = x + (size_t)blockIdx.y * ld_in;
    for (int b = tid; b < B; b += LV_THREADS) {
        const long long at = o0 - b0 + b;
        lds.u[b] = (at >= 0 && at < n_in) ? xr[at] : 0.f;
    }
    __syncthreads();
    lv_solve(lds, B, A, H, g, c, nullptr, 0, 0);
    const float denom = (float)(A * LV_ONE);
    float* orow = out + (size_t)blockIdx.y * ld_out + o0;
    for (int j = tid; j < n_out; j += LV_THREADS) orow[j] = lv_sample(lds, b0 + j, A, H, c, denom);
}

// zero the history rows of up to 16 streams (a kernel, not a memset node: DESIGN.md section 8)
struct LvIds { int id[16]; };
__global__ void vv_level_reset_kernel(float* __restrict__ hist, int nh, LvIds ids) {
    float* hrow = hist + (size_t)ids.id[blockIdx.x] * nh;
    for (int i = threadIdx.x; i < nh; i += blockDim.x) hrow[i] = 0.f;
}

bool lv_params_ok(int A, int H, float c) {
    return A >= 1 && A <= VV_LV_MAX_A && H >= 0 && (long long)H + 3LL * A - 3 < VV_LV_BUF && c > 0.f && c <= 1.0f;
}
bool lv_gain_ok(float g) { return g > 0.f && g <= 16.0f; }       // a NaN compares false

}  // namespace

// The caller (vv_level_rows, engine_codec.hip) has derived every row from its stream's counter; what the kernel indexes with is checked
// again here against the staging buffer's bounds: -1, nothing launched.
extern "C" int vv_level_rows_launch(const VVLvRows* rows, int n, int A, int H, float c, float* hist, int n_streams, const float* x, int ld_in,
                                    void* out, int ld_out, int pcm16, hipStream_t s) {
    if (!rows || !hist || !out || n < 1 || n > 16 || !lv_params_ok(A, H, c)) return -1;
    const int nh = H + 2 * A - 2;
    for (int i = 0; i < n; ++i) {
        const VVLvRow& r = rows->r[i];
        for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
        if (r.stream < 0 || r.stream >= n_streams || r.n_in < 0 || r.n_in > ld_in || (r.n_in > 0 && !x)) return -1;
        if ((long long)nh + r.n_in + A - 1 > VV_LV_BUF) return -1;
        if (r.n_out < 0 || r.n_out > ld_out || r.n_out > LV_THREADS * LV_PER) return -1;
        // an output is a sample that has arrived, no earlier than the first one whose windows the history still holds
        if (r.n_out > 0 && (r.b0 < H + A - 1 || (long long)r.b0 + r.n_out > (long long)nh + r.n_in)) return -1;
        if (!lv_gain_ok(r.gain)) return -1;
    }
    hipLaunchKernelGGL(vv_level_rows_kernel, dim3(n), dim3(LV_THREADS), 0, s, *rows, A, H, c, hist, x, ld_in, out, ld_out, pcm16);
    return vv_launch_rc(0);
}

// n signals of n_in samples -> n_in outputs each
extern "C" int vv_level_once_launch(int A, int H, float g, float c, int n, int n_in, const float* x, int ld_in, float* out, int ld_out,
                                    hipStream_t s) {
    if (!x || !out || n < 1 || n > 65535 || n_in < 1 || n_in > ld_in || n_in > ld_out || !lv_params_ok(A, H, c) || !lv_gain_ok(g)) return -1;
    const int tile = VV_LV_BUF - (H + 2 * A - 2);               // >= 1: lv_params_ok
    hipLaunchKernelGGL(vv_level_once_kernel, dim3((unsigned)(((long long)n_in + tile - 1) / tile), n), dim3(LV_THREADS), 0, s, A, H, g, c, tile,
                       n_in, x, ld_in, out, ld_out);
    return vv_launch_rc(0);
}

extern "C" int vv_level_reset_launch(float* hist, int nh, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!hist || !ids || n < 1 || n > 16 || nh < 0) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    LvIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_level_reset_kernel, dim3(n), dim3(256), 0, s, hist, nh, a);
    return vv_launch_rc(0);
}
