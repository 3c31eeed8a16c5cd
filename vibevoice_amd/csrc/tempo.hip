// tempo.hip -- speaking rate: a pitch-preserving tempo change P / Q by WSOLA with an exact integer similarity search
// (vibevoice_amd/tempo.py is the definition).  HS = 240, N = 480, DELTA = 160, w the periodic Hann table the host uploads.  Output block
// k sits at a_k = (k HS P) / Q of the input; t_k = p_{k-1} + HS continues the previous segment; over the search signal
// s[i] = rint(clamp(x[i], -1, 1) * 32767) (16 bits), ssd(d) = sum_{i < N} (s[t_k + i] - s[a_k + d + i])^2 for d in [-DELTA, DELTA];
// delta_k = the d of the smallest (ssd, |d|, d >= 0); p_k = a_k + delta_k;
// y[k HS + i] = fl(fl(w[HS + i] x[t_k + i]) + fl(w[i] x[p_k + i])): two rounded products, one rounded sum, no fma.
//
// Both kernels run ONE workgroup of 704 threads per signal, because block k needs delta_{k-1}: the workgroup stages a stretch of the
// signal in LDS (fp32 samples and their 16-bit search signal), walks the blocks that stretch holds in order (tp_search: two lanes per
// candidate, 240 terms each, one 64-bit packed key per candidate, a wave minimum by shuffles, the 11 wave minima through LDS, one
// barrier per block) and then forms every output sample of those blocks in parallel from the recorded positions (tp_sample).
//
// vv_tempo_rows_kernel (streaming, chunk-continuous): one workgroup per row of the push, the rows by value in the kernel arguments
// (VVTpRows, vv_common.h).  The staged stretch is [the stream's VV_TP_HIST history samples | the chunk | zeros]; the new history (the
// last VV_TP_HIST samples that have arrived) and delta of the row's last block go back with ordinary stores.  16-bit rows take the
// rule of vv_device.h (vv_block_peak, vv_pcm16_of) over the row's stretched chunk: the peak first, then the same samples again.
// vv_tempo_once_kernel (stateless, whole signals): one workgroup per signal, the signal staged a tile at a time.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int HS = VV_TP_HS, N = VV_TP_N, DELTA = VV_TP_DELTA, NCAND = 2 * DELTA + 1;
constexpr int TP_THREADS = 704, TP_WAVES = TP_THREADS / 64;       // 2 lanes x 321 candidates = 642 lanes: 11 waves
static_assert(2 * NCAND <= TP_THREADS && TP_THREADS % 64 == 0, "two lanes per candidate");

struct TpLds {
    float x[VV_TP_BUF];                         // the staged stretch of the signal
    short s[VV_TP_BUF];                         // its search signal
    float w[N];
    unsigned long long part[2][TP_WAVES];       // the waves' minima, double-buffered by block parity: one barrier per block
    int tpos[VV_TP_MAX_BLOCKS], ppos[VV_TP_MAX_BLOCKS], dsel[VV_TP_MAX_BLOCKS];     // t_k, p_k (indices into x) and delta_k per block
    float wmx[TP_WAVES];
};
static_assert(sizeof(TpLds) <= 65536, "static LDS");

__device__ __forceinline__ short tp_s16(float v) {
    // fmaxf / fminf return the other operand for a NaN: a NaN counts as -1, as in tempo.py (np.fmax / np.fmin)
    return (short)__float2int_rn(__fmul_rn(fminf(fmaxf(v, -1.0f), 1.0f), 32767.0f));
}

__device__ __forceinline__ long long tp_a(long long k, int P, int Q) { return k < 0 ? -(long long)HS : (k * HS * P) / Q; }

__device__ __forceinline__ unsigned long long tp_shfl_xor(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}

// Blocks k0 .. k0 + nblk - 1 over the staged stretch, lds.x[0] being signal index base; d_prev = delta_{k0 - 1}.  Returns the last
// block's delta (every thread holds it) and leaves tpos / ppos / dsel in LDS; the caller's barrier publishes them.
// Sums: a term is (s1 - s2)^2 <= 65534^2 = 4294705156 < 2^32, so the square is formed in 32 unsigned bits (the product of the
// difference's two's complement with itself is the square modulo 2^32, that is the square); 480 of them stay below 2^41 in the 64-bit
// accumulator.  Key = ssd << 9 | |d| << 1 | (d >= 0): below 2^50, and its minimum is the definition's tie order whatever the lane order.
__device__ int tp_search(TpLds& lds, long long k0, int nblk, long long base, int P, int Q, int d_prev) {
    const int tid = threadIdx.x, c = tid >> 1, g = tid & 1, d = c - DELTA;
    const bool act = c < NCAND;
    const unsigned long long tie = ((unsigned long long)(d < 0 ? -d : d) << 1) | (d >= 0 ? 1u : 0u);
    long long a_prev = tp_a(k0 - 1, P, Q);
    for (int j = 0; j < nblk; ++j) {
        const long long a_abs = tp_a(k0 + j, P, Q);
        const int a = (int)(a_abs - base), t = (int)(a_prev - base) + d_prev + HS;
        a_prev = a_abs;
        unsigned long long key = ~0ull;
        if (act) {
            const short* u = lds.s + t + g * (N / 2);
            const short* v = lds.s + a + d + g * (N / 2);
            unsigned long long acc = 0;
#pragma unroll 8
            for (int i = 0; i < N / 2; ++i) {
                const unsigned df = (unsigned)((int)u[i] - (int)v[i]);
                acc += df * df;
            }
            acc += tp_shfl_xor(acc, 1);                    // the pair's other half: both lanes of a pair are active together
            key = (acc << 9) | tie;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const unsigned long long q = tp_shfl_xor(key, o); key = q < key ? q : key; }
        if ((tid & 63) == 0) lds.part[j & 1][tid >> 6] = key;
        __syncthreads();
        unsigned long long m = lds.part[j & 1][0];
#pragma unroll
        for (int wv = 1; wv < TP_WAVES; ++wv) { const unsigned long long q = lds.part[j & 1][wv]; m = q < m ? q : m; }
        const int mag = (int)((m >> 1) & 255);
        d_prev = (m & 1) ? mag : -mag;
        if (tid == 0) { lds.tpos[j] = t; lds.ppos[j] = a + d_prev; lds.dsel[j] = d_prev; }
    }
    return d_prev;
}

__device__ __forceinline__ float tp_sample(const TpLds& lds, int o) {
#pragma clang fp contract(off)      // the definition rounds both products and the sum (__fmul_rn / __fadd_rn are * and + that may still fuse)
    const int j = o / HS, i = o - j * HS;
    const float a = lds.w[HS + i] * lds.x[lds.tpos[j] + i], b = lds.w[i] * lds.x[lds.ppos[j] + i];
    return a + b;
}

__global__ __launch_bounds__(TP_THREADS) void vv_tempo_rows_kernel(VVTpRows rows, const float* __restrict__ window, float* __restrict__ hist,
                                                                  int* __restrict__ dstate, const float* __restrict__ x, int ld_in,
                                                                  void* __restrict__ out, int ld_out, int pcm16, int* __restrict__ offsets,
                                                                  int ld_off) {
    __shared__ TpLds lds;
    const VVTpRow r = rows.r[blockIdx.x];                       // uniform index into the kernel arguments
    const int tid = threadIdx.x;
    float* hrow = hist + (size_t)r.stream * VV_TP_HIST;
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    for (int i = tid; i < N; i += TP_THREADS) lds.w[i] = window[i];
    for (int i = tid; i < VV_TP_HIST + r.n_in + VV_TP_PAD; i += TP_THREADS) {
        const float v = i < VV_TP_HIST ? hrow[i] : (i < VV_TP_HIST + r.n_in ? xr[i - VV_TP_HIST] : 0.f);
        lds.x[i] = v;
        lds.s[i] = tp_s16(v);
    }
    int d_prev = dstate[r.stream];
    d_prev = d_prev < -DELTA ? -DELTA : (d_prev > DELTA ? DELTA : d_prev);      // whatever the state holds, the reads stay inside the stretch
    __syncthreads();
    for (int i = tid; i < VV_TP_HIST; i += TP_THREADS) hrow[i] = lds.x[r.n_in + i];      // every read of the old row is done
    d_prev = tp_search(lds, r.k0, r.nblk, r.base, r.P, r.Q, d_prev);
    if (tid == 0) dstate[r.stream] = d_prev;
    __syncthreads();
    if (offsets)
        for (int j = tid; j < r.nblk; j += TP_THREADS) offsets[(size_t)blockIdx.x * ld_off + j] = lds.dsel[j];
    if (!pcm16) {
        float* orow = (float*)out + (size_t)blockIdx.x * ld_out;
        for (int o = tid; o < r.n_out; o += TP_THREADS) orow[o] = tp_sample(lds, o);
        return;
    }
    float mx = 0.f;
    for (int o = tid; o < r.n_out; o += TP_THREADS) mx = fmaxf(mx, fabsf(tp_sample(lds, o)));
    const float peak = vv_block_peak<TP_WAVES>(mx, lds.wmx);
    short* orow = (short*)out + (size_t)blockIdx.x * ld_out;
    for (int o = tid; o < r.n_out; o += TP_THREADS) orow[o] = vv_pcm16_of(tp_sample(lds, o), peak);
}

// Block k reads the signal from a_{k-1} - DELTA at the earliest and below hi(k) = max(a_k, a_{k-1} + HS) + DELTA + N (a_k + d + N and
// t_k + N = a_{k-1} + delta_{k-1} + HS + N), whatever the offsets: a tile starts at the first of those for its first block and takes the
// blocks whose hi fits in VV_TP_BUF samples -- at least one, hi(k) - (a_{k-1} - DELTA) <= 1280.
__global__ __launch_bounds__(TP_THREADS) void vv_tempo_once_kernel(const float* __restrict__ window, int P, int Q, int n_in, long long total,
                                                                  const float* __restrict__ x, int ld_in, float* __restrict__ out, int ld_out,
                                                                  int* __restrict__ offsets, int ld_off) {
    __shared__ TpLds lds;
    const int tid = threadIdx.x;
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    float* orow = out + (size_t)blockIdx.x * ld_out;
    for (int i = tid; i < N; i += TP_THREADS) lds.w[i] = window[i];
    const long long nb = (total + HS - 1) / HS;
    int d_prev = 0;
    long long k = 0;
    while (k < nb) {
        const long long base = tp_a(k - 1, P, Q) - DELTA;
        long long k1 = k, len = 0, a_lo = tp_a(k - 1, P, Q);
        while (k1 < nb && k1 - k < VV_TP_MAX_BLOCKS) {
            const long long a_hi = tp_a(k1, P, Q);
            const long long hi = (a_hi > a_lo + HS ? a_hi : a_lo + HS) + DELTA + N - base;
            if (hi > VV_TP_BUF) break;
            len = hi; a_lo = a_hi; ++k1;
        }
        for (int i = tid; i < (int)len; i += TP_THREADS) {
            const long long at = base + i;
            const float v = (at >= 0 && at < n_in) ? xr[at] : 0.f;
            lds.x[i] = v;
            lds.s[i] = tp_s16(v);
        }
        __syncthreads();
        const int nblk = (int)(k1 - k);
        d_prev = tp_search(lds, k, nblk, base, P, Q, d_prev);
        __syncthreads();
        if (offsets)
            for (int j = tid; j < nblk; j += TP_THREADS) offsets[(size_t)blockIdx.x * ld_off + k + j] = lds.dsel[j];
        const long long o0 = k * HS, left = total - o0;
        const int n_out = (int)(left < (long long)nblk * HS ? left : (long long)nblk * HS);
        for (int o = tid; o < n_out; o += TP_THREADS) orow[o0 + o] = tp_sample(lds, o);
        __syncthreads();                                        // the next tile overwrites what these reads use
        k = k1;
    }
}

// a stream back to its first sample: history and last offset zero (a kernel, not a memset node: DESIGN.md section 8)
struct TpIds { int id[16]; };
__global__ void vv_tempo_reset_kernel(float* __restrict__ hist, int* __restrict__ dstate, TpIds ids) {
    const int id = ids.id[blockIdx.x];
    float* hrow = hist + (size_t)id * VV_TP_HIST;
    for (int i = threadIdx.x; i < VV_TP_HIST; i += blockDim.x) hrow[i] = 0.f;
    if (threadIdx.x == 0) dstate[id] = 0;
}

long long tp_a_host(long long k, int P, int Q) { return k < 0 ? -(long long)HS : (k * HS * P) / Q; }

}  // namespace

// The caller (vv_tempo_rows, engine_codec.hip) has derived every row from its stream's counter; what the kernel indexes with is checked
// again here against the staging buffer's bounds: -1, nothing launched.
extern "C" int vv_tempo_rows_launch(const VVTpRows* rows, int n, const float* window, float* hist, int* dstate, int n_streams, const float* x,
                                    int ld_in, void* out, int ld_out, int pcm16, int* offsets, int ld_off, hipStream_t s) {
    if (!rows || !window || !hist || !dstate || !out || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) {
        const VVTpRow& r = rows->r[i];
        for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
        if (r.stream < 0 || r.stream >= n_streams || r.n_in < 0 || r.n_in > ld_in || r.n_in > VV_TP_MAX_IN || (r.n_in > 0 && !x)) return -1;
        if (r.P < 1 || r.Q < 1 || r.P > 2 * r.Q || r.Q > 2 * r.P || r.Q > 100) return -1;
        if (r.k0 < 0 || r.nblk < 0 || r.nblk > VV_TP_MAX_BLOCKS || r.n_out < 0 || r.n_out > r.nblk * HS || r.n_out > ld_out) return -1;
        if (offsets && r.nblk > ld_off) return -1;
        if (r.nblk > 0) {
            const long long k1 = r.k0 + r.nblk - 1, a1 = tp_a_host(k1, r.P, r.Q), a0 = tp_a_host(k1 - 1, r.P, r.Q);
            const long long lo = tp_a_host(r.k0 - 1, r.P, r.Q) - DELTA - r.base;
            const long long hi = (a1 > a0 + HS ? a1 : a0 + HS) + DELTA + N - r.base;
            if (lo < 0 || hi > (long long)VV_TP_HIST + r.n_in + VV_TP_PAD) return -1;
        }
    }
    hipLaunchKernelGGL(vv_tempo_rows_kernel, dim3(n), dim3(TP_THREADS), 0, s, *rows, window, hist, dstate, x, ld_in, out, ld_out, pcm16, offsets,
                       ld_off);
    return vv_launch_rc(0);
}

// n signals of n_in samples -> ceil(n_in * Q / P) outputs each
extern "C" int vv_tempo_once_launch(const float* window, int P, int Q, int n, int n_in, const float* x, int ld_in, float* out, int ld_out,
                                    int* offsets, int ld_off, hipStream_t s) {
    if (!window || !x || !out || n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return -1;
    if (P < 1 || Q < 1 || P > 2 * Q || Q > 2 * P || Q > 100) return -1;
    const long long total = ((long long)n_in * Q + P - 1) / P;
    if (total > ld_out || (long long)n_in + VV_TP_BUF >= ((long long)1 << 31)) return -1;
    if (offsets && (total + HS - 1) / HS > ld_off) return -1;
    hipLaunchKernelGGL(vv_tempo_once_kernel, dim3(n), dim3(TP_THREADS), 0, s, window, P, Q, n_in, total, x, ld_in, out, ld_out, offsets, ld_off);
    return vv_launch_rc(0);
}

extern "C" int vv_tempo_reset_launch(float* hist, int* dstate, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!hist || !dstate || !ids || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    TpIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_tempo_reset_kernel, dim3(n), dim3(256), 0, s, hist, dstate, a);
    return vv_launch_rc(0);
}
