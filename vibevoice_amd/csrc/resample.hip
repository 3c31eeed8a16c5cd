// resample.hip -- rational sample-rate conversion L / M by a polyphase FIR (vibevoice_amd/resample.py is the definition and designs
// the filter): output m is the input at time m * M / L, the input taken as zero outside itself.  With D = (L * T - 2) / 2,
// k = m * M + D, q = k / L, p = k % L:   y[m] = sum_{t < T} coef[p][t] * x[q - t],   fmaf in that order from 0 -- one rounding
// sequence, so the streaming kernel and the one-shot kernel give the same bits for the same m.
//
// vv_resample_rows_kernel (streaming, chunk-continuous): ONE workgroup of 1024 threads per row of the push.  It stages the coefficient
// table [L][T + 1] (odd phase stride: lanes at different phases hit different banks), the stream's T history samples, the chunk and
// T / 2 zeros (read by a flush only) in LDS; after the barrier it writes the stream's new history (the last T staged samples: every
// read of the old row is done) and each thread forms up to 8 outputs, j = thread + 1024 * i, in registers.  Float rows are stored
// as they are; 16-bit rows with the rule of vv_device.h (vv_block_peak, vv_pcm16_of) over the resampled chunk, in the same launch.
// The rows travel by value in the kernel arguments (VVRsRows, vv_common.h); a row's stream is distinct from every other row's.
//
// vv_resample_once_kernel (stateless, whole signals): outputs tiled over workgroups, coefficients and input read from global memory.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int RS_THREADS = 1024, RS_PER = VV_RS_MAX_OUT / RS_THREADS;
constexpr int RS_LDS_MAX = 65536 - 64;      // the default limit less the peak words below: no hipFuncSetAttribute

__global__ __launch_bounds__(RS_THREADS) void vv_resample_rows_kernel(VVRsRows rows, int L, int M, int T, const float* __restrict__ coef,
                                                                     float* __restrict__ hist, const float* __restrict__ x, int ld_in,
                                                                     void* __restrict__ out, int ld_out, int pcm16) {
    extern __shared__ float rs_lds[];
    __shared__ float wmx[RS_THREADS / 64];
    const VVRsRow r = rows.r[blockIdx.x];                       // uniform index into the kernel arguments
    const int tid = threadIdx.x, TP = T + 1, half = T >> 1;
    float* cf = rs_lds;                                         // [L][T + 1]
    float* buf = rs_lds + L * TP;                               // [T | n_in | T / 2]
    for (int i = tid; i < L * T; i += RS_THREADS) { const int p = i / T; cf[p * TP + (i - p * T)] = coef[i]; }
    float* hrow = hist + (size_t)r.stream * T;
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    for (int i = tid; i < T; i += RS_THREADS) buf[i] = hrow[i];
    for (int i = tid; i < r.n_in; i += RS_THREADS) buf[T + i] = xr[i];
    for (int i = tid; i < half; i += RS_THREADS) buf[T + r.n_in + i] = 0.f;
    __syncthreads();
    for (int i = tid; i < T; i += RS_THREADS) hrow[i] = buf[r.n_in + i];

    float acc[RS_PER];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < RS_PER; ++i) {
        const int j = tid + i * RS_THREADS;
        float a = 0.f;
        if (j < r.n_out) {
            const int kk = r.p0 + j * M, dq = kk / L, p = kk - dq * L;
            const float* c = cf + p * TP;
            const float* b = buf + r.b0 + dq;
            for (int t = 0; t < T; ++t) a = fmaf(c[t], b[-t], a);
        }
        acc[i] = a;
        mx = fmaxf(mx, fabsf(a));
    }
    if (!pcm16) {
        float* orow = (float*)out + (size_t)blockIdx.x * ld_out;
#pragma unroll
        for (int i = 0; i < RS_PER; ++i) { const int j = tid + i * RS_THREADS; if (j < r.n_out) orow[j] = acc[i]; }
        return;
    }
    const float peak = vv_block_peak<RS_THREADS / 64>(mx, wmx);
    short* orow = (short*)out + (size_t)blockIdx.x * ld_out;
#pragma unroll
    for (int i = 0; i < RS_PER; ++i) { const int j = tid + i * RS_THREADS; if (j < r.n_out) orow[j] = vv_pcm16_of(acc[i], peak); }
}

__global__ __launch_bounds__(256) void vv_resample_once_kernel(int L, int M, int T, const float* __restrict__ coef, int n_in, int n_out,
                                                              const float* __restrict__ x, int ld_in, float* __restrict__ out, int ld_out) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    const int64_t k = (int64_t)m * M + (L * T - 2) / 2;
    const int q = (int)(k / L), p = (int)(k - (int64_t)q * L);
    const float* c = coef + (size_t)p * T;
    const float* xr = x + (size_t)blockIdx.y * ld_in;
    float a = 0.f;
    for (int t = 0; t < T; ++t) {
        const int i = q - t;
        a = fmaf(c[t], (i >= 0 && i < n_in) ? xr[i] : 0.f, a);
    }
    out[(size_t)blockIdx.y * ld_out + m] = a;
}

// zero the history rows of up to 16 streams (a kernel, not a memset node: DESIGN.md section 8)
struct RsIds { int id[16]; };
__global__ void vv_resample_reset_kernel(float* __restrict__ hist, int T, RsIds ids) {
    float* hrow = hist + (size_t)ids.id[blockIdx.x] * T;
    for (int i = threadIdx.x; i < T; i += blockDim.x) hrow[i] = 0.f;
}

}  // namespace

extern "C" int vv_resample_lds_bytes(int L, int T, int n_in) {
    const int64_t b = ((int64_t)L * (T + 1) + T + (int64_t)n_in + T / 2) * 4;
    return b > 0x7fffffff ? 0x7fffffff : (int)b;
}

// The caller (vv_resample_rows, engine_codec.hip) has derived every row from its stream's counter; what the kernel indexes with is
// checked again here against the staging buffer's bounds: -1, nothing launched.
extern "C" int vv_resample_rows_launch(const VVRsRows* rows, int n, int L, int M, int T, const float* coef, float* hist, int n_streams,
                                       const float* x, int ld_in, void* out, int ld_out, int pcm16, hipStream_t s) {
    if (!rows || !coef || !hist || !out || n < 1 || n > 16 || L < 1 || L > 4096 || M < 1 || M > 4096 || T < 2 || (T & 1)) return -1;
    int max_in = 0;
    for (int i = 0; i < n; ++i) {
        const VVRsRow& r = rows->r[i];
        for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
        if (r.stream < 0 || r.stream >= n_streams || r.n_in < 0 || r.n_in > ld_in || r.n_out < 0 || r.n_out > VV_RS_MAX_OUT || r.n_out > ld_out) return -1;
        if (r.n_in > 0 && !x) return -1;
        if (r.p0 < 0 || r.p0 >= L) return -1;
        if (r.n_out > 0) {
            const int64_t last = (int64_t)r.b0 + ((int64_t)r.p0 + (int64_t)(r.n_out - 1) * M) / L;
            if (r.b0 - (T - 1) < 0 || last >= (int64_t)T + r.n_in + T / 2) return -1;
        }
        max_in = r.n_in > max_in ? r.n_in : max_in;
    }
    const int lds = vv_resample_lds_bytes(L, T, max_in);
    if (lds > RS_LDS_MAX) return -1;
    hipLaunchKernelGGL(vv_resample_rows_kernel, dim3(n), dim3(RS_THREADS), lds, s, *rows, L, M, T, coef, hist, x, ld_in, out, ld_out, pcm16);
    return vv_launch_rc(0);
}

// n signals of n_in samples -> ceil(n_in * L / M) outputs each
extern "C" int vv_resample_once_launch(int L, int M, int T, const float* coef, int n, int n_in, const float* x, int ld_in, float* out, int ld_out,
                                       hipStream_t s) {
    if (!coef || !x || !out || n < 1 || n > 65535 || n_in < 1 || n_in > ld_in || L < 1 || M < 1 || T < 2 || (T & 1)) return -1;
    const int64_t n_out = ((int64_t)n_in * L + M - 1) / M;
    if (n_out > ld_out || n_out >= ((int64_t)1 << 31) - 256 || (int64_t)n_in + T >= ((int64_t)1 << 31)) return -1;
    hipLaunchKernelGGL(vv_resample_once_kernel, dim3((unsigned)((n_out + 255) / 256), n), dim3(256), 0, s, L, M, T, coef, n_in, (int)n_out, x, ld_in,
                       out, ld_out);
    return vv_launch_rc(0);
}

extern "C" int vv_resample_reset_launch(float* hist, int T, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!hist || !ids || n < 1 || n > 16 || T < 1) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    RsIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_resample_reset_kernel, dim3(n), dim3(64), 0, s, hist, T, a);
    return vv_launch_rc(0);
}
