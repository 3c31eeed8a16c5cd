// formant.hip -- a spectral-envelope warp A / B, every row of a launch at its own fraction (vibevoice_amd/formant.py is the definition):
// frames of N = 1024 at hop H = 256 under the periodic Hann window w, frame j over samples [(j - 3) H, (j + 1) H), the signal zero
// outside itself and a non-finite sample 0.  Per frame, K = 513 bins:
//     X = rfft(w x), p = |X|^2, L = 0.5 logf(p + 2^-26 mean(p) + 2^-100), c = irfft(L), E = Re rfft(c for |q| < 64),
//     Ew[k] = E at k * B / A (i = k * B / A, f = fl((k * B % A) / A), fmaf(f, E[i + 1] - E[i], E[i]) where i < 512, E[512] beyond),
//     G = expf(clamp(Ew - E, +-30 dB)), y_j = (2/3) w irfft(G X)
// and out block b = ((y_b + y_b+1) + y_b+2) + y_b+3 over the blocks' own segments, from the zero a stream's partial sums start at.
// 1 / 1 is the identity: the row is copied.
//
// Two launches per push (or per 16 whole signals), the same two kernels for the streaming and the stateless form, so both give the same
// bits for the same frame:
// vv_formant_frames_kernel: grid (frames, rows), ONE workgroup of 256 threads per (row, frame).  The four 1024-point transforms are one
// in-place radix-2 routine in LDS (fm_fft: bit-reversed in, natural out; the caller writes its operand to the reversed index), complex
// fp32 as two planes of 1024 + 32 words (word i at i + i / 32: the small strides of the first stages spread over the banks), the
// twiddles cos / sin 2 pi i / N of the host's table (formant.twiddles(), the only trig here) staged beside them: 21 KB.  The real, even L
// and c go through the same routine as the signal (their imaginary plane zero): one routine, four calls.  The frame reads the stream's
// history and the chunk (VVFmRow, vv_common.h) and writes w-windowed y_j to the launch's scratch.
// vv_formant_sum_kernel: one workgroup per row of a push (per 8 blocks of a whole signal); thread t owns column t of every block:
// it adds the frames in ascending order onto the stream's partial sums, writes the complete blocks to out and the three open ones back,
// and rolls the stream's history (old words read before the barrier, new ones written behind it).
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int FM_THREADS = 256, FM_PER = VV_FM_N / FM_THREADS, FM_LOG2N = 10;
constexpr int FM_PAD = VV_FM_N + VV_FM_N / 32;
constexpr int FM_ONCE_BLOCKS = 8;           // output blocks per workgroup of the stateless sum
constexpr float FM_EPS = 1.4901161193847656e-08f;       // 2^-26
constexpr float FM_TINY = 7.888609052210118e-31f;       // 2^-100
constexpr float FM_GMAX = 3.4538776394910684f;          // 30 dB in nepers
static_assert(VV_FM_N == 1 << FM_LOG2N && FM_PER == 4 && VV_FM_H == FM_THREADS, "the frame is 4 words per thread, the hop one");

__device__ __forceinline__ int fm_p(int i) { return i + (i >> 5); }
__device__ __forceinline__ int fm_rev(int i) { return (int)(__brev((unsigned)i) >> (32 - FM_LOG2N)); }

// In place, 1024 points over the planes re / im (fm_p layout): the operand in bit-reversed order, the transform in natural order.
// sgn -1: sum x e^{-i...}, +1: the conjugate kernel (unscaled).  tc / ts: cos / sin of 2 pi i / N, i < N / 2.  Barriers in front of every
// stage and behind the last: the caller's writes are seen, and so is the result.
__device__ __forceinline__ void fm_fft(float* re, float* im, const float* tc, const float* ts, float sgn) {
    for (int s = 0; s < FM_LOG2N; ++s) {
        __syncthreads();
        const int h = 1 << s;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int b = threadIdx.x + u * FM_THREADS;
            const int j = b & (h - 1), i0 = ((b >> s) << (s + 1)) + j;
            const int t = j << (FM_LOG2N - 1 - s);
            const float wr = tc[t], wi = __fmul_rn(sgn, ts[t]);
            const int p0 = fm_p(i0), p1 = fm_p(i0 + h);
            const float ar = re[p0], ai = im[p0], br = re[p1], bi = im[p1];
            const float tr = fmaf(wr, br, -__fmul_rn(wi, bi)), ti = fmaf(wr, bi, __fmul_rn(wi, br));
            re[p0] = __fadd_rn(ar, tr); im[p0] = __fadd_rn(ai, ti);
            re[p1] = __fsub_rn(ar, tr); im[p1] = __fsub_rn(ai, ti);
        }
    }
    __syncthreads();
}

// E at k * B / A
__device__ __forceinline__ float fm_gain(const float* E, int k, int A, int B) {
    const int num = k * B, i = num / A, rem = num - i * A;              // k * B <= 512 * 10^4
    float ew = E[fm_p(VV_FM_K - 1)];
    if (i < VV_FM_K - 1) {
        const float e0 = E[fm_p(i)];
        ew = fmaf(__fdiv_rn((float)rem, (float)A), __fsub_rn(E[fm_p(i + 1)], e0), e0);
    }
    return expf(fminf(fmaxf(__fsub_rn(ew, E[fm_p(k)]), -FM_GMAX), FM_GMAX));
}

__global__ __launch_bounds__(FM_THREADS) void vv_formant_frames_kernel(VVFmRows rows, const float* __restrict__ tw, const float* __restrict__ hist,
                                                                      const float* __restrict__ x, int ld_in, float* __restrict__ scratch,
                                                                      int cap_frames) {
    __shared__ float xr[FM_PAD], xi[FM_PAD], cr[FM_PAD], ci[FM_PAD], tc[VV_FM_N / 2], ts[VV_FM_N / 2], red[FM_THREADS / 64];
    const VVFmRow r = rows.r[blockIdx.y];                       // uniform index into the kernel arguments
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= r.nf) return;                                      // the whole workgroup: no barrier is left waiting
    for (int i = tid; i < VV_FM_N / 2; i += FM_THREADS) { tc[i] = tw[i]; ts[i] = tw[VV_FM_N + i]; }
    const float* xrow = x + (size_t)blockIdx.y * ld_in;
    const float* hrow = hist ? hist + (size_t)r.stream * VV_FM_HIST : nullptr;
    const int pos0 = f * VV_FM_H - 3 * VV_FM_H - r.r;           // the frame's first sample, counted from the chunk's first: >= -(N - 1)
    float w[FM_PER];
#pragma unroll
    for (int m = 0; m < FM_PER; ++m) {
        const int i = tid + m * FM_THREADS, pos = pos0 + i;
        float v = 0.f;
        if (pos < 0) { if (hrow) v = hrow[VV_FM_HIST + pos]; }
        else if (pos < r.n_in) v = xrow[pos];
        if (!isfinite(v)) v = 0.f;
        w[m] = __fsub_rn(0.5f, __fmul_rn(0.5f, tw[i]));
        const int q = fm_p(fm_rev(i));
        xr[q] = __fmul_rn(w[m], v); xi[q] = 0.f;
    }
    fm_fft(xr, xi, tc, ts, -1.f);

    // p, its mean, L (real and even: bin k also stands at N - k), to the second pair of planes
    const bool last = tid == 0;                                 // thread 0 also owns bin K - 1
    float p[3];
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int q = fm_p(tid + m * FM_THREADS); p[m] = fmaf(xr[q], xr[q], __fmul_rn(xi[q], xi[q])); }
    p[2] = 0.f;
    if (last) { const int q = fm_p(VV_FM_K - 1); p[2] = fmaf(xr[q], xr[q], __fmul_rn(xi[q], xi[q])); }
    const float ws = vv_wave_sum(__fadd_rn(__fadd_rn(p[0], p[1]), p[2]));
    if ((tid & 63) == 0) red[tid >> 6] = ws;
#pragma unroll
    for (int m = 0; m < FM_PER; ++m) ci[fm_p(tid + m * FM_THREADS)] = 0.f;
    __syncthreads();
    const float mean = __fdiv_rn(__fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3])), (float)VV_FM_K);
    const float floor_ = __fmul_rn(FM_EPS, mean);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int k = m < 2 ? tid + m * FM_THREADS : VV_FM_K - 1;
        if (m == 2 && !last) break;
        const float L = __fmul_rn(0.5f, logf(__fadd_rn(__fadd_rn(p[m], floor_), FM_TINY)));
        cr[fm_p(fm_rev(k))] = L;
        if (k > 0 && k < VV_FM_K - 1) cr[fm_p(fm_rev(VV_FM_N - k))] = L;
    }
    fm_fft(cr, ci, tc, ts, -1.f);                               // N c[q], real

    // the lifter and 1 / N, back in reversed order: every word is read before any is written
    float c[FM_PER];
#pragma unroll
    for (int m = 0; m < FM_PER; ++m) {
        const int i = tid + m * FM_THREADS;
        c[m] = (i < VV_FM_QC || i > VV_FM_N - VV_FM_QC) ? __fmul_rn(cr[fm_p(i)], 1.0f / VV_FM_N) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < FM_PER; ++m) {
        const int i = tid + m * FM_THREADS;
        cr[fm_p(fm_rev(i))] = c[m]; ci[fm_p(i)] = 0.f;
    }
    fm_fft(cr, ci, tc, ts, -1.f);                               // E[k] = cr[k], k < K

    float g[3];
    g[0] = fm_gain(cr, tid, r.A, r.B);
    g[1] = fm_gain(cr, tid + FM_THREADS, r.A, r.B);
    g[2] = last ? fm_gain(cr, VV_FM_K - 1, r.A, r.B) : 0.f;
    __syncthreads();                                            // E has been read
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int k = m < 2 ? tid + m * FM_THREADS : VV_FM_K - 1;
        if (m == 2 && !last) break;
        const bool inner = k > 0 && k < VV_FM_K - 1;
        const float yr = __fmul_rn(g[m], xr[fm_p(k)]), yi = inner ? __fmul_rn(g[m], xi[fm_p(k)]) : 0.f;   // a real signal's bins 0 and N / 2 are real
        const int q = fm_p(fm_rev(k));
        cr[q] = yr; ci[q] = yi;
        if (inner) { const int qm = fm_p(fm_rev(VV_FM_N - k)); cr[qm] = yr; ci[qm] = -yi; }
    }
    fm_fft(cr, ci, tc, ts, 1.f);
    float* y = scratch + ((size_t)blockIdx.y * cap_frames + f) * VV_FM_N;
#pragma unroll
    for (int m = 0; m < FM_PER; ++m) {
        const int i = tid + m * FM_THREADS;
        y[i] = __fmul_rn(__fmul_rn(w[m], cr[fm_p(i)]), (float)(2.0 / 3.0 / VV_FM_N));
    }
}

__global__ __launch_bounds__(FM_THREADS) void vv_formant_sum_kernel(VVFmRows rows, float* __restrict__ hist, float* __restrict__ tail,
                                                                   const float* __restrict__ x, int ld_in, float* __restrict__ out, int ld_out,
                                                                   const float* __restrict__ scratch, int cap_frames, int blocks_per_wg) {
    const VVFmRow r = rows.r[blockIdx.y];                       // uniform index into the kernel arguments
    const int tid = threadIdx.x;
    const float* xrow = x + (size_t)blockIdx.y * ld_in;
    float* orow = out + (size_t)blockIdx.y * ld_out;
    if (r.A == r.B) {                                           // the identity: the chunk as it is
        for (int64_t i = (int64_t)blockIdx.x * FM_THREADS + tid; i < r.n_out; i += (int64_t)gridDim.x * FM_THREADS) orow[i] = xrow[i];
        return;
    }
    const bool st = hist != nullptr;                            // a stream: one workgroup per row (gridDim.x == 1)
    float* hrow = st ? hist + (size_t)r.stream * VV_FM_HIST : nullptr;
    float* trow = st ? tail + (size_t)r.stream * VV_FM_TAIL : nullptr;
    float t3[3] = {0.f, 0.f, 0.f}, hn[FM_PER];
    if (st) {
#pragma unroll
        for (int s = 0; s < 3; ++s) t3[s] = trow[s * VV_FM_H + tid];
#pragma unroll
        for (int m = 0; m < FM_PER; ++m) {                      // the last N samples of history | chunk
            const int src = tid + m * FM_THREADS + r.n_in;
            hn[m] = src < VV_FM_HIST ? hrow[src] : xrow[src - VV_FM_HIST];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < FM_PER; ++m) hrow[tid + m * FM_THREADS] = hn[m];
    }
    const float* sc = scratch + (size_t)blockIdx.y * cap_frames * VV_FM_N;
    const int c0 = blockIdx.x * blocks_per_wg, c1 = min(c0 + blocks_per_wg, r.nf + 3);
    for (int c = c0; c < c1; ++c) {
        float acc = c < 3 ? t3[c] : 0.f;
        const int f1 = min(c, r.nf - 1);
        for (int f = max(c - 3, 0); f <= f1; ++f) acc = __fadd_rn(acc, sc[(size_t)f * VV_FM_N + (c - f) * VV_FM_H + tid]);
        if (c < r.nf) {
            const int o = (c - r.c_min) * VV_FM_H + tid;
            if (c >= r.c_min && o < r.n_out) orow[o] = acc;
        } else if (st) trow[(c - r.nf) * VV_FM_H + tid] = acc;
    }
}

// zero the history and the partial sums of up to 16 streams (a kernel, not a memset node: DESIGN.md section 8)
struct FmIds { int id[16]; };
__global__ void vv_formant_reset_kernel(float* __restrict__ hist, float* __restrict__ tail, FmIds ids) {
    float* hrow = hist + (size_t)ids.id[blockIdx.x] * VV_FM_HIST;
    float* trow = tail + (size_t)ids.id[blockIdx.x] * VV_FM_TAIL;
    for (int i = threadIdx.x; i < VV_FM_HIST; i += blockDim.x) hrow[i] = 0.f;
    for (int i = threadIdx.x; i < VV_FM_TAIL; i += blockDim.x) trow[i] = 0.f;
}

}  // namespace

// The callers (vv_formant_rows, vv_formant_once, engine_codec.hip) have derived every row; what the kernels index with is checked again
// here against the buffers' bounds: -1, nothing launched.  hist and tail both set: streams; both null: whole signals (stream = -1).
extern "C" int vv_formant_rows_launch(const VVFmRows* rows, int n, const float* tw, float* hist, float* tail, int n_streams, const float* x, int ld_in,
                                      float* out, int ld_out, float* scratch, int cap_frames, hipStream_t s) {
    if (!rows || !tw || !out || !scratch || n < 1 || n > 16 || cap_frames < 1 || (hist == nullptr) != (tail == nullptr)) return -1;
    int max_nf = 0;
    for (int i = 0; i < n; ++i) {
        const VVFmRow& r = rows->r[i];
        if (hist) {
            if (r.stream < 0 || r.stream >= n_streams) return -1;
            for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
            if (r.nf > VV_FM_MAX_FRAMES) return -1;
        } else if (r.stream != -1 || r.r != 0 || r.c_min != 3) return -1;
        if (r.n_in < 0 || r.n_in > ld_in || (r.n_in > 0 && !x) || r.n_out < 0 || r.n_out > ld_out) return -1;
        if (!vv_fm_ratio_ok(r.A, r.B) || r.nf < 0 || r.nf > cap_frames || r.r < 0 || r.r >= VV_FM_H || r.c_min < 0 || r.c_min > 3) return -1;
        if ((int64_t)r.nf * VV_FM_H >= ((int64_t)1 << 31) - 2 * VV_FM_N) return -1;
        if (r.A == r.B ? (r.nf != 0 || r.n_out > r.n_in) : (int64_t)r.n_out > (int64_t)std::max(0, r.nf - r.c_min) * VV_FM_H) return -1;
        max_nf = std::max(max_nf, r.nf);
    }
    VVFmRows a = *rows;
    for (int i = n; i < 16; ++i) a.r[i] = a.r[0];
    if (max_nf > 0)
        hipLaunchKernelGGL(vv_formant_frames_kernel, dim3(max_nf, n), dim3(FM_THREADS), 0, s, a, tw, hist, x, ld_in, scratch, cap_frames);
    const int bpw = hist ? max_nf + 3 : FM_ONCE_BLOCKS;
    hipLaunchKernelGGL(vv_formant_sum_kernel, dim3(hist ? 1 : (max_nf + 3 + bpw - 1) / bpw, n), dim3(FM_THREADS), 0, s, a, hist, tail, x, ld_in, out, ld_out,
                       scratch, cap_frames, bpw);
    return vv_launch_rc(0);
}

extern "C" int vv_formant_reset_launch(float* hist, float* tail, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!hist || !tail || !ids || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    FmIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_formant_reset_kernel, dim3(n), dim3(256), 0, s, hist, tail, a);
    return vv_launch_rc(0);
}
