// pitch.hip -- variable-ratio band-limited resampling P / Q, every row of a launch at its own ratio over ONE prototype table
// (vibevoice_amd/pitch.py is the definition and designs the table): output m is the input at time m * P / Q, the input taken as zero
// outside itself.  With den = max(P, Q), rho = fl(Q / den), k = m * P, q = k / Q, a = k % Q, Tn = ceil(32 * den / Q) <= 64:
//     y[m] = sum_{t = -Tn .. Tn} fl(rho * c(a, t)) * x[q - t],   fmaf in that order from 0,
//     c(a, t): num = |a + t * Q| * R, i = num / den, f = fl((num % den) / den), c = fmaf(f, fl(H[i + 1] - H[i]), H[i]) where i < 32 * R, else 0
// -- one rounding sequence (pt_output), so the streaming kernel and the one-shot kernel give the same bits for the same m.  1 / 1 is the
// identity (Tn = 0, c = 1).  The table position advances by Q * R / den per tap, exactly, as a quotient and a remainder: two integer
// divisions per output, none per tap; the den values of f come from a small LDS table filled with one IEEE division each.
//
// vv_pitch_rows_kernel (streaming, chunk-continuous): ONE workgroup of 1024 threads per row of the push.  It stages the table H
// [32 * R + 1] in LDS, entry i at i + i / 32: lanes read it at a stride of about R * Q / den, and at a power-of-two den the plain layout
// would put every lane of a ds_read_b32 group (32 banks) on one bank; the skew spreads strides of 16, 32, 64, 128 over distinct banks.
// Beside it: the row's f table, the stream's 128 history samples, the chunk and 64 zeros (read by a flush only).  After the barrier it
// writes the stream's new history (the last 128 staged samples: every read of the old row is done) and each thread forms up to 8
// outputs, j = thread + 1024 * i, in registers.  Float rows are stored as they are; 16-bit rows with the rule of vv_device.h
// (vv_block_peak, vv_pcm16_of) over the row's chunk, in the same launch.  The rows travel by value in the kernel arguments
// (VVPitchRows, vv_common.h); a row's stream is distinct from every other row's.  64 KiB of LDS at most: the default limit.
//
// vv_pitch_once_kernel (stateless, whole signals): outputs tiled over workgroups, table and input read from global memory, the ratio
// of each of up to 16 signals in the kernel arguments.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int PT_THREADS = 1024, PT_PER = VV_PT_MAX_OUT / PT_THREADS;
constexpr int PT_LDS_MAX = 65536 - 64;      // the default limit less the peak words below: no hipFuncSetAttribute
constexpr int PT_FTAB = 128;                // >= den: f of every remainder

__host__ __device__ __forceinline__ int pt_sk(int i) { return i + (i >> 5); }
__device__ __forceinline__ int pt_taps(int P, int Q) { return P == Q ? 0 : (VV_PT_Z * (P > Q ? P : Q) + Q - 1) / Q; }   // vv_pt_taps, on the device

template <bool SKEW>
__device__ __forceinline__ float pt_coef(const float* __restrict__ H, const float* __restrict__ ftab, int i, int rem, int ZR) {
    const int ic = i < ZR ? i : ZR - 1;
    const float h0 = H[SKEW ? pt_sk(ic) : ic], h1 = H[SKEW ? pt_sk(ic + 1) : ic + 1];
    const float c = fmaf(ftab[rem], __fsub_rn(h1, h0), h0);
    return i < ZR ? c : 0.f;
}

// one output at phase a; xat(t) = x[q - t].  H: the table (SKEW: the LDS layout), ftab[r] = fl(r / den)
template <bool SKEW, class X>
__device__ __forceinline__ float pt_output(const float* __restrict__ H, const float* __restrict__ ftab, int R, int P, int Q, int a, X xat) {
    if (P == Q) return fmaf(1.f, xat(0), 0.f);
    const int den = P > Q ? P : Q, Tn = pt_taps(P, Q), ZR = VV_PT_Z * R;
    const int dq = (Q * R) / den, dr = Q * R - dq * den;            // the position's step per tap
    const float rho = __fdiv_rn((float)Q, (float)den);
    float acc = 0.f;
    int num = (Tn * Q - a) * R, i = num / den, rem = num - i * den;   // t = -Tn .. -1: |a + t Q| = |t| Q - a, descending
    for (int t = -Tn; t < 0; ++t) {
        acc = fmaf(__fmul_rn(rho, pt_coef<SKEW>(H, ftab, i, rem, ZR)), xat(t), acc);
        i -= dq; rem -= dr;
        if (rem < 0) { rem += den; --i; }
    }
    num = a * R; i = num / den; rem = num - i * den;                  // t = 0 .. Tn: a + t Q, ascending
    for (int t = 0; t <= Tn; ++t) {
        acc = fmaf(__fmul_rn(rho, pt_coef<SKEW>(H, ftab, i, rem, ZR)), xat(t), acc);
        i += dq; rem += dr;
        if (rem >= den) { rem -= den; ++i; }
    }
    return acc;
}

__device__ __forceinline__ void pt_fill_ftab(float* ftab, int den) {
    if (threadIdx.x < PT_FTAB) ftab[threadIdx.x] = (int)threadIdx.x < den ? __fdiv_rn((float)threadIdx.x, (float)den) : 0.f;
}

__global__ __launch_bounds__(PT_THREADS) void vv_pitch_rows_kernel(VVPitchRows rows, const float* __restrict__ table, int R,
                                                                  float* __restrict__ hist, const float* __restrict__ x, int ld_in,
                                                                  void* __restrict__ out, int ld_out, int pcm16) {
    extern __shared__ float pt_lds[];
    __shared__ float wmx[PT_THREADS / 64];
    const VVPitchRow r = rows.r[blockIdx.x];                    // uniform index into the kernel arguments
    const int tid = threadIdx.x, nt = VV_PT_Z * R + 1;
    float* H = pt_lds;                                          // [pt_sk(nt - 1) + 1], entry i at pt_sk(i)
    float* ftab = pt_lds + pt_sk(nt - 1) + 1;                   // [PT_FTAB]
    float* buf = ftab + PT_FTAB;                                // [VV_PT_HIST | n_in | VV_PT_MAX_TN]
    for (int i = tid; i < nt; i += PT_THREADS) H[pt_sk(i)] = table[i];
    pt_fill_ftab(ftab, r.P > r.Q ? r.P : r.Q);
    float* hrow = hist + (size_t)r.stream * VV_PT_HIST;
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    for (int i = tid; i < VV_PT_HIST; i += PT_THREADS) buf[i] = hrow[i];
    for (int i = tid; i < r.n_in; i += PT_THREADS) buf[VV_PT_HIST + i] = xr[i];
    for (int i = tid; i < VV_PT_MAX_TN; i += PT_THREADS) buf[VV_PT_HIST + r.n_in + i] = 0.f;
    __syncthreads();
    for (int i = tid; i < VV_PT_HIST; i += PT_THREADS) hrow[i] = buf[r.n_in + i];

    float acc[PT_PER];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < PT_PER; ++i) {
        const int j = tid + i * PT_THREADS;
        float v = 0.f;
        if (j < r.n_out) {
            const int kk = r.a0 + j * r.P, dq = kk / r.Q, a = kk - dq * r.Q;
            const float* b = buf + r.b0 + dq;
            v = pt_output<true>(H, ftab, R, r.P, r.Q, a, [b](int t) { return b[-t]; });
        }
        acc[i] = v;
        mx = fmaxf(mx, fabsf(v));
    }
    if (!pcm16) {
        float* orow = (float*)out + (size_t)blockIdx.x * ld_out;
#pragma unroll
        for (int i = 0; i < PT_PER; ++i) { const int j = tid + i * PT_THREADS; if (j < r.n_out) orow[j] = acc[i]; }
        return;
    }
    const float peak = vv_block_peak<PT_THREADS / 64>(mx, wmx);
    short* orow = (short*)out + (size_t)blockIdx.x * ld_out;
#pragma unroll
    for (int i = 0; i < PT_PER; ++i) { const int j = tid + i * PT_THREADS; if (j < r.n_out) orow[j] = vv_pcm16_of(acc[i], peak); }
}

__global__ __launch_bounds__(256) void vv_pitch_once_kernel(VVPitchRatios pq, const float* __restrict__ table, int R, int n_in,
                                                           const float* __restrict__ x, int ld_in, float* __restrict__ out, int ld_out) {
    __shared__ float ftab[PT_FTAB];
    const int P = pq.P[blockIdx.y], Q = pq.Q[blockIdx.y];      // uniform index into the kernel arguments
    pt_fill_ftab(ftab, P > Q ? P : Q);
    __syncthreads();
    const int64_t n_out = ((int64_t)n_in * Q + P - 1) / P;
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    const int64_t k = m * P;
    const int q = (int)(k / Q), a = (int)(k - (int64_t)q * Q);
    const float* xr = x + (size_t)blockIdx.y * ld_in;
    out[(size_t)blockIdx.y * ld_out + m] =
        pt_output<false>(table, ftab, R, P, Q, a, [=](int t) { const int i = q - t; return (i >= 0 && i < n_in) ? xr[i] : 0.f; });
}

// zero the history rows of up to 16 streams (a kernel, not a memset node: DESIGN.md section 8)
struct PtIds { int id[16]; };
__global__ void vv_pitch_reset_kernel(float* __restrict__ hist, PtIds ids) {
    float* hrow = hist + (size_t)ids.id[blockIdx.x] * VV_PT_HIST;
    for (int i = threadIdx.x; i < VV_PT_HIST; i += blockDim.x) hrow[i] = 0.f;
}

}  // namespace

extern "C" int vv_pitch_lds_bytes(int R, int n_in) {
    if (R < 1 || R > VV_PT_MAX_R || n_in < 0) return 0x7fffffff;
    const int64_t b = ((int64_t)pt_sk(VV_PT_Z * R) + 1 + PT_FTAB + VV_PT_HIST + (int64_t)n_in + VV_PT_MAX_TN) * 4;
    return b > 0x7fffffff ? 0x7fffffff : (int)b;
}

// The caller (vv_pitch_rows, engine_codec.hip) has derived every row from its stream's counter; what the kernel indexes with is
// checked again here against the staging buffer's bounds: -1, nothing launched.
extern "C" int vv_pitch_rows_launch(const VVPitchRows* rows, int n, const float* table, int R, float* hist, int n_streams, const float* x,
                                    int ld_in, void* out, int ld_out, int pcm16, hipStream_t s) {
    if (!rows || !table || !hist || !out || n < 1 || n > 16 || R < 1 || R > VV_PT_MAX_R) return -1;
    int max_in = 0;
    for (int i = 0; i < n; ++i) {
        const VVPitchRow& r = rows->r[i];
        for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
        if (r.stream < 0 || r.stream >= n_streams || r.n_in < 0 || r.n_in > ld_in || r.n_in > VV_PT_MAX_IN) return -1;
        if (r.n_out < 0 || r.n_out > VV_PT_MAX_OUT || r.n_out > ld_out) return -1;
        if (r.n_in > 0 && !x) return -1;
        if (!vv_pt_ratio_ok(r.P, r.Q) || r.a0 < 0 || r.a0 >= r.Q) return -1;
        if (r.n_out > 0) {
            const int Tn = vv_pt_taps(r.P, r.Q);
            const int64_t last = (int64_t)r.b0 + ((int64_t)r.a0 + (int64_t)(r.n_out - 1) * r.P) / r.Q;
            if ((int64_t)r.b0 - Tn < 0 || last + Tn >= (int64_t)VV_PT_HIST + r.n_in + VV_PT_MAX_TN) return -1;
        }
        max_in = r.n_in > max_in ? r.n_in : max_in;
    }
    const int lds = vv_pitch_lds_bytes(R, max_in);
    if (lds > PT_LDS_MAX) return -1;
    hipLaunchKernelGGL(vv_pitch_rows_kernel, dim3(n), dim3(PT_THREADS), lds, s, *rows, table, R, hist, x, ld_in, out, ld_out, pcm16);
    return vv_launch_rc(0);
}

// n <= 16 signals of n_in samples, signal i at pq->P[i] / pq->Q[i] -> ceil(n_in * Q / P) outputs
extern "C" int vv_pitch_once_launch(const float* table, int R, const VVPitchRatios* pq, int n, int n_in, const float* x, int ld_in, float* out,
                                    int ld_out, hipStream_t s) {
    if (!table || !pq || !x || !out || n < 1 || n > 16 || n_in < 1 || n_in > ld_in || R < 1 || R > VV_PT_MAX_R) return -1;
    int64_t most = 0;
    for (int i = 0; i < n; ++i) {
        if (!vv_pt_ratio_ok(pq->P[i], pq->Q[i])) return -1;
        const int64_t n_out = ((int64_t)n_in * pq->Q[i] + pq->P[i] - 1) / pq->P[i];
        if (n_out > ld_out) return -1;
        most = n_out > most ? n_out : most;
    }
    if (most >= ((int64_t)1 << 31) - 256 || (int64_t)n_in + VV_PT_MAX_TN >= ((int64_t)1 << 31)) return -1;
    VVPitchRatios a = *pq;
    for (int i = n; i < 16; ++i) { a.P[i] = a.P[0]; a.Q[i] = a.Q[0]; }
    hipLaunchKernelGGL(vv_pitch_once_kernel, dim3((unsigned)((most + 255) / 256), n), dim3(256), 0, s, a, table, R, n_in, x, ld_in, out, ld_out);
    return vv_launch_rc(0);
}

extern "C" int vv_pitch_reset_launch(float* hist, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!hist || !ids || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    PtIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_pitch_reset_kernel, dim3(n), dim3(64), 0, s, hist, a);
    return vv_launch_rc(0);
}
