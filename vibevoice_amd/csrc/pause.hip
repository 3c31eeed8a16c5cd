// pause.hip -- cap the silences of a stream and trim its lead-in (vibevoice_amd/pause.py is the definition).  In segments of seg = rate / 100
// samples, every decision an integer one:
//   q = clamp(rint(fl(x 32768)), +-32768), a non-finite x counts as 0;   E = sum q^2 over the segment;   quiet iff E < theta
//   with the cap C in force (C0 in front of the stream's first loud segment, C behind it), T = min(C / 2, 10), H = C - T, a quiet run of R
//   segments: the first H go out as they arrive, from segment H + 1 on the last T are held back and segment H + 1 is kept (`first`); the next
//   loud segment, or the flush, releases them: verbatim where R <= C; where R > C, (R - C) seg samples are dropped and the oldest held
//   segment b goes out as fl(fl(first[j] u[j]) + fl(b[j] w[j])), the rest verbatim.  Samples short of a segment wait; the flush emits them.
// Sums of integers do not depend on their order and the join is three single roundings: the kernels are held to the definition with no
// tolerance.  What a push emits depends on the data, so the count is the kernel's to write, into device memory.
//
// Both kernels run ps_push, 256 threads, over one LDS buffer [the stream's open segment | the chunk || the ring as it was || first as it was]:
//   1. stage it, barrier: every word of the stream's state this push needs has been read before any is written (a ring slot this push
//      releases and refills is safe), and every segment has ONE address in LDS whether it came with this push or an earlier one (a segment
//      held and released inside one push is read from the chunk, never from a ring slot nobody has written);
//   2. one wave per segment sums q^2 (64-bit, exact in any order) and writes the segment's flag;
//   3. one thread walks the flags in order and writes the copy plan: for each emitted segment where it comes from and, for a join, where
//      `first` comes from; where the held segments and `first` now come from; the counters;
//   4. all threads copy by the plan: fp32 as it is, or 16-bit with the rule of vv_device.h (vv_block_peak, vv_pcm16_of) over the row's own
//      emitted samples;
//   5. all threads write the open segment, the ring (oldest first from slot 0) and `first` back: plain vector stores.
// vv_pause_rows_kernel (streaming): ONE workgroup per row of the push, the rows by value in the kernel arguments (VVPsRows, vv_common.h).
// vv_pause_once_kernel (stateless, whole signals): one workgroup per signal walks it in pushes of VV_PS_MAX_IN samples, the counters in
// LDS, the samples a stream keeps in the caller's scratch: the same code, so the same bits as push + flush.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int PS_THREADS = 256, PS_WAVES = PS_THREADS / 64;
constexpr int PS_STAGE = VV_PS_MAX_IN + VV_PS_MAX_SEG;                 // >= (seg - 1) + n_in
constexpr int PS_RING = PS_STAGE, PS_FIRST = PS_RING + VV_PS_MAX_T * VV_PS_MAX_SEG, PS_BUF = PS_FIRST + VV_PS_MAX_SEG;
constexpr int PS_PLAN = VV_PS_MAX_SEGS + VV_PS_MAX_T;                  // segments one push emits at most

struct PsLds {
    float buf[PS_BUF];
    int src[PS_PLAN];                   // where emitted segment d starts in buf
    int jn[PS_PLAN];                    // ... and, for a join, where `first` does; -1: verbatim
    int quiet[VV_PS_MAX_SEGS];
    int hsrc[VV_PS_MAX_T];              // where the held segments start in buf, oldest first
    int n_plan, n_out, n_held, fsrc;
    VVPsState st;
    float wmx[PS_WAVES];
};
static_assert(sizeof(PsLds) <= 65536, "static LDS");

__device__ __forceinline__ int ps_quant(float x) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) return 0;      // inf or NaN
    return __float2int_rn(fminf(fmaxf(__fmul_rn(x, 32768.0f), -32768.0f), 32768.0f));
}

// three roundings: the products must not fuse with the sum (the compiler contracts a * b + c by default)
__device__ __forceinline__ float ps_join(float a, float b, float u, float w) {
#pragma clang fp contract(off)
    const float p = a * u, q = b * w;
    return p + q;
}

// the held segments go out (one thread): the plan grows by them, the run's surplus is counted
__device__ void ps_release(PsLds& l, int cap, int seg) {
    const bool cut = l.st.run > cap;
    if (cut) l.st.dropped += (long long)(l.st.run - cap) * seg;
    for (int i = 0; i < l.n_held; ++i) {
        l.src[l.n_plan] = l.hsrc[i];
        l.jn[l.n_plan] = cut && i == 0 ? l.fsrc : -1;
        ++l.n_plan;
    }
    l.n_held = 0;
}

__device__ __forceinline__ float ps_value(const PsLds& l, const float* __restrict__ wt, int seg, int n_whole, int tail_at, int idx) {
    if (idx >= n_whole) return l.buf[tail_at + idx - n_whole];              // the partial segment a flush emits
    const int d = idx / seg, j = idx - d * seg, a = l.jn[d];
    const float b = l.buf[l.src[d] + j];
    return a < 0 ? b : ps_join(l.buf[a + j], b, wt[seg + j], wt[j]);
}

// One push of one stream.  lds.st holds the stream's counters (published by a barrier); sbuf its VV_PS_FLOATS samples; wt [2][seg]: w, u.
// On return lds.st and lds.n_out are the new counters and what the push emitted (thread 0 wrote them, no barrier behind it).
__device__ void ps_push(PsLds& lds, const VVPsRow& r, float* __restrict__ sbuf, const float* __restrict__ wt, const float* __restrict__ xr,
                        float* __restrict__ of, short* __restrict__ oh) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, seg = r.seg;
    const int tot = r.carry + r.n_in, n_seg = tot / seg, rem = tot - n_seg * seg;
    const int held = min(max(lds.st.held, 0), VV_PS_MAX_T);
    // 1.
    for (int b = tid; b < tot; b += PS_THREADS) lds.buf[b] = b < r.carry ? sbuf[b] : xr[b - r.carry];
    if (held > 0) {
        for (int b = tid; b < held * seg; b += PS_THREADS) lds.buf[PS_RING + b] = sbuf[VV_PS_RING_AT + b];
        for (int b = tid; b < seg; b += PS_THREADS) lds.buf[PS_FIRST + b] = sbuf[VV_PS_FIRST_AT + b];
    }
    __syncthreads();
    // 2.
    for (int s = wv; s < n_seg; s += PS_WAVES) {
        long long e = 0;
        for (int j = lane; j < seg; j += 64) { const int q = ps_quant(lds.buf[s * seg + j]); e += (long long)(q * q); }
        e = vv_wave_sum(e);
        if (lane == 0) lds.quiet[s] = e < r.theta;
    }
    __syncthreads();
    // 3.
    if (tid == 0) {
        lds.n_plan = 0; lds.n_held = held; lds.fsrc = PS_FIRST;
        for (int i = 0; i < held; ++i) lds.hsrc[i] = PS_RING + i * seg;
        for (int s = 0; s < n_seg; ++s) {
            const int cap = lds.st.started ? r.C : r.C0, T = min(cap / 2, VV_PS_MAX_T), H = cap - T;
            if (lds.quiet[s]) {
                if (lds.st.run < 0x7fffffff) ++lds.st.run;
                if (lds.st.run <= H) { lds.src[lds.n_plan] = s * seg; lds.jn[lds.n_plan] = -1; ++lds.n_plan; }
                else {
                    if (lds.st.run == H + 1) lds.fsrc = s * seg;
                    if (T > 0) {
                        while (lds.n_held >= T) {                     // the oldest one leaves
                            for (int i = 1; i < lds.n_held; ++i) lds.hsrc[i - 1] = lds.hsrc[i];
                            --lds.n_held;
                        }
                        lds.hsrc[lds.n_held++] = s * seg;
                    }
                }
            } else {
                ps_release(lds, cap, seg);
                lds.src[lds.n_plan] = s * seg; lds.jn[lds.n_plan] = -1; ++lds.n_plan;
                lds.st.run = 0; lds.st.started = 1;
            }
        }
        if (r.flush) ps_release(lds, lds.st.started ? r.C : r.C0, seg);
        lds.n_out = lds.n_plan * seg + (r.flush ? rem : 0);
        lds.st.held = lds.n_held;
        lds.st.tin += r.n_in; lds.st.tout += lds.n_out;
    }
    __syncthreads();
    // 4.
    const int n_whole = lds.n_plan * seg, n_out = lds.n_out, tail_at = n_seg * seg;
    if (!oh) {
        for (int i = tid; i < n_out; i += PS_THREADS) of[i] = ps_value(lds, wt, seg, n_whole, tail_at, i);
    } else {
        float mx = 0.f;
        for (int i = tid; i < n_out; i += PS_THREADS) mx = fmaxf(mx, fabsf(ps_value(lds, wt, seg, n_whole, tail_at, i)));
        const float peak = vv_block_peak<PS_WAVES>(mx, lds.wmx);
        for (int i = tid; i < n_out; i += PS_THREADS) oh[i] = vv_pcm16_of(ps_value(lds, wt, seg, n_whole, tail_at, i), peak);
    }
    // 5. every source is in LDS: the order of these stores does not matter
    const int n_held = lds.n_held;
    for (int b = tid; b < n_held * seg; b += PS_THREADS) { const int i = b / seg; sbuf[VV_PS_RING_AT + b] = lds.buf[lds.hsrc[i] + b - i * seg]; }
    if (lds.fsrc != PS_FIRST) for (int b = tid; b < seg; b += PS_THREADS) sbuf[VV_PS_FIRST_AT + b] = lds.buf[lds.fsrc + b];
    if (!r.flush) for (int b = tid; b < rem; b += PS_THREADS) sbuf[b] = lds.buf[tail_at + b];
}

__global__ __launch_bounds__(PS_THREADS) void vv_pause_rows_kernel(VVPsRows rows, float* __restrict__ sbuf, VVPsState* __restrict__ state,
                                                                  const float* __restrict__ wt, const float* __restrict__ x, int ld_in,
                                                                  void* __restrict__ out, int ld_out, int pcm16, int* __restrict__ counts) {
    __shared__ PsLds lds;
    const VVPsRow r = rows.r[blockIdx.x];                       // uniform index into the kernel arguments
    VVPsState* st = state + r.stream;
    if (threadIdx.x == 0) lds.st = *st;
    __syncthreads();
    ps_push(lds, r, sbuf + (size_t)r.stream * VV_PS_FLOATS, wt, x + (size_t)blockIdx.x * ld_in,
            pcm16 ? nullptr : (float*)out + (size_t)blockIdx.x * ld_out, pcm16 ? (short*)out + (size_t)blockIdx.x * ld_out : nullptr);
    if (threadIdx.x == 0) { *st = lds.st; counts[blockIdx.x] = lds.n_out; }
}

// signal blockIdx.x of n_in samples in pushes of VV_PS_MAX_IN, the last one its flush; counts [n][2]: what it emitted and what it dropped
__global__ __launch_bounds__(PS_THREADS) void vv_pause_once_kernel(int seg, int C, int C0, long long theta, const float* __restrict__ wt, int n_in,
                                                                  const float* __restrict__ x, int ld_in, float* __restrict__ out, int ld_out,
                                                                  float* __restrict__ scratch, int* __restrict__ counts) {
    __shared__ PsLds lds;
    if (threadIdx.x == 0) lds.st = VVPsState{0, 0, 0, 0, 0, 0, 0};
    __syncthreads();
    const float* xr = x + (size_t)blockIdx.x * ld_in;
    float* orow = out + (size_t)blockIdx.x * ld_out;
    for (int at = 0;; at += VV_PS_MAX_IN) {
        VVPsRow r;
        r.stream = 0; r.n_in = min(VV_PS_MAX_IN, n_in - at); r.flush = at + r.n_in >= n_in; r.carry = at % seg;
        r.seg = seg; r.C = C; r.C0 = C0; r.pad = 0; r.theta = theta;
        const long long o0 = lds.st.tout;                      // <= at: never more out than in
        ps_push(lds, r, scratch + (size_t)blockIdx.x * VV_PS_ONCE_FLOATS, wt, xr + at, orow + o0, nullptr);
        __syncthreads();                                        // the next push reads what this one stored, and restages the buffer
        if (r.flush) break;
    }
    if (threadIdx.x == 0) { counts[2 * blockIdx.x] = (int)lds.st.tout; counts[2 * blockIdx.x + 1] = (int)lds.st.dropped; }
}

// the counters of up to 16 streams to zero: with nothing held and no open segment the stream's samples are never read
struct PsIds { int id[16]; };
__global__ void vv_pause_reset_kernel(VVPsState* __restrict__ state, PsIds ids) {
    int* st = (int*)(state + ids.id[blockIdx.x]);
    for (int i = threadIdx.x; i < (int)(sizeof(VVPsState) / 4); i += blockDim.x) st[i] = 0;
}

}  // namespace

// The caller (vv_pause_rows, engine_codec.hip) has derived every row from its stream's counter and parameters; what the kernel indexes
// with is checked again here against the buffers' bounds: -1, nothing launched.
extern "C" int vv_pause_rows_launch(const VVPsRows* rows, int n, int seg, float* sbuf, VVPsState* state, int n_streams, const float* wt,
                                    const float* x, int ld_in, void* out, int ld_out, int pcm16, int* counts, hipStream_t s) {
    if (!rows || !sbuf || !state || !wt || !out || !counts || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) {
        const VVPsRow& r = rows->r[i];
        for (int j = 0; j < i; ++j) if (rows->r[j].stream == r.stream) return -1;
        if (r.stream < 0 || r.stream >= n_streams || r.n_in < 0 || r.n_in > VV_PS_MAX_IN || r.n_in > ld_in || (r.n_in > 0 && !x)) return -1;
        if (r.seg != seg || !vv_ps_params_ok(r.seg, r.C, r.C0, r.theta) || r.carry < 0 || r.carry >= r.seg) return -1;
        if ((long long)r.n_in + (r.seg - 1) + (long long)VV_PS_MAX_T * r.seg > ld_out) return -1;      // the most any state lets a push emit
    }
    hipLaunchKernelGGL(vv_pause_rows_kernel, dim3(n), dim3(PS_THREADS), 0, s, *rows, sbuf, state, wt, x, ld_in, out, ld_out, pcm16, counts);
    return vv_launch_rc(0);
}

// n signals of n_in samples -> at most n_in outputs each; scratch [n][VV_PS_ONCE_FLOATS], counts [n][2]
extern "C" int vv_pause_once_launch(int seg, int C, int C0, long long theta, const float* wt, int n, int n_in, const float* x, int ld_in, float* out,
                                    int ld_out, float* scratch, int* counts, hipStream_t s) {
    if (!wt || !x || !out || !scratch || !counts || n < 1 || n > 65535 || n_in < 1 || n_in > ld_in || n_in > ld_out) return -1;
    if (!vv_ps_params_ok(seg, C, C0, theta)) return -1;
    hipLaunchKernelGGL(vv_pause_once_kernel, dim3(n), dim3(PS_THREADS), 0, s, seg, C, C0, theta, wt, n_in, x, ld_in, out, ld_out, scratch, counts);
    return vv_launch_rc(0);
}

extern "C" int vv_pause_reset_launch(VVPsState* state, int n_streams, const int* ids, int n, hipStream_t s) {
    if (!state || !ids || n < 1 || n > 16) return -1;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_streams) return -1;
    PsIds a;
    for (int i = 0; i < 16; ++i) a.id[i] = ids[i < n ? i : 0];
    hipLaunchKernelGGL(vv_pause_reset_kernel, dim3(n), dim3(64), 0, s, state, a);
    return vv_launch_rc(0);
}
