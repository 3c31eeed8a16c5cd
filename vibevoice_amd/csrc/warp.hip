// warp.hip -- the reference's full-vocabulary logits processors, evaluated for the <= 16 valid ids only.
//
// HF's list in front of the valid-token constraint (modeling_vibevoice_inference.py:310-319, 416-419): repetition penalty, then with
// do_sample temperature -> top-k -> top-p -> min-p.  Only the valid ids are ever read back, and for those every processor is a
// reduction over the row: with s[j] the penalised / tempered score, m = max s, e[j] = exp(s[j] - m),
//   top-k   v survives iff #{j : s[j] > s[v]} < k                (equivalently s[v] >= tau, tau the k-th largest value)
//   top-p   v is removed iff A[v] <= (1 - top_p) Z,  Z = sum_{j in T} e[j],  A[v] = sum_{j in T, s[j] <= s[v]} e[j],  T = {s >= tau}
//   min-p   v is removed iff exp(s[v] - m) < min_p
// and the row's maximum is never removed by top-p / min-p.  No sort, nothing of size V is written.
//
// One workgroup of 16 waves per row; the row (4 V bytes, 600 KB at V = 152064: more than the LDS) is streamed from L2 once per pass:
//   pass A   max, the per-token counts (top-k without top-p) and the first radix digit's histogram (top-k with top-p)
//   select   two more passes: exact radix select of tau on order-preserving 32-bit keys, digits of 11 / 11 / 10 bits, one LDS histogram
//            per wave (lanes of different waves never meet on a counter), summed once per digit
//   final    Z and A[v] (top-p only): fp32 partials per thread, combined in fp64 in a fixed order -> bit-identical run to run
// so a row costs 0 (no sampling), 1 (top-k and/or min-p), 2 (top-p) or 4 (top-k + top-p) passes of 4 V bytes.
#include "vv_common.h"
#include "vv_device.h"
#include "vv_launch.h"

namespace {

constexpr int WV_THREADS = 1024;
constexpr int WV_WAVES = WV_THREADS / VV_WAVE;
constexpr int WV_BINS = 2048;                                  // 11-bit digit
constexpr size_t WV_HIST_BYTES = (size_t)WV_WAVES * WV_BINS * sizeof(unsigned);

struct VVWarpIds { int n; int id[16]; };
struct VVWarpArgs {
    float pen, temp, top_p, min_p;
    int pen_on, temp_on, do_sample, top_k;
};

// float order == unsigned order of the key (-0 sorts just below +0; membership tests below compare floats, where they are equal)
__device__ __forceinline__ unsigned wv_key(float s) {
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float wv_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct WvRow {
    const float* l;               // the row's logits
    const unsigned char* seen;    // the row's seen bytes (null: no penalty)
    int V;
    float pen, temp;
    bool pen_on, temp_on;
    // RepetitionPenaltyLogitsProcessor then TemperatureLogitsWarper, torch's arithmetic: IEEE fp32 multiply / divide
    __device__ __forceinline__ float score(float x, unsigned seen_byte) const {
        if (pen_on && seen_byte) x = x < 0.f ? x * pen : x / pen;
        if (temp_on) x = x / temp;
        return x;
    }
    __device__ __forceinline__ float at(int j) const { return score(l[j], pen_on ? seen[j] : 0u); }
};

// f(score) for every element of the row, a fixed set of elements in a fixed order per thread.  The row base is 16-byte aligned only
// when (row * V) % 4 == 0: up to 3 head elements and up to 3 tail elements go one by one, the rest as float4, four loads in flight
template <class F>
__device__ __forceinline__ void wv_for_row(const WvRow& r, int tid, F&& f) {
    const int V = r.V;
    int head = (int)((4u - (unsigned)(((uintptr_t)r.l >> 2) & 3u)) & 3u);
    if (head > V) head = V;
    if (tid < head) f(r.at(tid));
    const int nvec = (V - head) >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(r.l + head);
    for (int i0 = tid; i0 < nvec; i0 += 4 * WV_THREADS) {
        float4 x[4];
        unsigned sb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * WV_THREADS;
            x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            sb[u] = 0;
            if (i < nvec) {
                x[u] = p4[i];
                if (r.pen_on) {
                    const unsigned char* sp = r.seen + head + 4 * i;      // byte loads: the seen row is aligned no better than the logits
                    sb[u] = (unsigned)sp[0] | ((unsigned)sp[1] << 8) | ((unsigned)sp[2] << 16) | ((unsigned)sp[3] << 24);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u * WV_THREADS < nvec) {
                f(r.score(x[u].x, sb[u] & 0xffu));
                f(r.score(x[u].y, (sb[u] >> 8) & 0xffu));
                f(r.score(x[u].z, (sb[u] >> 16) & 0xffu));
                f(r.score(x[u].w, sb[u] >> 24));
            }
        }
    }
    const int t0 = head + 4 * nvec;
    if (tid < V - t0) f(r.at(t0 + tid));
}

// The digit that holds the k-th largest element: tot[0 .. nb) are the digit counts (LDS), k >= 1 and sum(tot) >= k.  Wave 0 only.
// Lane L owns nb / 64 bins from the top down; an inclusive scan over the lanes finds the owner of the crossing, which walks its bins.
__device__ __forceinline__ void wv_find_digit(const unsigned* tot, int nb, unsigned k, int lane, unsigned* out_digit, unsigned* out_k) {
    const int per = nb / VV_WAVE;
    const int hi = nb - 1 - per * lane;
    unsigned c = 0;
    for (int i = 0; i < per; ++i) c += tot[hi - i];
    unsigned P = c;
#pragma unroll
    for (int o = 1; o < VV_WAVE; o <<= 1) {
        const unsigned t = __shfl_up(P, o);
        if (lane >= o) P += t;
    }
    if (P >= k && P - c < k) {
        unsigned run = P - c;
        for (int i = 0; i < per; ++i) {
            const unsigned t = tot[hi - i];
            if (run + t >= k) {
                *out_digit = (unsigned)(hi - i);
                *out_k = k - run;
                break;
            }
            run += t;
        }
    }
}

__global__ __launch_bounds__(WV_THREADS) void vv_warp_valid_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ seen,
                                                                   float* __restrict__ out, int* __restrict__ survivors, int V,
                                                                   VVWarpIds ids, VVWarpArgs a) {
    extern __shared__ unsigned wv_hist[];              // [WV_WAVES][WV_BINS], the select path only (the launcher sizes it)
    __shared__ float sv_s[16];
    __shared__ float red_f[WV_WAVES];
    __shared__ unsigned red_u[WV_WAVES][16];
    __shared__ double red_d[WV_WAVES][17];
    __shared__ unsigned cnt_s[16];
    __shared__ double mass_s[17];
    __shared__ float m_s;
    __shared__ unsigned sel_digit, sel_k;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, nv = ids.n;
    WvRow r;
    r.l = logits + (int64_t)row * V;
    r.seen = (a.pen_on && seen) ? seen + (int64_t)row * V : nullptr;
    r.V = V;
    r.pen = a.pen; r.temp = a.temp;
    r.pen_on = a.pen_on != 0 && r.seen != nullptr;
    r.temp_on = a.temp_on != 0;
    const float NEG_INF = -__builtin_inff();

    // the valid tokens' own scores
    if (tid < 16) {
        int id = ids.id[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) id = (tid == i) ? ids.id[i] : id;      // select chain: no dynamic indexing of a kernel argument
        sv_s[tid] = tid < nv ? r.at(id) : __builtin_inff();
    }
    __syncthreads();
    float sv[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) sv[v] = sv_s[v];

    if (!a.do_sample) {                                 // penalty only: the valid scores are the answer
        if (tid < 64) {
            const bool fin = tid < nv && fabsf(sv_s[tid & 15]) < __builtin_inff();
            if (tid < nv) out[(int64_t)row * nv + tid] = sv_s[tid];
            const unsigned long long b = __ballot(fin);
            if (tid == 0) survivors[row] = __popcll(b);
        }
        return;
    }

    const int kk = a.top_k > 0 ? (a.top_k < V ? a.top_k : V) : 0;
    const bool topk_on = kk > 0 && kk < V;              // k >= V keeps everything
    const bool topp_on = a.top_p < 1.f;
    const bool minp_on = a.min_p > 0.f;
    const bool need_sel = topk_on && topp_on;
    const bool need_cnt = topk_on && !topp_on;
    const bool need_m = topp_on || minp_on;

    float m = 0.f, tau = NEG_INF;
    // ---------------- pass A: max, counts, first digit ----------------
    if (need_m || need_cnt || need_sel) {
        if (need_sel) {
            for (int i = tid; i < WV_WAVES * WV_BINS; i += WV_THREADS) wv_hist[i] = 0;
            __syncthreads();
        }
        float mx = NEG_INF;
        unsigned cnt[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) cnt[v] = 0;
        unsigned* myh = wv_hist + wave * WV_BINS;
        wv_for_row(r, tid, [&](float s) {
            mx = fmaxf(mx, s);
            if (need_cnt) {
#pragma unroll
                for (int g = 0; g < 16; g += 4) {
                    if (g < nv) {
#pragma unroll
                        for (int v = g; v < g + 4; ++v) cnt[v] += (s > sv[v]) ? 1u : 0u;
                    }
                }
            }
            if (need_sel) atomicAdd(&myh[wv_key(s) >> 21], 1u);
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0) red_f[wave] = mx;
        if (need_cnt) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const unsigned c = vv_wave_sum(cnt[v]);
                if (lane == 0) red_u[wave][v] = c;
            }
        }
        __syncthreads();
        if (tid == 0) {
            float t = red_f[0];
            for (int w = 1; w < WV_WAVES; ++w) t = fmaxf(t, red_f[w]);
            m_s = t;
        }
        if (need_cnt && tid < 16) {
            unsigned c = 0;
            for (int w = 0; w < WV_WAVES; ++w) c += red_u[w][tid];
            cnt_s[tid] = c;
        }
        __syncthreads();
        m = m_s;
    }

    // ---------------- radix select of tau (top-k in front of top-p) ----------------
    if (need_sel) {
        unsigned prefix = 0, k_left = (unsigned)kk;
        for (int d = 0; d < 3; ++d) {
            const int nb = d < 2 ? WV_BINS : 1024;
            if (d > 0) {
                __syncthreads();
                for (int i = tid; i < WV_WAVES * WV_BINS; i += WV_THREADS) wv_hist[i] = 0;
                __syncthreads();
                unsigned* myh = wv_hist + wave * WV_BINS;
                if (d == 1) {
                    wv_for_row(r, tid, [&](float s) {
                        const unsigned key = wv_key(s);
                        if ((key >> 21) == prefix) atomicAdd(&myh[(key >> 10) & 2047u], 1u);
                    });
                } else {
                    wv_for_row(r, tid, [&](float s) {
                        const unsigned key = wv_key(s);
                        if ((key >> 10) == prefix) atomicAdd(&myh[key & 1023u], 1u);
                    });
                }
            }
            __syncthreads();
            for (int b = tid; b < nb; b += WV_THREADS) {          // one owner per bin: the total lands in wave 0's copy
                unsigned t = 0;
                for (int w = 0; w < WV_WAVES; ++w) t += wv_hist[w * WV_BINS + b];
                wv_hist[b] = t;
            }
            __syncthreads();
            if (wave == 0) wv_find_digit(wv_hist, nb, k_left, lane, &sel_digit, &sel_k);
            __syncthreads();
            prefix = (prefix << (d < 2 ? 11 : 10)) | sel_digit;
            k_left = sel_k;
        }
        tau = wv_unkey(prefix);
    }

    // ---------------- final pass: Z and A[v] over T ----------------
    if (topp_on) {
        float z = 0.f, am[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) am[v] = 0.f;
        wv_for_row(r, tid, [&](float s) {
            if (s >= tau) {
                const float e = __expf(s - m);
                z += e;
#pragma unroll
                for (int g = 0; g < 16; g += 4) {
                    if (g < nv) {
#pragma unroll
                        for (int v = g; v < g + 4; ++v) am[v] += (s <= sv[v]) ? e : 0.f;
                    }
                }
            }
        });
        // fp64 from here on, one fixed tree per wave and the waves in order
        {
            const double t = vv_wave_sum((double)z);
            if (lane == 0) red_d[wave][16] = t;
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const double t = vv_wave_sum((double)am[v]);
            if (lane == 0) red_d[wave][v] = t;
        }
        __syncthreads();
        if (tid < 17) {
            double t = 0.0;
            for (int w = 0; w < WV_WAVES; ++w) t += red_d[w][tid];
            mass_s[tid] = t;
        }
        __syncthreads();
    }

    // ---------------- the verdict per valid token ----------------
    if (tid < 64) {
        bool keep = false;
        float s = 0.f;
        if (tid < nv) {
            s = sv_s[tid];
            keep = true;
            if (topk_on) keep = need_sel ? (s >= tau) : (cnt_s[tid] < (unsigned)kk);
            if (topp_on && keep) keep = (s == m) || !(mass_s[tid] <= (1.0 - (double)a.top_p) * mass_s[16]);
            if (minp_on && keep) keep = (s == m) || !(exp((double)s - (double)m) < (double)a.min_p);
            out[(int64_t)row * nv + tid] = keep ? s : NEG_INF;
        }
        const unsigned long long b = __ballot(keep && fabsf(s) < __builtin_inff());
        if (tid == 0) survivors[row] = __popcll(b);
    }
}

}  // namespace

extern "C" int vv_warp_valid_launch(const float* logits, const unsigned char* seen, float* out, int* survivors, int n, int V,
                                    const int* ids, int n_valid, float pen, float temp, int do_sample, int top_k, float top_p,
                                    float min_p, hipStream_t s) {
    if (n < 1 || n > 16 || V < 1 || n_valid < 1 || n_valid > 16) return -1;
    VVWarpIds vi;
    vi.n = n_valid;
    for (int i = 0; i < 16; ++i) {
        vi.id[i] = i < n_valid ? ids[i] : 0;
        if (vi.id[i] < 0 || vi.id[i] >= V) return -1;
    }
    VVWarpArgs a;
    a.pen = pen; a.temp = temp; a.top_p = top_p; a.min_p = min_p;
    a.pen_on = (pen != 1.f && seen != nullptr) ? 1 : 0;
    a.temp_on = (do_sample && temp != 1.f) ? 1 : 0;
    a.do_sample = do_sample ? 1 : 0;
    a.top_k = top_k;
    const int kk = top_k > 0 ? (top_k < V ? top_k : V) : 0;
    const bool sel = do_sample && kk > 0 && kk < V && top_p < 1.f;
    static const hipError_t lds = vv_raise_lds_limit((int)WV_HIST_BYTES, &vv_warp_valid_kernel);
    if (lds != hipSuccess) { (void)hipGetLastError(); return -1; }
    hipLaunchKernelGGL(vv_warp_valid_kernel, dim3(n), dim3(WV_THREADS), sel ? WV_HIST_BYTES : 0, s, logits, seen, out, survivors, V, vi, a);
    return vv_launch_rc(0);
}
