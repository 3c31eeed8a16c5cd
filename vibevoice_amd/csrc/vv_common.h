// vv_common.h -- shared device/host declarations for libvvhip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define VV_WAVE 64

// ---- packed weight tile ------------------------------------------------------
// A [N x K] matrix is stored as tiles of 16 rows x 32 k.  One tile = 1 KiB =
// 64 lanes x 16 B, in exactly the order the lanes of a wave consume it as the
// A (or B) operand of v_mfma_f32_16x16x32_bf16:
//   lane l holds W[n0 + (l & 15)][k0 + (l >> 4) * 8 + 0..7]
// tiles are ordered [n_tile][k_tile]; rows >= N and columns >= K are zero.
// (the element index inside a tile, for device code: vv_packed_index in vv_device.h)
static inline __host__ __device__ int64_t vv_packed_elems(int N, int K) {
    return (int64_t)((N + 15) / 16) * ((K + 31) / 32) * 512;
}

// ---- row table for LM steps ---------------------------------------------------
struct VVRow {
    int cache;   // KV cache id
    int pos;     // position of this token == cache length before the append
};

// ---- workspace of the prefill GEMM's K-split partial round (prefill.hip: vv_gemm4_kernel) ----
struct VVGemmWs {
    float* partials;     // 256 slots x 256 KiB (a workgroup's 32 accumulators x 512 threads x f32x4)
    unsigned* flags;     // 256 arrival words, zero whenever no launch is in flight
    unsigned* err;       // host-mapped word, set by a wait that timed out
    // short prompts (vv_gemm3_kernel: a few dozen 128 x 128 tiles): K split over grid.y into dense fp32 partial tensors
    // [part][T][N], summed in part order (+ bias / residual) by vv_g3_reduce_kernel -- no hand-off inside a launch
    float* g3_partials;
    size_t g3_bytes;
};

// ---- generic skinny GEMM -----------------------------------------------------
// Y[t][n] (op)= sum_k f(X[t][k]) * W[n][k]
enum { VV_PRO_NONE = 0, VV_PRO_RMS = 1, VV_PRO_RMS_MOD = 2, VV_PRO_ADD_SILU = 3,
       VV_PRO_NORMDW = 4 };   // gemv.hip only, one row: Block1D's norm + causal depthwise conv + layer scale + residual, then RMSNorm (see VVGemm::dw_*)
enum { VV_EPI_STORE = 0, VV_EPI_BIAS = 1, VV_EPI_BIAS_GELU = 2, VV_EPI_SWIGLU = 3,
       VV_EPI_RESID = 4, VV_EPI_GATED_RESID = 5, VV_EPI_CFG_DPM = 6,
       VV_EPI_QKV_ROPE = 7 };   // prefill.hip only: bias + RoPE + KV-cache append in the QKV GEMM's epilogue

struct VVGemm {
    const u32x4* W;        // packed tiles
    const u32x4* W2;       // second matrix ("up") for VV_EPI_SWIGLU, else null
    const float* X;        // [T] rows, K contiguous floats each, row stride ldx
    float* Y;              // [T][N], row stride ldy
    const float* nw;       // PRO_RMS*: norm weight [K] (null = no affine)
    const float* mod_scale;// PRO_RMS_MOD: per-row [T][ld_mod]
    const float* mod_shift;
    const float* addvec;   // PRO_ADD_SILU: [K]
    const float* bias;     // [N] or null
    const float* nscale;   // EPI_RESID: per-n scale (gamma) or null
    const float* gate;     // EPI_GATED_RESID: per-row [T][ld_gate]
    int T, N, K;
    int ldx, ldy, ld_mod, ld_gate;
    int pro, epi;
    int ksplit;            // 1, 2 or 4 waves of the block split K
    int nt;                // non-temporal weight loads (streamed-once weights)
    int t_pad;             // LDS row stride of the staging tile (set by the launcher)
    // EPI_CFG_DPM (diffusion-head final layer): rows [0,n) cond, [n,2n) uncond -> CFG + DPM-Solver++ update in place
    float* z;              // [2n][N] noisy latent (both halves rewritten)
    float* x0p;            // [n][N] previous x0 prediction
    const float* coef;     // {a, s, cs, c0, c1, cn}: one 6-float row of the schedule table per solver step
    float cfg;
    int n_cfg;
    const float* cfg_rows; // [n_cfg] one guidance scale per utterance row, read in place of cfg; null = cfg for every row
    const float* sde_noise; // stochastic solver (sde-dpmsolver++): this step's variance noise [n][N], added as cn * eps; null = off
    unsigned long long* dbg;   // optional phase timestamps (VV_GEMM_TIMING builds only)
    // row t reads activation row (t % x_row_mod) and, for PRO_ADD_SILU, the add-vector (t / add_rows_per_vec)
    // (0 = off).  Used to batch the diffusion head's adaLN GEMM over all solver steps of a frame.
    int x_row_mod, add_rows_per_vec;
    float eps;
    // K split across workgroups (decode GEMV only, PRO_NONE + residual epilogues): workgroup column ks > 0 stores its
    // scaled partial to yparts + (ks-1)*part_stride instead of Y; consumers of that tensor add the parts back in a
    // fixed order (deterministic): xa/n_xa on the activation side, ya/n_ya on the residual side, same row strides.
    int kgrid;             // 0/1 = off
    float* yparts;
    const float* xa;       // n_xa part tensors laid out like X, part_stride floats apart
    const float* ya;       // n_ya part tensors laid out like Y
    int n_xa, n_ya;
    int part_stride;
    // Slot-batched rows (tokenizer stages of several utterances in ONE weight pass, 16-row GEMV form only): the launch has
    // sl_n * sl_T logical rows; row rg belongs to slot j = rg / sl_T, local row tt = rg % sl_T.  A side with a non-zero slot
    // stride (sl_x / sl_y, floats) lives in per-utterance streaming buffers: row pointer = base + sl_id[j] * stride + tt * ld;
    // a side with stride 0 is a dense [rows][ld] scratch tensor.  sl_n = 0: off.
    int sl_n, sl_T, sl_x, sl_y;
    int sl_id[8];
    // PRO_NORMDW (T = 1 tokenizer stages, modular_vibevoice_tokenizer.py:620-684 Block1D up to FFN1): X is the block's INPUT row
    // x [K]; the prologue forms  h = RMSNorm(x) * dw_nw,  xo = x + dw_gamma * (dw_b + sum_{j<6} dw_w[j] * dw_hist[j] + dw_w[6] * h)
    // (the causal k = 7 depthwise conv over the six cached normed rows and the new one), then feeds RMSNorm(xo) * nw to the
    // product like PRO_RMS.  The workgroup of tile 0 also writes xo -> dw_xout (FFN2's residual, the next block's input) and
    // h -> dw_hnew (the conv history's new row).  Replaces the separate vv_normdw_sliced launch in front of FFN1.
    const float* dw_hist;  // [6][K] normed history rows
    const float* dw_w;     // [7][K] taps
    const float* dw_b;     // [K]
    const float* dw_gamma; // [K]
    const float* dw_nw;    // [K] weight of the block's first norm
    float* dw_xout;        // [K]
    float* dw_hnew;        // [K]
    // W13 twins of W / W2 (vv_w13.h), or null: the launch streams the twins' planes where a W13 form exists for it (gemv_plan.h:
    // vv_gemv_w13_form) and produces the bits of the bf16 launch
    const void* w13;
    const void* w13_2;
    // the caller knows that every tile row of the twin(s) is exact (the folded ok word, read on the host): the launch takes the
    // instantiation that reads no ok word and holds no bf16 loop (gemv.hip: WF = 1); 0: the one with the per-tile-row fall-back (WF = 2)
    int w13_exact;
};

// ---- batch decode over pre-packed activations (gemv16p.hip) ----
struct VVGemv16p {
    const u32x4* W;        // packed [N][K]
    const u32x4* W2;       // SwiGLU "up" matrix, same shape
    const u32x4* Xp;       // packed activations, ONE 16-row tile: [K/32][64][8]
    float* Y;              // fp32 [T][ldy]  (bias / residual / gated residual)
    unsigned char* Yp;     // packed bf16 [16][N]  (SwiGLU; PK: the new residual rows x pk_nw (x (1 + pk_sc)))
    const float* bias;     // [N] or null
    const float* gate;     // gated residual: per-row [T][ld_gate]
    int T, N, K, ldy, ld_gate;
    // RS: the operand is UN-normalised (x * norm weight): the accumulator rows are scaled by rsqrt(sum_tiles ssq_in[tile][row] / K + eps)
    const float* ssq_in;   // [ssq_tiles][16]
    int ssq_tiles;
    float eps;
    const u32x4* Xs;       // SH: second packed operand (adaLN shift rows), added unscaled: y = rs * W.Xp + W.Xs
    // PK (residual epilogues): besides Y, write bf16(y_new * pk_nw[n] * (1 + pk_sc[row][n])) packed to Yp and sum_n y_new^2 to ssq_out
    const float* pk_nw;    // [N] or null (= 1)
    const float* pk_sc;    // per-row [T][ld_pk] or null
    int ld_pk;
    float* ssq_out;        // [N / 16][16]
    // VV_EPI_CFG_DPM (the sampler's final layer): rows [0, n) cond, [n, 2n) uncond -> CFG + DPM-Solver++ update of z in place (gemv.hip)
    float* z; float* x0p; const float* coef; float cfg; int n_cfg; const float* sde_noise;
    const float* cfg_rows; // [n_cfg] per-row guidance scale or null (VVGemm::cfg_rows)
};

// ---- the seam between two solver steps of the diffusion head (headtail.hip): final layer + CFG + DPM-Solver++ update + in-projection ----
struct VVTail {
    const u32x4* Wout;     // packed [L][H]   final layer (adaLN-modulated norm without affine, then linear)
    const u32x4* Win;      // packed [H][L]   noisy_images_proj of the NEXT step
    const float* bin;      // [H] or null
    const float* X;        // residual rows [T][H] after the last head layer (+ n_xa part tensors: xa, part_stride)
    const float* xa; int n_xa, part_stride;
    const float* sc; const float* sh; int ld_mod;      // the final layer's scale / shift rows [T][ld_mod]
    float* Xout;           // the next step's residual rows [T][H] (a DIFFERENT buffer than X)
    const float* z_in; const float* x0p_in;            // [2n][L], [n][L]: this step's state
    float* z_out; float* x0p_out;                      // the next step's state (different buffers)
    const float* coef; float cfg; int n_cfg; const float* sde_noise;
    const float* cfg_rows; // [n_cfg] per-row guidance scale or null (VVGemm::cfg_rows)
    int T, H, L; float eps;
};

// up to 8 utterance slots of one launch (per-utterance kernels take the slot from blockIdx.y / .z)
struct VVSlotIds { int n; int id[8]; };
// ids == null: no slot set (n = 0: the kernel works on the base pointers alone); unused entries are 0
static inline VVSlotIds vv_slot_ids(const int* ids, int n) {
    VVSlotIds sl; sl.n = ids ? n : 0;
    for (int i = 0; i < 8; ++i) sl.id[i] = (ids && i < n) ? ids[i] : 0;
    return sl;
}
__device__ __forceinline__ int vv_slot_id(const int (&id)[8], int j) {     // select chain: no dynamic indexing of a by-value kernel argument
    int r = id[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) r = (j == i) ? id[i] : r;
    return r;
}

// ---- streaming resampler (resample.hip): one row of a push, passed by value in the kernel arguments ----
// The host keeps each stream's 64-bit input total; what the kernel needs of it is the position of the row's first output:
// with k0 = m0 * M + (L * T - 2) / 2 for that output m0, p0 = k0 % L is its phase and b0 = k0 / L - total + T the index of its newest
// input sample in the row's staging buffer [T history | n_in chunk | T / 2 zeros].  Output j of the push then sits at
// phase (p0 + j * M) % L, index b0 + (p0 + j * M) / L: 32-bit arithmetic whatever the stream's age.
struct VVRsRow { int stream, n_in, n_out, p0, b0; };
struct VVRsRows { VVRsRow r[16]; };
constexpr int VV_RS_MAX_OUT = 8192;        // outputs one row of a push may emit (1024 threads x 8 accumulators)

// ---- streaming tempo change (tempo.hip): one row of a push, passed by value in the kernel arguments ----
// The host keeps each stream's 64-bit input total and speed P / Q; the row names the blocks the push completes, k0 .. k0 + nblk - 1,
// and base = total - VV_TP_HIST, the signal index of the first sample in the row's staging buffer [history | n_in chunk | zeros]:
// the kernel forms a_k = (k * 240 * P) / Q in 64 bits and indexes with a_k - base.  n_out: nblk * 240, less where a flush cuts the
// last block.
struct VVTpRow { long long k0, base; int stream, n_in, nblk, n_out, P, Q; };
struct VVTpRows { VVTpRow r[16]; };
constexpr int VV_TP_HS = 240, VV_TP_N = 480, VV_TP_DELTA = 160;
constexpr int VV_TP_HIST = 1280;           // input samples a stream keeps between pushes: > DELTA + 480 + 639 (vibevoice_amd/tempo.py)
constexpr int VV_TP_MAX_IN = 7680;         // input samples one row of a push may bring (the staging buffer is LDS)
constexpr int VV_TP_PAD = 896;             // zeros behind the chunk: a flush reads up to DELTA + HS + N = 880 samples past the signal's end
constexpr int VV_TP_BUF = VV_TP_HIST + VV_TP_MAX_IN + VV_TP_PAD;
constexpr int VV_TP_MAX_BLOCKS = 96;       // blocks per staged buffer: a block advances >= 120 input samples, (MAX_IN + PAD) / 120 < 96

// ---- streaming pitch resampler (pitch.hip): one row of a push, passed by value in the kernel arguments, each at its own ratio ----
// The host keeps each stream's 64-bit input total and its ratio P / Q; what the kernel needs of the total is the position of the row's
// first output m0: with k0 = m0 * P, a0 = k0 % Q is its phase and b0 = k0 / Q - total + VV_PT_HIST the index of the input sample it
// sits on in the row's staging buffer [VV_PT_HIST history | n_in chunk | VV_PT_MAX_TN zeros].  Output j of the push then has phase
// (a0 + j * P) % Q and sits on index b0 + (a0 + j * P) / Q: 32-bit arithmetic whatever the stream's age.
struct VVPitchRow { int stream, n_in, n_out, P, Q, a0, b0; };
struct VVPitchRows { VVPitchRow r[16]; };
struct VVPitchRatios { int P[16], Q[16]; };    // vv_pitch_once_kernel: the ratio of each of up to 16 signals of a launch
constexpr int VV_PT_Z = 32;                // zero crossings of the prototype either side (vibevoice_amd/pitch.py: Z)
constexpr int VV_PT_MAX_R = 256;           // table entries per crossing, at most: the table [Z R + 1] is staged in LDS
constexpr int VV_PT_MAX_TN = 64;           // Tn = ceil(Z max(P, Q) / Q) <= 64 for P <= 2 Q: input samples a stream holds back
constexpr int VV_PT_HIST = 2 * VV_PT_MAX_TN;   // input samples a stream keeps between pushes
constexpr int VV_PT_MAX_IN = 7552;         // input samples one row of a push may bring (the staging buffer is LDS, beside the table)
constexpr int VV_PT_MAX_OUT = 8192;        // outputs one row of a push may emit (1024 threads x 8 accumulators)
// Tn of a ratio: 0 at 1 / 1, which is the identity by definition (pitch.py, "Unison")
static inline int vv_pt_taps(int P, int Q) { return P == Q ? 0 : (VV_PT_Z * (P > Q ? P : Q) + Q - 1) / Q; }
// the ratios a row may run at: both terms in 1..100, P / Q in [1/2, 2]
static inline bool vv_pt_ratio_ok(int P, int Q) { return P >= 1 && P <= 100 && Q >= 1 && Q <= 100 && P <= 2 * Q && Q <= 2 * P; }

// ---- streaming formant warp (formant.hip): one row of a launch, passed by value in the kernel arguments, each at its own fraction ----
// The host keeps each stream's 64-bit input total and its fraction A / B; the kernels see a push relative to its first new frame.  With
// F0 = total / H frames done before the push: the push computes frames F0 .. F0 + nf - 1, frame f of them covers samples
// [f * H - 3 * H - r, f * H + H - r) counted from the chunk's first, r = total % H (below 0: the stream's history, beyond n_in: zeros).
// Block c = 0 .. nf + 2 of the push is output block F0 - 3 + c: blocks c < 3 start from the stream's partial sums, blocks c < c_min lie
// before the signal (c_min = max(0, 3 - F0)) and are dropped, blocks c < nf are complete and go to out at (c - c_min) * H, cut at n_out;
// blocks nf .. nf + 2 are the stream's new partial sums.  A == B: the identity, n_out = n_in copied, no frame.  32-bit arithmetic
// whatever the stream's age.  stream < 0 (vv_formant_once): no history, no partial sums.
struct VVFmRow { int stream, n_in, n_out, A, B, nf, r, c_min; };
struct VVFmRows { VVFmRow r[16]; };
constexpr int VV_FM_N = 1024;              // frame length (vibevoice_amd/formant.py: N)
constexpr int VV_FM_H = 256;               // hop
constexpr int VV_FM_K = VV_FM_N / 2 + 1;   // bins
constexpr int VV_FM_QC = 64;               // the lifter keeps quefrencies |q| < QC
constexpr int VV_FM_HIST = VV_FM_N;        // input samples a stream keeps between pushes: N - H behind the at most H - 1 of its open block
constexpr int VV_FM_TAIL = VV_FM_N - VV_FM_H;  // partial sums of a stream's overlap-add tail
constexpr int VV_FM_MAX_IN = 7552;         // input samples one row of a push may bring, as in the pitch stage
constexpr int VV_FM_MAX_FRAMES = 36;       // frames one row of a push computes: (255 + MAX_IN) / H = 30 complete ones, + 4 at a flush
constexpr int VV_FM_MAX_TERM = 10000;
// the fractions a row may run at: both terms in 1..10^4, A / B in [1/2, 2]
static inline bool vv_fm_ratio_ok(int A, int B) { return A >= 1 && A <= VV_FM_MAX_TERM && B >= 1 && B <= VV_FM_MAX_TERM && A <= 2 * B && B <= 2 * A; }

// ---- streaming output level (level.hip): one row of a push, passed by value in the kernel arguments ----
// The host keeps each stream's 64-bit input total and its gain; the row's staging buffer is [H + 2 A - 2 history | n_in chunk | A - 1
// zeros], its first output sits at index b0 = (first output's signal index) - total + H + 2 A - 2 of it, n_out outputs follow.
struct VVLvRow { int stream, n_in, n_out, b0; float gain; };
struct VVLvRows { VVLvRow r[16]; };
constexpr int VV_LV_BUF = 8128;            // samples of a row's staging buffer (two 32-bit words each in LDS; vibevoice_amd/level.py: BUF)
constexpr int VV_LV_MAX_A = 2047;          // keeps the window sums below 2^31

// ---- streaming loudness leveller (loudness.hip): one row of a push, passed by value in the kernel arguments ----
// The host keeps each stream's 64-bit input total and its parameters; of the total the kernels need k0 = total % VV_LD_S, the position of
// the row's first sample in its open segment, h0 = total % VV_LD_T, that sample's slot in the stream's ring of quantised inputs, and
// first = (total == 0): the stream's gains are g0 and its state counts as empty.  n_out = n_in: the stage holds nothing back.
struct VVLdRow { int stream, n_in, n_out, k0, h0, first; float t, g0, wmax; };
struct VVLdRows { VVLdRow r[16]; };
constexpr int VV_LD_S = 2400;              // samples of a segment (vibevoice_amd/loudness.py: S)
constexpr int VV_LD_T = 2400;              // taps of the K-weighting FIR; a stream's ring holds as many quantised inputs, T - 1 of them live
constexpr int VV_LD_RING = 30;             // counted segments the slow mean looks back over
constexpr int VV_LD_MAX_IN = 3200;         // input samples one row of a push may bring (loudness.py: MAX_IN): at most 2 segments close
constexpr int VV_LD_TILE = 320;            // outputs of one FIR workgroup: 64 lanes x 5
constexpr int VV_LD_MAX_TILES = VV_LD_MAX_IN / VV_LD_TILE;
constexpr long long VV_LD_GATE = 120856803LL;   // EG = floor(S 2^32 10^((-50 + 0.691) / 10)) (loudness.py: EG)
// what a stream keeps on the device besides its ring of inputs: the open segment's running sum, the ring of counted energies (the next
// one goes to e[head]; count of them are live) and the last two wanted gains
struct VVLdState { long long acc; long long e[VV_LD_RING]; int head, count; float w1, w2; };
// the ranges of a stream's parameters, for the entry points (engine_codec.hip) and the launchers (loudness.hip) alike: t of a target in
// [-36, -10] LUFS, g0 of [-24, +24] dB, wmax of [0, 24] dB; a NaN compares false
static inline bool vv_ld_params_ok(float t, float g0, float wmax) {
    return t > 0.f && t < 1.0f && g0 > 0.f && g0 <= 16.0f && wmax >= 1.0f && wmax <= 16.0f;
}

// ---- streaming pause shortener (pause.hip): one row of a push, passed by value in the kernel arguments ----
// The host keeps each stream's 64-bit input total and its parameters; of the total the kernel needs carry = total % seg, the samples of
// the stream's open segment that wait in its state.  What a row emits depends on the data: the kernel counts it (VVPsState, and the
// launch's count word), the host does not know it.  seg = rate / 100 samples a segment, C / C0 the caps in segments (2^31 - 1: none),
// theta the integer a segment's energy is compared with.
struct VVPsRow { int stream, n_in, flush, carry, seg, C, C0, pad; long long theta; };
struct VVPsRows { VVPsRow r[16]; };
constexpr int VV_PS_MIN_SEG = 80;          // 8 kHz
constexpr int VV_PS_MAX_SEG = 480;         // 48 kHz
constexpr int VV_PS_MAX_T = 10;            // segments a stream holds back at most (vibevoice_amd/pause.py: MAX_T)
constexpr int VV_PS_MAX_IN = 7680;         // input samples one row of a push may bring (pause.py: MAX_IN)
constexpr int VV_PS_MAX_SEGS = (VV_PS_MAX_IN + VV_PS_MIN_SEG - 1) / VV_PS_MIN_SEG;     // whole segments a push completes at most: 96
// what a stream keeps on the device: VV_PS_FLOATS samples [open segment, < seg | ring: held segments of seg samples, oldest first |
// first, seg], each part at its VV_PS_*_AT, and its counters: the samples taken, emitted and dropped, the open quiet run's length in
// segments, whether a loud segment has arrived, and the segments held
constexpr int VV_PS_RING_AT = VV_PS_MAX_SEG, VV_PS_FIRST_AT = VV_PS_RING_AT + VV_PS_MAX_T * VV_PS_MAX_SEG;
constexpr int VV_PS_FLOATS = VV_PS_FIRST_AT + VV_PS_MAX_SEG;
struct VVPsState { long long tin, tout, dropped; int run, started, held, pad; };
// scratch of one signal of vv_pause_once, in floats: the stream's samples and room for nothing else (its counters live in LDS)
constexpr int VV_PS_ONCE_FLOATS = VV_PS_FLOATS;
static inline bool vv_ps_params_ok(int seg, int C, int C0, long long theta) {
    return seg >= VV_PS_MIN_SEG && seg <= VV_PS_MAX_SEG && C >= 0 && C0 >= 0 && theta >= 0;
}

// Raise the dynamic-LDS limit of one or more kernels above the 64 KiB default; returns the first error.  A launcher calls it as
// the initialiser of a function-local `static const hipError_t`: C++11 runs that initialiser once per process and makes
// concurrent first calls wait for it (generate_interleaved and fork() drive two contexts from two host threads).
template <class... K>
static inline hipError_t vv_raise_lds_limit(int bytes, K*... kernels) {
    hipError_t rc = hipSuccess;
    for (const void* k : {reinterpret_cast<const void*>(kernels)...}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (rc == hipSuccess) rc = e;
    }
    return rc;
}

// what a launcher (or its plan) answers when nothing is launched: no compiled form of ITS kernel for this call (the caller may route
// the call to another kernel), or no kernel at all can run it
enum { VV_RC_NO_FORM = -3, VV_RC_NO_KERNEL = -4 };

// Launch status of the calling host thread: hipGetLastError() after a launch (it clears the thread's error state, so the code is
// kept here for the message the API layer prints).  rc_ok is what the launcher returns on success.
inline thread_local int g_vv_launch_err = 0;
static inline int vv_launch_rc(int rc_ok) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return rc_ok;
    g_vv_launch_err = (int)e;
    return -2;
}

