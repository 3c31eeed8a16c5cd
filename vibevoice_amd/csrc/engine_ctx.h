// engine_ctx.h -- what the host units (engine*.hip) share: the context, its descriptor types, error / launch macros.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <string>
#include <vector>
#include "../../include/vvhip.h"
#include "vv_common.h"
#include "vv_launch.h"

// A named namespace, not an anonymous one: vv_ctx holds these types, and it must be ONE type in every unit that includes this header.
namespace vv_engine {
struct VVShiftH { float* buf; int T, hist, C; };     // one row of a history-shift table (misc.hip: VVShift)
enum WKind { W_MAT = 0, W_VEC = 1, W_DW = 2, W_TABLE = 3, W_BIAS_REP = 4 };

struct Weight {
    std::string name;
    int kind = W_VEC;
    int64_t nelem = 0;          // source element count
    void* dev = nullptr;        // final storage
    // W_MAT packing parameters
    int N = 0, K = 0, pk = 0, Cin = 0, Cout = 0, ksz = 0, stride = 0;
    int rep = 1;                // W_BIAS_REP: repeat count
    bool loaded = false;
    bool optional = false;
    int twin = -1;              // W_MAT: row of vv_ctx::twins of the W13 twin this parameter's storage is part of, or none
};

// W13 twin of one packed matrix (vv_w13.h): the diffusion head's gate / up / down and the LM layers' QKV / o / gate / up / down.  Packed
// behind every write to the matrix (w13_repack); the launches read per tile row whether the twin holds it (gemv.hip: WF), so the host
// never needs the device's answer.  A twin never packed is all zero: every tile row streams bf16.
// exact / used (the head's twins): the folded ok word as the host last read it (-1: written since, not read), and the answer the
// sampler's graphs were built with.  An exact twin takes the launch without the fall-back (VVGemm::w13_exact); see head_w13_resolve.
struct W13Twin { void* planes; const void* src; int N, K; bool lm; int exact = -1, used = -1; };

struct Block {
    int C;
    float *norm_w, *ffn_norm_w, *gamma, *ffn_gamma, *dw_w, *dw_b, *b1, *b2;
    void *w1, *w2;
    float* nb;                  // unfused path: [6 + Tmax][C] normed buffer with history
    float* nst;                 // fused path: [12][C] normed history (rows 0..5) + next state (rows 6..11)
    int64_t nb_stride;          // floats between the nb (nst) buffers of consecutive utterance slots
};

struct ConvG {                  // conv / transposed conv as a GEMM over a time-major buffer
    void* w; float* bias;
    int K, N, ldx;              // per output row
    int rows_per_frame;         // output rows per frame
};

struct Stage {
    int C, Tpf;                 // channels, time steps per frame
    int hist;                   // history rows kept in front of xs
    float* xs;                  // [hist + Tmax][C]
    float* xs2;                 // fused stages ping-pong between xs and xs2
    float* xfinal;              // buffer holding the stage output (and its history rows)
    bool fused;                 // blocks run as one vv_block1d_kernel each
    bool pp;                    // unfused T <= 8 stage: channel-sliced norm+conv, blocks ping-pong between xs and xs2
    int64_t sl_stride;          // floats between the xs (xs2) buffers of consecutive utterance slots
    std::vector<Block> blocks;
    ConvG in;                   // produces this stage's rows from the previous buffer
};

struct CodecNet {
    bool decoder = false;
    int Fmax = 1, in_dim = 1, out_dim = 1, in_hist = 6, in_Tpf = 1;
    std::vector<float*> in_buf;            // per slot: [6 + Tin][in_dim]
    std::vector<std::vector<Stage>> st;    // per slot
    ConvG head;
    std::vector<float*> u;                 // FFN hidden scratch, one per slot (slots may run concurrently on different streams)
    std::map<std::pair<uint64_t, int>, std::pair<void*, int>> shift_tab;   // (slot bit mask, F) -> history-shift table on the device, its entries
    int maxC = 1;
    // slot-batched stages (several utterances' rows in ONE weight pass, run_codec with a slot set): the leading `kd` stages of a decoder,
    // the stages from `ke` on of an encoder -- the T <= 8, C >= 1024 stages that hold ~95 % of a tokenizer's weight bytes
    int kd = 0, ke = 1 << 30;
    bool head_batch = false;                 // the head conv has a slot-batched form too
    int64_t in_stride = 0, u_stride = 0;     // floats between the in_buf / u buffers of consecutive slots
};

struct GraphEntry { hipGraphExec_t exec; uint64_t last_use; };

// One generation of the diffusion sampler's state (headtail.hip, solver.hip: a solver step reads one and writes the other): the head's
// in-projection, the noisy latent, the previous x0 and -- null until the first general schedule -- the x0 before that
struct HeadGen { float *xh = nullptr, *zz = nullptr, *x0p = nullptr, *m2 = nullptr; };

}  // namespace vv_engine
using namespace vv_engine;      // this header is internal to the engine*.hip units

constexpr int PROBE_MAX = 1024;      // stages one NaN-probe record buffer holds (vv_ctx::probe_rec)

struct vv_ctx {
    vv_config c;
    char err[512];
    std::vector<Weight> w;
    std::map<std::string, int> widx;
    int H, D, Hq, Hkv, I, QKV;
    // LM params
    struct Layer { float *ln1, *ln2, *bqkv; void *wqkv, *wo, *wg, *wu, *wd; void *tqkv, *to, *tg, *tu, *td; };      // t*: W13 twins, or null
    std::vector<Layer> layers;
    float *lm_norm = nullptr, *inv_freq = nullptr;
    int ws_rows = 0;
    void* rope_tab = nullptr; bool rope_ready = false;
    float *tts_types = nullptr, *eos_b1 = nullptr, *eos_b2 = nullptr; void *eos_w1 = nullptr, *eos_w2 = nullptr;
    void *embed = nullptr, *lm_head = nullptr;
    bool lm_head_loaded = false;
    void* valid_w = nullptr; int n_valid = 0;
    int valid_ids[16] = {0};               // the ids themselves (vv_lm_warp_valid reads their columns of the full logits)
    // LM runtime
    void *kc = nullptr, *vc = nullptr;
    int64_t cache_stride = 0, head_stride = 0, layer_stride = 0;
    VVRow* rows_dev = nullptr; VVRow* rows_pin = nullptr; int rows_cap = 2048;
    int* ids_dev = nullptr; int* ids_pin = nullptr; int ids_cap = 64;      // token ids per vv_embed call: max(64, max_rows)
    // pinned staging is a ring (slot reuse waits on that slot's own copy event, long since complete): a step's
    // launches can be enqueued while the previous step is still running, no host-side stream sync
    static constexpr int RING = 32;
    hipEvent_t ring_ev[RING] = {}; bool ring_used[RING] = {}; int ring_i = 0;
    float *h = nullptr, *qkv = nullptr, *qrot = nullptr, *attn = nullptr, *act = nullptr;
    float *h_parts = nullptr, *xh_parts = nullptr;     // K-split partial tensors of the residual streams (2 x [rows][H] each)
    void *xp = nullptr, *actp = nullptr;               // prefill (prefill.hip): activations as packed bf16 MFMA fragments
    bool tile3_ok = false, attn2_ok = false;
    VVGemmWs gws = {nullptr, nullptr, nullptr, nullptr, 0};         // K-split workspace of the long-prompt GEMM (null: never split)
    // batch decode (5..16 rows, bf16 mode): activations as one 16-row packed fragment tile (gemv16p.hip).  The producer's residual
    // epilogue packs the next projection's operand (x * norm weight, un-normalised) and leaves per-tile partial sums of squares; the
    // consumer applies 1/rms to its accumulator rows (gemv16p.hip RS / PK / SH)
    void *p16_x = nullptr, *p16_act = nullptr, *p16_y = nullptr, *p16_shift = nullptr; float *ssq_a = nullptr, *ssq_b = nullptr; bool p16_ok = false;
    size_t p16_shift_tile = 0;      // bytes of one packed [16][H] tile of the head's shift rows
    float *pm = nullptr, *pl = nullptr, *po = nullptr;
    // head
    int HF = 0, MODW = 0;
    struct HLayer { float* norm; void *wg, *wu, *wd; int ig, iu, id; };      // ig / iu / id: the matrices' rows of the parameter table
    // W13 twins (bf16 mode, qualifying widths): w13_on the head's gate / up / down matrices, w13_lm the LM layers' five as well.
    // VVHIP_W13=0: none; VVHIP_W13=head: the head's alone
    bool w13_on = false, w13_lm = false;
    std::vector<W13Twin> twins;
    std::vector<HLayer> hl;
    void *h_in = nullptr, *h_cond = nullptr, *h_t0 = nullptr, *h_t2 = nullptr, *h_ada = nullptr, *h_out = nullptr;
    int n_steps = 0;
    // coef: the installed table, 64 rows of 8 floats: {a, s, cs, c0, c1, cn, 0, 0} shipped, {a, s, cs, c0, c1, c2, cn, 0} general
    float *temb = nullptr, *coef = nullptr, *tvals = nullptr;
    bool sde_on = false;                   // the schedule table carries variance-noise scales (sde-dpmsolver++)
    bool general_on = false;               // the table is a general one (vv_set_schedule_general; solver.hip ends every step)
    float* mod_all = nullptr; size_t mod_all_bytes = 0;
    float* ada_in = nullptr;
    void* ada_p = nullptr;                 // the same rows as packed bf16 MFMA fragments (bf16 mode: one tile GEMM for all steps)
    float *cproj = nullptr, *mod = nullptr, *hact = nullptr, *eps = nullptr;
    HeadGen hg[2];                  // the sampler's state: a solver step reads generation g and writes g ^ 1
    bool head_tail = false;         // the fused seam (headtail.hip); off in the exact modes or when its LDS size is refused
    bool solver_fuse = true;        // the step end carries the next in-projection where solver.hip's rule allows (VVHIP_SOLVER_FUSE=0: never)
    float *tmp1 = nullptr, *tmp2 = nullptr;
    // connectors
    struct Conn { void *fc1, *fc2; float *b1, *b2, *norm; } ac_conn, sem_conn;
    float *ct1 = nullptr;
    // codecs
    CodecNet dec, aenc, senc;
    int enc_pass = 0;                      // frames per voice-prompt encoder pass (0: aenc.Fmax)
    // vv_codec_chain_batch: the per-utterance parts of a batch's tokenizer chains fork onto these streams (graph branches)
    hipStream_t side[8] = {}; hipEvent_t ev_fork = nullptr, ev_join[8] = {}; bool side_ready = false;
    float scaling = 1.f, bias = 0.f;
    int hop = 3200;
    // staging
    void* stage = nullptr; size_t stage_bytes = 0;
    std::map<std::string, GraphEntry> graphs;      // bounded: least-recently-used entries are destroyed beyond graph_cap
    uint64_t graph_tick = 0; size_t graph_cap = 512;
    std::set<std::string> seen;
    std::set<void*> allocs;                // every dalloc() of this engine: released by vv_destroy
    // weight sharing (vv_create_shared): a child context's weight storage IS its parent's -- the k-th weight allocation of
    // vv_create returns the parent's k-th one (same model configuration -> same sequence); everything else (KV caches, activations,
    // tokenizer state, graphs, staging) is the child's own, so two contexts decode concurrently on two streams over one weight copy
    vv_ctx* parent = nullptr; int n_children = 0; bool zombie = false, creating = false;
    // VVHIP_NAN_PROBE=1 (debugging): scan kernels behind the sampler's launches, inside the captured graph as well; the first stage whose
    // output holds a non-finite value is printed after the call (nan_probe()).  The record buffer is allocated by vv_create
    unsigned* probe_rec = nullptr; std::vector<std::string> probe_names; bool probe_on = false; int probe_calls = 0;
    int64_t foreign_nodes = 0;        // nodes of captured graphs that are not kernel launches (memset / memcpy nodes: none must exist, see misc.hip's copy kernels)
    int64_t capture_fallbacks = 0; char last_capture_issue[256] = "";     // stream captures that fell back to an eager run (graphed())
    std::vector<std::pair<void*, size_t>> wallocs; size_t wshare_i = 0;
    // device-resident LoRA adapters (engine_lora.hip): parameter index -> a copy of its packed region taken at its first merge.  Every
    // merge writes active = f(snapshot, a, b); vv_lora_reset copies the snapshot back; vv_upload refreshes it (the upload is the new base)
    struct LoraBase { void* snap; size_t bytes; bool merged; };
    std::map<int, LoraBase> lora_base;
    int64_t lora_base_bytes = 0;      // vv_stat 7
    // what a streaming row stage (engine_codec.hip) keeps of each of its streams on the host: its input total (what the next push's
    // outputs are counted from) and whether it has been flushed
    struct RowStage { int n_streams = 0; std::vector<int64_t> total; std::vector<char> flushed; };
    // streaming resamplers (vv_resampler_set, engine_codec.hip; kernels: resample.hip): the filter and one history row of T samples per
    // stream on the device.  This context's own, a shared child's included; the buffers are dalloc()s, released by vv_destroy.
    struct Resampler : RowStage { int L = 0, M = 0, T = 0; float* coef = nullptr; float* hist = nullptr; };
    static constexpr int N_RESAMPLERS = 4;
    Resampler rs[N_RESAMPLERS];
    // streaming tempo changes (vv_tempo_set, engine_codec.hip; kernels: tempo.hip): the window table, per stream VV_TP_HIST history samples
    // and its last block's offset on the device, and on the host its speed P / Q (fixed by its first push, 0 before).  Kept like the
    // resamplers.
    struct Tempo : RowStage { float* window = nullptr; float* hist = nullptr; int* dstate = nullptr; std::vector<int> P, Q; };
    static constexpr int N_TEMPOS = 4;
    Tempo tp[N_TEMPOS];
    // streaming pitch resamplers (vv_pitch_set, engine_codec.hip; kernels: pitch.hip): the prototype table every ratio shares, per stream
    // VV_PT_HIST history samples on the device and on the host its ratio P / Q (fixed by its first push, 0 before).  Kept like the resamplers.
    struct Pitch : RowStage { int R = 0; float* table = nullptr; float* hist = nullptr; std::vector<int> P, Q; };
    static constexpr int N_PITCHES = 4;
    Pitch pt[N_PITCHES];
    // streaming formant warps (vv_formant_set, engine_codec.hip; kernels: formant.hip): the twiddle table, per stream VV_FM_HIST history
    // samples and VV_FM_TAIL partial sums on the device, on the host its fraction A / B (fixed by its first push, 0 before), and the frames
    // of one launch (16 rows) between its two kernels: the pushes of one configuration are ordered on one stream.  Kept like the resamplers.
    struct Formant : RowStage { float* tw = nullptr; float* hist = nullptr; float* tail = nullptr; float* scratch = nullptr; std::vector<int> A, B; };
    static constexpr int N_FORMANTS = 4;
    Formant fm[N_FORMANTS];
    // streaming output levels (vv_level_set, engine_codec.hip; kernels: level.hip): look-ahead A, hold H, ceiling c, per stream H + 2 A - 2
    // history samples on the device and on the host its gain (fixed by its first push, 0 before).  Kept like the resamplers.
    struct Level : RowStage { int A = 0, H = 0; float c = 0.f; float* hist = nullptr; std::vector<float> gain; };
    static constexpr int N_LEVELS = 4;
    Level lv[N_LEVELS];
    // streaming loudness levellers (vv_loud_set, engine_codec.hip; kernels: loudness.hip): the taps as fp64, per stream a ring of VV_LD_T
    // quantised inputs, a VVLdState and the FIR launch's tile sums on the device, and on the host its parameters t, g0, wmax (fixed by its
    // first push, t = 0 before).  Kept like the resamplers.
    struct Loud : RowStage { double* taps = nullptr; int* hist = nullptr; VVLdState* state = nullptr; long long* part = nullptr;
                             std::vector<float> t, g0, wmax; };
    static constexpr int N_LOUDS = 4;
    Loud loud[N_LOUDS];
    // streaming pause shorteners (vv_pause_set, engine_codec.hip; kernels: pause.hip): seg samples a segment, the join's weights, per stream
    // VV_PS_FLOATS samples and a VVPsState on the device, and on the host its caps and threshold (fixed by its first push, theta = -1
    // before).  Kept like the resamplers.
    struct Pause : RowStage { int seg = 0; float* wt = nullptr; float* sbuf = nullptr; VVPsState* state = nullptr;
                              std::vector<int> C, C0; std::vector<long long> theta; };
    static constexpr int N_PAUSES = 4;
    Pause ps[N_PAUSES];
    int64_t launches = 0;
    int64_t solver_fused = 0;         // general-path step ends that carried the next in-projection, last recorded body (vv_stat 8)
    int64_t seam_launches = 0;        // head-tail seam launches the last recorded sampler body issued (vv_stat 6; a replay keeps its capture's count)
    // optional per-GEMM-launch hipEvent timing (vv_profile_begin/end)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;
    int prof_n = 0;
    double prof_bytes = 0.0;
    struct ProfRec { int T, N, K, pro, epi, dual; double bytes; int gemv; };
    std::vector<ProfRec> prof_rec;
    std::vector<VVGemm> prof_gemv;          // the decode-GEMV launches of the last profile window, in issue order (vv_profile_replay)
    double prof_gemv_bytes = 0.0;
    // launches of the other timed kernel families recorded in the same window (vv_profile_replay_family): 1 = vv_gemv16p_kernel
    // (batch decode projections), 2 = decode attention (vv_attn_fused_kernel + its vv_attn_merge2_kernel)
    struct ProfLaunch { int family; double bytes; std::function<int(hipStream_t)> fn; };
    std::vector<ProfLaunch> prof_other;
    int64_t prof_raw_ns = 0, prof_ev_over_ns = 0;
    hipStream_t prof_stream = nullptr;     // last vv_profile_end: uncalibrated GEMV total, one empty event pair
#ifdef VV_GEMM_TIMING
    // timing builds only (tools/step_timeline.py): every GEMM launch gets a stamp slice for its workgroups' entry/exit clocks
    unsigned long long* tl_base = nullptr; int tl_idx = 0;
    struct TlRec { int T, N, K, pro, epi; };
    std::vector<TlRec> tl_rec;
#endif
};

// ---- defined once, in engine.hip (hidden like every non-API symbol: -fvisibility=hidden) ----
extern thread_local char g_err[512];
// Contexts that share weights are driven from several host threads (Engine.fork): a stream capture in one thread must not overlap
// device calls of this library in another (hipErrorStreamCaptureInvalidated was seen with three lanes: one capturing, one running
// first-sight eager launches).  Every API call that enqueues work holds this lock shared; a capture holds it exclusively.
extern std::shared_mutex g_dev_mu;
#define VV_SHARED std::shared_lock<std::shared_mutex> _vv_dev_lk(g_dev_mu)
// parent / child bookkeeping of shared contexts (n_children, zombie): forks are created and closed from lane threads that hold
// g_dev_mu only SHARED, so the counters have their own mutex
extern std::mutex g_family_mu;
int fail(vv_ctx* ctx, const char* fmt, ...);
#define HIPCHK(ctx, e) do { hipError_t _e = (e); if (_e != hipSuccess) return fail(ctx, "%s:%d hip error %s", __FILE__, __LINE__, hipGetErrorString(_e)); } while (0)
#define VVCHK(e) do { int _r = (e); if (_r != 0) return _r < 0 ? fail(ctx, "%s:%d launch failed (%d): hip error %d (%s)", __FILE__, __LINE__, _r, g_vv_launch_err, hipGetErrorString((hipError_t)g_vv_launch_err)) : _r; } while (0)
#define VVTRY(e) do { if (int _r = (e)) return _r; } while (0)      // a helper that has already recorded its failure

void* dalloc(vv_ctx* ctx, size_t bytes, bool zero = true);
void dfree(vv_ctx* ctx, void* p);
// weight storage and the parameter table.  vv_create_shared pairs a child's k-th walloc with its parent's k-th and compares the
// tables index by index: the ORDER of these calls in create_impl and build_codec is part of the contract
void* walloc(vv_ctx* ctx, size_t bytes, bool zero = true);
void* alloc_packed(vv_ctx* ctx, int N, int K);
int add_w(vv_ctx* ctx, const std::string& name, int kind, int64_t nelem, bool optional = false);
void add_mat(vv_ctx* ctx, const std::string& name, int N, int K, void* base, int ntile_off, int pk = 0, int Cin = 0, int Cout = 0,
             int ksz = 0, int stride = 0, int64_t src_nelem = -1);
float* add_vec(vv_ctx* ctx, const std::string& name, int64_t n, float* dst = nullptr, int kind = W_VEC, int rep = 1);
VVGemm mk_gemm(const void* W, const float* X, float* Y, int T, int N, int K, int ldx, int ldy);
int ksplit_parts(const vv_ctx* ctx, VVGemm& g, float* parts, int part_stride);
int ring_acquire(vv_ctx* ctx);
int build_codec(vv_ctx* ctx, CodecNet& net, const std::string& pfx, bool decoder, int vae_dim, int Fmax, int n_slots);      // engine_codec.hip
int ksplit_check(vv_ctx* ctx, hipStream_t st);                                                                               // engine_lm.hip
int p16_gemv(vv_ctx* ctx, hipStream_t st, const void* W, const void* W2, const void* Xp, float* Y, void* Yp, const float* bias,
             const float* gate, int T, int N, int K, int ldy, int ld_gate, int epi);
int p16_go(vv_ctx* ctx, hipStream_t st, const VVGemv16p& a, int epi, int flags);
VVGemv16p p16_args(const void* W, const void* W2, const void* Xp, float* Y, void* Yp, int T, int N, int K, int ldy);
void nan_probe(vv_ctx* ctx, hipStream_t st, const char* name, const void* p, size_t n);                                      // engine_prof.hip
void nan_probe_report(vv_ctx* ctx, hipStream_t st, const char* what);
int gemm_prof(vv_ctx* ctx, const VVGemm& g, hipStream_t st);
int lora_rebase(vv_ctx* ctx, int widx, hipStream_t st);                                                                       // engine_lora.hip
// Behind EVERY write to a parameter's packed storage (vv_upload, the LoRA merge and reset): re-packs the W13 twin it is part of, if
// any, on the same stream.  Enqueue only: no wait, no read-back, no graph is dropped (the twins' storage never moves and the kernels
// read the ok words themselves).  The caller holds g_dev_mu shared.
int w13_repack(vv_ctx* ctx, int widx, hipStream_t st);                                                                        // engine.hip

// One GEMM launch of an op body (`ctx` and `st` in scope).  ctx->launches counts these and what the bodies add by hand; some launches
// (vv_copy_launch, vv_sampler_init_launch, ...) are not counted, and bench.py reports the figure as it is: do not "fix" it in passing.
#ifdef VV_GEMM_TIMING
int gemm_tl(vv_ctx* ctx, VVGemm g, hipStream_t st);
#define GEMM(g) do { ctx->launches++; VVCHK(gemm_tl(ctx, g, st)); } while (0)
#else
#define GEMM(g) do { ctx->launches++; if (ctx->prof_on) VVCHK(gemm_prof(ctx, g, st)); else VVCHK(vv_gemm_launch(g, ctx->c.xsplit, st)); } while (0)
#endif

// Runs `body` (the launches of one op) eagerly at the first sight of `key`, captured into a hipGraph at the second, replayed after.
// The cache policy is graphed_run (engine.hip); the template only erases the body's type, by reference.
//
// A replay repeats every scalar argument and every pointer of the captured launches: whatever can change between two calls is READ
// FROM DEVICE MEMORY, is a FIELD OF THE KEY, or is changed only by a call that DROPS the family (drop_graphs).  Never moving, for
// every family: weight storage (vv_upload and the LoRA merges write in place), the buffers vv_create allocates, the route
// (pass_plan.h: a function of the row count, the key fields and what the context offers).  Per family (DESIGN.md section 3 has the
// same table; the tests are those of tests/test_gpu_graph_replay.py unless another file is named):
//   lm:     key: rows, x / hidden pointers, layer range, final norm, row-set mode, SPLIT COUNT of the attention (from 2 on the merge
//           kernel is in the graph).  device: the row table (cache, position), x, the KV caches, the (cos, sin) table (rebuilt in
//           place in front of the graph after an upload), inv_freq.  by value: nothing else.
//           test_lm_replays_follow_the_row_table, test_replays_after_an_upload
//   samp: sde:  key: n, cond / noise / step-noise / output pointers, CFG_SCALE.  device: conditions, noise, the rows of ctx->coef, ctx->hg.
//           by value: STEP COUNT, TABLE OFFSETS, THE PER-STEP MODULATION BUFFERS (a longer schedule reallocates them), sde_on --
//           dropped by vv_set_schedule / vv_set_schedule_sde.  test_sampler_graphs_follow_the_schedule, test_replays_after_an_upload
//           W13 twins: storage that never moves, re-packed in place behind every write; which tile rows stream them is read from the
//           device by the launch itself.  by value: WHETHER EACH HEAD TWIN IS EXACT (the launch without the fall-back) -- read back at
//           the first sampler call after a write to the matrix (head_w13_resolve), which drops the four families when an answer changed.  test_gpu_w13.py: test_sampler_arms_agree; test_gpu_w13_lm.py (the lm: family too)
//   rows:   as samp: / sde:, with the POINTER of the per-row scales in the key and the scales on the device.
//           test_gpu_cfg_rows.py: test_graph_replay_follows_the_buffer, test_a_new_schedule_drops_the_cached_rows_graph
//   gen:    the general solver table (vv_diffusion_sample_general).  key: n, cond / noise / step-noise / PER-ROW-SCALE / output
//           pointers, CFG_SCALE.  device: conditions, noise, the table's rows, the per-row scales.  by value: as samp: -- dropped by
//           all three vv_set_schedule* calls.  test_gpu_solver_family.py: test_cfg_rows_match_scalar_runs_and_replay,
//           test_switching_to_a_shipped_table_and_back
//   dec:    key: APPLY, slot, frames, latent / audio pointers.  device: latent, the slot's conv history.  by value: 1 / SCALING, -BIAS
//           (apply = 1) -- dropped by vv_set_speech_factors ("dec:1:").  test_speech_factors_reach_the_tokenizer_replays[dec-*]
//   senc:   key: slot, frames, audio / output pointers.  device: audio, the slot's conv history.  by value: nothing; no setter drops it.
//           test_speech_factors_reach_the_tokenizer_replays[dec-*]
//   chain:  key: APPLY, THE SLOT LIST IN ORDER, latent / audio / semantic pointers.  device: latents, both nets' conv history.
//           by value: 1 / SCALING, -BIAS (apply = 1) -- dropped by vv_set_speech_factors ("chain:1:"); the fork / join of the
//           per-utterance branches (VVHIP_BATCH_CODEC, read by vv_create).  test_speech_factors_reach_the_tokenizer_replays[chain-*],
//           test_chain_graphs_are_keyed_by_slot_order, test_warmup_before_the_speech_factors_leaves_no_stale_graph
// A new host-side value inside a body goes into the key or into a drop_graphs call, and into this table with the test that pins it.
int graphed_run(vv_ctx* ctx, const std::string& key, hipStream_t st, const std::function<int()>& body);
// Destroys the cached graphs whose key starts with one of `prefixes`, after waiting for the device (a victim's replay may still be
// running).  The caller holds g_dev_mu shared (VV_SHARED), so no capture of the process is open.  Which families a setter drops is said in
// its call of this function and nowhere else.
int drop_graphs(vv_ctx* ctx, std::initializer_list<const char*> prefixes);
template <class F>
static int graphed(vv_ctx* ctx, const std::string& key, hipStream_t st, F&& body) { return graphed_run(ctx, key, st, std::ref(body)); }
