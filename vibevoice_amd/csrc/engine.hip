// engine.hip -- host side of libvvhip.so: context create / destroy, allocators, parameter registry and upload, hipGraph
// capture / replay cache, connectors.  The op orchestration lives in engine_lm / engine_head / engine_codec / engine_prof.hip,
// the device-resident LoRA adapters (base snapshots, merge, reset, read-back) in engine_lora.hip.
#include "engine_ctx.h"
#include "vv_w13.h"

// declared (and explained) in engine_ctx.h; defined here and nowhere else
thread_local char g_err[512] = "";
std::shared_mutex g_dev_mu;
std::mutex g_family_mu;

int fail(vv_ctx* ctx, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    char* dst = ctx ? ctx->err : g_err;
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    if (ctx) snprintf(g_err, 512, "%s", ctx->err);
    return -1;
}

int ring_acquire(vv_ctx* ctx) {
    const int slot = ctx->ring_i;
    ctx->ring_i = (ctx->ring_i + 1) % vv_ctx::RING;
    if (ctx->ring_used[slot]) hipEventSynchronize(ctx->ring_ev[slot]);
    ctx->ring_used[slot] = true;
    return slot;
}

void* dalloc(vv_ctx* ctx, size_t bytes, bool zero) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) { fail(ctx, "hipMalloc(%zu) failed", bytes); return nullptr; }
    if (zero) hipMemset(p, 0, bytes);
    else { static const int poison = [] { const char* e = getenv("VVHIP_POISON"); return (e && e[0] == '1') ? 1 : 0; }();      // debugging: NaN words in
           if (poison) hipMemset(p, 0xFF, bytes); }                                                                              // every buffer handed out un-zeroed
    if (ctx) ctx->allocs.insert(p);
    return p;
}
void dfree(vv_ctx* ctx, void* p) {
    if (!p) return;
    if (ctx) ctx->allocs.erase(p);
    hipFree(p);
}

int add_w(vv_ctx* ctx, const std::string& name, int kind, int64_t nelem, bool optional) {
    Weight w; w.name = name; w.kind = kind; w.nelem = nelem; w.optional = optional;
    ctx->widx[name] = (int)ctx->w.size();
    ctx->w.push_back(w);
    return (int)ctx->w.size() - 1;
}
// registers a packed matrix stored inside `base` at n-tile offset `ntile_off` of a [Ntot x K] tile array
void add_mat(vv_ctx* ctx, const std::string& name, int N, int K, void* base, int ntile_off, int pk, int Cin, int Cout, int ksz,
             int stride, int64_t src_nelem) {
    int i = add_w(ctx, name, W_MAT, src_nelem < 0 ? (int64_t)N * K : src_nelem);
    Weight& w = ctx->w[i];
    w.N = N; w.K = K; w.pk = pk; w.Cin = Cin; w.Cout = Cout; w.ksz = ksz; w.stride = stride;
    const int k_tiles = (K + 31) / 32;
    w.dev = (char*)base + (int64_t)ntile_off * k_tiles * 1024;
}
// weight storage: during vv_create the allocation sequence is recorded (parent) or replayed from the parent (shared child)
void* walloc(vv_ctx* ctx, size_t bytes, bool zero) {
    if (!ctx->creating) return dalloc(ctx, bytes, zero);
    if (ctx->parent) {
        vv_ctx* p = ctx->parent;
        if (ctx->wshare_i >= p->wallocs.size() || p->wallocs[ctx->wshare_i].second != bytes) {
            fail(ctx, "vv_create_shared: weight allocation %zu (%zu bytes) does not match the parent's -- different model configuration", ctx->wshare_i, bytes);
            return nullptr;
        }
        void* q = p->wallocs[ctx->wshare_i++].first;
        ctx->wallocs.push_back({q, bytes});
        return q;
    }
    void* q = dalloc(ctx, bytes, zero);
    ctx->wallocs.push_back({q, bytes});
    return q;
}
void* alloc_packed(vv_ctx* ctx, int N, int K) { return walloc(ctx, (size_t)vv_packed_elems(N, K) * 2); }
float* add_vec(vv_ctx* ctx, const std::string& name, int64_t n, float* dst, int kind, int rep) {
    int i = add_w(ctx, name, kind, n);
    if (!dst) dst = (float*)walloc(ctx, (size_t)n * rep * 4);
    ctx->w[i].dev = dst; ctx->w[i].rep = rep;
    return dst;
}

VVGemm mk_gemm(const void* W, const float* X, float* Y, int T, int N, int K, int ldx, int ldy) {
    VVGemm g; memset(&g, 0, sizeof(g));
    g.W = (const u32x4*)W; g.X = X; g.Y = Y; g.T = T; g.N = N; g.K = K; g.ldx = ldx; g.ldy = ldy;
    g.pro = VV_PRO_NONE; g.epi = VV_EPI_STORE; g.ksplit = 0; g.nt = 0; g.eps = 1e-6f;
    return g;
}
// Few output tiles x long K (the down projections of small models): split K over 2-3 workgroup columns so every CU
// streams; the partial tensors are added back by the consumers (VVGemm::xa / ya).  Returns the number of EXTRA parts.
int ksplit_parts(const vv_ctx* ctx, VVGemm& g, float* parts, int part_stride) {
    const int n_tiles = (g.N + 15) / 16, k_tiles = (g.K + 31) / 32;
    // few tiles x long K only: at 7B widths (224 tiles for 256 CUs) three K columns put 672 workgroups on the chip, i.e. the SAME 87.5 %
    // balance (2.625 per CU against 3) as 224 workgroups on 256 CUs, and the consumer reads two more part tensors -- measured, not shipped
    // (profiles/r06_down_ksplit_7b_ab.json)
    constexpr int max_tiles = 128;
    if (g.T > 4 || n_tiles > max_tiles || k_tiles < 96) return 0;
    const int ks = 3;
    g.kgrid = ks; g.yparts = parts; g.part_stride = part_stride;
    if (!vv_gemv_ok(&g)) { g.kgrid = 0; g.yparts = nullptr; g.part_stride = 0; return 0; }
    return ks - 1;
}
// ------------------------------------------------------------------ graphs
int graphed_run(vv_ctx* ctx, const std::string& key, hipStream_t st, const std::function<int()>& body) {
    if (!ctx->c.use_graph || ctx->prof_on) { VV_SHARED; return body(); }
    auto it = ctx->graphs.find(key);
    if (it == ctx->graphs.end()) {
        // first sight of a key: run eagerly (lazy allocations, shift tables) and remember it; a key that comes back is
        // captured then.  One-off launch shapes (prompt prefill chunks: unique pointers) never pay for a capture.
        if (ctx->seen.size() > 8192) ctx->seen.clear();
        if (ctx->seen.insert(key).second) { VV_SHARED; return body(); }
        hipGraph_t graph = nullptr;
        GraphEntry ge; ge.last_use = 0;
        bool captured = false;
        {   // one capture at a time in the process: contexts sharing weights are driven from several host threads (Engine.fork)
            std::unique_lock<std::shared_mutex> lk(g_dev_mu);
            HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
            const int r = body();
            const hipError_t e = hipStreamEndCapture(st, &graph);
            if (r == 0 && e == hipSuccess) {
                size_t nn = 0;
                if (hipGraphGetNodes(graph, nullptr, &nn) == hipSuccess && nn) {
                    std::vector<hipGraphNode_t> nodes(nn);
                    if (hipGraphGetNodes(graph, nodes.data(), &nn) == hipSuccess)
                        for (size_t i = 0; i < nn; ++i) { hipGraphNodeType t; if (hipGraphNodeGetType(nodes[i], &t) == hipSuccess && t != hipGraphNodeTypeKernel) ctx->foreign_nodes++; }
                }
                HIPCHK(ctx, hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0));
                hipGraphDestroy(graph);
                captured = true;
            } else {
                // A capture that did not close cleanly executed nothing.  Known cause: ANOTHER host thread called a device-wide
                // synchronize (hipDeviceSynchronize / torch.cuda.synchronize()) while this capture was open -- ROCm 7.0.2 refuses
                // that call in its thread and marks this capture invalid although its mode is Relaxed.  The work is run the way the
                // first sight of a key runs (eagerly).  On that ROCm the stream itself does not recover from an invalidated capture
                // (every later call on it answers hipErrorStreamCaptureInvalidated; ending the capture a second time or destroying
                // the returned graph handle crashes inside the runtime -- both tried): then the eager run fails too and the message
                // below says why.  Callers keep device-wide synchronizes out of processes that generate.
                (void)hipGetLastError();
                ctx->capture_fallbacks++;
                snprintf(ctx->last_capture_issue, sizeof(ctx->last_capture_issue), "capture of '%s': body rc %d, hipStreamEndCapture: %s", key.c_str(), r, hipGetErrorString(e));
            }
        }
        if (!captured) {
            VV_SHARED;
            const int r2 = body();
            if (r2 != 0) {
                char prev[200]; snprintf(prev, sizeof(prev), "%s", ctx->err);
                return fail(ctx, "%s; the eager re-run failed as well (%s).  If another host thread called a device-wide synchronize "
                                 "(torch.cuda.synchronize()) during the capture, the stream is lost: synchronize streams or events instead", ctx->last_capture_issue, prev);
            }
            return 0;
        }
        if (ctx->graphs.size() >= ctx->graph_cap) {
            // a long-running process with varied launch shapes (prefill remainders over temporary buffers) must not
            // accumulate executables: drop the least-recently-used quarter.  Rare (a cache miss at the cap), so it may wait
            // for every stream: replays of the victims may still be running on this or a side stream.
            std::vector<std::pair<uint64_t, std::string>> order;
            for (auto& g : ctx->graphs) order.push_back({g.second.last_use, g.first});
            std::sort(order.begin(), order.end());
            std::unique_lock<std::shared_mutex> lk(g_dev_mu);      // a device-wide synchronize: never while another context's capture is open
            HIPCHK(ctx, hipDeviceSynchronize());
            for (size_t i = 0; i < order.size() / 4 + 1; ++i) {
                auto v = ctx->graphs.find(order[i].second);
                hipGraphExecDestroy(v->second.exec);
                ctx->graphs.erase(v);
            }
        }
        it = ctx->graphs.emplace(key, ge).first;
    }
    it->second.last_use = ++ctx->graph_tick;
    VV_SHARED;
    HIPCHK(ctx, hipGraphLaunch(it->second.exec, st));
    return 0;
}

// A setter that changes a host-side value captured launches hold (engine_ctx.h: the table above graphed()) drops the key families
// that hold it.  Waits first, as the eviction above does and for its reason: a victim's replay may still be running, on the caller's
// stream, a side stream or another stream the caller chose -- the setters have no stream of their own to wait on.  Device-wide is safe
// here because the caller holds g_dev_mu shared: no capture of the process is open.  Nothing matches (the usual case: factors and
// schedule are set before the first frame): no wait.
int drop_graphs(vv_ctx* ctx, std::initializer_list<const char*> prefixes) {
    auto hit = [&](const std::string& key) {
        for (const char* p : prefixes) if (key.rfind(p, 0) == 0) return true;
        return false;
    };
    bool any = false;
    for (auto& g : ctx->graphs) if (hit(g.first)) { any = true; break; }
    if (!any) return 0;
    HIPCHK(ctx, hipDeviceSynchronize());
    for (auto it = ctx->graphs.begin(); it != ctx->graphs.end();) {
        if (hit(it->first)) { hipGraphExecDestroy(it->second.exec); it = ctx->graphs.erase(it); } else ++it;
    }
    return 0;
}

// ------------------------------------------------------------------ API
extern "C" const char* vv_last_error(vv_ctx* ctx) { return ctx ? ctx->err : g_err; }

// Content hash of the sources this library was compiled from (vibevoice_amd/build.py passes -DVV_BUILD_ID): the loader
// compares it with the hash of the sources next to it, so a stale in-tree binary is rebuilt or refused instead of silently run.
// build.py keys THIS unit's object on the build id (_object_key): vv_build_id stays in engine.hip.
#ifndef VV_BUILD_ID
#define VV_BUILD_ID "unknown"
#endif
extern "C" const char* vv_build_id() { return "VVHIP_BUILD_ID=" VV_BUILD_ID; }

static int create_impl(const vv_config* cfg, vv_ctx* parent, vv_ctx** out) {
    VV_SHARED;
    vv_ctx* ctx = new vv_ctx();
    ctx->c = *cfg; ctx->err[0] = 0;
    ctx->parent = parent; ctx->creating = true;
    vv_config& c = ctx->c;
    if (c.max_rows < 1 || c.max_rows > 16384) { delete ctx; return fail(nullptr, "max_rows must be in [1,16384]"); }
    if (c.lm_head_dim != 64 && c.lm_head_dim != 128) { delete ctx; return fail(nullptr, "head_dim must be 64 or 128"); }
    // the attention kernels put the query heads of a GQA group on the 16 MFMA columns (attn.hip)
    if (c.lm_kv_heads < 1 || c.lm_heads % c.lm_kv_heads != 0 || c.lm_heads / c.lm_kv_heads > 16) {
        const int hq = c.lm_heads, hkv = c.lm_kv_heads;
        delete ctx;
        return fail(nullptr, "lm_heads=%d / lm_kv_heads=%d: the GQA group size must be an integer <= 16", hq, hkv);
    }
    if (c.xsplit < 1 || c.xsplit > 3) c.xsplit = 2;
    if (c.attn_splits < 1) c.attn_splits = 128;
    if (c.enc_frames < 1) c.enc_frames = 1;
    if (getenv("VVHIP_GRAPH_CAP")) ctx->graph_cap = (size_t)std::max(4, atoi(getenv("VVHIP_GRAPH_CAP")));
    c.max_ctx = (c.max_ctx + 127) & ~127;
    const int H = ctx->H = c.lm_hidden, D = ctx->D = c.lm_head_dim, Hq = ctx->Hq = c.lm_heads, Hkv = ctx->Hkv = c.lm_kv_heads;
    const int I = ctx->I = c.lm_inter;
    const int QKV = ctx->QKV = (Hq + 2 * Hkv) * D;
    const int R = c.max_rows;
    // Every walloc / add_w / add_mat / add_vec below and in build_codec keeps its place in the sequence: a shared child replays the
    // parent's k-th weight allocation as its own k-th (wshare_i) and the two parameter tables are compared index by index.
    // ---- LM ----
    ctx->embed = walloc(ctx, (size_t)c.lm_vocab * H * 2);
    { int i = add_w(ctx, "lm.embed_tokens.weight", W_TABLE, (int64_t)c.lm_vocab * H); ctx->w[i].dev = ctx->embed; }
    { int i = add_w(ctx, "lm_head.weight", W_TABLE, (int64_t)c.lm_vocab * H, true); ctx->w[i].dev = nullptr; }
    ctx->inv_freq = add_vec(ctx, "lm.rope.inv_freq", D / 2);
    ctx->lm_norm = add_vec(ctx, "lm.norm.weight", H);
    if (c.tts_layers > 0) {
        if (c.tts_layers >= c.lm_layers) { delete ctx; return fail(nullptr, "tts_layers must be < lm_layers"); }
        ctx->tts_types = add_vec(ctx, "tts_input_types.weight", 2 * (int64_t)H);
        ctx->eos_w1 = alloc_packed(ctx, H, H); add_mat(ctx, "eos.fc1.weight", H, H, ctx->eos_w1, 0);
        ctx->eos_b1 = add_vec(ctx, "eos.fc1.bias", H);
        ctx->eos_w2 = alloc_packed(ctx, 1, H); add_mat(ctx, "eos.fc2.weight", 1, H, ctx->eos_w2, 0);
        ctx->eos_b2 = add_vec(ctx, "eos.fc2.bias", 1);
    }
    // W13 twins (+13/16 of a matrix's bytes): bf16 mode, whole 4-k-tile groups.  The head's layers qualify together (w13_on), an LM
    // matrix by its own shape (w13_lm).  A shared context has its parent's
    {
        const char* e = getenv("VVHIP_W13");      // 0: no twins, no new launches; head: the diffusion head's alone (the A/B arms)
        const bool on = !(e && e[0] == '0') && c.xsplit == 1;
        ctx->w13_on = parent ? parent->w13_on : on && vv_w13_shape_ok(c.head_ffn, H) && vv_w13_shape_ok(H, c.head_ffn);
        ctx->w13_lm = parent ? parent->w13_lm : on && !(e && !strcmp(e, "head"));
    }
    // the twin of the matrix [N][K] at src, shared by the n_par parameters registered last (q / k / v are parts of one QKV matrix)
    auto twin = [&](bool want, bool lm, const void* src, int N, int K, int n_par = 1) -> void* {
        if (!want || !vv_w13_shape_ok(N, K)) return nullptr;
        ctx->twins.push_back({walloc(ctx, (size_t)vv_w13_bytes(N, K)), src, N, K, lm});
        for (int j = 0; j < n_par; ++j) ctx->w[ctx->w.size() - 1 - j].twin = (int)ctx->twins.size() - 1;
        return ctx->twins.back().planes;
    };
    ctx->layers.resize(c.lm_layers);
    for (int l = 0; l < c.lm_layers; ++l) {
        auto& L = ctx->layers[l];
        char nm[128]; snprintf(nm, 128, "lm.layers.%d.", l);
        std::string p(nm);
        L.ln1 = add_vec(ctx, p + "input_layernorm.weight", H);
        L.ln2 = add_vec(ctx, p + "post_attention_layernorm.weight", H);
        L.wqkv = alloc_packed(ctx, QKV, H);
        L.bqkv = (float*)walloc(ctx, (size_t)QKV * 4);
        add_mat(ctx, p + "self_attn.q_proj.weight", Hq * D, H, L.wqkv, 0);
        add_mat(ctx, p + "self_attn.k_proj.weight", Hkv * D, H, L.wqkv, Hq * D / 16);
        add_mat(ctx, p + "self_attn.v_proj.weight", Hkv * D, H, L.wqkv, (Hq + Hkv) * D / 16);
        L.tqkv = twin(ctx->w13_lm, true, L.wqkv, QKV, H, 3);
        add_vec(ctx, p + "self_attn.q_proj.bias", Hq * D, L.bqkv);
        add_vec(ctx, p + "self_attn.k_proj.bias", Hkv * D, L.bqkv + Hq * D);
        add_vec(ctx, p + "self_attn.v_proj.bias", Hkv * D, L.bqkv + (Hq + Hkv) * D);
        L.wo = alloc_packed(ctx, H, Hq * D); add_mat(ctx, p + "self_attn.o_proj.weight", H, Hq * D, L.wo, 0); L.to = twin(ctx->w13_lm, true, L.wo, H, Hq * D);
        L.wg = alloc_packed(ctx, I, H); add_mat(ctx, p + "mlp.gate_proj.weight", I, H, L.wg, 0); L.tg = twin(ctx->w13_lm, true, L.wg, I, H);
        L.wu = alloc_packed(ctx, I, H); add_mat(ctx, p + "mlp.up_proj.weight", I, H, L.wu, 0); L.tu = twin(ctx->w13_lm, true, L.wu, I, H);
        L.wd = alloc_packed(ctx, H, I); add_mat(ctx, p + "mlp.down_proj.weight", H, I, L.wd, 0); L.td = twin(ctx->w13_lm, true, L.wd, H, I);
    }
    const int n_caches = 2 * c.n_slots;
    ctx->head_stride = (int64_t)c.max_ctx * D;
    ctx->layer_stride = ctx->head_stride * Hkv;
    ctx->cache_stride = ctx->layer_stride * c.lm_layers;
    ctx->kc = dalloc(ctx, (size_t)ctx->cache_stride * n_caches * 2);
    ctx->vc = dalloc(ctx, (size_t)ctx->cache_stride * n_caches * 2);
    ctx->rows_cap = std::max(2048, c.max_rows);
    ctx->rows_dev = (VVRow*)dalloc(ctx, sizeof(VVRow) * ctx->rows_cap);
    hipHostMalloc((void**)&ctx->rows_pin, sizeof(VVRow) * (size_t)ctx->rows_cap * vv_ctx::RING);
    for (int i = 0; i < vv_ctx::RING; ++i) hipEventCreateWithFlags(&ctx->ring_ev[i], hipEventDisableTiming);
    ctx->ids_cap = std::max(64, c.max_rows);
    ctx->ids_dev = (int*)dalloc(ctx, sizeof(int) * ctx->ids_cap);
    hipHostMalloc((void**)&ctx->ids_pin, sizeof(int) * (size_t)ctx->ids_cap * vv_ctx::RING);
    ctx->h = (float*)dalloc(ctx, (size_t)R * H * 4);
    ctx->h_parts = (float*)dalloc(ctx, (size_t)2 * R * H * 4);
    ctx->qkv = (float*)dalloc(ctx, (size_t)R * QKV * 4);
    ctx->qrot = (float*)dalloc(ctx, (size_t)R * Hq * D * 4);
    ctx->attn = (float*)dalloc(ctx, (size_t)R * Hq * D * 4);
    ctx->act = (float*)dalloc(ctx, (size_t)R * I * 4);
    if (R >= 64 && (H % 8) == 0 && ((Hq * D) % 8) == 0 && (I % 8) == 0) {
        // prompt prefill in bf16-activation mode: LDS-staged 128 x 128 MFMA GEMM over packed activations (prefill.hip)
        ctx->xp = dalloc(ctx, (size_t)vv_packed_elems(R, std::max(H, Hq * D)) * 2);
        ctx->actp = dalloc(ctx, (size_t)vv_packed_elems(R, I) * 2);
        ctx->tile3_ok = c.xsplit == 1;
        if (ctx->tile3_ok) {      // short prompts: K parts of the 128 x 128 GEMM (up to 8 dense [rows][features] fp32 tensors, rows <= 1024)
            ctx->gws.g3_bytes = (size_t)8 * std::min(R, 1024) * std::max(ctx->QKV, H) * 4;
            ctx->gws.g3_partials = (float*)dalloc(ctx, ctx->gws.g3_bytes, false);
            if (!ctx->gws.g3_partials) ctx->gws.g3_bytes = 0;
        }
        const char* no_ks = getenv("VVHIP_NO_KSPLIT");  // opt-out: every tile of the partial round computed whole (no inter-workgroup hand-off)
        if (ctx->tile3_ok && R >= 1024 && !(no_ks && no_ks[0] == '1')) {   // prompts long enough for the 256 x 256 GEMM: its partial round is split along K
            ctx->gws.partials = (float*)dalloc(ctx, (size_t)256 * 32 * 512 * 16, false);
            ctx->gws.flags = (unsigned*)dalloc(ctx, 256 * sizeof(unsigned));
            if (hipHostMalloc((void**)&ctx->gws.err, sizeof(unsigned), hipHostMallocMapped) == hipSuccess && ctx->gws.err) *ctx->gws.err = 0u;
            else ctx->gws.err = nullptr;
        }
    }
    ctx->attn2_ok = c.xsplit == 1;
    if (c.xsplit == 1 && R > 4 && (H % 32) == 0 && ((Hq * D) % 32) == 0 && (I % 32) == 0) {
        const int kx = std::max(H, Hq * D), ka = std::max(I, c.head_ffn);
        ctx->p16_x = dalloc(ctx, (size_t)vv_packed_elems(16, kx) * 2);
        ctx->p16_act = dalloc(ctx, (size_t)vv_packed_elems(16, ka + 32) * 2);
        ctx->p16_y = dalloc(ctx, (size_t)vv_packed_elems(16, kx) * 2);
        ctx->ssq_a = (float*)dalloc(ctx, (size_t)(H / 16) * 16 * 4);
        ctx->ssq_b = (float*)dalloc(ctx, (size_t)(H / 16) * 16 * 4);
        ctx->p16_ok = ctx->p16_x && ctx->p16_act && ctx->p16_y && ctx->ssq_a && ctx->ssq_b;
    }
    ctx->rope_tab = dalloc(ctx, (size_t)c.max_ctx * (D / 2) * 8, false);
    // split-attention partials exist for decode rows and short ragged launches only (prompt chunks use the prefill kernel)
    ctx->ws_rows = std::min(R, 64);
    const size_t np = (size_t)ctx->ws_rows * Hkv * c.attn_splits * 16;
    ctx->pm = (float*)dalloc(ctx, np * 4); ctx->pl = (float*)dalloc(ctx, np * 4); ctx->po = (float*)dalloc(ctx, np * D * 4);
    // ---- diffusion head ----
    const int L = c.latent_dim, HL = c.head_layers, HF = ctx->HF = c.head_ffn;
    const int MODW = ctx->MODW = HL * 3 * H + 2 * H;
    ctx->h_in = alloc_packed(ctx, H, L); add_mat(ctx, "head.noisy_images_proj.weight", H, L, ctx->h_in, 0);
    ctx->h_cond = alloc_packed(ctx, H, H); add_mat(ctx, "head.cond_proj.weight", H, H, ctx->h_cond, 0);
    ctx->h_t0 = alloc_packed(ctx, H, 256); add_mat(ctx, "head.t_embedder.mlp.0.weight", H, 256, ctx->h_t0, 0);
    ctx->h_t2 = alloc_packed(ctx, H, H); add_mat(ctx, "head.t_embedder.mlp.2.weight", H, H, ctx->h_t2, 0);
    ctx->h_ada = alloc_packed(ctx, MODW, H);
    ctx->hl.resize(HL);
    auto htwin = [&](const void* src, int N, int K) {
        twin(ctx->w13_on, false, src, N, K);
        return (int)ctx->w.size() - 1;
    };
    for (int l = 0; l < HL; ++l) {
        char nm[128]; snprintf(nm, 128, "head.layers.%d.", l);
        std::string p(nm);
        ctx->hl[l].norm = add_vec(ctx, p + "norm.weight", H);
        add_mat(ctx, p + "adaLN_modulation.1.weight", 3 * H, H, ctx->h_ada, l * 3 * H / 16);
        ctx->hl[l].wg = alloc_packed(ctx, HF, H); add_mat(ctx, p + "ffn.gate_proj.weight", HF, H, ctx->hl[l].wg, 0); ctx->hl[l].ig = htwin(ctx->hl[l].wg, HF, H);
        ctx->hl[l].wu = alloc_packed(ctx, HF, H); add_mat(ctx, p + "ffn.up_proj.weight", HF, H, ctx->hl[l].wu, 0); ctx->hl[l].iu = htwin(ctx->hl[l].wu, HF, H);
        ctx->hl[l].wd = alloc_packed(ctx, H, HF); add_mat(ctx, p + "ffn.down_proj.weight", H, HF, ctx->hl[l].wd, 0); ctx->hl[l].id = htwin(ctx->hl[l].wd, H, HF);
    }
    add_mat(ctx, "head.final_layer.adaLN_modulation.1.weight", 2 * H, H, ctx->h_ada, HL * 3 * H / 16);
    ctx->h_out = alloc_packed(ctx, L, H); add_mat(ctx, "head.final_layer.linear.weight", L, H, ctx->h_out, 0);
    const int R2 = 16;
    ctx->cproj = (float*)dalloc(ctx, (size_t)R2 * H * 4);
    ctx->mod = (float*)dalloc(ctx, (size_t)R2 * MODW * 4);
    for (HeadGen& g : ctx->hg) {      // m2 waits for the first general schedule
        g.zz = (float*)dalloc(ctx, (size_t)R2 * L * 4);
        g.x0p = (float*)dalloc(ctx, (size_t)R2 * L * 4);
        g.xh = (float*)dalloc(ctx, (size_t)R2 * H * 4);
    }
    // decode rows of the bf16 mode: final layer + solver update + next in-projection as one launch (headtail.hip)
    ctx->head_tail = c.xsplit == 1 && L == 64 && (H % 32) == 0 && vv_head_tail_init() == 0;
    if (const char* e = getenv("VVHIP_SOLVER_FUSE"); e && e[0] == '0') ctx->solver_fuse = false;      // A/B: update kernel + the in-projection GEMM
    if (const char* e = getenv("VVHIP_NAN_PROBE"); e && e[0] == '1') {
        ctx->probe_rec = (unsigned*)dalloc(ctx, PROBE_MAX * 16);
        ctx->probe_on = ctx->probe_rec != nullptr;
    }
    ctx->xh_parts = (float*)dalloc(ctx, (size_t)4 * R2 * H * 4);      // two generations: a layer reads one while writing the other
    ctx->hact = (float*)dalloc(ctx, (size_t)R2 * HF * 4);
    ctx->eps = (float*)dalloc(ctx, (size_t)R2 * L * 4);
    ctx->tmp1 = (float*)dalloc(ctx, (size_t)64 * H * 4);
    ctx->tmp2 = (float*)dalloc(ctx, (size_t)64 * 256 * 4);
    // ---- connectors ----
    auto mk_conn = [&](vv_ctx::Conn& cn, const std::string& p, int din) {
        cn.fc1 = alloc_packed(ctx, H, din); add_mat(ctx, p + "fc1.weight", H, din, cn.fc1, 0);
        cn.b1 = add_vec(ctx, p + "fc1.bias", H);
        cn.norm = add_vec(ctx, p + "norm.weight", H);
        cn.fc2 = alloc_packed(ctx, H, H); add_mat(ctx, p + "fc2.weight", H, H, cn.fc2, 0);
        cn.b2 = add_vec(ctx, p + "fc2.bias", H);
    };
    mk_conn(ctx->ac_conn, "ac_conn.", L);
    if (c.sem_dim > 0) mk_conn(ctx->sem_conn, "sem_conn.", c.sem_dim);
    ctx->ct1 = (float*)dalloc(ctx, (size_t)256 * H * 4);
    // ---- codecs ----
    if (build_codec(ctx, ctx->dec, "dec.", true, L, 1, c.n_slots)) { *out = ctx; return -1; }
    if (c.sem_dim > 0 && build_codec(ctx, ctx->senc, "senc.", false, c.sem_dim, 1, c.n_slots)) { *out = ctx; return -1; }
    if (c.has_acoustic_encoder && build_codec(ctx, ctx->aenc, "aenc.", false, L, c.enc_frames, 1)) { *out = ctx; return -1; }
    if (hipDeviceSynchronize() != hipSuccess || ctx->err[0]) { *out = ctx; return fail(ctx, "vv_create: allocation failed: %s", ctx->err); }
    ctx->creating = false;
    if (parent) {
        if (ctx->wshare_i != parent->wallocs.size() || ctx->w.size() != parent->w.size()) {
            *out = ctx;
            return fail(ctx, "vv_create_shared: the child registered %zu weight buffers / %zu parameters, the parent %zu / %zu -- different model configuration",
                        ctx->wshare_i, ctx->w.size(), parent->wallocs.size(), parent->w.size());
        }
        for (size_t i = 0; i < ctx->w.size(); ++i) {
            if (ctx->w[i].name != parent->w[i].name || ctx->w[i].nelem != parent->w[i].nelem) { *out = ctx; return fail(ctx, "vv_create_shared: parameter table differs at '%s'", ctx->w[i].name.c_str()); }
            ctx->w[i].loaded = parent->w[i].loaded;
            if (ctx->w[i].name == "lm_head.weight") ctx->w[i].dev = parent->w[i].dev;
        }
        ctx->lm_head = parent->lm_head; ctx->lm_head_loaded = parent->lm_head_loaded;
        ctx->scaling = parent->scaling; ctx->bias = parent->bias;
        { std::lock_guard<std::mutex> fl(g_family_mu); parent->n_children++; }
    }
    *out = ctx;
    return 0;
}

extern "C" int vv_create(const vv_config* cfg, vv_ctx** out) { return create_impl(cfg, nullptr, out); }

// A second context over the SAME weight storage as `parent` (which must be fully uploaded and is not a shared child itself): own KV
// caches, activations, tokenizer state, graphs and staging, sized by cfg's runtime fields (n_slots, max_ctx, max_rows, attn_splits,
// use_graph); the model fields must equal the parent's.  Two such contexts, each driven on its own stream, interleave two independent
// decode chains on one GPU over one copy of the weights: one chain's launch boundaries are filled by the other's kernels.
extern "C" int vv_create_shared(const vv_config* cfg, vv_ctx* parent, vv_ctx** out) {
    if (!parent) return fail(nullptr, "vv_create_shared: no parent context");
    if (parent->parent) return fail(nullptr, "vv_create_shared: the parent is itself a shared context; share from the owner of the weights");
    for (auto& w : parent->w)
        if (!w.loaded && !w.optional) return fail(nullptr, "vv_create_shared: parent parameter '%s' is not uploaded yet", w.name.c_str());
    vv_config a = *cfg, b = parent->c;
    a.n_slots = b.n_slots; a.max_ctx = b.max_ctx; a.max_rows = b.max_rows; a.attn_splits = b.attn_splits; a.use_graph = b.use_graph;
    if (a.xsplit < 1 || a.xsplit > 3) a.xsplit = 2;
    if (a.enc_frames < 1) a.enc_frames = 1;
    if (memcmp(&a, &b, sizeof(vv_config)) != 0) return fail(nullptr, "vv_create_shared: the model fields of the configuration differ from the parent's");
    int r = create_impl(cfg, parent, out);
    if (r != 0 && *out) { vv_ctx* c = *out; c->parent = nullptr; }      // a failed child holds no reference
    return r;
}

static void destroy_impl(vv_ctx* ctx) {
    if (!ctx) return;
    hipDeviceSynchronize();
    {   // shared children still read these weights: the last of them frees
        std::lock_guard<std::mutex> fl(g_family_mu);
        if (ctx->n_children > 0) { ctx->zombie = true; return; }
    }
    vv_ctx* par = ctx->parent;
    for (auto& g : ctx->graphs) hipGraphExecDestroy(g.second.exec);
    if (ctx->side_ready) {
        for (int j = 0; j < 8; ++j) { hipStreamDestroy(ctx->side[j]); hipEventDestroy(ctx->ev_join[j]); }
        hipEventDestroy(ctx->ev_fork);
    }
    for (void* p : ctx->allocs) hipFree(p);          // weights, KV caches, state and scratch buffers
    ctx->allocs.clear();
    if (ctx->stage) hipFree(ctx->stage);
    hipHostFree(ctx->rows_pin); hipHostFree(ctx->ids_pin);
    if (ctx->gws.err) hipHostFree(ctx->gws.err);
    for (int i = 0; i < vv_ctx::RING; ++i) if (ctx->ring_ev[i]) hipEventDestroy(ctx->ring_ev[i]);
    delete ctx;
    bool last_child = false;
    if (par) { std::lock_guard<std::mutex> fl(g_family_mu); last_child = (--par->n_children == 0 && par->zombie); }
    if (last_child) destroy_impl(par);
}
extern "C" void vv_destroy(vv_ctx* ctx) {
    VV_SHARED;                   // device-wide synchronisation + frees: never while another context's capture is open
    destroy_impl(ctx);
}

extern "C" int vv_num_weights(vv_ctx* ctx) { return (int)ctx->w.size(); }
extern "C" int vv_weight_info(vv_ctx* ctx, int idx, char* name, int cap, int64_t* nelem, int* loaded) {
    if (idx < 0 || idx >= (int)ctx->w.size()) return fail(ctx, "weight index out of range");
    const Weight& w = ctx->w[idx];
    snprintf(name, cap, "%s", w.name.c_str());
    if (nelem) *nelem = w.nelem;
    if (loaded) *loaded = (w.loaded || w.optional) ? 1 : 0;
    return 0;
}

extern "C" int vv_upload(vv_ctx* ctx, const char* name, const void* src, int src_dtype, int64_t nelem) {
    VV_SHARED;
    auto it = ctx->widx.find(name);
    if (it == ctx->widx.end()) return fail(ctx, "unknown parameter '%s'", name);
    Weight& w = ctx->w[it->second];
    if (ctx->parent) return fail(ctx, "parameter '%s': this context shares its parent's weights -- upload through the parent", name);
    {   // a child snapshots what it derives from the parameters when it is created (lm_head / tied embedding table, the valid-token
        // rows, the RoPE table from inv_freq, the speech factors): an upload behind its back would leave those stale
        std::lock_guard<std::mutex> fl(g_family_mu);
        if (ctx->n_children > 0)
            return fail(ctx, "parameter '%s': %d shared context(s) were created from this one and hold snapshots derived from its parameters -- "
                             "destroy them (model.close_lanes()), upload / merge, then fork again", name, ctx->n_children);
    }
    if (nelem != w.nelem) return fail(ctx, "parameter '%s': expected %lld elements, got %lld", name, (long long)w.nelem, (long long)nelem);
    const size_t esz = src_dtype ? 2 : 4;
    hipPointerAttribute_t attr;
    bool on_dev = (hipPointerGetAttributes(&attr, src) == hipSuccess) && (attr.type == hipMemoryTypeDevice);
    (void)hipGetLastError();
    const void* dsrc = src;
    if (!on_dev) {
        const size_t need = (size_t)nelem * esz;
        if (need > ctx->stage_bytes) {
            if (ctx->stage) hipFree(ctx->stage);
            ctx->stage = nullptr; ctx->stage_bytes = 0;
            HIPCHK(ctx, hipMalloc(&ctx->stage, need));
            ctx->stage_bytes = need;
        }
        HIPCHK(ctx, hipMemcpy(ctx->stage, src, need, hipMemcpyHostToDevice));
        dsrc = ctx->stage;
    }
    hipStream_t st = 0;
    if (w.kind == W_TABLE) {
        if (w.name == "lm_head.weight" && !ctx->lm_head_loaded) {
            ctx->lm_head = dalloc(ctx, (size_t)nelem * 2, false);
            if (!ctx->lm_head) return -1;
            ctx->lm_head_loaded = true; w.dev = ctx->lm_head;
        }
        if (src_dtype) HIPCHK(ctx, hipMemcpy(w.dev, dsrc, (size_t)nelem * 2, hipMemcpyDeviceToDevice));
        else VVCHK(vv_cvt_launch(dsrc, w.dev, nelem, 1, st));
    } else if (w.kind == W_MAT) {
        VVCHK(vv_pack_launch(dsrc, src_dtype, w.dev, w.N, w.K, w.pk, w.Cin, w.Cout, w.ksz, w.stride, st));
        VVTRY(lora_rebase(ctx, it->second, st));      // a parameter with a LoRA base snapshot: the upload is the new base
        VVTRY(w13_repack(ctx, it->second, st));
    } else {
        // fp32 vectors
        const float* f32 = (const float*)dsrc;
        float* tmp = nullptr;
        if (src_dtype) {
            tmp = (float*)dalloc(ctx, (size_t)nelem * 4, false);
            if (!tmp) return -1;
            VVCHK(vv_cvt_launch(dsrc, tmp, nelem, 0, st));
            f32 = tmp;
        }
        if (w.kind == W_DW) {
            VVCHK(vv_dw_transpose_launch(f32, (float*)w.dev, (int)(nelem / 7), st));
        } else if (w.kind == W_BIAS_REP) {
            for (int r = 0; r < w.rep; ++r)
                HIPCHK(ctx, hipMemcpyAsync((float*)w.dev + (size_t)r * nelem, f32, (size_t)nelem * 4, hipMemcpyDeviceToDevice, st));
        } else {
            HIPCHK(ctx, hipMemcpyAsync(w.dev, f32, (size_t)nelem * 4, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        dfree(ctx, tmp);
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    w.loaded = true;
    ctx->rope_ready = false;      // (cos, sin) table is rebuilt from the current inv_freq on the next decode step
    return 0;
}

int w13_repack(vv_ctx* ctx, int widx, hipStream_t st) {
    const Weight& w = ctx->w[widx];
    if (w.twin < 0) return 0;
    W13Twin& t = ctx->twins[w.twin];            // the matrix the parameter is part of (q / k / v: the layer's QKV): its own tile rows alone
    const int tile0 = (int)(((const char*)w.dev - (const char*)t.src) / ((int64_t)(t.K / 32) * 1024));
    VVCHK(vv_w13_pack_rows_launch(t.src, t.planes, t.N, t.K, tile0, w.N / 16, st));
    t.exact = -1;                               // the host's copy of the folded word is stale: the next sampler call reads it again
    return 0;
}

// statistics only: the ok words of a twin's tile rows, or (folded) the one word that says all of them are set, as the device holds them now
static bool w13_ok_words(const W13Twin& t, std::vector<unsigned>& ok, bool folded) {
    const int n_tiles = t.N / 16;
    ok.resize(folded ? 1 : n_tiles);
    return hipMemcpy(ok.data(), (const char*)t.planes + vv_w13_plane_bytes(t.N, t.K) + (size_t)(folded ? 2 * n_tiles : n_tiles) * 4, ok.size() * 4,
                     hipMemcpyDeviceToHost) == hipSuccess;
}

extern "C" int vv_set_speech_factors(vv_ctx* ctx, float scaling, float bias) {
    VV_SHARED;
    ctx->scaling = scaling; ctx->bias = bias;
    // 1 / scaling and -bias are arguments of the affine launch in front of the decoder: every graph captured with apply = 1
    return drop_graphs(ctx, {"dec:1:", "chain:1:"});
}

extern "C" int vv_set_valid_tokens(vv_ctx* ctx, const int* ids, int n) {
    VV_SHARED;
    if (n < 1 || n > 16) return fail(ctx, "n_valid must be in [1,16]");
    const int H = ctx->H;
    const void* table = ctx->lm_head_loaded ? ctx->lm_head : ctx->embed;
    void* rows = dalloc(ctx, (size_t)n * H * 2, false);
    if (!rows) return -1;
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= ctx->c.lm_vocab) return fail(ctx, "token id %d out of range", ids[i]);
        HIPCHK(ctx, hipMemcpy((char*)rows + (size_t)i * H * 2, (const char*)table + (size_t)ids[i] * H * 2, (size_t)H * 2, hipMemcpyDeviceToDevice));
    }
    if (!ctx->valid_w) ctx->valid_w = alloc_packed(ctx, 16, H);
    VVCHK(vv_pack_launch(rows, 1, ctx->valid_w, n, H, 0, 0, 0, 0, 0, 0));
    HIPCHK(ctx, hipDeviceSynchronize());
    dfree(ctx, rows);
    ctx->n_valid = n;
    for (int i = 0; i < n; ++i) ctx->valid_ids[i] = ids[i];
    return 0;
}
extern "C" int vv_check(vv_ctx* ctx, void* stream) {
    if (!ctx) return -1;
    return ksplit_check(ctx, (hipStream_t)stream);
}
extern "C" int vv_audio_to_pcm16(vv_ctx* ctx, void* stream, int n, int samples, const float* audio_dev, int16_t* pcm_out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || samples < 1) return fail(ctx, "vv_audio_to_pcm16: n and samples must be positive");
    VVCHK(vv_pcm16_launch(audio_dev, (short*)pcm_out_dev, n, samples, st));
    return 0;
}
extern "C" int vv_connect(vv_ctx* ctx, void* stream, int n, const float* latent_dev, const float* sem_dev, float* out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    const int H = ctx->H, L = ctx->c.latent_dim;
    for (int i0 = 0; i0 < n; i0 += 16) {
        const int nn = std::min(16, n - i0);
        float* out = out_dev + (size_t)i0 * H;
        VVGemm a1 = mk_gemm(ctx->ac_conn.fc1, latent_dev + (size_t)i0 * L, ctx->ct1, nn, H, L, L, H);
        a1.epi = VV_EPI_BIAS; a1.bias = ctx->ac_conn.b1; GEMM(a1);
        VVGemm a2 = mk_gemm(ctx->ac_conn.fc2, ctx->ct1, out, nn, H, H, H, H);
        a2.pro = VV_PRO_RMS; a2.nw = ctx->ac_conn.norm; a2.eps = 1e-6f; a2.epi = VV_EPI_BIAS; a2.bias = ctx->ac_conn.b2; GEMM(a2);
        if (sem_dev) {
            const int S = ctx->c.sem_dim;
            VVGemm s1 = mk_gemm(ctx->sem_conn.fc1, sem_dev + (size_t)i0 * S, ctx->ct1, nn, H, S, S, H);
            s1.epi = VV_EPI_BIAS; s1.bias = ctx->sem_conn.b1; GEMM(s1);
            VVGemm s2 = mk_gemm(ctx->sem_conn.fc2, ctx->ct1, out, nn, H, H, H, H);
            s2.pro = VV_PRO_RMS; s2.nw = ctx->sem_conn.norm; s2.eps = 1e-6f; s2.epi = VV_EPI_RESID; s2.bias = ctx->sem_conn.b2; GEMM(s2);
        }
    }
    return 0;
}

extern "C" int64_t vv_packed_bytes(int N, int K) { return vv_packed_elems(N, K) * 2; }
extern "C" int vv_pack_matrix(void* stream, const float* src_dev, void* dst_dev, int N, int K) {
    return vv_pack_launch(src_dev, 0, dst_dev, N, K, 0, 0, 0, 0, 0, (hipStream_t)stream);
}
extern "C" int64_t vv_stat(vv_ctx* ctx, int what) {
    switch (what) {
        case 0: return ctx->launches;
        case 2: return ctx->prof_raw_ns;          // last profile: sum of raw event-pair times over the decode-GEMV launches
        case 3: return ctx->prof_ev_over_ns;      // last profile: time of an empty event pair
        case 5: return ctx->foreign_nodes;        // nodes of the captured graphs that are not kernel launches (expected: 0)
        case 4: return ctx->capture_fallbacks;    // stream captures that did not close and ran eagerly instead (multi-threaded lanes)
        case 6: return ctx->seam_launches;        // head-tail seam launches of the last recorded sampler body
        case 8: return ctx->solver_fused;         // general-path step ends that carried the next in-projection (last recorded sampler body)
        case 7: return ctx->lora_base_bytes;      // bytes held by the base snapshots of LoRA-merged parameters
        case 9: case 11: {                        // the twins' ok words, read back now (the launches never need them on the host)
            VV_SHARED;
            if (hipDeviceSynchronize() != hipSuccess) return -1;
            std::vector<unsigned> tail;
            if (what == 11) {                     // tile rows of twinned matrices that stream bf16
                int64_t n = 0;
                for (const W13Twin& t : ctx->twins) {
                    if (!w13_ok_words(t, tail, false)) return -1;
                    for (unsigned v : tail) n += v == 0;
                }
                return n;
            }
            auto exact = [&](int widx) {          // the folded word: every tile row of the matrix is held by its twin
                const int ti = ctx->w[widx].twin;
                return ti >= 0 && w13_ok_words(ctx->twins[ti], tail, true) && tail[0] == 1;
            };
            int64_t n = 0;                        // head matrices exact in every tile row; gate and up of a layer count together
            for (const auto& l : ctx->hl) {
                if (exact(l.ig) && exact(l.iu)) n += 2;
                if (exact(l.id)) n += 1;
            }
            return n;
        }
        case 10: {                                // LM matrices (QKV, o, gate, up, down of every layer) that have a twin
            int64_t n = 0;
            for (const W13Twin& t : ctx->twins) n += t.lm;
            return n;
        }
        default: return (int64_t)ctx->graphs.size();
    }
}
