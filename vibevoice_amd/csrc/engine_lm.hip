// engine_lm.hip -- host side of libvvhip.so: the LM forward (prefill / batch decode / GEMV layers), KV cache entries, logits.
#include "engine_ctx.h"
#include "pass_plan.h"

// batch-decode projection (gemv16p.hip); inside a profile window the launch is also recorded for the family replay
int p16_gemv(vv_ctx* ctx, hipStream_t st, const void* W, const void* W2, const void* Xp, float* Y, void* Yp, const float* bias,
                    const float* gate, int T, int N, int K, int ldy, int ld_gate, int epi) {
    if (ctx->prof_on) {
        const double by = (double)vv_packed_elems(N, K) * 2.0 * (W2 ? 2.0 : 1.0) + (double)vv_packed_elems(16, K) * 2.0 +
                          (Yp ? (double)T * N * 2.0 : (double)T * N * 4.0 * (epi == VV_EPI_RESID || epi == VV_EPI_GATED_RESID ? 2.0 : 1.0));
        ctx->prof_other.push_back({1, by, [=](hipStream_t s) { return vv_gemv16p_launch(W, W2, Xp, Y, Yp, bias, gate, T, N, K, ldy, ld_gate, epi, s); }});
    }
    return vv_gemv16p_launch(W, W2, Xp, Y, Yp, bias, gate, T, N, K, ldy, ld_gate, epi, st);
}

// the struct form (round 6: RS / SH / PK operands); recorded for the family replay like p16_gemv
int p16_go(vv_ctx* ctx, hipStream_t st, const VVGemv16p& a, int epi, int flags) {
    if (ctx->prof_on) {
        const double by = (double)vv_packed_elems(a.N, a.K) * 2.0 * (a.W2 ? 2.0 : 1.0) + (double)vv_packed_elems(16, a.K) * 2.0 * ((flags & 2) ? 2.0 : 1.0) +
                          ((epi == VV_EPI_SWIGLU) ? (double)a.T * a.N * 2.0 : (double)a.T * a.N * 4.0 * (epi == VV_EPI_RESID || epi == VV_EPI_GATED_RESID ? 2.0 : 1.0)) +
                          ((flags & 4) ? (double)a.T * a.N * 2.0 : 0.0);
        const VVGemv16p ac = a;
        ctx->prof_other.push_back({1, by, [=](hipStream_t s) { return vv_gemv16p_launch2(&ac, epi, flags, s); }});
    }
    return vv_gemv16p_launch2(&a, epi, flags, st);
}
VVGemv16p p16_args(const void* W, const void* W2, const void* Xp, float* Y, void* Yp, int T, int N, int K, int ldy) {
    VVGemv16p a{};
    a.W = (const u32x4*)W; a.W2 = (const u32x4*)W2; a.Xp = (const u32x4*)Xp; a.Y = Y; a.Yp = (unsigned char*)Yp;
    a.T = T; a.N = N; a.K = K; a.ldy = ldy;
    return a;
}

// ---- the three layer paths of one LM pass.  The plan (pass_plan.h) names one and its attention; the launch sequence of each is what it was when they were interleaved ----
static char* lm_kc(vv_ctx* ctx, int l) { return (char*)ctx->kc + (size_t)l * ctx->layer_stride * 2; }
static char* lm_vc(vv_ctx* ctx, int l) { return (char*)ctx->vc + (size_t)l * ctx->layer_stride * 2; }
// cache slots past a prompt chunk inside its last 64-position stage: V zeroed once for every layer of this pass (0 x NaN, see misc.hip)
static int lm_zero_v_tail(vv_ctx* ctx, hipStream_t st, int R, int l0, int l1) {
    ctx->launches++;
    VVCHK(vv_kv_zero_v_tail_launch(lm_vc(ctx, l0), ctx->rows_dev, R, l1 - l0, ctx->Hkv, ctx->D, ctx->cache_stride, ctx->layer_stride, ctx->head_stride,
                                   ctx->c.max_ctx, st));
    return 0;
}
static int lm_finish(vv_ctx* ctx, hipStream_t st, int R, float* hidden_out, int final_norm) {
    ctx->launches++;
    if (final_norm) VVCHK(vv_rmsnorm_rows_launch(ctx->h, ctx->H, hidden_out, ctx->H, ctx->lm_norm, R, ctx->H, ctx->c.lm_eps, st));
    else VVCHK(vv_copy_launch(hidden_out, ctx->h, (size_t)R * ctx->H * 4, st));
    return 0;
}

// prompt prefill, bf16-activation mode (a contiguous chunk of >= 64 rows): packed activations + LDS-staged MFMA GEMMs + 64-row prefill attention
static int lm_prefill_layers(vv_ctx* ctx, hipStream_t st, int R, float* hidden_out, int l0, int l1, int final_norm) {
    const vv_config& c = ctx->c;
    const int H = ctx->H, D = ctx->D, Hq = ctx->Hq, Hkv = ctx->Hkv, I = ctx->I, QKV = ctx->QKV;
    for (int l = l0; l < l1; ++l) {
        auto& L = ctx->layers[l];
        char *kl = lm_kc(ctx, l), *vl = lm_vc(ctx, l);
        ctx->launches += 9;
        VVCHK(vv_pack_rows_launch(ctx->h, H, L.ln1, c.lm_eps, ctx->xp, R, H, st));
        // long prompts at head_dim 128: bias + RoPE + cache append in the QKV GEMM's epilogue; otherwise GEMM, then vv_rope_append
        const int fq = vv_gemm_qkv_rope_launch(L.wqkv, ctx->xp, L.bqkv, R, H, D, Hq, Hkv, ctx->rows_dev, ctx->rope_tab, ctx->qrot, kl, vl,
                                               ctx->cache_stride, ctx->head_stride, &ctx->gws, st);
        if (fq < 0) return fail(ctx, "vv_gemm_qkv_rope_launch failed (%d)", fq);
        if (fq == 0) {
            VVCHK(vv_gemm3_launch(L.wqkv, nullptr, ctx->xp, ctx->qkv, nullptr, L.bqkv, R, QKV, H, QKV, VV_EPI_BIAS, &ctx->gws, st));
            VVCHK(vv_rope_append_launch(D, ctx->qkv, ctx->rows_dev, ctx->inv_freq, ctx->qrot, kl, vl,
                                        R, Hq, Hkv, ctx->cache_stride, ctx->head_stride, st));
        }
        // the attention writes the o-projection's packed operand itself (K = Hq * D: whole 32-wide k-tiles)
        const bool apk = ((Hq * D) & 31) == 0;
        VVCHK(vv_attn_prefill4_launch(D, ctx->qrot, ctx->rows_dev, kl, vl, R, Hq, Hkv, ctx->cache_stride, ctx->head_stride, ctx->attn,
                                      apk ? ctx->xp : nullptr, st));
        if (!apk) VVCHK(vv_pack_rows_launch(ctx->attn, Hq * D, nullptr, 0.f, ctx->xp, R, Hq * D, st));
        VVCHK(vv_gemm3_launch(L.wo, nullptr, ctx->xp, ctx->h, nullptr, nullptr, R, H, Hq * D, H, VV_EPI_RESID, &ctx->gws, st));
        VVCHK(vv_pack_rows_launch(ctx->h, H, L.ln2, c.lm_eps, ctx->xp, R, H, st));
        VVCHK(vv_gemm3_launch(L.wg, L.wu, ctx->xp, nullptr, ctx->actp, nullptr, R, I, H, 0, VV_EPI_SWIGLU, &ctx->gws, st));
        VVCHK(vv_gemm3_launch(L.wd, nullptr, ctx->actp, ctx->h, nullptr, nullptr, R, H, I, H, VV_EPI_RESID, &ctx->gws, st));
    }
    return lm_finish(ctx, st, R, hidden_out, final_norm);
}

// decode rows (one cache each): RoPE + KV append + split attention in ONE launch (+ the merge launch when split).  out_packed (batch
// decode): the attention (or its merge) writes the o-projection's packed bf16 operand itself
static int lm_decode_attn(vv_ctx* ctx, hipStream_t st, int R, int l, const VVLmPlan& p, void* out_packed) {
    const vv_config& c = ctx->c;
    const int D = ctx->D, Hq = ctx->Hq, Hkv = ctx->Hkv;
    char *kl = lm_kc(ctx, l), *vl = lm_vc(ctx, l);
    const int attn_S = p.attn_S;
    ctx->launches += (attn_S > 1) ? 2 : 1;
    if (ctx->prof_on) {
        // algorithmic bytes: every cached position of every row once, K and V (bf16) + the row's q / new k, v / output
        const double by = (double)p.kv_positions * Hkv * D * 2.0 * 2.0 + (double)R * (ctx->QKV + Hq * D) * 4.0;
        const int xs = c.xsplit; vv_ctx* cx = ctx;
        ctx->prof_other.push_back({2, by, [=](hipStream_t s) {
            return vv_attn_fused_launch(D, xs, cx->qkv, cx->rows_dev, cx->rope_tab, kl, vl, R, Hq, Hkv, cx->cache_stride,
                                        cx->head_stride, attn_S, cx->pm, cx->pl, cx->po, cx->attn, out_packed, s); }});
    }
    VVCHK(vv_attn_fused_launch(D, c.xsplit, ctx->qkv, ctx->rows_dev, ctx->rope_tab, kl, vl, R, Hq, Hkv, ctx->cache_stride,
                               ctx->head_stride, attn_S, ctx->pm, ctx->pl, ctx->po, ctx->attn, out_packed, st));
    return 0;
}

// batch decode (5..16 rows, one cache each): packed-activation projections (gemv16p.hip)
static int lm_p16_layer(vv_ctx* ctx, hipStream_t st, int R, int l, int l0, int l1, const VVLmPlan& p) {
    const vv_config& c = ctx->c;
    const int H = ctx->H, Hq = ctx->Hq, D = ctx->D, I = ctx->I, QKV = ctx->QKV;
    auto& L = ctx->layers[l];
    if (l > l0) {
        // the previous layer's down projection left x * ln1 packed in p16_x and the rows' partial sums of squares in ssq_b
        ctx->launches += 1;
        VVGemv16p a = p16_args(L.wqkv, nullptr, ctx->p16_x, ctx->qkv, nullptr, R, QKV, H, QKV);
        a.bias = L.bqkv; a.ssq_in = ctx->ssq_b; a.ssq_tiles = H / 16; a.eps = c.lm_eps;
        VVCHK(p16_go(ctx, st, a, VV_EPI_BIAS, 1));
    } else {
        ctx->launches += 2;
        VVCHK(vv_pack16_launch(ctx->h, H, 1, L.ln1, c.lm_eps, nullptr, nullptr, 0, ctx->p16_x, R, H, st));
        VVCHK(p16_gemv(ctx, st, L.wqkv, nullptr, ctx->p16_x, ctx->qkv, nullptr, L.bqkv, nullptr, R, QKV, H, QKV, 0, VV_EPI_BIAS));
    }
    VVTRY(lm_decode_attn(ctx, st, R, l, p, ctx->p16_y));
    ctx->launches += 3;
    // o-projection: h += Wo . attn; its epilogue packs h * ln2 (-> p16_x) and the rows' partial sums of squares (-> ssq_a)
    VVGemv16p ao = p16_args(L.wo, nullptr, ctx->p16_y, ctx->h, ctx->p16_x, R, H, Hq * D, H);
    ao.pk_nw = L.ln2; ao.ssq_out = ctx->ssq_a;
    VVCHK(p16_go(ctx, st, ao, VV_EPI_RESID, 4));
    VVGemv16p ag = p16_args(L.wg, L.wu, ctx->p16_x, nullptr, ctx->p16_act, R, I, H, 0);
    ag.ssq_in = ctx->ssq_a; ag.ssq_tiles = H / 16; ag.eps = c.lm_eps;
    VVCHK(p16_go(ctx, st, ag, VV_EPI_SWIGLU, 1));
    // down projection: h += Wd . act; the next layer's QKV operand (h * its ln1 -> p16_x, ssq_b) unless this is the last layer
    VVGemv16p ad = p16_args(L.wd, nullptr, ctx->p16_act, ctx->h, nullptr, R, H, I, H);
    if (l + 1 < l1) {
        ad.Yp = (unsigned char*)ctx->p16_x; ad.pk_nw = ctx->layers[l + 1].ln1; ad.ssq_out = ctx->ssq_b;
        VVCHK(p16_go(ctx, st, ad, VV_EPI_RESID, 4));
    } else VVCHK(p16_go(ctx, st, ad, VV_EPI_RESID, 0));
    return 0;
}

// every other row set: the GEMM dispatcher's kernels (decode GEMV for <= 4 rows).  hp: extra K-split parts the residual stream h
// consists of on entry and on return (the down projection may split, the next layer's consumers add the parts back)
static int lm_gemv_layer(vv_ctx* ctx, hipStream_t st, int R, int l, int l1, const VVLmPlan& p, int& hp) {
    const vv_config& c = ctx->c;
    const int H = ctx->H, D = ctx->D, Hq = ctx->Hq, Hkv = ctx->Hkv, I = ctx->I, QKV = ctx->QKV;
    const int hps = ctx->c.max_rows * H;
    auto& L = ctx->layers[l];
    VVGemm g = mk_gemm(L.wqkv, ctx->h, ctx->qkv, R, QKV, H, H, QKV);
    g.pro = VV_PRO_RMS; g.nw = L.ln1; g.eps = c.lm_eps; g.epi = VV_EPI_BIAS; g.bias = L.bqkv; g.nt = 1;
    g.xa = ctx->h_parts; g.n_xa = hp; g.part_stride = hps;
    // W13: a launch streams its matrix's twin where the plan's form of it has a W13 instantiation (7B widths: QKV, gate/up and down;
    // o keeps bf16, below)
    const auto w13 = [&](const VVGemm& a, const void* t) { return p.w13 && t && vv_gemv_w13_form(&a, c.xsplit) >= 0; };
    if (w13(g, L.tqkv)) g.w13 = L.tqkv;
    GEMM(g);
    if (p.attn == VV_ATTN_FUSED) {
        VVTRY(lm_decode_attn(ctx, st, R, l, p, nullptr));
    } else {
        // rows of one launch share caches (prefill chunks): every append must land before any row attends
        char *kl = lm_kc(ctx, l), *vl = lm_vc(ctx, l);
        ctx->launches += 3;
        VVCHK(vv_rope_append_launch(D, ctx->qkv, ctx->rows_dev, ctx->inv_freq, ctx->qrot, kl, vl,
                                    R, Hq, Hkv, ctx->cache_stride, ctx->head_stride, st));
        if (p.attn == VV_ATTN_PREFILL4)       // prompt chunk, bf16 mode: 64 query rows x all heads of the group share every K/V block
            VVCHK(vv_attn_prefill4_launch(D, ctx->qrot, ctx->rows_dev, kl, vl, R, Hq, Hkv, ctx->cache_stride, ctx->head_stride, ctx->attn, nullptr, st));
        else {
            // ragged row sets (the streaming model's text windows) and the prompt chunks of the exact modes (xsplit 2, 3): the
            // split + merge pair, at most ws_rows rows per launch (its partial buffers); every row attends its own causal prefix
            for (int k = 0; k < p.attn_groups; ++k) {
                const int g0 = k * ctx->ws_rows, ng = std::min(ctx->ws_rows, R - g0);
                if (g0) ctx->launches += 2;
                VVCHK(vv_attn_launch(D, c.xsplit, ctx->qrot + (size_t)g0 * Hq * D, ctx->rows_dev + g0, kl, vl, ng, Hq, Hkv, ctx->cache_stride,
                                     ctx->head_stride, p.attn_S, ctx->pm, ctx->pl, ctx->po, ctx->attn + (size_t)g0 * Hq * D, st));
            }
        }
    }
    VVGemm go = mk_gemm(L.wo, ctx->attn, ctx->h, R, H, Hq * D, Hq * D, H);
    go.epi = VV_EPI_RESID; go.nt = 1;
    go.ya = ctx->h_parts; go.n_ya = hp; go.part_stride = hps;     // o_proj folds the parts back: h is whole again
    // o keeps its bf16 launch although the residual form has a W13 instantiation: 25.7 MB at 7B is too short a stream for the decode to
    // pay (6.94 us bf16 against 7.21 us W13 per launch, profiles/w13_lm_ab.json); its twin exists and is kept packed, unused
    GEMM(go);
    hp = 0;
    VVGemm gm = mk_gemm(L.wg, ctx->h, ctx->act, R, I, H, H, I);
    gm.W2 = (const u32x4*)L.wu; gm.pro = VV_PRO_RMS; gm.nw = L.ln2; gm.eps = c.lm_eps; gm.epi = VV_EPI_SWIGLU; gm.nt = 1;
    if (L.tu && w13(gm, L.tg)) { gm.w13 = L.tg; gm.w13_2 = L.tu; }
    GEMM(gm);
    VVGemm gd = mk_gemm(L.wd, ctx->act, ctx->h, R, H, I, I, H);
    gd.epi = VV_EPI_RESID; gd.nt = 1;
    if (l + 1 < l1) hp = ksplit_parts(ctx, gd, ctx->h_parts, hps);     // the last layer leaves h whole for the final norm
    if (w13(gd, L.td)) gd.w13 = L.td;
    GEMM(gd);
    return 0;
}

static int lm_body(vv_ctx* ctx, hipStream_t st, int R, const float* x_in, float* hidden_out, int l0, int l1, int final_norm, const VVLmPlan& p) {
    VVCHK(vv_copy_launch(ctx->h, x_in, (size_t)R * ctx->H * 4, st));   // copies / fills inside captured sequences are kernels, never memcpy / memset nodes (misc.hip)
    if (p.zero_v_tail) VVTRY(lm_zero_v_tail(ctx, st, R, l0, l1));      // every pass that reaches vv_attn_prefill4, on either route
    if (p.route == VV_LM_PREFILL) return lm_prefill_layers(ctx, st, R, hidden_out, l0, l1, final_norm);
    int hp = 0;                                    // extra parts the residual stream h currently consists of
    for (int l = l0; l < l1; ++l)
        VVTRY(p.route == VV_LM_P16 ? lm_p16_layer(ctx, st, R, l, l0, l1, p) : lm_gemv_layer(ctx, st, R, l, l1, p, hp));
    return lm_finish(ctx, st, R, hidden_out, final_norm);
}

// The prefill GEMM's K-split hand-off (prefill.hip g4_finish) reports a lost producer through a host-mapped word instead of
// hanging the GPU; the affected tile is wrong (summed from incomplete partials) and the arrival words are left untouched.  Recovery, done here at the next
// enqueue / vv_check: wait for the stream (nothing of that launch is in flight any more), re-zero the arrival words, clear the
// word and fail THIS call -- the caller knows the output of the prompt pass in flight is invalid and can retry; the context
// stays usable.
int ksplit_check(vv_ctx* ctx, hipStream_t st) {
    if (!(ctx->gws.err && *ctx->gws.err)) return 0;
    {   // stream-level waits only, under the lock captures take exclusively: a device-wide synchronize (or a null-stream memset) here
        // would invalidate a capture ANOTHER context of the process has open (lanes: vv_create_shared) -- exactly when one lane
        // recovers from a timed-out hand-off while the other keeps decoding.  The arrival words belong to this context; the launches
        // that touch them run on st (the only stream a prompt pass is enqueued on).
        VV_SHARED;
        hipStreamSynchronize(st);
        if (ctx->gws.flags) { hipMemsetAsync(ctx->gws.flags, 0, 256 * sizeof(unsigned), st); hipStreamSynchronize(st); }
    }
    *ctx->gws.err = 0u;
    return fail(ctx, "prefill GEMM: a K-split hand-off timed out (lost producer workgroup); the prompt pass that was in flight is invalid -- "
                     "the arrival words were re-armed, retry the pass (VVHIP_NO_KSPLIT=1 disables the split)");
}
extern "C" int vv_lm_forward(vv_ctx* ctx, void* stream, int n_rows, const vv_row* rows, const float* x_in_dev, float* hidden_out_dev) {
    return vv_lm_forward_range(ctx, stream, n_rows, rows, x_in_dev, hidden_out_dev, 0, ctx->c.lm_layers, 1);
}
extern "C" int vv_lm_forward_range(vv_ctx* ctx, void* stream, int n_rows, const vv_row* rows, const float* x_in_dev,
                                   float* hidden_out_dev, int l0, int l1, int final_norm) {
    hipStream_t st = (hipStream_t)stream;
    if (l0 < 0 || l1 > ctx->c.lm_layers || l0 >= l1) return fail(ctx, "layer range [%d,%d) invalid", l0, l1);
    if (n_rows < 1 || n_rows > ctx->c.max_rows) return fail(ctx, "n_rows %d out of range [1,%d]", n_rows, ctx->c.max_rows);
    if (ksplit_check(ctx, st)) return -1;
    (void)hipGetLastError();            // a stale error of this host thread (another library's query) is not a launch failure of ours
    for (int i = 0; i < n_rows; ++i) {
        if (rows[i].cache < 0 || rows[i].cache >= 2 * ctx->c.n_slots) return fail(ctx, "row %d: cache id %d out of range", i, rows[i].cache);
        if (rows[i].pos < 0 || rows[i].pos >= ctx->c.max_ctx) return fail(ctx, "row %d: position %d exceeds max_ctx %d", i, rows[i].pos, ctx->c.max_ctx);
    }
    const int slot = ring_acquire(ctx);
    VVRow* pin = ctx->rows_pin + (size_t)slot * ctx->rows_cap;
    for (int i = 0; i < n_rows; ++i) { pin[i].cache = rows[i].cache; pin[i].pos = rows[i].pos; }
    HIPCHK(ctx, hipMemcpyAsync(ctx->rows_dev, pin, sizeof(VVRow) * n_rows, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ctx->ring_ev[slot], st));
    ctx->launches = 0;
    if (!ctx->rope_ready) {                   // (cos, sin) table of every position, once the inv_freq parameter is in place
        VVCHK(vv_rope_table_launch(ctx->inv_freq, ctx->rope_tab, ctx->c.max_ctx, ctx->D / 2, st));
        ctx->rope_ready = true;
    }
    VVLmPlan plan;
    if (vv_lm_pass_plan(pin, n_rows, {ctx->ws_rows, ctx->c.attn_splits, ctx->Hkv, ctx->tile3_ok, ctx->attn2_ok, ctx->p16_ok, ctx->w13_lm}, &plan))
        return fail(ctx, "a launch of %d rows must be consecutive positions of one cache (decode / ragged launches take <= %d rows)", n_rows, ctx->ws_rows);
    char key[160]; snprintf(key, 160, "lm:%d:%p:%p:%d:%d:%d:%d:%d", n_rows, (const void*)x_in_dev, (void*)hidden_out_dev, l0, l1, final_norm,
                            plan.key_mode, plan.key_split);
    return graphed(ctx, key, st, [&]() { return lm_body(ctx, st, n_rows, x_in_dev, hidden_out_dev, l0, l1, final_norm, plan); });
}

extern "C" int vv_kv_import_at(vv_ctx* ctx, void* stream, int cache, int layer, int pos0, int n_pos, const void* k_dev, const void* v_dev, int src_dtype) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (cache < 0 || cache >= 2 * ctx->c.n_slots) return fail(ctx, "cache id %d out of range", cache);
    if (layer < 0 || layer >= ctx->c.lm_layers) return fail(ctx, "layer %d out of range", layer);
    if (pos0 < 0 || n_pos < 0 || (int64_t)pos0 + n_pos > ctx->c.max_ctx) return fail(ctx, "positions [%d, %d) exceed max_ctx %d", pos0, pos0 + n_pos, ctx->c.max_ctx);
    if (n_pos == 0) return 0;
    const size_t off = ((size_t)cache * ctx->cache_stride + (size_t)layer * ctx->layer_stride) * 2;
    VVCHK(vv_kv_import_launch(k_dev, v_dev, src_dtype, (char*)ctx->kc + off, (char*)ctx->vc + off, n_pos, ctx->Hkv, ctx->D, ctx->head_stride, pos0, st));
    return 0;
}
extern "C" int vv_kv_move(vv_ctx* ctx, void* stream, int cache, int src_pos, int dst_pos) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (cache < 0 || cache >= 2 * ctx->c.n_slots) return fail(ctx, "cache id %d out of range", cache);
    if (src_pos < 0 || dst_pos < 0 || src_pos >= ctx->c.max_ctx || dst_pos >= ctx->c.max_ctx)
        return fail(ctx, "vv_kv_move: positions %d -> %d outside [0, %d)", src_pos, dst_pos, ctx->c.max_ctx);
    if (src_pos == dst_pos) return 0;
    const size_t off = (size_t)cache * ctx->cache_stride * 2;
    ctx->launches++;
    VVCHK(vv_kv_move_launch((char*)ctx->kc + off, (char*)ctx->vc + off, ctx->c.lm_layers, ctx->Hkv, ctx->D, ctx->layer_stride, ctx->head_stride,
                            src_pos, dst_pos, st));
    return 0;
}
extern "C" int vv_kv_import(vv_ctx* ctx, void* stream, int cache, int layer, int n_pos, const void* k_dev, const void* v_dev, int src_dtype) {
    return vv_kv_import_at(ctx, stream, cache, layer, 0, n_pos, k_dev, v_dev, src_dtype);
}
extern "C" int vv_kv_export(vv_ctx* ctx, void* stream, int cache, int layer, int pos0, int n_pos, void* k_out_dev, void* v_out_dev, int dst_dtype) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (cache < 0 || cache >= 2 * ctx->c.n_slots) return fail(ctx, "cache id %d out of range", cache);
    if (layer < 0 || layer >= ctx->c.lm_layers) return fail(ctx, "layer %d out of range", layer);
    if (pos0 < 0 || n_pos < 0 || (int64_t)pos0 + n_pos > ctx->c.max_ctx)
        return fail(ctx, "vv_kv_export: positions [%d, %lld) exceed max_ctx %d", pos0, (long long)pos0 + n_pos, ctx->c.max_ctx);
    if (dst_dtype != 0 && dst_dtype != 1) return fail(ctx, "vv_kv_export: dst_dtype %d (0 = fp32, 1 = bf16)", dst_dtype);
    if (n_pos == 0) return 0;
    if (!k_out_dev || !v_out_dev) return fail(ctx, "vv_kv_export: null output");
    if (((uintptr_t)k_out_dev | (uintptr_t)v_out_dev) & 15) return fail(ctx, "vv_kv_export: outputs must be 16-byte aligned");
    const size_t off = ((size_t)cache * ctx->cache_stride + (size_t)layer * ctx->layer_stride) * 2;
    VVCHK(vv_kv_export_launch((char*)ctx->kc + off, (char*)ctx->vc + off, k_out_dev, v_out_dev, dst_dtype, n_pos, ctx->Hkv, ctx->D, ctx->head_stride, pos0, st));
    return 0;
}
extern "C" int64_t vv_kv_snapshot_bytes(vv_ctx* ctx, int n_pos) {
    if (n_pos < 0 || n_pos > ctx->c.max_ctx) return fail(ctx, "vv_kv_snapshot_bytes: %d positions outside [0, max_ctx %d]", n_pos, ctx->c.max_ctx);
    return (int64_t)ctx->c.lm_layers * ctx->Hkv * ((n_pos + 31) & ~31) * ctx->D * 2;
}
// snapshot (to_cache = 0) and restore (1): one eager launch over K, V and every layer
static int kv_span_copy(vv_ctx* ctx, void* stream, const char* who, int cache, int n_pos, void* k_dev, void* v_dev, int to_cache) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (cache < 0 || cache >= 2 * ctx->c.n_slots) return fail(ctx, "%s: cache id %d out of range", who, cache);
    if (n_pos < 0 || n_pos > ctx->c.max_ctx) return fail(ctx, "%s: %d positions outside [0, max_ctx %d]", who, n_pos, ctx->c.max_ctx);
    if (n_pos == 0) return 0;
    if (!k_dev || !v_dev) return fail(ctx, "%s: null snapshot buffer", who);
    if (((uintptr_t)k_dev | (uintptr_t)v_dev) & 15) return fail(ctx, "%s: snapshot buffers must be 16-byte aligned", who);
    const size_t off = (size_t)cache * ctx->cache_stride * 2;
    VVCHK(vv_kv_span_copy_launch((char*)ctx->kc + off, (char*)ctx->vc + off, k_dev, v_dev, to_cache, ctx->c.lm_layers, ctx->Hkv, ctx->D,
                                 ctx->layer_stride, ctx->head_stride, n_pos, st));
    return 0;
}
extern "C" int vv_kv_snapshot(vv_ctx* ctx, void* stream, int cache, int n_pos, void* k_out_dev, void* v_out_dev) {
    return kv_span_copy(ctx, stream, "vv_kv_snapshot", cache, n_pos, k_out_dev, v_out_dev, 0);
}
extern "C" int vv_kv_restore(vv_ctx* ctx, void* stream, int cache, int n_pos, const void* k_dev, const void* v_dev) {
    return kv_span_copy(ctx, stream, "vv_kv_restore", cache, n_pos, (void*)k_dev, (void*)v_dev, 1);
}
extern "C" int vv_add_type_embedding(vv_ctx* ctx, void* stream, int n, const float* x_dev, int type, float* out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->tts_types) return fail(ctx, "engine was not configured with tts_layers");
    if (type < 0 || type > 1) return fail(ctx, "type must be 0 (speech) or 1 (text)");
    VVCHK(vv_add_rows_launch(x_dev, ctx->tts_types + (size_t)type * ctx->H, out_dev, n, ctx->H, st));
    return 0;
}

extern "C" int vv_eos_logit(vv_ctx* ctx, void* stream, int n, const float* hidden_dev, float* out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->eos_w1) return fail(ctx, "engine was not configured with tts_layers");
    if (n < 1 || n > 16) return fail(ctx, "vv_eos_logit: n must be in [1,16]");
    const int H = ctx->H;
    VVGemm g1 = mk_gemm(ctx->eos_w1, hidden_dev, ctx->ct1, n, H, H, H, H);
    g1.epi = VV_EPI_BIAS; g1.bias = ctx->eos_b1; GEMM(g1);
    VVCHK(vv_relu_launch(ctx->ct1, n * H, st));
    VVGemm g2 = mk_gemm(ctx->eos_w2, ctx->ct1, out_dev, n, 1, H, H, 1);
    g2.epi = VV_EPI_BIAS; g2.bias = ctx->eos_b2; GEMM(g2);
    return 0;
}

extern "C" int vv_embed(vv_ctx* ctx, void* stream, int n, const int* ids, float* out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || n > ctx->ids_cap) return fail(ctx, "vv_embed: n must be in [1,%d] (max(64, max_rows))", ctx->ids_cap);
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= ctx->c.lm_vocab) return fail(ctx, "token id %d out of range", ids[i]);
    const int slot = ring_acquire(ctx);
    int* pin = ctx->ids_pin + (size_t)slot * ctx->ids_cap;
    memcpy(pin, ids, sizeof(int) * n);
    HIPCHK(ctx, hipMemcpyAsync(ctx->ids_dev, pin, sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ctx->ring_ev[slot], st));
    VVCHK(vv_embed_launch(ctx->embed, ctx->ids_dev, out_dev, n, ctx->H, st));
    return 0;
}

extern "C" int vv_lm_logits_full(vv_ctx* ctx, void* stream, int n, const float* hidden_dev, float* logits_out_dev) {
    VV_SHARED;
    const void* table = ctx->lm_head_loaded ? ctx->lm_head : ctx->embed;
    if (!table) return fail(ctx, "vv_lm_logits_full: no lm_head / embedding table has been uploaded");
    if (n < 1 || n > 16) return fail(ctx, "vv_lm_logits_full: n must be in [1,16]");
    if (ctx->H & 7) return fail(ctx, "vv_lm_logits_full: hidden size %d is not a multiple of 8", ctx->H);
    VVCHK(vv_logits_full_launch(table, hidden_dev, logits_out_dev, n, ctx->c.lm_vocab, ctx->H, (hipStream_t)stream));
    return 0;
}
extern "C" int vv_lm_warp_valid(vv_ctx* ctx, void* stream, int n, const float* logits_dev, const unsigned char* seen_dev,
                                float repetition_penalty, float temperature, int do_sample, int top_k, float top_p, float min_p,
                                float* out_dev, int* survivors_dev) {
    VV_SHARED;
    if (n < 1 || n > 16) return fail(ctx, "vv_lm_warp_valid: n must be in [1,16]");
    if (!ctx->valid_w || ctx->n_valid < 1) return fail(ctx, "vv_lm_warp_valid: vv_set_valid_tokens has not been called");
    if (!(repetition_penalty > 0.f)) return fail(ctx, "vv_lm_warp_valid: repetition_penalty %g must be > 0", (double)repetition_penalty);
    if (!(temperature > 0.f)) return fail(ctx, "vv_lm_warp_valid: temperature %g must be > 0", (double)temperature);
    if (top_k < 0) return fail(ctx, "vv_lm_warp_valid: top_k %d must be >= 0", top_k);
    if (!(top_p >= 0.f && top_p <= 1.f)) return fail(ctx, "vv_lm_warp_valid: top_p %g must be in [0,1]", (double)top_p);
    if (!(min_p >= 0.f && min_p <= 1.f)) return fail(ctx, "vv_lm_warp_valid: min_p %g must be in [0,1]", (double)min_p);
    if (!seen_dev && repetition_penalty != 1.f) return fail(ctx, "vv_lm_warp_valid: a repetition_penalty other than 1 needs the seen mask");
    if (!logits_dev || !out_dev || !survivors_dev) return fail(ctx, "vv_lm_warp_valid: null logits / out / survivors pointer");
    ctx->launches++;
    VVCHK(vv_warp_valid_launch(logits_dev, seen_dev, out_dev, survivors_dev, n, ctx->c.lm_vocab, ctx->valid_ids, ctx->n_valid,
                               repetition_penalty, temperature, do_sample, top_k, top_p, min_p, (hipStream_t)stream));
    return 0;
}
extern "C" int vv_noise_rows(vv_ctx* ctx, void* stream, int n, const vv_noise_key* keys_host, uint32_t stream0, int n_streams, int n_t,
                             int width, float* out_dev) {
    VV_SHARED;
    if (n < 1 || n > 16) return fail(ctx, "vv_noise_rows: n = %d must be in [1,16]", n);
    if (n_t < 1) return fail(ctx, "vv_noise_rows: n_t = %d must be >= 1", n_t);
    if (n_streams < 1 || n_streams > 65) return fail(ctx, "vv_noise_rows: n_streams = %d must be in [1,65]", n_streams);
    if (width < 4 || (width & 3)) return fail(ctx, "vv_noise_rows: width = %d must be a positive multiple of 4", width);
    if ((int64_t)n_streams * n * n_t * width >= ((int64_t)1 << 31))
        return fail(ctx, "vv_noise_rows: %d x %d x %d x %d elements: the total must stay below 2^31", n_streams, n, n_t, width);
    if (!keys_host || !out_dev) return fail(ctx, "vv_noise_rows: null keys / out pointer");
    if ((uintptr_t)out_dev & 15u) return fail(ctx, "vv_noise_rows: out_dev must be 16-byte aligned");
    static_assert(sizeof(vv_noise_key) == 16, "vv_noise_key is four uint32 words");
    ctx->launches++;
    VVCHK(vv_noise_rows_launch(out_dev, n, reinterpret_cast<const uint32_t*>(keys_host), stream0, n_streams, n_t, width, (hipStream_t)stream));
    return 0;
}
extern "C" int vv_lm_logits(vv_ctx* ctx, void* stream, int n, const float* hidden_dev, float* logits_out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->valid_w) return fail(ctx, "vv_set_valid_tokens has not been called");
    if (n < 1 || n > 16) return fail(ctx, "vv_lm_logits: n must be in [1,16]");
    VVGemm g = mk_gemm(ctx->valid_w, hidden_dev, logits_out_dev, n, ctx->n_valid, ctx->H, ctx->H, ctx->n_valid);
    GEMM(g);
    return 0;
}
