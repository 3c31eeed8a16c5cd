// engine_lora.hip -- device-resident LoRA adapters: base snapshots, in-place merge / reset of packed parameters, parameter read-back.
#include "engine_ctx.h"

// what every raw launch of the merge kernel is checked for, before anything is enqueued
static int lora_args_ok(vv_ctx* ctx, const char* what, int N, int K, const void* a, const void* b, int r, float scale) {
    if (N < 1 || K < 1 || vv_packed_elems(N, K) * 2 >= ((int64_t)1 << 31))
        return fail(ctx, "%s: N = %d, K = %d: a packed matrix of 1 .. 2^31 - 1 bytes", what, N, K);
    if (r < 1 || r > 256) return fail(ctx, "%s: r = %d is outside [1, 256]", what, r);
    if ((int64_t)N * r >= ((int64_t)1 << 31) || (int64_t)K * r >= ((int64_t)1 << 31)) return fail(ctx, "%s: a factor of 2^31 elements or more", what);
    if (!std::isfinite(scale)) return fail(ctx, "%s: scale is not finite", what);
    if (!a || !b) return fail(ctx, "%s: null factor (a_dev %p, b_dev %p)", what, a, b);
    if (((uintptr_t)a | (uintptr_t)b) & 15) return fail(ctx, "%s: a_dev / b_dev must be 16-byte aligned", what);
    return 0;
}

extern "C" int vv_unpack_matrix(void* stream, const void* packed_dev, float* dst_dev, int N, int K) {
    if (N < 1 || K < 1 || vv_packed_elems(N, K) * 2 >= ((int64_t)1 << 31)) return fail(nullptr, "vv_unpack_matrix: N = %d, K = %d", N, K);
    if (!packed_dev || !dst_dev || (((uintptr_t)packed_dev | (uintptr_t)dst_dev) & 15)) return fail(nullptr, "vv_unpack_matrix: null or misaligned pointer");
    vv_ctx* ctx = nullptr;
    VVCHK(vv_unpack_launch(packed_dev, dst_dev, N, K, (hipStream_t)stream));
    return 0;
}

extern "C" int vv_lora_merge_raw(void* stream, const void* base_packed_dev, void* dst_packed_dev, int N, int K, const float* a_dev,
                                 const float* b_dev, int r, float scale, int delta_bf16) {
    vv_ctx* ctx = nullptr;
    VVTRY(lora_args_ok(ctx, "vv_lora_merge_raw", N, K, a_dev, b_dev, r, scale));
    if (!base_packed_dev || !dst_packed_dev || (((uintptr_t)base_packed_dev | (uintptr_t)dst_packed_dev) & 15))
        return fail(ctx, "vv_lora_merge_raw: null or misaligned packed matrix");
    VVCHK(vv_lora_merge_launch(base_packed_dev, dst_packed_dev, N, K, a_dev, b_dev, r, scale, delta_bf16 ? 1 : 0, (hipStream_t)stream));
    return 0;
}

// the parameter the three engine entries work on: vv_upload's guards, then a plain linear W_MAT that has been uploaded
static int lora_target(vv_ctx* ctx, const char* what, const char* name, int* idx) {
    if (!name) return fail(ctx, "%s: no parameter name", what);
    if (ctx->parent) return fail(ctx, "%s('%s'): this context shares its parent's weights -- go through the parent", what, name);
    {
        std::lock_guard<std::mutex> fl(g_family_mu);
        if (ctx->n_children > 0)
            return fail(ctx, "%s('%s'): %d shared context(s) were created from this one and read these weights -- destroy them "
                             "(model.close_lanes()) first", what, name, ctx->n_children);
    }
    auto it = ctx->widx.find(name);
    if (it == ctx->widx.end()) return fail(ctx, "%s: unknown parameter '%s'", what, name);
    const Weight& w = ctx->w[it->second];
    if (w.kind != W_MAT || w.pk != 0)
        return fail(ctx, "%s: parameter '%s' is not a plain linear matrix (tables, vectors and convolution weights have no LoRA path)", what, name);
    if (!w.loaded) return fail(ctx, "%s: parameter '%s' is not uploaded yet", what, name);
    *idx = it->second;
    return 0;
}

// vv_upload on a parameter that has a snapshot: what was uploaded is the new base, and no adapter is merged into it
int lora_rebase(vv_ctx* ctx, int widx, hipStream_t st) {
    auto it = ctx->lora_base.find(widx);
    if (it == ctx->lora_base.end()) return 0;
    VVCHK(vv_copy_launch(it->second.snap, ctx->w[widx].dev, it->second.bytes, st));
    it->second.merged = false;
    return 0;
}

extern "C" int vv_weight_shape(vv_ctx* ctx, const char* name, int* N, int* K) {
    auto it = name ? ctx->widx.find(name) : ctx->widx.end();
    if (it == ctx->widx.end()) return fail(ctx, "vv_weight_shape: unknown parameter '%s'", name ? name : "(null)");
    const Weight& w = ctx->w[it->second];
    if (w.kind != W_MAT || w.pk != 0) return fail(ctx, "vv_weight_shape: parameter '%s' is not a plain linear matrix", name);
    if (N) *N = w.N;
    if (K) *K = w.K;
    return 0;
}

extern "C" int vv_weight_read(vv_ctx* ctx, void* stream, const char* name, float* out_dev) {
    VV_SHARED;
    int i = -1;
    VVTRY(lora_target(ctx, "vv_weight_read", name, &i));
    if (!out_dev || ((uintptr_t)out_dev & 15)) return fail(ctx, "vv_weight_read('%s'): out_dev is null or not 16-byte aligned", name);
    const Weight& w = ctx->w[i];
    ctx->launches++;
    VVCHK(vv_unpack_launch(w.dev, out_dev, w.N, w.K, (hipStream_t)stream));
    return 0;
}

extern "C" int vv_lora_merge(vv_ctx* ctx, void* stream, const char* name, const float* a_dev, const float* b_dev, int r, float scale,
                             int delta_bf16) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    int i = -1;
    VVTRY(lora_target(ctx, "vv_lora_merge", name, &i));
    const Weight& w = ctx->w[i];
    VVTRY(lora_args_ok(ctx, "vv_lora_merge", w.N, w.K, a_dev, b_dev, r, scale));
    auto it = ctx->lora_base.find(i);
    if (it == ctx->lora_base.end()) {
        const size_t bytes = (size_t)vv_packed_elems(w.N, w.K) * 2;
        void* snap = dalloc(ctx, bytes, false);
        if (!snap) return -1;
        it = ctx->lora_base.emplace(i, vv_ctx::LoraBase{snap, bytes, false}).first;
        ctx->lora_base_bytes += (int64_t)bytes;
        ctx->launches++;
        VVCHK(vv_copy_launch(snap, w.dev, bytes, st));
    }
    ctx->launches++;
    VVCHK(vv_lora_merge_launch(it->second.snap, w.dev, w.N, w.K, a_dev, b_dev, r, scale, delta_bf16 ? 1 : 0, st));
    it->second.merged = true;
    VVTRY(w13_repack(ctx, i, st));
    return 0;
}

extern "C" int vv_lora_reset(vv_ctx* ctx, void* stream, const char* name) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    int only = -1;
    if (name) VVTRY(lora_target(ctx, "vv_lora_reset", name, &only));
    else {
        if (ctx->parent) return fail(ctx, "vv_lora_reset: this context shares its parent's weights -- go through the parent");
        std::lock_guard<std::mutex> fl(g_family_mu);
        if (ctx->n_children > 0) return fail(ctx, "vv_lora_reset: %d shared context(s) read these weights -- destroy them (model.close_lanes()) first", ctx->n_children);
    }
    for (auto& kv : ctx->lora_base) {
        if ((only >= 0 && kv.first != only) || !kv.second.merged) continue;
        ctx->launches++;
        VVCHK(vv_copy_launch(ctx->w[kv.first].dev, kv.second.snap, kv.second.bytes, st));
        kv.second.merged = false;
        VVTRY(w13_repack(ctx, kv.first, st));
    }
    return 0;
}
