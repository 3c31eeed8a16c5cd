// engine_prof.hip -- host side of libvvhip.so: per-launch profiling, the timing builds' timeline, the NaN probe, raw test entries.
#include "engine_ctx.h"
#include "vv_w13.h"

static __global__ void vv_nan_probe_kernel(const float* __restrict__ p, int n, unsigned* __restrict__ rec) {
    unsigned cnt = 0, first = 0xffffffffu, mx = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float v = p[i];
        if (!(fabsf(v) <= 3.0e38f)) { cnt++; first = min(first, (unsigned)i); }
        else mx = max(mx, __float_as_uint(fabsf(v)));
    }
    if (cnt) { atomicAdd(rec, cnt); atomicMax(rec + 1, 0xffffffffu - first); }
    atomicMax(rec + 2, mx);
}
void nan_probe(vv_ctx* ctx, hipStream_t st, const char* name, const void* p, size_t n) {
    if (!ctx->probe_on || !p || n == 0) return;
    const int id = (int)ctx->probe_names.size();
    if (id >= PROBE_MAX) return;
    ctx->probe_names.push_back(name);
    if (id == 0) (void)vv_zero_launch(ctx->probe_rec, PROBE_MAX * 16, st);      // a kernel, like every fill of a captured sequence
    hipLaunchKernelGGL(vv_nan_probe_kernel, dim3(64), dim3(256), 0, st, (const float*)p, (int)n, ctx->probe_rec + 4 * id);
}
void nan_probe_report(vv_ctx* ctx, hipStream_t st, const char* what) {
    if (!ctx->probe_on) return;
    std::vector<unsigned> h(PROBE_MAX * 4);
    const hipError_t e1 = hipStreamSynchronize(st);
    const hipError_t e2 = hipMemcpy(h.data(), ctx->probe_rec, PROBE_MAX * 16, hipMemcpyDeviceToHost);
    const int call = ctx->probe_calls++;
    if (e1 != hipSuccess || e2 != hipSuccess) { fprintf(stderr, "[nan_probe] %s call %d: sync %d copy %d\n", what, call, (int)e1, (int)e2); (void)hipGetLastError(); return; }
    { const size_t ns = ctx->probe_names.size(); bool tail_dirty = false;      // the words past the last stage must still be zeros
      for (size_t i = 4 * ns; i < (size_t)PROBE_MAX * 4; ++i) if (h[i]) { tail_dirty = true; break; }
      if (tail_dirty) fprintf(stderr, "[nan_probe] %s call %d (prof %d): record buffer %p holds words nobody wrote: %08x %08x %08x %08x | %08x %08x %08x %08x (last 4 words)\n",
                              what, call, (int)ctx->prof_on, (void*)ctx->probe_rec, h[0], h[1], h[2], h[3], h[4092], h[4093], h[4094], h[4095]); }
    int bad = 0;
    for (size_t i = 0; i < ctx->probe_names.size(); ++i) if (h[4 * i]) bad++;
    if (!bad) { if (call < 6) fprintf(stderr, "[nan_probe] %s call %d: %zu stages clean\n", what, call, ctx->probe_names.size()); return; }
    fprintf(stderr, "[nan_probe] %s call %d: %d of %zu stages hold non-finite values\n", what, call, bad, ctx->probe_names.size());
    int shown = 0;
    for (size_t i = 0; i < ctx->probe_names.size() && shown < 12; ++i) {
        float mx; memcpy(&mx, &h[4 * i + 2], 4);
        if (h[4 * i] || (i + 1 < ctx->probe_names.size() && h[4 * (i + 1)] && !shown)) {
            fprintf(stderr, "[nan_probe]   stage %3zu %-28s non-finite %u (first at %u), finite absmax %.4e\n", i, ctx->probe_names[i].c_str(), h[4 * i],
                    h[4 * i] ? 0xffffffffu - h[4 * i + 1] : 0u, mx);
            if (h[4 * i]) shown++;
        }
    }
}
static double gemm_bytes(const VVGemm& g) {
    // algorithmic bytes of one launch: packed weights once (+ second matrix), activations in, result out (RMW epilogues twice)
    double w = (double)vv_packed_elems(g.N, g.K) * 2.0 * (g.W2 ? 2.0 : 1.0);
    if (g.w13) w = (double)vv_w13_plane_bytes(g.N, g.K) * (g.W2 ? 2.0 : 1.0);      // the bytes actually streamed
    double x = (double)g.T * g.K * 4.0;
    double y = (double)g.T * g.N * 4.0 * ((g.epi == VV_EPI_RESID || g.epi == VV_EPI_GATED_RESID) ? 2.0 : 1.0);
    return w + x + y;
}
int gemm_prof(vv_ctx* ctx, const VVGemm& g, hipStream_t st) {
    if ((size_t)(2 * ctx->prof_n + 2) > ctx->prof_ev.size()) {
        size_t old = ctx->prof_ev.size();
        ctx->prof_ev.resize(old + 2048);
        for (size_t i = old; i < ctx->prof_ev.size(); ++i) hipEventCreate(&ctx->prof_ev[i]);
    }
    ctx->prof_stream = st;
    hipEventRecord(ctx->prof_ev[2 * ctx->prof_n], st);
    int r = vv_gemm_launch(g, ctx->c.xsplit, st);
    hipEventRecord(ctx->prof_ev[2 * ctx->prof_n + 1], st);
    ctx->prof_n++;
    ctx->prof_bytes += gemm_bytes(g);
    // which kernel vv_gemm_launch picks (gemm.hip): MFMA tile GEMM, decode GEMV, or the general kernel
    const bool is_gemv = vv_gemm_route(&g, ctx->c.xsplit) == VV_ROUTE_GEMV;
    ctx->prof_rec.push_back({g.T, g.N, g.K, g.pro, g.epi, g.W2 ? 1 : 0, gemm_bytes(g), is_gemv});
    if (is_gemv) { ctx->prof_gemv.push_back(g); ctx->prof_gemv_bytes += gemm_bytes(g); }
    return r;
}
#ifdef VV_GEMM_TIMING
constexpr int TL_MAX = 4096, TL_STRIDE = 16 + 2 * 3200;
int gemm_tl(vv_ctx* ctx, VVGemm g, hipStream_t st) {
    if (!ctx->tl_base && getenv("VVHIP_TIMELINE")) {
        if (hipMalloc(&ctx->tl_base, (size_t)TL_MAX * TL_STRIDE * 8) != hipSuccess) return -9;
        hipMemset(ctx->tl_base, 0, (size_t)TL_MAX * TL_STRIDE * 8);
    }
    const bool gv = vv_gemm_route(&g, ctx->c.xsplit) == VV_ROUTE_GEMV;
    const bool want = gv ? ((g.T <= 4 || g.T != 16 || g.N > 16384) && (g.N + 15) / 16 <= 3200) : (g.T > 16);
    if (ctx->tl_base && ctx->tl_idx < TL_MAX && want) {
        g.dbg = ctx->tl_base + (size_t)ctx->tl_idx * TL_STRIDE;
        ctx->tl_rec.push_back({g.T, g.N, g.K, g.pro, gv ? g.epi : g.epi + 100});
        ctx->tl_idx++;
    }
    return vv_gemm_launch(g, ctx->c.xsplit, st);
}
extern "C" int vv_timeline_dump(vv_ctx* ctx, unsigned long long* out_host, int* meta_host, int max_launches) {
    VV_SHARED;                   // a device-wide synchronize: never while another context's capture is open
    hipDeviceSynchronize();
    const int n = std::min(max_launches, ctx->tl_idx);
    if (n > 0) hipMemcpy(out_host, ctx->tl_base, (size_t)n * TL_STRIDE * 8, hipMemcpyDeviceToHost);
    for (int i = 0; i < n; ++i) { const auto& r = ctx->tl_rec[i]; int* m = meta_host + 5 * i; m[0] = r.T; m[1] = r.N; m[2] = r.K; m[3] = r.pro; m[4] = r.epi; }
    return n;
}
#endif

extern "C" int vv_gemm_raw(void* stream, const void* w, const void* w2, const float* x, float* y, int T, int N, int K,
                           int ldx, int ldy, int pro, int epi, const float* nw, float eps, const float* bias,
                           const float* nscale, int xsplit, int ksplit, int nontemporal) {
    VVGemm g = mk_gemm(w, x, y, T, N, K, ldx, ldy);
    g.W2 = (const u32x4*)w2; g.pro = pro; g.epi = epi; g.nw = nw; g.eps = eps; g.bias = bias; g.nscale = nscale;
    g.ksplit = ksplit & 0xff; g.nt = 1;
    g.dbg = (unsigned long long*)(uintptr_t)0;
    if (nontemporal > 1) g.dbg = reinterpret_cast<unsigned long long*>(const_cast<float*>(nscale));   // timing builds: nscale slot carries the stamp buffer
    if (g.dbg) g.nscale = nullptr;
    return vv_gemm_launch(g, xsplit, (hipStream_t)stream);
}
static VVGemm case_gemm(const vv_gemv_case_args* c) {
    VVGemm g = mk_gemm(c->W, c->X, c->Y, c->T, c->N, c->K, c->ldx, c->ldy);
    g.W2 = (const u32x4*)c->W2; g.pro = c->pro; g.epi = c->epi; g.nw = c->nw; g.eps = c->eps; g.bias = c->bias; g.nscale = c->nscale;
    g.mod_scale = c->mod_scale; g.mod_shift = c->mod_shift; g.ld_mod = c->ld_mod;
    g.addvec = c->addvec; g.x_row_mod = c->x_row_mod; g.add_rows_per_vec = c->add_rows_per_vec;
    g.gate = c->gate; g.ld_gate = c->ld_gate;
    g.z = c->z; g.x0p = c->x0p; g.coef = c->coef; g.cfg = c->cfg; g.n_cfg = c->n_cfg; g.sde_noise = c->sde_noise;
    g.cfg_rows = c->cfg_rows;
    g.kgrid = c->kgrid; g.yparts = c->yparts; g.xa = c->xa; g.n_xa = c->n_xa; g.ya = c->ya; g.n_ya = c->n_ya; g.part_stride = c->part_stride;
    g.sl_n = c->sl_n; g.sl_T = c->sl_T; g.sl_x = c->sl_x; g.sl_y = c->sl_y;
    for (int j = 0; j < 8; ++j) g.sl_id[j] = c->sl_id[j];
    g.dw_hist = c->dw_hist; g.dw_w = c->dw_w; g.dw_b = c->dw_b; g.dw_gamma = c->dw_gamma; g.dw_nw = c->dw_nw;
    g.dw_xout = c->dw_xout; g.dw_hnew = c->dw_hnew;
    g.nt = 1;
    return g;
}
// tests: one launch of the decode GEMV kernel in the form its own launcher picks, or a refusal; no dispatcher, no stand-in kernel
extern "C" int vv_gemv_case(void* stream, const vv_gemv_case_args* c, int xsplit, int* form_out) {
    if (!c || xsplit < 1 || xsplit > 3) return -1;
    VVGemm g = case_gemm(c);
    if (!vv_gemv_ok(&g)) return VV_GEMV_REFUSED;
    int form[5] = {0, 0, 0, 0, 0};
    const int r = vv_gemv_launch(g, xsplit, (hipStream_t)stream, form);
    if (r == VV_RC_NO_FORM) return VV_GEMV_REFUSED;
    if (r == 0 && form_out) for (int j = 0; j < 5; ++j) form_out[j] = form[j];
    return r;
}
// tests: W13 twins one matrix at a time, and one launch of a named W13 form over the twins or over the bf16 fragments
extern "C" int64_t vv_w13_twin_bytes(int N, int K) { return vv_w13_shape_ok(N, K) ? vv_w13_bytes(N, K) : 0; }
extern "C" int vv_w13_pack_matrix(void* stream, const void* packed_dev, void* twin_dev, int N, int K) {
    return vv_w13_pack_launch(packed_dev, twin_dev, N, K, (hipStream_t)stream);
}
extern "C" int vv_w13_unpack_matrix(void* stream, const void* twin_dev, void* packed_dev, int N, int K) {
    return vv_w13_unpack_launch(twin_dev, packed_dev, N, K, (hipStream_t)stream);
}
extern "C" int vv_w13_gemv_case(void* stream, const vv_gemv_case_args* c, const void* twin_dev, const void* twin2_dev, int mr, int wpb) {
    if (!c) return -1;
    VVGemm g = case_gemm(c);
    g.w13 = twin_dev; g.w13_2 = twin2_dev;
    const int r = vv_gemv_w13_form_launch(g, mr, wpb, (hipStream_t)stream);
    return r == VV_RC_NO_FORM ? VV_GEMV_REFUSED : r;
}
// tests: one launch of the batch-decode packed GEMV (gemv16p.hip) through its own launcher, or a refusal; and its two activation packers
extern "C" int vv_gemv16p_case(void* stream, const vv_gemv16p_case_args* c, int epi, int flags, int* wpb_out) {
    if (!c) return -1;
    VVGemv16p a{};
    a.W = (const u32x4*)c->W; a.W2 = (const u32x4*)c->W2; a.Xp = (const u32x4*)c->Xp; a.Y = c->Y; a.Yp = (unsigned char*)c->Yp;
    a.bias = c->bias; a.gate = c->gate;
    a.T = c->T; a.N = c->N; a.K = c->K; a.ldy = c->ldy; a.ld_gate = c->ld_gate;
    a.ssq_in = c->ssq_in; a.ssq_tiles = c->ssq_tiles; a.eps = c->eps;
    a.Xs = (const u32x4*)c->Xs;
    a.pk_nw = c->pk_nw; a.pk_sc = c->pk_sc; a.ld_pk = c->ld_pk; a.ssq_out = c->ssq_out;
    a.z = c->z; a.x0p = c->x0p; a.coef = c->coef; a.cfg = c->cfg; a.n_cfg = c->n_cfg; a.sde_noise = c->sde_noise;
    a.cfg_rows = c->cfg_rows;
    int wpb = 0;
    const int r = vv_gemv16p_launch2(&a, epi, flags, (hipStream_t)stream, &wpb);
    if (r == VV_RC_NO_FORM) return VV_GEMV_REFUSED;
    if (r == 0 && wpb_out) *wpb_out = wpb;
    return r;
}
extern "C" int vv_pack16_case(void* stream, const float* x_dev, int ldx, int mode, const float* nw_dev, float eps, const float* sc_dev,
                              const float* sh_dev, int ld_mod, void* xp_dev, int T, int K) {
    const int r = vv_pack16_launch(x_dev, ldx, mode, nw_dev, eps, sc_dev, sh_dev, ld_mod, xp_dev, T, K, (hipStream_t)stream);
    return r == -1 ? VV_GEMV_REFUSED : r;
}
extern "C" int vv_pack16_tiles_case(void* stream, const float* x_dev, int ldx, int64_t stride_outer, int n_inner, int64_t stride_inner,
                                    void* xp_dev, int64_t tile_bytes, int T, int K, int n_tiles) {
    const int r = vv_pack16_tiles_launch(x_dev, ldx, stride_outer, n_inner, stride_inner, xp_dev, tile_bytes, T, K, n_tiles, (hipStream_t)stream);
    return r == -1 ? VV_GEMV_REFUSED : r;
}
// tests: Y = f(X) . W^T through the prefill GEMM (prefill.hip): X fp32 [T][K] is packed (optionally RMS-normalised) into xp_scratch,
// epi STORE/BIAS/RESID write fp32 Y [T][N]; epi SWIGLU (W = gate, W2 = up) writes packed bf16 into yp_scratch, unpacked to Y.
extern "C" int vv_gemm3_raw(vv_ctx* ctx, void* stream, const void* w, const void* w2, const float* x_dev, int T, int N, int K, int epi,
                            const float* nw_dev, float eps, const float* bias_dev, float* y_dev, void* xp_scratch, void* yp_scratch) {
    hipStream_t st = (hipStream_t)stream;
    if (ctx && ksplit_check(ctx, st)) return -1;
    int r = vv_pack_rows_launch(x_dev, K, nw_dev, eps, xp_scratch, T, K, st);
    if (r) return r;
    r = vv_gemm3_launch(w, w2, xp_scratch, y_dev, yp_scratch, bias_dev, T, N, K, N, epi, ctx ? &ctx->gws : nullptr, st);
    if (r) return r;
    if (epi == VV_EPI_SWIGLU) r = vv_unpack_rows_launch(yp_scratch, y_dev, T, N, st);
    return r;
}
extern "C" int vv_profile_begin(vv_ctx* ctx) {
    { VV_SHARED; HIPCHK(ctx, hipDeviceSynchronize()); }     // device-wide: excluded from other contexts' open captures by the lock
    ctx->prof_on = true; ctx->prof_n = 0; ctx->prof_bytes = 0.0; ctx->prof_rec.clear();
    ctx->prof_gemv.clear(); ctx->prof_gemv_bytes = 0.0; ctx->prof_other.clear();
    return 0;
}
extern "C" int vv_profile_end(vv_ctx* ctx, int64_t* launches, double* total_ms, double* bytes) {
    { VV_SHARED; HIPCHK(ctx, hipDeviceSynchronize()); }
    double ms = 0.0, raw_ms = 0.0;
    int64_t n_other = 0; double ms_other = 0.0, by_other = 0.0;
    // The fixed cost of an event pair with nothing in between, measured in the regime the samples were taken in: pairs
    // enqueued back to back on the SAME stream behind a real kernel (an idle-stream, synchronised-per-pair calibration reads
    // ~2x higher and over-corrects).  Subtracted from every sample.
    double ev_over = 0.0;
    {
        const int reps = 64;
        std::vector<hipEvent_t> ev(2 * reps);
        for (auto& e : ev) hipEventCreate(&e);
        hipStream_t ps = ctx->prof_stream;
        if (ctx->tmp1) vv_silu_launch(ctx->tmp1, 64, ps);            // something for the first pair to queue behind
        for (int i = 0; i < reps; ++i) { hipEventRecord(ev[2 * i], ps); hipEventRecord(ev[2 * i + 1], ps); }
        hipStreamSynchronize(ps);
        std::vector<float> d(reps);
        for (int i = 0; i < reps; ++i) { d[i] = 0.f; hipEventElapsedTime(&d[i], ev[2 * i], ev[2 * i + 1]); }
        std::sort(d.begin(), d.end());
        ev_over = d[reps / 2];                                        // median
        for (auto& e : ev) hipEventDestroy(e);
    }
    const char* csv = getenv("VVHIP_PROF_CSV");
    FILE* f = csv ? fopen(csv, "w") : nullptr;
    if (f) fprintf(f, "idx,T,N,K,pro,epi,dual,bytes,us\n");
    for (int i = 0; i < ctx->prof_n; ++i) {
        float e = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&e, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
        if (ctx->prof_rec[i].gemv) raw_ms += e;          // event-to-event time as recorded (what rocprofv3's per-kernel duration matches)
        e = (float)std::max(0.0, (double)e - ev_over);
        if (ctx->prof_rec[i].gemv) ms += e;
        else { n_other++; ms_other += e; by_other += ctx->prof_rec[i].bytes; }
        if (f) { const auto& r = ctx->prof_rec[i]; fprintf(f, "%d,%d,%d,%d,%d,%d,%d,%.0f,%.3f\n", i, r.T, r.N, r.K, r.pro, r.epi, r.dual, r.bytes, e * 1e3); }
    }
    if (f) fclose(f);
    // [0] = the dominant kernel (vv_gemv_kernel, decode rows), [1] = the general kernel (T > 4 / unaligned)
    if (launches) { launches[0] = ctx->prof_n - n_other; launches[1] = n_other; }
    if (total_ms) { total_ms[0] = ms; total_ms[1] = ms_other; }
    if (bytes) { bytes[0] = ctx->prof_bytes - by_other; bytes[1] = by_other; }
    ctx->prof_raw_ns = (int64_t)(raw_ms * 1e6); ctx->prof_ev_over_ns = (int64_t)(ev_over * 1e6);
    ctx->prof_on = false;
    return 0;
}
// Launch duration of the dominant kernel in the execution mode of the timed region: the vv_gemv_kernel launches recorded by
// the last profile window are captured, in issue order, into ONE hipGraph (a dependent chain on `stream`, as inside the step
// graphs) and replayed `reps` times between two events.  total_ms / (launches * reps) = start-to-start period of a GEMV
// launch in a dependent chain = kernel time + the kernel boundary, which is what rocprofv3 --kernel-trace reports per kernel
// under graph replay (profiles/): an upper bound on the kernel's own duration.  The replay re-runs residual epilogues on the
// engine's scratch / codec state buffers: call it after the measurements that need those states.
extern "C" int vv_profile_replay_family(vv_ctx* ctx, void* stream, int family, int reps, int64_t* launches, double* total_ms, double* bytes) {
    hipStream_t st = (hipStream_t)stream;
    if (ctx->prof_on) return fail(ctx, "vv_profile_replay: call vv_profile_end first");
    int64_t n = 0; double by = 0.0;
    if (family == 0) { n = (int64_t)ctx->prof_gemv.size(); by = ctx->prof_gemv_bytes; }
    else for (const auto& l : ctx->prof_other) if (l.family == family) { ++n; by += l.bytes; }
    if (launches) *launches = 0;
    if (total_ms) *total_ms = 0.0;
    if (bytes) *bytes = 0.0;
    if (n == 0) return family == 0 ? fail(ctx, "vv_profile_replay: the last profile window recorded no GEMV launches") : 0;
    if (reps < 1) reps = 1;
    HIPCHK(ctx, hipStreamSynchronize(st));
    hipGraph_t graph; hipGraphExec_t exec;
    HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    int rr = 0;
    if (family == 0) { for (const VVGemm& g : ctx->prof_gemv) { rr = vv_gemm_launch(g, ctx->c.xsplit, st); if (rr) break; } }
    else for (const auto& l : ctx->prof_other) if (l.family == family) { rr = l.fn(st); if (rr) break; }
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (rr) return fail(ctx, "vv_profile_replay: launch failed (%d)", rr);
    HIPCHK(ctx, e);
    HIPCHK(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    hipGraphDestroy(graph);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    HIPCHK(ctx, hipGraphLaunch(exec, st));                  // warm-up replay
    HIPCHK(ctx, hipEventRecord(e0, st));
    for (int i = 0; i < reps; ++i) HIPCHK(ctx, hipGraphLaunch(exec, st));
    HIPCHK(ctx, hipEventRecord(e1, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipGraphExecDestroy(exec);
    if (launches) *launches = n * reps;
    if (total_ms) *total_ms = ms;
    if (bytes) *bytes = by * reps;
    return 0;
}
extern "C" int vv_profile_replay(vv_ctx* ctx, void* stream, int reps, int64_t* launches, double* total_ms, double* bytes) {
    return vv_profile_replay_family(ctx, stream, 0, reps, launches, total_ms, bytes);
}
