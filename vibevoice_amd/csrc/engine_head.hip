// engine_head.hip -- host side of libvvhip.so: the diffusion head: schedule tables, one head evaluation, the sampler.
#include "engine_ctx.h"
#include "pass_plan.h"
#include "vv_w13.h"

// width 5 / 6: the shipped tables;  8: a general table, stochastic as the caller says.  All of them are rows of ctx->coef, 8 floats each
static int set_schedule(vv_ctx* ctx, int n_steps, const float* t, const float* coef, int width, void* stream, bool stochastic = false) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (n_steps < 1 || n_steps > 64) return fail(ctx, "n_steps must be in [1,64]");
    const int H = ctx->H;
    if (!ctx->temb) {
        ctx->temb = (float*)dalloc(ctx, (size_t)64 * H * 4);
        ctx->coef = (float*)dalloc(ctx, 64 * 8 * 4);
        ctx->tvals = (float*)dalloc(ctx, 64 * 4);
    }
    const bool general = width == 8;
    if (general && !ctx->hg[0].m2) {
        for (HeadGen& g : ctx->hg) g.m2 = (float*)dalloc(ctx, (size_t)8 * ctx->c.latent_dim * 4);
        if (!ctx->hg[0].m2 || !ctx->hg[1].m2) return fail(ctx, "vv_set_schedule_general: out of device memory");
    }
    float rows[64 * 8] = {};                      // a shipped row's 5 or 6 values, zeros after them; a general row as given
    for (int i = 0; i < n_steps; ++i)
        for (int j = 0; j < width; ++j) rows[i * 8 + j] = coef[i * width + j];
    // by the API used, not by the values: a one-step stochastic schedule has sigma_t = 0 on its only step (all noise scales
    // zero) and must still be sampled through vv_diffusion_sample_sde, as the reference runs it (a noise-free first-order step)
    ctx->sde_on = general ? stochastic : (width == 6);
    ctx->general_on = general;
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipMemcpy(ctx->coef, rows, (size_t)n_steps * 8 * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->tvals, t, (size_t)n_steps * 4, hipMemcpyHostToDevice));
    // t_emb[i] = W2 . silu(W1 . sinusoid(t_i))   (TimestepEmbedder, modular_vibevoice_diffusion_head.py:66-93)
    VVCHK(vv_tfreq_launch(ctx->tvals, ctx->tmp2, n_steps, st));
    for (int i0 = 0; i0 < n_steps; i0 += 16) {
        const int nn = std::min(16, n_steps - i0);
        VVGemm g = mk_gemm(ctx->h_t0, ctx->tmp2 + (size_t)i0 * 256, ctx->tmp1 + (size_t)i0 * H, nn, H, 256, 256, H);
        GEMM(g);
    }
    VVCHK(vv_silu_launch(ctx->tmp1, n_steps * H, st));
    for (int i0 = 0; i0 < n_steps; i0 += 16) {
        const int nn = std::min(16, n_steps - i0);
        VVGemm g = mk_gemm(ctx->h_t2, ctx->tmp1 + (size_t)i0 * H, ctx->temb + (size_t)i0 * H, nn, H, H, H, H);
        GEMM(g);
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->n_steps = n_steps;
    {   // room for the batched adaLN modulations of up to 8 sampled utterances (16 rows) per step
        const size_t need = (size_t)n_steps * 16 * ctx->MODW * 4;
        if (need > ctx->mod_all_bytes) {
            dfree(ctx, ctx->mod_all);
            dfree(ctx, ctx->ada_in);
            ctx->mod_all = (float*)dalloc(ctx, need, false);
            ctx->ada_in = (float*)dalloc(ctx, (size_t)n_steps * 16 * ctx->H * 4, false);
            dfree(ctx, ctx->ada_p);
            ctx->ada_p = (ctx->c.xsplit == 1 && (ctx->H & 7) == 0) ? dalloc(ctx, (size_t)vv_packed_elems(n_steps * 16, ctx->H) * 2, false) : nullptr;
            ctx->mod_all_bytes = (ctx->mod_all && ctx->ada_in) ? need : 0;
            dfree(ctx, ctx->p16_shift); ctx->p16_shift = nullptr;
            if (ctx->p16_ok) {            // the adaLN shift rows of every (solver step, layer) as packed bf16 operand tiles
                ctx->p16_shift_tile = (size_t)vv_packed_elems(16, ctx->H) * 2;
                ctx->p16_shift = dalloc(ctx, (size_t)n_steps * (ctx->c.head_layers + 1) * ctx->p16_shift_tile);
            }
        }
    }
    // every sampler key family: a captured sample_body holds the step count, the table offsets and the buffers reallocated above
    return drop_graphs(ctx, {"samp:", "sde:", "rows:", "gen:"});
}
// coef: n_steps rows {a, s, cs, c0, c1} (the deterministic DPM-Solver++(2M) the model classes build)
extern "C" int vv_set_schedule(vv_ctx* ctx, int n_steps, const float* t, const float* coef, void* stream) {
    return set_schedule(ctx, n_steps, t, coef, 5, stream);
}
// coef: n_steps rows {a, s, cs, c0, c1, cn} -- sde-dpmsolver++ (demo/gradio_demo.py:142-146); sampling then needs the per-step
// variance noise: vv_diffusion_sample_sde
extern "C" int vv_set_schedule_sde(vv_ctx* ctx, int n_steps, const float* t, const float* coef6, void* stream) {
    return set_schedule(ctx, n_steps, t, coef6, 6, stream);
}

// coef: n_steps rows {a, s, cs, c0, c1, c2, cn, 0} (vibevoice_amd/schedule.py: make_general_table); sampled by vv_diffusion_sample_general
extern "C" int vv_set_schedule_general(vv_ctx* ctx, int n_steps, const float* t, const float* coef, int stochastic, void* stream) {
    return set_schedule(ctx, n_steps, t, coef, 8, stream, stochastic != 0);
}

// has_coef: a sampler's plan, which ends its steps as the installed table says (general_on: solver.hip's launch)
static VVHeadPlan head_plan(const vv_ctx* ctx, int rows, int n_steps, bool has_coef) {
    return vv_head_plan(rows, n_steps, ctx->HF, ctx->c.head_layers, ctx->MODW,
                        {ctx->p16_ok, ctx->p16_shift != nullptr, ctx->ada_p != nullptr, ctx->mod_all_bytes != 0, ctx->head_tail, ctx->w13_on}, has_coef,
                        has_coef && ctx->general_on);
}

// How a shipped sampler's step ends inside the head (an epilogue of the final layer, or the seam): the step's row of ctx->coef, the
// guidance scale or cfg_rows [rows / 2], one per utterance on the device and read in its place, the step's variance noise or null
struct StepEnd { const float* coef; float cfg; const float *cfg_rows, *noise; };
// One head evaluation: solver step `step` of the plan, on the plan's rows
struct HeadStep {
    int step;
    const float *z, *temb, *mod;        // the rows the in-projection reads, the t-embedding row, the modulation rows (null: evaluated here)
    const unsigned char* sh_tiles;      // the step's packed shift tiles (VV_FINAL_P16_CFG), else null
    float* eps_out;                     // where the GEMM dispatcher's final layer stores
    const HeadGen &cur, &nxt;           // the generation the step reads (xh: its in-projection) and the one a seam writes
    bool have_x;                        // the previous step's end left this step's in-projection in cur.xh
    const StepEnd* end;                 // null: a plain final layer (vv_head_forward; a general table, whose step end is solver.hip's launch)
};

// mod / hact are ctx scratch.  < 0: failure;  1: the step ended with the seam (final layer + CFG + solver update + the NEXT step's
// in-projection, all written to s.nxt);  0: otherwise
static int head_eval(vv_ctx* ctx, hipStream_t st, const VVHeadPlan& p, const HeadStep& s) {
    const vv_config& c = ctx->c;
    const int rows = p.rows, final_stage = vv_head_final(p, s.step);
    const int H = ctx->H, L = c.latent_dim, HL = c.head_layers, HF = ctx->HF, MODW = ctx->MODW;
    const float* mod = s.mod ? s.mod : ctx->mod;
    const StepEnd end = s.end ? *s.end : StepEnd{};
    auto put_end = [&](auto& a) { a.coef = end.coef; a.cfg = end.cfg; a.n_cfg = rows / 2; a.sde_noise = end.noise; a.cfg_rows = end.cfg_rows; };
    float* const xh = s.cur.xh;
    if (!s.mod) {
        VVGemm ga = mk_gemm(ctx->h_ada, ctx->cproj, ctx->mod, rows, MODW, H, H, MODW);
        ga.pro = VV_PRO_ADD_SILU; ga.addvec = s.temb; ga.nt = 1;
        GEMM(ga);
    }
    if (!s.have_x) {
        VVGemm gi = mk_gemm(ctx->h_in, s.z, xh, rows, H, L, L, H);
        GEMM(gi);
        nan_probe(ctx, st, "in-proj xh", xh, (size_t)rows * H);
    }
    int xp = 0;                                    // extra parts xh currently consists of
    const int xps = 16 * H;
    for (int l = 0; l < HL; ++l) {
        const float* base = mod + (size_t)l * 3 * H;
        if (p.layers == VV_HEAD_P16) {
            // batch rows: normalise + modulate + pack ONCE, then both projections stream weights against packed fragments
            ctx->launches += 3;
            VVCHK(vv_pack16_launch(xh, H, 2, ctx->hl[l].norm, c.head_eps, base + H, base, MODW, ctx->p16_x, rows, H, st));
            VVCHK(p16_gemv(ctx, st, ctx->hl[l].wg, ctx->hl[l].wu, ctx->p16_x, nullptr, ctx->p16_act, nullptr, nullptr, rows, HF, H, 0, 0, VV_EPI_SWIGLU));
            if (l + 1 == HL && final_stage == VV_FINAL_P16_CFG) {
                // the last layer's down projection leaves the FINAL layer's operand (x * (1 + scale), un-normalised) packed and the rows' sums of squares
                VVGemv16p ad = p16_args(ctx->hl[l].wd, nullptr, ctx->p16_act, xh, ctx->p16_x, rows, H, HF, H);
                ad.gate = base + 2 * H; ad.ld_gate = MODW; ad.ssq_out = ctx->ssq_a;
                ad.pk_nw = nullptr; ad.pk_sc = mod + (size_t)HL * 3 * H + H; ad.ld_pk = MODW;
                VVCHK(p16_go(ctx, st, ad, VV_EPI_GATED_RESID, 4));
            } else
            VVCHK(p16_gemv(ctx, st, ctx->hl[l].wd, nullptr, ctx->p16_act, xh, nullptr, nullptr, base + 2 * H, rows, H, HF, H, MODW, VV_EPI_GATED_RESID));
            continue;
        }
        VVGemm g1 = mk_gemm(ctx->hl[l].wg, xh, ctx->hact, rows, HF, H, H, HF);
        g1.W2 = (const u32x4*)ctx->hl[l].wu; g1.pro = VV_PRO_RMS_MOD; g1.nw = ctx->hl[l].norm; g1.eps = c.head_eps;
        g1.mod_shift = base; g1.mod_scale = base + H; g1.ld_mod = MODW; g1.epi = VV_EPI_SWIGLU; g1.nt = 1;
        float* cur = ctx->xh_parts + (size_t)(l & 1) * 2 * xps;          // parts written by layer l-1
        float* nxt = ctx->xh_parts + (size_t)((l + 1) & 1) * 2 * xps;    // parts layer l writes
        g1.xa = cur; g1.n_xa = xp; g1.part_stride = xps;
        // a launch without a W13 form (part tensors) keeps its bf16 launch; a tile row its twin cannot hold streams bf16 inside the W13 one
        const int tg = ctx->w[ctx->hl[l].ig].twin, tu = ctx->w[ctx->hl[l].iu].twin, td = ctx->w[ctx->hl[l].id].twin;
        if (p.w13 && tg >= 0 && tu >= 0 && vv_gemv_w13_form(&g1, c.xsplit) >= 0) {
            g1.w13 = ctx->twins[tg].planes; g1.w13_2 = ctx->twins[tu].planes;
            g1.w13_exact = ctx->twins[tg].exact == 1 && ctx->twins[tu].exact == 1;
        }
        GEMM(g1);
        VVGemm g2 = mk_gemm(ctx->hl[l].wd, ctx->hact, xh, rows, H, HF, HF, H);
        g2.epi = VV_EPI_GATED_RESID; g2.gate = base + 2 * H; g2.ld_gate = MODW; g2.nt = 1;
        g2.ya = cur; g2.n_ya = xp; g2.part_stride = xps;
        xp = ksplit_parts(ctx, g2, nxt, xps);
        if (p.w13 && td >= 0 && vv_gemv_w13_form(&g2, c.xsplit) >= 0) { g2.w13 = ctx->twins[td].planes; g2.w13_exact = ctx->twins[td].exact == 1; }
        if (ctx->probe_on) { char nm[64]; snprintf(nm, 64, "layer %d hact (parts in %d)", l, g1.n_xa); nan_probe(ctx, st, nm, ctx->hact, (size_t)rows * HF); }
        GEMM(g2);
        if (ctx->probe_on) {
            char nm[64]; snprintf(nm, 64, "layer %d xh", l); nan_probe(ctx, st, nm, xh, (size_t)rows * H);
            for (int q = 0; q < xp; ++q) { snprintf(nm, 64, "layer %d part %d", l, q); nan_probe(ctx, st, nm, nxt + (size_t)q * xps, (size_t)rows * H); }
        }
    }
    const float* fb = mod + (size_t)HL * 3 * H;
    if (final_stage == VV_FINAL_P16_CFG) {
        // the sampler's final layer over the packed operand the last down projection left (4 workgroups that only stream: the 16-row
        // vv_gemv form staged 16 x H modulated rows in each of its 4 workgroups, 21 us), CFG + DPM-Solver++ update in the epilogue
        ctx->launches += 1;
        VVGemv16p af = p16_args(ctx->h_out, nullptr, ctx->p16_x, nullptr, nullptr, rows, L, H, L);
        af.ssq_in = ctx->ssq_a; af.ssq_tiles = H / 16; af.eps = c.head_eps;
        af.Xs = (const u32x4*)(s.sh_tiles + (size_t)HL * ctx->p16_shift_tile);
        af.z = s.cur.zz; af.x0p = s.cur.x0p; put_end(af);
        VVCHK(p16_go(ctx, st, af, VV_EPI_CFG_DPM, 3));
        return 0;
    }
    if (final_stage == VV_FINAL_SEAM) {
        VVTail t{};
        t.Wout = (const u32x4*)ctx->h_out; t.Win = (const u32x4*)ctx->h_in; t.bin = nullptr;
        t.X = xh; t.xa = ctx->xh_parts + (size_t)(HL & 1) * 2 * xps; t.n_xa = xp; t.part_stride = xps;
        t.sc = fb + H; t.sh = fb; t.ld_mod = MODW;
        t.Xout = s.nxt.xh;
        t.z_in = s.cur.zz; t.x0p_in = s.cur.x0p; t.z_out = s.nxt.zz; t.x0p_out = s.nxt.x0p; put_end(t);
        t.T = rows; t.H = H; t.L = L; t.eps = c.head_eps;
        if (vv_head_tail_ok(&t)) {
            ctx->launches++;
            ctx->seam_launches++;
            if (ctx->prof_on) {
                const VVTail tc = t;
                ctx->prof_other.push_back({3, (double)vv_packed_elems(L, H) * 2.0 + (double)vv_packed_elems(H, L) * 2.0 + (double)rows * H * 8.0,
                                           [=](hipStream_t s2) { return vv_head_tail_launch(&tc, s2); }});
            }
            VVCHK(vv_head_tail_launch(&t, st));
            return 1;          // the next step's in-projection is done (in s.nxt)
        }
    }
    VVGemm gf = mk_gemm(ctx->h_out, xh, s.eps_out, rows, L, H, H, L);
    gf.pro = VV_PRO_RMS_MOD; gf.nw = nullptr; gf.eps = c.head_eps; gf.mod_shift = fb; gf.mod_scale = fb + H; gf.ld_mod = MODW;
    gf.xa = ctx->xh_parts + (size_t)(HL & 1) * 2 * xps; gf.n_xa = xp; gf.part_stride = xps;
    if (final_stage != VV_FINAL_GEMM) {   // CFG + DPM-Solver++ update fused into the epilogue: the noisy latent is rewritten in place
        gf.epi = VV_EPI_CFG_DPM; gf.z = s.cur.zz; gf.x0p = s.cur.x0p; put_end(gf);
    }
    GEMM(gf);
    return 0;
}

// what one sampler call asks for, whichever entry point it came through: step_noise / cfg_rows null where the call has none
struct SampleReq { int n; const float *cond, *noise, *step_noise; float cfg; const float* cfg_rows; float* out; };
// how a step ended.  rc < 0: failure;  1: the next step's in-projection is done;  0: otherwise.  flipped: its result is in the other generation
struct StepDone { int rc; bool flipped; };

// a shipped table: the step ends inside the head, in an epilogue of the final layer (the state is rewritten in place) or -- decode rows,
// bf16 mode, every step but the last -- in the fused seam (headtail.hip), which leaves the next step's state in the other generation
static StepDone step_shipped(vv_ctx* ctx, hipStream_t st, const VVHeadPlan& p, const SampleReq& r, HeadStep s) {
    const StepEnd end{ctx->coef + s.step * 8, r.cfg, r.cfg_rows,
                      r.step_noise ? r.step_noise + (size_t)s.step * r.n * ctx->c.latent_dim : nullptr};
    s.end = &end;
    const int hr = head_eval(ctx, st, p, s);
    return {hr, hr == 1};
}

// a general table: the head (plain final layer -> eps), then ONE launch: CFG + the table-driven update of s.cur into s.nxt and, on every
// step but the last, the next step's in-projection where solver.hip's rule holds (else the next head_eval does its own)
static StepDone step_general(vv_ctx* ctx, hipStream_t st, const VVHeadPlan& p, const SampleReq& r, const HeadStep& s) {
    const int L = ctx->c.latent_dim;
    if (head_eval(ctx, st, p, s) < 0) return {-1, false};
    VVSolverStep v{};
    v.eps = s.eps_out; v.coef = ctx->coef + s.step * 8; v.cfg = r.cfg; v.cfg_rows = r.cfg_rows; v.n = r.n; v.L = L;
    v.noise = r.step_noise ? r.step_noise + (size_t)s.step * r.n * L : nullptr;
    v.z_in = s.cur.zz; v.m1_in = s.cur.x0p; v.m2_in = s.cur.m2;
    v.z_out = s.nxt.zz; v.m1_out = s.nxt.x0p; v.m2_out = s.nxt.m2;
    if (s.step + 1 < p.n_steps && ctx->solver_fuse) { v.Win = (const u32x4*)ctx->h_in; v.Xout = s.nxt.xh; v.H = ctx->H; v.xs = ctx->c.xsplit; }
    ctx->launches++;
    const int sr = vv_solver_step_launch(&v, st);
    if (sr == VV_RC_NO_FORM) return {fail(ctx, "vv_diffusion_sample_general: solver.hip has no form for n = %d, latent_dim = %d", r.n, L), false};
    if (sr < 0) return {fail(ctx, "%s:%d launch failed (%d): hip error %d (%s)", __FILE__, __LINE__, sr, g_vv_launch_err, hipGetErrorString((hipError_t)g_vv_launch_err)), false};
    if (sr == 1) ctx->solver_fused++;
    return {sr == 1, true};
}

static int sample_body(vv_ctx* ctx, hipStream_t st, const SampleReq& r) {
    const int H = ctx->H, L = ctx->c.latent_dim, HL = ctx->c.head_layers;
    const int n = r.n, rows = 2 * n;
    ctx->seam_launches = ctx->solver_fused = 0;
    ctx->probe_names.clear();
    nan_probe(ctx, st, "cond (input)", r.cond, (size_t)rows * H);
    nan_probe(ctx, st, "noise (input)", r.noise, (size_t)n * L);
    // both CFG halves see the same noisy latent (modeling_vibevoice_inference.py:703-704)
    VVCHK(vv_sampler_init_launch(r.noise, ctx->hg[0].zz, ctx->hg[0].x0p, n * L, st));
    VVGemm gc = mk_gemm(ctx->h_cond, r.cond, ctx->cproj, rows, H, H, H, H);
    gc.nt = 1;
    GEMM(gc);
    // adaLN modulations depend on (cond, t) only, not on the evolving latent: evaluate them for ALL solver steps
    // up front, <=16 rows per GEMM, so the (3*layers+2)*H x H modulation matrix is streamed ceil(2nN/16) times per
    // frame instead of N times (the reference recomputes it inside every head call)
    const int MODW = ctx->MODW;
    const VVHeadPlan p = head_plan(ctx, rows, ctx->n_steps, true);
    const bool batch_ada = p.ada != VV_ADA_PER_STEP;
    if (batch_ada) {
        // SiLU(cond + t) for all (step, row) pairs in one small launch: the GEMM workgroups (one per 16 output features,
        // > 1000 of them) then stage plain rows instead of each re-evaluating 16 x H SiLUs
        const int total = rows * ctx->n_steps;
        if (p.ada == VV_ADA_TILE) {      // ONE MFMA tile GEMM over all (step, row) pairs instead
            ctx->launches += 2;
            VVCHK(vv_ada_pack_launch(ctx->cproj, ctx->temb, ctx->ada_p, rows, ctx->n_steps, H, st));
            VVCHK(vv_gemm3_launch(ctx->h_ada, nullptr, ctx->ada_p, ctx->mod_all, nullptr, nullptr, total, MODW, H, MODW, VV_EPI_STORE, nullptr, st));
        } else {
        VVCHK(vv_ada_in_launch(ctx->cproj, ctx->temb, ctx->ada_in, rows, ctx->n_steps, H, st));
        ctx->launches++;
        for (int t0 = 0; t0 < total; t0 += 16) {
            const int T = std::min(16, total - t0);
            VVGemm ga = mk_gemm(ctx->h_ada, ctx->ada_in + (size_t)t0 * H, ctx->mod_all + (size_t)t0 * MODW, T, MODW, H, H, MODW);
            GEMM(ga);
        }
        }
    }
    nan_probe(ctx, st, "cproj", ctx->cproj, (size_t)rows * H);
    if (batch_ada) nan_probe(ctx, st, "mod_all", ctx->mod_all, (size_t)rows * ctx->n_steps * MODW);
    if (p.sh_tiles) {
        // the shift rows of every (solver step, layer) -- and the final layer's -- as packed bf16 tiles, one launch per frame:
        // tile (i, l) = rows [i * rows, (i + 1) * rows) of mod_all, columns [l * 3H, l * 3H + H).  Only the final layer's tile (l == HL) is read
        ctx->launches++;
        VVCHK(vv_pack16_tiles_launch(ctx->mod_all, MODW, (int64_t)rows * MODW, HL + 1, (int64_t)3 * H, ctx->p16_shift,
                                     (int64_t)ctx->p16_shift_tile, rows, H, ctx->n_steps * (HL + 1), st));
    }
    int gen = 0; bool have_x = false;
    for (int i = 0; i < ctx->n_steps; ++i) {
        const HeadGen& cur = ctx->hg[gen];
        const HeadStep s{.step = i, .z = cur.zz, .temb = ctx->temb + (size_t)i * H,
                         .mod = batch_ada ? ctx->mod_all + (size_t)i * rows * MODW : nullptr,
                         .sh_tiles = p.sh_tiles ? (const unsigned char*)ctx->p16_shift + (size_t)i * (HL + 1) * ctx->p16_shift_tile : nullptr,
                         .eps_out = ctx->eps, .cur = cur, .nxt = ctx->hg[gen ^ 1], .have_x = have_x, .end = nullptr};
        const StepDone d = p.solver_step ? step_general(ctx, st, p, r, s) : step_shipped(ctx, st, p, r, s);
        if (d.rc < 0) return -1;
        have_x = d.rc == 1;
        gen ^= d.flipped;
        if (ctx->probe_on) {
            const HeadGen& now = ctx->hg[gen];      // where the step left its result
            char nm[64];
            snprintf(nm, 64, "step %d z%s", i, p.solver_step ? " (general)" : have_x ? " (seam, next gen)" : ""); nan_probe(ctx, st, nm, now.zz, (size_t)rows * L);
            if (!p.solver_step) { snprintf(nm, 64, "step %d x0p", i); nan_probe(ctx, st, nm, now.x0p, (size_t)n * L); }
            if (!p.solver_step && have_x) { snprintf(nm, 64, "step %d next xh", i); nan_probe(ctx, st, nm, now.xh, (size_t)rows * H); }
        }
    }
    VVCHK(vv_copy_launch(r.out, ctx->hg[gen].zz, (size_t)n * L * 4, st));
    return 0;
}

// In front of every head evaluation, outside any capture: the folded ok words of the head's twins that were written since the host last
// read them (an upload, a LoRA merge or reset; a new context).  One stream wait and one 4-byte copy per such twin, once per write, not
// per call.  An exact twin takes the launch without the fall-back; that is a kernel choice, so a changed answer drops the sampler's
// graph families.  The caller holds g_dev_mu shared.
static int head_w13_resolve(vv_ctx* ctx, hipStream_t st) {
    if (!ctx->w13_on) return 0;
    bool changed = false, waited = false;
    for (W13Twin& t : ctx->twins) {
        if (t.lm || t.exact >= 0) continue;
        if (!waited) { HIPCHK(ctx, hipStreamSynchronize(st)); waited = true; }
        unsigned ok = 0;
        HIPCHK(ctx, hipMemcpy(&ok, (const char*)t.planes + vv_w13_plane_bytes(t.N, t.K) + (size_t)2 * (t.N / 16) * 4, 4, hipMemcpyDeviceToHost));
        t.exact = ok == 1;
        if (t.used >= 0 && t.used != t.exact) changed = true;
        t.used = t.exact;
    }
    return changed ? drop_graphs(ctx, {"samp:", "sde:", "rows:", "gen:"}) : 0;
}

// The tail of every sampler entry point, behind its own checks and its key: eager, captured or replayed, then the NaN probe's report
static int run_sampler(vv_ctx* ctx, hipStream_t st, const char* key, const SampleReq& r) {
    ctx->launches = 0;
    { VV_SHARED; VVTRY(head_w13_resolve(ctx, st)); }
    const int rc = graphed(ctx, key, st, [&]() { return sample_body(ctx, st, r); });
    nan_probe_report(ctx, st, key);
    return rc;
}

extern "C" int vv_diffusion_sample(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev, float cfg_scale, float* latent_out_dev) {
    if (ctx->n_steps < 1) return fail(ctx, "vv_set_schedule has not been called");
    if (n < 1 || n > 8) return fail(ctx, "vv_diffusion_sample: n must be in [1,8]");
    if (ctx->general_on) return fail(ctx, "the installed table is a general one (vv_set_schedule_general): sample with vv_diffusion_sample_general");
    if (ctx->sde_on) return fail(ctx, "the schedule is stochastic (vv_set_schedule_sde): sample with vv_diffusion_sample_sde and its per-step noise");
    char key[128]; snprintf(key, 128, "samp:%d:%p:%p:%p:%a", n, (const void*)cond_dev, (const void*)noise_dev, (void*)latent_out_dev, cfg_scale);
    return run_sampler(ctx, (hipStream_t)stream, key, {n, cond_dev, noise_dev, nullptr, cfg_scale, nullptr, latent_out_dev});
}

// The stochastic solver: step_noise_dev = [n_steps][n][latent_dim] fp32, the variance noise scheduler.step() draws per solver step
// (dpm_solver.py:994-997; the reference draws [2n][latent] and only the first n rows reach the next step, :703-704).
extern "C" int vv_diffusion_sample_sde(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev,
                                       const float* step_noise_dev, float cfg_scale, float* latent_out_dev) {
    if (ctx->n_steps < 1) return fail(ctx, "vv_set_schedule_sde has not been called");
    if (n < 1 || n > 8) return fail(ctx, "vv_diffusion_sample_sde: n must be in [1,8]");
    if (ctx->general_on) return fail(ctx, "the installed table is a general one (vv_set_schedule_general): sample with vv_diffusion_sample_general");
    if (!ctx->sde_on) return fail(ctx, "the schedule is deterministic (vv_set_schedule): sample with vv_diffusion_sample");
    if (!step_noise_dev) return fail(ctx, "vv_diffusion_sample_sde: step_noise is null");
    char key[160]; snprintf(key, 160, "sde:%d:%p:%p:%p:%p:%a", n, (const void*)cond_dev, (const void*)noise_dev, (const void*)step_noise_dev,
                            (void*)latent_out_dev, cfg_scale);
    return run_sampler(ctx, (hipStream_t)stream, key, {n, cond_dev, noise_dev, step_noise_dev, cfg_scale, nullptr, latent_out_dev});
}

// Either sampler with one guidance scale per utterance, cfg_rows_dev [n] fp32.  The kernels read the values at run time: the graph key
// holds the POINTER, so rewriting the buffer between calls replays the same captured graph.
extern "C" int vv_diffusion_sample_rows(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev,
                                        const float* step_noise_dev, const float* cfg_rows_dev, float* latent_out_dev) {
    if (ctx->n_steps < 1) return fail(ctx, "vv_set_schedule / vv_set_schedule_sde has not been called");
    if (n < 1 || n > 8) return fail(ctx, "vv_diffusion_sample_rows: n must be in [1,8]");
    if (ctx->general_on) return fail(ctx, "the installed table is a general one (vv_set_schedule_general): sample with vv_diffusion_sample_general");
    if (!cfg_rows_dev) return fail(ctx, "vv_diffusion_sample_rows: cfg_rows is null");
    if (ctx->sde_on && !step_noise_dev) return fail(ctx, "the schedule is stochastic (vv_set_schedule_sde): vv_diffusion_sample_rows needs its per-step noise");
    if (!ctx->sde_on && step_noise_dev) return fail(ctx, "the schedule is deterministic (vv_set_schedule): vv_diffusion_sample_rows takes no step noise");
    char key[192]; snprintf(key, 192, "rows:%d:%p:%p:%p:%p:%p", n, (const void*)cond_dev, (const void*)noise_dev, (const void*)step_noise_dev,
                            (const void*)cfg_rows_dev, (void*)latent_out_dev);
    return run_sampler(ctx, (hipStream_t)stream, key, {n, cond_dev, noise_dev, step_noise_dev, 0.f, cfg_rows_dev, latent_out_dev});
}

// The sampler under a general table (vv_set_schedule_general): one guidance scale, or cfg_rows_dev [n] read at run time (the key
// holds the POINTER); step_noise_dev as the table's kind demands.  Its own graph family, dropped by every vv_set_schedule* call.
extern "C" int vv_diffusion_sample_general(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev,
                                           const float* step_noise_dev, float cfg_scale, const float* cfg_rows_dev, float* latent_out_dev) {
    if (ctx->n_steps < 1) return fail(ctx, "vv_set_schedule_general has not been called");
    if (n < 1 || n > 8) return fail(ctx, "vv_diffusion_sample_general: n must be in [1,8]");
    if (!ctx->general_on) return fail(ctx, "the installed table is a shipped one (vv_set_schedule / vv_set_schedule_sde): sample with vv_diffusion_sample, _sde or _rows");
    if (ctx->sde_on && !step_noise_dev) return fail(ctx, "the general table is stochastic: vv_diffusion_sample_general needs its per-step noise");
    if (!ctx->sde_on && step_noise_dev) return fail(ctx, "the general table is deterministic: vv_diffusion_sample_general takes no step noise");
    char key[224]; snprintf(key, 224, "gen:%d:%p:%p:%p:%p:%p:%a", n, (const void*)cond_dev, (const void*)noise_dev, (const void*)step_noise_dev,
                            (const void*)cfg_rows_dev, (void*)latent_out_dev, cfg_rows_dev ? 0.f : cfg_scale);
    return run_sampler(ctx, (hipStream_t)stream, key, {n, cond_dev, noise_dev, step_noise_dev, cfg_scale, cfg_rows_dev, latent_out_dev});
}

extern "C" int vv_head_forward(vv_ctx* ctx, void* stream, int n, const float* noisy_dev, const float* t_host, const float* cond_dev, float* out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || n > 16) return fail(ctx, "vv_head_forward: n must be in [1,16]");
    const int H = ctx->H;
    for (int i = 1; i < n; ++i) if (t_host[i] != t_host[0]) return fail(ctx, "vv_head_forward: all rows must share one timestep");
    VVTRY(head_w13_resolve(ctx, st));
    float* tdev = ctx->tmp2 + 63 * 256;     // scratch
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipMemcpy(tdev + 128, t_host, 4, hipMemcpyHostToDevice));
    VVCHK(vv_tfreq_launch(tdev + 128, ctx->tmp2, 1, st));
    VVGemm g = mk_gemm(ctx->h_t0, ctx->tmp2, ctx->tmp1, 1, H, 256, 256, H); GEMM(g);
    VVCHK(vv_silu_launch(ctx->tmp1, H, st));
    VVGemm g2 = mk_gemm(ctx->h_t2, ctx->tmp1, ctx->tmp1 + H, 1, H, H, H, H); GEMM(g2);
    VVGemm gc = mk_gemm(ctx->h_cond, cond_dev, ctx->cproj, n, H, H, H, H); GEMM(gc);
    const HeadStep s{.step = 0, .z = noisy_dev, .temb = ctx->tmp1 + H, .mod = nullptr, .sh_tiles = nullptr, .eps_out = out_dev,
                     .cur = ctx->hg[0], .nxt = ctx->hg[1], .have_x = false, .end = nullptr};
    if (head_eval(ctx, st, head_plan(ctx, n, 1, false), s)) return -1;
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
