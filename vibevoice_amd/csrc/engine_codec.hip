// engine_codec.hip -- host side of libvvhip.so: the streaming tokenizer (codec) nets: build, history tables, the stage walker, API.
#include "engine_ctx.h"

// the two conv shapes with a kernel of their own instead of a GEMM (misc.hip)
static bool is_stem(const ConvG& g) { return g.K == 7 && g.ldx == 1; }       // encoder stem: mono input, k = 7 (only a net's first conv can have this shape)
static bool is_conv1_head(const ConvG& g) { return g.N == 1 && g.K == 7 * g.ldx && (g.ldx & 3) == 0 && g.ldx <= 1024; }     // decoder head: k = 7 conv to one channel

// Registers a net's weights and allocates its per-slot state.  The walloc / add_mat / add_vec calls keep their order: a shared child
// replays the parent's allocation sequence and the parameter tables are compared index by index (create_impl).
int build_codec(vv_ctx* ctx, CodecNet& net, const std::string& pfx, bool decoder, int vae_dim, int Fmax, int n_slots) {
    const vv_config& c = ctx->c;
    const int ns = c.n_stages;
    const int nf = c.n_filters;
    net.decoder = decoder; net.Fmax = Fmax;
    std::vector<int> depths(ns), ratios(c.n_ratios);
    if (decoder) { for (int i = 0; i < ns; ++i) depths[i] = c.enc_depths[ns - 1 - i]; for (int i = 0; i < c.n_ratios; ++i) ratios[i] = c.ratios[i]; }
    else { for (int i = 0; i < ns; ++i) depths[i] = c.enc_depths[i]; for (int i = 0; i < c.n_ratios; ++i) ratios[i] = c.ratios[c.n_ratios - 1 - i]; }
    int hop = 1; for (int i = 0; i < c.n_ratios; ++i) hop *= c.ratios[i];
    ctx->hop = hop;
    // per-stage geometry
    std::vector<int> C(ns), Tpf(ns);
    for (int i = 0; i < ns; ++i) {
        if (decoder) { C[i] = nf << (ns - 1 - i); Tpf[i] = (i == 0) ? 1 : Tpf[i - 1] * ratios[i - 1]; }
        else { C[i] = nf << i; Tpf[i] = (i == 0) ? hop : Tpf[i - 1] / ratios[i - 1]; }
    }
    net.in_dim = decoder ? vae_dim : 1;
    net.out_dim = decoder ? 1 : vae_dim;
    net.in_Tpf = decoder ? 1 : hop;
    net.in_hist = 6;
    net.maxC = 1;
    size_t umax = 0;
    // ---- weights (shared across slots) ----
    struct StageW { ConvG in; std::vector<Block> blocks; };
    std::vector<StageW> sw(ns);
    for (int i = 0; i < ns; ++i) {
        ConvG& g = sw[i].in;
        char nm[256];
        if (i == 0) {
            const int Cin = net.in_dim;
            g.K = 7 * Cin; g.N = C[0]; g.ldx = Cin; g.rows_per_frame = Tpf[0];
            g.w = alloc_packed(ctx, g.N, g.K);
            snprintf(nm, 256, "%s%s.0.0.conv.conv.", pfx.c_str(), decoder ? "upsample_layers" : "downsample_layers");
            add_mat(ctx, std::string(nm) + "weight", g.N, g.K, g.w, 0, 1, Cin, g.N, 7, 1);
            g.bias = add_vec(ctx, std::string(nm) + "bias", g.N);
        } else if (decoder) {
            const int s = ratios[i - 1], Cin = C[i - 1], Cout = C[i];
            g.K = 2 * Cin; g.N = s * Cout; g.ldx = Cin; g.rows_per_frame = Tpf[i - 1];
            g.w = alloc_packed(ctx, g.N, g.K);
            snprintf(nm, 256, "%supsample_layers.%d.0.convtr.convtr.", pfx.c_str(), i);
            add_mat(ctx, std::string(nm) + "weight", g.N, g.K, g.w, 0, 2, Cin, Cout, 2 * s, s, (int64_t)Cin * Cout * 2 * s);
            g.bias = add_vec(ctx, std::string(nm) + "bias", Cout, nullptr, W_BIAS_REP, s);
        } else {
            const int s = ratios[i - 1], Cin = C[i - 1], Cout = C[i];
            g.K = 2 * s * Cin; g.N = Cout; g.ldx = s * Cin; g.rows_per_frame = Tpf[i];
            g.w = alloc_packed(ctx, g.N, g.K);
            snprintf(nm, 256, "%sdownsample_layers.%d.0.conv.conv.", pfx.c_str(), i);
            add_mat(ctx, std::string(nm) + "weight", g.N, g.K, g.w, 0, 1, Cin, Cout, 2 * s, s);
            g.bias = add_vec(ctx, std::string(nm) + "bias", Cout);
        }
        if (C[i] > net.maxC) net.maxC = C[i];
        for (int j = 0; j < depths[i]; ++j) {
            Block b; b.C = C[i]; b.nb = nullptr;
            snprintf(nm, 256, "%sstages.%d.%d.", pfx.c_str(), i, j);
            std::string p(nm);
            b.gamma = add_vec(ctx, p + "gamma", C[i]);
            b.ffn_gamma = add_vec(ctx, p + "ffn_gamma", C[i]);
            b.norm_w = add_vec(ctx, p + "norm.weight", C[i]);
            b.ffn_norm_w = add_vec(ctx, p + "ffn_norm.weight", C[i]);
            b.dw_w = add_vec(ctx, p + "mixer.conv.conv.conv.weight", (int64_t)C[i] * 7, nullptr, W_DW);
            b.dw_b = add_vec(ctx, p + "mixer.conv.conv.conv.bias", C[i]);
            b.w1 = alloc_packed(ctx, 4 * C[i], C[i]);
            add_mat(ctx, p + "ffn.linear1.weight", 4 * C[i], C[i], b.w1, 0);
            b.b1 = add_vec(ctx, p + "ffn.linear1.bias", 4 * C[i]);
            b.w2 = alloc_packed(ctx, C[i], 4 * C[i]);
            add_mat(ctx, p + "ffn.linear2.weight", C[i], 4 * C[i], b.w2, 0);
            b.b2 = add_vec(ctx, p + "ffn.linear2.bias", C[i]);
            sw[i].blocks.push_back(b);
            size_t ub = (size_t)Tpf[i] * Fmax * 4 * C[i] * 4;
            if (ub > umax) umax = ub;
        }
    }
    {   // head conv k7
        ConvG& g = net.head;
        const int Cin = C[ns - 1];
        g.K = 7 * Cin; g.N = net.out_dim; g.ldx = Cin; g.rows_per_frame = Tpf[ns - 1];
        g.w = alloc_packed(ctx, g.N, g.K);
        add_mat(ctx, pfx + "head.conv.conv.weight", g.N, g.K, g.w, 0, 1, Cin, g.N, 7, 1);
        g.bias = add_vec(ctx, pfx + "head.conv.conv.bias", g.N);
    }
    // ---- per-slot buffers + shift tables.  Every kind of buffer is ONE allocation with a uniform slot stride (a multiple of
    // 64 floats), so a slot-batched launch reaches utterance k's copy at base + k * stride ----
    auto pad64 = [](size_t n) { return (n + 63) / 64 * 64; };
    net.u.resize(n_slots);
    net.u_stride = (int64_t)pad64(umax / 4 + 1);
    float* u_all = (float*)dalloc(ctx, (size_t)n_slots * net.u_stride * 4, false);
    net.in_buf.resize(n_slots); net.st.resize(n_slots);
    net.in_stride = (int64_t)pad64((size_t)(6 + net.in_Tpf * Fmax) * net.in_dim);
    float* in_all = (float*)dalloc(ctx, (size_t)n_slots * net.in_stride * 4);
    if (!u_all || !in_all) return -1;
    for (int sl = 0; sl < n_slots; ++sl) {
        net.u[sl] = u_all + (size_t)sl * net.u_stride;
        net.in_buf[sl] = in_all + (size_t)sl * net.in_stride;
        net.st[sl].resize(ns);
    }
    for (int i = 0; i < ns; ++i) {
        const int hist = (i == ns - 1) ? 6 : (decoder ? 1 : ratios[i]);
        const bool fused = vv_block1d_supported(C[i]) && Tpf[i] >= 8 && !sw[i].blocks.empty();
        // unfused stages ping-pong between xs and xs2 when a one-launch norm + depthwise-conv kernel exists for them:
        // channel-sliced (T <= 8, C = 1024 / 2048) or row-tiled (middle stages, any T)
        const bool pp = !fused && !sw[i].blocks.empty() && (vv_normdw_sliced_ok(Tpf[i], C[i]) || vv_normdw_rows_ok(Tpf[i], C[i]));
        const int64_t xstride = (int64_t)pad64((size_t)(hist + (size_t)Tpf[i] * Fmax) * C[i]);
        float* xs_all = (float*)dalloc(ctx, (size_t)n_slots * xstride * 4);
        float* xs2_all = (fused || pp) ? (float*)dalloc(ctx, (size_t)n_slots * xstride * 4) : nullptr;
        if (!xs_all || ((fused || pp) && !xs2_all)) return -1;
        const int64_t nbstride = (int64_t)pad64(fused ? (size_t)12 * C[i] : (size_t)(6 + (size_t)Tpf[i] * Fmax) * C[i]);
        std::vector<float*> nb_all(sw[i].blocks.size());
        for (auto& p : nb_all) { p = (float*)dalloc(ctx, (size_t)n_slots * nbstride * 4); if (!p) return -1; }
        for (int sl = 0; sl < n_slots; ++sl) {
            Stage& s = net.st[sl][i];
            s.C = C[i]; s.Tpf = Tpf[i]; s.in = sw[i].in; s.hist = hist; s.fused = fused; s.pp = pp; s.sl_stride = xstride;
            s.xs = xs_all + (size_t)sl * xstride;
            s.xs2 = xs2_all ? xs2_all + (size_t)sl * xstride : nullptr;
            s.blocks = sw[i].blocks;
            s.xfinal = ((s.fused || s.pp) && (s.blocks.size() & 1)) ? s.xs2 : s.xs;
            for (size_t j = 0; j < s.blocks.size(); ++j) {
                Block& b = s.blocks[j];
                b.nb = nullptr; b.nst = nullptr; b.nb_stride = nbstride;
                if (s.fused) b.nst = nb_all[j] + (size_t)sl * nbstride;
                else b.nb = nb_all[j] + (size_t)sl * nbstride;
            }
        }
    }
    // which stages can run slot-batched (bf16 modes): the incoming conv as a slot-batched GEMV (or the stem kernel), the blocks
    // as fused block kernels, or channel-sliced / row-tiled norm+conv + slot-batched FFN GEMVs.  VVHIP_BATCH_CODEC=heavy keeps
    // only the weight-heavy T <= 8 stages batched (the rest per utterance on forked streams), =0 turns batching off.
    {
        const char* mode = getenv("VVHIP_BATCH_CODEC");
        const bool off = (mode && !strcmp(mode, "0")) || ctx->c.xsplit > 2 || n_slots < 2 || Fmax != 1;
        const bool heavy_only = mode && !strcmp(mode, "heavy");
        auto gemm_ok = [&](const ConvG& cg, int64_t sx, int64_t sy) {
            VVGemm g = mk_gemm(cg.w, net.in_buf[0], net.u[0], 2 * cg.rows_per_frame, cg.N, cg.K, cg.ldx, cg.N);
            g.epi = VV_EPI_BIAS; g.bias = cg.bias;
            g.sl_n = 2; g.sl_T = cg.rows_per_frame; g.sl_x = (int)sx; g.sl_y = (int)sy; g.sl_id[0] = 0; g.sl_id[1] = n_slots - 1;
            return vv_gemv_ok(&g) != 0;
        };
        auto ok = [&](int i) {
            const Stage& s = net.st[0][i];
            if (off || s.blocks.empty() || (s.C & 31)) return false;
            if (!is_stem(s.in) && !gemm_ok(s.in, i == 0 ? net.in_stride : net.st[0][i - 1].sl_stride, s.sl_stride)) return false;
            if (s.pp && vv_normdw_sliced_ok(s.Tpf, s.C)) return true;
            if (heavy_only) return false;
            return s.fused || (s.pp && vv_normdw_rows_ok(s.Tpf, s.C));
        };
        net.kd = 0; net.ke = ns;
        if (decoder) { while (net.kd < ns && ok(net.kd)) net.kd++; }
        else { while (net.ke > 0 && ok(net.ke - 1)) net.ke--; }
        const ConvG& h = net.head;
        const bool conv1 = is_conv1_head(h);
        net.head_batch = !off && !heavy_only && (conv1 || gemm_ok(h, net.st[0][ns - 1].sl_stride, 0));
        if (!decoder && net.ke < ns && !(conv1 || gemm_ok(h, net.st[0][ns - 1].sl_stride, 0))) net.ke = ns;   // encoder tail needs its head batched
    }
    return 0;
}

// The slots one pass of the walker covers.  n == 0 (ids null): slot `sl` alone -- its base pointers, no VVGemm::sl_* fields, zero slot
// strides.  n >= 1: slots ids[0..n) (ascending, one frame each) in ONE pass over the weights -- base pointers of slot 0, uniform slot
// strides; every GEMM carries the rows of all n slots (sl_*: gathered from / scattered to the per-slot buffers), other kernels take the slot from blockIdx.y.
struct SlotSet { const int* ids; int n; int sl; };
static SlotSet one_slot(int sl) { return {nullptr, 0, sl}; }

static void codec_table_entries(CodecNet& net, int sl, int F, std::vector<VVShiftH>& t) {
    t.push_back({net.in_buf[sl], net.in_Tpf * F, 6, net.in_dim});
    for (auto& s : net.st[sl]) {
        t.push_back({s.xfinal, s.Tpf * F, s.hist, s.C});
        for (auto& b : s.blocks) {
            if (s.fused) t.push_back({b.nst, 6, 6, s.C});
            else t.push_back({b.nb, s.Tpf * F, 6, s.C});
        }
    }
}
// the history-shift table of a slot set at F frames per pass (one launch moves every buffer's history), cached by (slot mask, F)
static int codec_tables(vv_ctx* ctx, CodecNet& net, SlotSet ss, int F, void** tab_out, int* n_out) {
    const int* ids = ss.n ? ss.ids : &ss.sl;
    const int n = ss.n ? ss.n : 1;
    uint64_t mask = 0;
    for (int j = 0; j < n; ++j) {
        if (ids[j] >= 64) return fail(ctx, "tokenizer slot %d: the history tables are keyed by a 64-bit slot mask", ids[j]);
        mask |= 1ull << ids[j];
    }
    auto it = net.shift_tab.find({mask, F});
    if (it == net.shift_tab.end()) {
        std::vector<VVShiftH> t;
        for (int j = 0; j < n; ++j) codec_table_entries(net, ids[j], F, t);
        void* d = dalloc(ctx, t.size() * sizeof(VVShiftH), false);
        if (!d) return -1;
        HIPCHK(ctx, hipMemcpy(d, t.data(), t.size() * sizeof(VVShiftH), hipMemcpyHostToDevice));
        it = net.shift_tab.emplace(std::make_pair(mask, F), std::make_pair(d, (int)t.size())).first;
    }
    *tab_out = it->second.first; *n_out = it->second.second;
    return 0;
}

// Runs stages [i0, i1) (i1 < 0: to the end) of one codec net over F frames for a slot set; `head` / `shift`: run the head conv / the
// history shift at the end.  The caller has already written the input rows into in_buf + 6 * in_dim of every slot.  `out`: the head
// conv's rows, dense [n][rows][out_dim] for a set.  vv_codec_chain_batch runs part of a net for a set and the rest per utterance.
// tail_valid >= 0 (encoder, last pass of a ragged input): only the first tail_valid rows of stage 0's output are real signal.
// The reference's non-streaming encoder right-pads with zeros PER strided conv (SConv1d: get_extra_padding_for_conv1d), i.e. the
// rows past the end of the signal are ZERO at the input of every strided conv -- not conv(0) + bias, which is what the rows past the
// end hold here when the waveform is zero-padded to whole frames.  Every layer is causal, so zeroing those rows of stage i-1's
// output right before stage i's incoming conv reproduces the reference exactly; only the last, partial frame's latent changes.
// Only the voice-prompt encoder passes tail_valid, and only stages build_codec admits (fused, or pp with a one-launch norm + conv
// kernel) run for a set: the fallback norm / conv forms below never see one.
static int run_codec(vv_ctx* ctx, CodecNet& net, SlotSet ss, int F, float* out, hipStream_t st, int i0 = 0, int i1 = -1,
                     bool head = true, bool shift = true, int tail_valid = -1) {
    const float eps = ctx->c.codec_eps;
    const bool batched = ss.n > 0;
    const bool stream_w = (F == 1);      // T=1 stages stream their weights exactly once
    const int base = batched ? 0 : ss.sl;      // the slot whose descriptors hold the base pointers
    auto& stages = net.st[base];
    float* u = net.u[base];                    // FFN hidden scratch; a set's is dense [n * T][4C]
    const int ns = (int)stages.size();
    if (i1 < 0) i1 = ns;
    // what the set means for a launch: a kernel's slot stride (zero for a single slot) and a GEMM's sl_* fields (rows per slot; sx /
    // sy: slot stride of its input / output side, 0 = dense scratch).  A single slot leaves the GEMM as mk_gemm made it.
    auto stride = [&](int64_t s) { return batched ? s : (int64_t)0; };
    auto slots = [&](VVGemm& g, int rows, int64_t sx, int64_t sy) {
        if (!batched) return;
        g.sl_n = ss.n; g.sl_T = rows; g.sl_x = (int)sx; g.sl_y = (int)sy; g.T = ss.n * rows;
        for (int j = 0; j < 8; ++j) g.sl_id[j] = j < ss.n ? ss.ids[j] : 0;
    };
    // FIRST of the two places the walks of a set and of a single slot differ: a set's GEMMs always stream their weights non-temporally
    auto nt = [&](int rows) { return batched ? 1 : (int)(stream_w && rows <= 16); };
    // a block's FFN pair over the rows in xo.  dw_in (one-row stages): FFN1's prologue also runs the block's norm + depthwise conv +
    // layer scale + residual on the block's input row dw_in (VV_PRO_NORMDW) and writes xo itself
    auto ffn1 = [&](const Stage& s, const Block& b, float* xo, int T, const float* dw_in) {
        VVGemm g1 = mk_gemm(b.w1, dw_in ? dw_in : xo, u, T, 4 * s.C, s.C, s.C, 4 * s.C);
        g1.pro = VV_PRO_RMS; g1.nw = b.ffn_norm_w; g1.eps = eps; g1.epi = VV_EPI_BIAS_GELU; g1.bias = b.b1; g1.nt = nt(T);
        if (dw_in) {
            g1.pro = VV_PRO_NORMDW;
            g1.dw_hist = b.nb; g1.dw_w = b.dw_w; g1.dw_b = b.dw_b; g1.dw_gamma = b.gamma; g1.dw_nw = b.norm_w;
            g1.dw_xout = xo; g1.dw_hnew = b.nb + 6 * (size_t)s.C;
        }
        slots(g1, T, s.sl_stride, 0);
        return g1;
    };
    auto ffn = [&](const Stage& s, const Block& b, const VVGemm& g1, float* xo, int T) -> int {
        GEMM(g1);
        VVGemm g2 = mk_gemm(b.w2, u, xo, T, s.C, 4 * s.C, 4 * s.C, s.C);
        g2.epi = VV_EPI_RESID; g2.bias = b.b2; g2.nscale = b.ffn_gamma; g2.nt = nt(T);
        slots(g2, T, 0, s.sl_stride);
        GEMM(g2);
        return 0;
    };
    for (int i = i0; i < i1; ++i) {
        Stage& s = stages[i];
        const int T = s.Tpf * F;
        float* x = s.xs + (size_t)s.hist * s.C;
        if (tail_valid >= 0 && i > 0) {
            Stage& pv = stages[i - 1];
            const int Tp = pv.Tpf * F;
            if (tail_valid < Tp)
                VVCHK(vv_zero_launch(pv.xfinal + ((size_t)pv.hist + tail_valid) * pv.C, (size_t)(Tp - tail_valid) * pv.C * 4, st));
            const int r = pv.Tpf / s.Tpf;                       // this stage's incoming stride
            tail_valid = (tail_valid + r - 1) / r;
        }
        {   // incoming conv: per-slot window rows in, per-slot stage rows out
            const ConvG& cg = s.in;
            const float* X = (i == 0) ? net.in_buf[base] : stages[i - 1].xfinal;
            const int64_t sx = (i == 0) ? net.in_stride : stages[i - 1].sl_stride;
            const int Trows = cg.rows_per_frame * F;
            if (is_stem(cg)) {
                ctx->launches++;
                VVCHK(vv_stem_conv_slots_launch(X, cg.w, cg.bias, x, Trows, cg.N, ss.ids, ss.n, stride(sx), stride(s.sl_stride), st));
            } else {
                VVGemm g = mk_gemm(cg.w, X, x, Trows, cg.N, cg.K, cg.ldx, cg.N);
                g.epi = VV_EPI_BIAS; g.bias = cg.bias; g.nt = nt(Trows);
                slots(g, Trows, sx, s.sl_stride);
                GEMM(g);
            }
        }
        // fused and pp stages: each block reads one of xs / xs2 and writes the other
        float* xo = (s.fused || s.pp) ? s.xs2 + (size_t)s.hist * s.C : x;
        if (s.fused) {
            for (auto& b : s.blocks) {
                ctx->launches++;
                VVCHK(vv_block1d_slots_launch(s.C, ctx->c.xsplit, x, xo, b.nst, b.norm_w, b.ffn_norm_w, b.gamma, b.ffn_gamma, b.dw_w, b.dw_b,
                                              b.b1, b.b2, b.w1, b.w2, T, eps, ss.ids, ss.n, stride(s.sl_stride), stride(b.nb_stride), st));
                std::swap(x, xo);
            }
            continue;
        }
        for (auto& b : s.blocks) {
            const bool sliced = s.pp && vv_normdw_sliced_ok(T, s.C);
            // SECOND place: one-row stages of a single slot (C = 2048: 8 blocks per net) run the block's norm + depthwise conv + layer
            // scale + residual in FFN1's prologue -- one launch less per block on a chain where every launch is a latency link
            if (sliced && T == 1 && !batched) {
                const VVGemm g1 = ffn1(s, b, xo, T, x);
                if (vv_gemv_ok(&g1)) {
                    VVTRY(ffn(s, b, g1, xo, T));
                    std::swap(x, xo);
                    continue;
                }
            }
            if (sliced) {
                ctx->launches += 1;
                VVCHK(vv_normdw_sliced_slots_launch(x, xo, b.nb, b.norm_w, b.dw_w, b.dw_b, b.gamma, T, s.C, eps, ss.ids, ss.n, stride(s.sl_stride),
                                                    stride(b.nb_stride), st));
            } else if (s.pp && vv_normdw_rows_ok(T, s.C)) {
                ctx->launches += 1;
                VVCHK(vv_normdw_rows_slots_launch(x, xo, b.nb, b.norm_w, b.dw_w, b.dw_b, b.gamma, T, s.C, eps, ss.ids, ss.n, stride(s.sl_stride),
                                                  stride(b.nb_stride), st));
            } else if (!s.pp && (size_t)T * s.C <= 8192 && (s.C & 3) == 0) {     // one workgroup is only faster for tiny row sets
                ctx->launches += 1;
                VVCHK(vv_normdw_launch(x, b.nb, b.norm_w, b.dw_w, b.dw_b, b.gamma, T, s.C, eps, st));
            } else {
                ctx->launches += 2;
                VVCHK(vv_rmsnorm_rows_launch(x, s.C, b.nb + 6 * (size_t)s.C, s.C, b.norm_w, T, s.C, eps, st));
                VVCHK(vv_dwconv_res_launch(b.nb, x, xo, b.dw_w, b.dw_b, b.gamma, T, s.C, st));
            }
            VVTRY(ffn(s, b, ffn1(s, b, xo, T, nullptr), xo, T));
            if (s.pp) std::swap(x, xo);
        }
    }
    if (head) {   // head conv
        const ConvG& cg = net.head;
        Stage& s = stages[ns - 1];
        const int Trows = cg.rows_per_frame * F;
        if (is_conv1_head(cg)) {
            ctx->launches++;
            VVCHK(vv_head_conv1_slots_launch(s.xfinal, cg.w, cg.bias, out, Trows, cg.ldx, ss.ids, ss.n, stride(s.sl_stride), stride(Trows), st));
        } else {
            VVGemm g = mk_gemm(cg.w, s.xfinal, out, Trows, cg.N, cg.K, cg.ldx, cg.N);
            g.epi = VV_EPI_BIAS; g.bias = cg.bias;
            slots(g, Trows, s.sl_stride, 0);
            GEMM(g);
        }
    }
    if (!shift) return 0;
    void* tab; int n_tab;
    if (codec_tables(ctx, net, ss, F, &tab, &n_tab)) return -1;
    ctx->launches++;
    VVCHK(vv_shift_rows_launch(tab, n_tab, net.maxC, st));
    return 0;
}

static int zero_codec(vv_ctx* ctx, CodecNet& net, int sl, hipStream_t st) {
    void* tab; int nt;
    if (codec_tables(ctx, net, one_slot(sl), 1, &tab, &nt)) return -1;
    ctx->launches++;
    VVCHK(vv_zero_hist_launch(tab, nt, st));
    return 0;
}
extern "C" int vv_codec_decode(vv_ctx* ctx, void* stream, int slot, int frames, const float* latent_dev, float* audio_out_dev, int apply) {
    hipStream_t st = (hipStream_t)stream;
    if (slot < 0 || slot >= ctx->c.n_slots) return fail(ctx, "slot %d out of range", slot);
    if (frames != 1) return fail(ctx, "vv_codec_decode: streaming decode takes one frame per call");
    CodecNet& net = ctx->dec;
    ctx->launches = 0;
    // apply leads the key: vv_set_speech_factors drops the graphs that hold the factors by the prefix "dec:1:"
    char key[128]; snprintf(key, 128, "dec:%d:%d:%d:%p:%p", apply ? 1 : 0, slot, frames, (const void*)latent_dev, (void*)audio_out_dev);
    return graphed(ctx, key, st, [&]() {
        const int L = ctx->c.latent_dim;
        const float mul = apply ? 1.0f / ctx->scaling : 1.0f, add = apply ? -ctx->bias : 0.0f;
        ctx->launches++;
        VVCHK(vv_affine_launch(latent_dev, net.in_buf[slot] + 6 * L, mul, add, frames * L, st));
        return run_codec(ctx, net, one_slot(slot), frames, audio_out_dev, st);
    });
}

extern "C" int vv_semantic_encode(vv_ctx* ctx, void* stream, int slot, int frames, const float* audio_dev, float* sem_out_dev) {
    hipStream_t st = (hipStream_t)stream;
    if (ctx->c.sem_dim <= 0) return fail(ctx, "no semantic tokenizer configured");
    if (slot < 0 || slot >= ctx->c.n_slots) return fail(ctx, "slot %d out of range", slot);
    if (frames != 1) return fail(ctx, "vv_semantic_encode: streaming encode takes one frame per call");
    CodecNet& net = ctx->senc;
    ctx->launches = 0;
    char key[128]; snprintf(key, 128, "senc:%d:%d:%p:%p", slot, frames, (const void*)audio_dev, (void*)sem_out_dev);
    return graphed(ctx, key, st, [&]() {
        VVCHK(vv_copy_launch(net.in_buf[slot] + 6, audio_dev, (size_t)frames * ctx->hop * 4, st));
        return run_codec(ctx, net, one_slot(slot), frames, sem_out_dev, st);
    });
}

// One frame of n utterances through the acoustic decoder and (sem_out_dev != null) the semantic encoder -- the batched
// `acoustic_tokenizer.decode(..., sample_indices=diffusion_indices)` + `semantic_tokenizer.encode(...)` pair of the reference's
// loop (modeling_vibevoice_inference.py:636-672).  Row j of latent / audio / sem belongs to slot slots[j].  The stages that
// hold the weight bytes (decoder stages [0, kd), encoder stages [ke, end) + head) run slot-batched: one pass over the weights
// for the whole batch; the many-row, few-channel stages in between run per utterance on forked streams.
extern "C" int vv_codec_chain_batch(vv_ctx* ctx, void* stream, int n, const int* slots, const float* latent_dev,
                                    float* audio_out_dev, float* sem_out_dev, int apply) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || n > 8) return fail(ctx, "vv_codec_chain_batch: n = %d, must be 1..8", n);
    uint64_t mask = 0;
    for (int j = 0; j < n; ++j) {
        if (slots[j] < 0 || slots[j] >= ctx->c.n_slots || slots[j] >= 64) return fail(ctx, "slot %d out of range", slots[j]);
        if (mask & (1ull << slots[j])) return fail(ctx, "vv_codec_chain_batch: slot %d listed twice", slots[j]);
        mask |= 1ull << slots[j];
    }
    const bool sem = sem_out_dev != nullptr;
    if (sem && ctx->c.sem_dim <= 0) return fail(ctx, "no semantic tokenizer configured");
    if (!ctx->side_ready) {
        for (int j = 0; j < 8; ++j) {
            HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->side[j], hipStreamNonBlocking));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_join[j], hipEventDisableTiming));
        }
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        ctx->side_ready = true;
    }
    ctx->launches = 0;
    std::string key = apply ? "chain:1:" : "chain:0:";      // vv_set_speech_factors drops "chain:1:", the graphs that hold the factors
    for (int j = 0; j < n; ++j) key += std::to_string(slots[j]) + ",";
    char kp[128]; snprintf(kp, 128, ":%p:%p:%p", (const void*)latent_dev, (void*)audio_out_dev, (void*)sem_out_dev);
    key += kp;
    std::vector<int> ids(slots, slots + n);
    return graphed(ctx, key, st, [&]() {
        CodecNet& dec = ctx->dec; CodecNet& senc = ctx->senc;
        const int L = ctx->c.latent_dim, S = ctx->c.sem_dim, hop = ctx->hop;
        const float mul = apply ? 1.0f / ctx->scaling : 1.0f, add = apply ? -ctx->bias : 0.0f;
        const int ns_d = (int)dec.st[0].size(), ns_e = sem ? (int)senc.st[0].size() : 0;
        const bool bd = n > 1 && dec.kd > 0, be = sem && n > 1 && senc.ke < ns_e;
        const bool dec_full = bd && dec.kd == ns_d && dec.head_batch;      // the whole decoder runs slot-batched
        const bool enc_full = be && senc.ke == 0;
        const bool fork = n > 1 && !(dec_full && (!sem || enc_full));      // some part still runs per utterance
        const SlotSet set = {ids.data(), n, 0};
        if (bd) {
            ctx->launches++;
            VVCHK(vv_affine_slots_launch(latent_dev, dec.in_buf[0] + 6 * L, mul, add, L, ids.data(), n, dec.in_stride, st));
            if (run_codec(ctx, dec, set, 1, audio_out_dev, st, 0, dec.kd, dec_full, dec_full)) return -1;
        }
        if (fork || n == 1) {
            if (fork) HIPCHK(ctx, hipEventRecord(ctx->ev_fork, st));
            for (int j = 0; j < n; ++j) {
                hipStream_t ss = fork ? ctx->side[j] : st;
                const int sl = ids[j];
                if (fork) HIPCHK(ctx, hipStreamWaitEvent(ss, ctx->ev_fork, 0));
                float* audio = audio_out_dev + (size_t)j * hop;
                if (!dec_full) {
                    if (!bd) {
                        ctx->launches++;
                        VVCHK(vv_affine_launch(latent_dev + (size_t)j * L, dec.in_buf[sl] + 6 * L, mul, add, L, ss));
                    }
                    if (run_codec(ctx, dec, one_slot(sl), 1, audio, ss, bd ? dec.kd : 0, ns_d, true, true)) return -1;
                }
                if (sem) {
                    VVCHK(vv_copy_launch(senc.in_buf[sl] + 6, audio, (size_t)hop * 4, ss));
                    if (run_codec(ctx, senc, one_slot(sl), 1, sem_out_dev + (size_t)j * S, ss, 0, be ? senc.ke : ns_e, !be, !be)) return -1;
                }
                if (fork) HIPCHK(ctx, hipEventRecord(ctx->ev_join[j], ss));
            }
            if (fork) for (int j = 0; j < n; ++j) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join[j], 0));
        } else if (sem) {
            ctx->launches++;       // the batch's audio rows into the encoder's per-utterance input buffers
            VVCHK(vv_affine_slots_launch(audio_out_dev, senc.in_buf[0] + 6, 1.0f, 0.0f, hop, ids.data(), n, senc.in_stride, st));
        }
        if (be && run_codec(ctx, senc, set, 1, sem_out_dev, st, senc.ke, ns_e, true, true)) return -1;
        return 0;
    });
}

// valid_samples: samples of real signal in wav_dev [frames * hop] (the rest must be zeros); frames = ceil(valid_samples / hop).
extern "C" int vv_acoustic_encode_ragged(vv_ctx* ctx, void* stream, int frames, long long valid_samples, const float* wav_dev, float* mean_out_dev) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->c.has_acoustic_encoder) return fail(ctx, "no acoustic encoder configured");
    if (valid_samples <= (int64_t)(frames - 1) * ctx->hop || valid_samples > (int64_t)frames * ctx->hop)
        return fail(ctx, "vv_acoustic_encode_ragged: %lld valid samples do not end in frame %d of %d", (long long)valid_samples, frames - 1, frames);
    CodecNet& net = ctx->aenc;
    if (zero_codec(ctx, net, 0, st)) return -1;
    const int L = ctx->c.latent_dim;
    const int pass = ctx->enc_pass > 0 ? std::min(ctx->enc_pass, net.Fmax) : net.Fmax;
    for (int f0 = 0; f0 < frames; f0 += pass) {
        const int F = std::min(pass, frames - f0);
        VVCHK(vv_copy_launch(net.in_buf[0] + 6, wav_dev + (size_t)f0 * ctx->hop, (size_t)F * ctx->hop * 4, st));
        const int64_t v = valid_samples - (int64_t)f0 * ctx->hop;            // real samples inside this pass
        const int tail = (f0 + F == frames && v < (int64_t)F * ctx->hop) ? (int)v : -1;
        if (run_codec(ctx, net, one_slot(0), F, mean_out_dev + (size_t)f0 * L, st, 0, -1, true, true, tail)) return -1;
    }
    return 0;
}

extern "C" int vv_acoustic_encode(vv_ctx* ctx, void* stream, int frames, const float* wav_dev, float* mean_out_dev) {
    return vv_acoustic_encode_ragged(ctx, stream, frames, (long long)frames * ctx->hop, wav_dev, mean_out_dev);
}

extern "C" int vv_set_enc_pass_frames(vv_ctx* ctx, int frames_per_pass) {
    if (!ctx->c.has_acoustic_encoder) return fail(ctx, "no acoustic encoder configured");
    if (frames_per_pass < 1 || frames_per_pass > ctx->aenc.Fmax) return fail(ctx, "frames_per_pass %d out of range [1,%d]", frames_per_pass, ctx->aenc.Fmax);
    ctx->enc_pass = frames_per_pass;
    return 0;
}

extern "C" int vv_codec_reset(vv_ctx* ctx, void* stream, int slot) {
    VV_SHARED;
    hipStream_t st = (hipStream_t)stream;
    if (slot < 0 || slot >= ctx->c.n_slots) return fail(ctx, "slot %d out of range", slot);
    if (zero_codec(ctx, ctx->dec, slot, st)) return -1;
    if (ctx->c.sem_dim > 0 && zero_codec(ctx, ctx->senc, slot, st)) return -1;
    return 0;
}

// ------------------------------------------------------------------ streaming row stages: what the resampler, the tempo change, the level and the loudness leveller share
// A stage keeps chunk-continuous streams (vv_ctx::RowStage) and takes up to 16 rows per push, one stream each.  `fn` is the entry
// point's name: every refusal carries it.  `s` is null where the configuration is not set.  Every stage calls the same three.

// streams back to their first sample: launch(ids, n) zeroes the device state of up to 16 of them, clear(id) the stage's own host state
template <class Launch, class Clear>
static int stage_reset(vv_ctx* ctx, const char* fn, vv_ctx::RowStage* s, int cfg, int n, const int* stream_ids_host, Launch launch, Clear clear) {
    if (!s) return fail(ctx, "%s: configuration %d is not set", fn, cfg);
    std::vector<int> ids;
    if (!stream_ids_host) { for (int i = 0; i < s->n_streams; ++i) ids.push_back(i); }
    else {
        if (n < 1) return fail(ctx, "%s: n = %d must be >= 1", fn, n);
        ids.assign(stream_ids_host, stream_ids_host + n);
    }
    for (int id : ids)
        if (id < 0 || id >= s->n_streams) return fail(ctx, "%s: stream id %d out of range [0,%d)", fn, id, s->n_streams);
    for (size_t i0 = 0; i0 < ids.size(); i0 += 16)
        VVCHK(launch(ids.data() + i0, (int)std::min<size_t>(16, ids.size() - i0)));
    for (int id : ids) { s->total[id] = 0; s->flushed[id] = 0; clear(id); }
    return 0;
}

// The refusals of a push that do not depend on the stage, in the order the entry points make them: head() once, then per row stream(),
// input() and open(), the stage's own checks between them where it has some.  A refusal has recorded its text and returns -1.
struct RowCheck {
    vv_ctx* ctx; const char* fn; const vv_ctx::RowStage* s; const float* audio_dev; int ld_in;
    int head(int cfg, int n, const void* rows_host, const void* out_dev, const int* n_out_host, int out_fmt) const {
        if (!s) return fail(ctx, "%s: configuration %d is not set", fn, cfg);
        if (n < 1 || n > 16) return fail(ctx, "%s: n = %d must be in [1,16]", fn, n);
        if (!rows_host || !out_dev || !n_out_host) return fail(ctx, "%s: null rows / out / n_out pointer", fn);
        if (out_fmt != 0 && out_fmt != 1) return fail(ctx, "%s: out_fmt = %d must be 0 (fp32) or 1 (int16)", fn, out_fmt);
        return 0;
    }
    template <class Row>
    int stream(const Row* rows, int i) const {
        const Row& q = rows[i];
        if (q.stream < 0 || q.stream >= s->n_streams) return fail(ctx, "%s: row %d: stream id %d out of range [0,%d)", fn, i, q.stream, s->n_streams);
        for (int j = 0; j < i; ++j)
            if (rows[j].stream == q.stream) return fail(ctx, "%s: stream %d is named twice (rows %d and %d)", fn, q.stream, j, i);
        if (q.n_in < 0) return fail(ctx, "%s: row %d: n_in = %d must be >= 0", fn, i, q.n_in);
        return 0;
    }
    int input(int i, int n_in) const {
        if (n_in > ld_in || (n_in > 0 && !audio_dev)) return fail(ctx, "%s: row %d: n_in = %d exceeds the input rows (ld_in = %d)", fn, i, n_in, ld_in);
        return 0;
    }
    int open(int stream) const {
        if (s->flushed[stream]) return fail(ctx, "%s: stream %d has been flushed; reset it before its next push", fn, stream);
        return 0;
    }
};

// the end of a push: the unused rows of the kernel's argument repeat row 0, launch() runs it, and only then do the streams move on
template <class Row, class KRows, class Launch>
static int stage_launch(vv_ctx* ctx, vv_ctx::RowStage& s, const Row* rows_host, int n, KRows& kr, int* n_out_host, Launch launch) {
    for (int i = n; i < 16; ++i) kr.r[i] = kr.r[0];
    VVCHK(launch());
    for (int i = 0; i < n; ++i) {
        s.total[rows_host[i].stream] += rows_host[i].n_in;
        if (rows_host[i].flush) s.flushed[rows_host[i].stream] = 1;
        n_out_host[i] = kr.r[i].n_out;
    }
    return 0;
}

// ------------------------------------------------------------------ audio at another sample rate (kernels: resample.hip)
// Outputs a stream has emitted once `total` input samples have arrived: every m whose newest input sample, index
// (m * M + D) / L with D = (L * T - 2) / 2, is below total.  vibevoice_amd/resample.py (emitted) is the same arithmetic.
static int64_t rs_emitted(int64_t total, int L, int M, int T) {
    const int64_t a = total * L - (L * T - 2) / 2 - 1;
    return a < 0 ? 0 : a / M + 1;
}

extern "C" int vv_resampler_set(vv_ctx* ctx, int rs, int L, int M, int T, const float* coef_host, int n_streams, void* stream) {
    VV_SHARED;
    if (rs < 0 || rs >= vv_ctx::N_RESAMPLERS) return fail(ctx, "vv_resampler_set: configuration %d out of range [0,%d)", rs, vv_ctx::N_RESAMPLERS);
    if (L < 1 || L > 4096 || M < 1 || M > 4096) return fail(ctx, "vv_resampler_set: L = %d, M = %d must be in [1,4096]", L, M);
    if (T < 2 || (T & 1) || T > 4096) return fail(ctx, "vv_resampler_set: T = %d must be even and in [2,4096]", T);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_resampler_set: n_streams = %d must be in [1,65536]", n_streams);
    if (!coef_host) return fail(ctx, "vv_resampler_set: null coefficient table");
    // the table, the history and at least the T / 2 samples a push must be able to bring must fit the kernel's LDS
    if (vv_resample_lds_bytes(L, T, T) > 65536 - 64)
        return fail(ctx, "vv_resampler_set: the %d x %d coefficient table (%d bytes) does not fit the resampling kernel's 64 KiB of LDS; "
                         "this rate pair is not served", L, T, L * T * 4);
    vv_ctx::Resampler& r = ctx->rs[rs];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, r.coef); dfree(ctx, r.hist);
    r = vv_ctx::Resampler();
    float* coef = (float*)dalloc(ctx, (size_t)L * T * 4, false);
    float* hist = (float*)dalloc(ctx, (size_t)n_streams * T * 4, true);
    if (!coef || !hist) { dfree(ctx, coef); dfree(ctx, hist); return -1; }
    if (hipMemcpy(coef, coef_host, (size_t)L * T * 4, hipMemcpyHostToDevice) != hipSuccess) {
        dfree(ctx, coef); dfree(ctx, hist);
        return fail(ctx, "vv_resampler_set: the coefficient upload failed");
    }
    r.L = L; r.M = M; r.T = T; r.n_streams = n_streams; r.coef = coef; r.hist = hist;
    r.total.assign(n_streams, 0); r.flushed.assign(n_streams, 0);
    return 0;
}

extern "C" int vv_resampler_reset(vv_ctx* ctx, void* stream, int rs, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Resampler* r = rs >= 0 && rs < vv_ctx::N_RESAMPLERS && ctx->rs[rs].coef ? &ctx->rs[rs] : nullptr;
    return stage_reset(ctx, "vv_resampler_reset", r, rs, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_resample_reset_launch(r->hist, r->T, r->n_streams, ids, k, (hipStream_t)stream); }, [](int) {});
}

extern "C" int vv_resample_rows(vv_ctx* ctx, void* stream, int rs, int n, const vv_resample_row* rows_host, const float* audio_dev, int ld_in,
                                void* out_dev, int ld_out, int out_fmt, int* n_out_host) {
    VV_SHARED;
    vv_ctx::Resampler* rp = rs >= 0 && rs < vv_ctx::N_RESAMPLERS && ctx->rs[rs].coef ? &ctx->rs[rs] : nullptr;
    const RowCheck ck{ctx, "vv_resample_rows", rp, audio_dev, ld_in};
    VVTRY(ck.head(rs, n, rows_host, out_dev, n_out_host, out_fmt));
    vv_ctx::Resampler& r = *rp;
    VVRsRows kr;
    memset(&kr, 0, sizeof(kr));
    int max_in = 0;
    for (int i = 0; i < n; ++i) {
        const vv_resample_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        VVTRY(ck.input(i, q.n_in));
        VVTRY(ck.open(q.stream));
        const int64_t before = r.total[q.stream], after = before + q.n_in;
        const int64_t m0 = rs_emitted(before, r.L, r.M, r.T);
        const int64_t m1 = q.flush ? (after * r.L + r.M - 1) / r.M : rs_emitted(after, r.L, r.M, r.T);
        const int64_t n_out = m1 - m0;
        if (n_out > ld_out) return fail(ctx, "vv_resample_rows: row %d emits %lld samples, the output rows hold %d", i, (long long)n_out, ld_out);
        if (n_out > VV_RS_MAX_OUT) return fail(ctx, "vv_resample_rows: row %d emits %lld samples, one push emits at most %d per row", i, (long long)n_out, VV_RS_MAX_OUT);
        const int64_t k0 = m0 * r.M + (r.L * r.T - 2) / 2;
        kr.r[i].stream = q.stream; kr.r[i].n_in = q.n_in; kr.r[i].n_out = (int)n_out;
        kr.r[i].p0 = (int)(k0 % r.L); kr.r[i].b0 = (int)(k0 / r.L - before + r.T);
        max_in = std::max(max_in, q.n_in);
    }
    if (vv_resample_lds_bytes(r.L, r.T, max_in) > 65536 - 64)
        return fail(ctx, "vv_resample_rows: a chunk of %d samples does not fit the kernel's LDS beside the %d x %d table; push at most %d at a time",
                    max_in, r.L, r.T, (65536 - 64) / 4 - r.L * (r.T + 1) - r.T - r.T / 2);
    return stage_launch(ctx, r, rows_host, n, kr, n_out_host, [&] {
        return vv_resample_rows_launch(&kr, n, r.L, r.M, r.T, r.coef, r.hist, r.n_streams, audio_dev, ld_in, out_dev, ld_out, out_fmt, (hipStream_t)stream); });
}

extern "C" int vv_resample_once(vv_ctx* ctx, void* stream, int L, int M, int T, const float* coef_dev, int n, int n_in, const float* audio_dev,
                                int ld_in, float* out_dev, int ld_out) {
    VV_SHARED;
    if (L < 1 || L > 4096 || M < 1 || M > 4096 || T < 2 || (T & 1) || T > 4096) return fail(ctx, "vv_resample_once: L = %d, M = %d in [1,4096], T = %d even in [2,4096]", L, M, T);
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_resample_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    const int64_t n_out = ((int64_t)n_in * L + M - 1) / M;
    if (n_out > ld_out || n_out >= ((int64_t)1 << 31) - 256) return fail(ctx, "vv_resample_once: %lld output samples per row, the output rows hold %d", (long long)n_out, ld_out);
    if (!coef_dev || !audio_dev || !out_dev) return fail(ctx, "vv_resample_once: null coef / audio / out pointer");
    VVCHK(vv_resample_once_launch(L, M, T, coef_dev, n, n_in, audio_dev, ld_in, out_dev, ld_out, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------ speaking rate (kernels: tempo.hip; vibevoice_amd/tempo.py defines it)
static int64_t tp_a(int64_t k, int P, int Q) { return k < 0 ? -(int64_t)VV_TP_HS : (k * VV_TP_HS * P) / Q; }

// Blocks a stream has emitted before its flush once `total` input samples have arrived: every k with
// max(a_k, a_{k-1} + HS) + DELTA + N <= total.  vibevoice_amd/tempo.py (emitted_blocks) is the same arithmetic.
static int64_t tp_emitted(int64_t total, int P, int Q) {
    const int64_t room = total - VV_TP_DELTA - VV_TP_N;
    if (room < 0) return 0;
    int64_t k = ((room + 1) * Q) / ((int64_t)VV_TP_HS * P) + 1;
    while (k > 0 && std::max(tp_a(k - 1, P, Q), tp_a(k - 2, P, Q) + VV_TP_HS) > room) --k;
    return k;
}

static bool tp_speed_ok(int P, int Q) { return P >= 1 && Q >= 1 && Q <= 100 && P <= 2 * Q && Q <= 2 * P; }

extern "C" int vv_tempo_set(vv_ctx* ctx, int tp, const float* window_host, int n_streams, void* stream) {
    VV_SHARED;
    if (tp < 0 || tp >= vv_ctx::N_TEMPOS) return fail(ctx, "vv_tempo_set: configuration %d out of range [0,%d)", tp, vv_ctx::N_TEMPOS);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_tempo_set: n_streams = %d must be in [1,65536]", n_streams);
    if (!window_host) return fail(ctx, "vv_tempo_set: null window table");
    vv_ctx::Tempo& t = ctx->tp[tp];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, t.window); dfree(ctx, t.hist); dfree(ctx, t.dstate);
    t = vv_ctx::Tempo();
    float* window = (float*)dalloc(ctx, (size_t)VV_TP_N * 4, false);
    float* hist = (float*)dalloc(ctx, (size_t)n_streams * VV_TP_HIST * 4, true);
    int* dstate = (int*)dalloc(ctx, (size_t)n_streams * 4, true);
    if (!window || !hist || !dstate || hipMemcpy(window, window_host, (size_t)VV_TP_N * 4, hipMemcpyHostToDevice) != hipSuccess) {
        dfree(ctx, window); dfree(ctx, hist); dfree(ctx, dstate);
        return fail(ctx, "vv_tempo_set: allocating the state or uploading the window failed");
    }
    t.n_streams = n_streams; t.window = window; t.hist = hist; t.dstate = dstate;
    t.total.assign(n_streams, 0); t.P.assign(n_streams, 0); t.Q.assign(n_streams, 0); t.flushed.assign(n_streams, 0);
    return 0;
}

extern "C" int vv_tempo_reset(vv_ctx* ctx, void* stream, int tp, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Tempo* t = tp >= 0 && tp < vv_ctx::N_TEMPOS && ctx->tp[tp].hist ? &ctx->tp[tp] : nullptr;
    return stage_reset(ctx, "vv_tempo_reset", t, tp, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_tempo_reset_launch(t->hist, t->dstate, t->n_streams, ids, k, (hipStream_t)stream); },
                       [&](int id) { t->P[id] = 0; t->Q[id] = 0; });
}

extern "C" int vv_tempo_rows(vv_ctx* ctx, void* stream, int tp, int n, const vv_tempo_row* rows_host, const float* audio_dev, int ld_in,
                             void* out_dev, int ld_out, int out_fmt, int* n_out_host, int* offsets_dev, int ld_off) {
    VV_SHARED;
    vv_ctx::Tempo* t_ = tp >= 0 && tp < vv_ctx::N_TEMPOS && ctx->tp[tp].hist ? &ctx->tp[tp] : nullptr;
    const RowCheck ck{ctx, "vv_tempo_rows", t_, audio_dev, ld_in};
    VVTRY(ck.head(tp, n, rows_host, out_dev, n_out_host, out_fmt));
    vv_ctx::Tempo& t = *t_;
    VVTpRows kr;
    memset(&kr, 0, sizeof(kr));
    for (int i = 0; i < n; ++i) {
        const vv_tempo_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        if (q.n_in > VV_TP_MAX_IN) {
            fail(ctx, "vv_tempo_rows: row %d brings %d samples, one push takes at most %d per row; split it", i, q.n_in, VV_TP_MAX_IN);
            return VV_TEMPO_OVER_CAPACITY;
        }
        VVTRY(ck.input(i, q.n_in));
        if (!tp_speed_ok(q.P, q.Q)) return fail(ctx, "vv_tempo_rows: row %d: speed %d / %d must lie in [1/2, 2] with a denominator of at most 100", i, q.P, q.Q);
        if (t.P[q.stream] && (t.P[q.stream] != q.P || t.Q[q.stream] != q.Q))
            return fail(ctx, "vv_tempo_rows: stream %d runs at speed %d / %d since its first push; reset it before it changes to %d / %d", q.stream,
                        t.P[q.stream], t.Q[q.stream], q.P, q.Q);
        VVTRY(ck.open(q.stream));
        const int64_t before = t.total[q.stream], after = before + q.n_in;
        const int64_t k0 = tp_emitted(before, q.P, q.Q), total = (after * q.Q + q.P - 1) / q.P;
        const int64_t k1 = q.flush ? (total + VV_TP_HS - 1) / VV_TP_HS : tp_emitted(after, q.P, q.Q);
        const int64_t n_out = q.flush ? total - k0 * VV_TP_HS : (k1 - k0) * VV_TP_HS;
        if (n_out > ld_out || k1 - k0 > VV_TP_MAX_BLOCKS) {
            fail(ctx, "vv_tempo_rows: row %d emits %lld samples in %lld blocks, the output rows hold %d and one push walks at most %d blocks; split it", i,
                 (long long)n_out, (long long)(k1 - k0), ld_out, VV_TP_MAX_BLOCKS);
            return VV_TEMPO_OVER_CAPACITY;
        }
        if (offsets_dev && k1 - k0 > ld_off) return fail(ctx, "vv_tempo_rows: row %d walks %lld blocks, the offset rows hold %d", i, (long long)(k1 - k0), ld_off);
        kr.r[i].k0 = k0; kr.r[i].base = before - VV_TP_HIST; kr.r[i].stream = q.stream; kr.r[i].n_in = q.n_in;
        kr.r[i].nblk = (int)(k1 - k0); kr.r[i].n_out = (int)n_out; kr.r[i].P = q.P; kr.r[i].Q = q.Q;
    }
    VVTRY(stage_launch(ctx, t, rows_host, n, kr, n_out_host, [&] {
        return vv_tempo_rows_launch(&kr, n, t.window, t.hist, t.dstate, t.n_streams, audio_dev, ld_in, out_dev, ld_out, out_fmt, offsets_dev, ld_off,
                                    (hipStream_t)stream); }));
    for (int i = 0; i < n; ++i) { t.P[rows_host[i].stream] = rows_host[i].P; t.Q[rows_host[i].stream] = rows_host[i].Q; }
    return 0;
}

extern "C" int vv_tempo_once(vv_ctx* ctx, void* stream, const float* window_dev, int P, int Q, int n, int n_in, const float* audio_dev, int ld_in,
                             float* out_dev, int ld_out, int* offsets_dev, int ld_off) {
    VV_SHARED;
    if (!tp_speed_ok(P, Q)) return fail(ctx, "vv_tempo_once: speed %d / %d must lie in [1/2, 2] with a denominator of at most 100", P, Q);
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_tempo_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    const int64_t total = ((int64_t)n_in * Q + P - 1) / P;
    if (total > ld_out) return fail(ctx, "vv_tempo_once: %lld output samples per row, the output rows hold %d", (long long)total, ld_out);
    if (offsets_dev && (total + VV_TP_HS - 1) / VV_TP_HS > ld_off)
        return fail(ctx, "vv_tempo_once: %lld blocks per row, the offset rows hold %d", (long long)((total + VV_TP_HS - 1) / VV_TP_HS), ld_off);
    if (!window_dev || !audio_dev || !out_dev) return fail(ctx, "vv_tempo_once: null window / audio / out pointer");
    VVCHK(vv_tempo_once_launch(window_dev, P, Q, n, n_in, audio_dev, ld_in, out_dev, ld_out, offsets_dev, ld_off, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------ pitch (kernels: pitch.hip; vibevoice_amd/pitch.py defines it)
// Outputs a stream has emitted before its flush once `total` input samples have arrived: every m whose newest input sample, index
// (m * P) / Q + Tn, is below total.  vibevoice_amd/pitch.py (emitted) is the same arithmetic.
static int64_t pt_emitted(int64_t total, int P, int Q) {
    const int64_t room = total - vv_pt_taps(P, Q);
    return room <= 0 ? 0 : (room * Q - 1) / P + 1;
}

extern "C" int vv_pitch_set(vv_ctx* ctx, int pt, const float* table_host, int n_table, int R, int n_streams, void* stream) {
    VV_SHARED;
    if (pt < 0 || pt >= vv_ctx::N_PITCHES) return fail(ctx, "vv_pitch_set: configuration %d out of range [0,%d)", pt, vv_ctx::N_PITCHES);
    if (R < 1 || R > VV_PT_MAX_R || n_table != VV_PT_Z * R + 1)
        return fail(ctx, "vv_pitch_set: R = %d must be in [1,%d] and n_table = %d must be %d * R + 1", R, VV_PT_MAX_R, n_table, VV_PT_Z);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_pitch_set: n_streams = %d must be in [1,65536]", n_streams);
    if (!table_host) return fail(ctx, "vv_pitch_set: null prototype table");
    vv_ctx::Pitch& p = ctx->pt[pt];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, p.table); dfree(ctx, p.hist);
    p = vv_ctx::Pitch();
    float* table = (float*)dalloc(ctx, (size_t)n_table * 4, false);
    float* hist = (float*)dalloc(ctx, (size_t)n_streams * VV_PT_HIST * 4, true);
    if (!table || !hist || hipMemcpy(table, table_host, (size_t)n_table * 4, hipMemcpyHostToDevice) != hipSuccess) {
        dfree(ctx, table); dfree(ctx, hist);
        return fail(ctx, "vv_pitch_set: allocating the state or uploading the table failed");
    }
    p.R = R; p.n_streams = n_streams; p.table = table; p.hist = hist;
    p.total.assign(n_streams, 0); p.P.assign(n_streams, 0); p.Q.assign(n_streams, 0); p.flushed.assign(n_streams, 0);
    return 0;
}

extern "C" int vv_pitch_reset(vv_ctx* ctx, void* stream, int pt, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Pitch* p = pt >= 0 && pt < vv_ctx::N_PITCHES && ctx->pt[pt].hist ? &ctx->pt[pt] : nullptr;
    return stage_reset(ctx, "vv_pitch_reset", p, pt, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_pitch_reset_launch(p->hist, p->n_streams, ids, k, (hipStream_t)stream); },
                       [&](int id) { p->P[id] = 0; p->Q[id] = 0; });
}

extern "C" int vv_pitch_rows(vv_ctx* ctx, void* stream, int pt, int n, const vv_pitch_row* rows_host, const float* audio_dev, int ld_in,
                             void* out_dev, int ld_out, int out_fmt, int* n_out_host) {
    VV_SHARED;
    vv_ctx::Pitch* pp = pt >= 0 && pt < vv_ctx::N_PITCHES && ctx->pt[pt].hist ? &ctx->pt[pt] : nullptr;
    const RowCheck ck{ctx, "vv_pitch_rows", pp, audio_dev, ld_in};
    VVTRY(ck.head(pt, n, rows_host, out_dev, n_out_host, out_fmt));
    vv_ctx::Pitch& p = *pp;
    VVPitchRows kr;
    memset(&kr, 0, sizeof(kr));
    for (int i = 0; i < n; ++i) {
        const vv_pitch_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        VVTRY(ck.input(i, q.n_in));
        if (q.n_in > VV_PT_MAX_IN) return fail(ctx, "vv_pitch_rows: row %d brings %d samples, one push takes at most %d per row; push it in pieces", i, q.n_in, VV_PT_MAX_IN);
        if (!vv_pt_ratio_ok(q.P, q.Q))
            return fail(ctx, "vv_pitch_rows: row %d: ratio %d / %d must have both terms in [1,100] and lie in [1/2, 2]", i, q.P, q.Q);
        if (p.P[q.stream] && (p.P[q.stream] != q.P || p.Q[q.stream] != q.Q))
            return fail(ctx, "vv_pitch_rows: stream %d runs at ratio %d / %d since its first push; reset it before it changes to %d / %d", q.stream,
                        p.P[q.stream], p.Q[q.stream], q.P, q.Q);
        VVTRY(ck.open(q.stream));
        const int64_t before = p.total[q.stream], after = before + q.n_in;
        const int64_t m0 = pt_emitted(before, q.P, q.Q);
        const int64_t m1 = q.flush ? (after * q.Q + q.P - 1) / q.P : pt_emitted(after, q.P, q.Q);
        const int64_t n_out = m1 - m0;
        if (n_out > ld_out) return fail(ctx, "vv_pitch_rows: row %d emits %lld samples, the output rows hold %d", i, (long long)n_out, ld_out);
        if (n_out > VV_PT_MAX_OUT)
            return fail(ctx, "vv_pitch_rows: row %d emits %lld samples, one push emits at most %d per row; push it in pieces", i, (long long)n_out, VV_PT_MAX_OUT);
        const int64_t k0 = m0 * q.P;
        kr.r[i].stream = q.stream; kr.r[i].n_in = q.n_in; kr.r[i].n_out = (int)n_out; kr.r[i].P = q.P; kr.r[i].Q = q.Q;
        kr.r[i].a0 = (int)(k0 % q.Q); kr.r[i].b0 = (int)(k0 / q.Q - before + VV_PT_HIST);
    }
    VVTRY(stage_launch(ctx, p, rows_host, n, kr, n_out_host, [&] {
        return vv_pitch_rows_launch(&kr, n, p.table, p.R, p.hist, p.n_streams, audio_dev, ld_in, out_dev, ld_out, out_fmt, (hipStream_t)stream); }));
    for (int i = 0; i < n; ++i) { p.P[rows_host[i].stream] = rows_host[i].P; p.Q[rows_host[i].stream] = rows_host[i].Q; }
    return 0;
}

extern "C" int vv_pitch_once(vv_ctx* ctx, void* stream, const float* table_dev, int n_table, int R, int n, const int* pq_host, int n_in,
                             const float* audio_dev, int ld_in, float* out_dev, int ld_out) {
    VV_SHARED;
    if (R < 1 || R > VV_PT_MAX_R || n_table != VV_PT_Z * R + 1)
        return fail(ctx, "vv_pitch_once: R = %d must be in [1,%d] and n_table = %d must be %d * R + 1", R, VV_PT_MAX_R, n_table, VV_PT_Z);
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_pitch_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    if (!table_dev || !pq_host || !audio_dev || !out_dev) return fail(ctx, "vv_pitch_once: null table / ratios / audio / out pointer");
    for (int i = 0; i < n; ++i) {
        const int P = pq_host[2 * i], Q = pq_host[2 * i + 1];
        if (!vv_pt_ratio_ok(P, Q)) return fail(ctx, "vv_pitch_once: signal %d: ratio %d / %d must have both terms in [1,100] and lie in [1/2, 2]", i, P, Q);
        const int64_t n_out = ((int64_t)n_in * Q + P - 1) / P;
        if (n_out > ld_out || n_out >= ((int64_t)1 << 31) - 256)
            return fail(ctx, "vv_pitch_once: signal %d: %lld output samples, the output rows hold %d", i, (long long)n_out, ld_out);
    }
    for (int i0 = 0; i0 < n; i0 += 16) {
        const int k = std::min(16, n - i0);
        VVPitchRatios a;
        for (int i = 0; i < 16; ++i) { a.P[i] = pq_host[2 * (i0 + (i < k ? i : 0))]; a.Q[i] = pq_host[2 * (i0 + (i < k ? i : 0)) + 1]; }
        VVCHK(vv_pitch_once_launch(table_dev, R, &a, k, n_in, audio_dev + (size_t)i0 * ld_in, ld_in, out_dev + (size_t)i0 * ld_out, ld_out, (hipStream_t)stream));
    }
    return 0;
}

// ------------------------------------------------------------------ formants (kernels: formant.hip; vibevoice_amd/formant.py defines it)
static const char* const FM_RATIO_MSG = "must have both terms in [1,10000] and lie in [1/2, 2]";

extern "C" int vv_formant_set(vv_ctx* ctx, int fm, const float* twiddles_host, int n_streams, void* stream) {
    VV_SHARED;
    if (fm < 0 || fm >= vv_ctx::N_FORMANTS) return fail(ctx, "vv_formant_set: configuration %d out of range [0,%d)", fm, vv_ctx::N_FORMANTS);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_formant_set: n_streams = %d must be in [1,65536]", n_streams);
    if (!twiddles_host) return fail(ctx, "vv_formant_set: null twiddle table");
    vv_ctx::Formant& f = ctx->fm[fm];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, f.tw); dfree(ctx, f.hist); dfree(ctx, f.tail); dfree(ctx, f.scratch);
    f = vv_ctx::Formant();
    float* tw = (float*)dalloc(ctx, (size_t)2 * VV_FM_N * 4, false);
    float* hist = (float*)dalloc(ctx, (size_t)n_streams * VV_FM_HIST * 4, true);
    float* tail = (float*)dalloc(ctx, (size_t)n_streams * VV_FM_TAIL * 4, true);
    float* scratch = (float*)dalloc(ctx, (size_t)16 * VV_FM_MAX_FRAMES * VV_FM_N * 4, false);
    if (!tw || !hist || !tail || !scratch || hipMemcpy(tw, twiddles_host, (size_t)2 * VV_FM_N * 4, hipMemcpyHostToDevice) != hipSuccess) {
        dfree(ctx, tw); dfree(ctx, hist); dfree(ctx, tail); dfree(ctx, scratch);
        return fail(ctx, "vv_formant_set: allocating the state or uploading the table failed");
    }
    f.n_streams = n_streams; f.tw = tw; f.hist = hist; f.tail = tail; f.scratch = scratch;
    f.total.assign(n_streams, 0); f.A.assign(n_streams, 0); f.B.assign(n_streams, 0); f.flushed.assign(n_streams, 0);
    return 0;
}

extern "C" int vv_formant_reset(vv_ctx* ctx, void* stream, int fm, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Formant* f = fm >= 0 && fm < vv_ctx::N_FORMANTS && ctx->fm[fm].hist ? &ctx->fm[fm] : nullptr;
    return stage_reset(ctx, "vv_formant_reset", f, fm, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_formant_reset_launch(f->hist, f->tail, f->n_streams, ids, k, (hipStream_t)stream); },
                       [&](int id) { f->A[id] = 0; f->B[id] = 0; });
}

extern "C" int vv_formant_rows(vv_ctx* ctx, void* stream, int fm, int n, const vv_formant_row* rows_host, const float* audio_dev, int ld_in,
                               void* out_dev, int ld_out, int out_fmt, int* n_out_host) {
    VV_SHARED;
    vv_ctx::Formant* fp = fm >= 0 && fm < vv_ctx::N_FORMANTS && ctx->fm[fm].hist ? &ctx->fm[fm] : nullptr;
    const RowCheck ck{ctx, "vv_formant_rows", fp, audio_dev, ld_in};
    VVTRY(ck.head(fm, n, rows_host, out_dev, n_out_host, out_fmt));
    if (out_fmt != 0) return fail(ctx, "vv_formant_rows: out_fmt = 1 (int16) is not served: the warp is never the last stage, a level stage follows it");
    vv_ctx::Formant& f = *fp;
    VVFmRows kr;
    memset(&kr, 0, sizeof(kr));
    for (int i = 0; i < n; ++i) {
        const vv_formant_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        VVTRY(ck.input(i, q.n_in));
        if (q.n_in > VV_FM_MAX_IN) return fail(ctx, "vv_formant_rows: row %d brings %d samples, one push takes at most %d per row; push it in pieces", i, q.n_in, VV_FM_MAX_IN);
        if (!vv_fm_ratio_ok(q.A, q.B)) return fail(ctx, "vv_formant_rows: row %d: warp %d / %d %s", i, q.A, q.B, FM_RATIO_MSG);
        if (f.A[q.stream] && (f.A[q.stream] != q.A || f.B[q.stream] != q.B))
            return fail(ctx, "vv_formant_rows: stream %d runs at warp %d / %d since its first push; reset it before it changes to %d / %d", q.stream,
                        f.A[q.stream], f.B[q.stream], q.A, q.B);
        VVTRY(ck.open(q.stream));
        const int64_t before = f.total[q.stream], after = before + q.n_in;
        int64_t n_out = q.n_in, nf = 0, F0 = 3;                 // 1 / 1: the identity, nothing held back
        if (q.A != q.B) {
            F0 = before / VV_FM_H;
            const int64_t F1 = q.flush ? (after + VV_FM_H - 1) / VV_FM_H + 3 : after / VV_FM_H;
            nf = F1 - F0;
            n_out = (q.flush ? after : VV_FM_H * std::max<int64_t>(0, F1 - 3)) - VV_FM_H * std::max<int64_t>(0, F0 - 3);
        }
        if (n_out > ld_out) return fail(ctx, "vv_formant_rows: row %d emits %lld samples, the output rows hold %d", i, (long long)n_out, ld_out);
        kr.r[i].stream = q.stream; kr.r[i].n_in = q.n_in; kr.r[i].n_out = (int)n_out; kr.r[i].A = q.A; kr.r[i].B = q.B;
        kr.r[i].nf = (int)nf; kr.r[i].r = q.A != q.B ? (int)(before % VV_FM_H) : 0; kr.r[i].c_min = (int)std::max<int64_t>(0, 3 - F0);
    }
    VVTRY(stage_launch(ctx, f, rows_host, n, kr, n_out_host, [&] {
        return vv_formant_rows_launch(&kr, n, f.tw, f.hist, f.tail, f.n_streams, audio_dev, ld_in, (float*)out_dev, ld_out, f.scratch, VV_FM_MAX_FRAMES,
                                      (hipStream_t)stream); }));
    for (int i = 0; i < n; ++i) { f.A[rows_host[i].stream] = rows_host[i].A; f.B[rows_host[i].stream] = rows_host[i].B; }
    return 0;
}

extern "C" int vv_formant_once(vv_ctx* ctx, void* stream, const float* twiddles_dev, int n, const int* ab_host, int n_in, const float* audio_dev,
                               int ld_in, float* out_dev, int ld_out, float* scratch_dev, long long scratch_floats) {
    VV_SHARED;
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in || n_in > ((int64_t)1 << 31) - 4 * VV_FM_N)
        return fail(ctx, "vv_formant_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    if (n_in > ld_out) return fail(ctx, "vv_formant_once: %d output samples per row, the output rows hold %d", n_in, ld_out);
    if (!twiddles_dev || !ab_host || !audio_dev || !out_dev || !scratch_dev) return fail(ctx, "vv_formant_once: null table / fractions / audio / out / scratch pointer");
    const int nf = (n_in + VV_FM_H - 1) / VV_FM_H + 3;
    if ((int64_t)std::min(n, 16) * nf * VV_FM_N > scratch_floats)
        return fail(ctx, "vv_formant_once: the frames of %d signals of %d samples need %lld floats of scratch, %lld are given", std::min(n, 16), n_in,
                    (long long)std::min(n, 16) * nf * VV_FM_N, scratch_floats);
    for (int i = 0; i < n; ++i)
        if (!vv_fm_ratio_ok(ab_host[2 * i], ab_host[2 * i + 1]))
            return fail(ctx, "vv_formant_once: signal %d: warp %d / %d %s", i, ab_host[2 * i], ab_host[2 * i + 1], FM_RATIO_MSG);
    for (int i0 = 0; i0 < n; i0 += 16) {
        const int k = std::min(16, n - i0);
        VVFmRows kr;
        memset(&kr, 0, sizeof(kr));
        for (int i = 0; i < k; ++i) {
            const int A = ab_host[2 * (i0 + i)], B = ab_host[2 * (i0 + i) + 1];
            kr.r[i].stream = -1; kr.r[i].n_in = n_in; kr.r[i].n_out = n_in; kr.r[i].A = A; kr.r[i].B = B;
            kr.r[i].nf = A == B ? 0 : nf; kr.r[i].r = 0; kr.r[i].c_min = 3;
        }
        VVCHK(vv_formant_rows_launch(&kr, k, twiddles_dev, nullptr, nullptr, 0, audio_dev + (size_t)i0 * ld_in, ld_in, out_dev + (size_t)i0 * ld_out, ld_out,
                                     scratch_dev, nf, (hipStream_t)stream));
    }
    return 0;
}

// ------------------------------------------------------------------ output level (kernels: level.hip; vibevoice_amd/level.py defines it)
// Outputs a stream has emitted before its flush once `total` input samples have arrived: every sample whose A - 1 samples of look-ahead
// are there.  vibevoice_amd/level.py (emitted) is the same arithmetic.
static int64_t lv_emitted(int64_t total, int A) { return std::max<int64_t>(0, total - (A - 1)); }

static bool lv_params_ok(int A, int H, float c) {
    return A >= 1 && A <= VV_LV_MAX_A && H >= 0 && (int64_t)H + 3 * (int64_t)A - 3 < VV_LV_BUF && c > 0.f && c <= 1.0f;
}
static bool lv_gain_ok(float g) { return g > 0.f && g <= 16.0f; }       // a NaN compares false

extern "C" int vv_level_set(vv_ctx* ctx, int lv, int A, int H, float ceiling, int n_streams, void* stream) {
    VV_SHARED;
    if (lv < 0 || lv >= vv_ctx::N_LEVELS) return fail(ctx, "vv_level_set: configuration %d out of range [0,%d)", lv, vv_ctx::N_LEVELS);
    if (!lv_params_ok(A, H, ceiling))
        return fail(ctx, "vv_level_set: A = %d must be in [1,%d], H = %d >= 0 with H + 3 A - 3 < %d, ceiling = %g in (0,1]", A, VV_LV_MAX_A, H, VV_LV_BUF,
                    (double)ceiling);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_level_set: n_streams = %d must be in [1,65536]", n_streams);
    vv_ctx::Level& l = ctx->lv[lv];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, l.hist);
    l = vv_ctx::Level();
    // one word more than the rows: a configuration with H + 2 A - 2 = 0 still holds a buffer, which marks it as set
    float* hist = (float*)dalloc(ctx, ((size_t)n_streams * (H + 2 * A - 2) + 1) * 4, true);
    if (!hist) return -1;
    l.A = A; l.H = H; l.c = ceiling; l.n_streams = n_streams; l.hist = hist;
    l.total.assign(n_streams, 0); l.flushed.assign(n_streams, 0); l.gain.assign(n_streams, 0.f);
    return 0;
}

extern "C" int vv_level_reset(vv_ctx* ctx, void* stream, int lv, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Level* l = lv >= 0 && lv < vv_ctx::N_LEVELS && ctx->lv[lv].hist ? &ctx->lv[lv] : nullptr;
    return stage_reset(ctx, "vv_level_reset", l, lv, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_level_reset_launch(l->hist, l->H + 2 * l->A - 2, l->n_streams, ids, k, (hipStream_t)stream); },
                       [&](int id) { l->gain[id] = 0.f; });
}

extern "C" int vv_level_rows(vv_ctx* ctx, void* stream, int lv, int n, const vv_level_row* rows_host, const float* audio_dev, int ld_in,
                             void* out_dev, int ld_out, int out_fmt, int* n_out_host) {
    VV_SHARED;
    vv_ctx::Level* lp = lv >= 0 && lv < vv_ctx::N_LEVELS && ctx->lv[lv].hist ? &ctx->lv[lv] : nullptr;
    const RowCheck ck{ctx, "vv_level_rows", lp, audio_dev, ld_in};
    VVTRY(ck.head(lv, n, rows_host, out_dev, n_out_host, out_fmt));
    vv_ctx::Level& l = *lp;
    const int nh = l.H + 2 * l.A - 2, max_in = VV_LV_BUF - nh - (l.A - 1);
    VVLvRows kr;
    memset(&kr, 0, sizeof(kr));
    for (int i = 0; i < n; ++i) {
        const vv_level_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        VVTRY(ck.input(i, q.n_in));
        if (q.n_in > max_in) return fail(ctx, "vv_level_rows: row %d brings %d samples, one push takes at most %d per row; push it in pieces", i, q.n_in, max_in);
        if (!lv_gain_ok(q.gain)) return fail(ctx, "vv_level_rows: row %d: gain %g must lie in (0,16]", i, (double)q.gain);
        if (l.gain[q.stream] != 0.f && l.gain[q.stream] != q.gain)
            return fail(ctx, "vv_level_rows: stream %d runs at gain %g since its first push; reset it before it changes to %g", q.stream,
                        (double)l.gain[q.stream], (double)q.gain);
        VVTRY(ck.open(q.stream));
        const int64_t before = l.total[q.stream], after = before + q.n_in;
        const int64_t o0 = lv_emitted(before, l.A), o1 = q.flush ? after : lv_emitted(after, l.A);
        const int64_t n_out = o1 - o0;
        if (n_out > ld_out) return fail(ctx, "vv_level_rows: row %d emits %lld samples, the output rows hold %d", i, (long long)n_out, ld_out);
        kr.r[i].stream = q.stream; kr.r[i].n_in = q.n_in; kr.r[i].n_out = (int)n_out; kr.r[i].b0 = (int)(o0 - before + nh); kr.r[i].gain = q.gain;
    }
    VVTRY(stage_launch(ctx, l, rows_host, n, kr, n_out_host, [&] {
        return vv_level_rows_launch(&kr, n, l.A, l.H, l.c, l.hist, l.n_streams, audio_dev, ld_in, out_dev, ld_out, out_fmt, (hipStream_t)stream); }));
    for (int i = 0; i < n; ++i) l.gain[rows_host[i].stream] = rows_host[i].gain;
    return 0;
}

extern "C" int vv_level_once(vv_ctx* ctx, void* stream, int A, int H, float gain, float ceiling, int n, int n_in, const float* audio_dev, int ld_in,
                             float* out_dev, int ld_out) {
    VV_SHARED;
    if (!lv_params_ok(A, H, ceiling))
        return fail(ctx, "vv_level_once: A = %d must be in [1,%d], H = %d >= 0 with H + 3 A - 3 < %d, ceiling = %g in (0,1]", A, VV_LV_MAX_A, H, VV_LV_BUF,
                    (double)ceiling);
    if (!lv_gain_ok(gain)) return fail(ctx, "vv_level_once: gain %g must lie in (0,16]", (double)gain);
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_level_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    if (n_in > ld_out) return fail(ctx, "vv_level_once: %d output samples per row, the output rows hold %d", n_in, ld_out);
    if (!audio_dev || !out_dev) return fail(ctx, "vv_level_once: null audio / out pointer");
    VVCHK(vv_level_once_launch(A, H, gain, ceiling, n, n_in, audio_dev, ld_in, out_dev, ld_out, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------ loudness (kernels: loudness.hip; vibevoice_amd/loudness.py defines it)
// The leveller holds nothing back: a push emits as many samples as it brings, the flush none.
extern "C" int vv_loud_set(vv_ctx* ctx, int ld, const int* taps_host, int n_streams, void* stream) {
    VV_SHARED;
    if (ld < 0 || ld >= vv_ctx::N_LOUDS) return fail(ctx, "vv_loud_set: configuration %d out of range [0,%d)", ld, vv_ctx::N_LOUDS);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_loud_set: n_streams = %d must be in [1,65536]", n_streams);
    if (!taps_host) return fail(ctx, "vv_loud_set: null tap table");
    std::vector<double> h(VV_LD_T);
    double sum = 0.0;
    for (int k = 0; k < VV_LD_T; ++k) { h[k] = (double)taps_host[k]; sum += std::fabs(h[k]); }
    // |z| <= 2^23 sum |hq| must stay below 2^53 for the fp64 sums to be exact; the K-weighting's is 3.25 2^24
    if (sum >= 1073741824.0) return fail(ctx, "vv_loud_set: the taps' absolute sum %.0f must stay below 2^30", sum);
    vv_ctx::Loud& l = ctx->loud[ld];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, l.taps); dfree(ctx, l.hist); dfree(ctx, l.state); dfree(ctx, l.part);
    l = vv_ctx::Loud();
    double* taps = (double*)dalloc(ctx, (size_t)VV_LD_T * 8, false);
    int* hist = (int*)dalloc(ctx, (size_t)n_streams * VV_LD_T * 4, true);
    VVLdState* state = (VVLdState*)dalloc(ctx, (size_t)n_streams * sizeof(VVLdState), true);
    long long* part = (long long*)dalloc(ctx, (size_t)n_streams * VV_LD_MAX_TILES * 2 * 8, true);
    if (!taps || !hist || !state || !part || hipMemcpy(taps, h.data(), (size_t)VV_LD_T * 8, hipMemcpyHostToDevice) != hipSuccess) {
        dfree(ctx, taps); dfree(ctx, hist); dfree(ctx, state); dfree(ctx, part);
        return fail(ctx, "vv_loud_set: allocating the state or uploading the taps failed");
    }
    l.n_streams = n_streams; l.taps = taps; l.hist = hist; l.state = state; l.part = part;
    l.total.assign(n_streams, 0); l.flushed.assign(n_streams, 0);
    l.t.assign(n_streams, 0.f); l.g0.assign(n_streams, 0.f); l.wmax.assign(n_streams, 0.f);
    return 0;
}

extern "C" int vv_loud_reset(vv_ctx* ctx, void* stream, int ld, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Loud* l = ld >= 0 && ld < vv_ctx::N_LOUDS && ctx->loud[ld].hist ? &ctx->loud[ld] : nullptr;
    return stage_reset(ctx, "vv_loud_reset", l, ld, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_loud_reset_launch(l->hist, l->state, l->n_streams, ids, k, (hipStream_t)stream); },
                       [&](int id) { l->t[id] = 0.f; l->g0[id] = 0.f; l->wmax[id] = 0.f; });
}

extern "C" int vv_loud_rows(vv_ctx* ctx, void* stream, int ld, int n, const vv_loud_row* rows_host, const float* audio_dev, int ld_in,
                            void* out_dev, int ld_out, int out_fmt, int* n_out_host) {
    VV_SHARED;
    vv_ctx::Loud* lp = ld >= 0 && ld < vv_ctx::N_LOUDS && ctx->loud[ld].hist ? &ctx->loud[ld] : nullptr;
    const RowCheck ck{ctx, "vv_loud_rows", lp, audio_dev, ld_in};
    VVTRY(ck.head(ld, n, rows_host, out_dev, n_out_host, out_fmt));
    if (out_fmt != 0) return fail(ctx, "vv_loud_rows: out_fmt = 1 (int16) is not served: the leveller is never the last stage, a level stage follows it");
    vv_ctx::Loud& l = *lp;
    VVLdRows kr;
    memset(&kr, 0, sizeof(kr));
    for (int i = 0; i < n; ++i) {
        const vv_loud_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        VVTRY(ck.input(i, q.n_in));
        if (q.n_in > VV_LD_MAX_IN)
            return fail(ctx, "vv_loud_rows: row %d brings %d samples, one push takes at most %d per row; push it in pieces", i, q.n_in, VV_LD_MAX_IN);
        if (!vv_ld_params_ok(q.t, q.g0, q.wmax))
            return fail(ctx, "vv_loud_rows: row %d: t = %g must lie in (0,1), g0 = %g in (0,16], wmax = %g in [1,16]", i, (double)q.t, (double)q.g0, (double)q.wmax);
        if (l.t[q.stream] != 0.f && (l.t[q.stream] != q.t || l.g0[q.stream] != q.g0 || l.wmax[q.stream] != q.wmax))
            return fail(ctx, "vv_loud_rows: stream %d runs at t = %g, g0 = %g, wmax = %g since its first push; reset it before they change", q.stream,
                        (double)l.t[q.stream], (double)l.g0[q.stream], (double)l.wmax[q.stream]);
        VVTRY(ck.open(q.stream));
        if (q.n_in > ld_out) return fail(ctx, "vv_loud_rows: row %d emits %d samples, the output rows hold %d", i, q.n_in, ld_out);
        const int64_t before = l.total[q.stream];
        kr.r[i].stream = q.stream; kr.r[i].n_in = q.n_in; kr.r[i].n_out = q.n_in; kr.r[i].k0 = (int)(before % VV_LD_S); kr.r[i].h0 = (int)(before % VV_LD_T);
        kr.r[i].first = before == 0; kr.r[i].t = q.t; kr.r[i].g0 = q.g0; kr.r[i].wmax = q.wmax;
    }
    VVTRY(stage_launch(ctx, l, rows_host, n, kr, n_out_host, [&] {
        return vv_loud_rows_launch(&kr, n, l.taps, l.hist, l.state, l.part, l.n_streams, audio_dev, ld_in, (float*)out_dev, ld_out, (hipStream_t)stream); }));
    for (int i = 0; i < n; ++i) { l.t[rows_host[i].stream] = rows_host[i].t; l.g0[rows_host[i].stream] = rows_host[i].g0; l.wmax[rows_host[i].stream] = rows_host[i].wmax; }
    return 0;
}

extern "C" int vv_loud_energy(vv_ctx* ctx, void* stream, const double* taps_dev, int n, int n_in, const float* audio_dev, int ld_in,
                              long long* energies_dev, int ld_e, long long* fine_dev, int ld_f) {
    VV_SHARED;
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_loud_energy: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    if ((energies_dev && n_in / VV_LD_S > ld_e) || (fine_dev && n_in / VV_LD_S > ld_f))
        return fail(ctx, "vv_loud_energy: %d segments per row, the energy rows hold %d", n_in / VV_LD_S, energies_dev && n_in / VV_LD_S > ld_e ? ld_e : ld_f);
    if (!taps_dev || !audio_dev || (n_in >= VV_LD_S && !energies_dev && !fine_dev)) return fail(ctx, "vv_loud_energy: null taps / audio / energies pointer");
    VVCHK(vv_loud_energy_launch(taps_dev, n, n_in, audio_dev, ld_in, energies_dev, ld_e, fine_dev, ld_f, (hipStream_t)stream));
    return 0;
}

extern "C" int vv_loud_once(vv_ctx* ctx, void* stream, const double* taps_dev, float t, float g0, float wmax, int n, int n_in, const float* audio_dev,
                            int ld_in, float* out_dev, int ld_out, float* gain_dev, int ld_gain, long long* energies_dev, int ld_e) {
    VV_SHARED;
    if (!vv_ld_params_ok(t, g0, wmax)) return fail(ctx, "vv_loud_once: t = %g must lie in (0,1), g0 = %g in (0,16], wmax = %g in [1,16]", (double)t, (double)g0, (double)wmax);
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_loud_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    if (n_in > ld_out || (gain_dev && n_in > ld_gain)) return fail(ctx, "vv_loud_once: %d output samples per row, the output rows hold %d", n_in, gain_dev ? std::min(ld_out, ld_gain) : ld_out);
    if (n_in / VV_LD_S > ld_e) return fail(ctx, "vv_loud_once: %d segments per row, the energy rows hold %d", n_in / VV_LD_S, ld_e);
    if (!taps_dev || !audio_dev || !out_dev || (n_in >= VV_LD_S && !energies_dev)) return fail(ctx, "vv_loud_once: null taps / audio / out / energies pointer");
    VVCHK(vv_loud_once_launch(taps_dev, t, g0, wmax, n, n_in, audio_dev, ld_in, out_dev, ld_out, gain_dev, ld_gain, energies_dev, ld_e, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------ pauses (kernels: pause.hip; vibevoice_amd/pause.py defines them)
// The one stage whose counts the host does not know: what a push emits depends on the data, the kernel writes it to device memory.  The
// host still keeps each stream's input total (the open segment's samples are total % seg) and its parameters.
extern "C" int vv_pause_set(vv_ctx* ctx, int ps, int seg, const float* weights_host, int n_streams, void* stream) {
    VV_SHARED;
    if (ps < 0 || ps >= vv_ctx::N_PAUSES) return fail(ctx, "vv_pause_set: configuration %d out of range [0,%d)", ps, vv_ctx::N_PAUSES);
    if (seg < VV_PS_MIN_SEG || seg > VV_PS_MAX_SEG) return fail(ctx, "vv_pause_set: seg = %d must be in [%d,%d] (8 to 48 kHz)", seg, VV_PS_MIN_SEG, VV_PS_MAX_SEG);
    if (n_streams < 1 || n_streams > 65536) return fail(ctx, "vv_pause_set: n_streams = %d must be in [1,65536]", n_streams);
    if (!weights_host) return fail(ctx, "vv_pause_set: null weight table");
    vv_ctx::Pause& p = ctx->ps[ps];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));      // pushes that still read what is replaced
    dfree(ctx, p.wt); dfree(ctx, p.sbuf); dfree(ctx, p.state);
    p = vv_ctx::Pause();
    float* wt = (float*)dalloc(ctx, (size_t)2 * seg * 4, false);
    float* sbuf = (float*)dalloc(ctx, (size_t)n_streams * VV_PS_FLOATS * 4, true);
    VVPsState* state = (VVPsState*)dalloc(ctx, (size_t)n_streams * sizeof(VVPsState), true);
    if (!wt || !sbuf || !state || hipMemcpy(wt, weights_host, (size_t)2 * seg * 4, hipMemcpyHostToDevice) != hipSuccess) {
        dfree(ctx, wt); dfree(ctx, sbuf); dfree(ctx, state);
        return fail(ctx, "vv_pause_set: allocating the state or uploading the weights failed");
    }
    p.seg = seg; p.n_streams = n_streams; p.wt = wt; p.sbuf = sbuf; p.state = state;
    p.total.assign(n_streams, 0); p.flushed.assign(n_streams, 0);
    p.C.assign(n_streams, 0); p.C0.assign(n_streams, 0); p.theta.assign(n_streams, -1);
    return 0;
}

extern "C" int vv_pause_reset(vv_ctx* ctx, void* stream, int ps, int n, const int* stream_ids_host) {
    VV_SHARED;
    vv_ctx::Pause* p = ps >= 0 && ps < vv_ctx::N_PAUSES && ctx->ps[ps].state ? &ctx->ps[ps] : nullptr;
    return stage_reset(ctx, "vv_pause_reset", p, ps, n, stream_ids_host,
                       [&](const int* ids, int k) { return vv_pause_reset_launch(p->state, p->n_streams, ids, k, (hipStream_t)stream); },
                       [&](int id) { p->theta[id] = -1; });
}

extern "C" int vv_pause_rows(vv_ctx* ctx, void* stream, int ps, int n, const vv_pause_row* rows_host, const float* audio_dev, int ld_in,
                             void* out_dev, int ld_out, int out_fmt, int* n_out_dev) {
    VV_SHARED;
    vv_ctx::Pause* pp = ps >= 0 && ps < vv_ctx::N_PAUSES && ctx->ps[ps].state ? &ctx->ps[ps] : nullptr;
    const RowCheck ck{ctx, "vv_pause_rows", pp, audio_dev, ld_in};
    VVTRY(ck.head(ps, n, rows_host, out_dev, n_out_dev, out_fmt));
    vv_ctx::Pause& p = *pp;
    VVPsRows kr;
    memset(&kr, 0, sizeof(kr));
    for (int i = 0; i < n; ++i) {
        const vv_pause_row& q = rows_host[i];
        VVTRY(ck.stream(rows_host, i));
        VVTRY(ck.input(i, q.n_in));
        if (q.n_in > VV_PS_MAX_IN)
            return fail(ctx, "vv_pause_rows: row %d brings %d samples, one push takes at most %d per row; push it in pieces", i, q.n_in, VV_PS_MAX_IN);
        if (q.seg != p.seg) return fail(ctx, "vv_pause_rows: row %d: seg = %d, the configuration was set for %d", i, q.seg, p.seg);
        if (!vv_ps_params_ok(q.seg, q.C, q.C0, q.theta))
            return fail(ctx, "vv_pause_rows: row %d: C = %d, C0 = %d and theta = %lld must be >= 0", i, q.C, q.C0, q.theta);
        if (p.theta[q.stream] >= 0 && (p.theta[q.stream] != q.theta || p.C[q.stream] != q.C || p.C0[q.stream] != q.C0))
            return fail(ctx, "vv_pause_rows: stream %d runs at C = %d, C0 = %d, theta = %lld since its first push; reset it before they change", q.stream,
                        p.C[q.stream], p.C0[q.stream], p.theta[q.stream]);
        VVTRY(ck.open(q.stream));
        const int64_t most = (int64_t)q.n_in + (p.seg - 1) + (int64_t)VV_PS_MAX_T * p.seg;
        if (most > ld_out) return fail(ctx, "vv_pause_rows: row %d may emit %lld samples, the output rows hold %d", i, (long long)most, ld_out);
        VVPsRow& k = kr.r[i];
        k.stream = q.stream; k.n_in = q.n_in; k.flush = q.flush != 0; k.carry = (int)(p.total[q.stream] % p.seg);
        k.seg = q.seg; k.C = q.C; k.C0 = q.C0; k.theta = q.theta;
    }
    for (int i = n; i < 16; ++i) kr.r[i] = kr.r[0];
    VVCHK(vv_pause_rows_launch(&kr, n, p.seg, p.sbuf, p.state, p.n_streams, p.wt, audio_dev, ld_in, out_dev, ld_out, out_fmt, n_out_dev, (hipStream_t)stream));
    for (int i = 0; i < n; ++i) {
        const vv_pause_row& q = rows_host[i];
        p.total[q.stream] += q.n_in;
        if (q.flush) p.flushed[q.stream] = 1;
        p.C[q.stream] = q.C; p.C0[q.stream] = q.C0; p.theta[q.stream] = q.theta;
    }
    return 0;
}

extern "C" int vv_pause_totals(vv_ctx* ctx, void* stream, int ps, int n, const int* stream_ids_host, long long* totals_host) {
    VV_SHARED;
    vv_ctx::Pause* p = ps >= 0 && ps < vv_ctx::N_PAUSES && ctx->ps[ps].state ? &ctx->ps[ps] : nullptr;
    if (!p) return fail(ctx, "vv_pause_totals: configuration %d is not set", ps);
    if (n < 1 || !stream_ids_host || !totals_host) return fail(ctx, "vv_pause_totals: n = %d must be >= 1, with ids and totals", n);
    for (int i = 0; i < n; ++i)
        if (stream_ids_host[i] < 0 || stream_ids_host[i] >= p->n_streams)
            return fail(ctx, "vv_pause_totals: stream id %d out of range [0,%d)", stream_ids_host[i], p->n_streams);
    std::vector<VVPsState> h(p->n_streams);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), p->state, h.size() * sizeof(VVPsState), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < n; ++i) {
        const VVPsState& s = h[stream_ids_host[i]];
        totals_host[3 * i] = s.tin; totals_host[3 * i + 1] = s.tout; totals_host[3 * i + 2] = s.dropped;
    }
    return 0;
}

extern "C" int vv_pause_once(vv_ctx* ctx, void* stream, const float* weights_dev, int seg, int C, int C0, long long theta, int n, int n_in,
                             const float* audio_dev, int ld_in, float* out_dev, int ld_out, float* scratch_dev, long long scratch_floats,
                             int* counts_dev) {
    VV_SHARED;
    if (!vv_ps_params_ok(seg, C, C0, theta))
        return fail(ctx, "vv_pause_once: seg = %d must be in [%d,%d], C = %d, C0 = %d and theta = %lld >= 0", seg, VV_PS_MIN_SEG, VV_PS_MAX_SEG, C, C0, theta);
    if (n < 1 || n > 65535 || n_in < 1 || n_in > ld_in) return fail(ctx, "vv_pause_once: n = %d in [1,65535], n_in = %d in [1, ld_in = %d]", n, n_in, ld_in);
    if (n_in > ld_out) return fail(ctx, "vv_pause_once: up to %d output samples per row, the output rows hold %d", n_in, ld_out);
    if (!weights_dev || !audio_dev || !out_dev || !scratch_dev || !counts_dev) return fail(ctx, "vv_pause_once: null weights / audio / out / scratch / counts pointer");
    if (scratch_floats < (long long)n * VV_PS_ONCE_FLOATS)
        return fail(ctx, "vv_pause_once: the scratch holds %lld floats, %d signals need %lld", scratch_floats, n, (long long)n * VV_PS_ONCE_FLOATS);
    VVCHK(vv_pause_once_launch(seg, C, C0, theta, weights_dev, n, n_in, audio_dev, ld_in, out_dev, ld_out, scratch_dev, counts_dev, (hipStream_t)stream));
    return 0;
}
