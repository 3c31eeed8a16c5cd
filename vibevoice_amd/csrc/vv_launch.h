// vv_launch.h -- prototypes of the extern "C" launchers and _ok predicates one .hip unit defines and another calls.
// Every unit that defines one includes this header: a definition that drifts from its prototype is a compile error
// ("conflicting types"), not undefined behaviour at the call.  Internal: hidden visibility, not part of include/vvhip.h.
#pragma once
#include "vv_common.h"
#include "gemv_plan.h"       // VV_ROUTE_* and vv_gemm_route(a, xs): which kernel vv_gemm_launch runs a call on

// ---- the end of a solver step on the general path (solver.hip): CFG + table-driven DPM-Solver++ update (+ the next in-projection) ----
struct VVSolverStep {
    const float* eps;      // [2n][L] the final layer's plain output: conditional rows, then the negative ones
    const float* z_in; const float* m1_in; const float* m2_in;      // this step's state: z [2n][L] (rows < n read), previous two x0 [n][L]
    float* z_out; float* m1_out; float* m2_out;                     // the next step's state (DIFFERENT buffers)
    const float* coef;     // {a, s, cs, c0, c1, c2, cn, 0}: one 8-float row of the general table
    float cfg; const float* cfg_rows;      // one guidance scale, or [n] of them on the device (then read in place of cfg)
    const float* noise;    // [n][L] this step's variance noise (stochastic solver) or null
    int n, L;
    const u32x4* Win;      // packed [H][L] noisy_images_proj, or null: the update alone
    float* Xout;           // [2n][H] the next step's in-projection
    int H, xs;             // xs: bf16 terms per operand element (the engine's xsplit)
};
extern "C" {
int vv_gemm_launch(VVGemm a, int xs, hipStream_t s);
int vv_pack_launch(const void* src, int src_is_bf16, void* dst, int N, int K, int kind, int Cin, int Cout, int ksz, int stride, hipStream_t s);
int vv_rope_append_launch(int D, const float* qkv, const VVRow* rows, const float* inv_freq, float* q_out, void* kc, void* vc, int R, int Hq, int Hkv,
                          int64_t cache_stride, int64_t head_stride, hipStream_t s);
int vv_rope_table_launch(const float* inv_freq, void* tab, int n_pos, int half, hipStream_t s);
int vv_attn_fused_launch(int D, int xs, const float* qkv, const VVRow* rows, const void* rope_tab, void* kc, void* vc, int R, int Hq, int Hkv,
                         int64_t cache_stride, int64_t head_stride, int S, float* pm, float* pl, float* po, float* out, void* out_packed,
                         hipStream_t s);
int vv_attn_launch(int D, int xs, const float* q, const VVRow* rows, const void* kc, const void* vc, int R, int Hq, int Hkv, int64_t cache_stride,
                   int64_t head_stride, int S, float* pm, float* pl, float* po, float* out, hipStream_t s);
int vv_embed_launch(const void* table, const int* ids, float* out, int n, int H, hipStream_t s);
int vv_logits_full_launch(const void* table, const float* hidden, float* out, int n, int V, int H, hipStream_t s);
int vv_warp_valid_launch(const float* logits, const unsigned char* seen, float* out, int* survivors, int n, int V, const int* ids, int n_valid,
                         float pen, float temp, int do_sample, int top_k, float top_p, float min_p, hipStream_t s);
int vv_noise_rows_launch(float* out, int n, const uint32_t* keys, uint32_t stream0, int n_streams, int n_t, int width, hipStream_t s);
int vv_rmsnorm_rows_launch(const float* x, int ldx, float* y, int ldy, const float* w, int T, int C, float eps, hipStream_t s);
int vv_dwconv_res_launch(const float* nb, const float* x, float* xo, const float* w, const float* b, const float* gamma, int T, int C, hipStream_t s);
int vv_normdw_sliced_ok(int T, int C);
int vv_normdw_sliced_slots_launch(const float* xin, float* xout, float* nb, const float* nw, const float* w, const float* b, const float* gamma,
                                  int T, int C, float eps, const int* ids, int n, int64_t sx, int64_t snb, hipStream_t s);
int vv_normdw_rows_slots_launch(const float* xin, float* xout, float* nb, const float* nw, const float* w, const float* b, const float* gamma, int T,
                                int C, float eps, const int* ids, int n, int64_t sx, int64_t snb, hipStream_t s);
int vv_stem_conv_slots_launch(const float* in, const void* wp, const float* bias, float* out, int T, int N, const int* ids, int n, int64_t s_in,
                              int64_t s_out, hipStream_t s);
int vv_head_conv1_slots_launch(const float* x, const void* wp, const float* bias, float* out, int T, int Cin, const int* ids, int n, int64_t s_in,
                               int64_t s_out, hipStream_t s);
int vv_block1d_slots_launch(int C, int xs, const float* xin, float* xout, float* nst, const float* norm_w, const float* ffn_norm_w,
                            const float* gamma, const float* ffn_gamma, const float* dw_w, const float* dw_b, const float* b1, const float* b2,
                            const void* w1, const void* w2, int T, float eps, const int* ids, int n, int64_t sx, int64_t snst, hipStream_t s);
int vv_affine_slots_launch(const float* x, float* y, float mul, float add, int L, const int* ids, int n, int64_t stride, hipStream_t s);
int vv_normdw_launch(float* x, float* nb, const float* nw, const float* w, const float* b, const float* gamma, int T, int C, float eps,
                     hipStream_t s);
int vv_normdw_rows_ok(int T, int C);
int vv_shift_rows_launch(const void* tab, int n_entries, int maxC, hipStream_t s);
int vv_zero_hist_launch(const void* tab, int n_entries, hipStream_t s);
int vv_affine_launch(const float* x, float* y, float mul, float add, int n, hipStream_t s);
int vv_copy_launch(void* dst, const void* src, size_t bytes, hipStream_t s);
int vv_zero_launch(void* dst, size_t bytes, hipStream_t s);
int vv_sampler_init_launch(const float* noise, float* z, float* x0p, int nL, hipStream_t s);
int vv_tfreq_launch(const float* t, float* out, int n, hipStream_t s);
int vv_silu_launch(float* x, int n, hipStream_t s);
int vv_ada_in_launch(const float* cproj, const float* temb, float* out, int rows, int n_steps, int H, hipStream_t s);
int vv_add_rows_launch(const float* x, const float* v, float* y, int n, int C, hipStream_t s);
int vv_relu_launch(float* x, int n, hipStream_t s);
int vv_kv_import_launch(const void* k, const void* v, int src_bf16, void* kc, void* vc, int L, int Hkv, int D, int64_t head_stride, int pos0,
                        hipStream_t s);
int vv_kv_move_launch(void* kc, void* vc, int layers, int Hkv, int D, int64_t layer_stride, int64_t head_stride, int src, int dst, hipStream_t s);
int vv_kv_zero_v_tail_launch(void* vc, const VVRow* rows, int R, int layers, int Hkv, int D, int64_t cache_stride, int64_t layer_stride,
                             int64_t head_stride, int max_ctx, hipStream_t s);
int vv_kv_span_copy_launch(void* kc, void* vc, void* ks, void* vs, int to_cache, int layers, int Hkv, int D, int64_t layer_stride,
                           int64_t head_stride, int n_pos, hipStream_t s);
int vv_kv_export_launch(const void* kc, const void* vc, void* k, void* v, int dst_bf16, int L, int Hkv, int D, int64_t head_stride, int pos0,
                        hipStream_t s);
int vv_pcm16_launch(const float* x, short* out, int n, int samples, hipStream_t s);
int vv_cvt_launch(const void* src, void* dst, int64_t n, int to_bf16, hipStream_t s);
int vv_dw_transpose_launch(const float* src, float* dst, int C, hipStream_t s);
int vv_pack_rows_launch(const float* x, int ldx, const float* nw, float eps, void* xp, int T, int K, hipStream_t s);
int vv_unpack_rows_launch(const void* xp, float* x, int T, int K, hipStream_t s);
int vv_pack16_launch(const float* x, int ldx, int mode, const float* nw, float eps, const float* sc, const float* sh, int ld_mod, void* xp, int T,
                     int K, hipStream_t s);
int vv_gemv16p_launch(const void* W, const void* W2, const void* Xp, float* Y, void* Yp, const float* bias, const float* gate, int T, int N, int K,
                      int ldy, int ld_gate, int epi, hipStream_t s);
int vv_gemv16p_launch2(const VVGemv16p* a, int epi, int flags, hipStream_t s, int* wpb_out = nullptr);
int vv_head_tail_ok(const VVTail* a);
int vv_head_tail_init();
int vv_head_tail_launch(const VVTail* a, hipStream_t s);
int vv_solver_step_ok(const VVSolverStep* a);
int vv_solver_step_fused_ok(const VVSolverStep* a);
int vv_solver_step_launch(const VVSolverStep* a, hipStream_t s);
int vv_pack16_tiles_launch(const float* x, int ldx, int64_t stride_outer, int n_inner, int64_t stride_inner, void* xp, int64_t tile_bytes, int T,
                           int K, int n_tiles, hipStream_t s);
int vv_ada_pack_launch(const float* cproj, const float* temb, void* xp, int rows, int n_steps, int H, hipStream_t s);
int vv_gemm3_launch(const void* W, const void* W2, const void* Xp, float* Y, void* Yp, const float* bias, int T, int N, int K, int ldy, int epi,
                    const VVGemmWs* ws, hipStream_t s);
int vv_gemm_qkv_rope_launch(const void* W, const void* Xp, const float* bias, int T, int K, int D, int Hq, int Hkv, const VVRow* rows_dev,
                            const void* rope_tab, float* q_out, void* kc, void* vc, int64_t cache_stride, int64_t head_stride, const VVGemmWs* ws,
                            hipStream_t s);
int vv_attn_prefill4_launch(int D, const float* q, const VVRow* rows, const void* kc, const void* vc, int R, int Hq, int Hkv, int64_t cache_stride,
                            int64_t head_stride, float* out, void* out_packed, hipStream_t s);
int vv_block1d_supported(int C);
int vv_gemv_ok(const VVGemm* a);
// vv_gemv_plan (gemv_plan.h) -> the kernel of that form -> launch; VV_RC_NO_FORM where the plan finds none.  form (tests): the plan's form.
int vv_gemv_launch(VVGemm a, int xs, hipStream_t s, int* form);
int vv_gemv_w13_form_launch(VVGemm a, int mr, int wpb, hipStream_t s);      // tests: one named W13 form, streaming the twins or (w13 null) bf16
int vv_w13_pack_launch(const void* packed, void* twin, int N, int K, hipStream_t s);
int vv_w13_pack_rows_launch(const void* packed, void* twin, int N, int K, int tile0, int tiles, hipStream_t s);      // the tile rows tile0 .. tile0 + tiles - 1 alone
int vv_w13_unpack_launch(const void* twin, void* packed, int N, int K, hipStream_t s);
int vv_tile_ok(const VVGemm* a, int xs);
int vv_tile_launch(VVGemm a, int xs, hipStream_t s);
int vv_lora_merge_launch(const void* base, void* dst, int N, int K, const float* a, const float* b, int r, float scale, int delta_bf16,
                         hipStream_t s);
int vv_unpack_launch(const void* packed, float* dst, int N, int K, hipStream_t s);
// resample.hip.  _lds_bytes: what a push of n_in samples per row needs of the 64 KiB a workgroup has (the launcher refuses more).
int vv_resample_lds_bytes(int L, int T, int n_in);
int vv_resample_rows_launch(const VVRsRows* rows, int n, int L, int M, int T, const float* coef, float* hist, int n_streams, const float* x,
                            int ld_in, void* out, int ld_out, int pcm16, hipStream_t s);
int vv_resample_once_launch(int L, int M, int T, const float* coef, int n, int n_in, const float* x, int ld_in, float* out, int ld_out, hipStream_t s);
int vv_resample_reset_launch(float* hist, int T, int n_streams, const int* ids, int n, hipStream_t s);
// tempo.hip.  hist [n_streams][VV_TP_HIST], dstate [n_streams] (each stream's last offset), window [VV_TP_N]; offsets (may be null):
// the chosen offset of every block, row i at offsets + i * ld_off.
int vv_tempo_rows_launch(const VVTpRows* rows, int n, const float* window, float* hist, int* dstate, int n_streams, const float* x, int ld_in,
                         void* out, int ld_out, int pcm16, int* offsets, int ld_off, hipStream_t s);
int vv_tempo_once_launch(const float* window, int P, int Q, int n, int n_in, const float* x, int ld_in, float* out, int ld_out, int* offsets,
                         int ld_off, hipStream_t s);
int vv_tempo_reset_launch(float* hist, int* dstate, int n_streams, const int* ids, int n, hipStream_t s);
// pitch.hip.  table [VV_PT_Z * R + 1] the prototype's non-negative half, hist [n_streams][VV_PT_HIST].  _lds_bytes: what a push of n_in
// samples per row needs of the 64 KiB a workgroup has (the launcher refuses more).
int vv_pitch_lds_bytes(int R, int n_in);
int vv_pitch_rows_launch(const VVPitchRows* rows, int n, const float* table, int R, float* hist, int n_streams, const float* x, int ld_in,
                         void* out, int ld_out, int pcm16, hipStream_t s);
int vv_pitch_once_launch(const float* table, int R, const VVPitchRatios* pq, int n, int n_in, const float* x, int ld_in, float* out, int ld_out,
                         hipStream_t s);
int vv_pitch_reset_launch(float* hist, int n_streams, const int* ids, int n, hipStream_t s);
// formant.hip.  tw [2][VV_FM_N] cos and sin of 2 pi i / N; hist [n_streams][VV_FM_HIST], tail [n_streams][VV_FM_TAIL] (both null: stateless,
// whole signals); scratch [>= n][cap_frames][VV_FM_N] the windowed frames between the two launches of a push, row i of the launch at
// scratch + i * cap_frames * VV_FM_N.  Two launches: the frames, then the sums, the outputs and the streams' new state.
int vv_formant_rows_launch(const VVFmRows* rows, int n, const float* tw, float* hist, float* tail, int n_streams, const float* x, int ld_in,
                           float* out, int ld_out, float* scratch, int cap_frames, hipStream_t s);
int vv_formant_reset_launch(float* hist, float* tail, int n_streams, const int* ids, int n, hipStream_t s);
// level.hip.  A look-ahead / ramp, H hold (samples), c the ceiling; hist [n_streams][nh], nh = H + 2 A - 2.
int vv_level_rows_launch(const VVLvRows* rows, int n, int A, int H, float c, float* hist, int n_streams, const float* x, int ld_in, void* out,
                         int ld_out, int pcm16, hipStream_t s);
int vv_level_once_launch(int A, int H, float g, float c, int n, int n_in, const float* x, int ld_in, float* out, int ld_out, hipStream_t s);
int vv_level_reset_launch(float* hist, int nh, int n_streams, const int* ids, int n, hipStream_t s);
// loudness.hip.  taps [VV_LD_T] the integer taps as fp64; hist [n_streams][VV_LD_T] each stream's ring of quantised inputs, state [n_streams],
// part [n_streams][VV_LD_MAX_TILES][2] the FIR launch's sums for the apply launch.  E [n][ld_e]: segment energies, F [n][ld_f]: the same at 16 times
// the resolution, sum (z >> 24)^2 (either may be null).
int vv_loud_rows_launch(const VVLdRows* rows, int n, const double* taps, int* hist, VVLdState* state, long long* part, int n_streams, const float* x,
                        int ld_in, float* out, int ld_out, hipStream_t s);
int vv_loud_energy_launch(const double* taps, int n, int n_in, const float* x, int ld_in, long long* E, int ld_e, long long* F, int ld_f, hipStream_t s);
int vv_loud_once_launch(const double* taps, float t, float g0, float wmax, int n, int n_in, const float* x, int ld_in, float* out, int ld_out,
                        float* gain, int ld_gain, long long* E, int ld_e, hipStream_t s);
int vv_loud_reset_launch(int* hist, VVLdState* state, int n_streams, const int* ids, int n, hipStream_t s);
// pause.hip.  seg samples a segment; sbuf [n_streams][VV_PS_FLOATS] each stream's open segment, ring and `first`, state [n_streams] its counters;
// wt [2][seg] the join's weights w, u; counts [n] (device): what each row emitted.  _once: scratch [n][VV_PS_ONCE_FLOATS], counts [n][2]
// (device): what each signal emitted and dropped.
int vv_pause_rows_launch(const VVPsRows* rows, int n, int seg, float* sbuf, VVPsState* state, int n_streams, const float* wt, const float* x,
                         int ld_in, void* out, int ld_out, int pcm16, int* counts, hipStream_t s);
int vv_pause_once_launch(int seg, int C, int C0, long long theta, const float* wt, int n, int n_in, const float* x, int ld_in, float* out,
                         int ld_out, float* scratch, int* counts, hipStream_t s);
int vv_pause_reset_launch(VVPsState* state, int n_streams, const int* ids, int n, hipStream_t s);
}
