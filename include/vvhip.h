/* vvhip.h -- C ABI of libvvhip.so, the MI355X (gfx950) engine behind
 * VibeVoiceForConditionalGenerationInference.generate().
 *
 * The reference (vibevoice-community/VibeVoice) is pure Python: its "operator
 * interface" for this path is the set of nn.Module calls generate() makes per
 * step.  Each entry point below replaces one of those calls (file:line into
 * /root/reference/vibevoice/modular/); INTEGRATION.md shows the ctypes binding a
 * maintainer would add to modeling_vibevoice_inference.py.
 *
 * Conventions: plain C, opaque context, no torch types.  Pointers suffixed _dev
 * are device pointers (e.g. tensor.data_ptr()); the caller keeps them alive until
 * the stream has consumed them.  `stream` is a hipStream_t passed as void*
 * (0 = default stream).  Every function returns 0 on success, <0 on error
 * (vv_last_error() gives the text).  No hidden syncs except where stated; no
 * allocation after vv_create() except lazily-built hipGraphs and scratch on the
 * first call of a given shape.
 */
#ifndef VVHIP_H
#define VVHIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* libvvhip.so is built with -fvisibility=hidden: the functions declared in this header are its whole dynamic symbol table (the
 * kernel-launch helpers the translation units share stay internal; __graft_entry__.build() fails on any other exported vv_*). */
typedef struct vv_ctx vv_ctx;

typedef struct vv_config {
    /* Qwen2 decoder (configs/qwen2.5_*.json "decoder_config") */
    int lm_hidden, lm_layers, lm_heads, lm_kv_heads, lm_head_dim, lm_inter, lm_vocab;
    float lm_eps;
    /* diffusion head ("diffusion_head_config") */
    int head_layers, head_ffn, latent_dim;
    float head_eps;
    /* tokenizers ("acoustic_tokenizer_config", "semantic_tokenizer_config") */
    int n_filters, n_ratios, ratios[8];
    int n_stages, enc_depths[8]; /* encoder order; decoder uses the reverse */
    int sem_dim;                 /* semantic vae_dim (0 = no semantic tokenizer) */
    int has_acoustic_encoder;    /* voice-prompt path */
    float codec_eps;
    /* runtime */
    int n_slots;       /* concurrent utterances: 2 KV caches (cond/uncond) + 2 conv states each */
    int max_ctx;       /* KV positions per cache (rounded up to 128) */
    int max_rows;      /* max LM rows per launch (<=16384): decode uses 2 per utterance, prompt prefill fills it */
    int xsplit;        /* activation precision inside MFMA: 1 bf16, 2 ~fp24, 3 fp32-exact */
    int attn_splits;   /* flash-decoding splits along the sequence */
    int enc_frames;    /* frames per chunk of the voice-prompt encoder (>=1) */
    int use_graph;     /* replay captured hipGraphs for repeated shapes */
    /* Streaming-0.5B split LM (modeling_vibevoice_streaming.py:108-164): the last `tts_layers` of the
     * lm_layers stack form the TTS LM (own final norm), the first lm_layers-tts_layers the text LM
     * (final norm = Identity); adds tts_input_types + the binary EOS classifier.  0 = ordinary model. */
    int tts_layers;
} vv_config;

#pragma GCC visibility push(default)
int vv_create(const vv_config* cfg, vv_ctx** out);
/* A second context over the SAME weight storage as `parent` (fully uploaded, not itself shared): its own KV caches, activations,
 * tokenizer state, graphs and staging, sized by cfg's runtime fields (n_slots, max_ctx, max_rows, attn_splits, use_graph); the model
 * fields must equal the parent's.  Two contexts driven on two streams interleave two independent utterance batches on one GPU over
 * one copy of the weights (new surface: the reference shares weights between concurrent generate() calls by being one nn.Module,
 * and forbids the concurrency -- it is not re-entrant).  vv_upload / LoRA merges go through the parent, BEFORE any child
 * exists: a child snapshots what it derives from the parameters (lm_head / tied table, valid-token rows, RoPE table, speech factors), so
 * vv_upload on a parent with live children is refused -- destroy the children, upload, create them again.  Destroying the parent
 * first is allowed (the storage lives until the last child is destroyed). */
int vv_create_shared(const vv_config* cfg, vv_ctx* parent, vv_ctx** out);
void vv_destroy(vv_ctx* ctx);
const char* vv_last_error(vv_ctx* ctx);
/* "VVHIP_BUILD_ID=<sha256[:16] of the sources and flags the library was compiled from>": the Python loader refuses
 * (or rebuilds) a binary whose id differs from the sources beside it.  New surface: the reference has no native
 * code, hence no counterpart (its "is the install current" check is pip's, pyproject.toml:1-40). */
const char* vv_build_id(void);
/* Asynchronous device-side errors, checked on the host: today the one inter-workgroup hand-off on the path (the K-split of the
 * long-prompt GEMM's partial round, prefill.hip) reports a lost producer through a host-mapped word instead of spinning.  Waits
 * for `stream`, and if the word is set: re-arms the hand-off state, clears it and returns <0 (the prompt pass that was in flight
 * produced a wrong tile and must be repeated; the context stays usable).  The same check runs at the head of every vv_lm_forward*.  Callers: after the
 * stream sync that ends a prompt prefill.  New surface (the reference has no native code); its closest counterpart is the
 * CUDA error a torch.cuda.synchronize() raises after modeling_vibevoice_inference.py:467-482. */
int vv_check(vv_ctx* ctx, void* stream);

/* ---- parameters.  Names are the reference state_dict keys with the prefixes
 * model.language_model.->"lm."  model.prediction_head.->"head."
 * model.acoustic_tokenizer.decoder.->"dec."  model.acoustic_tokenizer.encoder.->"aenc."
 * model.semantic_tokenizer.encoder.->"senc."  model.acoustic_connector.->"ac_conn."
 * model.semantic_connector.->"sem_conn."  lm_head.weight (optional: tied -> embed_tokens),
 * plus "lm.rope.inv_freq" (fp32 [head_dim/2], the table HF computes in Qwen2RotaryEmbedding).
 * The engine repacks every matrix into MFMA-fragment tiles (bf16). */
int vv_num_weights(vv_ctx* ctx);
int vv_weight_info(vv_ctx* ctx, int idx, char* name, int name_cap, int64_t* nelem, int* loaded);
/* src may be a host or a device pointer; src_dtype 0 = fp32, 1 = bf16. Synchronous. */
int vv_upload(vv_ctx* ctx, const char* name, const void* src, int src_dtype, int64_t nelem);
/* ---- device-resident LoRA adapters.  What the reference does by wrapping live modules in peft (lora_loading.py:140-176) and
 * merging on the host, done on the packed weights in place: the A / B factors stay on the device and a switch is one streaming pass
 * per target matrix.  Parent contexts only, under vv_upload's guards (refused on a shared child and while shared children exist).
 * All three are eager launches on `stream`, never captured; no pointer changes, so cached hipGraphs stay valid, and the KV caches
 * are not touched (K/V computed under other weights is the caller's to discard).  Refusals -- unknown name, a parameter that is not
 * a plain linear matrix (tables, vectors, the tokenizers' convolutions), r outside [1, 256], a non-finite scale, null or misaligned
 * (16-byte) operands -- return < 0 before anything is launched.
 * vv_weight_read: the parameter as it is now, row-major fp32 [N][K] (exact: the storage is bf16).
 * vv_lora_merge: active = bf16(base + scale * B.A) with the arithmetic of vv_lora_merge_raw.  The FIRST merge of a parameter copies
 * its packed region into a base snapshot (engine allocator; vv_stat 7 counts the bytes); every merge reads that snapshot, so a merge
 * is never cumulative: merging adapter Y after adapter X leaves no trace of X.  Parameters that share one packed region (q / k / v,
 * the adaLN matrices) keep to their own tiles.
 * vv_lora_reset: the snapshot copied back over the active region; name == NULL: every merged parameter.  A parameter that was
 * never merged is left alone.  vv_upload to a parameter that has a snapshot makes the uploaded tensor the new base. */
int vv_weight_read(vv_ctx* ctx, void* stream, const char* name, float* out_dev);
/* [N][K] of a plain linear matrix parameter, for callers that size a_dev / b_dev / out_dev (Engine.lora_merge and weight_read check
 * their tensors against it before the call); < 0 for an unknown name or any other kind of parameter.  No device work. */
int vv_weight_shape(vv_ctx* ctx, const char* name, int* N, int* K);
int vv_lora_merge(vv_ctx* ctx, void* stream, const char* name, const float* a_dev, const float* b_dev, int r, float scale,
                  int delta_bf16);
int vv_lora_reset(vv_ctx* ctx, void* stream, const char* name);
/* scalar buffers speech_scaling_factor / speech_bias_factor (modeling_vibevoice.py:131-132).  May be called at any time: graphs
 * captured by vv_codec_decode / vv_codec_chain_batch with apply = 1 hold the old factors and are dropped (after a device-wide wait
 * when there are any), so the next frame applies the new ones. */
int vv_set_speech_factors(vv_ctx* ctx, float scaling, float bias);
/* ids the constrained sampler may emit (VibeVoiceTokenConstraintProcessor, modeling_vibevoice_inference.py:53-66,405-419) */
int vv_set_valid_tokens(vv_ctx* ctx, const int* ids, int n);
/* DPM-Solver++ table for N steps: t[N] (the timestep values fed to the head) and coef[N][5] =
 * {alpha_i, sigma_i, sigma_{i+1}/sigma_i, -alpha_{i+1}(e^{-h}-1), second-order term}
 * (dpm_solver.py:321-423,581-584,669-677,738-764) -- computed by vibevoice_amd/schedule.py */
int vv_set_schedule(vv_ctx* ctx, int n_steps, const float* t, const float* coef, void* stream);
/* The sde-dpmsolver++ table (noise_scheduler.from_config(..., algorithm_type='sde-dpmsolver++'), demo/gradio_demo.py:142-146):
 * coef6[N][6] = {alpha_i, sigma_i, (sigma_{i+1}/sigma_i) e^{-h}, alpha_{i+1}(1 - e^{-2h}), second-order term,
 * sigma_{i+1} sqrt(1 - e^{-2h})} (dpm_solver.py:680-686,785-793); sample with vv_diffusion_sample_sde */
int vv_set_schedule_sde(vv_ctx* ctx, int n_steps, const float* t, const float* coef6, void* stream);

/* ---- KV caches: cache id = 2*slot (+1 for the CFG-negative branch) */
typedef struct vv_row { int cache; int pos; } vv_row;

/* One Qwen2 forward over n_rows tokens, each appended to its cache at rows[i].pos
 * (== the cache length before this token).  Replaces self(**model_inputs, ...)
 * (modeling_vibevoice_inference.py:480-482 -> modeling_vibevoice.py:187-199 -> HF Qwen2Model)
 * for the positive rows and :583-585 for the negative rows -- both in ONE pass
 * over the weights.  hidden_out = last_hidden_state (after the final RMSNorm).
 * Row sets: (a) every row a different cache (decode steps; one fused attention launch per layer), or (b) consecutive
 * positions of one cache (prompt prefill, up to max_rows rows; LDS-staged MFMA GEMM + 64-row prefill attention), or (c) any other
 * mix of at most 64 rows (3-launch attention: all appends land before any row attends). */
int vv_lm_forward(vv_ctx* ctx, void* stream, int n_rows, const vv_row* rows,
                  const float* x_in_dev, float* hidden_out_dev);
/* Same over the layer range [layer_begin, layer_end) only; final_norm selects whether lm.norm is applied.
 * Streaming-0.5B: forward_lm = layers [0, n_lm) without norm (modeling_vibevoice_streaming_inference.py:181-241),
 * forward_tts_lm = layers [n_lm, n_lm+n_tts) with norm (:243-318). */
int vv_lm_forward_range(vv_ctx* ctx, void* stream, int n_rows, const vv_row* rows, const float* x_in_dev,
                        float* hidden_out_dev, int layer_begin, int layer_end, int final_norm);
/* Import n_pos cached positions of one layer into cache `cache` from HF layout k/v [kv_heads][n_pos][head_dim]
 * (keys already rotated, as DynamicCache stores them); src_dtype 0 fp32, 1 bf16.  Used for the voice presets
 * (demo/voices/streaming_model/ presets -> all_prefilled_outputs). */
int vv_kv_import(vv_ctx* ctx, void* stream, int cache, int layer, int n_pos, const void* k_dev, const void* v_dev,
                 int src_dtype);
/* The same for cache positions [pos0, pos0 + n_pos): source row i lands at position pos0 + i.  Lets a caller resume an
 * utterance from KV state computed elsewhere (and the long-context tests / bench place known K/V at chosen positions). */
int vv_kv_import_at(vv_ctx* ctx, void* stream, int cache, int layer, int pos0, int n_pos, const void* k_dev,
                    const void* v_dev, int src_dtype);
/* Cached position src_pos copied onto dst_pos in every layer of `cache` (keys keep the rotation they were computed with).  The one
 * place the reference re-arranges a row's negative cache so that an entry ends up at another index with its ORIGINAL rotation: the
 * correction of a non-diffusing batch row that holds exactly one valid entry (modeling_vibevoice_inference.py:594-624: the mask
 * shifts, :603, and the K/V does not, :613 -- the entry appended at that step stays, the older one is masked out). */
int vv_kv_move(vv_ctx* ctx, void* stream, int cache, int src_pos, int dst_pos);
/* The exact inverse of vv_kv_import_at: positions [pos0, pos0 + n_pos) of one layer of `cache` written out in HF layout
 * k/v [kv_heads][n_pos][head_dim], keys as cached (rotated); dst_dtype 0 fp32, 1 bf16 (both exact: the cache holds bf16).  Outputs
 * 16-byte aligned.  What makes a prompt prefix storable on disk independent of the tile layout, and how the tests read a cache.
 * New surface; closest reference counterpart: reading past_key_values[layer] of the DynamicCache generate() carries
 * (modeling_vibevoice_inference.py:480-482), which the reference can slice because its cache is a list of plain tensors. */
int vv_kv_export(vv_ctx* ctx, void* stream, int cache, int layer, int pos0, int n_pos, void* k_out_dev, void* v_out_dev,
                 int dst_dtype);
/* A prompt prefix as data (voice presets for the non-streaming class): positions [0, n_pos) of EVERY layer and kv head of `cache`
 * copied to two compact buffers in the cache's own tile layouts (K tiles [pos/16][d/32][lane][8], V blocks [pos/32][d/16][lane][8],
 * DESIGN.md section 2), each [layer][kv_head][ceil32(n_pos) * head_dim] bf16 = vv_kv_snapshot_bytes bytes, 16-byte aligned.  The
 * buffer does not depend on max_ctx: a context created with another max_ctx over the same model (a vv_create_shared child) restores
 * it.  Slots of positions >= n_pos inside the last 32-position block are written as ZERO whatever the source holds there (V: the
 * prefill attention multiplies whole stages and 0 x NaN = NaN; K: so that a snapshot is a function of the n_pos positions alone).
 * vv_kv_restore is the inverse, into positions [0, ceil32(n_pos)) of `cache`; the caller then appends behind n_pos with
 * vv_lm_forward.  One eager launch each (K, V and all layers), never part of a captured sequence.  New surface; closest reference
 * counterpart: the Streaming class's prefilled presets, copy.deepcopy(all_prefilled_outputs) at the head of its generate()
 * (modeling_vibevoice_streaming_inference.py) -- the non-streaming generate() re-runs the prompt on every call (:467-482). */
int64_t vv_kv_snapshot_bytes(vv_ctx* ctx, int n_pos);
int vv_kv_snapshot(vv_ctx* ctx, void* stream, int cache, int n_pos, void* k_out_dev, void* v_out_dev);
int vv_kv_restore(vv_ctx* ctx, void* stream, int cache, int n_pos, const void* k_dev, const void* v_dev);
/* y[t][:] = x[t][:] + tts_input_types[type]  (forward_tts_lm, :293) */
int vv_add_type_embedding(vv_ctx* ctx, void* stream, int n, const float* x_dev, int type, float* out_dev);
/* tts_eos_classifier: fc2(relu(fc1(h))) -> out_dev[n] logits (BinaryClassifier, modeling_vibevoice_streaming.py:42-53) */
int vv_eos_logit(vv_ctx* ctx, void* stream, int n, const float* hidden_dev, float* out_dev);
/* embed_tokens lookup (modeling_vibevoice_inference.py:218,569); ids on host, 1 <= n <= max(64, max_rows) per call */
int vv_embed(vv_ctx* ctx, void* stream, int n, const int* ids, float* out_dev);
/* logits restricted to the valid ids: replaces lm_head + constraint mask (:241-242,488-490).
 * logits_out_dev [n][n_valid] fp32 in the order given to vv_set_valid_tokens. */
int vv_lm_logits(vv_ctx* ctx, void* stream, int n, const float* hidden_dev, float* logits_out_dev);
/* lm_head over the whole vocabulary (:241-242, `outputs.logits[:, -1, :]` of :486): logits_out_dev [n][lm_vocab] fp32, 1 <= n <= 16.
 * Needed only when a full-vocabulary logits processor is requested (top-k / top-p / min-p / repetition penalty run before the
 * valid-id constraint in the reference's processor list, :310-319); the default path evaluates the valid rows only. */
int vv_lm_logits_full(vv_ctx* ctx, void* stream, int n, const float* hidden_dev, float* logits_out_dev);
/* The full-vocabulary logits processors of :310-319 (HF's order: repetition penalty; with do_sample temperature, top-k, top-p,
 * min-p with min_tokens_to_keep = 1) followed by the valid-id constraint of :416-419, evaluated for the valid ids only: each
 * processor is a reduction over the row, nothing is sorted and nothing of size lm_vocab is written.  logits_dev [n][lm_vocab] fp32
 * as vv_lm_logits_full wrote them (read only); seen_dev [n][lm_vocab] bytes, non-zero where the id occurs in the row's input_ids
 * (NULL when repetition_penalty == 1); top_k 0 = off (HF: k = min(top_k, lm_vocab)), top_p 1 = off, min_p 0 = off; temperature and
 * the three filters apply only with do_sample.  out_dev [n][n_valid] fp32 in the order given to vv_set_valid_tokens: the processed
 * score, bit-equal to torch's fp32 arithmetic, or -inf where a filter removed the id; survivors_dev [n]: finite entries per row
 * (0: the reference would fail in torch.multinomial).  1 <= n <= 16.  One eager launch on `stream`, never captured; bit-identical
 * run to run. */
int vv_lm_warp_valid(vv_ctx* ctx, void* stream, int n, const float* logits_dev, const unsigned char* seen_dev,
                     float repetition_penalty, float temperature, int do_sample, int top_k, float top_p, float min_p,
                     float* out_dev, int* survivors_dev);
/* The normals of seeded requests (vibevoice_amd/noise.py defines them: Philox4x32-10, key = the seed, counter = (element / 4, t,
 * stream id, aux), Box-Muller on the four output words): one request's draws are a function of its own key and counters only.
 * out[s][r][f][j], s < n_streams (stream id stream0 + s), r < n, f < n_t (counter word t = keys[r].t0 + f), j < width: the j-th
 * normal of row r.  keys_host: n keys in HOST memory, passed to the kernel by value.  1 <= n <= 16, n_t >= 1, 1 <= n_streams <= 65,
 * width a positive multiple of 4, total elements < 2^31, out_dev 16-byte aligned; anything else: negative return + vv_last_error,
 * nothing launched.  One eager launch on `stream`, never captured; no device-side state. */
typedef struct vv_noise_key { uint32_t seed_lo, seed_hi, t0, aux; } vv_noise_key;
int vv_noise_rows(vv_ctx* ctx, void* stream, int n, const vv_noise_key* keys_host, uint32_t stream0, int n_streams,
                  int n_t, int width, float* out_dev);

/* sample_speech_tokens (:697-710): cond_dev [2n][H] = n positive then n negative
 * conditions, noise_dev [n][latent], -> latent_out_dev [n][latent] */
int vv_diffusion_sample(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev,
                        float cfg_scale, float* latent_out_dev);
/* The same sampler under the stochastic solver the gradio demo installs (demo/gradio_demo.py:142-146:
 * noise_scheduler.from_config(config, algorithm_type='sde-dpmsolver++', ...)): scheduler.step() adds
 * sigma_t sqrt(1 - e^{-2h}) * eps_i with eps_i = randn(model_output.shape) drawn per solver step
 * (vibevoice/schedule/dpm_solver.py:680-686, 785-793, 994-997).  step_noise_dev [n_steps][n][latent] fp32
 * = those draws (first n rows of each: only they reach the next step, modeling_vibevoice_inference.py:703-704).
 * Needs a table from vv_set_schedule_sde; vv_diffusion_sample refuses to run on a stochastic table. */
int vv_diffusion_sample_sde(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev,
                            const float* step_noise_dev, float cfg_scale, float* latent_out_dev);
/* vv_diffusion_sample / vv_diffusion_sample_sde with one guidance scale per utterance: cfg_rows_dev [n] fp32, read by the
 * kernels at run time (the values are NOT part of the graph key; rewriting the buffer between calls needs no re-capture).
 * step_noise_dev == NULL: deterministic table required; non-NULL: stochastic table required (the same guard rails as the two
 * scalar entry points).  New surface: the reference's sample_speech_tokens takes one cfg_scale for the whole batch. */
int vv_diffusion_sample_rows(vv_ctx*, void* stream, int n, const float* cond_dev, const float* noise_dev,
                             const float* step_noise_dev, const float* cfg_rows_dev, float* latent_out_dev);
/* The reference scheduler's other sampling-time settings (DPMSolverMultistepScheduler: solver_order 1..3, solver_type midpoint /
 * heun, lower_order_final, euler_at_final, final_sigmas_type, timestep_spacing, steps_offset, lambda_min_clipped; both
 * dpmsolver++ and sde-dpmsolver++) as one table row per solver step, coef8 = n_steps rows {a, s, cs, c0, c1, c2, cn, 0}:
 *   x0 = a z - s v;   z' = cs z + c0 x0 + c1 (x0 - m1) + c2 (m1 - m2) + cn noise      (m1, m2: the two previous x0)
 * (schedule/dpm_solver.py:669-686, 738-800, 861-893 with the model-output differences factored out; the host side is
 * vibevoice_amd/schedule.py: make_general_table).  stochastic != 0: the table carries variance-noise scales and sampling needs the
 * per-step noise.  Replaces whatever table was installed; the two shipped configurations keep vv_set_schedule / _sde and their
 * samplers, and each sampler refuses the other kind of table. */
int vv_set_schedule_general(vv_ctx* ctx, int n_steps, const float* t, const float* coef8, int stochastic, void* stream);
/* sample_speech_tokens under a general table, 1 <= n <= 8.  step_noise_dev [n_steps][n][latent] for a stochastic table, NULL for
 * a deterministic one (the other way round is refused); cfg_rows_dev [n] per-utterance guidance scales read at run time (the
 * graph key holds the pointer, never the values), or NULL: cfg_scale for every row.  A step is the head's layers, the final
 * layer's plain GEMM and one launch of solver.hip (update + the next step's in-projection where its rule allows). */
int vv_diffusion_sample_general(vv_ctx* ctx, void* stream, int n, const float* cond_dev, const float* noise_dev,
                                const float* step_noise_dev, float cfg_scale, const float* cfg_rows_dev, float* latent_out_dev);
/* one prediction_head forward (modular_vibevoice_diffusion_head.py:254-280) for tests:
 * noisy [n][latent], t[n] (host), cond [n][H] -> out [n][latent].  Synchronous. */
int vv_head_forward(vv_ctx* ctx, void* stream, int n, const float* noisy_dev, const float* t_host,
                    const float* cond_dev, float* out_dev);

/* acoustic_tokenizer.decode(latent/scale - bias, cache, use_cache=True) (:636-643) for one
 * utterance slot: latent_dev [frames][latent] -> audio_out_dev [frames*hop]. */
int vv_codec_decode(vv_ctx* ctx, void* stream, int slot, int frames, const float* latent_dev,
                    float* audio_out_dev, int apply_speech_factors);
/* semantic_tokenizer.encode(audio, cache, use_cache=True).mean (:658-664) */
int vv_semantic_encode(vv_ctx* ctx, void* stream, int slot, int frames, const float* audio_dev,
                       float* sem_out_dev);
/* One frame of n utterances (1..8) through both tokenizers in one call: the reference decodes / re-encodes the whole set of
 * diffusion rows of a step as ONE batch -- acoustic_tokenizer.decode(scaled_latent, cache=acoustic_cache,
 * sample_indices=diffusion_indices) then semantic_tokenizer.encode(audio_chunk, cache=semantic_cache, sample_indices=...)
 * (modeling_vibevoice_inference.py:636-672; per-sample cache rows: modular_vibevoice_tokenizer.py:76-126).  Row j of
 * latent_dev [n][latent] / audio_out_dev [n][hop] / sem_out_dev [n][sem_dim] belongs to streaming slot slots[j] (distinct).
 * sem_out_dev = NULL: decode only.  Same results as n vv_codec_decode + vv_semantic_encode calls up to bf16 summation order;
 * the weight-heavy stages of both nets read their weights once for the whole batch. */
int vv_codec_chain_batch(vv_ctx* ctx, void* stream, int n, const int* slots, const float* latent_dev,
                         float* audio_out_dev, float* sem_out_dev, int apply_speech_factors);
/* acoustic_tokenizer.encode(wav).mean, non-streaming (:154; modular_vibevoice_tokenizer.py:1081-1085):
 * wav_dev [frames*hop] -> mean_out_dev [frames][latent] */
int vv_acoustic_encode(vv_ctx* ctx, void* stream, int frames, const float* wav_dev, float* mean_out_dev);
/* The same for a signal that does not fill its last frame: valid_samples in ((frames - 1) * hop, frames * hop], wav_dev zero beyond them.
 * The reference right-pads PER strided conv layer (SConv1d.forward -> get_extra_padding_for_conv1d, modular_vibevoice_tokenizer.py):
 * past the end of the signal every strided conv reads zeros, not the activations a zero waveform would produce.  Only the last,
 * partial frame's latent depends on it (every layer is causal). */
int vv_acoustic_encode_ragged(vv_ctx* ctx, void* stream, int frames, long long valid_samples, const float* wav_dev, float* mean_out_dev);
/* Frames the voice-prompt encoder takes per pass, 1..config.enc_frames (the buffers are sized for enc_frames; the default).
 * The reference's non-streaming encode runs the whole prompt as one sequence (modular_vibevoice_tokenizer.py:384-418,
 * 1081-1085); a pass of F frames is that computation on F frames with the causal history carried over, so the result does
 * not depend on F -- tests/test_gpu_shipped.py holds every pass size to the oracle's one-sequence encode. */
int vv_set_enc_pass_frames(vv_ctx* ctx, int frames_per_pass);
/* 16-bit PCM of n chunks of `samples` fp32 samples each, on device, before the chunk leaves for the host: the arithmetic
 * of convert_to_16_bit_wav (demo/gradio_demo.py:1058-1073, applied per streamed chunk at :404-418): peak = max|x| of the
 * chunk; x /= peak when peak > 1; int16(trunc(x * 32767)).  audio_dev [n][samples] fp32 -> pcm_out_dev [n][samples] int16. */
int vv_audio_to_pcm16(vv_ctx* ctx, void* stream, int n, int samples, const float* audio_dev, int16_t* pcm_out_dev);
/* ---- audio at another sample rate: a streaming rational resampler L / M (vibevoice_amd/resample.py defines it and designs the
 * filter).  Output m is the input at time m * M / L, the input taken as zero outside itself: with k = m * M + (L * T - 2) / 2,
 * y[m] = sum_{t < T} coef[k % L][t] * x[k / L - t], fp32 fmaf in that order.  What a stream emits does not depend on how its input
 * was cut into pushes: a push emits every output whose last input sample has arrived (the last T / 2 samples wait for the next
 * push), the flush emits the rest against zeros, ceil(total * L / M) outputs in all.
 * vv_resampler_set: configuration rs (0..3) of this context: coef_host [L][T] fp32 in HOST memory, T even, n_streams history rows,
 * all zero.  Replaces what rs held.  Synchronous.  Refused with a message: a table that does not fit the kernel's 64 KiB of LDS. */
int vv_resampler_set(vv_ctx* ctx, int rs, int L, int M, int T, const float* coef_host, int n_streams, void* stream);
/* Back to the state after vv_resampler_set for n streams (stream_ids_host == NULL: all of them): history zeroed by a kernel on
 * `stream`, input total 0, flush mark cleared. */
int vv_resampler_reset(vv_ctx* ctx, void* stream, int rs, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, ONE launch on `stream`: row i = n_in samples at audio_dev + i * ld_in for stream rows_host[i].stream
 * (distinct), flush != 0: the stream's last push.  Its outputs go to out_dev + i * ld_out (elements): out_fmt 0 = fp32, 1 = int16
 * with the arithmetic of vv_audio_to_pcm16 over the row's resampled chunk.  n_out_host [n]: what each row emitted, computed on the
 * host from the streams' input totals (no sync).  Rows may stand at different totals.  Refused with a message, nothing written, no
 * state changed: n outside [1,16], a stream id out of range or named twice, n_in < 0 or above ld_in, a row that emits more than
 * ld_out or more than 8192 samples, a chunk too long for the kernel's LDS, a push to a flushed stream before its reset. */
typedef struct vv_resample_row { int stream; int n_in; int flush; } vv_resample_row;
int vv_resample_rows(vv_ctx* ctx, void* stream, int rs, int n, const vv_resample_row* rows_host, const float* audio_dev, int ld_in,
                     void* out_dev, int ld_out, int out_fmt, int* n_out_host);
/* Stateless: n whole signals of n_in samples (audio_dev + i * ld_in) -> ceil(n_in * L / M) fp32 samples each (out_dev + i * ld_out),
 * coef_dev [L][T] on the device.  Bit-identical to the same signal pushed and flushed through vv_resample_rows. */
int vv_resample_once(vv_ctx* ctx, void* stream, int L, int M, int T, const float* coef_dev, int n, int n_in, const float* audio_dev,
                     int ld_in, float* out_dev, int ld_out);
/* ---- speaking rate: a streaming, pitch-preserving tempo change P / Q in [1/2, 2], Q <= 100, at 24 kHz (vibevoice_amd/tempo.py
 * defines it: WSOLA, hop 240, window 480, search radius 160, an exact integer similarity search -- the device chooses the offsets the
 * definition chooses).  A signal of n samples yields ceil(n * Q / P), in blocks of 240.  What a stream emits does not depend on how
 * its input was cut into pushes: a push emits every block all of whose input has arrived (at most 640 samples wait for the next
 * push), the flush emits the rest against zeros.
 * vv_tempo_set: configuration tp (0..3) of this context: window_host [480] fp32 in HOST memory (the periodic Hann table of the
 * definition), n_streams streams at their first sample.  Replaces what tp held.  Synchronous. */
int vv_tempo_set(vv_ctx* ctx, int tp, const float* window_host, int n_streams, void* stream);
/* Back to the state after vv_tempo_set for n streams (stream_ids_host == NULL: all of them): history and last offset zeroed by a
 * kernel on `stream`, input total 0, speed and flush mark cleared. */
int vv_tempo_reset(vv_ctx* ctx, void* stream, int tp, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, ONE launch on `stream`: row i = n_in samples at audio_dev + i * ld_in for stream rows_host[i].stream
 * (distinct) at speed P / Q (a stream keeps the speed of its first push until its reset), flush != 0: the stream's last push.  Its
 * outputs go to out_dev + i * ld_out (elements): out_fmt 0 = fp32, 1 = int16 with the arithmetic of vv_audio_to_pcm16 over the row's
 * stretched chunk.  n_out_host [n]: what each row emitted, computed on the host from the streams' input totals (no sync).
 * offsets_dev (may be NULL): the offset chosen for each block the row walked, row i at offsets_dev + i * ld_off, n_out / 240 rounded
 * up of them.  Refused with a message, nothing written, no state changed: as vv_resample_rows, and a stream whose speed changes; with
 * the return value VV_TEMPO_OVER_CAPACITY a row of more than 7680 input samples, more than 96 blocks or more than ld_out outputs:
 * the caller splits that push. */
#define VV_TEMPO_OVER_CAPACITY 3
typedef struct vv_tempo_row { int stream; int n_in; int flush; int P; int Q; } vv_tempo_row;
int vv_tempo_rows(vv_ctx* ctx, void* stream, int tp, int n, const vv_tempo_row* rows_host, const float* audio_dev, int ld_in,
                  void* out_dev, int ld_out, int out_fmt, int* n_out_host, int* offsets_dev, int ld_off);
/* Stateless: n whole signals of n_in samples (audio_dev + i * ld_in) -> ceil(n_in * Q / P) fp32 samples each (out_dev + i * ld_out),
 * window_dev [480] on the device; offsets_dev as above.  Bit-identical to the same signal pushed and flushed through vv_tempo_rows. */
int vv_tempo_once(vv_ctx* ctx, void* stream, const float* window_dev, int P, int Q, int n, int n_in, const float* audio_dev, int ld_in,
                  float* out_dev, int ld_out, int* offsets_dev, int ld_off);
/* ---- pitch: a streaming variable-ratio band-limited resampler P / Q, both terms in 1..100, P / Q in [1/2, 2], each row of a push at
 * its own ratio over one prototype table (vibevoice_amd/pitch.py defines it).  Behind a tempo change by Q / P it moves the pitch by
 * P / Q and keeps the duration; the formants move with the pitch.  Output m is the input at time m * P / Q, the input taken as zero
 * outside itself: with den = max(P, Q), q = m * P / Q, a = m * P % Q, Tn = ceil(32 * den / Q) <= 64,
 * y[m] = sum_{t = -Tn .. Tn} (Q / den) c(a, t) x[q - t], c the table at |a + t * Q| * R / den by linear interpolation, fp32 fmaf in that
 * order; 1 / 1 is the identity (Tn = 0).  What a stream emits does not depend on how its input was cut into pushes: a push emits every
 * output whose newest input sample q + Tn has arrived, the flush emits the rest against zeros, ceil(total * Q / P) outputs in all.
 * vv_pitch_set: configuration pt (0..3) of this context: table_host [n_table = 32 * R + 1] fp32 in HOST memory, the non-negative half of
 * the prototype at R <= 256 entries per zero crossing; n_streams streams at their first sample.  Replaces what pt held.  Synchronous. */
int vv_pitch_set(vv_ctx* ctx, int pt, const float* table_host, int n_table, int R, int n_streams, void* stream);
/* Back to the state after vv_pitch_set for n streams (stream_ids_host == NULL: all of them): history zeroed by a kernel on `stream`,
 * input total 0, ratio and flush mark cleared. */
int vv_pitch_reset(vv_ctx* ctx, void* stream, int pt, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, ONE launch on `stream`: row i = n_in samples at audio_dev + i * ld_in for stream rows_host[i].stream
 * (distinct) at ratio P / Q (a stream keeps the ratio of its first push until its reset), flush != 0: the stream's last push.  Its
 * outputs go to out_dev + i * ld_out (elements): out_fmt 0 = fp32, 1 = int16 with the arithmetic of vv_audio_to_pcm16 over the row's
 * resampled chunk.  n_out_host [n]: what each row emitted, computed on the host from the streams' input totals (no sync).  Refused with
 * a message, nothing written, no state changed: as vv_resample_rows, and P or Q outside 1..100 or P / Q outside [1/2, 2], a stream
 * whose ratio changes, a row of more than 7552 input samples or one that emits more than 8192 or more than ld_out. */
typedef struct vv_pitch_row { int stream; int n_in; int flush; int P; int Q; } vv_pitch_row;
int vv_pitch_rows(vv_ctx* ctx, void* stream, int pt, int n, const vv_pitch_row* rows_host, const float* audio_dev, int ld_in,
                  void* out_dev, int ld_out, int out_fmt, int* n_out_host);
/* Stateless: n whole signals of n_in samples (audio_dev + i * ld_in), signal i at ratio pq_host[2 i] / pq_host[2 i + 1] (HOST memory)
 * -> ceil(n_in * Q / P) fp32 samples (out_dev + i * ld_out); table_dev [n_table = 32 * R + 1] on the device.  One launch per 16 signals.
 * Bit-identical to the same signal pushed and flushed through vv_pitch_rows. */
int vv_pitch_once(vv_ctx* ctx, void* stream, const float* table_dev, int n_table, int R, int n, const int* pq_host, int n_in,
                  const float* audio_dev, int ld_in, float* out_dev, int ld_out);
/* ---- formants: a streaming spectral-envelope warp A / B, both terms in 1..10^4, A / B in [1/2, 2], each row of a push at its own
 * fraction, at 24 kHz (vibevoice_amd/formant.py defines it): frames of 1024 at hop 256 under a periodic Hann window, per frame the
 * cepstral envelope (quefrencies below 64) read at k * B / A by linear interpolation, a real gain exp(clamp(Ew - E, +-30 dB)) on the
 * spectrum, overlap-add in ascending frame order with the scale 2/3.  The envelope moves up by A / B, the pitch stays; in front of
 * vv_pitch_rows at P / Q, A / B = Q / P keeps the formants where they were.  1 / 1 is the identity, nothing held back.  n samples in,
 * n out.  What a stream emits does not depend on how its input was cut into pushes: a push emits every block of 256 whose input
 * through 768 samples past its end has arrived (at most 1023 samples wait for the next push), the flush emits the rest against zeros.
 * vv_formant_set: configuration fm (0..3) of this context: twiddles_host [2][1024] fp32 in HOST memory, cos and sin of 2 pi i / 1024;
 * n_streams streams at their first sample.  Replaces what fm held.  Synchronous.  The pushes of one configuration are ordered on one
 * stream: the frames of a launch pass through a buffer of the configuration. */
int vv_formant_set(vv_ctx* ctx, int fm, const float* twiddles_host, int n_streams, void* stream);
/* Back to the state after vv_formant_set for n streams (stream_ids_host == NULL: all of them): history and partial sums zeroed by a
 * kernel on `stream`, input total 0, fraction and flush mark cleared. */
int vv_formant_reset(vv_ctx* ctx, void* stream, int fm, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, TWO launches on `stream` (the frames; the sums, the outputs and the new state): row i = n_in samples at
 * audio_dev + i * ld_in for stream rows_host[i].stream (distinct) at the fraction A / B (a stream keeps the fraction of its first push
 * until its reset), flush != 0: the stream's last push.  Its outputs go to out_dev + i * ld_out, fp32.  n_out_host [n]: what each row
 * emitted, computed on the host from the streams' input totals (no sync).  Refused with a message, nothing written, no state changed:
 * as vv_pitch_rows, and A or B outside 1..10^4 or A / B outside [1/2, 2], a stream whose fraction changes, a row of more than 7552
 * input samples or one that emits more than ld_out, and out_fmt = 1: a level stage follows this one, it never writes int16. */
typedef struct vv_formant_row { int stream; int n_in; int flush; int A; int B; } vv_formant_row;
int vv_formant_rows(vv_ctx* ctx, void* stream, int fm, int n, const vv_formant_row* rows_host, const float* audio_dev, int ld_in,
                    void* out_dev, int ld_out, int out_fmt, int* n_out_host);
/* Stateless: n whole signals of n_in samples (audio_dev + i * ld_in), signal i at the fraction ab_host[2 i] / ab_host[2 i + 1] (HOST
 * memory) -> n_in fp32 samples (out_dev + i * ld_out); twiddles_dev [2][1024] on the device; scratch_dev: scratch_floats fp32 on the
 * device, at least min(n, 16) * (ceil(n_in / 256) + 3) * 1024, for the frames.  One launch group per 16 signals.  Bit-identical to
 * the same signal pushed and flushed through vv_formant_rows. */
int vv_formant_once(vv_ctx* ctx, void* stream, const float* twiddles_dev, int n, const int* ab_host, int n_in, const float* audio_dev,
                    int ld_in, float* out_dev, int ld_out, float* scratch_dev, long long scratch_floats);
/* ---- output level: a streaming gain and look-ahead peak limiter (vibevoice_amd/level.py defines it).  A: look-ahead and ramp, H: hold,
 * in samples; g: the gain, c: the ceiling.  u = fl(g x) (non-finite: 0), r = 1 where |u| <= c else fl(c / |u|), q = floor(r 2^20),
 * h[j] = min q[j - H .. j + A - 1], S[i] = sum h[i - A + 1 .. i], a = fl(float(S) / float(A 2^20)), y = clamp(fl(a u), -c, c): no
 * output exceeds c, and a stream that never reaches c passes as fl(g x) bit for bit.  As many outputs as inputs.  What a stream emits
 * does not depend on how its input was cut into pushes: a push emits every output whose A - 1 samples of look-ahead have arrived, the
 * flush emits the rest.
 * vv_level_set: configuration lv (0..3) of this context: A in [1,2047], H >= 0, H + 3 A - 3 < 8128, ceiling in (0,1], n_streams streams
 * at their first sample.  Replaces what lv held.  Synchronous. */
int vv_level_set(vv_ctx* ctx, int lv, int A, int H, float ceiling, int n_streams, void* stream);
/* Back to the state after vv_level_set for n streams (stream_ids_host == NULL: all of them): history zeroed by a kernel on `stream`,
 * input total 0, gain and flush mark cleared. */
int vv_level_reset(vv_ctx* ctx, void* stream, int lv, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, ONE launch on `stream`: row i = n_in samples at audio_dev + i * ld_in for stream rows_host[i].stream
 * (distinct) at gain rows_host[i].gain in (0,16] (a stream keeps the gain of its first push until its reset), flush != 0: the stream's
 * last push.  Its outputs go to out_dev + i * ld_out (elements): out_fmt 0 = fp32, 1 = int16 with the arithmetic of vv_audio_to_pcm16
 * over the row's own output (whose peak is <= ceiling <= 1: its rescale never fires).  n_out_host [n]: what each row emitted, computed
 * on the host from the streams' input totals (no sync).  Refused with a message, nothing written, no state changed: as
 * vv_resample_rows, a stream whose gain changes, and a row of more than 8128 - (H + 3 A - 3) input samples. */
typedef struct vv_level_row { int stream; int n_in; int flush; float gain; } vv_level_row;
int vv_level_rows(vv_ctx* ctx, void* stream, int lv, int n, const vv_level_row* rows_host, const float* audio_dev, int ld_in, void* out_dev,
                  int ld_out, int out_fmt, int* n_out_host);
/* Stateless: n whole signals of n_in samples (audio_dev + i * ld_in) -> n_in fp32 samples each (out_dev + i * ld_out).  Bit-identical
 * to the same signal pushed and flushed through vv_level_rows. */
int vv_level_once(vv_ctx* ctx, void* stream, int A, int H, float gain, float ceiling, int n, int n_in, const float* audio_dev, int ld_in,
                  float* out_dev, int ld_out);
/* ---- loudness: BS.1770 segment energies and a causal adaptive leveller at 24 kHz (vibevoice_amd/loudness.py defines them).  S = 2400
 * samples a segment, hq the 2400 integer taps of the K-weighting (impulse response times 2^24).  xq = rint(fl(clamp(x, -8, 8) 2^20)),
 * non-finite x: 0; z[i] = sum hq[k] xq[i - k], exact (|z| < 2^49, evaluated in fp64); zs = z >> 28; E[m] = sum of zs^2 over segment m:
 * E / (S 2^32) is the segment's mean square.  Leveller: a segment counts if E >= 120856803 (-50 LUFS); with M30 / c30 the sum and
 * number of the last <= 30 counted segments and M4 the sum of the last 4, w[m] = w[m-1] while c30 < 4, else
 * clamp(sqrt(t / max(float(M30 >> 8) / float(c30 S 2^24), float(M4 >> 8) / float(4 S 2^24))), 10^(-24/20), wmax), every operation one
 * fp32 rounding; w[-1] = w[-2] = g0; sample k of segment m: y = fl(fl(w[m-2] + fl(fl(w[m-1] - w[m-2]) fl(k / S))) x).  As many outputs
 * as inputs, none held back; what a stream emits does not depend on how its input was cut into pushes.
 * vv_loud_set: configuration ld (0..3) of this context: taps_host [2400] int32 = hq, n_streams streams at their first sample.  Replaces
 * what ld held.  Synchronous. */
int vv_loud_set(vv_ctx* ctx, int ld, const int* taps_host, int n_streams, void* stream);
/* Back to the state after vv_loud_set for n streams (stream_ids_host == NULL: all of them): inputs, energies and gains zeroed by a kernel
 * on `stream`, input total 0, parameters and flush mark cleared. */
int vv_loud_reset(vv_ctx* ctx, void* stream, int ld, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, TWO kernel launches on `stream` (the FIR over tiles of 320 samples x rows, then one workgroup per row that
 * closes segments and applies the gains): row i = n_in <= 3200 samples at audio_dev + i * ld_in for stream rows_host[i].stream
 * (distinct) with t = float32(10^((target + 0.691) / 10)) in (0,1), g0 in (0,16], wmax in [1,16] (a stream keeps the parameters of its
 * first push until its reset), flush != 0: the stream's last push (it emits nothing extra).  n_in fp32 outputs go to
 * out_dev + i * ld_out; n_out_host [n] = n_in.  Refused with a message, nothing written, no state changed: as vv_resample_rows, a stream
 * whose parameters change, a row of more than 3200 samples, and out_fmt = 1 (the stage is never the last one). */
typedef struct vv_loud_row { int stream; int n_in; int flush; float t; float g0; float wmax; } vv_loud_row;
int vv_loud_rows(vv_ctx* ctx, void* stream, int ld, int n, const vv_loud_row* rows_host, const float* audio_dev, int ld_in, void* out_dev,
                 int ld_out, int out_fmt, int* n_out_host);
/* Stateless: the energies E[i][m], m < n_in / 2400, of n whole signals of n_in samples (audio_dev + i * ld_in) as int64 at
 * energies_dev + i * ld_e, and the same sums at 16 times the resolution, F[i][m] = sum (z >> 24)^2 < 2^62 (F / (S 2^40) is the mean
 * square: what the meter reads, so that the floor of zs does not show at -60 LUFS), at fine_dev + i * ld_f.  Either pointer may be NULL,
 * not both.  taps_dev [2400]: hq as fp64 on the device; the call does not inspect it.  The bounds E < 2^54 and F < 2^62 (and the exactness
 * of z) are those of the K-weighting taps, sum |hq| = 3.25 2^24: vv_loud_set admits a tap sum up to 2^30 for the exactness of z in the
 * leveller alone, and a caller that passes other taps here owns the range of the int64 sums. */
int vv_loud_energy(vv_ctx* ctx, void* stream, const double* taps_dev, int n, int n_in, const float* audio_dev, int ld_in,
                   long long* energies_dev, int ld_e, long long* fine_dev, int ld_f);
/* Stateless: n whole signals of any length through the leveller -> n_in fp32 samples each (out_dev + i * ld_out) and, where gain_dev is
 * not NULL, the gain of every sample (gain_dev + i * ld_gain).  energies_dev [n][ld_e >= n_in / 2400]: room for the energies, which the
 * call leaves there.  Bit-identical to the same signal pushed through vv_loud_rows. */
int vv_loud_once(vv_ctx* ctx, void* stream, const double* taps_dev, float t, float g0, float wmax, int n, int n_in, const float* audio_dev,
                 int ld_in, float* out_dev, int ld_out, float* gain_dev, int ld_gain, long long* energies_dev, int ld_e);
/* ---- pauses: cap the silences of a stream and trim its lead-in, the last stage, at the delivered rate (vibevoice_amd/pause.py defines
 * it).  seg = rate / 100 samples a segment (80 .. 480).  q = clamp(rint(fl(x 32768)), +-32768), non-finite x: 0; E = sum of q^2 over
 * the segment (64-bit); the segment is quiet iff E < theta.  A cap is C segments (2^31 - 1: none): C0 for the quiet run in front of the
 * stream's first loud segment, C for every run behind it.  With the cap in force, T = min(C / 2, 10), H = C - T: the first H segments
 * of a quiet run go out as they arrive; from segment H + 1 on the stream holds the last T back and keeps a copy of segment H + 1
 * (`first`); the next loud segment, or the flush, releases them: verbatim where the run had R <= C segments (a stream with no run above
 * its cap passes bit for bit), else (R - C) seg samples are dropped and the oldest held segment b goes out joined,
 * fl(fl(first[j] u[j]) + fl(b[j] w[j])), w[j] = fl32((j + 0.5) / seg), u[j] = fl32(1 - (j + 0.5) / seg), the rest verbatim.  Samples
 * short of a segment wait for the next push; the flush releases what is held, then emits them.  What a stream emits does not depend on
 * how its input was cut into pushes; how much a push emits depends on the data, at most n_in + (seg - 1) + 10 seg.
 * vv_pause_set: configuration ps (0..3) of this context: seg in [80,480], weights_host [2][seg] = w, u, n_streams streams at their first
 * sample.  Replaces what ps held.  Synchronous. */
int vv_pause_set(vv_ctx* ctx, int ps, int seg, const float* weights_host, int n_streams, void* stream);
/* Back to the state after vv_pause_set for n streams (stream_ids_host == NULL: all of them): counters zeroed by a kernel on `stream`
 * (nothing held, no open run, totals 0), input total 0, parameters and flush mark cleared. */
int vv_pause_reset(vv_ctx* ctx, void* stream, int ps, int n, const int* stream_ids_host);
/* One push of n <= 16 rows, ONE launch on `stream`, one workgroup per row: row i = n_in <= 7680 samples at audio_dev + i * ld_in for
 * stream rows_host[i].stream (distinct) with seg (the configuration's), C, C0 >= 0 and theta >= 0 (a stream keeps the parameters of its
 * first push until its reset), flush != 0: the stream's last push.  Its outputs go to out_dev + i * ld_out (elements): out_fmt 0 =
 * fp32, 1 = int16 with the arithmetic of vv_audio_to_pcm16 over the row's own emitted samples.  n_out_dev [n], int32 in DEVICE memory:
 * what each row emitted, written by the launch; the host does not know it.  Refused with a message, nothing written, no state changed:
 * as vv_resample_rows, a stream whose parameters change, a row of more than 7680 samples, and ld_out < n_in + (seg - 1) + 10 seg. */
typedef struct vv_pause_row { int stream; int n_in; int flush; int seg; int C; int C0; long long theta; } vv_pause_row;
int vv_pause_rows(vv_ctx* ctx, void* stream, int ps, int n, const vv_pause_row* rows_host, const float* audio_dev, int ld_in, void* out_dev,
                  int ld_out, int out_fmt, int* n_out_dev);
/* totals_host [n][3]: the samples streams stream_ids_host[i] have taken, emitted and dropped.  Waits for `stream`. */
int vv_pause_totals(vv_ctx* ctx, void* stream, int ps, int n, const int* stream_ids_host, long long* totals_host);
/* Stateless: n whole signals of n_in samples (audio_dev + i * ld_in) -> at most n_in fp32 samples each (out_dev + i * ld_out);
 * weights_dev [2][seg] on the device; scratch_dev: scratch_floats fp32 on the device, at least n * 5760; counts_dev [n][2], int32 on the
 * device: what each signal emitted and what it dropped (their sum is n_in).  Bit-identical to the same signal pushed and flushed
 * through vv_pause_rows. */
int vv_pause_once(vv_ctx* ctx, void* stream, const float* weights_dev, int seg, int C, int C0, long long theta, int n, int n_in,
                  const float* audio_dev, int ld_in, float* out_dev, int ld_out, float* scratch_dev, long long scratch_floats, int* counts_dev);
/* acoustic_cache.set_to_zero + semantic_cache.set_to_zero for a slot (:542-546) */
int vv_codec_reset(vv_ctx* ctx, void* stream, int slot);
/* acoustic_connector(latent) [+ semantic_connector(sem)] (:667-669, :161); sem_dev may be NULL */
int vv_connect(vv_ctx* ctx, void* stream, int n, const float* latent_dev, const float* sem_dev,
               float* embeds_out_dev);

/* ---- low-level entry points (tests, microbenchmarks) */
/* pack a row-major fp32 [N][K] matrix into fragment tiles; dst needs vv_packed_bytes(N,K) */
int64_t vv_packed_bytes(int N, int K);
int vv_pack_matrix(void* stream, const float* src_dev, void* dst_dev, int N, int K);
/* The inverse of vv_pack_matrix for a linear matrix: packed bf16 tiles -> row-major fp32 dst_dev [N][K] (exact); padding is skipped.
 * packed_dev and dst_dev 16-byte aligned.  New surface (tests, vv_weight_read); the reference reads module.weight. */
int vv_unpack_matrix(void* stream, const void* packed_dev, float* dst_dev, int N, int K);
/* One launch of the LoRA merge kernel (lora.hip) on raw buffers: dst_packed = bf16(base_packed + scale * B.A) in the packed tile
 * layout, a_dev [r][K] and b_dev [N][r] fp32, 1 <= r <= 256, scale finite.  delta_bf16 = 0: peft's fp32 merge, delta = scale * (B.A)
 * in fp32 (rank index ascending, fused multiply-adds), one rounding of the product by scale and one of the sum with the base;
 * delta_bf16 = 1: a and b rounded to bf16 as they are read and the delta rounded to bf16 before the add (lora.merge_lora's two
 * merge_dtype paths).  Padding of edge tiles is copied from the base; dst_packed_dev == base_packed_dev is allowed.  A refusal
 * (bad sizes, null or misaligned pointers) returns < 0 before anything is launched; vv_last_error(NULL) has the text. */
int vv_lora_merge_raw(void* stream, const void* base_packed_dev, void* dst_packed_dev, int N, int K,
                      const float* a_dev, const float* b_dev, int r, float scale, int delta_bf16);
/* Y[T][N] = X[T][K] . W^T with the given prologue/epilogue ids (vv_common.h) */
int vv_gemm_raw(void* stream, const void* w_packed_dev, const void* w2_packed_dev, const float* x_dev,
                float* y_dev, int T, int N, int K, int ldx, int ldy, int pro, int epi,
                const float* nw_dev, float eps, const float* bias_dev, const float* nscale_dev,
                int xsplit, int ksplit, int nontemporal);
/* Exactly ONE launch of the decode GEMV kernel (gemv.hip: vv_gemv_kernel), or a refusal -- never another kernel in its place
 * (vv_gemm_raw goes through the dispatcher, which answers a shape the GEMV refuses with the tile or the general kernel).  The
 * struct carries every operand of the kernel (field meanings: VVGemm in csrc/vv_common.h); unused ones are 0 / NULL.  W / W2 are
 * vv_pack_matrix outputs.  Returns 0 after the launch, VV_GEMV_REFUSED (nothing was launched: the eligibility check said no, or
 * there is no instantiation for this pair / row count / xsplit), < 0 on a bad xsplit or a launch error.  form_out (optional)
 * receives {XS, MR rows, WPB waves, PARTS (0 none, 1 activation side, 2 residual side), SL (1 = slot-batched)} of the instantiation
 * that ran, as decided by the launcher itself.  The caller vouches for the sizes of every buffer (Engine.gemv_case checks them).
 * New surface (tests); the reference has no native code. */
#define VV_GEMV_REFUSED 1
typedef struct vv_gemv_case_args {
    const void* W; const void* W2; const float* X; float* Y;
    int T, N, K, ldx, ldy;
    int pro, epi;
    const float* nw; float eps; const float* bias; const float* nscale;
    const float* mod_scale; const float* mod_shift; int ld_mod;
    const float* addvec; int x_row_mod, add_rows_per_vec;
    const float* gate; int ld_gate;
    float* z; float* x0p; const float* coef; float cfg; int n_cfg; const float* sde_noise;
    int kgrid; float* yparts; const float* xa; int n_xa; const float* ya; int n_ya; int part_stride;
    int sl_n, sl_T, sl_x, sl_y; int sl_id[8];
    const float* dw_hist; const float* dw_w; const float* dw_b; const float* dw_gamma; const float* dw_nw;
    float* dw_xout; float* dw_hnew;
    const float* cfg_rows;      /* VV_EPI_CFG_DPM: [n_cfg] one guidance scale per utterance row, or NULL (cfg for every row) */
} vv_gemv_case_args;
int vv_gemv_case(void* stream, const vv_gemv_case_args* args, int xsplit, int* form_out);
/* W13: the lossless 13-bit twin of a packed bf16 matrix (format: vibevoice_amd/w13.py, csrc/vv_w13.h), N % 16 == 0, K % 128 == 0.
 * vv_w13_twin_bytes: size of a twin (planes, then per tile row a scale word and an ok word, then the folded ok word), 0 for a shape
 * without one.  vv_w13_pack_matrix: packed_dev (a vv_pack_matrix output) -> twin_dev; the kernel decodes what it wrote and compares
 * it with the source bit for bit -- that is the ok word.  vv_w13_unpack_matrix: twin_dev -> packed fragments (the same decoder).
 * vv_w13_gemv_case: ONE launch of the W13 form (mr rows, wpb waves; csrc/gemv_plan.h: vv_gemv_w13_forms) on the operands of args:
 * over the twins (twin_dev, twin2_dev for SwiGLU's second matrix), or with twin_dev == NULL the same form over the bf16 fragments --
 * the two must agree bit for bit; args' W / W2 stay the bf16 fragments either way, and a tile row whose ok word in the twin is 0 streams
 * them inside the same launch.  Returns VV_GEMV_REFUSED where the form or the shape does not exist.  New surface (tests); the engine
 * keeps twins of the diffusion head's gate / up / down matrices and of every LM layer's QKV / o / gate / up / down matrices itself
 * (VVHIP_W13=head: the head's alone; VVHIP_W13=0: none). */
int64_t vv_w13_twin_bytes(int N, int K);
int vv_w13_pack_matrix(void* stream, const void* packed_dev, void* twin_dev, int N, int K);
int vv_w13_unpack_matrix(void* stream, const void* twin_dev, void* packed_dev, int N, int K);
int vv_w13_gemv_case(void* stream, const vv_gemv_case_args* args, const void* twin_dev, const void* twin2_dev, int mr, int wpb);
/* Exactly ONE launch of the batch-decode packed GEMV (gemv16p.hip: vv_gemv16p_kernel) through its own launcher, or a refusal.  The
 * struct mirrors VVGemv16p (csrc/vv_common.h, field meanings there); unused operands are 0 / NULL.  W / W2 are vv_pack_matrix
 * outputs; Xp / Xs are ONE packed 16-row activation tile each (the layout of a 16-row weight tile: ceil(K / 32) KiB); Yp is one such
 * tile of the N output features.  epi: VV_EPI_* of vv_common.h (0 / 1 bias or store, 3 SwiGLU, 4 residual, 5 gated residual,
 * 6 CFG + solver update); flags: 1 = RS (row scale from ssq_in), 2 = SH (second operand Xs), 4 = PK (the residual epilogue also
 * packs the new rows and writes their sums of squares).  Returns 0 after the launch, VV_GEMV_REFUSED (nothing was launched: the
 * shape, a missing operand, or a (epi, flags) pair without an instantiation), < 0 on a launch error.  wpb_out (optional) receives
 * the waves per workgroup the launcher chose (4 or 8).  The caller vouches for the sizes of every buffer (Engine.gemv16p_case
 * checks them).  New surface (tests), like vv_gemv_case; the engine reaches the kernel through its passes. */
typedef struct vv_gemv16p_case_args {
    const void* W; const void* W2; const void* Xp; float* Y; void* Yp; const float* bias; const float* gate;
    int T, N, K, ldy, ld_gate;
    const float* ssq_in; int ssq_tiles; float eps;
    const void* Xs;
    const float* pk_nw; const float* pk_sc; int ld_pk; float* ssq_out;
    float* z; float* x0p; const float* coef; float cfg; int n_cfg; const float* sde_noise;
    const float* cfg_rows;
} vv_gemv16p_case_args;
int vv_gemv16p_case(void* stream, const vv_gemv16p_case_args* args, int epi, int flags, int* wpb_out);
/* One launch of the activation packers of gemv16p.hip, or a refusal (VV_GEMV_REFUSED, nothing launched).  vv_pack16_case: rows
 * x_dev [T][ldx] fp32 (T <= 16, K % 32 == 0, K <= 8192) -> one packed 16-row tile xp_dev (K / 32 KiB, rows >= T zero); mode 1:
 * RMSNorm with weight nw_dev (NULL: none), mode 2: adaLN-modulated RMSNorm, x^ = rs x nw (1 + sc) + sh with sc_dev / sh_dev rows of
 * stride ld_mod.  vv_pack16_tiles_case: n_tiles plain bf16 conversions in one launch; tile j reads rows at x_dev + (j / n_inner) *
 * stride_outer + (j % n_inner) * stride_inner (floats, row stride ldx) and writes xp_dev + j * tile_bytes.  New surface (tests). */
int vv_pack16_case(void* stream, const float* x_dev, int ldx, int mode, const float* nw_dev, float eps, const float* sc_dev,
                   const float* sh_dev, int ld_mod, void* xp_dev, int T, int K);
int vv_pack16_tiles_case(void* stream, const float* x_dev, int ldx, int64_t stride_outer, int n_inner, int64_t stride_inner,
                         void* xp_dev, int64_t tile_bytes, int T, int K, int n_tiles);
/* The prompt-prefill GEMM (bf16-activation mode): x_dev fp32 [T][K] is packed (RMS-normalised when nw_dev != NULL) into
 * xp_scratch (vv_packed_bytes(T, K)); epi 0/1/4 (store / bias / residual) -> fp32 y_dev [T][N]; epi 3 (SwiGLU: w = gate,
 * w2 = up) -> packed bf16 in yp_scratch (vv_packed_bytes(T, N), zero-initialised), unpacked into y_dev.  K % 8 == 0, N % 4 == 0.
 * ctx lends its K-split workspace (the partial last round of the 256 x 256 kernel is split along K, as in the prompt prefill);
 * ctx == NULL: every tile is computed whole. */
int vv_gemm3_raw(vv_ctx* ctx, void* stream, const void* w_packed_dev, const void* w2_packed_dev, const float* x_dev, int T, int N, int K,
                 int epi, const float* nw_dev, float eps, const float* bias_dev, float* y_dev, void* xp_scratch, void* yp_scratch);
/* hipEvent timing of every GEMM launch issued between begin and end (graphs are bypassed meanwhile):
 * number of launches, summed kernel time, summed algorithmic bytes (packed weights once + activations
 * in + result out).  Each output is a 2-element array: [0] the decode kernel vv_gemv_kernel with T <= 4,
 * [1] the general vv_gemm_kernel.  Used by bench.py's roofline. */
int vv_profile_begin(vv_ctx* ctx);
int vv_profile_end(vv_ctx* ctx, int64_t* launches, double* total_ms, double* bytes);
/* The vv_gemv_kernel launches recorded by the last begin/end window, captured in issue order into one hipGraph and replayed
 * `reps` times between two events on `stream`: launches = recorded x reps, total_ms, algorithmic bytes.  total_ms/launches
 * is the start-to-start period of a GEMV launch inside a dependent graph chain (kernel + boundary) -- the execution mode of
 * the timed region, and what rocprofv3 --kernel-trace reports per kernel under graph replay.  Clobbers engine scratch and
 * streaming-codec state: call it last. */
int vv_profile_replay(vv_ctx* ctx, void* stream, int reps, int64_t* launches, double* total_ms, double* bytes);
/* The same replay for the other timed kernel families of the window: family 0 = the GEMV kernel as above, 1 = vv_gemv16p_kernel,
 * the packed-activation projections of batch decode with 5..16 rows, 2 = decode attention: vv_attn_fused_kernel and, for contexts
 * split over several workgroups, its vv_attn_merge2_kernel: one unit per layer; algorithmic bytes = every cached position's K and
 * V once.  launches = 0 when the window recorded none of that family.  bench.py's roofline for batch decode and for the
 * attention kernels. */
int vv_profile_replay_family(vv_ctx* ctx, void* stream, int family, int reps, int64_t* launches, double* total_ms, double* bytes);
/* what = 0: kernel launches issued by the last engine call (graph nodes when replayed); 1: hipGraph executables cached; 2 / 3: raw
 * timings of the last profile window; 4: stream captures that did not close cleanly and were run eagerly instead (seen when
 * several host threads drive several contexts: another thread's activity can invalidate a capture; the result is unaffected);
 * 5: nodes of the captured graphs that are not kernel launches -- 0 by construction: copies and fills inside captured sequences are
 * kernels of the library, because a memset node of a replayed graph was seen to fill with stale words;
 * 6: head-tail seam launches (headtail.hip: final layer + CFG + solver update + the next step's in-projection in one launch) that
 * the last recorded sampler body issued -- n_steps - 1 for one utterance in bf16 mode, 0 where the two-launch form ran; a graph
 * replay keeps the count of its capture;
 * 7: bytes of device memory held by the base snapshots of LoRA-merged parameters (vv_lora_merge);
 * 8: step ends of the general sampler (vv_diffusion_sample_general) that carried the next step's in-projection in the same launch,
 * in the last recorded sampler body -- n_steps - 1 where solver.hip's rule holds, 0 where the update ran alone;
 * 9: matrices of the diffusion head (gate, up and down of every layer) whose W13 twin decoded exactly on the device in every tile row;
 * gate and up of a layer count together or not at all.  0 with VVHIP_W13=0, in the exact modes and at widths without whole groups.
 * (A matrix that does not count still streams its twin: the tile rows that are not exact read bf16 inside the same launch.);
 * 10: matrices of the LM (QKV, o, gate, up and down of every layer) that have a W13 twin: 5 x layers, or 0 with VVHIP_W13=head or 0, in
 * the exact modes and for a matrix without whole groups;
 * 11: tile rows (16 output features) of all twinned matrices, head and LM, that stream bf16 because the format cannot hold one of
 * their elements (or because the matrix was never uploaded).  9 and 11 wait for the device and read the twins' ok words back */
int64_t vv_stat(vv_ctx* ctx, int what);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
