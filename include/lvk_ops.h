/* include/lvk_ops.h -- operator-level C ABI of llama.vk_amd (secondary boundary).
 *
 * The reference exposes its quantization codecs through quantize_fns_t /
 * ggml_internal_get_quantize_fn (reference ggml.h:803-814, ggml.c:6489-6508)
 * and its ops through the ggml graph API (ggml.h:500-611).  These entry points
 * run the corresponding MI355X kernels on host buffers (H2D, kernel, D2H) so
 * each op can be pinned against the CPU oracle in isolation.  `type` is the
 * ggjt ftype id: 2 = Q4_0, 3 = Q4_1.  All functions return 0 on success and a
 * negative value on failure (message on stderr).
 */
#ifndef LVK_OPS_H
#define LVK_OPS_H

#include <stddef.h>
#include <stdint.h>

#define LVK_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

/* number of visible GPUs (0 when none); never fails */
LVK_API int lvk_device_count(void);
/* select the HIP device for subsequent contexts/ops of this host thread (hipSetDevice) */
LVK_API int lvk_set_device(int dev);
/* version string of the library */
LVK_API const char * lvk_version(void);

/* quantize_row_q (ggml.c:621-685 / 847-920): x[n][k] -> n rows of blocks in
 * the reference block layout (20 / 24 bytes per 32 values) */
LVK_API int lvk_quantize_rows(int type, const float * x, int n, int k, void * y);

/* y[t][r] = vec_dot_q(k, w_row r, quantize_row_q(x[t]))  for r < m, t < n
 * (ggml_compute_forward_mul_mat_q_f32, ggml.c:6510-6696).  w: m rows in the
 * file block layout. */
LVK_API int lvk_mul_mat_q(int type, const void * w, int m, int k, const float * x, int n, float * y);

/* same with the fused RMSNorm prologue: y[t][r] = dot(w_r, quant(g * rms_norm(x[t]))) */
LVK_API int lvk_mul_mat_q_norm(int type, const void * w, int m, int k, const float * g, const float * x, int n,
                               float * y);

/* The prompt-batch (N > 1) matmul on the MFMA cores (mm_mfma.hip for Q4_0,
 * mm_mfma41.hip for Q4_1): same inputs and meaning as lvk_mul_mat_q /
 * lvk_mul_mat_q_norm (g != NULL: fused RMSNorm * g), and the same result bits:
 * the matrix cores produce each AVX2 chain's exact 4-element integer partial
 * (Q4_1 also the exact cross-term sums) and the f32 scale products (one rounding
 * each), and the VALU runs the reference's 8 fp32 chains and horizontal order
 * (ggml.c:1950-2026 / 2188-2258).  Needs m % 128 == 0, k % 256 == 0, n >= 1. */
LVK_API int lvk_mul_mat_q_mfma(int type, const void * w, int m, int k, const float * g, const float * x, int n,
                               float * y);

/* f16 weights (ggml type 1): y[t][r] = ggml_vec_dot_f16(k, w_r, f16(a[t])) with a = x, or
 * a = g * rms_norm(x) when g != NULL, exactly as ggml_compute_forward_mul_mat_f16_f32 (AVX2)
 * computes it.  w: m rows of k f16 values in file layout; k % 256 == 0, any m >= 1, n >= 1.
 * kernel: 0 = the kernel a context would choose (n == 1: the decode matvec, else the batched
 * matmul), 1 = the decode matvec (matvec_f16.hip, n == 1 only), 2 = the batched matmul
 * (mm_f16.hip).  Any other combination returns nonzero. */
LVK_API int lvk_mul_mat_f16(const uint16_t * w, int m, int k, const float * g, const float * x, int n, float * y,
                            int kernel);

/* f32 weights (ggml type 0): y[t][r] = ggml_vec_dot_f32(k, w_r, a[t]) with a = x, or
 * a = g * rms_norm(x) when g != NULL, exactly as ggml_compute_forward_mul_mat_f32 (AVX2)
 * computes it.  w: m rows of k f32 values in file layout; k % 256 == 0, any m >= 1, n >= 1.
 * kernel: 0 = the kernel a context would choose (n == 1: the decode matvec, else the batched
 * matmul), 1 = the decode matvec (matvec_f32.hip, n == 1 only), 2 = the batched matmul on the
 * f32 matrix cores (mm_f32.hip).  Any other combination returns nonzero. */
LVK_API int lvk_mul_mat_f32(const float * w, int m, int k, const float * g, const float * x, int n, float * y,
                            int kernel);

/* one layer's attention block on an f16 KV cache (llama.cpp:1010-1061):
 * kc [n_ctx][n_embd] f16, vc [n_embd][n_ctx] f16, q [n][n_embd] f32 (post-RoPE)
 * -> out [n][n_embd] f32 (merged heads, before the Wo quantization) */
LVK_API int lvk_attention(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                          int n_ctx, int n_past, int n, float * out);

/* lvk_attention plus the pre-softmax scores [n][n_head][n_ctx] (scaled, -inf where masked), followed in
 * scores_out by the f16 probabilities [n][n_head][n_ctx] (so scores_out holds 1.5x that many floats) */
LVK_API int lvk_attention_scores(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                                 int n_ctx, int n_past, int n, float * out, float * scores_out);

/* lvk_attention through the prompt-batch kernels (attention_prompt.hip: scores +
 * softmax per 32 query tokens, P.V per 32-dim slice); same result bits.  Needs
 * head_dim 128, n_ctx % 32 == 0, n_ctx <= 1024. */
LVK_API int lvk_attention_prompt(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                                 int n_ctx, int n_past, int n, float * out);

/* lvk_attention for one token (n = 1) through the decode kernels
 * (attention_decode.hip: scores per 64 positions, softmax + P.V per 32-dim
 * slice); same result bits.  Needs head_dim 128, n_ctx % 64 == 0, n_ctx <= 2048. */
LVK_API int lvk_attention_decode(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                                 int n_ctx, int n_past, float * out);

/* Score-helper workgroups per head that a decode-attention launch of this shape runs on the
 * current device (attention_decode.hip): 4 when n_head * 8 <= compute units, else 0; 0 as well
 * with env LVK_ATTN_HELPERS=0 (read once per process) or for a shape the decode kernels do
 * not take. */
LVK_API int lvk_attn_helpers_active(int n_embd, int n_head, int n_ctx);

/* lvk_attention (kind 0), lvk_attention_prompt (kind 1) or lvk_attention_decode (kind 2, n = 1)
 * with the kernel's fused Wo quantizer exposed: type 2 (Q4_0) or 3 (Q4_1) selects the quantizer,
 * blocks (optional) receives the quantized Wo input, n rows of n_embd/32 blocks in the reference
 * block layout (20 / 24 bytes), i.e. quantize_row_q of each out row.  kinds 1 and 2 keep the shape
 * limits of their functions; every kind needs head_dim 128, n >= 1, 0 <= n_past <= n_ctx - n. */
LVK_API int lvk_attention_q(int kind, int type, const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd,
                            int n_head, int n_ctx, int n_past, int n, float * out, void * blocks);

/* The two kernels of a batched decode layer (attention_rows.hip) on host data.  A cache argument
 * is a host array [n_slots][n_layer][n_ctx * n_embd] of f16 bits (K [n_ctx][n_embd], V
 * [n_embd][n_ctx] per slot and layer); slot s is handed to the kernel as its base and the launch
 * gets the element offset of `layer`.  Row i belongs to slot slots[i] at position pos[i].  Every
 * argument is checked on the host before anything is uploaded: a slot outside 0..n_slots-1, a
 * position outside 0..n_ctx-1, layer outside 0..n_layer-1, n < 1, a shape other than head_dim 128,
 * n_ctx % 32 == 0, n_ctx >= 128, or a bad type returns -1 with a message and launches nothing.
 *
 * lvk_rope_kv_rows: k_rope_kv_rows.  qkv [n][3 * n_embd] f32 (stored Q|K|V rows).  Row i is RoPE'd
 * at pos[i] (the table a context builds); its K and V are written at pos[i] of slot slots[i],
 * layer `layer`.  kc and vc are read and written in place (whole arrays, up and back).  q16_out is
 * [n][n_embd] f16 bits.
 *
 * lvk_attention_rows: k_attn_rows<type>, type 2 (Q4_0) or 3 (Q4_1).  q [n][n_embd] f32 post-RoPE,
 * converted to f16 on the host as lvk_attention does.  Row i attends over pos[i] + 1 positions of
 * slot slots[i], layer `layer`, nothing masked.  out is [n][n_embd] f32; blocks (optional): the
 * quantized Wo input, n rows of n_embd/32 blocks in the reference block layout (20 / 24 bytes). */
LVK_API int lvk_rope_kv_rows(const float * qkv, const int * slots, const int * pos, int n, int n_embd, int n_head,
                             int n_ctx, int n_slots, int n_layer, int layer, uint16_t * kc, uint16_t * vc,
                             uint16_t * q16_out);
LVK_API int lvk_attention_rows(int type, const uint16_t * kc, const uint16_t * vc, int n_slots, int n_layer, int layer,
                               const float * q, const int * slots, const int * pos, int n, int n_embd, int n_head,
                               int n_ctx, float * out, void * blocks);

/* The fused steps of a transformer layer as a context launches them (lvk_context.cpp
 * enqueue_forward), each on host data: weights in file layout, f32 rows in, results out.
 * type is the weight type (0 f32, 1 f16, 2 Q4_0, 3 Q4_1).  path selects the launcher:
 *   0  what a context chooses for this n (n == 1: launch_matvec_auto; a batch: the generic kernels
 *      for Q4 below 16 tokens, else the batched route)
 *   1  launch_matvec_cu (n == 1: matvec_cu.hip / matvec_cu41.hip, or the one f16 / f32 matvec)
 *   2  launch_matvec (the generic kernels of matvec_q4.hip / matvec_q41.hip, any n; f16 / f32: n == 1)
 *   3  the batched route: launch_act (or launch_actq_to_image) + launch_mm
 * Every argument is checked on the host before anything is uploaded (k % 256 == 0, 1 <= n <= 4096,
 * path 1 with n > 1, null pointers, the limits named below): -1 with a message on stderr, nothing
 * launched.  A (path, type, shape) a launcher has no kernel for returns -1 as well (its
 * hipErrorNotSupported / hipErrorInvalidValue), with nothing written to the outputs.  The Q4 weight
 * images are built as the model loader builds them, for path 3 including the prompt images
 * (Q4_1 always, Q4_0 unless LVK_PROMPT_A16=0); the Q4 batched matmul needs 128 | rows.
 *
 * lvk_layer_qkv: q | k | v = W . quant(g * rms_norm(x[t])) for the n rows of x [n][k]; w is
 * [3 * n_embd][k] (wq, wk, wv rows).  Row t is RoPE'd at n_past + t; q16_out [n][n_embd] receives
 * the f16 queries, row n_past + t of kc ([n_ctx][n_embd] f16 bits) the keys and column n_past + t
 * of vc ([n_embd][n_ctx]) the values.  kc / vc go up and come back whole.  fused = 1: EPI_QKV (paths
 * 1, 2) or EPI_ROPE_KV (path 3, Q4 only); fused = 0: EPI_STORE, then launch_rope_kv.  n_embd is
 * independent of k (the kernels read it in the epilogue only); n_embd % 32 == 0, head_dim % 4 == 0,
 * n_ctx <= 16384, 0 <= n_past <= n_ctx - n.  f16 KV only.
 *
 * lvk_layer_resid: y[t] += W . conv(a[t]), w [m][k], a [n][k] f32, y [n][m] in / out.  input = 0:
 * the kernel converts the f32 rows (PRO_ACTF: the W2 role of the CU kernels, f16, f32; launch_act
 * on path 3); input = 1 (Q4 only): a is quantized by launch_quantize_act and handed over as
 * PRO_ACTQ (the Wo role; launch_actq_to_image on path 3).  Every EPI_RESID kernel needs m % 8 == 0.
 *
 * lvk_layer_swiglu: u[t] = silu(W1 . a[t]) * (W3 . a[t]) with a = quant(g * rms_norm(x[t])), w1 / w3
 * [f][k] each, interleaved per 4 rows as the loader fuses them.  Paths 1 and 3 give u_out [n][f]
 * f32 (EPI_SWIGLU_F32), path 2 (Q4 only, f % 32 == 0) blocks_out, n rows of f / 32 blocks of
 * quantize_row_q(u[t]) in the reference block layout (EPI_SWIGLU); the other output must be NULL.
 *
 * lvk_layer_ffn: the batch FFN pair, x[t] += W2 . conv(u[t]) with u as above; x [n][k] in / out,
 * w2 [k][f], f % 256 == 0.  swiglu_q = 1 (Q4_0 only): EPI_SWIGLU_Q writes W2's operand image in the
 * W1|W3 epilogue; swiglu_q = 0: EPI_SWIGLU_F32, launch_act, then EPI_RESID.
 *
 * lvk_embed_rows: x_out[i] = the dequantized / widened row tokens[i] of emb [n_vocab][n_embd] (file
 * layout; launch_embed), every token in 0..n_vocab-1, n_embd % 32 == 0. */
LVK_API int lvk_layer_qkv(int type, int path, const void * w, int n_embd, int n_head, int k, const float * g,
                          const float * x, int n, int n_ctx, int n_past, int fused, uint16_t * kc, uint16_t * vc,
                          uint16_t * q16_out);
LVK_API int lvk_layer_resid(int type, int path, const void * w, int m, int k, const float * a, int n, int input,
                            float * y);
LVK_API int lvk_layer_swiglu(int type, int path, const void * w1, const void * w3, int f, int k, const float * g,
                             const float * x, int n, float * u_out, void * blocks_out);
LVK_API int lvk_layer_ffn(int type, const void * w1, const void * w3, const void * w2, int f, int k, const float * g,
                          float * x, int n, int swiglu_q);
LVK_API int lvk_embed_rows(int type, const void * emb, int n_vocab, int n_embd, const int * tokens, int n,
                           float * x_out);

/* Self-check of the softmax exp: the number of arguments h <= 0 (fp16 bits)
 * where the device's computed fp16(exp(h)) differs from this host's
 * table_exp_f16[h] (ggml.c:2915-2927) -- 0 when the device expf reproduces it,
 * else the count of the double-precision exp.  Contexts compute exp only in a
 * mode with 0 mismatches (env LVK_EXP_TABLE forces the table).  -1 on error. */
LVK_API int lvk_exp_table_mismatches(void);

/* y[t] = g * rms_norm(x[t]) (ggml.c:6024-6080 + llama.cpp:984) */
LVK_API int lvk_rms_norm_mul(const float * x, const float * g, int k, int n, float * y);

/* the 64Ki-entry fp16 exp / silu tables the library uploads (ggml.c:2915-2927) */
LVK_API void lvk_host_tables(uint16_t * exp_tab, uint16_t * silu_tab);

/* decode-step profiling of a llama_context: when enabled, every eval records
 * HIP events around each kernel class (0 embed, 1 qkv, 2 attention, 3 wo,
 * 4 w1|w3, 5 w2, 6 lm_head) and accumulates device ms, launches and algorithmic
 * weight bytes. */
struct llama_context;
LVK_API void lvk_set_profiling(struct llama_context * ctx, int on);
LVK_API int lvk_get_profile(struct llama_context * ctx, double * ms, long * launches, double * bytes, int n);
LVK_API void lvk_reset_profile(struct llama_context * ctx);
/* bytes of quantized weights resident in HBM for this context's model */
LVK_API size_t lvk_weight_bytes(struct llama_context * ctx);
/* bytes of the prompt matmul's f16 A-fragment images (+ the Q4_1 side images) resident in
 * HBM; 0 when they were not built (LVK_PROMPT_A16=0, or too little free memory at load) */
LVK_API size_t lvk_prompt_image_bytes(struct llama_context * ctx);
/* 1 = prompt batches (N > 1) use the bit-faithful VALU matmuls (the reference's
 * exact fp32 chain order), 0 = the MFMA matmuls (default; env LVK_PROMPT_EXACT=1
 * makes 1 the default) */
LVK_API void lvk_set_prompt_exact(struct llama_context * ctx, int on);
/* 1 = replay the captured decode graph for single-token evals (default), 0 = eager */
LVK_API void lvk_set_graph(struct llama_context * ctx, int on);
/* On-device greedy sampling.  lvk_eval_greedy(ctx, token, n_past)
 * is llama_eval(ctx, &token, 1, n_past, .) followed by
 * llama_sample_top_p_top_k(ctx, ., ., ., ., temp <= 0) (llama.cpp:1703-1719,
 * 1382-1394): the argmax runs over the logits in HBM and only the 4-byte token
 * crosses PCIe.  Returns the next token id, or -1 on error (message on stderr).
 * The host logits of llama_get_logits are NOT refreshed by this call.
 * lvk_argmax(x, n) is the op-level kernel on a host array: the first index whose
 * value is strictly greater than all earlier ones (0 when x[0] is NaN). */
LVK_API int lvk_eval_greedy(struct llama_context * ctx, int token, int n_past);
/* n_steps decode steps in one call: step i evaluates token t_i at position n_past + i, with
 * t_0 = tokens[0], t_{i+1} = tokens[i + 1] while i + 1 < n_tokens (a teacher-forced sequence,
 * 1 <= n_tokens <= n_steps) and the argmax of step i's logits after that (n_tokens = 1: greedy).
 * out_tokens[i] is the argmax of step i's logits (what lvk_eval_greedy(ctx, t_i, n_past + i)
 * returns); out_digests (optional, may be NULL) receives lvk_logits_digest of step i's logits
 * row, computed on the device, so a caller can check every step's logits without copying them.
 * The KV cache ends as after the n_steps single-token evals.  The steps run as back-to-back
 * replays of one decode graph whose last kernel picks the next token, advances the step block and
 * writes the next embedding row on the device, so nothing crosses PCIe between steps.
 * n_past + n_steps <= n_ctx.  Returns 0, or -1 on error (layer splits and logits_all contexts
 * refuse it).  The host logits of llama_get_logits are NOT refreshed. */
LVK_API int lvk_decode_chain(struct llama_context * ctx, const int * tokens, int n_tokens, int n_past, int n_steps,
                             int * out_tokens, uint64_t * out_digests);
/* lvk_decode_chain(ctx, &token, 1, n_past, n_steps, out_tokens, NULL) */
LVK_API int lvk_decode_greedy(struct llama_context * ctx, int token, int n_past, int n_steps, int * out_tokens);
/* digest of a logits row: sum over k (mod 2^64) of splitmix64((k << 32) | bits(x[k])) -- position
 * sensitive, order independent, equal for two rows only if (almost surely) bit-identical */
LVK_API uint64_t lvk_logits_digest(const float * x, int n);
/* On-device sampling: lvk_eval_sample(ctx, token, n_past, last_n, n_last,
 * top_k, top_p, temp, repeat_penalty) returns what llama_eval(ctx, &token, 1, n_past, .)
 * followed by llama_sample_top_p_top_k(ctx, last_n, n_last, top_k, top_p, temp,
 * repeat_penalty) returns (llama.cpp:1356-1459, 1703-1719, 1777-1805), drawing from the same
 * mt19937 stream.  The repeat penalty, the temperature and the top-k selection run over the
 * logits in HBM (sample.hip); only the candidates >= the k-th value cross PCIe and the host
 * finishes the reference's softmax / top-p / discrete_distribution over k values.  Ties among
 * the candidates, NaN logits, top_k <= 0 or > 1024, a last-n window > 1024, split or
 * logits_all contexts take the reference path over all logits (same result, slower).
 * temp <= 0 is lvk_eval_greedy.  The host logits of llama_get_logits are NOT refreshed
 * (except on the all-logits path).  Returns the token, or -1 on error. */
/* op-level device candidate selection on a host array (sample.hip): the values the reference
 * sorts (x[i] / temp, with the repeat penalty for ids in last[]), every one >= the k-th largest
 * written to vals/ids (arbitrary order, up to 1024), *flags bit 1 = NaN seen, bit 2 = more than
 * 1024 candidates.  Returns the candidate count, -1 on bad arguments. */
LVK_API int lvk_sample_candidates(const float * x, int n, const int * last, int n_last, int k, float temp, float rp,
                                  float * vals, int * ids, int * flags);
LVK_API int lvk_eval_sample(struct llama_context * ctx, int token, int n_past, const int * last_n, int n_last,
                            int top_k, float top_p, float temp, float repeat_penalty);
LVK_API int lvk_argmax(const float * x, int n);

/* Device-side KV state (the host-bytes form is llama_get_kv_cache /
 * llama_set_kv_cache, llama.cpp:1678-1701): copy positions [0, n_tokens) of every
 * layer's K and V from src to dst in HBM (same model shape and n_ctx, same device) and
 * set dst's KV token count to n_tokens.  dst can then continue with
 * llama_eval(dst, ., ., n_past = n_tokens, .) exactly as src would.  0 / -1. */
LVK_API int lvk_kv_copy(struct llama_context * dst, struct llama_context * src, int n_tokens);

/* Batched decode: several sequences per step on one context, one stream of the weights per step.
 * A context has n_seq KV slots.  Slot 0 is the context's own cache: llama_eval, lvk_eval_greedy /
 * _sample, lvk_decode_chain, llama_get/set_kv_cache and lvk_kv_copy act on it as ever, and its
 * token count is llama_get_kv_cache_token_count (an eval of n tokens at n_past leaves n_past + n).
 * Slots 1..n_seq-1 are further caches of the same layout, zeroed.
 *
 * lvk_decode_batch evaluates n rows (tokens[i], seqs[i], pos[i]).  Row i is computed exactly as
 * llama_eval(ctx', &tokens[i], 1, pos[i], .) computes it on a context whose cache holds sequence
 * seqs[i]: RoPE at pos[i], K / V appended at pos[i] of slot seqs[i], attention over pos[i] + 1
 * positions with nothing masked (not the reference's N-token batch, whose columns all run over
 * n_past + N).  Every logits row is bit-identical to that single-token eval, for Q4_0, Q4_1, f16
 * and f32 model files.  Rows of one sequence in a call have consecutive ascending positions and
 * behave like that many single-token evals in order; a sequence's first position in a call is
 * <= its token count (rewinding is allowed, holes are not), and its count afterwards is its
 * last position + 1.
 * Layer-split contexts, stage contexts and contexts with the f32 KV cache (f16_kv = false)
 * refuse lvk_seq_init: the f32 KV cache has no batched decode. */
/* allocate slots 1..n_seq-1 (n_seq >= 1; calling again with a larger n_seq grows, smaller is a no-op). 0 / -1;
 * on failure (out of memory, split / stage context, f16_kv = false) the context is unchanged and usable */
LVK_API int lvk_seq_init(struct llama_context * ctx, int n_seq);
LVK_API int lvk_seq_count(struct llama_context * ctx);                 /* slots (1 before lvk_seq_init) */
LVK_API int lvk_seq_tokens(struct llama_context * ctx, int seq);       /* positions held by a slot, -1 on a bad id */
/* copy positions [0, n_tokens) of every layer's K and V from slot src to slot dst (device copy), set dst's count;
 * n_tokens <= src's count */
LVK_API int lvk_seq_copy(struct llama_context * ctx, int dst, int src, int n_tokens);
/* n rows (1 <= n <= n_ctx): see above.  logits (optional): [n][n_vocab] floats, row order;
 * argmax (optional): [n] ints, the reference's first-maximum rule per row, taken on the device.
 * Every argument is checked before anything is enqueued; 0, or -1 with a message on stderr and the
 * context and every slot unchanged.  llama_get_logits is NOT refreshed.  The rows count into the
 * eval timings. */
LVK_API int lvk_decode_batch(struct llama_context * ctx, const int * tokens, const int * seqs, const int * pos, int n,
                             float * logits, int * argmax);
/* n_steps batched decode steps in one call.  Row r (0 <= r < n) is sequence seqs[r], starting at
 * position pos[r].  Step i evaluates, for every row, token t_i[r] at position pos[r] + i on slot
 * seqs[r], exactly as lvk_decode_batch would with those n rows.  t_0[r] = forced[r];
 * t_{i+1}[r] = forced[(i + 1) * n + r] while i + 1 < n_forced (1 <= n_forced <= n_steps), else the
 * argmax (first-maximum rule) of row r's logits of step i.
 * out_tokens[i * n + r]: that argmax.  out_digests (optional): lvk_logits_digest of that logits row.
 * logits (optional): the last step's [n][n_vocab].
 * Nothing crosses PCIe between steps: the steps are replays of one captured graph whose last
 * kernel picks every row's next token, writes its embedding row and advances the row's position
 * on the device (with lvk_set_graph(ctx, 0) or the profiler on, the same launches enqueued
 * eagerly).  Every result is bit-identical to the same rows fed step by step through
 * lvk_decode_batch.
 * 1 <= n <= n_ctx; every slot at most once per call (one row per sequence); 0 <= pos[r] <= the
 * slot's count (rewinding is allowed, holes are not); pos[r] + n_steps <= n_ctx; n_steps >= 1;
 * every forced token in 0..n_vocab-1.  Everything is checked before anything is enqueued: 0, or -1
 * with a message on stderr and the context and every slot unchanged.  Afterwards slot seqs[r]
 * holds pos[r] + n_steps positions.  A context that never called lvk_seq_init has its slot 0;
 * the contexts that refuse lvk_seq_init refuse this call.  llama_get_logits is NOT refreshed.  The
 * n * n_steps rows count into the eval timings. */
LVK_API int lvk_decode_batch_chain(struct llama_context * ctx, const int * forced, int n_forced,
                                   const int * seqs, const int * pos, int n, int n_steps,
                                   int * out_tokens, uint64_t * out_digests, float * logits);
/* one launch of the chain's tail kernel on host logits [n][V]: step index i (same for all rows),
 * forced [n_forced][n] / n_forced as above.  Writes amax[n], digest[n], next_tok[n].  0 / -1. */
LVK_API int lvk_rows_step(const float * logits, int n, int V, const int * forced, int n_forced, int step,
                          int * amax, uint64_t * digest, int * next_tok);
/* A batched decode step that ends in the reference's sampler, per row.  Every slot has its own
 * mt19937: slot 0 draws from the context's (the one llama_sample_top_p_top_k and lvk_eval_sample
 * draw from, so the three share one stream), slots >= 1 get theirs at lvk_seq_init, seeded with
 * the context's seed (llama_context_params.seed as resolved at init).  lvk_seq_copy leaves the
 * generators alone; lvk_seq_seed reseeds one.
 *
 * lvk_decode_batch_sample is lvk_decode_batch(ctx, tokens, seqs, pos, n, NULL, NULL), then for every
 * row i with rows[i].sample != 0: out_tokens[i] = what llama_sample_top_p_top_k(., last_n, n_last,
 * top_k, top_p, temp, repeat_penalty) returns on row i's logits (llama.cpp:1356-1459), drawing from
 * slot seqs[i]'s generator; temp <= 0 is the first-maximum argmax and draws nothing.  Rows with
 * sample == 0 (prefill rows) give out_tokens[i] = -1.  Several sampled rows of one sequence draw in
 * row order.  last_n is the caller's window, as llama_sample_top_p_top_k takes it.
 * The repeat penalty, the temperature and the top-k selection of all sampled rows run in one launch
 * over the logits in HBM (sample.hip, one workgroup per row); only each row's candidates >= its
 * k-th value cross PCIe and the host finishes the reference's softmax / top-p /
 * discrete_distribution over k values per row.  A row with ties among its candidates, NaN logits,
 * top_k <= 0 or > 1024, or a window > 1024 takes the reference path over all of its logits (that
 * row alone is copied to the host; same result, slower; counted by lvk_sample_fallbacks).
 * Every argument is checked before anything is enqueued (lvk_decode_batch's checks; n_last >= 0 and
 * last_n != NULL when n_last > 0 for every sampled row; out_tokens != NULL): 0, or -1 with a message
 * on stderr and the context, every slot and every generator unchanged.  The contexts that refuse
 * lvk_seq_init refuse this call.  llama_get_logits is NOT refreshed.  The rows count into the eval
 * timings, the sampled rows into the sample timings. */
struct lvk_row_sample {
    int sample;            /* 0: no token wanted (prefill rows), out_tokens[i] = -1 */
    int top_k; float top_p; float temp; float repeat_penalty;
    int n_last; const int * last_n;      /* the caller's window, as llama_sample_top_p_top_k takes it */
};
LVK_API int lvk_decode_batch_sample(struct llama_context * ctx, const int * tokens, const int * seqs, const int * pos,
                                    int n, const struct lvk_row_sample * rows, int * out_tokens);
/* reseed a slot's generator (0: the context's rng); seed <= 0 is time(), as at init.  0, -1 on a bad id */
LVK_API int lvk_seq_seed(struct llama_context * ctx, int seq, int seed);
/* lvk_eval_sample calls and lvk_decode_batch_sample rows so far that took the all-logits path */
LVK_API int lvk_sample_fallbacks(struct llama_context * ctx);
/* op level, on host arrays: the rows kernel (sample.hip) on x[n_rows][n] for the selected rows
 * sel[n_sel] (row indices, any order, any subset).  Selected row j has k[j] (1..min(n, 1024)),
 * temp[j] (> 0), rp[j] and the last ids last[last_off[j] .. last_off[j + 1]) (at most 1024; last_off
 * has n_sel + 1 ascending entries).  Outputs per selected row, as lvk_sample_candidates gives them
 * for one: vals / ids [n_sel][1024] (the first min(counts[j], 1024) of a row are written),
 * counts[n_sel], flags[n_sel].  0, -1 on bad arguments. */
LVK_API int lvk_sample_candidates_rows(const float * x, int n_rows, int n, const int * sel, int n_sel, const int * k,
                                       const float * temp, const float * rp, const int * last, const int * last_off,
                                       float * vals, int * ids, int * counts, int * flags);

/* Scoring on the device: the probability of a given token per logits row, what perplexity, the
 * log-likelihood of a continuation and multiple-choice evals need, without the [n][n_vocab] copy
 * and the host softmax of the logits_all route (examples/perplexity/perplexity.cpp:6-20, 63-73).
 *
 * probs[i] = softmax(logits row i)[targets[i]] with the reference's arithmetic: the row maximum
 * from logits[0] on by std::max's rule, e = expf(x - max) as a float, the sum of the e in
 * double, (float) ((double) e_target / sum).  A row with targets[i] < 0 is not scored: probs[i] =
 * -1.0f.  NaN anywhere in a row, a +inf maximum or an all -inf row give NaN; a target about 104 or
 * more below the maximum gives 0, one between about 87.3 and 104 below it a denormal.
 * lvk_score_host is that definition on the host, bit for bit the reference's result on this
 * host (same operations, same order, this host's expf).  The device kernel (score.hip, one
 * workgroup per row, the row read once) rounds a double-precision exp to float where the host
 * calls expf and sums in a tree: a finite result is within 2 ulp of lvk_score_host's (distance of
 * the floats' ordered integer representations, denormals included); 0, NaN and -1.0f match.
 * argmax (optional, may be NULL): [n] ints, the first-maximum rule of lvk_decode_batch per row,
 * unscored rows included.
 *
 * lvk_score_rows / lvk_score_host: op level on host arrays logits [n][V], n >= 1, every target
 * < V.  lvk_score_rows takes 1 <= V <= 32768 (the row is held in registers); 0 / -1.
 *
 * lvk_eval_score is llama_eval(ctx, tokens, n_tokens, n_past, .) with the lm_head over every row,
 * whatever the context's logits_all and f16_kv, ended by the score kernel over targets[n_tokens]:
 * only probs (and argmax) cross PCIe.  The KV cache, its token count and the timings end as after
 * that llama_eval.  Runs eagerly (no graph).  A model with n_vocab > 32768 takes lvk_score_host
 * over the scored rows, copied to the host one by one.
 * lvk_decode_batch_score is lvk_decode_batch(ctx, tokens, seqs, pos, n, NULL, NULL) ended by the
 * score kernel, with that call's row rules, refusals and timings.
 * Both check every argument before anything is enqueued (null pointers, the row count, token ids,
 * every target < n_vocab): 0, or -1 with a message on stderr and the context and every slot
 * unchanged.  Layer-split and stage contexts return -1.  llama_get_logits is NOT refreshed
 * (after lvk_eval_score the host logits are stale, as after lvk_eval_greedy: llama_sample_top_p_top_k
 * refuses them until the next llama_eval). */
LVK_API int lvk_score_rows(const float * logits, int n, int V, const int * targets, float * probs, int * argmax);
LVK_API int lvk_score_host(const float * logits, int n, int V, const int * targets, float * probs);
LVK_API int lvk_eval_score(struct llama_context * ctx, const int * tokens, int n_tokens, int n_past,
                           const int * targets, float * probs, int * argmax);
LVK_API int lvk_decode_batch_score(struct llama_context * ctx, const int * tokens, const int * seqs, const int * pos,
                                   int n, const int * targets, float * probs, int * argmax);

/* Pipeline stages (the 65B layer split).  A stage context holds
 * layers [layer_begin, layer_end) of the model file (weights and KV cache); the
 * first stage (layer_begin == 0) also holds the token embeddings, the last one
 * (layer_end == n_layer) the final norm and lm_head.  This replaces running
 * llama_eval_internal (llama.cpp:927-1197) as one process: the residual stream
 * `inpL` is handed from stage s to s+1 (RCCL send/recv in
 * llama.vk_amd/pipeline.py).  NULL on error. */
LVK_API struct llama_context * lvk_init_stage(const char * path_model, struct llama_context_params params,
                                              int layer_begin, int layer_end);
/* run the stage on n_tokens at positions n_past..: the first stage embeds tokens,
 * the others start from the residual stream set by lvk_stage_set_x; the last
 * stage leaves logits for llama_get_logits.  0 on success, 1 on error. */
LVK_API int lvk_stage_eval(struct llama_context * ctx, const int * tokens, int n_tokens, int n_past);
/* copy the residual stream x [n_tokens][n_embd] f32 out of / into the stage;
 * buf is memory of the context's HIP device when on_device != 0, else host */
LVK_API int lvk_stage_get_x(struct llama_context * ctx, void * buf, int n_tokens, int on_device);
LVK_API int lvk_stage_set_x(struct llama_context * ctx, const void * buf, int n_tokens, int on_device);
/* the stage's layer range; returns the model's n_layer */
LVK_API int lvk_stage_layers(struct llama_context * ctx, int * layer_begin, int * layer_end);

/* One stage per process over RCCL (torchrun, one rank per GPU).  Rank 0 makes the
 * communicator id (lvk_rccl_unique_id: NCCL_UNIQUE_ID_BYTES = 128 bytes into id, n >= 128)
 * and shares it with the other ranks; every rank then joins with its stage context
 * (lvk_init_stage with the layers of stage `stage`, on its own GPU).  lvk_stage_step runs
 * one llama_eval slice of the pipeline on this rank: ncclRecv of inpL from stage-1, the
 * stage's layers, ncclSend to stage+1, all on the context's stream, prompts cut into
 * micro-batches of `micro` tokens (0: none).  greedy != 0 (one token): the last stage's
 * device argmax is sent to stage 0; both return it.  Otherwise 0 (the last stage leaves
 * logits for llama_get_logits).  -1 on error.  Every argument is checked before the first
 * transfer; a step that fails on any rank aborts the link (ncclCommAbort / the shm ring's
 * abort word), so the neighbours' steps fail too instead of waiting, and every wait is
 * bounded by LVK_STAGE_TIMEOUT_S seconds (default 300).  An aborted link must be
 * reconnected.  The replaced code is the single-process llama_eval_internal
 * (reference llama.cpp:927-1197). */
LVK_API int lvk_rccl_unique_id(void * id, size_t n);
LVK_API int lvk_stage_connect(struct llama_context * ctx, const void * id, int n_stages, int stage);
/* The same link through a host shared-memory ring (POSIX shm object `name`, a single path
 * component such as "/lvk_run42"): any stage placement, several stages on one GPU included,
 * no RCCL.  Stage 0 creates a fresh object under the name (removing one a crashed run left),
 * the others wait for it; the call returns once all n_stages stages have joined, and stage 0
 * then unlinks the name, so a reconnect (the only way on after an abort) under the same name
 * starts clean.  Messages travel in 1 MiB pieces: the object takes
 * n_stages * 4 MiB + 4 KiB of /dev/shm (32 MiB at 8 stages), reserved at connect -- a
 * /dev/shm too small fails the connect with an error. */
LVK_API int lvk_stage_connect_shm(struct llama_context * ctx, const char * name, int n_stages, int stage);
LVK_API int lvk_stage_step(struct llama_context * ctx, const int * tokens, int n_tokens, int n_past, int greedy,
                           int micro);
/* The stage link alone (per-hop time of the 65B split): `iters` laps of a `bytes`
 * message (one token's residual stream is n_embd * 4) around the stage ring -- stage 0 sends
 * to 1, ..., the last stage back to 0 -- on the same transport and stream as lvk_stage_step;
 * every stage calls it.  *us_per_hop: the wall time of a lap over the number of stages.  0 on
 * success, -1 on error (the link is aborted as in lvk_stage_step).  No reference counterpart:
 * the reference has no inter-device hop (llama.cpp:927-1197 runs every layer in one process). */
LVK_API int lvk_stage_link_probe(struct llama_context * ctx, int bytes, int iters, double * us_per_hop);

/* ggml_graph_compute keeps the host ranges of its tensors mirrored in HBM across calls and
 * uploads only bytes a node reads before the call writes them, and of those only pages the
 * host may have changed: pages of read-only mappings (a PROT_READ model file, an mprotect'ed
 * buffer) while the mapping is unchanged; writable pages go again on every call unless
 * LVK_GGML_CACHE=2 tracks them with the kernel's soft-dirty bits (process-wide clear_refs,
 * opt-in: measured slower in a HIP process).  Q4 weights are repacked once per upload.
 * lvk_ggml_stats: the last call's out[0] host->device bytes, out[1] device->host bytes (the
 * byte ranges the nodes wrote), out[2] bytes of Q4 weights repacked, out[3] host bytes
 * mirrored in HBM after the call; out[4] the tracking mode (0 off: LVK_GGML_CACHE=0, 1
 * read-only mappings only: the default, 2 soft-dirty pages: LVK_GGML_CACHE=2),
 * out[5] 1 once any graph has run, out[6] the call's host microseconds of tracking
 * bookkeeping, out[7] of them the microseconds in clear_refs.  Fills min(n, 8) values,
 * returns 8 (-1 on bad arguments).
 * lvk_ggml_invalidate: the caller changed [p, p + n) in a way that tracking cannot see
 * (write-enabled a read-only buffer, wrote, protected it again between two calls; or
 * hipHostRegister'ed the range after a call had used it, so that DMA may now write it);
 * its pages are uploaded again by the next call, and whether the range is HIP host memory
 * is decided again.  0 / -1. */
LVK_API int lvk_ggml_stats(uint64_t * out, int n);
LVK_API int lvk_ggml_invalidate(const void * p, size_t n);

/* The layer split behind llama.h, one process driving n_stages HIP
 * devices: stage s holds layers [s*L/S, (s+1)*L/S) on devices[s].  llama_eval /
 * lvk_eval_greedy / llama_get_logits / the KV-cache calls work on the returned context as
 * on a single-device one.  The residual stream moves between stages with grouped
 * ncclSend/ncclRecv (transport "rccl", the default when the devices are distinct) or a
 * stream-ordered device copy ("copy"; also used when a device repeats, e.g. a one-GPU
 * rehearsal); the host waits once per eval.  Prompts are cut into micro-batches of
 * `micro` tokens (0: none) that flow through the stages back to back.
 * llama_init_from_file does the same when the environment holds LVK_SPLIT_DEVICES=0,1,..
 * or LVK_SPLIT=S (devices 0..S-1), with LVK_SPLIT_TRANSPORT and LVK_SPLIT_MICRO (64). */
LVK_API struct llama_context * lvk_init_split(const char * path_model, struct llama_context_params params,
                                              int n_stages, const int * devices, const char * transport, int micro);
/* stages of ctx (1 without a split), whether they hand off over RCCL, the micro-batch */
LVK_API int lvk_split_info(struct llama_context * ctx, int * n_stages, int * rccl, int * micro);

#ifdef __cplusplus
}
#endif
#endif
