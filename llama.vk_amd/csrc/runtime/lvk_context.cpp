// lvk_context.cpp -- llama_eval on one HIP stream.
//
// The reference builds a ~1253-node ggml graph per token and runs it on a CPU
// thread pool (llama.cpp:927-1137, ggml.c:9230-9651).  Here the same forward
// pass is 5 fused kernels per layer (+ embedding and lm_head) on one stream:
//   QKV matvec  (rms_norm*g -> Q4 quantize -> Wq|Wk|Wv -> RoPE -> KV append)
//   attention   (scores; softmax -> P.V -> Q4 quantize of the merged heads)
//   Wo matvec   (+ residual)
//   W1|W3 matvec(rms_norm*g -> quantize -> silu(w1x)*w3x -> Q4 quantize)
//   W2 matvec   (+ residual)
// Single-token decode is captured once into a hipGraph; the position and the
// token come from a 16-byte step block copied to HBM before each replay, so
// the same graph serves every n_past.
#include "lvk_context.h"

#include <immintrin.h>

#include <cmath>
#include <cstring>

#include "../../../include/llama.h"
#include "../../../include/lvk_ops.h"

namespace lvk {

int64_t now_us() {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

namespace {
// host F16C conversion, identical to the reference's GGML_FP32_TO_FP16 (ggml.c:183)
__attribute__((target("f16c"))) uint16_t h_f32_to_f16(float f) { return _cvtss_sh(f, 0); }
__attribute__((target("f16c"))) float h_f16_to_f32(uint16_t h) { return _cvtsh_ss(h); }
}  // namespace

void host_fp16_tables(std::vector<uint16_t> & te, std::vector<uint16_t> & ts) {
    te.resize(65536);
    ts.resize(65536);
    for (int i = 0; i < 65536; ++i) {
        const float f = h_f16_to_f32((uint16_t) i);
        ts[i] = h_f32_to_f16(f / (1.0f + expf(-f)));
        te[i] = h_f32_to_f16(expf(f));
    }
}

// RoPE cos/sin table (ggml.c:7209-7213): theta = powf(10000, -i0/n_dims), angle = p*theta
void host_rope_table(std::vector<float2> & rt, size_t n_ctx, size_t hd) {
    rt.resize(n_ctx * (hd / 2));
    for (size_t pos = 0; pos < n_ctx; ++pos)
        for (size_t i0 = 0; i0 < hd; i0 += 2) {
            const float theta = powf(10000.0f, ((float) -(int) i0) / (float) hd);
            const float ang = (float) (int) pos * theta;
            rt[pos * (hd / 2) + i0 / 2] = make_float2(cosf(ang), sinf(ang));
        }
}

// the softmax may compute exp instead of reading the table, but only in a mode
// that reproduces this host's table on every argument it can see: 2 (device
// expf) if exact, else 1 (double exp) if exact, else 0 (table).  LVK_EXP_TABLE
// forces the table.
int pick_exp_mode(const uint16_t * exp_tab_d) {
    if (getenv("LVK_EXP_TABLE")) return 0;
    int * bad_d = nullptr;
    LVK_HIP(hipMalloc((void **) &bad_d, 2 * sizeof(int)));
    int bad[2] = {-1, -1};
    const hipError_t e1 = exp_check(exp_tab_d, bad_d, nullptr);
    const hipError_t e2 = e1 == hipSuccess ? hipMemcpy(bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost) : e1;
    (void) hipFree(bad_d);
    LVK_HIP(e2);
    return bad[1] == 0 ? 2 : bad[0] == 0 ? 1 : 0;
}

Context::~Context() {
    if (graph_exec) (void) hipGraphExecDestroy(graph_exec);
    if (graph) (void) hipGraphDestroy(graph);
    if (graph_greedy_exec) (void) hipGraphExecDestroy(graph_greedy_exec);
    if (graph_greedy) (void) hipGraphDestroy(graph_greedy);
    if (graph_sample_exec) (void) hipGraphExecDestroy(graph_sample_exec);
    if (graph_sample) (void) hipGraphDestroy(graph_sample);
    if (graph_chain_exec) (void) hipGraphExecDestroy(graph_chain_exec);
    if (graph_chain) (void) hipGraphDestroy(graph_chain);
    drop_rows_graph();
    for (void * p : {(void *) rc_tok_d, (void *) rc_dig_d, (void *) rc_forced_d, (void *) rc_ctl_d})
        if (p) (void) hipFree(p);
    for (void * p : {(void *) rc_tok_h, (void *) rc_dig_h, (void *) rc_forced_h, (void *) rc_ctl_h})
        if (p) (void) hipHostFree(p);
    for (void * p : {(void *) sr_rec_d, (void *) sr_pool_d})
        if (p) (void) hipFree(p);
    for (void * p : {(void *) sr_out_h, (void *) sr_rec_h, (void *) sr_pool_h})
        if (p) (void) hipHostFree(p);
    if (chain_h) (void) hipHostFree(chain_h);
    if (chain_ctl_h) (void) hipHostFree(chain_ctl_h);
    if (forced_h) (void) hipHostFree(forced_h);
    if (digest_h) (void) hipHostFree(digest_h);
    if (samp_h) (void) hipHostFree(samp_h);
    if (sout_h) (void) hipHostFree(sout_h);
    if (greedy_h) (void) hipHostFree(greedy_h);
    for (SeqKV & s : seq_kv) { (void) hipFree(s.kc); (void) hipFree(s.vc); }
    if (slots_d) (void) hipFree(slots_d);
    if (rows_d) (void) hipFree(rows_d);
    if (amax_d) (void) hipFree(amax_d);
    if (rows_h) (void) hipHostFree(rows_h);
    for (auto & e : ev_pool) { (void) hipEventDestroy(e.first); (void) hipEventDestroy(e.second); }
    if (sp_h) (void) hipHostFree(sp_h);
    if (tok_h) (void) hipHostFree(tok_h);
    if (err_h) (void) hipHostFree(err_h);
    if (stream) (void) hipStreamDestroy(stream);
}

void Context::init(const llama_context_params & p) {
    // the caller's window (llama.h accepts any positive n_ctx); buffers and kernels use it
    // rounded up to the 32-position attention tile, at least 128 (positions past the
    // caller's window are never written or read)
    if (p.n_ctx <= 0) throw Error("llama.vk_amd: n_ctx must be positive");
    n_ctx_user = p.n_ctx;
    n_ctx = std::max(128, (p.n_ctx + 31) / 32 * 32);
    logits_all = p.logits_all;
    want_embedding = p.embedding;
    const HParams & hp = model.hp;
    const size_t E = hp.n_embd, L = model.layers.size(), V = hp.n_vocab, H = hp.n_head, F = hp.n_ff();
    const size_t hd = E / H, C = (size_t) n_ctx;
    // KV cache element type (llama.cpp:1614): f16, or f32 when the caller asks for it
    kv32 = !p.f16_kv;
    const size_t es = kv_elem_bytes();
    kc = (uint16_t *) model.alloc(L * C * E * es);
    vc = (uint16_t *) model.alloc(L * C * E * es);
    LVK_HIP(hipMemset(kc, 0, L * C * E * es));
    LVK_HIP(hipMemset(vc, 0, L * C * E * es));
    x = (float *) model.alloc(C * E * 4);
    q16 = (uint16_t *) model.alloc(C * E * es);      // queries in the KV element type
    scores = (float *) model.alloc(C * H * C * 4);
    aq_attn.nb = (int) (E / 32);
    aq_attn.d = (float *) model.alloc(C * (E / 32) * 4);
    aq_attn.m = (float *) model.alloc(C * (E / 32) * 4);
    aq_attn.qs = (uint4 *) model.alloc(C * (E / 32) * 16);
    aq_ffn.nb = (int) (F / 32);
    aq_ffn.d = (float *) model.alloc(C * (F / 32) * 4);
    aq_ffn.m = (float *) model.alloc(C * (F / 32) * 4);
    aq_ffn.qs = (uint4 *) model.alloc(C * (F / 32) * 16);
    u_ffn = (float *) model.alloc(F * 4);
    {
        // xm zeroed once: the masked slots / padding rows are never written (lvk_kernels.h ActImage)
        auto alloc_image = [&](size_t K) {
            const ActImageBytes nbytes = act_image_bytes(model.qtype, (int) C, (int) K);
            ActImage im;
            im.xm = model.alloc(nbytes.xm);
            LVK_HIP(hipMemset(im.xm, 0, nbytes.xm));
            if (nbytes.da) im.da = (float *) model.alloc(nbytes.da);
            if (nbytes.xs) im.xs = model.alloc(nbytes.xs);
            return im;
        };
        img = alloc_image(std::max(E, F));
        const char * sq = getenv("LVK_MM_SWIGLU_Q");
        if (mm_epi_supported(model.qtype, EPI_SWIGLU_Q) && (!sq || atoi(sq) != 0)) img_w2 = alloc_image(F);
        // f16 and f32 weights take the Wo input in f32; the Q4 types take the quantized aq_attn
        if (model.qtype == F16 || model.qtype == F32) attn_f32 = (float *) model.alloc(C * E * 4);
        qkv32 = (float *) model.alloc(C * 3 * E * 4);
        uf = (float *) model.alloc(C * F * 4);
        prompt_exact = getenv("LVK_PROMPT_EXACT") && atoi(getenv("LVK_PROMPT_EXACT")) != 0;
        old_attention = getenv("LVK_ATTN_V1") && atoi(getenv("LVK_ATTN_V1")) != 0;
        attn_gran = model.alloc(attention_decode_scratch_bytes((int) H, (int) C));
        LVK_HIP(hipMemset(attn_gran, 0, attention_decode_scratch_bytes((int) H, (int) C)));
        // granule tags (seq << 7) + layer + 1 stay unique per token with up to 126 layers
        seq_epochs = L <= 126;
        // test hook (tests/test_gpu_seq_wrap.py): start the step counter near its 25-bit wrap
        if (const char * e = getenv("LVK_SEQ_START")) seq = (unsigned) strtoul(e, nullptr, 0) & ((1u << 25) - 1);
    }
    logits_d = (float *) model.alloc(C * V * 4);
    emb_d = (float *) model.alloc(E * 4);
    sp_d = (StepParams *) model.alloc(sizeof(StepParams));
    tok_d = (int *) model.alloc(C * 4);
    LVK_HIP(hipHostMalloc((void **) &sp_h, (1 + C) * sizeof(StepParams), hipHostMallocDefault));
    LVK_HIP(hipHostMalloc((void **) &tok_h, C * 4, hipHostMallocDefault));
    LVK_HIP(hipGetDevice(&device));
    LVK_HIP(hipHostMalloc((void **) &err_h, 64, hipHostMallocMapped | hipHostMallocCoherent));
    *err_h = 0;
    LVK_HIP(hipHostGetDevicePointer((void **) &err_d, err_h, 0));
    greedy_d = (int *) model.alloc(4);
    chain_d = (int *) model.alloc((CHAIN_HDR + C) * 4);
    forced_d = (int *) model.alloc(C * 4);
    digest_d = (unsigned long long *) model.alloc(C * 8);
    LVK_HIP(hipHostMalloc((void **) &chain_h, C * 4, hipHostMallocDefault));
    LVK_HIP(hipHostMalloc((void **) &chain_ctl_h, CHAIN_HDR * 4, hipHostMallocDefault));
    LVK_HIP(hipHostMalloc((void **) &forced_h, C * 4, hipHostMallocDefault));
    LVK_HIP(hipHostMalloc((void **) &digest_h, C * 8, hipHostMallocDefault));
    // the device argmax also stores the token straight into host-mapped memory
    LVK_HIP(hipHostMalloc((void **) &greedy_h, 64, hipHostMallocMapped | hipHostMallocCoherent));
    LVK_HIP(hipHostGetDevicePointer((void **) &greedy_hd, greedy_h, 0));
    samp_d = (SampleParams *) model.alloc(sizeof(SampleParams));
    LVK_HIP(hipHostMalloc((void **) &samp_h, sizeof(SampleParams), hipHostMallocDefault));
    std::memset(samp_h, 0, sizeof(SampleParams));
    LVK_HIP(hipHostMalloc((void **) &sout_h, sizeof(SampleOut), hipHostMallocMapped | hipHostMallocCoherent));
    LVK_HIP(hipHostGetDevicePointer((void **) &sout_d, sout_h, 0));

    // fp16 exp / silu tables (ggml.c:2915-2927), built with this host's glibc
    std::vector<uint16_t> te, ts;
    host_fp16_tables(te, ts);
    exp_tab = (uint16_t *) model.alloc(65536 * 2);
    silu_tab = (uint16_t *) model.alloc(65536 * 2);
    LVK_HIP(hipMemcpy(exp_tab, te.data(), 65536 * 2, hipMemcpyHostToDevice));
    LVK_HIP(hipMemcpy(silu_tab, ts.data(), 65536 * 2, hipMemcpyHostToDevice));
    exp_computed = pick_exp_mode(exp_tab);
    std::vector<float2> rt;
    host_rope_table(rt, C, hd);
    rope = (float2 *) model.alloc(rt.size() * sizeof(float2));
    LVK_HIP(hipMemcpy(rope, rt.data(), rt.size() * sizeof(float2), hipMemcpyHostToDevice));

    LVK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    logits.reserve(logits_all ? C * V : V);
    if (want_embedding) embedding.resize(E);
}

void Context::check_device_error() {
    const unsigned e = __atomic_load_n(err_h, __ATOMIC_ACQUIRE);
    if (e == LVK_ERR_NONE) return;
    __atomic_store_n(err_h, 0u, __ATOMIC_RELEASE);
    logits_valid = false;
    throw Error(e == LVK_ERR_ATTN_SPIN ? "llama.vk_amd: decode attention: a workgroup wait timed out (results discarded)"
                                       : "llama.vk_amd: a kernel wait timed out (results discarded)");
}

void Context::timed_launch(int cls, double bytes, const std::function<hipError_t()> & fn) {
    if (!profiling) {
        LVK_HIP(fn());
        return;
    }
    if (ev_used == ev_pool.size()) {
        hipEvent_t a, b;
        LVK_HIP(hipEventCreate(&a));
        LVK_HIP(hipEventCreate(&b));
        ev_pool.push_back({a, b});
        ev_class.push_back(0);
    }
    auto & e = ev_pool[ev_used];
    ev_class[ev_used] = cls;
    ++ev_used;
    g_launch_events = {e.first, e.second};
    const hipError_t err = fn();
    g_launch_events = {};
    LVK_HIP(err);
    prof.launches[cls] += 1;
    prof.bytes[cls] += bytes;
}

void Context::collect_profile() {
    for (size_t i = 0; i < ev_used; ++i) {
        float ms = 0.0f;
        LVK_HIP(hipEventElapsedTime(&ms, ev_pool[i].first, ev_pool[i].second));
        prof.ms[ev_class[i]] += ms;
    }
    ev_used = 0;
}

static double qbytes(const QMatrix & w) {
    if (w.qtype == F16) return (double) w.M * w.K * 2;
    if (w.qtype == F32) return (double) w.M * w.K * 4;
    return (double) w.M * (w.K / 32) * (w.qtype == Q4_0 ? 20 : 24);
}

// batches go through the batched matmuls (launch_act + launch_mm) when every matrix of the
// model fits them: f16 and f32 weights from 2 tokens on (their matvec is single-token only), the Q4
// types from 16 (the MFMA tile is 16 tokens wide; below that the per-row VALU kernels win)
bool Context::use_batched(int n) const {
    const bool q4 = model.qtype == Q4_0 || model.qtype == Q4_1;
    if (n == 1 || (q4 && (n < 16 || prompt_exact))) return false;
    for (const Layer & ly : model.layers)
        if (!mm_supported(ly.wqkv) || !mm_supported(ly.wo) || !mm_supported(ly.w13) || !mm_supported(ly.w2))
            return false;
    return true;
}

// The layer sequence, the same for every weight type (f16 weights:
// ggml_compute_forward_mul_mat_f16_f32 where the Q4 types run mul_mat_q_f32; the activations are
// converted to f16 where the Q4 types quantize them; f32 weights: ggml_compute_forward_mul_mat_f32
// on the f32 rows as they are):
//   embed, then per layer norm -> QKV, RoPE + KV append, attention, Wo (+x),
//   norm -> W1|W3 (SwiGLU), W2 (+x), then the head.
// Batches (use_batched) run it as operand image + matmul per matrix, everything else as one
// matvec launch per matrix with the conversion in its prologue.
//
// A batched decode step (rows; decode_rows) runs the same sequence.  Its rows sit at a position
// and on a KV slot each, so the fused QKV epilogues, which place row t at sp->n_past + t of slot
// 0, are not used: QKV is stored to qkv32, launch_rope_kv_rows appends every row's K / V, and one
// launch_attention_rows serves all rows.
void Context::enqueue_forward(int n, bool last_only, const int * tok_src, int logit_row, bool head, bool embed, bool rows) {
    const HParams & hp = model.hp;
    if (!tok_src) tok_src = tok_d;
    float * const logits_out = logits_d + (size_t) logit_row * hp.n_vocab;
    const int E = (int) hp.n_embd, H = (int) hp.n_head, hd = E / H, F = (int) hp.n_ff(), V = (int) hp.n_vocab;
    const int qt = model.qtype;
    const bool batched = use_batched(n);
    const bool prompt_attn = !rows && n > 1 && !kv32 && attention_prompt_supported(E, H, n_ctx);
    const bool decode_attn = !rows && n == 1 && !old_attention && !kv32 && attention_decode_supported(E, H, n_ctx);
    if (decode_attn && !seq_epochs)
        // the decode attention's score granules carry epoch = layer + 1: zero them once per token
        LVK_HIP(hipMemsetAsync(attn_gran, 0, attention_decode_scratch_bytes(H, n_ctx), stream));
    if (model.has_embed && embed)
        // a single-token eval takes its token from the step block (one H2D copy per token)
        timed_launch(K_EMBED, 0, [&] {
            return launch_embed(model.tok_emb, model.emb_type, E, n == 1 ? &sp_d->pad0 : tok_src, n, x, stream);
        });
    // x[n][K] (rms_norm * g when g) -> img, and y = / += W img.  f32 weights read f32 rows:
    // without a norm the input itself is the image
    auto act = [&](int cls, const float * xin, const float * g, int K) -> ActImage {
        if (qt == F32 && !g) {
            ActImage in;
            in.xm = (void *) xin;
            return in;
        }
        timed_launch(cls, 0, [&] { return launch_act(qt, xin, g, n, K, img, stream); });
        return img;
    };
    auto mm = [&](int cls, const QMatrix & w, const ActImage & in, float * y, int ldy, int epi, const RopeKV * rk = nullptr,
                  const ActImage & out = {}) {
        MmLaunch L;
        L.w = w; L.x = in; L.N = n; L.y = y; L.ldy = ldy; L.silu_tab = silu_tab; L.rk = rk; L.out = out;
        timed_launch(cls, qbytes(w), [&] { return launch_mm(L, epi, stream); });
    };
    // single-token FFN: W1|W3 hands silu(w1 x)*(w3 x) to W2 in f32, W2 converts it
    const bool ffn_f32 = n == 1 && matvec_cu_supported(E, qt) && matvec_cu_supported(F, qt);
    for (size_t il = 0; il < model.layers.size(); ++il) {
        const Layer & ly = model.layers[il];
        uint16_t * kcl = kc_layer(il);
        uint16_t * vcl = vc_layer(il);
        // every attention kernel writes the Wo input quantized (aq_attn; Q4_0 blocks for an f16 or
        // f32 model, which reads attn_f32 instead)
        AttnLaunch at{q16, kcl, vcl, scores, aq_attn, qt == F16 || qt == F32 ? Q4_0 : qt, exp_tab, sp_d, n, E, H, n_ctx};
        at.out_f32 = attn_f32;
        at.exp_computed = exp_computed;
        at.err = err_d;
        at.kv32 = kv32;
        at.seq_epochs = seq_epochs ? 1 : 0;
        // a batched decode step: RoPE + KV append per row from qkv32, then all rows' attention
        const size_t layer_off = il * (size_t) n_ctx * E;
        auto rows_rope_attn = [&] {
            timed_launch(K_QKV, 0, [&] {
                return launch_rope_kv_rows(qkv32, n, E, hd, rope, rows_d, slots_d, layer_off, n_ctx, q16, stream);
            });
            timed_launch(K_ATTN, 0, [&] { return launch_attention_rows(at, rows_d, slots_d, layer_off, stream); });
        };
        if (batched) {
            ActImage in = act(K_QKV, x, ly.attn_norm, E);
            if (rows) {
                mm(K_QKV, ly.wqkv, in, qkv32, 3 * E, EPI_STORE);
            } else if (!kv32 && mm_rope_fused && mm_epi_supported(qt, EPI_ROPE_KV)) {
                // RoPE + KV append in the matmul's epilogue (the f32 rows never reach memory)
                const RopeKV rk{rope, sp_d, n_ctx, E, hd, q16, kcl, vcl};
                mm(K_QKV, ly.wqkv, in, nullptr, 0, EPI_ROPE_KV, &rk);
            } else {
                mm(K_QKV, ly.wqkv, in, qkv32, 3 * E, EPI_STORE);
                timed_launch(K_QKV, 0, [&] {
                    return launch_rope_kv(qkv32, n, E, hd, rope, sp_d, n_ctx, q16, kcl, vcl, stream, kv32);
                });
            }
            // the Wo input image: written by the prompt attention itself (Q4), else from the
            // attention's f32 rows (f16 weights) or its quantized blocks
            const bool wo_fused = prompt_attn && !attn_f32;
            if (rows)
                rows_rope_attn();
            else if (prompt_attn)
                timed_launch(K_ATTN, 0, [&] {
                    return launch_attention_prompt(at, (uint16_t *) scores, wo_fused ? img : ActImage{}, stream);
                });
            else
                timed_launch(K_ATTN, 0, [&] { return launch_attention(at, stream); });
            in = img;
            if (attn_f32) in = act(K_WO, attn_f32, nullptr, E);
            else if (!wo_fused) timed_launch(K_WO, 0, [&] { return launch_actq_to_image(qt, aq_attn, n, E, img, stream); });
            mm(K_WO, ly.wo, in, x, E, EPI_RESID);
            in = act(K_W13, x, ly.ffn_norm, E);
            if (img_w2.xm) {
                // SwiGLU + the W2 input's quantization in the W1|W3 epilogue
                mm(K_W13, ly.w13, in, nullptr, 0, EPI_SWIGLU_Q, nullptr, img_w2);
                mm(K_W2, ly.w2, img_w2, x, E, EPI_RESID);
            } else {
                mm(K_W13, ly.w13, in, uf, F, EPI_SWIGLU_F32);
                in = act(K_W2, uf, nullptr, F);
                mm(K_W2, ly.w2, in, x, E, EPI_RESID);
            }
            continue;
        }
        MvLaunch a;
        a.w = ly.wqkv; a.x = x; a.g = ly.attn_norm; a.sp = sp_d; a.n_tokens = n;
        a.q16 = q16; a.kc = kcl; a.vc = vcl; a.rope.cs = rope;
        a.n_embd = E; a.head_dim = hd; a.n_ctx = n_ctx; a.kv32 = kv32;
        if (rows) a.y = qkv32;
        timed_launch(K_QKV, qbytes(ly.wqkv), [&] { return launch_matvec_auto(a, PRO_NORM, rows ? EPI_STORE : EPI_QKV, stream); });
        if (rows)
            rows_rope_attn();
        else if (prompt_attn)
            timed_launch(K_ATTN, 0, [&] { return launch_attention_prompt(at, (uint16_t *) scores, ActImage{}, stream); });
        else if (decode_attn)
            timed_launch(K_ATTN, 0, [&] { return launch_attention_decode(at, attn_gran, (unsigned) il + 1, stream); });
        else
            timed_launch(K_ATTN, 0, [&] { return launch_attention(at, stream); });
        MvLaunch b;      // input: the attention's f32 rows (f16 weights) or its quantized blocks
        b.w = ly.wo; b.x = attn_f32; b.xq = aq_attn; b.y = x; b.sp = sp_d; b.n_tokens = n;
        timed_launch(K_WO, qbytes(ly.wo), [&] { return launch_matvec_auto(b, attn_f32 ? PRO_ACTF : PRO_ACTQ, EPI_RESID, stream); });
        MvLaunch c;
        c.w = ly.w13; c.x = x; c.g = ly.ffn_norm; c.sp = sp_d; c.n_tokens = n; c.silu_tab = silu_tab;
        c.out_q = aq_ffn; c.u = u_ffn;
        MvLaunch d;
        d.w = ly.w2; d.xq = aq_ffn; d.x = u_ffn; d.y = x; d.sp = sp_d; d.n_tokens = n;
        if (ffn_f32) {
            timed_launch(K_W13, qbytes(ly.w13), [&] { return launch_matvec_cu(c, PRO_NORM, EPI_SWIGLU_F32, stream); });
            timed_launch(K_W2, qbytes(ly.w2), [&] { return launch_matvec_cu(d, PRO_ACTF, EPI_RESID, stream); });
        } else {
            timed_launch(K_W13, qbytes(ly.w13), [&] { return launch_matvec(c, PRO_NORM, EPI_SWIGLU, stream); });
            timed_launch(K_W2, qbytes(ly.w2), [&] { return launch_matvec(d, PRO_ACTQ, EPI_RESID, stream); });
        }
    }
    if (!model.has_head || !head) return;   // not the last pipeline stage: x is the output
    if (batched && !last_only && mm_supported(model.output)) {
        // logits_all: lm_head over every row
        const ActImage in = act(K_LMHEAD, x, model.norm, E);
        mm(K_LMHEAD, model.output, in, logits_out, V, EPI_STORE);
    } else {
        MvLaunch o;
        o.w = model.output; o.x = x; o.g = model.norm; o.sp = sp_d; o.y = logits_out;
        o.tok0 = last_only ? n - 1 : 0;
        o.n_tokens = last_only ? 1 : n;
        timed_launch(K_LMHEAD, qbytes(model.output), [&] { return launch_matvec_auto(o, PRO_NORM, EPI_STORE, stream); });
    }
    if (want_embedding && !rows)
        LVK_HIP(launch_rmsnorm_rows(x + (size_t) (n - 1) * E, model.norm, E, 1, emb_d, stream));
}

void Context::build_graph(int kind) {
    // one replay per token: the step block H2D, the forward pass and the logits D2H
    // (both host buffers page-locked, the logits one sized before the capture); the
    // greedy variant ends in the device argmax (token into host-mapped memory), the sample
    // variant copies the sampler block in and ends in the device top-k candidates
    LVK_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
        if (kind == 3) {
            // a chained step: the step block and x were left by the previous step (or the
            // call's setup); the argmax advances both for the next replay
            enqueue_forward(1, true, nullptr, 0, true, false);
            LVK_HIP(launch_argmax_step(logits_d, (int) model.hp.n_vocab, sp_d, chain_d, forced_d, digest_d, model.tok_emb, model.emb_type,
                                       (int) model.hp.n_embd, x, stream));
        } else {
            LVK_HIP(hipMemcpyAsync(sp_d, sp_h, sizeof(StepParams), hipMemcpyHostToDevice, stream));
            if (kind == 2) LVK_HIP(hipMemcpyAsync(samp_d, samp_h, sizeof(SampleParams), hipMemcpyHostToDevice, stream));
            enqueue_forward(1, true);
            if (kind == 1) {
                enqueue_argmax();
            } else if (kind == 2) {
                LVK_HIP(launch_sample_cand(logits_d, (int) model.hp.n_vocab, samp_d, sout_d, stream));
            } else if (model.has_head) {
                LVK_HIP(hipMemcpyAsync(logits.data(), logits_d, sizeof(float) * logits.size(), hipMemcpyDeviceToHost,
                                       stream));
            }
        }
    } catch (...) {
        hipGraph_t g;
        (void) hipStreamEndCapture(stream, &g);
        throw;
    }
    hipGraph_t & g = kind == 1 ? graph_greedy : kind == 2 ? graph_sample : kind == 3 ? graph_chain : graph;
    hipGraphExec_t & ge = kind == 1 ? graph_greedy_exec : kind == 2 ? graph_sample_exec : kind == 3 ? graph_chain_exec : graph_exec;
    LVK_HIP(hipStreamEndCapture(stream, &g));
    LVK_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
}

// greedy token of the last logits row: the device word feeds the stage link (lvk_split.cpp),
// the host-mapped one the caller (read after the stream sync; no D2H copy node)
void Context::enqueue_argmax() {
    LVK_HIP(launch_argmax(logits_d, (int) model.hp.n_vocab, greedy_d, stream, greedy_hd));
}

// One decode step whose sampler is greedy, chosen on the device:
// the same forward pass and KV append as eval(&token, 1, n_past), then the argmax
// of llama_sample_top_p_top_k(temp <= 0) (llama.cpp:1382-1394) over the logits in
// HBM.  Host logits are not refreshed (llama_get_logits keeps the previous eval's).
int Context::eval_greedy(int token, int n_past) {
    if (!model.has_head || !model.has_embed) throw Error("llama.vk_amd: greedy eval needs the whole model");
    EvalPart part;
    part.greedy = true;
    begin_eval_safe(&token, 1, n_past, part);
    end_eval(true);
    kv_n = n_past + 1;
    return *greedy_h;
}

// the step counter of the next device step (StepParams::seq); before it would run past the
// 25 bits that keep (seq << 7) + layer + 1 unique, the granules are zeroed (stream-ordered
// ahead of the steps that use the restarted counter) and the count restarts
unsigned Context::next_seq(unsigned k) {
    if (seq + k >= (1u << 25)) {
        if (attn_gran)
            LVK_HIP(hipMemsetAsync(attn_gran, 0, attention_decode_scratch_bytes((int) model.hp.n_head, n_ctx), stream));
        seq = 0;
    }
    const unsigned first = seq + 1;
    seq += k;
    return first;
}

// n_steps decode steps in one call (lvk_decode_chain): step i evaluates token t_i at n_past + i,
// t_0 = tokens[0], t_{i+1} = tokens[i + 1] while i + 1 < n_tokens (teacher forcing), else the
// argmax of step i's logits (greedy: n_tokens = 1).  The same logits as n_steps single-token
// evals, but the host only sets the step block up once and replays the chained graph back to back
// (no host round trip, step-block copy or embedding launch between the steps).  out[i]: the
// argmax of step i; digests (optional): lvk_logits_digest of step i's logits row.
int Context::decode_chain(const int * tokens, int n_tokens, int n_past, int n_steps, int * out,
                          unsigned long long * digests) {
    if (!model.has_head || !model.has_embed) throw Error("llama.vk_amd: chained decode needs the whole model");
    if (logits_all) throw Error("llama.vk_amd: chained decode needs last-token logits");
    if (n_steps <= 0 || n_past < 0 || n_past + n_steps > n_ctx_user)
        throw Error("llama.vk_amd: n_past + n_steps exceeds n_ctx");
    if (!tokens || n_tokens < 1 || n_tokens > n_steps) throw Error("llama.vk_amd: chained decode needs 1..n_steps tokens");
    for (int i = 0; i < n_tokens; ++i)
        if (tokens[i] < 0 || tokens[i] >= (int) model.hp.n_vocab) throw Error("llama.vk_amd: token id out of range");
    if (!use_graph || profiling)
        throw Error("llama.vk_amd: chained decode needs the launch-per-phase decode graph");
    try {
        StepParams * sh = sp_h;
        sh->n_past = n_past;
        sh->n_tokens = 1;
        sh->pad0 = tokens[0];
        sh->seq = next_seq((unsigned) n_steps);     // the steps take seq, seq + 1, ...
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        chain_ctl_h[0] = 0;
        chain_ctl_h[1] = n_tokens > 1 ? n_tokens : 0;
        chain_ctl_h[2] = digests ? 1 : 0;
        chain_ctl_h[3] = 0;
        LVK_HIP(hipMemcpyAsync(chain_d, chain_ctl_h, CHAIN_HDR * 4, hipMemcpyHostToDevice, stream));
        if (n_tokens > 1) {
            std::memcpy(forced_h, tokens, sizeof(int) * (size_t) n_tokens);
            LVK_HIP(hipMemcpyAsync(forced_d, forced_h, sizeof(int) * (size_t) n_tokens, hipMemcpyHostToDevice, stream));
        }
        LVK_HIP(launch_embed(model.tok_emb, model.emb_type, (int) model.hp.n_embd, &sp_d->pad0, 1, x, stream));
        if (!graph_chain_exec) build_graph(3);
        for (int i = 0; i < n_steps; ++i) LVK_HIP(hipGraphLaunch(graph_chain_exec, stream));
        LVK_HIP(hipMemcpyAsync(chain_h, chain_d + CHAIN_HDR, sizeof(int) * (size_t) n_steps, hipMemcpyDeviceToHost, stream));
        if (digests)
            LVK_HIP(hipMemcpyAsync(digest_h, digest_d, 8 * (size_t) n_steps, hipMemcpyDeviceToHost, stream));
    } catch (...) {
        (void) hipStreamSynchronize(stream);
        logits_valid = false;
        throw;
    }
    end_eval(true);
    kv_n = n_past + n_steps;
    std::memcpy(out, chain_h, sizeof(int) * (size_t) n_steps);
    if (digests) std::memcpy(digests, digest_h, 8 * (size_t) n_steps);
    return out[n_steps - 1];
}

// One decode step whose sampler runs its O(n_vocab) part on the device:
// the forward pass of eval(&token, 1, n_past), then sample.hip's repeat penalty, temperature
// and top-k candidates over the logits in HBM (parameters in *samp_h).  Host logits are not
// refreshed (llama_get_logits keeps the previous eval's).
void Context::eval_sample(int token, int n_past) {
    if (!model.has_head || !model.has_embed) throw Error("llama.vk_amd: sampling eval needs the whole model");
    if ((int) model.hp.n_vocab > SAMPLE_MAX_VOCAB) throw Error("llama.vk_amd: vocabulary too large for the device sampler");
    EvalPart part;
    part.sample = true;
    begin_eval_safe(&token, 1, n_past, part);
    end_eval(true);
    kv_n = n_past + 1;
}

void Context::fetch_logits() {
    const size_t V = model.hp.n_vocab;
    logits.resize(V);
    LVK_HIP(hipMemcpy(logits.data(), logits_d, V * sizeof(float), hipMemcpyDeviceToHost));
    logits_valid = true;
}

void Context::eval(const int * tokens, int n, int n_past) {
    begin_eval_safe(tokens, n, n_past, EvalPart{});
    end_eval(false);
    kv_n = n_past + n;      // the positions the cache holds: slot 0's count for lvk_decode_batch
}

// begin_eval for a caller that ends the eval itself: if the enqueue fails part-way, the
// work already queued drains, the step blocks are released and the host logits are marked
// stale before the error propagates (llama_get_logits then refuses them)
void Context::begin_eval_safe(const int * tokens, int n, int n_past, const EvalPart & part) {
    try {
        begin_eval(tokens, n, n_past, part);
    } catch (...) {
        (void) hipStreamSynchronize(stream);
        sp_next = 1;
        logits_valid = false;
        throw;
    }
}

void Context::begin_eval(const int * tokens, int n, int n_past, const EvalPart & part) {
    const HParams & hp = model.hp;
    const int V = (int) hp.n_vocab;
    const int n_total = part.n_total < 0 ? n : part.n_total;
    if (n <= 0 || n_past < 0 || n_past + n > n_ctx_user || part.tok_off < 0 || part.tok_off + n > n_total)
        throw Error("llama.vk_amd: n_past + n_tokens exceeds n_ctx");
    if ((part.greedy || part.sample) && (!model.has_head || n != 1 || logits_all))
        throw Error("llama.vk_amd: greedy / sampling eval needs the lm_head stage, one token and last-token logits");
    if (model.has_embed) {
        if (!tokens) throw Error("llama.vk_amd: the first stage needs tokens");
        for (int i = 0; i < n; ++i)
            if (tokens[i] < 0 || tokens[i] >= V) throw Error("llama.vk_amd: token id out of range");
        std::memcpy(tok_h + part.tok_off, tokens, sizeof(int) * (size_t) n);
    }
    const bool last_only = !logits_all;
    const bool single = part.n_total < 0 || part.n_total == n;
    const bool graph_ok = n == 1 && last_only && single && use_graph && !profiling;
    // the graphs read step block 0; eager slices each take their own (the H2D copy reads
    // the pinned block when it executes, after the host may have queued further slices)
    if (!graph_ok && sp_next > n_ctx) throw Error("llama.vk_amd: too many slices before a sync");
    StepParams * sh = graph_ok ? sp_h : sp_h + sp_next++;
    sh->n_past = n_past;
    sh->n_tokens = n;
    sh->pad0 = (n == 1 && model.has_embed) ? tokens[0] : 0;
    sh->seq = next_seq();
    if (model.has_head && part.tok_off == 0)   // within the reserve: the pointer never moves
        logits.resize((size_t) (last_only ? 1 : n_total) * V);
    if (graph_ok) {
        const int kind = part.greedy ? 1 : part.sample ? 2 : 0;
        hipGraphExec_t & ge = kind == 1 ? graph_greedy_exec : kind == 2 ? graph_sample_exec : graph_exec;
        if (!ge) build_graph(kind);
        LVK_HIP(hipGraphLaunch(ge, stream));
    } else {
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        if (part.sample) LVK_HIP(hipMemcpyAsync(samp_d, samp_h, sizeof(SampleParams), hipMemcpyHostToDevice, stream));
        if (n > 1)
            LVK_HIP(hipMemcpyAsync(tok_d + part.tok_off, tok_h + part.tok_off, sizeof(int) * (size_t) n,
                                   hipMemcpyHostToDevice, stream));
        enqueue_forward(n, last_only, tok_d + part.tok_off, last_only ? 0 : part.tok_off, part.head);
        if (part.greedy) {
            enqueue_argmax();
        } else if (part.sample) {
            LVK_HIP(launch_sample_cand(logits_d, V, samp_d, sout_d, stream));
        } else if (model.has_head && part.copy_out) {
            LVK_HIP(hipMemcpyAsync(logits.data(), logits_d, sizeof(float) * logits.size(), hipMemcpyDeviceToHost,
                                   stream));
        }
    }
    if (want_embedding && model.has_head && part.copy_out && !part.greedy && !part.sample) {
        embedding.resize(hp.n_embd);
        LVK_HIP(hipMemcpyAsync(embedding.data(), emb_d, sizeof(float) * hp.n_embd, hipMemcpyDeviceToHost, stream));
    }
}

void Context::end_eval(bool no_host_logits) {
    sp_next = 1;
    LVK_HIP(hipStreamSynchronize(stream));
    if (profiling) collect_profile();
    check_device_error();
    // after lvk_eval_greedy llama_get_logits still holds an earlier eval's row
    logits_valid = model.has_head && !no_host_logits;
}

size_t Context::kv_bytes() const {
    return 2u * (size_t) model.layers.size() * n_ctx * model.hp.n_embd * kv_elem_bytes();
}

void Context::kv_get() {
    const size_t half = kv_bytes() / 2;
    kv_host.resize(kv_bytes());
    LVK_HIP(hipMemcpy(kv_host.data(), kc, half, hipMemcpyDeviceToHost));
    LVK_HIP(hipMemcpy(kv_host.data() + half, vc, half, hipMemcpyDeviceToHost));
}

void Context::kv_set(const uint8_t * src, size_t n) {
    if (n != kv_bytes()) throw Error("llama_set_kv_cache: size mismatch");
    const size_t half = n / 2;
    LVK_HIP(hipMemcpy(kc, src, half, hipMemcpyHostToDevice));
    LVK_HIP(hipMemcpy(vc, src + half, half, hipMemcpyHostToDevice));
}

// device-to-device copy of positions [0, n_tokens) of every layer's K and V from
// another context of the same shape (a shared prompt prefix): K rows
// [L][n_ctx][E] are one pitched block per layer, V [L][E][n_ctx] one short row per
// (layer, dim).  Only the n_tokens positions move, not the whole cache.
void Context::kv_copy_from(const Context & src, int n_tokens) {
    const size_t E = model.hp.n_embd, L = model.layers.size(), C = (size_t) n_ctx;
    if (src.model.hp.n_embd != model.hp.n_embd || src.model.layers.size() != L || src.n_ctx != n_ctx || src.n_ctx_user != n_ctx_user ||
        src.model.hp.n_head != model.hp.n_head || src.model.layer_begin != model.layer_begin)
        throw Error("lvk_kv_copy: contexts differ in n_embd, n_head, n_layer, layer range or n_ctx");
    if (src.device != device) throw Error("lvk_kv_copy: contexts live on different HIP devices");
    // the K/V bytes are only meaningful under the weights that wrote them: same model
    // file contents (size and quantization type are checked; the caller owns identity)
    if (src.model.qtype != model.qtype || src.model.file_bytes != model.file_bytes)
        throw Error("lvk_kv_copy: contexts hold different models");
    if (src.kv32 != kv32) throw Error("lvk_kv_copy: contexts differ in the KV cache type (f16_kv)");
    if (n_tokens < 0 || n_tokens > n_ctx_user) throw Error("lvk_kv_copy: n_tokens out of range");
    if (n_tokens > 0) {
        const size_t n = (size_t) n_tokens;
        LVK_HIP(hipStreamSynchronize(src.stream));
        const size_t es = kv_elem_bytes();
        LVK_HIP(hipMemcpy2DAsync(kc, C * E * es, src.kc, C * E * es, n * E * es, L, hipMemcpyDeviceToDevice, stream));
        LVK_HIP(hipMemcpy2DAsync(vc, C * es, src.vc, C * es, n * es, L * E, hipMemcpyDeviceToDevice, stream));
        LVK_HIP(hipStreamSynchronize(stream));
    }
    kv_n = n_tokens;
}

// KV slots 1..n_seq-1 and, on the first call, the row and slot tables of decode_rows.  Everything
// new is allocated before anything is committed, so a failure leaves the context as it was.
void Context::seq_init(int n_seq) {
    const HParams & hp = model.hp;
    if (n_seq < 1) throw Error("lvk_seq_init: n_seq must be at least 1");
    if (kv32) throw Error("lvk_seq_init: batched decode needs the f16 KV cache (f16_kv = true)");
    if (!model.has_embed || !model.has_head || link) throw Error("lvk_seq_init: not available on a stage context");
    if (!attention_rows_supported((int) hp.n_embd, (int) hp.n_head, n_ctx))
        throw Error("lvk_seq_init: batched decode needs head_dim 128");
    const int have = seq_count();
    if (n_seq <= have && slots_d) return;
    const int want = std::max(n_seq, have);
    const size_t bytes = kv_bytes() / 2, C = (size_t) n_ctx;
    struct Fresh {      // freed unless committed
        std::vector<void *> dev;
        void * host = nullptr;
        ~Fresh() {
            for (void * p : dev) (void) hipFree(p);
            if (host) (void) hipHostFree(host);
        }
        void * get(size_t n) {
            void * p = nullptr;
            if (hipMalloc(&p, n) != hipSuccess) {
                (void) hipGetLastError();
                throw Error("lvk_seq_init: out of device memory");
            }
            dev.push_back(p);
            return p;
        }
    } fresh;
    std::vector<SeqKV> add((size_t) (want - have));
    for (SeqKV & s : add) {
        s.kc = (uint16_t *) fresh.get(bytes);
        s.vc = (uint16_t *) fresh.get(bytes);
        LVK_HIP(hipMemset(s.kc, 0, bytes));
        LVK_HIP(hipMemset(s.vc, 0, bytes));
    }
    // the new slots' generators start from the context's seed; the existing ones stay as they are
    std::vector<std::mt19937> gens;
    gens.reserve((size_t) want - 1);
    gens.assign(seq_rng.begin(), seq_rng.end());
    gens.resize((size_t) want - 1, std::mt19937((unsigned) seed));
    std::vector<SeqSlot> table;
    table.push_back({kc, vc});
    for (const SeqKV & s : seq_kv) table.push_back({s.kc, s.vc});
    for (const SeqKV & s : add) table.push_back({s.kc, s.vc});
    SeqSlot * table_d = (SeqSlot *) fresh.get(table.size() * sizeof(SeqSlot));
    SeqRow * rd = rows_d;
    int * ad = amax_d;
    if (!rows_d) {
        rd = (SeqRow *) fresh.get(C * sizeof(SeqRow));
        ad = (int *) fresh.get(C * sizeof(int));
        LVK_HIP(hipHostMalloc(&fresh.host, C * sizeof(SeqRow), hipHostMallocDefault));
    }
    LVK_HIP(hipStreamSynchronize(stream));      // nothing in flight reads the old table
    LVK_HIP(hipMemcpy(table_d, table.data(), table.size() * sizeof(SeqSlot), hipMemcpyHostToDevice));
    // commit
    drop_rows_graph();      // its launches hold the old slot table
    if (slots_d) (void) hipFree(slots_d);
    slots_d = table_d;
    if (!rows_d) {
        rows_d = rd;
        amax_d = ad;
        rows_h = (SeqRow *) fresh.host;
        fresh.host = nullptr;
    }
    seq_kv.insert(seq_kv.end(), add.begin(), add.end());
    seq_rng.swap(gens);
    fresh.dev.clear();
}

// positions [0, n_tokens) of every layer's K and V from slot src to slot dst, device to device
// (the copies of kv_copy_from)
void Context::seq_copy(int dst, int src, int n_tokens) {
    if (dst < 0 || dst >= seq_count() || src < 0 || src >= seq_count()) throw Error("lvk_seq_copy: sequence id out of range");
    if (n_tokens < 0 || n_tokens > seq_n(src)) throw Error("lvk_seq_copy: n_tokens exceeds the source sequence");
    if (dst != src && n_tokens > 0) {
        const size_t E = model.hp.n_embd, L = model.layers.size(), C = (size_t) n_ctx, n = (size_t) n_tokens, es = kv_elem_bytes();
        uint16_t * dk = dst == 0 ? kc : seq_kv[(size_t) dst - 1].kc, * dv = dst == 0 ? vc : seq_kv[(size_t) dst - 1].vc;
        const uint16_t * sk = src == 0 ? kc : seq_kv[(size_t) src - 1].kc, * sv = src == 0 ? vc : seq_kv[(size_t) src - 1].vc;
        LVK_HIP(hipMemcpy2DAsync(dk, C * E * es, sk, C * E * es, n * E * es, L, hipMemcpyDeviceToDevice, stream));
        LVK_HIP(hipMemcpy2DAsync(dv, C * es, sv, C * es, n * es, L * E, hipMemcpyDeviceToDevice, stream));
        LVK_HIP(hipStreamSynchronize(stream));
    }
    seq_n(dst) = n_tokens;
}

// the argument checks of a batched decode step (decode_rows, decode_rows_sample), messages under
// the caller's name
std::vector<int> Context::rows_check(const char * fn, const int * tokens, const int * seqs, const int * pos, int n) {
    const int V = (int) model.hp.n_vocab;
    const std::string f = std::string(fn) + ": ";
    if (!tokens || !seqs || !pos) throw Error(f + "null argument");
    if (n < 1 || n > n_ctx_user) throw Error(f + "the row count must be in 1..n_ctx");
    // next[s]: the position the next row of slot s must have (-1: no row yet)
    std::vector<int> next((size_t) seq_count(), -1);
    for (int i = 0; i < n; ++i) {
        if (tokens[i] < 0 || tokens[i] >= V) throw Error(f + "token id out of range");
        if (seqs[i] < 0 || seqs[i] >= seq_count()) throw Error(f + "sequence id out of range");
        if (pos[i] < 0 || pos[i] >= n_ctx_user) throw Error(f + "position outside n_ctx");
        int & nx = next[(size_t) seqs[i]];
        if (nx < 0 && pos[i] > seq_n(seqs[i])) throw Error(f + "position past the end of its sequence (a hole)");
        if (nx >= 0 && pos[i] != nx) throw Error(f + "rows of one sequence must have consecutive ascending positions");
        nx = pos[i] + 1;
    }
    return next;
}

// One batched decode step (lvk_decode_batch).  Every argument is checked before anything is
// enqueued; the slots' counts move only after the step has completed.
void Context::decode_rows(const int * tokens, const int * seqs, const int * pos, int n, float * logits_out, int * argmax_out) {
    const HParams & hp = model.hp;
    const int V = (int) hp.n_vocab;
    if (!slots_d) seq_init(1);
    const std::vector<int> next = rows_check("lvk_decode_batch", tokens, seqs, pos, n);
    try {
        if (sp_next > n_ctx) throw Error("llama.vk_amd: too many slices before a sync");
        StepParams * sh = sp_h + sp_next++;
        sh->n_past = 0;             // no kernel of this path takes a position from the step block
        sh->n_tokens = n;
        sh->pad0 = n == 1 ? tokens[0] : 0;
        sh->seq = next_seq();
        std::memcpy(tok_h, tokens, sizeof(int) * (size_t) n);
        for (int i = 0; i < n; ++i) rows_h[i] = {seqs[i], pos[i]};
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(tok_d, tok_h, sizeof(int) * (size_t) n, hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(rows_d, rows_h, sizeof(SeqRow) * (size_t) n, hipMemcpyHostToDevice, stream));
        enqueue_forward(n, false, tok_d, 0, true, true, true);
        if (argmax_out) {
            LVK_HIP(launch_argmax_rows(logits_d, V, n, amax_d, stream));
            LVK_HIP(hipMemcpyAsync(argmax_out, amax_d, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost, stream));
        }
        if (logits_out)
            LVK_HIP(hipMemcpyAsync(logits_out, logits_d, sizeof(float) * (size_t) n * V, hipMemcpyDeviceToHost, stream));
    } catch (...) {
        (void) hipStreamSynchronize(stream);
        sp_next = 1;
        throw;
    }
    // the host logits of llama_get_logits are an earlier eval's: they stay as they are
    const bool valid = logits_valid;
    end_eval(true);
    logits_valid = valid;
    for (int s = 0; s < seq_count(); ++s)
        if (next[(size_t) s] >= 0) seq_n(s) = next[(size_t) s];
}

// room for `rows` sampled rows of a step and `pool` last-n ids: the host-mapped candidates, the
// records and the pool, on the device and page-locked on the host.  Everything new is allocated
// before anything is committed (as rows_chain_reserve); a buffer that is large enough stays.
void Context::rows_sample_reserve(size_t rows, size_t pool) {
    const bool grow_rows = rows > sr_cap, grow_pool = pool > sr_pool_cap || !sr_pool_d;
    if (!grow_rows && !grow_pool) return;
    struct Fresh {      // freed unless committed
        std::vector<void *> dev, host;
        ~Fresh() {
            for (void * p : dev) (void) hipFree(p);
            for (void * p : host) (void) hipHostFree(p);
        }
        void * get(size_t n, int kind) {      // 0 device, 1 pinned, 2 host-mapped
            void * p = nullptr;
            const hipError_t e = kind == 0 ? hipMalloc(&p, n)
                                           : hipHostMalloc(&p, n, kind == 1 ? hipHostMallocDefault
                                                                            : hipHostMallocMapped | hipHostMallocCoherent);
            if (e != hipSuccess) {
                (void) hipGetLastError();
                throw Error("lvk_decode_batch_sample: out of memory for the sampler's rows");
            }
            (kind == 0 ? dev : host).push_back(p);
            return p;
        }
    } fresh;
    const size_t rcap = grow_rows ? std::max(rows, (size_t) 16) : sr_cap;
    const size_t pcap = grow_pool ? std::max(std::max(pool, sr_pool_cap), (size_t) 1024) : sr_pool_cap;
    SampleOut * out_hn = sr_out_h, * out_dn = sr_out_d;
    SampleRow * rec_hn = sr_rec_h, * rec_dn = sr_rec_d;
    int * pool_hn = sr_pool_h, * pool_dn = sr_pool_d;
    if (grow_rows) {
        out_hn = (SampleOut *) fresh.get(rcap * sizeof(SampleOut), 2);
        LVK_HIP(hipHostGetDevicePointer((void **) &out_dn, out_hn, 0));
        rec_hn = (SampleRow *) fresh.get(rcap * sizeof(SampleRow), 1);
        rec_dn = (SampleRow *) fresh.get(rcap * sizeof(SampleRow), 0);
    }
    if (grow_pool) {
        pool_hn = (int *) fresh.get(pcap * sizeof(int), 1);
        pool_dn = (int *) fresh.get(pcap * sizeof(int), 0);
    }
    LVK_HIP(hipStreamSynchronize(stream));      // nothing in flight uses the old buffers
    // commit
    if (grow_rows) {
        if (sr_rec_d) (void) hipFree(sr_rec_d);
        for (void * p : {(void *) sr_out_h, (void *) sr_rec_h})
            if (p) (void) hipHostFree(p);
        sr_out_h = out_hn; sr_out_d = out_dn;
        sr_rec_h = rec_hn; sr_rec_d = rec_dn;
        sr_cap = rcap;
    }
    if (grow_pool) {
        if (sr_pool_d) (void) hipFree(sr_pool_d);
        if (sr_pool_h) (void) hipHostFree(sr_pool_h);
        sr_pool_h = pool_hn; sr_pool_d = pool_dn;
        sr_pool_cap = pcap;
    }
    fresh.dev.clear();
    fresh.host.clear();
}

// One batched decode step that ends in the sampler (lvk_decode_batch_sample): decode_rows' forward
// pass, enqueued eagerly; launch_argmax_rows over the span of rows that ask for a greedy token
// (temp <= 0); one launch_sample_cand_rows for the rows that sample within the device limits; one
// stream sync; then, in row order, the host tail of lvk_eval_sample over each row's candidates
// with the generator of the row's slot.  A row with ties, NaN, overflow, top_k <= 0 or >
// SAMPLE_CAP, or a window > SAMPLE_MAX_LAST has its own logits row copied to the host and takes
// sample_logits there with the same generator (n_sample_fallback counts it); no other row notices.
// Every argument is checked before anything is enqueued; the slots' counts move after the step
// has completed.  The rows count into the eval timings, the sampled rows into the sample timings.
void Context::decode_rows_sample(const int * tokens, const int * seqs, const int * pos, int n, const lvk_row_sample * rows,
                                 int * out_tokens) {
    const int64_t t0 = now_us();
    const int V = (int) model.hp.n_vocab;
    if (!slots_d) seq_init(1);
    const std::vector<int> next = rows_check("lvk_decode_batch_sample", tokens, seqs, pos, n);
    if (!rows || !out_tokens) throw Error("lvk_decode_batch_sample: null argument");
    enum : char { NONE, GREEDY, DEVICE, HOST };
    std::vector<char> kind((size_t) n, NONE);
    std::vector<int> top((size_t) n, 0);      // the reference's k: top_k, or all of them
    size_t n_dev = 0, n_pool = 0;
    int n_samp = 0, g_lo = n, g_hi = -1;
    for (int i = 0; i < n; ++i) {
        const lvk_row_sample & r = rows[i];
        if (!r.sample) continue;
        if (r.n_last < 0 || (r.n_last > 0 && !r.last_n)) throw Error("lvk_decode_batch_sample: bad last-n window");
        ++n_samp;
        const int k = top[(size_t) i] = r.top_k > 0 ? std::min(r.top_k, V) : V;
        if (r.temp <= 0) {                              // llama.cpp:1382-1394
            kind[(size_t) i] = GREEDY;
            g_lo = std::min(g_lo, i);
            g_hi = i;
        } else if (k > SAMPLE_CAP || r.n_last > SAMPLE_MAX_LAST || V > SAMPLE_MAX_VOCAB) {
            kind[(size_t) i] = HOST;
        } else {
            kind[(size_t) i] = DEVICE;
            ++n_dev;
            n_pool += (size_t) r.n_last;
        }
    }
    if (n_dev) rows_sample_reserve(n_dev, n_pool);
    std::vector<int> amax((size_t) n, -1), slot_of((size_t) n, -1);
    try {
        if (sp_next > n_ctx) throw Error("llama.vk_amd: too many slices before a sync");
        StepParams * sh = sp_h + sp_next++;
        sh->n_past = 0;             // no kernel of this path takes a position from the step block
        sh->n_tokens = n;
        sh->pad0 = n == 1 ? tokens[0] : 0;
        sh->seq = next_seq();
        std::memcpy(tok_h, tokens, sizeof(int) * (size_t) n);
        for (int i = 0; i < n; ++i) rows_h[i] = {seqs[i], pos[i]};
        size_t j = 0, off = 0;
        for (int i = 0; i < n; ++i) {
            if (kind[(size_t) i] != DEVICE) continue;
            const lvk_row_sample & r = rows[i];
            sr_rec_h[j] = {i, top[(size_t) i], r.n_last, (int) off, 1.0f / r.temp /* llama.cpp:1398 */, r.repeat_penalty};
            if (r.n_last > 0) std::memcpy(sr_pool_h + off, r.last_n, sizeof(int) * (size_t) r.n_last);
            off += (size_t) r.n_last;
            slot_of[(size_t) i] = (int) j++;
        }
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(tok_d, tok_h, sizeof(int) * (size_t) n, hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(rows_d, rows_h, sizeof(SeqRow) * (size_t) n, hipMemcpyHostToDevice, stream));
        if (n_dev) {
            LVK_HIP(hipMemcpyAsync(sr_rec_d, sr_rec_h, sizeof(SampleRow) * n_dev, hipMemcpyHostToDevice, stream));
            if (n_pool) LVK_HIP(hipMemcpyAsync(sr_pool_d, sr_pool_h, sizeof(int) * n_pool, hipMemcpyHostToDevice, stream));
        }
        enqueue_forward(n, false, tok_d, 0, true, true, true);
        if (g_hi >= 0) {
            const size_t m = (size_t) (g_hi - g_lo + 1);
            LVK_HIP(launch_argmax_rows(logits_d + (size_t) g_lo * V, V, (int) m, amax_d + g_lo, stream));
            LVK_HIP(hipMemcpyAsync(amax.data() + g_lo, amax_d + g_lo, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
        }
        if (n_dev) LVK_HIP(launch_sample_cand_rows(logits_d, V, sr_rec_d, sr_pool_d, (int) n_dev, sr_out_d, stream));
    } catch (...) {
        (void) hipStreamSynchronize(stream);
        sp_next = 1;
        throw;
    }
    // the host logits of llama_get_logits are an earlier eval's: they stay as they are
    const bool valid = logits_valid;
    end_eval(true);
    logits_valid = valid;
    for (int s = 0; s < seq_count(); ++s)
        if (next[(size_t) s] >= 0) seq_n(s) = next[(size_t) s];
    const int64_t t1 = now_us();
    t_eval_us += t1 - t0;       // n decode evals (llama.cpp:1186-1195)
    n_eval += n;
    std::vector<float> row;
    for (int i = 0; i < n; ++i) {
        const lvk_row_sample & r = rows[i];
        int tok = -1;
        if (kind[(size_t) i] == GREEDY) tok = amax[(size_t) i];
        else if (kind[(size_t) i] == DEVICE)
            tok = sample_from_candidates(sr_out_h[slot_of[(size_t) i]], top[(size_t) i], r.top_p, seq_gen(seqs[i]));
        if (tok < 0 && (kind[(size_t) i] == DEVICE || kind[(size_t) i] == HOST)) {
            row.resize((size_t) V);
            LVK_HIP(hipMemcpy(row.data(), logits_d + (size_t) i * V, sizeof(float) * (size_t) V, hipMemcpyDeviceToHost));
            tok = sample_logits(row.data(), V, r.last_n, r.n_last, r.top_k, r.top_p, r.temp, r.repeat_penalty, seq_gen(seqs[i]));
            n_sample_fallback++;
        }
        out_tokens[i] = tok;
    }
    t_sample_us += now_us() - t1;
    n_sample += n_samp;
}

void Context::drop_rows_graph() {
    if (graph_rows_exec) (void) hipGraphExecDestroy(graph_rows_exec);
    if (graph_rows) (void) hipGraphDestroy(graph_rows);
    graph_rows_exec = nullptr;
    graph_rows = nullptr;
    graph_rows_n = 0;
}

// room for `entries` = n_steps * n tokens, digests and forced tokens of a chained batched decode,
// on the device and page-locked on the host, and on the first call the control block.  Everything
// new is allocated before anything is committed (as seq_init); the step graph holds the old
// addresses, so it goes with them.
void Context::rows_chain_reserve(size_t entries) {
    if (entries <= rc_cap && rc_ctl_d) return;
    const size_t cap = std::max(std::max(entries, rc_cap), (size_t) n_ctx);
    struct Fresh {      // freed unless committed
        std::vector<void *> dev, host;
        ~Fresh() {
            for (void * p : dev) (void) hipFree(p);
            for (void * p : host) (void) hipHostFree(p);
        }
        void * get(size_t n, bool pinned) {
            void * p = nullptr;
            const hipError_t e = pinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
            if (e != hipSuccess) {
                (void) hipGetLastError();
                throw Error("lvk_decode_batch_chain: out of memory for the step outputs");
            }
            (pinned ? host : dev).push_back(p);
            return p;
        }
    } fresh;
    int * tok_dn = (int *) fresh.get(cap * sizeof(int), false), * tok_hn = (int *) fresh.get(cap * sizeof(int), true);
    auto * dig_dn = (unsigned long long *) fresh.get(cap * 8, false), * dig_hn = (unsigned long long *) fresh.get(cap * 8, true);
    int * for_dn = (int *) fresh.get(cap * sizeof(int), false), * for_hn = (int *) fresh.get(cap * sizeof(int), true);
    int * ctl_dn = rc_ctl_d, * ctl_hn = rc_ctl_h;
    if (!rc_ctl_d) {
        ctl_dn = (int *) fresh.get((2 + (size_t) n_ctx) * sizeof(int), false);
        ctl_hn = (int *) fresh.get((2 + (size_t) n_ctx) * sizeof(int), true);
    }
    LVK_HIP(hipStreamSynchronize(stream));      // nothing in flight uses the old buffers
    // commit
    drop_rows_graph();
    for (void * p : {(void *) rc_tok_d, (void *) rc_dig_d, (void *) rc_forced_d})
        if (p) (void) hipFree(p);
    for (void * p : {(void *) rc_tok_h, (void *) rc_dig_h, (void *) rc_forced_h})
        if (p) (void) hipHostFree(p);
    rc_tok_d = tok_dn; rc_tok_h = tok_hn;
    rc_dig_d = dig_dn; rc_dig_h = dig_hn;
    rc_forced_d = for_dn; rc_forced_h = for_hn;
    rc_ctl_d = ctl_dn; rc_ctl_h = ctl_hn;
    rc_cap = cap;
    fresh.dev.clear();
    fresh.host.clear();
}

// n_steps batched decode steps in one call (lvk_decode_batch_chain): step i evaluates, for every
// row r, token t_i[r] at pos[r] + i on slot seqs[r], as decode_rows would with those n rows;
// t_0[r] = forced[r], t_{i+1}[r] = forced[(i + 1) * n + r] while i + 1 < n_forced, else the argmax
// of row r's logits of step i.  The host sets the rows, the forced table and the first embedding
// rows up once; each step is the rows' forward pass followed by k_rows_step, which leaves x and
// rows_d as the next step reads them.  The rows path of enqueue_forward takes positions and slots
// from rows_d / slots_d alone (sp_d is read only by the fused QKV epilogues, which a rows step
// does not run), so the step block needs no advancing on the device.  The steps are replays of
// one captured graph, or the same launches enqueued eagerly when the graph is off or the
// profiler is on.  Every argument is checked before anything is enqueued; the slots' counts move
// only after the last step has completed.
void Context::decode_rows_chain(const int * forced, int n_forced, const int * seqs, const int * pos, int n, int n_steps,
                                int * out_tokens, unsigned long long * out_digests, float * logits_out) {
    const HParams & hp = model.hp;
    const int V = (int) hp.n_vocab, E = (int) hp.n_embd;
    if (!slots_d) seq_init(1);
    if (!forced || !seqs || !pos || !out_tokens) throw Error("lvk_decode_batch_chain: null argument");
    if (n < 1 || n > n_ctx_user) throw Error("lvk_decode_batch_chain: the row count must be in 1..n_ctx");
    if (n_steps < 1 || n_steps > n_ctx_user) throw Error("lvk_decode_batch_chain: n_steps must be in 1..n_ctx");
    if (n_forced < 1 || n_forced > n_steps) throw Error("lvk_decode_batch_chain: n_forced must be in 1..n_steps");
    std::vector<char> named((size_t) seq_count(), 0);
    for (int r = 0; r < n; ++r) {
        if (seqs[r] < 0 || seqs[r] >= seq_count()) throw Error("lvk_decode_batch_chain: sequence id out of range");
        if (named[(size_t) seqs[r]]) throw Error("lvk_decode_batch_chain: a sequence may have one row only");
        named[(size_t) seqs[r]] = 1;
        if (pos[r] < 0 || pos[r] > seq_n(seqs[r]))
            throw Error("lvk_decode_batch_chain: position past the end of its sequence (a hole)");
        if (pos[r] > n_ctx_user - n_steps) throw Error("lvk_decode_batch_chain: pos + n_steps exceeds n_ctx");
    }
    const size_t nf = (size_t) n_forced * n, total = (size_t) n_steps * n;
    for (size_t k = 0; k < nf; ++k)
        if (forced[k] < 0 || forced[k] >= V) throw Error("lvk_decode_batch_chain: token id out of range");
    rows_chain_reserve(total);
    auto step = [&] {
        enqueue_forward(n, false, tok_d, 0, true, /*embed=*/false, /*rows=*/true);
        LVK_HIP(launch_rows_step(logits_d, V, n, rows_d, rc_ctl_d + 2, rc_ctl_d, rc_forced_d, rc_tok_d, rc_dig_d, nullptr,
                                 model.tok_emb, model.emb_type, E, x, stream));
    };
    try {
        if (sp_next > n_ctx) throw Error("llama.vk_amd: too many slices before a sync");
        StepParams * sh = sp_h + sp_next++;
        sh->n_past = 0;             // no kernel of this path takes a position from the step block
        sh->n_tokens = n;
        sh->pad0 = 0;
        sh->seq = next_seq((unsigned) n_steps);
        rc_ctl_h[0] = n_forced;
        rc_ctl_h[1] = out_digests ? 1 : 0;
        for (int r = 0; r < n; ++r) {
            rows_h[r] = {seqs[r], pos[r]};
            rc_ctl_h[2 + r] = pos[r];
        }
        std::memcpy(rc_forced_h, forced, sizeof(int) * nf);
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(rows_d, rows_h, sizeof(SeqRow) * (size_t) n, hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(rc_ctl_d, rc_ctl_h, sizeof(int) * (2 + (size_t) n), hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(rc_forced_d, rc_forced_h, sizeof(int) * nf, hipMemcpyHostToDevice, stream));
        LVK_HIP(launch_embed(model.tok_emb, model.emb_type, E, rc_forced_d, n, x, stream));
        if (use_graph && !profiling) {
            // the row count (and the matmul path it selects) is baked into the graph's launches
            if (graph_rows_exec && (graph_rows_n != n || graph_rows_exact != prompt_exact)) drop_rows_graph();
            if (!graph_rows_exec) {
                LVK_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
                try {
                    step();
                } catch (...) {
                    hipGraph_t g = nullptr;
                    (void) hipStreamEndCapture(stream, &g);
                    if (g) (void) hipGraphDestroy(g);
                    throw;
                }
                LVK_HIP(hipStreamEndCapture(stream, &graph_rows));
                const hipError_t e = hipGraphInstantiate(&graph_rows_exec, graph_rows, nullptr, nullptr, 0);
                if (e != hipSuccess) {
                    graph_rows_exec = nullptr;
                    drop_rows_graph();
                    LVK_HIP(e);
                }
                graph_rows_n = n;
                graph_rows_exact = prompt_exact;
            }
            for (int i = 0; i < n_steps; ++i) LVK_HIP(hipGraphLaunch(graph_rows_exec, stream));
        } else {
            for (int i = 0; i < n_steps; ++i) step();
        }
        LVK_HIP(hipMemcpyAsync(rc_tok_h, rc_tok_d, sizeof(int) * total, hipMemcpyDeviceToHost, stream));
        if (out_digests) LVK_HIP(hipMemcpyAsync(rc_dig_h, rc_dig_d, 8 * total, hipMemcpyDeviceToHost, stream));
        if (logits_out)
            LVK_HIP(hipMemcpyAsync(logits_out, logits_d, sizeof(float) * (size_t) n * V, hipMemcpyDeviceToHost, stream));
    } catch (...) {
        (void) hipStreamSynchronize(stream);
        sp_next = 1;
        throw;
    }
    // the host logits of llama_get_logits are an earlier eval's: they stay as they are
    const bool valid = logits_valid;
    end_eval(true);
    logits_valid = valid;
    std::memcpy(out_tokens, rc_tok_h, sizeof(int) * total);
    if (out_digests) std::memcpy(out_digests, rc_dig_h, 8 * total);
    for (int r = 0; r < n; ++r) seq_n(seqs[r]) = pos[r] + n_steps;
}

}  // namespace lvk

namespace lvk {
// pipeline stages: the residual stream crosses stage boundaries
void Context::x_copy(void * buf, int n, bool to_ctx, bool on_device) {
    if (n <= 0 || n > n_ctx) throw Error("llama.vk_amd: bad token count for the stage residual stream");
    const size_t bytes = sizeof(float) * (size_t) n * model.hp.n_embd;
    const hipMemcpyKind k = to_ctx ? (on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                                   : (on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    if (to_ctx) LVK_HIP(hipMemcpyAsync(x, buf, bytes, k, stream));
    else LVK_HIP(hipMemcpyAsync(buf, x, bytes, k, stream));
    LVK_HIP(hipStreamSynchronize(stream));
}
}  // namespace lvk
