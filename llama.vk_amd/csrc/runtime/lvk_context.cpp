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
    const DevPtr<int> bad_d = dev_alloc<int>(2);
    int bad[2] = {-1, -1};
    LVK_HIP(exp_check(exp_tab_d, bad_d.get(), nullptr));
    LVK_HIP(hipMemcpy(bad, bad_d.get(), sizeof(bad), hipMemcpyDeviceToHost));
    return bad[1] == 0 ? 2 : bad[0] == 0 ? 1 : 0;
}

// Every allocation lands in a member that owns it (or in the model's arena), so a throw part-way
// frees what came before it when the half-built Context is destroyed.
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
    // the score kernel holds a row in registers; a larger vocabulary is scored on the host
    // (test hook, tests/test_gpu_score.py: LVK_SCORE_HOST=1 sends any vocabulary that way)
    score_on_host = V > (size_t) SCORE_MAX_VOCAB || (getenv("LVK_SCORE_HOST") && atoi(getenv("LVK_SCORE_HOST")) != 0);
    emb_d = (float *) model.alloc(E * 4);
    sp_d = (StepParams *) model.alloc(sizeof(StepParams));
    tok_d = (int *) model.alloc(C * 4);
    sp_h = pinned_alloc<StepParams>(1 + C);
    tok_h = pinned_alloc<int>(C);
    LVK_HIP(hipGetDevice(&device));
    err_h = mapped_alloc<unsigned>(16);
    err_h[0] = 0;
    err_d = device_address(err_h);
    greedy_d = (int *) model.alloc(4);
    chain_d = (int *) model.alloc((CHAIN_HDR + C) * 4);
    forced_d = (int *) model.alloc(C * 4);
    digest_d = (unsigned long long *) model.alloc(C * 8);
    chain_h = pinned_alloc<int>(C);
    chain_ctl_h = pinned_alloc<int>(CHAIN_HDR);
    forced_h = pinned_alloc<int>(C);
    digest_h = pinned_alloc<unsigned long long>(C);
    // the device argmax also stores the token straight into host-mapped memory
    greedy_h = mapped_alloc<int>(16);
    greedy_hd = device_address(greedy_h);
    samp_d = (SampleParams *) model.alloc(sizeof(SampleParams));
    samp_h = pinned_alloc<SampleParams>(1);
    std::memset(samp_h.get(), 0, sizeof(SampleParams));
    sout_h = mapped_alloc<SampleOut>(1);
    sout_d = device_address(sout_h);

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

    LVK_HIP(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    logits.reserve(logits_all ? C * V : V);
    if (want_embedding) embedding.resize(E);
}

void Context::check_device_error() {
    const unsigned e = __atomic_load_n(err_h.get(), __ATOMIC_ACQUIRE);
    if (e == LVK_ERR_NONE) return;
    __atomic_store_n(err_h.get(), 0u, __ATOMIC_RELEASE);
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
        Event a = make_event(), b = make_event();
        ev_pool.emplace_back(std::move(a), std::move(b));
        ev_class.push_back(0);
    }
    auto & e = ev_pool[ev_used];
    ev_class[ev_used] = cls;
    ++ev_used;
    g_launch_events = {e.first.get(), e.second.get()};
    const hipError_t err = fn();
    g_launch_events = {};
    LVK_HIP(err);
    prof.launches[cls] += 1;
    prof.bytes[cls] += bytes;
}

void Context::collect_profile() {
    for (size_t i = 0; i < ev_used; ++i) {
        float ms = 0.0f;
        LVK_HIP(hipEventElapsedTime(&ms, ev_pool[i].first.get(), ev_pool[i].second.get()));
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
void Context::enqueue_forward(const Forward & f) {
    const HParams & hp = model.hp;
    const int n = f.n;
    const bool last_only = f.last_only, head = f.head, embed = f.embed, rows = f.rows;
    const int * tok_src = f.tok_src ? f.tok_src : tok_d;
    float * const logits_out = logits_d + (size_t) f.logit_row * hp.n_vocab;
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
                return launch_rope_kv_rows(qkv32, n, E, hd, rope, rows_d.get(), slots_d.get(), layer_off, n_ctx, q16, stream);
            });
            timed_launch(K_ATTN, 0, [&] { return launch_attention_rows(at, rows_d.get(), slots_d.get(), layer_off, stream); });
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

void Context::build_graph(DecodeGraph kind) {
    // one replay per token: the step block H2D, the forward pass and the logits D2H
    // (both host buffers page-locked, the logits one sized before the capture); the
    // greedy variant ends in the device argmax (token into host-mapped memory), the sample
    // variant copies the sampler block in and ends in the device top-k candidates
    const int V = (int) model.hp.n_vocab;
    capture(stream, graph_of(kind), [&] {
        if (kind == DecodeGraph::CHAIN) {
            // a chained step: the step block and x were left by the previous step (or the
            // call's setup); the argmax advances both for the next replay
            Forward f;
            f.embed = false;
            enqueue_forward(f);
            LVK_HIP(launch_argmax_step(logits_d, V, sp_d, chain_d, forced_d, digest_d, model.tok_emb, model.emb_type,
                                       (int) model.hp.n_embd, x, stream));
            return;
        }
        LVK_HIP(hipMemcpyAsync(sp_d, sp_h.get(), sizeof(StepParams), hipMemcpyHostToDevice, stream));
        if (kind == DecodeGraph::SAMPLE)
            LVK_HIP(hipMemcpyAsync(samp_d, samp_h.get(), sizeof(SampleParams), hipMemcpyHostToDevice, stream));
        enqueue_forward(Forward{});
        if (kind == DecodeGraph::GREEDY) {
            enqueue_argmax();
        } else if (kind == DecodeGraph::SAMPLE) {
            LVK_HIP(launch_sample_cand(logits_d, V, samp_d, sout_d, stream));
        } else if (model.has_head) {
            LVK_HIP(hipMemcpyAsync(logits.data(), logits_d, sizeof(float) * logits.size(), hipMemcpyDeviceToHost, stream));
        }
    });
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
    return greedy_h[0];
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
    drain_on_error(false, true, [&] {
        StepParams * sh = sp_h.get();
        sh->n_past = n_past;
        sh->n_tokens = 1;
        sh->pad0 = tokens[0];
        sh->seq = next_seq((unsigned) n_steps);     // the steps take seq, seq + 1, ...
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        chain_ctl_h[0] = 0;
        chain_ctl_h[1] = n_tokens > 1 ? n_tokens : 0;
        chain_ctl_h[2] = digests ? 1 : 0;
        chain_ctl_h[3] = 0;
        LVK_HIP(hipMemcpyAsync(chain_d, chain_ctl_h.get(), CHAIN_HDR * 4, hipMemcpyHostToDevice, stream));
        if (n_tokens > 1) {
            std::memcpy(forced_h.get(), tokens, sizeof(int) * (size_t) n_tokens);
            LVK_HIP(hipMemcpyAsync(forced_d, forced_h.get(), sizeof(int) * (size_t) n_tokens, hipMemcpyHostToDevice, stream));
        }
        LVK_HIP(launch_embed(model.tok_emb, model.emb_type, (int) model.hp.n_embd, &sp_d->pad0, 1, x, stream));
        if (!graph_of(DecodeGraph::CHAIN)) build_graph(DecodeGraph::CHAIN);
        for (int i = 0; i < n_steps; ++i) LVK_HIP(graph_of(DecodeGraph::CHAIN).launch(stream));
        LVK_HIP(hipMemcpyAsync(chain_h.get(), chain_d + CHAIN_HDR, sizeof(int) * (size_t) n_steps, hipMemcpyDeviceToHost, stream));
        if (digests)
            LVK_HIP(hipMemcpyAsync(digest_h.get(), digest_d, 8 * (size_t) n_steps, hipMemcpyDeviceToHost, stream));
    });
    end_eval(true);
    kv_n = n_past + n_steps;
    std::memcpy(out, chain_h.get(), sizeof(int) * (size_t) n_steps);
    if (digests) std::memcpy(digests, digest_h.get(), 8 * (size_t) n_steps);
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

// The scoring tail's buffers, n_ctx rows each: reserved into local owners, committed once nothing
// can throw any more (the pattern of lvk_rows.cpp).
void Context::score_reserve() {
    if (sc_tgt_d) return;
    const size_t C = (size_t) n_ctx;
    const char * oom = "llama.vk_amd: out of memory for the scoring buffers";
    DevPtr<int> td = dev_alloc<int>(C, oom), ad = dev_alloc<int>(C, oom);
    DevPtr<float> pd = dev_alloc<float>(C, oom);
    HostPtr<int> th = pinned_alloc<int>(C, oom), ah = pinned_alloc<int>(C, oom);
    HostPtr<float> ph = pinned_alloc<float>(C, oom);
    // commit
    sc_tgt_d = std::move(td);
    sc_amax_d = std::move(ad);
    sc_prob_d = std::move(pd);
    sc_tgt_h = std::move(th);
    sc_amax_h = std::move(ah);
    sc_prob_h = std::move(ph);
}

void Context::score_stage(const char * fn, int n, const int * targets, const float * probs) {
    const int V = (int) model.hp.n_vocab;
    const std::string f = std::string(fn) + ": ";
    if (!targets || !probs) throw Error(f + "null argument");
    if (n < 1 || n > n_ctx_user) throw Error(f + "the row count must be in 1..n_ctx");
    for (int i = 0; i < n; ++i)
        if (targets[i] >= V) throw Error(f + "target id out of range");
    score_reserve();
    std::memcpy(sc_tgt_h.get(), targets, sizeof(int) * (size_t) n);
}

void Context::enqueue_score(int n, bool want_argmax) {
    const int V = (int) model.hp.n_vocab;
    if (!score_on_host) {
        LVK_HIP(hipMemcpyAsync(sc_tgt_d.get(), sc_tgt_h.get(), sizeof(int) * (size_t) n, hipMemcpyHostToDevice, stream));
        LVK_HIP(launch_score_rows(logits_d, V, n, sc_tgt_d.get(), sc_prob_d.get(), stream));
        LVK_HIP(hipMemcpyAsync(sc_prob_h.get(), sc_prob_d.get(), sizeof(float) * (size_t) n, hipMemcpyDeviceToHost, stream));
    }
    if (want_argmax) {
        LVK_HIP(launch_argmax_rows(logits_d, V, n, sc_amax_d.get(), stream));
        LVK_HIP(hipMemcpyAsync(sc_amax_h.get(), sc_amax_d.get(), sizeof(int) * (size_t) n, hipMemcpyDeviceToHost, stream));
    }
}

void Context::score_collect(int n, float * probs, int * argmax) {
    const size_t V = model.hp.n_vocab;
    if (!score_on_host) {
        std::memcpy(probs, sc_prob_h.get(), sizeof(float) * (size_t) n);
    } else {
        std::vector<float> row(V);
        for (int i = 0; i < n; ++i) {
            if (sc_tgt_h[i] >= 0) LVK_HIP(hipMemcpy(row.data(), logits_d + (size_t) i * V, V * sizeof(float), hipMemcpyDeviceToHost));
            score_host(row.data(), 1, (int) V, &sc_tgt_h[i], &probs[i]);
        }
    }
    if (argmax) std::memcpy(argmax, sc_amax_h.get(), sizeof(int) * (size_t) n);
}

// llama_eval(tokens, n, n_past) with the lm_head over every row (logits_all or not; one token: the
// matvec lm_head, a batch: the prompt matmul), enqueued eagerly and ended by the score kernel:
// probs[i] = softmax(row i)[targets[i]], -1.0f where targets[i] < 0.  The KV cache and its count
// end as after eval(); the host logits are not refreshed.  Every argument is checked before
// anything is enqueued.
void Context::eval_score(const int * tokens, int n, int n_past, const int * targets, float * probs, int * argmax) {
    const char * fn = "lvk_eval_score";
    if (!model.has_head || !model.has_embed || link) throw Error(std::string(fn) + ": not available on a stage context");
    if (!tokens) throw Error(std::string(fn) + ": null argument");
    if (n < 1 || n_past < 0 || n > n_ctx_user || n_past > n_ctx_user - n) throw Error(std::string(fn) + ": n_past + n_tokens exceeds n_ctx");
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= (int) model.hp.n_vocab) throw Error(std::string(fn) + ": token id out of range");
    score_stage(fn, n, targets, probs);
    EvalPart part;
    part.score = true;
    part.score_argmax = argmax != nullptr;
    drain_on_error(true, false, [&] { begin_eval(tokens, n, n_past, part); });
    end_eval(true);     // llama_get_logits is stale from here on, as after eval_greedy
    kv_n = n_past + n;
    score_collect(n, probs, argmax);
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
    drain_on_error(true, true, [&] { begin_eval(tokens, n, n_past, part); });
}

void Context::begin_eval(const int * tokens, int n, int n_past, const EvalPart & part) {
    const HParams & hp = model.hp;
    const int V = (int) hp.n_vocab;
    const int n_total = part.n_total < 0 ? n : part.n_total;
    if (n <= 0 || n_past < 0 || n_past + n > n_ctx_user || part.tok_off < 0 || part.tok_off + n > n_total)
        throw Error("llama.vk_amd: n_past + n_tokens exceeds n_ctx");
    if ((part.greedy || part.sample) && (!model.has_head || n != 1 || logits_all))
        throw Error("llama.vk_amd: greedy / sampling eval needs the lm_head stage, one token and last-token logits");
    if (part.score && (!model.has_head || !model.has_embed || part.n_total >= 0 || !sc_tgt_d))
        throw Error("llama.vk_amd: a scoring eval needs the whole model in one slice and its targets staged");
    if (model.has_embed) {
        if (!tokens) throw Error("llama.vk_amd: the first stage needs tokens");
        for (int i = 0; i < n; ++i)
            if (tokens[i] < 0 || tokens[i] >= V) throw Error("llama.vk_amd: token id out of range");
        std::memcpy(tok_h.get() + part.tok_off, tokens, sizeof(int) * (size_t) n);
    }
    const bool last_only = !logits_all && !part.score;      // a scoring eval: every row's logits, in HBM only
    const bool single = part.n_total < 0 || part.n_total == n;
    const bool graph_ok = n == 1 && last_only && single && use_graph && !profiling;
    // the graphs read step block 0; eager slices each take their own (the H2D copy reads
    // the pinned block when it executes, after the host may have queued further slices)
    if (!graph_ok && sp_next > n_ctx) throw Error("llama.vk_amd: too many slices before a sync");
    StepParams * sh = &sp_h[graph_ok ? 0 : sp_next++];
    sh->n_past = n_past;
    sh->n_tokens = n;
    sh->pad0 = (n == 1 && model.has_embed) ? tokens[0] : 0;
    sh->seq = next_seq();
    if (model.has_head && part.tok_off == 0 && !part.score)   // within the reserve: the pointer never moves
        logits.resize((size_t) (last_only ? 1 : n_total) * V);
    if (graph_ok) {
        const DecodeGraph kind = part.greedy ? DecodeGraph::GREEDY : part.sample ? DecodeGraph::SAMPLE : DecodeGraph::LOGITS;
        if (!graph_of(kind)) build_graph(kind);
        LVK_HIP(graph_of(kind).launch(stream));
    } else {
        LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
        if (part.sample) LVK_HIP(hipMemcpyAsync(samp_d, samp_h.get(), sizeof(SampleParams), hipMemcpyHostToDevice, stream));
        if (n > 1)
            LVK_HIP(hipMemcpyAsync(tok_d + part.tok_off, tok_h.get() + part.tok_off, sizeof(int) * (size_t) n,
                                   hipMemcpyHostToDevice, stream));
        Forward f;
        f.n = n;
        f.last_only = last_only;
        f.tok_src = tok_d + part.tok_off;
        f.logit_row = last_only ? 0 : part.tok_off;
        f.head = part.head;
        enqueue_forward(f);
        if (part.score) {
            enqueue_score(n, part.score_argmax);
        } else if (part.greedy) {
            enqueue_argmax();
        } else if (part.sample) {
            LVK_HIP(launch_sample_cand(logits_d, V, samp_d, sout_d, stream));
        } else if (model.has_head && part.copy_out) {
            LVK_HIP(hipMemcpyAsync(logits.data(), logits_d, sizeof(float) * logits.size(), hipMemcpyDeviceToHost,
                                   stream));
        }
    }
    if (want_embedding && model.has_head && part.copy_out && !part.greedy && !part.sample && !part.score) {
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
    const size_t L = model.layers.size();
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
        LVK_HIP(hipStreamSynchronize(src.stream));
        copy_kv_prefix(kc, vc, src.kc, src.vc, n_tokens);
    }
    kv_n = n_tokens;
}

void Context::copy_kv_prefix(uint16_t * dk, uint16_t * dv, const uint16_t * sk, const uint16_t * sv, int n_tokens) {
    const size_t E = model.hp.n_embd, L = model.layers.size(), C = (size_t) n_ctx, n = (size_t) n_tokens, es = kv_elem_bytes();
    LVK_HIP(hipMemcpy2DAsync(dk, C * E * es, sk, C * E * es, n * E * es, L, hipMemcpyDeviceToDevice, stream));
    LVK_HIP(hipMemcpy2DAsync(dv, C * es, sv, C * es, n * es, L * E, hipMemcpyDeviceToDevice, stream));
    LVK_HIP(hipStreamSynchronize(stream));
}

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
