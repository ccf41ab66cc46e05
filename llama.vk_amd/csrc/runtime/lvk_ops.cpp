// lvk_ops.cpp -- operator-level C ABI (include/lvk_ops.h): each op runs the
// production kernel on host buffers so tests can pin it against the oracle.
#include <algorithm>
#include <immintrin.h>

#include <cstdio>
#include <cstring>
#include <ctime>
#include <vector>

#include "../../../include/llama.h"
#include "../../../include/lvk_ops.h"
#include "lvk_split.h"

namespace {

int fail(const char * fn, const std::string & m) {
    fprintf(stderr, "%s: %s\n", fn, m.c_str());
    return -1;
}

size_t block_bytes(int type) { return type == lvk::Q4_0 ? 20 : 24; }

__attribute__((target("f16c"))) uint16_t h_f32_to_f16(float f) { return _cvtss_sh(f, 0); }

// device arrays of a quantized activation: n rows of nb blocks
lvk::ActQ actq_alloc(lvk::Scratch & dv, size_t n, size_t nb) {
    lvk::ActQ q;
    q.nb = (int) nb;
    q.d = (float *) dv.get(n * nb * 4);
    q.m = (float *) dv.get(n * nb * 4);
    q.qs = (uint4 *) dv.get(n * nb * 16);
    return q;
}

// the first n_blocks blocks of a device ActQ (d, m, qs) as reference blocks (20 / 24 bytes) in host memory
void pack_blocks(int type, const lvk::ActQ & q, size_t n_blocks, void * y) {
    std::vector<float> d(n_blocks), m(n_blocks);
    std::vector<uint8_t> qs(n_blocks * 16);
    LVK_HIP(hipMemcpy(d.data(), q.d, d.size() * 4, hipMemcpyDeviceToHost));
    LVK_HIP(hipMemcpy(m.data(), q.m, m.size() * 4, hipMemcpyDeviceToHost));
    LVK_HIP(hipMemcpy(qs.data(), q.qs, qs.size(), hipMemcpyDeviceToHost));
    uint8_t * out = (uint8_t *) y;
    const size_t bb = block_bytes(type);
    for (size_t i = 0; i < n_blocks; ++i) {
        std::memcpy(out + i * bb, &d[i], 4);
        if (type == lvk::Q4_1) std::memcpy(out + i * bb + 4, &m[i], 4);
        std::memcpy(out + i * bb + bb - 16, &qs[i * 16], 16);
    }
}

}  // namespace

extern "C" {

int lvk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lvk_set_device(int dev) { return hipSetDevice(dev) == hipSuccess ? 0 : -1; }

const char * lvk_version(void) { return "llama.vk_amd 0.1 (gfx950)"; }

int lvk_quantize_rows(int type, const float * x, int n, int k, void * y) {
    try {
        if (k % 32) return fail(__func__, "k must be a multiple of 32");
        lvk::Scratch dv;
        const size_t nb = (size_t) k / 32;
        float * xd = dv.up(x, (size_t) n * k);
        const lvk::ActQ q = actq_alloc(dv, (size_t) n, nb);
        LVK_HIP(lvk::launch_quantize_act(xd, n, k, type, q, nullptr));
        pack_blocks(type, q, (size_t) n * nb, y);
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

static int mul_mat_impl(int type, const void * w, int m, int k, const float * g, const float * x, int n, float * y,
                        bool norm) {
    if (m % 8 || k % 256) return fail("lvk_mul_mat_q", "need m % 8 == 0 and k % 256 == 0");
    lvk::Scratch dv;
    const size_t nb = (size_t) k / 32, bb = block_bytes(type);
    void * wd = dv.up((const uint8_t *) w, (size_t) m * nb * bb);
    lvk::QMatrix q;
    q.qtype = type; q.M = m; q.K = k;
    q.nib = (const uint4 *) dv.get(lvk::qimage_nib_bytes(m, k));
    q.scl = dv.get(lvk::qimage_scl_bytes(m, k, type));
    LVK_HIP(lvk::launch_repack(wd, type, m, k, (uint4 *) q.nib, (void *) q.scl, nullptr));
    lvk::StepParams sp{0, n, 0, 0};
    lvk::StepParams * spd = dv.up(&sp, 1);
    float * yd = (float *) dv.get((size_t) n * m * 4);
    lvk::MvLaunch L;
    L.w = q; L.sp = spd; L.n_tokens = n; L.y = yd;
    float * xd = dv.up(x, (size_t) n * k);
    if (type == lvk::Q4_1 || norm || (n == 1 && lvk::matvec_cu_supported(k, type))) {
        // the kernel quantizes the f32 input in its prologue: every Q4_1 kernel, the Q4_0 norm
        // kernels, and the Q4_0 single-column decode kernel (matvec_cu.hip) where compiled in
        L.x = xd;
        if (norm) L.g = dv.up(g, (size_t) k);
        LVK_HIP(lvk::launch_matvec_auto(L, norm ? lvk::PRO_NORM : lvk::PRO_ACTF, lvk::EPI_STORE, nullptr));
    } else {
        lvk::ActQ a;
        a.nb = (int) nb;
        a.d = (float *) dv.get((size_t) n * nb * 4);
        a.m = (float *) dv.get((size_t) n * nb * 4);
        a.qs = (uint4 *) dv.get((size_t) n * nb * 16);
        LVK_HIP(lvk::launch_quantize_act(xd, n, k, type, a, nullptr));
        L.xq = a;
        LVK_HIP(lvk::launch_matvec(L, lvk::PRO_ACTQ, lvk::EPI_STORE, nullptr));
    }
    LVK_HIP(hipMemcpy(y, yd, (size_t) n * m * 4, hipMemcpyDeviceToHost));
    return 0;
}

int lvk_mul_mat_q(int type, const void * w, int m, int k, const float * x, int n, float * y) {
    try { return mul_mat_impl(type, w, m, k, nullptr, x, n, y, false); }
    catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_mul_mat_q_norm(int type, const void * w, int m, int k, const float * g, const float * x, int n, float * y) {
    try { return mul_mat_impl(type, w, m, k, g, x, n, y, true); }
    catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

// y[n][M] = W . act(x) through the batched interface: operand image (xm zeroed once), then the matmul
static void mm_batched(lvk::Scratch & dv, const lvk::QMatrix & q, const float * xd, const float * gd, int n, float * yd) {
    const lvk::ActImageBytes nbytes = lvk::act_image_bytes(q.qtype, n, q.K);
    lvk::MmLaunch L;
    L.w = q; L.N = n; L.y = yd; L.ldy = q.M;
    if (q.qtype == lvk::F32 && !gd) {
        L.x.xm = (void *) xd;           // f32 weights read the f32 rows in place
    } else {
        L.x.xm = dv.get(nbytes.xm);
        LVK_HIP(hipMemset(L.x.xm, 0, nbytes.xm));
        if (nbytes.da) L.x.da = (float *) dv.get(nbytes.da);
        if (nbytes.xs) L.x.xs = dv.get(nbytes.xs);
        LVK_HIP(lvk::launch_act(q.qtype, xd, gd, n, q.K, L.x, nullptr));
    }
    LVK_HIP(lvk::launch_mm(L, lvk::EPI_STORE, nullptr));
}

int lvk_mul_mat_q_mfma(int type, const void * w, int m, int k, const float * g, const float * x, int n, float * y) {
    try {
        if (type != lvk::Q4_0 && type != lvk::Q4_1) return fail(__func__, "Q4_0 / Q4_1 only");
        if (m % 128 || k % 256 || n < 1) return fail(__func__, "need m % 128 == 0, k % 256 == 0, n >= 1");
        lvk::Scratch dv;
        const size_t nb = (size_t) k / 32;
        void * wd = dv.up((const uint8_t *) w, (size_t) m * nb * (type == lvk::Q4_0 ? 20 : 24));
        lvk::QMatrix q;
        q.qtype = type; q.M = m; q.K = k;
        q.nib = (const uint4 *) dv.get(lvk::qimage_nib_bytes(m, k));
        q.scl = dv.get(lvk::qimage_scl_bytes(m, k, type));
        LVK_HIP(lvk::launch_repack(wd, type, m, k, (uint4 *) q.nib, (void *) q.scl, nullptr));
        if (type == lvk::Q4_1) {            // the Q4_1 path always runs on its f16 + side images
            q.a16 = dv.get(lvk::mm_a16_bytes(m, k));
            q.side = dv.get(lvk::mm41_side_bytes(m, k));
            LVK_HIP(lvk::launch_build_mm41(q, (void *) q.a16, (void *) q.side, nullptr));
        } else if (lvk::prompt_a16_env()) {  // the f16 A-fragment variant, as the model loader builds it
            q.a16 = dv.get(lvk::mm_a16_bytes(m, k));
            LVK_HIP(lvk::launch_build_a16(q, (void *) q.a16, nullptr));
        }
        float * xd = dv.up(x, (size_t) n * k);
        const float * gd = g ? dv.up(g, (size_t) k) : nullptr;
        float * yd = (float *) dv.get((size_t) n * m * 4);
        mm_batched(dv, q, xd, gd, n, yd);
        LVK_HIP(hipMemcpy(y, yd, (size_t) n * m * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_mul_mat_f16(const uint16_t * w, int m, int k, const float * g, const float * x, int n, float * y, int kernel) {
    try {
        if (!w || !x || !y || m < 1 || n < 1 || k < 256 || k % 256) return fail(__func__, "need m >= 1, n >= 1, k % 256 == 0");
        if (kernel < 0 || kernel > 2 || (kernel == 1 && n != 1)) return fail(__func__, "kernel: 0 auto, 1 decode matvec (n == 1), 2 batched");
        if (kernel == 0) kernel = n == 1 ? 1 : 2;
        lvk::Scratch dv;
        const uint16_t * wd = dv.up(w, (size_t) m * k);
        lvk::QMatrix q;
        q.qtype = lvk::F16; q.M = m; q.K = k;
        q.nib = (const uint4 *) dv.get(lvk::f16_image_bytes(m, k));
        LVK_HIP(lvk::launch_repack_f16(wd, m, k, (uint4 *) q.nib, nullptr));
        float * xd = dv.up(x, (size_t) n * k);
        const float * gd = g ? dv.up(g, (size_t) k) : nullptr;
        float * yd = (float *) dv.get((size_t) n * m * 4);
        if (kernel == 1) {
            lvk::StepParams sp{0, 1, 0, 0};
            lvk::MvLaunch L;
            L.w = q; L.x = xd; L.g = gd; L.sp = dv.up(&sp, 1); L.y = yd;
            LVK_HIP(lvk::launch_matvec_f16(L, g ? lvk::PRO_NORM : lvk::PRO_ACTF, lvk::EPI_STORE, nullptr));
        } else {
            mm_batched(dv, q, xd, gd, n, yd);
        }
        LVK_HIP(hipMemcpy(y, yd, (size_t) n * m * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_mul_mat_f32(const float * w, int m, int k, const float * g, const float * x, int n, float * y, int kernel) {
    try {
        if (!w || !x || !y || m < 1 || n < 1 || k < 256 || k % 256) return fail(__func__, "need m >= 1, n >= 1, k % 256 == 0");
        if (kernel < 0 || kernel > 2 || (kernel == 1 && n != 1)) return fail(__func__, "kernel: 0 auto, 1 decode matvec (n == 1), 2 batched");
        if (kernel == 0) kernel = n == 1 ? 1 : 2;
        lvk::Scratch dv;
        const float * wd = dv.up(w, (size_t) m * k);
        lvk::QMatrix q;
        q.qtype = lvk::F32; q.M = m; q.K = k;
        q.nib = (const uint4 *) dv.get(lvk::f32_image_bytes(m, k));
        LVK_HIP(lvk::launch_repack_f32(wd, m, k, (uint4 *) q.nib, nullptr));
        float * xd = dv.up(x, (size_t) n * k);
        const float * gd = g ? dv.up(g, (size_t) k) : nullptr;
        float * yd = (float *) dv.get((size_t) n * m * 4);
        if (kernel == 1) {
            lvk::StepParams sp{0, 1, 0, 0};
            lvk::MvLaunch L;
            L.w = q; L.x = xd; L.g = gd; L.sp = dv.up(&sp, 1); L.y = yd;
            LVK_HIP(lvk::launch_matvec_f32(L, g ? lvk::PRO_NORM : lvk::PRO_ACTF, lvk::EPI_STORE, nullptr));
        } else {
            mm_batched(dv, q, xd, gd, n, yd);
        }
        LVK_HIP(hipMemcpy(y, yd, (size_t) n * m * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_attention_scores(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                         int n_ctx, int n_past, int n, float * out, float * scores_out);
int lvk_attention(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head, int n_ctx,
                  int n_past, int n, float * out) {
    return lvk_attention_scores(kc, vc, q, n_embd, n_head, n_ctx, n_past, n, out, nullptr);
}

static int attention_impl(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                          int n_ctx, int n_past, int n, float * out, float * scores_out, int kind,
                          int type = lvk::Q4_0, void * blocks = nullptr);

int lvk_attention_scores(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                         int n_ctx, int n_past, int n, float * out, float * scores_out) {
    return attention_impl(kc, vc, q, n_embd, n_head, n_ctx, n_past, n, out, scores_out, 0);
}

int lvk_attention_prompt(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                         int n_ctx, int n_past, int n, float * out) {
    if (!lvk::attention_prompt_supported(n_embd, n_head, n_ctx))
        return fail(__func__, "needs head_dim 128, n_ctx % 32 == 0, n_ctx <= 1024");
    return attention_impl(kc, vc, q, n_embd, n_head, n_ctx, n_past, n, out, nullptr, 1);
}

int lvk_attention_decode(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                         int n_ctx, int n_past, float * out) {
    if (!lvk::attention_decode_supported(n_embd, n_head, n_ctx))
        return fail(__func__, "needs head_dim 128, n_ctx % 64 == 0, n_ctx <= 2048");
    return attention_impl(kc, vc, q, n_embd, n_head, n_ctx, n_past, 1, out, nullptr, 2);
}

int lvk_attn_helpers_active(int n_embd, int n_head, int n_ctx) {
    if (n_embd < 1 || n_head < 1 || n_ctx < 1) return 0;
    return lvk::attention_decode_helpers(n_embd, n_head, n_ctx);
}

int lvk_attention_q(int kind, int type, const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd,
                    int n_head, int n_ctx, int n_past, int n, float * out, void * blocks) {
    if (kind < 0 || kind > 2) return fail(__func__, "kind: 0 lvk_attention, 1 lvk_attention_prompt, 2 lvk_attention_decode");
    if (type != lvk::Q4_0 && type != lvk::Q4_1) return fail(__func__, "type: 2 (Q4_0) or 3 (Q4_1)");
    if (!kc || !vc || !q || !out || n_head < 1 || n_embd != n_head * 128 || n < 1 || n_past < 0 || n_ctx < 1 ||
        n_past > n_ctx - n)
        return fail(__func__, "need head_dim 128, n >= 1 and 0 <= n_past <= n_ctx - n");
    if (kind == 1 && !lvk::attention_prompt_supported(n_embd, n_head, n_ctx))
        return fail(__func__, "kind 1 needs head_dim 128, n_ctx % 32 == 0, n_ctx <= 1024");
    if (kind == 2 && (n != 1 || !lvk::attention_decode_supported(n_embd, n_head, n_ctx)))
        return fail(__func__, "kind 2 needs n == 1, head_dim 128, n_ctx % 64 == 0, n_ctx <= 2048");
    return attention_impl(kc, vc, q, n_embd, n_head, n_ctx, n_past, n, out, nullptr, kind, type, blocks);
}

static int attention_impl(const uint16_t * kc, const uint16_t * vc, const float * q, int n_embd, int n_head,
                          int n_ctx, int n_past, int n, float * out, float * scores_out, int kind, int type,
                          void * blocks) {
    const char * fn = kind == 1 ? "lvk_attention_prompt" : kind == 2 ? "lvk_attention_decode" : "lvk_attention";
    try {
        lvk::Scratch dv;
        const size_t CE = (size_t) n_ctx * n_embd;
        std::vector<uint16_t> q16((size_t) n * n_embd);
        for (size_t i = 0; i < q16.size(); ++i) q16[i] = h_f32_to_f16(q[i]);   // ggml.c:6420-6433
        lvk::StepParams sp{n_past, n, 0, 0};
        lvk::AttnLaunch A{};
        A.q16 = dv.up(q16.data(), q16.size());
        A.kc = dv.up(kc, CE);
        A.vc = dv.up(vc, CE);
        A.scores = (float *) dv.get((size_t) n * n_head * n_ctx * 4);
        A.out = actq_alloc(dv, (size_t) n, (size_t) n_embd / 32);
        A.out_qtype = type;
        std::vector<uint16_t> te, ts;
        lvk::host_fp16_tables(te, ts);
        A.exp_tab = dv.up(te.data(), te.size());
        A.exp_computed = lvk::pick_exp_mode(A.exp_tab);
        A.sp = dv.up(&sp, 1);
        A.n_tokens = n; A.n_embd = n_embd; A.n_head = n_head; A.n_ctx = n_ctx;
        float * od = (float *) dv.get((size_t) n * n_embd * 4);
        A.out_f32 = od;
        uint16_t * pd = nullptr;
        if (scores_out) pd = (uint16_t *) dv.get((size_t) n * n_head * n_ctx * 2);
        A.p16_out = pd;
        if (kind == 1) LVK_HIP(lvk::launch_attention_prompt(A, (uint16_t *) A.scores, lvk::ActImage{}, nullptr));
        else if (kind == 2) {
            void * gran = dv.get(lvk::attention_decode_scratch_bytes(n_head, n_ctx));
            LVK_HIP(hipMemset(gran, 0, lvk::attention_decode_scratch_bytes(n_head, n_ctx)));
            LVK_HIP(lvk::launch_attention_decode(A, gran, 1, nullptr));
        }
        else LVK_HIP(lvk::launch_attention(A, nullptr));
        LVK_HIP(hipMemcpy(out, od, (size_t) n * n_embd * 4, hipMemcpyDeviceToHost));
        if (blocks) pack_blocks(type, A.out, (size_t) n * A.out.nb, blocks);
        if (scores_out) {
            LVK_HIP(hipMemcpy(scores_out, A.scores, (size_t) n * n_head * n_ctx * 4, hipMemcpyDeviceToHost));
            // the f16 probabilities follow the scores (lvk_ops.h: scores_out holds 1.5x the floats)
            LVK_HIP(hipMemcpy(scores_out + (size_t) n * n_head * n_ctx, pd, (size_t) n * n_head * n_ctx * 2,
                              hipMemcpyDeviceToHost));
        }
        return 0;
    } catch (const lvk::Error & e) { return fail(fn, e.msg); }
}

// ---- the batched-decode rows kernels (attention_rows.hip) on host data
namespace {

// the host-side checks of both rows entry points: nothing out of range reaches a kernel
const char * rows_args_bad(const int * slots, const int * pos, int n, int n_embd, int n_head, int n_ctx, int n_slots,
                           int n_layer, int layer) {
    if (!slots || !pos) return "null argument";
    if (n < 1) return "n must be >= 1";
    if (n_slots < 1 || n_layer < 1) return "n_slots and n_layer must be >= 1";
    if (layer < 0 || layer >= n_layer) return "layer outside 0..n_layer-1";
    if (!lvk::attention_rows_supported(n_embd, n_head, n_ctx)) return "needs head_dim 128, n_ctx % 32 == 0, n_ctx >= 128";
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= n_slots) return "a slot outside 0..n_slots-1";
        if (pos[i] < 0 || pos[i] >= n_ctx) return "a position outside 0..n_ctx-1";
    }
    return nullptr;
}

// host caches [n_slots][n_layer][n_ctx * n_embd] -> device copies, the slot table and the row table
struct RowsDev {
    uint16_t * kc, * vc;
    lvk::SeqSlot * slots;
    lvk::SeqRow * rows;
    size_t layer_off, total;
};
RowsDev rows_upload(lvk::Scratch & dv, const uint16_t * kc, const uint16_t * vc, const int * slots, const int * pos, int n,
                    int n_embd, int n_ctx, int n_slots, int n_layer, int layer) {
    const size_t CE = (size_t) n_ctx * n_embd;
    RowsDev r;
    r.total = (size_t) n_slots * n_layer * CE;
    r.layer_off = (size_t) layer * CE;
    r.kc = dv.up(kc, r.total);
    r.vc = dv.up(vc, r.total);
    std::vector<lvk::SeqSlot> st((size_t) n_slots);
    for (int s = 0; s < n_slots; ++s) st[(size_t) s] = {r.kc + (size_t) s * n_layer * CE, r.vc + (size_t) s * n_layer * CE};
    std::vector<lvk::SeqRow> rw((size_t) n);
    for (int i = 0; i < n; ++i) rw[(size_t) i] = {slots[i], pos[i]};
    r.slots = dv.up(st.data(), st.size());
    r.rows = dv.up(rw.data(), rw.size());
    return r;
}

}  // namespace

int lvk_rope_kv_rows(const float * qkv, const int * slots, const int * pos, int n, int n_embd, int n_head, int n_ctx,
                     int n_slots, int n_layer, int layer, uint16_t * kc, uint16_t * vc, uint16_t * q16_out) {
    try {
        if (!qkv || !kc || !vc || !q16_out) return fail(__func__, "null argument");
        if (const char * bad = rows_args_bad(slots, pos, n, n_embd, n_head, n_ctx, n_slots, n_layer, layer))
            return fail(__func__, bad);
        lvk::Scratch dv;
        const int hd = n_embd / n_head;
        const RowsDev r = rows_upload(dv, kc, vc, slots, pos, n, n_embd, n_ctx, n_slots, n_layer, layer);
        std::vector<float2> rt;
        lvk::host_rope_table(rt, (size_t) n_ctx, (size_t) hd);
        const float2 * rope = dv.up(rt.data(), rt.size());
        const float * qd = dv.up(qkv, (size_t) n * 3 * n_embd);
        uint16_t * q16 = (uint16_t *) dv.get((size_t) n * n_embd * 2);
        LVK_HIP(lvk::launch_rope_kv_rows(qd, n, n_embd, hd, rope, r.rows, r.slots, r.layer_off, n_ctx, q16, nullptr));
        LVK_HIP(hipMemcpy(q16_out, q16, (size_t) n * n_embd * 2, hipMemcpyDeviceToHost));
        LVK_HIP(hipMemcpy(kc, r.kc, r.total * 2, hipMemcpyDeviceToHost));
        LVK_HIP(hipMemcpy(vc, r.vc, r.total * 2, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_attention_rows(int type, const uint16_t * kc, const uint16_t * vc, int n_slots, int n_layer, int layer,
                       const float * q, const int * slots, const int * pos, int n, int n_embd, int n_head, int n_ctx,
                       float * out, void * blocks) {
    try {
        if (!kc || !vc || !q || !out) return fail(__func__, "null argument");
        if (type != lvk::Q4_0 && type != lvk::Q4_1) return fail(__func__, "type: 2 (Q4_0) or 3 (Q4_1)");
        if (const char * bad = rows_args_bad(slots, pos, n, n_embd, n_head, n_ctx, n_slots, n_layer, layer))
            return fail(__func__, bad);
        lvk::Scratch dv;
        const RowsDev r = rows_upload(dv, kc, vc, slots, pos, n, n_embd, n_ctx, n_slots, n_layer, layer);
        std::vector<uint16_t> q16((size_t) n * n_embd);
        for (size_t i = 0; i < q16.size(); ++i) q16[i] = h_f32_to_f16(q[i]);   // ggml.c:6420-6433
        lvk::AttnLaunch A{};
        A.q16 = dv.up(q16.data(), q16.size());
        A.out = actq_alloc(dv, (size_t) n, (size_t) n_embd / 32);
        A.out_qtype = type;
        std::vector<uint16_t> te, ts;
        lvk::host_fp16_tables(te, ts);
        A.exp_tab = dv.up(te.data(), te.size());
        A.exp_computed = lvk::pick_exp_mode(A.exp_tab);
        A.n_tokens = n; A.n_embd = n_embd; A.n_head = n_head; A.n_ctx = n_ctx;
        float * od = (float *) dv.get((size_t) n * n_embd * 4);
        A.out_f32 = od;
        LVK_HIP(lvk::launch_attention_rows(A, r.rows, r.slots, r.layer_off, nullptr));
        LVK_HIP(hipMemcpy(out, od, (size_t) n * n_embd * 4, hipMemcpyDeviceToHost));
        if (blocks) pack_blocks(type, A.out, (size_t) n * A.out.nb, blocks);
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

}  // extern "C"

// ---- the fused steps of a transformer layer (lvk_context.cpp enqueue_forward) on host data
namespace {

bool type_ok(int type) { return type == lvk::F32 || type == lvk::F16 || type == lvk::Q4_0 || type == lvk::Q4_1; }
bool is_q4(int type) { return type == lvk::Q4_0 || type == lvk::Q4_1; }

// bytes of a file-layout row of k weights
size_t row_bytes(int type, int k) {
    if (type == lvk::F32) return (size_t) k * 4;
    if (type == lvk::F16) return (size_t) k * 2;
    return (size_t) (k / 32) * block_bytes(type);
}

// the checks every layer entry point shares; nullptr when they pass
const char * layer_args_bad(int type, int path, int k, int n) {
    if (!type_ok(type)) return "type: 0 f32, 1 f16, 2 Q4_0, 3 Q4_1";
    if (path < 0 || path > 3) return "path: 0 as a context chooses, 1 launch_matvec_cu, 2 launch_matvec, 3 launch_act + launch_mm";
    if (k < 256 || k % 256) return "k must be a positive multiple of 256";
    if (n < 1 || n > 4096) return "n must be in 1..4096";
    if (path == 1 && n != 1) return "path 1 (launch_matvec_cu) takes n == 1";
    return nullptr;
}

// path 0 of a batch: use_batched's rule (lvk_context.cpp): f16 / f32 weights from 2 tokens on,
// the Q4 types from 16
int batch_path(int type, int n) { return is_q4(type) && n < 16 ? 2 : 3; }

// the device image of M rows (file layout: rows_a, then rows_b when the matrix is two stacked
// ones), built as the model loader builds it (lvk_model.cpp repack): the octet image, and for the
// batched route the prompt images of the Q4 types
lvk::QMatrix layer_matrix(lvk::Scratch & dv, int type, const void * rows_a, int Ma, const void * rows_b, int Mb, int K,
                          int interleave4, bool batched) {
    const int M = Ma + Mb;
    const size_t rb = row_bytes(type, K);
    uint8_t * stage = (uint8_t *) dv.get((size_t) M * rb);
    LVK_HIP(hipMemcpy(stage, rows_a, (size_t) Ma * rb, hipMemcpyHostToDevice));
    if (Mb) LVK_HIP(hipMemcpy(stage + (size_t) Ma * rb, rows_b, (size_t) Mb * rb, hipMemcpyHostToDevice));
    lvk::QMatrix q;
    q.qtype = type; q.M = M; q.K = K;
    if (type == lvk::F16) {
        q.nib = (const uint4 *) dv.get(lvk::f16_image_bytes(M, K));
        LVK_HIP(lvk::launch_repack_f16(stage, M, K, (uint4 *) q.nib, nullptr, interleave4));
        return q;
    }
    if (type == lvk::F32) {
        q.nib = (const uint4 *) dv.get(lvk::f32_image_bytes(M, K));
        LVK_HIP(lvk::launch_repack_f32(stage, M, K, (uint4 *) q.nib, nullptr, interleave4));
        return q;
    }
    q.nib = (const uint4 *) dv.get(lvk::qimage_nib_bytes(M, K));
    q.scl = dv.get(lvk::qimage_scl_bytes(M, K, type));
    LVK_HIP(lvk::launch_repack(stage, type, M, K, (uint4 *) q.nib, (void *) q.scl, nullptr, interleave4));
    if (batched && type == lvk::Q4_1) {
        q.a16 = dv.get(lvk::mm_a16_bytes(M, K));
        q.side = dv.get(lvk::mm41_side_bytes(M, K));
        LVK_HIP(lvk::launch_build_mm41(q, (void *) q.a16, (void *) q.side, nullptr));
    } else if (batched && type == lvk::Q4_0 && lvk::prompt_a16_env()) {
        q.a16 = dv.get(lvk::mm_a16_bytes(M, K));
        LVK_HIP(lvk::launch_build_a16(q, (void *) q.a16, nullptr));
    }
    return q;
}

// an operand image for n rows of K (xm zeroed once, lvk_kernels.h ActImage)
lvk::ActImage layer_image(lvk::Scratch & dv, int type, int n, int K) {
    const lvk::ActImageBytes nbytes = lvk::act_image_bytes(type, n, K);
    lvk::ActImage im;
    im.xm = dv.get(nbytes.xm);
    LVK_HIP(hipMemset(im.xm, 0, nbytes.xm));
    if (nbytes.da) im.da = (float *) dv.get(nbytes.da);
    if (nbytes.xs) im.xs = dv.get(nbytes.xs);
    return im;
}

// x[n][K] (rms_norm * g when g) as the batched matmul's operand: enqueue_forward's `act`
lvk::ActImage layer_act(int type, const float * xd, const float * gd, int n, int K, const lvk::ActImage & img) {
    if (type == lvk::F32 && !gd) {
        lvk::ActImage in;
        in.xm = (void *) xd;
        return in;
    }
    LVK_HIP(lvk::launch_act(type, xd, gd, n, K, img, nullptr));
    return img;
}

hipError_t mv_by_path(int path, const lvk::MvLaunch & L, int pro, int epi) {
    if (path == 1) return lvk::launch_matvec_cu(L, pro, epi, nullptr);
    if (path == 2) return lvk::launch_matvec(L, pro, epi, nullptr);
    return lvk::launch_matvec_auto(L, pro, epi, nullptr);
}

const uint16_t * silu_table(lvk::Scratch & dv) {
    std::vector<uint16_t> te, ts;
    lvk::host_fp16_tables(te, ts);
    return dv.up(ts.data(), ts.size());
}

}  // namespace

extern "C" {

int lvk_layer_qkv(int type, int path, const void * w, int n_embd, int n_head, int k, const float * g, const float * x,
                  int n, int n_ctx, int n_past, int fused, uint16_t * kc, uint16_t * vc, uint16_t * q16_out) {
    try {
        if (!w || !g || !x || !kc || !vc || !q16_out) return fail(__func__, "null argument");
        if (const char * bad = layer_args_bad(type, path, k, n)) return fail(__func__, bad);
        if (n_head < 1 || n_embd < 32 || n_embd % 32 || n_embd % n_head || (n_embd / n_head) % 4 || n_embd > 16384)
            return fail(__func__, "need n_embd % 32 == 0, n_embd <= 16384 and a head_dim that is a multiple of 4");
        if (n_ctx < 1 || n_ctx > 16384 || n_past < 0 || n_past > n_ctx - n)
            return fail(__func__, "need 1 <= n_ctx <= 16384 and 0 <= n_past <= n_ctx - n");
        if (fused != 0 && fused != 1) return fail(__func__, "fused: 0 or 1");
        if (path == 0 && n > 1) path = batch_path(type, n);
        if (path == 3 && fused && !lvk::mm_epi_supported(type, lvk::EPI_ROPE_KV))
            return fail(__func__, "the batched matmul fuses RoPE + KV append for Q4_0 / Q4_1 only");
        if (path == 3 && is_q4(type) && n_embd % 128) return fail(__func__, "the Q4 batched matmul needs n_embd % 128 == 0");
        lvk::Scratch dv;
        const int E = n_embd, hd = n_embd / n_head;
        const size_t CE = (size_t) n_ctx * E;
        const lvk::QMatrix q = layer_matrix(dv, type, w, 3 * E, nullptr, 0, k, 0, path == 3);
        std::vector<float2> rt;
        lvk::host_rope_table(rt, (size_t) n_ctx, (size_t) hd);
        const float2 * rope = dv.up(rt.data(), rt.size());
        lvk::StepParams sp{n_past, n, 0, 0};
        const lvk::StepParams * spd = dv.up(&sp, 1);
        const float * xd = dv.up(x, (size_t) n * k);
        const float * gd = dv.up(g, (size_t) k);
        uint16_t * kcd = dv.up(kc, CE);
        uint16_t * vcd = dv.up(vc, CE);
        uint16_t * q16 = (uint16_t *) dv.get((size_t) n * E * 2);
        float * qkv32 = fused ? nullptr : (float *) dv.get((size_t) n * 3 * E * 4);
        if (path == 3) {
            const lvk::ActImage img = layer_image(dv, type, n, k);
            lvk::MmLaunch L;
            L.w = q; L.x = layer_act(type, xd, gd, n, k, img); L.N = n;
            const lvk::RopeKV rk{rope, spd, n_ctx, E, hd, q16, kcd, vcd};
            if (fused) {
                L.rk = &rk;
                LVK_HIP(lvk::launch_mm(L, lvk::EPI_ROPE_KV, nullptr));
            } else {
                L.y = qkv32; L.ldy = 3 * E;
                LVK_HIP(lvk::launch_mm(L, lvk::EPI_STORE, nullptr));
            }
        } else {
            lvk::MvLaunch a;
            a.w = q; a.x = xd; a.g = gd; a.sp = spd; a.n_tokens = n;
            a.q16 = q16; a.kc = kcd; a.vc = vcd; a.rope.cs = rope;
            a.n_embd = E; a.head_dim = hd; a.n_ctx = n_ctx;
            a.y = qkv32;
            LVK_HIP(mv_by_path(path, a, lvk::PRO_NORM, fused ? lvk::EPI_QKV : lvk::EPI_STORE));
        }
        if (!fused) LVK_HIP(lvk::launch_rope_kv(qkv32, n, E, hd, rope, spd, n_ctx, q16, kcd, vcd, nullptr));
        LVK_HIP(hipMemcpy(q16_out, q16, (size_t) n * E * 2, hipMemcpyDeviceToHost));
        LVK_HIP(hipMemcpy(kc, kcd, CE * 2, hipMemcpyDeviceToHost));
        LVK_HIP(hipMemcpy(vc, vcd, CE * 2, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_layer_resid(int type, int path, const void * w, int m, int k, const float * a, int n, int input, float * y) {
    try {
        if (!w || !a || !y) return fail(__func__, "null argument");
        if (const char * bad = layer_args_bad(type, path, k, n)) return fail(__func__, bad);
        if (m < 8 || m % 8 || m > (1 << 20)) return fail(__func__, "the EPI_RESID kernels need m % 8 == 0");
        if (input != 0 && input != 1) return fail(__func__, "input: 0 f32 rows, 1 quantized blocks");
        if (input == 1 && !is_q4(type)) return fail(__func__, "input 1 (quantized blocks) is for Q4_0 / Q4_1 weights");
        if (path == 0 && n > 1) path = batch_path(type, n);
        // a single token as a context runs it: the Q4 W2 role is the CU kernels' (PRO_ACTF)
        if (path == 0 && input == 0 && is_q4(type)) path = 1;
        if (path == 3 && is_q4(type) && m % 128) return fail(__func__, "the Q4 batched matmul needs m % 128 == 0");
        lvk::Scratch dv;
        const lvk::QMatrix q = layer_matrix(dv, type, w, m, nullptr, 0, k, 0, path == 3);
        const float * ad = dv.up(a, (size_t) n * k);
        float * yd = dv.up(y, (size_t) n * m);
        lvk::ActQ aq;
        if (input == 1) {
            aq = actq_alloc(dv, (size_t) n, (size_t) k / 32);
            LVK_HIP(lvk::launch_quantize_act(ad, n, k, type, aq, nullptr));
        }
        if (path == 3) {
            const lvk::ActImage img = layer_image(dv, type, n, k);
            lvk::MmLaunch L;
            L.w = q; L.N = n; L.y = yd; L.ldy = m;
            if (input == 1) {
                LVK_HIP(lvk::launch_actq_to_image(type, aq, n, k, img, nullptr));
                L.x = img;
            } else {
                L.x = layer_act(type, ad, nullptr, n, k, img);
            }
            LVK_HIP(lvk::launch_mm(L, lvk::EPI_RESID, nullptr));
        } else {
            lvk::StepParams sp{0, n, 0, 0};
            lvk::MvLaunch b;
            b.w = q; b.y = yd; b.sp = dv.up(&sp, 1); b.n_tokens = n;
            if (input == 1) b.xq = aq; else b.x = ad;
            LVK_HIP(mv_by_path(path, b, input == 1 ? lvk::PRO_ACTQ : lvk::PRO_ACTF, lvk::EPI_RESID));
        }
        LVK_HIP(hipMemcpy(y, yd, (size_t) n * m * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_layer_swiglu(int type, int path, const void * w1, const void * w3, int f, int k, const float * g, const float * x,
                     int n, float * u_out, void * blocks_out) {
    try {
        if (!w1 || !w3 || !g || !x) return fail(__func__, "null argument");
        if (const char * bad = layer_args_bad(type, path, k, n)) return fail(__func__, bad);
        if (f < 4 || f % 4 || f > (1 << 19)) return fail(__func__, "the interleaved W1|W3 image needs f % 4 == 0");
        if (path == 0)
            path = n > 1 ? batch_path(type, n)
                         : lvk::matvec_cu_supported(k, type) && lvk::matvec_cu_supported(f, type) ? 1 : 2;
        if (path == 2) {
            if (!is_q4(type)) return fail(__func__, "path 2 (EPI_SWIGLU, quantized output) is for Q4_0 / Q4_1 weights");
            if (!blocks_out || u_out) return fail(__func__, "path 2 produces blocks_out only");
            if (f % 32) return fail(__func__, "path 2 needs f % 32 == 0");
        } else {
            if (!u_out || blocks_out) return fail(__func__, "paths 1 and 3 produce u_out only");
            if (path == 3 && is_q4(type) && f % 64) return fail(__func__, "the Q4 batched matmul needs f % 64 == 0");
        }
        lvk::Scratch dv;
        const lvk::QMatrix q = layer_matrix(dv, type, w1, f, w3, f, k, 1, path == 3);
        const float * xd = dv.up(x, (size_t) n * k);
        const float * gd = dv.up(g, (size_t) k);
        const uint16_t * st = silu_table(dv);
        if (path == 2) {
            const lvk::ActQ out = actq_alloc(dv, (size_t) n, (size_t) f / 32);
            lvk::StepParams sp{0, n, 0, 0};
            lvk::MvLaunch c;
            c.w = q; c.x = xd; c.g = gd; c.sp = dv.up(&sp, 1); c.n_tokens = n; c.silu_tab = st; c.out_q = out;
            LVK_HIP(lvk::launch_matvec(c, lvk::PRO_NORM, lvk::EPI_SWIGLU, nullptr));
            pack_blocks(type, out, (size_t) n * (f / 32), blocks_out);
            return 0;
        }
        float * ud = (float *) dv.get((size_t) n * f * 4);
        if (path == 3) {
            const lvk::ActImage img = layer_image(dv, type, n, k);
            lvk::MmLaunch L;
            L.w = q; L.x = layer_act(type, xd, gd, n, k, img); L.N = n; L.y = ud; L.ldy = f; L.silu_tab = st;
            LVK_HIP(lvk::launch_mm(L, lvk::EPI_SWIGLU_F32, nullptr));
        } else {
            lvk::StepParams sp{0, 1, 0, 0};
            lvk::MvLaunch c;
            c.w = q; c.x = xd; c.g = gd; c.sp = dv.up(&sp, 1); c.n_tokens = 1; c.silu_tab = st; c.u = ud;
            LVK_HIP(lvk::launch_matvec_cu(c, lvk::PRO_NORM, lvk::EPI_SWIGLU_F32, nullptr));
        }
        LVK_HIP(hipMemcpy(u_out, ud, (size_t) n * f * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_layer_ffn(int type, const void * w1, const void * w3, const void * w2, int f, int k, const float * g, float * x,
                  int n, int swiglu_q) {
    try {
        if (!w1 || !w3 || !w2 || !g || !x) return fail(__func__, "null argument");
        if (const char * bad = layer_args_bad(type, 3, k, n)) return fail(__func__, bad);
        if (f < 256 || f % 256 || f > (1 << 19)) return fail(__func__, "f must be a positive multiple of 256");
        if (swiglu_q != 0 && swiglu_q != 1) return fail(__func__, "swiglu_q: 0 or 1");
        if (swiglu_q && !lvk::mm_epi_supported(type, lvk::EPI_SWIGLU_Q))
            return fail(__func__, "swiglu_q = 1 (EPI_SWIGLU_Q) is for Q4_0 weights");
        lvk::Scratch dv;
        const lvk::QMatrix q13 = layer_matrix(dv, type, w1, f, w3, f, k, 1, true);
        const lvk::QMatrix q2 = layer_matrix(dv, type, w2, k, nullptr, 0, f, 0, true);
        float * xd = dv.up(x, (size_t) n * k);
        const float * gd = dv.up(g, (size_t) k);
        const uint16_t * st = silu_table(dv);
        // one operand image for both matrices, as a context holds it (sized for the longer row)
        const lvk::ActImage img = layer_image(dv, type, n, std::max(k, f));
        lvk::MmLaunch a;
        a.w = q13; a.x = layer_act(type, xd, gd, n, k, img); a.N = n; a.silu_tab = st;
        lvk::MmLaunch b;
        b.w = q2; b.N = n; b.y = xd; b.ldy = k; b.silu_tab = st;
        if (swiglu_q) {
            a.out = layer_image(dv, type, n, f);
            LVK_HIP(lvk::launch_mm(a, lvk::EPI_SWIGLU_Q, nullptr));
            b.x = a.out;
        } else {
            float * uf = (float *) dv.get((size_t) n * f * 4);
            a.y = uf; a.ldy = f;
            LVK_HIP(lvk::launch_mm(a, lvk::EPI_SWIGLU_F32, nullptr));
            b.x = layer_act(type, uf, nullptr, n, f, img);
        }
        LVK_HIP(lvk::launch_mm(b, lvk::EPI_RESID, nullptr));
        LVK_HIP(hipMemcpy(x, xd, (size_t) n * k * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_embed_rows(int type, const void * emb, int n_vocab, int n_embd, const int * tokens, int n, float * x_out) {
    try {
        if (!emb || !tokens || !x_out) return fail(__func__, "null argument");
        if (!type_ok(type)) return fail(__func__, "type: 0 f32, 1 f16, 2 Q4_0, 3 Q4_1");
        if (n_vocab < 1 || n_vocab > (1 << 20) || n_embd < 32 || n_embd % 32 || n_embd > 16384 || n < 1 || n > 4096)
            return fail(__func__, "need n_vocab >= 1, n_embd % 32 == 0 and 1 <= n <= 4096");
        for (int i = 0; i < n; ++i)
            if (tokens[i] < 0 || tokens[i] >= n_vocab) return fail(__func__, "a token id outside 0..n_vocab-1");
        lvk::Scratch dv;
        const uint8_t * ed = dv.up((const uint8_t *) emb, (size_t) n_vocab * row_bytes(type, n_embd));
        const int * td = dv.up(tokens, (size_t) n);
        float * xd = (float *) dv.get((size_t) n * n_embd * 4);
        LVK_HIP(lvk::launch_embed(ed, type, n_embd, td, n, xd, nullptr));
        LVK_HIP(hipMemcpy(x_out, xd, (size_t) n * n_embd * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_exp_table_mismatches(void) {
    try {
        lvk::Scratch dv;
        std::vector<uint16_t> te, ts;
        lvk::host_fp16_tables(te, ts);
        const uint16_t * tab = dv.up(te.data(), te.size());
        int * bad_d = (int *) dv.get(2 * sizeof(int));
        int bad[2] = {-1, -1};
        LVK_HIP(lvk::exp_check(tab, bad_d, nullptr));
        LVK_HIP(hipMemcpy(bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost));
        return bad[1] == 0 ? 0 : bad[0];     // the computed exp a context would use (f32, else double)
    } catch (const std::exception & e) {
        return fail("lvk_exp_table_mismatches", e.what());
    }
}

int lvk_rms_norm_mul(const float * x, const float * g, int k, int n, float * y) {
    try {
        lvk::Scratch dv;
        float * xd = dv.up(x, (size_t) n * k);
        float * gd = dv.up(g, (size_t) k);
        float * yd = (float *) dv.get((size_t) n * k * 4);
        LVK_HIP(lvk::launch_rmsnorm_rows(xd, gd, k, n, yd, nullptr));
        LVK_HIP(hipMemcpy(y, yd, (size_t) n * k * 4, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

void lvk_host_tables(uint16_t * exp_tab, uint16_t * silu_tab) {
    std::vector<uint16_t> te, ts;
    lvk::host_fp16_tables(te, ts);
    std::memcpy(exp_tab, te.data(), 65536 * 2);
    std::memcpy(silu_tab, ts.data(), 65536 * 2);
}

// settings and profiles of a layer-split context cover every stage
void lvk_set_profiling(struct llama_context * ctx, int on) {
    for (lvk::Context * c : ctx->stages()) c->profiling = on != 0;
}
void lvk_reset_profile(struct llama_context * ctx) {
    for (lvk::Context * c : ctx->stages()) c->prof = lvk::Profile{};
}
int lvk_get_profile(struct llama_context * ctx, double * ms, long * launches, double * bytes, int n) {
    for (int i = 0; i < n && i < lvk::K_NCLASS; ++i) {
        ms[i] = 0;
        launches[i] = 0;
        bytes[i] = 0;
        for (lvk::Context * c : ctx->stages()) {
            ms[i] += c->prof.ms[i];
            launches[i] += c->prof.launches[i];
            bytes[i] += c->prof.bytes[i];
        }
    }
    return lvk::K_NCLASS;
}
size_t lvk_weight_bytes(struct llama_context * ctx) {
    size_t b = 0;
    for (lvk::Context * c : ctx->stages()) b += c->model.weight_bytes;
    return b;
}
size_t lvk_prompt_image_bytes(struct llama_context * ctx) {
    size_t b = 0;
    for (lvk::Context * c : ctx->stages()) b += c->model.prompt_image_bytes;
    return b;
}
void lvk_set_graph(struct llama_context * ctx, int on) {
    for (lvk::Context * c : ctx->stages()) c->use_graph = on != 0;
}
void lvk_set_prompt_exact(struct llama_context * ctx, int on) {
    for (lvk::Context * c : ctx->stages()) c->prompt_exact = on != 0;
}

int lvk_kv_copy(struct llama_context * dst, struct llama_context * src, int n_tokens) {
    try {
        if (!dst || !src || dst == src) throw lvk::Error("need two distinct contexts");
        if (dst->split || src->split) throw lvk::Error("layer-split contexts copy KV state through llama_get_kv_cache");
        dst->c.kv_copy_from(src->c, n_tokens);
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

// ---- batched decode over KV slots (include/lvk_ops.h)
int lvk_seq_init(struct llama_context * ctx, int n_seq) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        ctx->c.seq_init(n_seq);
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_seq_count(struct llama_context * ctx) { return ctx ? ctx->c.seq_count() : -1; }

int lvk_seq_tokens(struct llama_context * ctx, int seq) {
    if (!ctx || seq < 0 || seq >= ctx->c.seq_count()) return -1;
    return ctx->c.seq_n(seq);
}

int lvk_seq_copy(struct llama_context * ctx, int dst, int src, int n_tokens) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        ctx->c.seq_copy(dst, src, n_tokens);
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_decode_batch(struct llama_context * ctx, const int * tokens, const int * seqs, const int * pos, int n,
                     float * logits, int * argmax) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        lvk::Context & c = ctx->c;
        const int64_t t0 = lvk::now_us();
        c.decode_rows(tokens, seqs, pos, n, logits, argmax);
        c.t_eval_us += lvk::now_us() - t0;   // n decode evals (llama.cpp:1186-1195)
        c.n_eval += n;
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_decode_batch_chain(struct llama_context * ctx, const int * forced, int n_forced, const int * seqs, const int * pos,
                           int n, int n_steps, int * out_tokens, uint64_t * out_digests, float * logits) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        lvk::Context & c = ctx->c;
        const int64_t t0 = lvk::now_us();
        c.decode_rows_chain(forced, n_forced, seqs, pos, n, n_steps, out_tokens, (unsigned long long *) out_digests, logits);
        c.t_eval_us += lvk::now_us() - t0;   // n * n_steps decode evals (llama.cpp:1186-1195)
        c.n_eval += n * n_steps;
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_decode_batch_sample(struct llama_context * ctx, const int * tokens, const int * seqs, const int * pos, int n,
                            const struct lvk_row_sample * rows, int * out_tokens) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        ctx->c.decode_rows_sample(tokens, seqs, pos, n, rows, out_tokens);   // it keeps the timings itself
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_decode_batch_score(struct llama_context * ctx, const int * tokens, const int * seqs, const int * pos, int n,
                           const int * targets, float * probs, int * argmax) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        lvk::Context & c = ctx->c;
        const int64_t t0 = lvk::now_us();
        c.decode_rows_score(tokens, seqs, pos, n, targets, probs, argmax);
        c.t_eval_us += lvk::now_us() - t0;   // n decode evals (llama.cpp:1186-1195)
        c.n_eval += n;
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_eval_score(struct llama_context * ctx, const int * tokens, int n_tokens, int n_past, const int * targets,
                   float * probs, int * argmax) {
    try {
        if (!ctx) throw lvk::Error("null context");
        if (ctx->split) throw lvk::Error("not available on a layer split");
        lvk::Context & c = ctx->c;
        const int64_t t0 = lvk::now_us();
        c.eval_score(tokens, n_tokens, n_past, targets, probs, argmax);
        const int64_t dt = lvk::now_us() - t0;
        if (n_tokens == 1) { c.t_eval_us += dt; c.n_eval++; }          // as llama_eval counts it (llama.cpp:1186-1195)
        else { c.t_p_eval_us += dt; c.n_p_eval += n_tokens; }
        if (!c.has_evaluated_once) {
            c.t_load_us = lvk::now_us() - c.t_start_us;
            c.has_evaluated_once = true;
        }
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

static void score_args(const float * logits, int n, int V, const int * targets, const float * probs) {
    if (!logits || !targets || !probs || n <= 0 || V <= 0 || (size_t) n * (size_t) V > ((size_t) 1 << 28))
        throw lvk::Error("arguments out of range");
    for (int i = 0; i < n; ++i)
        if (targets[i] >= V) throw lvk::Error("target id out of range");
}

int lvk_score_host(const float * logits, int n, int V, const int * targets, float * probs) {
    try {
        score_args(logits, n, V, targets, probs);
        lvk::score_host(logits, n, V, targets, probs);
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_score_rows(const float * logits, int n, int V, const int * targets, float * probs, int * argmax) {
    try {
        score_args(logits, n, V, targets, probs);
        if (V > lvk::SCORE_MAX_VOCAB) throw lvk::Error("the kernel takes V <= 32768 (lvk_score_host takes any)");
        lvk::Scratch dv;
        float * xd = dv.up(logits, (size_t) n * V);
        int * td = dv.up(targets, (size_t) n);
        float * pd = (float *) dv.get((size_t) n * sizeof(float));
        LVK_HIP(lvk::launch_score_rows(xd, V, n, td, pd, nullptr));
        LVK_HIP(hipMemcpy(probs, pd, sizeof(float) * (size_t) n, hipMemcpyDeviceToHost));
        if (argmax) {
            int * ad = (int *) dv.get((size_t) n * sizeof(int));
            LVK_HIP(lvk::launch_argmax_rows(xd, V, n, ad, nullptr));
            LVK_HIP(hipMemcpy(argmax, ad, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost));
        }
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_seq_seed(struct llama_context * ctx, int seq, int seed) {
    if (!ctx || seq < 0 || seq >= ctx->c.seq_count()) return -1;
    if (seed <= 0) seed = (int) time(nullptr);      // as llama_init_from_file resolves it
    ctx->c.seq_gen(seq) = std::mt19937((unsigned) seed);
    return 0;
}

int lvk_sample_fallbacks(struct llama_context * ctx) { return ctx ? ctx->c.n_sample_fallback : -1; }

int lvk_sample_candidates_rows(const float * x, int n_rows, int n, const int * sel, int n_sel, const int * k,
                               const float * temp, const float * rp, const int * last, const int * last_off,
                               float * vals, int * ids, int * counts, int * flags) {
    try {
        if (!x || !sel || !k || !temp || !rp || !last_off || !vals || !ids || !counts || !flags || n_rows <= 0 ||
            n <= 0 || n > lvk::SAMPLE_MAX_VOCAB || n_sel <= 0 || last_off[0] < 0 || (size_t) n_rows * (size_t) n > ((size_t) 1 << 28))
            throw lvk::Error("arguments out of range");
        std::vector<lvk::SampleRow> rec((size_t) n_sel);
        for (int j = 0; j < n_sel; ++j) {
            const int nl = last_off[j + 1] - last_off[j];
            if (sel[j] < 0 || sel[j] >= n_rows || k[j] < 1 || k[j] > std::min(n, lvk::SAMPLE_CAP) || !(temp[j] > 0) ||
                nl < 0 || nl > lvk::SAMPLE_MAX_LAST || (nl > 0 && !last))
                throw lvk::Error("arguments out of range");
            rec[(size_t) j] = {sel[j], k[j], nl, last_off[j], 1.0f / temp[j], rp[j]};
        }
        lvk::Scratch dv;
        float * xd = dv.up(x, (size_t) n_rows * n);
        lvk::SampleRow * rd = dv.up(rec.data(), rec.size());
        const size_t n_pool = (size_t) last_off[n_sel];
        int * pd = n_pool ? dv.up(last, n_pool) : (int *) dv.get(4);
        auto * od = (lvk::SampleOut *) dv.get((size_t) n_sel * sizeof(lvk::SampleOut));
        LVK_HIP(lvk::launch_sample_cand_rows(xd, n, rd, pd, n_sel, od, nullptr));
        std::vector<lvk::SampleOut> o((size_t) n_sel);
        LVK_HIP(hipMemcpy(o.data(), od, o.size() * sizeof(lvk::SampleOut), hipMemcpyDeviceToHost));
        for (int j = 0; j < n_sel; ++j) {
            const size_t m = (size_t) std::min(o[(size_t) j].count, lvk::SAMPLE_CAP);
            std::memcpy(vals + (size_t) j * lvk::SAMPLE_CAP, o[(size_t) j].val, sizeof(float) * m);
            std::memcpy(ids + (size_t) j * lvk::SAMPLE_CAP, o[(size_t) j].id, sizeof(int) * m);
            counts[j] = o[(size_t) j].count;
            flags[j] = o[(size_t) j].flags;
        }
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_rows_step(const float * logits, int n, int V, const int * forced, int n_forced, int step, int * amax,
                  uint64_t * digest, int * next_tok) {
    try {
        // the kernel indexes its outputs by step: (step + 1) * n entries, the last n are this step's
        if (!logits || !amax || !digest || !next_tok || n <= 0 || V <= 0 || step < 0 || n_forced < 0 ||
            (n_forced > 0 && !forced) || (size_t) n * ((size_t) step + 1) > ((size_t) 1 << 24) ||
            (size_t) n * (size_t) n_forced > ((size_t) 1 << 24))
            throw lvk::Error("arguments out of range");
        lvk::Scratch dv;
        const size_t total = (size_t) n * ((size_t) step + 1), off = (size_t) n * (size_t) step;
        float * xd = dv.up(logits, (size_t) n * V);
        std::vector<lvk::SeqRow> rows((size_t) n, lvk::SeqRow{0, step});
        std::vector<int> ctl(2 + (size_t) n, 0);     // {n_forced, digest flag}, then the start positions (0)
        ctl[0] = n_forced;
        ctl[1] = 1;
        lvk::SeqRow * rd = dv.up(rows.data(), rows.size());
        int * cd = dv.up(ctl.data(), ctl.size());
        int * fd = n_forced > 0 ? dv.up(forced, (size_t) n * n_forced) : (int *) dv.get(4);
        int * od = (int *) dv.get(total * sizeof(int));
        auto * dd = (unsigned long long *) dv.get(total * 8);
        int * nd = (int *) dv.get((size_t) n * sizeof(int));
        LVK_HIP(lvk::launch_rows_step(xd, V, n, rd, cd + 2, cd, fd, od, dd, nd, nullptr, 0, 0, nullptr, nullptr));
        LVK_HIP(hipMemcpy(amax, od + off, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost));
        LVK_HIP(hipMemcpy(digest, dd + off, 8 * (size_t) n, hipMemcpyDeviceToHost));
        LVK_HIP(hipMemcpy(next_tok, nd, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost));
        return 0;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_argmax(const float * x, int n) {
    try {
        if (n <= 0) throw lvk::Error("n must be positive");
        lvk::Scratch dv;
        float * xd = dv.up(x, (size_t) n);
        int * od = (int *) dv.get(4);
        int r = -1;
        LVK_HIP(lvk::launch_argmax(xd, n, od, nullptr));
        LVK_HIP(hipMemcpy(&r, od, 4, hipMemcpyDeviceToHost));
        return r;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_sample_candidates(const float * x, int n, const int * last, int n_last, int k, float temp, float rp,
                          float * vals, int * ids, int * flags) {
    try {
        if (n <= 0 || n > lvk::SAMPLE_MAX_VOCAB || k < 1 || k > std::min(n, lvk::SAMPLE_CAP) || temp <= 0 ||
            n_last < 0 || n_last > lvk::SAMPLE_MAX_LAST || (n_last > 0 && !last))
            throw lvk::Error("arguments out of range");
        lvk::Scratch dv;
        float * xd = dv.up(x, (size_t) n);
        lvk::SampleParams p{};
        p.k = k;
        p.n_last = n_last;
        p.scale = 1.0f / temp;
        p.rp = rp;
        if (n_last > 0) std::memcpy(p.last, last, sizeof(int) * (size_t) n_last);
        auto * pd = (lvk::SampleParams *) dv.get(sizeof(p));
        LVK_HIP(hipMemcpy(pd, &p, sizeof(p), hipMemcpyHostToDevice));
        auto * od = (lvk::SampleOut *) dv.get(sizeof(lvk::SampleOut));
        LVK_HIP(lvk::launch_sample_cand(xd, n, pd, od, nullptr));
        lvk::SampleOut o;
        LVK_HIP(hipMemcpy(&o, od, sizeof(o), hipMemcpyDeviceToHost));
        const int m = std::min(o.count, lvk::SAMPLE_CAP);
        std::memcpy(vals, o.val, sizeof(float) * (size_t) m);
        std::memcpy(ids, o.id, sizeof(int) * (size_t) m);
        *flags = o.flags;
        return o.count;
    } catch (const lvk::Error & e) { return fail(__func__, e.msg); }
}

int lvk_eval_greedy(struct llama_context * ctx, int token, int n_past) {
    lvk::Context & c = ctx->c;
    const int64_t t0 = lvk::now_us();
    int r;
    try {
        if (ctx->split) {
            ctx->split->eval(&token, 1, n_past, true);
            c.kv_n = n_past + 1;
            r = c.greedy_h[0];
        } else {
            r = c.eval_greedy(token, n_past);
        }
    } catch (const lvk::Error & e) {
        fprintf(stderr, "%s: failed to eval: %s\n", __func__, e.msg.c_str());
        return -1;
    }
    c.t_eval_us += lvk::now_us() - t0;   // counted as a decode eval (llama.cpp:1186-1195)
    c.n_eval++;
    return r;
}

int lvk_decode_chain(struct llama_context * ctx, const int * tokens, int n_tokens, int n_past, int n_steps,
                     int * out_tokens, uint64_t * out_digests) {
    if (!ctx || !tokens || !out_tokens) {
        fprintf(stderr, "%s: null argument\n", __func__);
        return -1;
    }
    if (ctx->split) {
        fprintf(stderr, "%s: not available on a layer split (use lvk_eval_greedy per step)\n", __func__);
        return -1;
    }
    lvk::Context & c = ctx->c;
    const int64_t t0 = lvk::now_us();
    try {
        c.decode_chain(tokens, n_tokens, n_past, n_steps, out_tokens, (unsigned long long *) out_digests);
    } catch (const lvk::Error & e) {
        fprintf(stderr, "%s: failed to eval: %s\n", __func__, e.msg.c_str());
        return -1;
    }
    c.t_eval_us += lvk::now_us() - t0;   // n_steps decode evals (llama.cpp:1186-1195)
    c.n_eval += n_steps;
    return 0;
}

int lvk_decode_greedy(struct llama_context * ctx, int token, int n_past, int n_steps, int * out_tokens) {
    return lvk_decode_chain(ctx, &token, 1, n_past, n_steps, out_tokens, nullptr);
}

uint64_t lvk_logits_digest(const float * x, int n) {
    uint64_t d = 0;
    for (int k = 0; k < n; ++k) {
        uint32_t bits;
        std::memcpy(&bits, x + k, 4);
        uint64_t z = ((uint64_t) k << 32 | bits) + 0x9E3779B97F4A7C15ull;   // splitmix64 finalizer
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        d += z ^ (z >> 31);
    }
    return d;
}

}  // extern "C"
