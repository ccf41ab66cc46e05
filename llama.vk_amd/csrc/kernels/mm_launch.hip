// mm_launch.hip -- the batched (N > 1) matmul interface of lvk_kernels.h: the weight-type
// dispatch of launch_act / launch_actq_to_image / launch_mm with the checks every type shares
// (the kernels are in mm_mfma.hip Q4_0, mm_mfma41.hip Q4_1, mm_f16.hip F16, mm_f32.hip F32), and the unfused
// RoPE + KV append of stored Q|K|V rows.
#include "mm_common.h"

namespace lvk {

static bool image_complete(int qtype, const ActImage & im) {
    return im.xm && (qtype != Q4_0 || im.da) && (qtype != Q4_1 || im.xs);
}

bool mm_supported(const QMatrix & w) {
    switch (w.qtype) {
        case Q4_0: return w.M % MM_TM == 0 && w.K % 256 == 0;
        case Q4_1: return w.a16 && w.side && w.M % MM_TM == 0 && w.K % 256 == 0;
        case F16: case F32: return w.M >= 1 && w.K % 256 == 0;
    }
    return false;
}

hipError_t launch_act(int qtype, const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s) {
    if (K % 256 || N <= 0 || !x || !image_complete(qtype, out)) return hipErrorInvalidValue;
    switch (qtype) {
        case Q4_0: return act_q40(x, g, N, K, out, s);
        case Q4_1: return act_q41(x, g, N, K, out, s);
        case F16: return act_f16(x, g, N, K, out, s);
        case F32: return act_f32(x, g, N, K, out, s);
    }
    return hipErrorNotSupported;
}

hipError_t launch_actq_to_image(int qtype, const ActQ & q, int N, int K, const ActImage & out, hipStream_t s) {
    if (qtype != Q4_0 && qtype != Q4_1) return hipErrorNotSupported;
    if (K % 32 || N <= 0 || !image_complete(qtype, out)) return hipErrorInvalidValue;
    return qtype == Q4_0 ? actq_image_q40(q, N, K, out, s) : actq_image_q41(q, N, K, out, s);
}

hipError_t launch_mm(const MmLaunch & L, int epi, hipStream_t s) {
    const QMatrix & w = L.w;
    if (!mm_epi_supported(w.qtype, epi)) return hipErrorNotSupported;
    if (!mm_supported(w) || L.N <= 0 || !image_complete(w.qtype, L.x) || (epi == EPI_ROPE_KV) != (L.rk != nullptr))
        return hipErrorInvalidValue;
    // EPI_ROPE_KV: the rows are Q|K|V, a wave's 32 rows lie in one of them, a lane's 4 in one head
    if (L.rk && (w.M != 3 * L.rk->E || L.rk->E % 32 || L.rk->hd % 4 || !L.rk->sp)) return hipErrorInvalidValue;
    switch (w.qtype) {
        case Q4_0: return mm_q40(L, epi, s);
        case Q4_1: return mm_q41(L, epi, s);
        case F16: return mm_f16(L, epi, s);
        default: return mm_f32(L, epi, s);
    }
}

namespace {

// RoPE mode 0 (ggml.c:7156-7227) + KV append (llama.cpp:996-1008) of the
// stored Q|K|V rows [N][3E] -> q16 [N][E], K cache [pos][E], V cache [E][pos]
__global__ void k_rope_kv(const float * __restrict__ qkv, int N, int E, int hd, const float2 * __restrict__ rope,
                          const StepParams * __restrict__ sp, int n_ctx, uint16_t * __restrict__ q16,
                          uint16_t * __restrict__ kc, uint16_t * __restrict__ vc, int kv32) {
    const int t = blockIdx.y;
    const int e2 = blockIdx.x * blockDim.x + threadIdx.x;     // pair index over Q|K (E/2 each) then V
    const int pos = sp->n_past + t;
    const float * row = qkv + (size_t) t * 3 * E;
    if (e2 < E) {                // Q and K pairs: e2 in [0, E): which = e2 / (E/2)
        const int which = e2 / (E / 2);
        const int e = 2 * (e2 - which * (E / 2));
        const float x0 = row[which * E + e], x1 = row[which * E + e + 1];
        const int i0 = e % hd;
        const float2 cs = rope[(size_t) pos * (hd / 2) + (i0 >> 1)];
        const float a0 = x0 * cs.x, b0 = x1 * cs.y;
        const float o0 = a0 - b0;
        const float a1 = x0 * cs.y, b1 = x1 * cs.x;
        const float o1 = a1 + b1;
        if (which == 0) {
            kv_store(q16, (size_t) t * E + e, o0, kv32);
            kv_store(q16, (size_t) t * E + e + 1, o1, kv32);
        } else {
            kv_store(kc, (size_t) pos * E + e, o0, kv32);
            kv_store(kc, (size_t) pos * E + e + 1, o1, kv32);
        }
    } else if (e2 < E + E / 2) {
        const int e = 2 * (e2 - E);
        kv_store(vc, (size_t) e * n_ctx + pos, row[2 * E + e], kv32);
        kv_store(vc, (size_t) (e + 1) * n_ctx + pos, row[2 * E + e + 1], kv32);
    }
}

}  // namespace

hipError_t launch_rope_kv(const float * qkv, int N, int E, int hd, const float2 * rope, const StepParams * sp,
                          int n_ctx, uint16_t * q16, uint16_t * kc, uint16_t * vc, hipStream_t s, int kv32) {
    const int pairs = E + E / 2;
    LVK_LAUNCH(k_rope_kv, dim3((pairs + 255) / 256, N), dim3(256), 0, s, qkv, N, E, hd, rope, sp, n_ctx, q16, kc, vc,
               kv32);
    return hipGetLastError();
}

}  // namespace lvk
