// mm_f16.hip -- batched (2 <= N tokens) W[M][K] . X for f16 weights, bit-identical to
// ggml_compute_forward_mul_mat_f16_f32 (AVX2): the chains of matvec_f16.hip (f16_common.h),
// tiled so that a weight value is loaded once per tile of T tokens.
//
// The activations are converted once per launch sequence (launch_act: optional
// RMSNorm * g, then f32 -> f16 RNE) into a global buffer of paired-step rows; a wave owns one
// 8-row group and T tokens, i.e. 4 T independent fp32 chains per lane.  Per 16-byte weight
// load a lane issues T 16-byte activation loads (the 8 row lanes of a chain slot read the
// same unit, a wave one 128-byte line per token) and 8 T v_fma_mix_f32.  v_fma_mix_f32 on
// the f16 operands was chosen over v_pk_fma_f32 on pre-converted operands: it needs no
// conversion instructions and half the activation bytes, and both are exact here.
#include "f16_common.h"
#include "mm_common.h"

namespace lvk {

namespace {
using namespace f16k;

struct MmParams {
    const uint4 * img;
    int M, K, G;
    const uint4 * x16;          // [Npad][K / 64][8] uint4, Npad a multiple of MM_F16_TPAD
    int N;
    float * y;                  // EPI_STORE / EPI_RESID [N][ldy];  EPI_SWIGLU_F32 u [N][M / 2]
    int ldy;
    const uint16_t * silu_tab;
};

template <int T, int EPI>
__global__ __launch_bounds__(256) void k_mm_f16(MmParams P) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane & 7, r = lane >> 3;
    const int grp = blockIdx.y * 4 + wave;
    if (grp >= P.G) return;                              // wave-uniform; the kernel has no barrier
    const int t0 = blockIdx.x * T;
    const int S = P.K / 64;
    const uint4 * wp = P.img + (size_t) grp * S * 64 + lane;
    // rows t0 .. t0 + T - 1 exist in the padded buffer (rows >= N hold stale finite or
    // non-finite bits; their results are never stored)
    const uint4 * xp = P.x16 + (size_t) t0 * S * 8 + c;
    const size_t xstride = (size_t) S * 8;
    float acc[T][4];
#pragma unroll
    for (int tt = 0; tt < T; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[tt][i] = 0.0f;
    uint4 w = wp[0];
    for (int s = 0; s < S; ++s) {
        const uint4 wn = wp[(size_t) (s + 1 < S ? s + 1 : s) * 64];
#pragma unroll
        for (int tt = 0; tt < T; ++tt) fma8(acc[tt], w, xp[(size_t) tt * xstride + (size_t) s * 8]);
        w = wn;
    }
    const int row = grp * 8 + r;
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
        const float res = chain_reduce(acc[tt]);
        const int t = t0 + tt;
        if constexpr (EPI == EPI_STORE) {
            if (c == 0 && t < P.N && row < P.M) P.y[(size_t) t * P.ldy + row] = res;
        } else if constexpr (EPI == EPI_RESID) {
            if (c == 0 && t < P.N && row < P.M) {
                float * yp = P.y + (size_t) t * P.ldy + row;
                *yp = res + *yp;                          // ggml_add(cur, inpSA) (llama.cpp:1071,1103)
            }
        } else if constexpr (EPI == EPI_SWIGLU_F32) {
            // rows 0-3 of the group: w1 rows 4grp .. 4grp+3, rows 4-7 the w3 rows
            const float a3 = __shfl_xor(res, 32);
            if (r < 4 && c == 0 && t < P.N) {
                const float sl = f16_to_f32(P.silu_tab[f32_to_f16(res)]);   // ggml_vec_silu_f32 (ggml.c:2495)
                P.y[(size_t) t * P.ldy + grp * 4 + r] = sl * a3;             // ggml_mul (llama.cpp:1096)
            }
        }
    }
}

template <bool NORM>
__global__ __launch_bounds__(256) void k_act_f16p(const float * __restrict__ x, const float * __restrict__ g, int K,
                                                  uint2 * __restrict__ x16) {
    __shared__ double red[4];
    const size_t t = blockIdx.x;
    act_row_f16<256, NORM>(x + t * K, g, K, x16 + t * (K / 4), red);
}

template <int T, int EPI>
hipError_t go(const MmParams & P, hipStream_t s) {
    const dim3 grid((P.N + T - 1) / T, (P.G + 3) / 4);
    if (grid.y > 65535) return hipErrorInvalidValue;
    LVK_LAUNCH((k_mm_f16<T, EPI>), grid, dim3(256), 0, s, P);
    return hipGetLastError();
}

template <int EPI>
hipError_t go_t(const MmParams & P, hipStream_t s) {
    // token tile: 4 for the smallest batches, 16 up to 32 tokens, 32 beyond
    if (P.N <= 4) return go<4, EPI>(P, s);
    if (P.N <= 32) return go<16, EPI>(P, s);
    return go<32, EPI>(P, s);
}

}  // namespace

hipError_t act_f16(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s) {
    if (g) LVK_LAUNCH((k_act_f16p<true>), dim3(N), dim3(256), 0, s, x, g, K, (uint2 *) out.xm);
    else LVK_LAUNCH((k_act_f16p<false>), dim3(N), dim3(256), 0, s, x, g, K, (uint2 *) out.xm);
    return hipGetLastError();
}

hipError_t mm_f16(const MmLaunch & L, int epi, hipStream_t s) {
    const QMatrix & w = L.w;
    if (epi != EPI_STORE && w.M % 8) return hipErrorInvalidValue;
    MmParams P{};
    P.img = w.nib; P.M = w.M; P.K = w.K; P.G = (w.M + 7) / 8;
    P.x16 = (const uint4 *) L.x.xm; P.N = L.N; P.y = L.y; P.ldy = L.ldy; P.silu_tab = L.silu_tab;
    return mm_epi_dispatch<F16>(epi, [&](auto e) { return go_t<decltype(e)::value>(P, s); });
}

}  // namespace lvk
