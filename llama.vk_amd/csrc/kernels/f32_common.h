// f32_common.h -- device pieces shared by the f32 decode matvec (matvec_f32.hip) and the f32
// batched matmul (mm_f32.hip).
//
// Reference arithmetic (ggml_compute_forward_mul_mat_f32, ggml.c:6134-6297): one
// ggml_vec_dot_f32 (AVX2, ggml.c:1713-1748) per (row, column) on the f32 activation row as it
// is: 4 accumulators x 8 lanes of fp32, accumulator a lane l takes elements 32 st + 8 a + l in
// step order, each step one fused fma(w, x, acc); then GGML_F32x8_REDUCE, the reduce of the f16
// dot: (s0+s1)+(s2+s3) per lane, S[l]+S[l+4], (t0+t1)+(t2+t3).  K % 32 == 0, no scalar tail.
//
// MI355X mapping ("step octet"): a wavefront owns 8 rows; lane 8r + c (c = 2a + h) owns the 4
// chains (accumulator a, AVX lanes 4h .. 4h+3) of row r, as in f16_common.h, whose chain_reduce
// is used unchanged.  16-byte unit (st, c) of a row holds elements 32 st + 4c + {0..3}: the
// file's row order, 8 rows interleaved at 16-byte granularity.
//   weights     : img[ceil(M/8)][K/32][64 lanes] uint4 -- a wave reads 1 KiB contiguous per load
//   activations : the f32 row itself (float4 unit st * 8 + c)
#pragma once
#include "f16_common.h"

namespace lvk {
namespace f32k {

using f16k::chain_reduce;

// one step of the lane's 4 chains: _mm256_fmadd_ps
__device__ __forceinline__ void fma4(float (&acc)[4], const uint4 & w, const float4 & x) {
    acc[0] = __builtin_fmaf(__uint_as_float(w.x), x.x, acc[0]);
    acc[1] = __builtin_fmaf(__uint_as_float(w.y), x.y, acc[1]);
    acc[2] = __builtin_fmaf(__uint_as_float(w.z), x.z, acc[2]);
    acc[3] = __builtin_fmaf(__uint_as_float(w.w), x.w, acc[3]);
}

// One activation row -> dst (K floats, LDS or global), by the NT threads of a workgroup.  NORM:
// rms_norm(x) * g exactly as f16k::act_row_f16 computes it before its conversion; else a copy.
// red: NT / 64 doubles of LDS.  Ends with a workgroup barrier.
template <int NT, bool NORM>
__device__ __forceinline__ void act_row_f32(const float * __restrict__ x, const float * __restrict__ g, int K,
                                            float4 * dst, double * red) {
    const int tid = threadIdx.x;
    const int nunits = K / 8;
    float scale = 1.0f;
    if constexpr (NORM) {
        double acc = 0.0;
        for (int u = tid; u < nunits; u += NT) {
            const float4 a = ((const float4 *) x)[2 * u], b = ((const float4 *) x)[2 * u + 1];
            const float e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int q = 0; q < 8; ++q) { const float sq = e[q] * e[q]; acc += (double) sq; }
        }
        acc = warp_sum_d(acc);
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        double s = 0.0;
        for (int w = 0; w < NT / 64; ++w) s += red[w];
        const float mean = rms_mean_wave(s, x, K);
        scale = 1.0f / sqrtf(mean + 1e-6f);
    }
    for (int u = tid; u < K / 4; u += NT) {
        float4 v = ((const float4 *) x)[u];
        if constexpr (NORM) {
            const float4 gg = ((const float4 *) g)[u];
            // ggml_vec_scale_f32 (ggml.c:6076), then ggml_mul(repeat(g), cur) (llama.cpp:984)
            const float y0 = v.x * scale, y1 = v.y * scale, y2 = v.z * scale, y3 = v.w * scale;
            v = make_float4(gg.x * y0, gg.y * y1, gg.z * y2, gg.w * y3);
        }
        dst[u] = v;
    }
    __syncthreads();
}

}  // namespace f32k
}  // namespace lvk
