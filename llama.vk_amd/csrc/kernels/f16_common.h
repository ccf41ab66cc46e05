// f16_common.h -- device pieces shared by the f16 decode matvec (matvec_f16.hip) and the
// f16 batched matmul (mm_f16.hip).
//
// Reference arithmetic (ggml_compute_forward_mul_mat_f16_f32, ggml.c:6299-6487): every f32
// activation row is converted to f16 (RNE, _cvtss_sh), then one ggml_vec_dot_f16 (AVX2,
// ggml.c:1781-1815) per (row, column): 4 accumulators x 8 lanes of fp32, accumulator a lane
// l takes elements 32 st + 8 a + l in step order, each step one fused fma(f32(w), f32(x),
// acc); then (s0+s1)+(s2+s3) per lane, S[l]+S[l+4], (t0+t1)+(t2+t3).
//
// MI355X mapping ("paired-step octet"): a wavefront owns 8 rows; lane
// 8r + c (c = 2a + h) owns the 4 chains (accumulator a, AVX lanes 4h .. 4h+3) of row r, so
// the 32 sequential chains of a row are spread over 8 lanes with 4 independent FMA chains
// each.  Both operands are stored "paired": 16-byte unit (s, c) of a row holds elements
// 64s + 4c + {0..3} (step 2s) followed by 64s + 32 + 4c + {0..3} (step 2s+1), so one
// 16-byte load feeds two steps of the lane's 4 chains.
//   weights     : img[M/8][K/64][64 lanes] uint4 -- a wave reads 1 KiB contiguous per load
//   activations : x16[K/64][8] uint4 per token (LDS in the matvec, a global buffer in the
//                 matmul); the 8 row lanes of one c read the same unit (broadcast)
#pragma once
#include "lvk_device.h"
#include "lvk_kernels.h"

namespace lvk {
namespace f16k {

// two steps of the lane's 4 chains: v_fma_mix_f32 converts both f16 operands exactly and
// rounds once, i.e. _mm256_fmadd_ps on the F16C-converted values
__device__ __forceinline__ void fma8(float (&acc)[4], const uint4 & w, const uint4 & x) {
    acc[0] = fma_mix_hh<0, 0>(w.x, x.x, acc[0]);
    acc[1] = fma_mix_hh<1, 1>(w.x, x.x, acc[1]);
    acc[2] = fma_mix_hh<0, 0>(w.y, x.y, acc[2]);
    acc[3] = fma_mix_hh<1, 1>(w.y, x.y, acc[3]);
    acc[0] = fma_mix_hh<0, 0>(w.z, x.z, acc[0]);
    acc[1] = fma_mix_hh<1, 1>(w.z, x.z, acc[1]);
    acc[2] = fma_mix_hh<0, 0>(w.w, x.w, acc[2]);
    acc[3] = fma_mix_hh<1, 1>(w.w, x.w, acc[3]);
}

// GGML_F16_VEC_REDUCE (ggml.c:1318-1416) over the 8 lanes of a row: lane c = 2a + h holds
// s_a[4h + i] in acc[i].  Every lane of the row returns the dot product.  The adds pair the
// same operands as the reference (IEEE addition commutes).
__device__ __forceinline__ float chain_reduce(const float (&acc)[4]) {
    float S[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = acc[i] + __shfl_xor(acc[i], 2);     // s0 + s1 | s2 + s3
        const float b = a + __shfl_xor(a, 4);               // (s0 + s1) + (s2 + s3) = S[4h + i]
        S[i] = b + __shfl_xor(b, 1);                        // S[i] + S[i + 4]
    }
    const float t01 = S[0] + S[1], t23 = S[2] + S[3];
    return t01 + t23;
}

// One activation row -> its paired f16 image (dst: K/4 uint2, LDS or global), by the NT
// threads of a workgroup.  NORM: rms_norm(x) * g first (ggml.c:6058-6076, llama.cpp:984; the
// double sum of squares is a tree, rms_mean_wave returns the index-order mean); else the
// plain conversion.  red: NT / 64 doubles of LDS.  Ends with a workgroup barrier.
template <int NT, bool NORM>
__device__ __forceinline__ void act_row_f16(const float * __restrict__ x, const float * __restrict__ g, int K,
                                            uint2 * dst, double * red) {
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
    for (int u = tid; u < nunits; u += NT) {
        const float4 a = ((const float4 *) x)[2 * u], b = ((const float4 *) x)[2 * u + 1];
        float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if constexpr (NORM) {
            const float4 ga = ((const float4 *) g)[2 * u], gb = ((const float4 *) g)[2 * u + 1];
            const float gg[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float yn = v[e] * scale;      // ggml_vec_scale_f32 (ggml.c:6076)
                v[e] = gg[e] * yn;                  // ggml_mul(repeat(g), cur) (llama.cpp:984)
            }
        }
        uint32_t h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (uint32_t) f32_to_f16(v[2 * e]) | (uint32_t) f32_to_f16(v[2 * e + 1]) << 16;
        // elements 8u .. 8u+7: step st = u / 4, accumulator a = u % 4, both halves h
        const int st = u >> 2, a4 = u & 3;
        const int base = (((st >> 1) * 8 + 2 * a4) * 2) + (st & 1);
        dst[base] = make_uint2(h[0], h[1]);
        dst[base + 2] = make_uint2(h[2], h[3]);
    }
    __syncthreads();
}

}  // namespace f16k
}  // namespace lvk
