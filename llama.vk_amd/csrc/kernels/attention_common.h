// attention_common.h -- the reference-defined arithmetic the attention kernels share
// (attention.hip, attention_decode.hip, attention_prompt.hip; graph_ops.hip for the graph
// evaluator's soft_max and mul_mat): the ggml_vec_dot_f16 reduce (ggml.c:1781-1815), the
// workgroup reductions of a softmax row (ggml.c:7099-7121), and what the launchers agree on.
// Device-only: include it from .hip files.
#pragma once
#include "lvk_device.h"

#include <cmath>
#include <type_traits>

namespace lvk {

constexpr int ATTN_HD = 128;      // head dim every attention kernel is written for

// KQ scale (llama.cpp:1028)
inline float attn_scale(int n_embd, int n_head) { return 1.0f / sqrtf((float) n_embd / (float) n_head); }

// f(std::integral_constant<int, EM>) with EM the compiled-in softmax exp mode (lvk_device.h
// exp_softmax) of the run-time `mode` (AttnLaunch::exp_computed)
template <class F>
inline void with_exp_mode(int mode, F && f) {
    if (mode == 2) f(std::integral_constant<int, 2>{});
    else if (mode == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

// 8 f16 of a 16-byte load -> floats (exact)
__device__ __forceinline__ void unpack8h(const uint4 v, float f[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = f16_to_f32((uint16_t) (w[k] & 0xFFFFu));
        f[2 * k + 1] = f16_to_f32((uint16_t) (w[k] >> 16));
    }
}

// ggml_vec_dot_f16 / _f32 keep 4 AVX registers x 8 lanes of accumulators: element i of a
// 32-wide step feeds (register i / 8, lane i % 8).  GGML_F16_VEC_REDUCE sums the registers per
// lane, S[l] = (s0 + s1) + (s2 + s3), then f32cx8_hsum(S).
// The tail: t_l = S[l] + S[l + 4], then (t0 + t1) + (t2 + t3) (the two hadds).
__device__ __forceinline__ float f32cx8_hsum(const float (&S)[8]) {
    const float t0 = S[0] + S[4], t1 = S[1] + S[5], t2 = S[2] + S[6], t3 = S[3] + S[7];
    return (t0 + t1) + (t2 + t3);
}
// (v0 + v1) + (v2 + v3) of a lane quad's values (lane j = AVX register j) in every lane of the
// quad, by two DPP butterflies: fp addition is commutative, so lane 1's v1 + v0 and lane 2's
// (v2 + v3) + (v0 + v1) are the same bits -- 4 instructions instead of the 7 of four broadcasts
__device__ __forceinline__ float quad_sum(float x) {
    const float y = x + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
    return y + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, y), 0x4E, 0xF, 0xF, false));
}
// the same sum from four quad_perm broadcasts (7 instructions).  The decode kernel keeps this
// form: with the butterflies hipcc schedules k_attn_d differently (71 instead of 74 VGPRs) and
// a launch measured 0.1-0.15 us slower (profiles/attn_pieces_decode_speed.json)
__device__ __forceinline__ float quad_sum_bcast(float v) {
    const float v0 = quad_bcast<0>(v), v1 = quad_bcast<1>(v), v2 = quad_bcast<2>(v), v3 = quad_bcast<3>(v);
    return (v0 + v1) + (v2 + v3);
}
// the whole reduce where the 4 registers of a dot are the 4 lanes of a quad (s: this lane's 8)
__device__ __forceinline__ float quad_reduce(const float (&s)[8]) {
    float S[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) S[l] = quad_sum(s[l]);
    return f32cx8_hsum(S);
}
__device__ __forceinline__ float quad_reduce_bcast(const float (&s)[8]) {
    float S[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) S[l] = quad_sum_bcast(s[l]);
    return f32cx8_hsum(S);
}

// Softmax row reductions of a 256-thread workgroup (4 waves), through 4 LDS slots; bar() is the
// workgroup barrier between the slot writes and reads (__syncthreads, or an LDS-only barrier
// where loads must stay in flight).  Call from uniform control flow.
// max: exact in any order
template <class Bar>
__device__ __forceinline__ float wg_max_f(float v, float * red, Bar && bar) {
    v = wave_max_f(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    bar();
    const float a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}
// sum of the exp values in double: every term is an fp16 value in [0, 1], so it is exact in
// any order (ggml.c:7113-7117 adds them in index order)
template <class Bar>
__device__ __forceinline__ double wg_sum_d(double v, double * redd, Bar && bar) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) redd[threadIdx.x >> 6] = v;
    bar();
    return (redd[0] + redd[1]) + (redd[2] + redd[3]);
}

}  // namespace lvk
