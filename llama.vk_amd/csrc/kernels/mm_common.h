// mm_common.h -- what the prompt (N > 1) MFMA matmul kernels (mm_mfma.hip Q4_0, mm_mfma41.hip
// Q4_1), their activation quantizers and weight image builders, the interface dispatch
// (mm_launch.hip) and the prompt attention's Wo-input epilogue (attention_prompt.hip) share:
// the tile and its origin, the operand image layouts and their writers, the activation
// quantizer skeleton, the AVX2 horizontal order and the epilogue stores, the epilogue dispatch.
#pragma once
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

#include <type_traits>

namespace lvk {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x32_t __attribute__((ext_vector_type(32)));

// ---- the tile: a workgroup of 4 waves takes 128 rows x 16 tokens (one token tile, MM_TN);
// wave w rows 32w .. 32w+31, all 8 chains: 4 x 16 accumulator registers per lane
constexpr int MM_TM = 128;
constexpr int MM_NT = 256;

// prompt-matmul tile of workgroup slot L (its XCD-contiguous index, mm_origin): row tile
// rt, token tile tt.  Super tiles of R = 4 row tiles x every token tile with the token tiles
// outer, so the 64 workgroups an XCD runs at once share 4 weight tiles and 16 activation
// tiles in its L2 instead of 2 weight tiles and the whole activation image (7B 512-token
// prompt 45.3 -> 43.7 ms, profiles/r04_prompt_variants.jsonl); the row tiles left over after
// the last whole super tile go row tile outer, token tile inner
__device__ __forceinline__ void mm_tile(int L, int ntt, int nrt, int & rt, int & tt) {
    constexpr int R = 4;
    tt = L % ntt;
    rt = L / ntt;
    const int per = R * ntt, sidx = L / per, wi = L % per;
    if (R * sidx + R - 1 < nrt) { tt = wi / R; rt = R * sidx + wi % R; }
}

// The tile of this workgroup in a launch of nrt * ntt workgroups.  XCD-aware order: workgroup
// b runs on XCD b % 8; each XCD gets a contiguous range of slots (the weight tile is fetched
// into that XCD's L2 once for all its token tiles), the slot's tile is mm_tile's
struct MmOrigin {
    int rt, tt;      // row tile, token tile
    int m0, n0;      // first row, first token
};
__device__ __forceinline__ MmOrigin mm_origin(int ntt, int nrt) {
    const int nwg = gridDim.x;
    const int bid = blockIdx.x;
    const int full = nwg & ~7;
    const int L = bid < full ? (bid & 7) * (full >> 3) + (bid >> 3) : bid;
    MmOrigin o;
    mm_tile(L, ntt, nrt, o.rt, o.tt);
    o.m0 = o.rt * MM_TM;
    o.n0 = o.tt * MM_TN;
    return o;
}

__device__ __forceinline__ void mm_zero(f32x16_t & a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.0f;
}
__device__ __forceinline__ void mm_zero(f32x16_t (&acc)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) mm_zero(acc[c]);
}

// ---- operand images

constexpr uint32_t F16_ONE = 0x3C00u;

__device__ __forceinline__ uint32_t nib(uint32_t w, int i) { return (w >> (4 * i)) & 15u; }
// f16 bits of the nibble value q (Q4_1 operands) and of q - 8 (Q4_0 operands)
__device__ __forceinline__ uint32_t h16(uint32_t q) { return __builtin_bit_cast(uint16_t, (_Float16) (float) q); }
__device__ __forceinline__ uint32_t h16m8(uint32_t q) { return __builtin_bit_cast(uint16_t, (_Float16) (float) ((int) q - 8)); }

// Masked B fragment image of the MFMA prompt matmul: token t, block b of nb, chain pair c
// (chains 2c, 2c+1), fragment lane l.  The fragments of chain pairs 2q and 2q+1 sit side by
// side per lane, so a wave fetches two MFMA B operands with one 16-byte-per-lane load (the
// texture unit's cost is per load instruction: 8-byte loads moved half the bytes per cycle).
// Returns the index in 8-byte units.
__device__ __forceinline__ size_t xm_slot(int t, int nb, int b, int c, int l) {
    return ((((size_t) (t >> 4) * nb + b) * 2 + (c >> 1)) * 64 + l) * 2 + (c & 1);
}
// The same for the f16 A fragment image (QMatrix::a16) [M/32][nb][c/2][64 lanes][c%2] x 8 B:
// 32-row tile rt, lane (rho, h) = row 32 rt + rho, chain 2c + h
__device__ __forceinline__ size_t a16_slot(int rt, int nb, int b, int c, int lane) {
    return ((((size_t) rt * nb + b) * 2 + (c >> 1)) * 64 + lane) * 2 + (c & 1);
}
// the 16-bit field (4 nibbles) of chain j of block b of a row in the octet image (k_repack_q40 /
// k_repack_q41 layout, NC chunks of 32 blocks): byte 0 the chain's first two elements, byte 1
// the other two
__device__ __forceinline__ uint32_t octet_chain_field(const uint4 * __restrict__ nibi, int row, int b, int NC, int j) {
    const uint4 v = nibi[(((size_t) (row >> 3) * NC + (b >> 5)) * 4 + ((b & 31) >> 3)) * 64 + 8 * (row & 7) + j];
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    return (wd[(b & 7) >> 1] >> (16 * (b & 1))) & 0xFFFFu;
}

// The Q4_0 operand writes of group c (elements 8c .. 8c+7) of block b of token t, qword the
// group's reference nibbles (nibble e = q_e), stored as f16 q_e - 8: chain 2c -> fragment lane
// n = t % 16 (h = jj = 0), chain 2c+1 -> lane 48 + n (h = jj = 1), each in the order e0 e2 e1
// e3; the lane of group 0 also stores the block scale d (first: with no other store between
// them, hipcc merges the fragment stores of two adjacent groups, EPI_SWIGLU_Q, into 16 bytes)
__device__ __forceinline__ void act40_emit(int t, int nb, int b, int c, uint32_t qword, float d,
                                           uint2 * __restrict__ xm, float * __restrict__ da) {
    if (c == 0) da[(size_t) t * nb + b] = d;
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = h16m8(nib(qword, e));
    xm[xm_slot(t, nb, b, c, t & 15)] = make_uint2(h[0] | h[2] << 16, h[1] | h[3] << 16);
    xm[xm_slot(t, nb, b, c, 48 + (t & 15))] = make_uint2(h[4] | h[6] << 16, h[5] | h[7] << 16);
}

// the Q4_1 operand writes of one quantized block of token t held by a lane quad: quad lane k
// has the block's elements 8k..8k+7 as qword (nibble i = element 8k+i), d and m
// Fragment image xm (chain pairs, as xm_slot) and side image xs [N/16][nb][64] x 16 B:
//   lane (n, jj 0, h 0) {ones, d, m}, (n, 1, 0) {0, d, 0}, (n, 0, 1) {0, m, 0},
//   (n, 1, 1) {the four group sums, m, d}
__device__ __forceinline__ void act41_emit(int t, int nb, int b, int k, uint32_t qword, float d, float m,
                                           uint4 * __restrict__ xm, uint4 * __restrict__ xs) {
    const int lane = threadIdx.x & 63;
    const int base = lane & ~3;
    // chain pair (2k, 2k+1) = elements 4k..4k+3 (quad lane k/2) and 16+4k.. (quad lane 2+k/2)
    const uint32_t lo = (uint32_t) __shfl((int) qword, base | (k >> 1));
    const uint32_t hi = (uint32_t) __shfl((int) qword, base | (2 + (k >> 1)));
    const int o = 4 * (k & 1);
    // fragment order e0 e2 e1 e3 with e = {2j, 2j+1, 16+2j, 17+2j} (as the a16 image)
    const uint2 f0 = make_uint2(h16(nib(lo, o)) | h16(nib(hi, o)) << 16, h16(nib(lo, o + 1)) | h16(nib(hi, o + 1)) << 16);
    const uint2 f1 = make_uint2(h16(nib(lo, o + 2)) | h16(nib(hi, o + 2)) << 16,
                                h16(nib(lo, o + 3)) | h16(nib(hi, o + 3)) << 16);
    uint2 * xm2 = (uint2 *) xm;
    const int n = t & 15;
    xm2[xm_slot(t, nb, b, k, n)] = f0;          // chain 2k   -> lane (n, jj 0, h 0)
    xm2[xm_slot(t, nb, b, k, 48 + n)] = f1;     // chain 2k+1 -> lane (n, jj 1, h 1)
    // the activation sums of groups 0..3 (quad lane q sums group q)
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += nib(qword, i);
    const float sf = (float) s;
    const uint32_t y0 = h16((uint32_t) quad_bcast<0>(sf)), y1 = h16((uint32_t) quad_bcast<1>(sf));
    const uint32_t y2 = h16((uint32_t) quad_bcast<2>(sf)), y3 = h16((uint32_t) quad_bcast<3>(sf));
    const uint32_t db = __builtin_bit_cast(uint32_t, d), mb = __builtin_bit_cast(uint32_t, m);
    uint4 v;
    switch (k) {
        case 0: v = make_uint4(F16_ONE | F16_ONE << 16, F16_ONE | F16_ONE << 16, db, mb); break;  // (jj 0, h 0)
        case 1: v = make_uint4(0u, 0u, db, 0u); break;                                           // (jj 1, h 0)
        case 2: v = make_uint4(0u, 0u, mb, 0u); break;                                           // (jj 0, h 1)
        default: v = make_uint4(y0 | y1 << 16, y2 | y3 << 16, mb, db); break;                    // (jj 1, h 1)
    }
    xs[((size_t) (t >> 4) * nb + b) * 64 + 16 * k + n] = v;
}

// ---- activation quantizer skeleton

// token of workgroup i in a one-workgroup-per-token launch of ceil(N/128)*128 workgroups:
// workgroup i runs on XCD i % 8, and the 16 tokens of token tile tau all go to XCD tau % 8,
// so the 16-byte pieces they write into the same fragment-image lines (xm_slot) meet in one
// L2 instead of being merged from 8 XCDs (>= N: no token)
__device__ __forceinline__ int xcd_grouped_token(int i) {
    const int tau = ((i >> 7) << 3) | (i & 7);
    return tau * 16 + ((i >> 3) & 15);
}

// x[t] (rms_norm * g when NORM) by 8-element units, one 256-thread workgroup per token in
// xcd_grouped_token order: emit(t, u, live, v) gets unit u's values in every thread of a lane
// quad = one 32-block (live: the unit exists; nunits % 4 == 0, so quads are all live or all
// dead, and dead lanes hold zeros).  The RMSNorm double sum is the same per-thread strided /
// wave tree / in-order-waves reduction as the matvec prologue (rms_scale_256), the unit and
// its norm the matvec prologue's (mv::unit_vals, mv::pro_norm_unit).
template <bool NORM, typename Emit>
__device__ __forceinline__ void act_units(const float * __restrict__ x, const float * __restrict__ g, int N, int K,
                                          Emit emit) {
    const int t = xcd_grouped_token(blockIdx.x);
    if (t >= N) return;
    const int tid = threadIdx.x;
    const int nunits = K / 8;
    const float * xr = x + (size_t) t * K;
    float scale = 1.0f;
    if constexpr (NORM) scale = rms_scale_256(xr, K);
    for (int u0 = 0; u0 < nunits; u0 += 256) {
        const int u = u0 + tid;
        const bool live = u < nunits;
        float v[8];
        if (live) {
            const float4 * xp = (const float4 *) (xr + u * 8);
            mv::unit_vals(xp[0], xp[1], v);
            if constexpr (NORM) {
                const float4 * gp = (const float4 *) (g + u * 8);
                mv::pro_norm_unit<PRO_NORM>(v, gp[0], gp[1], scale);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.0f;
        }
        emit(t, u, live, v);
    }
}

// ---- epilogue

// The token extent and what the epilogue stores need, embedded in both kernels' parameter
// blocks.  N and ntt lead, which keeps the argument order the kernels were tuned with (M, nb, N,
// ntt, y, ...): with N behind y the 13B Q4_1 prompt measured 0.9 % slower
// (profiles/mm_pieces_kernel_resources.md)
struct MmOut {
    int N, ntt;                  // tokens, token tiles
    float * y;                   // EPI_STORE / EPI_RESID [N][ldy];  EPI_SWIGLU_F32 u [N][ldy]
    int ldy;
    const uint16_t * silu_tab;
    RopeKV rk;                   // EPI_ROPE_KV only
};
inline MmOut mm_out(const MmLaunch & L, int epi) {
    MmOut o{};
    o.N = L.N; o.ntt = (L.N + MM_TN - 1) / MM_TN; o.y = L.y; o.ldy = L.ldy; o.silu_tab = L.silu_tab;
    if (epi == EPI_ROPE_KV) o.rk = *L.rk;
    return o;
}

// the RoPE + KV epilogue of a prompt-matmul lane: the lane holds rows m0 + 32w + 8q + 4h + p
// (p = 0..3) of token n; rows [0, E) Q, [E, 2E) K, [2E, 3E) V.
// rope_kv_cs loads the 8 cos / sin pairs (before the reduction and any store: issued between
// stores they each wait a full latency), rope_kv_store does RoPE (ggml.c:7209-7232, as
// k_rope_kv) and the f16 stores of the cache views (llama.cpp:1010-1024)
__device__ __forceinline__ void rope_kv_cs(const RopeKV & r, int N, int n, int h, int w, int m0, float2 (&cs)[4][2]) {
    const int pos = r.sp->n_past + (n < N ? n : N - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = (m0 + 32 * w + 8 * q + 4 * h) % r.hd;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) cs[q][pp] = r.rope[(size_t) pos * (r.hd / 2) + (e >> 1) + pp];
    }
}
__device__ __forceinline__ void rope_kv_store(const RopeKV & r, const float (&res)[16], const float2 (&cs)[4][2], int n,
                                              int h, int w, int m0) {
    const int pos = r.sp->n_past + n;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = m0 + 32 * w + 8 * q + 4 * h;
        const int which = row / r.E, e = row - which * r.E;
        if (which < 2) {
            uint32_t hw[2];
#pragma unroll
            for (int pp = 0; pp < 4; pp += 2) {
                const float x0 = res[4 * q + pp], x1 = res[4 * q + pp + 1];
                const float2 c = cs[q][pp >> 1];
                const float a0 = x0 * c.x, b0 = x1 * c.y;
                const float o0 = a0 - b0;
                const float a1 = x0 * c.y, b1 = x1 * c.x;
                const float o1 = a1 + b1;
                hw[pp >> 1] = (uint32_t) f32_to_f16(o0) | (uint32_t) f32_to_f16(o1) << 16;
            }
            uint16_t * dst = which == 0 ? r.q16 + (size_t) n * r.E + e : r.kc + (size_t) pos * r.E + e;
            *(uint2 *) dst = make_uint2(hw[0], hw[1]);
        } else {
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) r.vc[(size_t) (e + pp) * r.n_ctx + pos] = f32_to_f16(res[4 * q + pp]);
        }
    }
}

// The stores of a prompt-matmul lane's 16 results res (rows and lanes as above, the jj = 0
// lanes hold the results): EPI_STORE, EPI_RESID (y += res), EPI_SWIGLU_F32 and EPI_ROPE_KV
// (cs from rope_kv_cs)
template <int EPI>
__device__ __forceinline__ void mm_epi_store(const MmOut & o, const float (&res)[16], const float2 (&cs)[4][2], int n,
                                             int lane, int w, int m0) {
    const int h = lane >> 5;
    const int jj = (lane >> 4) & 1;
    if constexpr (EPI == EPI_SWIGLU_F32) {
        // W1|W3 image interleaved per 4 rows: h = 0 lanes hold the w1 rows, h = 1 the w3 rows of the
        // same outputs (llama.cpp:1085-1096)
        float a3[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a3[i] = __shfl_xor(res[i], 32);
        if (jj == 0 && h == 0 && n < o.N) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float uu[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float sl = f16_to_f32(o.silu_tab[f32_to_f16(res[4 * q + p])]);  // ggml.c:2495
                    uu[p] = sl * a3[4 * q + p];                                           // ggml_mul
                }
                const int row = m0 + 32 * w + 8 * q;
                *(float4 *) (o.y + (size_t) n * o.ldy + row / 2) = make_float4(uu[0], uu[1], uu[2], uu[3]);
            }
        }
    } else if constexpr (EPI == EPI_ROPE_KV) {
        // RoPE + the f16 q / K / V stores (rope_kv_store); a wave's 32 rows lie in one of Q, K, V
        if (jj == 0 && n < o.N) rope_kv_store(o.rk, res, cs, n, h, w, m0);
    } else {
        if (jj == 0 && n < o.N) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 * yp = (float4 *) (o.y + (size_t) n * o.ldy + m0 + 32 * w + 8 * q + 4 * h);
                if constexpr (EPI == EPI_RESID) {
                    const float4 r = *yp;                 // the residual add, as mv_epilogue
                    *yp = make_float4(res[4 * q] + r.x, res[4 * q + 1] + r.y, res[4 * q + 2] + r.z, res[4 * q + 3] + r.w);
                } else {
                    *yp = make_float4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
                }
            }
        }
    }
}

// AVX2 horizontal order (ggml.c:2019-2024, 2250-2256) of a wave's 32 rows x 16 tokens: lane
// (h, n, jj) register set c holds chain 2c+jj; r_j = a_j + a_{j+4} (same lane, sets c and
// c+2), (r0+r2) | (r1+r3) in lanes jj = 0 | 1, then across the lane pair (xor 16): the jj = 0
// lanes hold rows 32w + 8q + 4h + p (i = 4q + p) of token n.  Q4_1: + off * 32 (ggml.c:2257)
__device__ __forceinline__ void mm_hsum(const f32x16_t (&acc)[4], float (&res)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float r0 = acc[0][i] + acc[2][i];       // r_jj     = a_jj + a_{jj+4}
        const float r2 = acc[1][i] + acc[3][i];       // r_{2+jj} = a_{2+jj} + a_{6+jj}
        const float v = r0 + r2;
        res[i] = v + __shfl_xor(v, 16);               // (r0 + r2) + (r1 + r3) in the jj = 0 lanes
    }
}
__device__ __forceinline__ void mm_hsum(const f32x16_t (&acc)[4], const f32x16_t & off, float (&res)[16]) {
    mm_hsum(acc, res);
#pragma unroll
    for (int i = 0; i < 16; ++i) res[i] = res[i] + off[i] * 32.0f;
}

// The end of both kernels: the RoPE pairs (EPI_ROPE_KV), the horizontal sum, the role's stores.
// off: the Q4_1 offset chain (Q4_0 passes none)
template <int EPI, typename... Off>
__device__ __forceinline__ void mm_finish(const MmOut & o, const f32x16_t (&acc)[4], int lane, int w, int m0, int n0,
                                          const Off &... off) {
    const int n = n0 + (lane & 15);
    float2 cs[4][2];                                  // EPI_ROPE_KV: cos / sin
    if constexpr (EPI == EPI_ROPE_KV) rope_kv_cs(o.rk, o.N, n, lane >> 5, w, m0, cs);
    float res[16];
    mm_hsum(acc, off..., res);
    mm_epi_store<EPI>(o, res, cs, n, lane, w, m0);
}

// launch side: the compile-time epilogue of run-time epi, for the epilogues weight type QT's
// kernels implement (mm_epi_supported): go(epi_c<EPI>) launches and returns the launch's error
template <int E>
using epi_c = std::integral_constant<int, E>;
template <int QT, typename Go>
hipError_t mm_epi_dispatch(int epi, Go go) {
    switch (epi) {
        case EPI_STORE: return go(epi_c<EPI_STORE>{});
        case EPI_RESID: return go(epi_c<EPI_RESID>{});
        case EPI_SWIGLU_F32: return go(epi_c<EPI_SWIGLU_F32>{});
        case EPI_ROPE_KV:
            if constexpr (mm_epi_supported(QT, EPI_ROPE_KV)) return go(epi_c<EPI_ROPE_KV>{});
            break;
        case EPI_SWIGLU_Q:
            if constexpr (mm_epi_supported(QT, EPI_SWIGLU_Q)) return go(epi_c<EPI_SWIGLU_Q>{});
            break;
    }
    return hipErrorNotSupported;
}

}  // namespace lvk
