// matvec_common.h -- what the matvec kernels share: the argument block, the activation tables
// in LDS with their prologue pieces (reference Q4_0 / Q4_1 quantizers), the octet reduce and
// the epilogues.
#pragma once
#include "lvk_device.h"
#include "lvk_kernels.h"

namespace lvk {

// the Q4_1 half of matvec_cu_supported / launch_matvec_cu (matvec_cu41.hip)
bool matvec_cu41_supported(int K);
hipError_t launch_matvec_cu41(const MvLaunch & L, int pro, int epi, hipStream_t s);

namespace mv {

// Marks loaded values as produced here for hipcc's wait-count pass.  A load whose result is
// first used after a branch join (e.g. the optional weight issue of a matvec prologue) is
// otherwise waited for with the most conservative count of the two paths -- vmcnt(1) behind
// a weight burst, i.e. the whole burst.  Passing the values through an empty asm statement
// where the exact count is known (right after the burst, in each branch) puts the precise
// wait there and none later.
__device__ __forceinline__ void launder(float4 & v) {
    float a = v.x, b = v.y, c = v.z, d = v.w;
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    v = make_float4(a, b, c, d);
}
__device__ __forceinline__ void launder(uint4 & v) {
    uint32_t a = v.x, b = v.y, c = v.z, d = v.w;
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    v = make_uint4(a, b, c, d);
}
__device__ __forceinline__ void launder(float & v) { asm volatile("" : "+v"(v)); }

// LDS activation table of one token:
//   act[nb/4][8] uint4 : for 4 blocks 4u..4u+3 and chain j:
//       {a(4u,j), a(4u+1,j) << 16, a(4u+2,j), a(4u+3,j) << 16}
//     a(i,j) = signed nibbles of elements 4j..4j+3 of block i (16 bits)
//   dxp[NC][8][4] float : dx of block 32c + 8m + j at [c][j][m]
__device__ __forceinline__ void act_store(uint32_t * act, float * dxp, int i, int q, uint32_t dw_ref, float d,
                                          bool write_d) {
    // dw_ref = elements 8q..8q+7 of block i in the reference nibble convention (q+8)
    const uint32_t s = dw_ref ^ 0x88888888u;
    const uint32_t lo = s & 0xFFFFu, hi = s >> 16;       // chains 2q, 2q+1
    const int slot = i & 3;
    const uint32_t sh = (slot & 1) ? 16u : 0u;
    uint32_t * base = act + (size_t) (i >> 2) * 32;      // 8 chains x 4 dwords
    base[(2 * q) * 4 + slot] = lo << sh;
    base[(2 * q + 1) * 4 + slot] = hi << sh;
    if (write_d) dxp[(size_t) (i >> 5) * 32 + (i & 7) * 4 + ((i >> 3) & 3)] = d;
}

// RNE quantization of 8 values (ggml.c:655-684) -> reference nibble dword
__device__ __forceinline__ uint32_t q40_pack8(const float v[8], float id) {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q = (int) __builtin_rintf(v[k] * id) + 8;
        w |= (uint32_t) (q & 15) << (4 * k);
    }
    return w;
}

// the Q4_0 block scale d of a block's amax; returns the quantization factor id
__device__ __forceinline__ float q40_scale(float amax, float & d) {
    d = amax / 7.0f;                                          // ggml.c:651
    return (amax != 0.0f) ? 7.0f / amax : 0.0f;               // ggml.c:653
}

// quantize_row_q4_0 (AVX2, ggml.c:621-685) of one block held by a lane quad (lane k: elements
// 8k..8k+7): every lane returns d, lane k the reference nibble word of its elements
__device__ __forceinline__ void q40_quad(const float (&v)[8], float & d, uint32_t & qword) {
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float a = fabsf(v[e]);
        amax = a > amax ? a : amax;
    }
    // block amax (ggml.c:636-649)
    const float o0 = quad_bcast<0>(amax), o1 = quad_bcast<1>(amax);
    const float o2 = quad_bcast<2>(amax), o3 = quad_bcast<3>(amax);
    const float m01 = o1 > o0 ? o1 : o0, m23 = o3 > o2 ? o3 : o2;
    amax = m23 > m01 ? m23 : m01;
    qword = q40_pack8(v, q40_scale(amax, d));
}

// quantize_row_q4_0 (AVX2, ggml.c:621-685) of 32 values held one per lane of a 32-lane half
// (element = lane & 31; call with the whole half active): every lane of the half returns the
// block's d and its four nibble words
__device__ __forceinline__ void q40_block32(float v, int lane, float & d, uint4 & qs) {
    float amax = fabsf(v);
    for (int o = 16; o > 0; o >>= 1) { const float w = __shfl_xor(amax, o); amax = w > amax ? w : amax; }
    const float id = q40_scale(amax, d);
    const uint32_t q = (uint32_t) ((int) __builtin_rintf(v * id) + 8) & 15u;
    uint32_t part = q << (4 * (lane & 7));
    part |= __shfl_xor(part, 1);
    part |= __shfl_xor(part, 2);
    part |= __shfl_xor(part, 4);
    // lanes 0, 8, 16, 24 of the half hold the words
    const int h0 = lane & 32;
    qs = make_uint4(__shfl(part, h0), __shfl(part, h0 + 8), __shfl(part, h0 + 16), __shfl(part, h0 + 24));
}

// a finished block `blk` of token t's quantized activation row: one lane stores a Q4_0 block;
// of a Q4_1 block lane k < 4 stores qs word k (q41_block_lds / q41_quad) and lane 0 d and m
__device__ __forceinline__ void actq_store_block(const ActQ & out, int t, int blk, float d, uint4 qs) {
    out.d[(size_t) t * out.nb + blk] = d;
    out.qs[(size_t) t * out.nb + blk] = qs;
}
__device__ __forceinline__ void actq_store_block41(const ActQ & out, int t, int blk, int k, float d, float m,
                                                   uint32_t qword) {
    ((uint32_t *) (out.qs + (size_t) t * out.nb + blk))[k] = qword;
    if (k == 0) {
        out.d[(size_t) t * out.nb + blk] = d;
        out.m[(size_t) t * out.nb + blk] = m;
    }
}

// fixed AVX2 horizontal order of the 8 chains of a row (ggml.c:2019-2024):
// lanes 8r..8r+7 hold a_0..a_7; every lane returns the row's dot product
__device__ __forceinline__ float octet_reduce(float a) {
    const float b = a + __shfl_xor(a, 4);       // r_j = a_j + a_{j+4}
    const float c = b + __shfl_xor(b, 2);       // r0+r2, r1+r3
    return c + __shfl_xor(c, 1);                // (r0+r2) + (r1+r3)
}

// AVX2 emulation helpers (ggml.c:890-915): cvtps_epi32 of an out-of-range value
// gives INT_MIN; packs_epi32 + packs_epi16 saturate to int8; packNibbles packs
// (b0 | b1 << 4) with unsigned saturation (ggml.c:440-452)
__device__ __forceinline__ int32_t cvt_ps_epi32(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return (int32_t) 0x80000000u;
    return (int32_t) v;
}
__device__ __forceinline__ uint32_t sat8u(int32_t v) {
    v = v > 127 ? 127 : (v < -128 ? -128 : v);
    return (uint32_t) (uint8_t) (int8_t) v;
}
__device__ __forceinline__ uint32_t pack_nib(uint32_t b0, uint32_t b1) {
    const uint32_t v = b0 | (b1 << 4);
    return v > 255u ? 255u : v;
}

// the AVX2 max/min tree of quantize_row_q4_1 (ggml.c:857-871) on a block whose
// element e is e8[l] of "lane" k = e/8, l = e%8: max(a,b) = a > b ? a : b, so
// the sign of a zero extremum follows the reference's lane order
struct MinMax { float mx, mn; };
__device__ __forceinline__ MinMax q41_tree(const float (&cm)[8], const float (&cn)[8]) {
    float x4[4], n4[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        x4[l] = cm[4 + l] > cm[l] ? cm[4 + l] : cm[l];
        n4[l] = cn[4 + l] < cn[l] ? cn[4 + l] : cn[l];
    }
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        x4[l] = x4[l] > x4[l + 2] ? x4[l] : x4[l + 2];
        n4[l] = n4[l] < n4[l + 2] ? n4[l] : n4[l + 2];
    }
    return {x4[0] > x4[1] ? x4[0] : x4[1], n4[0] < n4[1] ? n4[0] : n4[1]};
}

// quantize 8 elements of a block given its min and 1/d: 4 qs bytes
__device__ __forceinline__ uint32_t q41_pack8(const float v[8], float vmin, float id) {
    uint32_t qword = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float t0 = v[2 * p] - vmin, t1 = v[2 * p + 1] - vmin;     // sub, then mul (ggml.c:883-886)
        const float w0 = t0 * id, w1 = t1 * id;
        const uint32_t b0 = sat8u(cvt_ps_epi32(__builtin_rintf(w0)));
        const uint32_t b1 = sat8u(cvt_ps_epi32(__builtin_rintf(w1)));
        qword |= pack_nib(b0, b1) << (8 * p);
    }
    return qword;
}


// quantize_row_q4_1 of 32 values staged in LDS (xb[0..31]); lanes k < 4 of the
// calling group return qs word k; every lane returns d and m
__device__ __forceinline__ void q41_block_lds(const float * xb, int k, float & d, float & m, uint32_t & qword) {
    float cm[8], cn[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const float a0 = xb[l], a1 = xb[8 + l], a2 = xb[16 + l], a3 = xb[24 + l];
        float x = a0 > a1 ? a0 : a1;  x = x > a2 ? x : a2;  x = x > a3 ? x : a3;
        float n = a0 < a1 ? a0 : a1;  n = n < a2 ? n : a2;  n = n < a3 ? n : a3;
        cm[l] = x; cn[l] = n;
    }
    const MinMax mm = q41_tree(cm, cn);
    d = (mm.mx - mm.mn) / 15.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    m = mm.mn;
    float v[8];
    const int kk = k & 3;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = xb[8 * kk + e];
    qword = q41_pack8(v, mm.mn, id);
}

// ---- Q4_1 pieces shared by matvec_q41.hip and matvec_cu41.hip

// quantize_row_q4_1 of one block held by a lane quad (lane k: elements 8k..8k+7)
__device__ __forceinline__ void q41_quad(const float v[8], float & d, float & m, uint32_t & qword) {
    float cm[8], cn[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const float a0 = quad_bcast<0>(v[l]), a1 = quad_bcast<1>(v[l]);
        const float a2 = quad_bcast<2>(v[l]), a3 = quad_bcast<3>(v[l]);
        float x = a0 > a1 ? a0 : a1;  x = x > a2 ? x : a2;  x = x > a3 ? x : a3;
        float n = a0 < a1 ? a0 : a1;  n = n < a2 ? n : a2;  n = n < a3 ? n : a3;
        cm[l] = x; cn[l] = n;
    }
    const MinMax mm = q41_tree(cm, cn);
    d = (mm.mx - mm.mn) / 15.0f;                          // ggml.c:874
    const float id = d != 0.0f ? 1.0f / d : 0.0f;         // ggml.c:875
    m = mm.mn;
    qword = q41_pack8(v, mm.mn, id);
}

// Q4_1 activation table of one token:
//   act[nb/4][8] uint4 : {a(4u,j), a(4u+1,j) << 16, a(4u+2,j), a(4u+3,j) << 16}
//   dyv, myv [NC][8][4] : d / m of block 32c + 8m + j at [c][j][m]
//   ysum[nb/4][4 q][4]  : sum of the 8 nibbles 8q..8q+7 of block 4u+t at [u][q][t]
// ysum: float per (block, chain pair) for matvec_q41.hip; one byte each for
// matvec_cu41.hip (the sums are integers <= 120), same index
template <typename YS>
__device__ __forceinline__ void act41_store(uint32_t * act, float * dyv, float * myv, YS * ysum, int i,
                                            const uint32_t qs[4], float d, float m) {
    const int slot = i & 3;
    const uint32_t sh = (slot & 1) ? 16u : 0u;
    uint32_t * base = act + (size_t) (i >> 2) * 32;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t lo = (qs[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        const uint32_t hi = (qs[2 + (j >> 2)] >> (8 * (j & 3))) & 0xFFu;
        base[j * 4 + slot] = (lo | (hi << 8)) << sh;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ysum[(size_t) (i >> 2) * 16 + q * 4 + slot] = (YS) udot8(qs[q], 0x11111111u);
    const int o = (i >> 5) * 32 + (i & 7) * 4 + ((i >> 3) & 3);
    dyv[o] = d;
    myv[o] = m;
}

// even-chain weight sums of two blocks packed in one weight word (low 16 bits
// block A, high 16 bits block B; each 16-bit group = [qs byte j, qs byte 8+j]).
// Quad 0 of a row holds chains 0-3 (first bytes: elements 0-7, second bytes:
// 16-23), quad 1 chains 4-7 (8-15, 24-31); chain 2q needs elements 8q..8q+7:
// j=0 own quad first, j=2 other quad first, j=4 other quad second, j=6 own
// quad second.  Returns {S_A, S_B} in the low/high 16 bits (odd lanes: junk).
__device__ __forceinline__ uint32_t wsum_word(uint32_t w, bool other, uint32_t shift) {
    uint32_t t = (w & 0x0F0F0F0Fu) + ((w >> 4) & 0x0F0F0F0Fu);                  // per byte: its 2 nibbles
    t += (uint32_t) __builtin_amdgcn_mov_dpp((int) t, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
    t += (uint32_t) __builtin_amdgcn_mov_dpp((int) t, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
    const uint32_t mir = (uint32_t) __builtin_amdgcn_mov_dpp((int) t, 0x141, 0xF, 0xF, false);   // row_half_mirror
    return ((other ? mir : t) >> shift) & 0x00FF00FFu;
}

// ---- the arguments every matvec kernel takes.  A kernel's parameter block is this plus what
// only it needs: its weight images and extents (and, for the generic kernels of matvec_q4.hip /
// matvec_q41.hip, the token window and the quantized output).
struct MvArgs {
    const float * x;            // PRO_NORM / PRO_ACTF: f32 input
    const float * g;            // PRO_NORM: norm weight [K]
    ActQ xq;                    // PRO_ACTQ: quantized input
    const StepParams * sp;
    float * y;                  // EPI_STORE / EPI_RESID
    float * u;                  // EPI_SWIGLU_F32: silu(w1 x) * (w3 x) [M/2]
    uint16_t * q16;
    uint16_t * kc;
    uint16_t * vc;
    const float2 * rope;
    int n_embd, head_dim, n_ctx;
    int kv32;                   // f32 KV cache and queries (f16_kv = false)
    const uint16_t * silu_tab;
};

// at_tok0: the single-token kernels take their inputs advanced to token L.tok0 (every input
// pointer that is set); the generic kernels index the token window themselves
inline void mv_fill(MvArgs & A, const MvLaunch & L, bool at_tok0) {
    const size_t t = at_tok0 ? (size_t) L.tok0 : 0;
    A.x = L.x ? L.x + t * L.w.K : nullptr;
    A.g = L.g;
    A.xq = L.xq;
    if (A.xq.qs) A.xq.qs += t * L.xq.nb;
    if (A.xq.d) A.xq.d += t * L.xq.nb;
    if (A.xq.m) A.xq.m += t * L.xq.nb;
    A.sp = L.sp;
    A.y = L.y;
    A.u = L.u;
    A.q16 = L.q16; A.kc = L.kc; A.vc = L.vc; A.rope = L.rope.cs;
    A.n_embd = L.n_embd; A.head_dim = L.head_dim; A.n_ctx = L.n_ctx; A.kv32 = L.kv32;
    A.silu_tab = L.silu_tab;
}

// the input that prologue pro reads must be there
inline bool mv_inputs_set(const MvLaunch & L, int pro) {
    switch (pro) {
        case PRO_NORM: return L.x && L.g;
        case PRO_ACTF: return L.x != nullptr;
        case PRO_ACTQ: return L.xq.qs && L.xq.d && (L.w.qtype != Q4_1 || L.xq.m);
    }
    return false;
}

// ---- f32 -> activation table prologue.  A work unit is 8 consecutive elements; thread t of NT
// holds units k * NT + t (k < UM) in registers; the 4 units of a block are a lane quad
// (nunits % 4 == 0, NT % 4 == 0).

__device__ __forceinline__ void unit_vals(const float4 & a, const float4 & b, float (&v)[8]) {
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// the unit loads (x, and g for PRO_NORM), clamped to the last unit: every thread issues them all
template <int NT, int PRO, int UM, int GM>
__device__ __forceinline__ void pro_load_units(const float * x, const float * g, int nunits, int t,
                                               float4 (&xv)[UM][2], float4 (&gv)[GM][2]) {
#pragma unroll
    for (int k = 0; k < UM; ++k) {
        const int un = min(k * NT + t, nunits - 1);
        const float4 * xp = (const float4 *) (x + (size_t) un * 8);
        xv[k][0] = xp[0]; xv[k][1] = xp[1];
        if constexpr (PRO == PRO_NORM) {
            const float4 * gp = (const float4 *) (g + (size_t) un * 8);
            gv[k][0] = gp[0]; gv[k][1] = gp[1];
        }
    }
}

// ggml_compute_forward_rms_norm_f32's sum (ggml.c:6058-6070): float squares carried in double,
// in element order (RMSNorm order)
__device__ __forceinline__ void sumsq4(double & acc, const float4 & v) {
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float sq = e[q] * e[q]; acc += (double) sq; }
}
template <int NT, int UM>
__device__ __forceinline__ double pro_sumsq_units(const float4 (&xv)[UM][2], int nunits, int t) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < UM; ++k)
        if (k * NT + t < nunits) { sumsq4(acc, xv[k][0]); sumsq4(acc, xv[k][1]); }
    return acc;
}

// PRO_NORM: a unit of rms_norm(x) * g
template <int PRO>
__device__ __forceinline__ void pro_norm_unit(float (&v)[8], const float4 & ga, const float4 & gb, float scale) {
    if constexpr (PRO == PRO_NORM) {
        float gg[8];
        unit_vals(ga, gb, gg);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float yn = v[e] * scale;      // ggml_vec_scale_f32 (ggml.c:6076)
            v[e] = gg[e] * yn;                  // ggml_mul(repeat(g), cur) (llama.cpp:984)
        }
    }
}

// quantize_row_q4_0 of the block a lane quad holds, unit un = this lane's 8 elements, into the
// table (act_store; the quad's first lane also writes d).  q40_quad's arithmetic written out:
// through the call hipcc schedules the decode kernels' prologues differently
// (profiles/mm_pieces_kernel_resources.md), and those kernels are tuned as they stand
__device__ __forceinline__ void q40_unit_store(const float (&v)[8], int un, bool live, uint32_t * act, float * dxp) {
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float a = fabsf(v[e]);
        amax = a > amax ? a : amax;
    }
    // block amax (ggml.c:636-649)
    const float o0 = quad_bcast<0>(amax), o1 = quad_bcast<1>(amax);
    const float o2 = quad_bcast<2>(amax), o3 = quad_bcast<3>(amax);
    const float m01 = o1 > o0 ? o1 : o0, m23 = o3 > o2 ? o3 : o2;
    amax = m23 > m01 ? m23 : m01;
    const float d = amax / 7.0f;                              // ggml.c:651
    const float id = (amax != 0.0f) ? 7.0f / amax : 0.0f;     // ggml.c:653
    const uint32_t w = q40_pack8(v, id);
    if (live) act_store(act, dxp, un >> 2, un & 3, w, d, (un & 3) == 0);
}

// quantize_row_q4_1 of the block a lane quad holds (q41_quad), its 4 qs words gathered into
// every lane; the quad's first lane stores the block (act41_store)
template <typename YS>
__device__ __forceinline__ void q41_unit_store(const float (&v)[8], int un, bool live, uint32_t * act, float * dyv,
                                               float * myv, YS * ysum) {
    float d, m;
    uint32_t qw;
    q41_quad(v, d, m, qw);
    uint32_t qs[4];
    qs[0] = __builtin_bit_cast(uint32_t, quad_bcast<0>(__builtin_bit_cast(float, qw)));
    qs[1] = __builtin_bit_cast(uint32_t, quad_bcast<1>(__builtin_bit_cast(float, qw)));
    qs[2] = __builtin_bit_cast(uint32_t, quad_bcast<2>(__builtin_bit_cast(float, qw)));
    qs[3] = __builtin_bit_cast(uint32_t, quad_bcast<3>(__builtin_bit_cast(float, qw)));
    if (live && (un & 3) == 0) act41_store(act, dyv, myv, ysum, un >> 2, qs, d, m);
}

// the register-held units of thread t: scale * g (PRO_NORM), quantize, store
template <int NT, int PRO, int UM, int GM>
__device__ __forceinline__ void pro_q40_units(const float4 (&xv)[UM][2], const float4 (&gv)[GM][2], float scale,
                                              int nunits, int t, uint32_t * act, float * dxp) {
#pragma unroll
    for (int k = 0; k < UM; ++k) {
        if (k * NT >= nunits) break;
        const int un = k * NT + t;
        constexpr int GK = PRO == PRO_NORM ? 1 : 0;
        float v[8];
        unit_vals(xv[k][0], xv[k][1], v);
        pro_norm_unit<PRO>(v, gv[GK * k][0], gv[GK * k][1], scale);
        q40_unit_store(v, un, un < nunits, act, dxp);
    }
}
template <int NT, int PRO, int UM, int GM, typename YS>
__device__ __forceinline__ void pro_q41_units(const float4 (&xv)[UM][2], const float4 (&gv)[GM][2], float scale,
                                              int nunits, int t, uint32_t * act, float * dyv, float * myv, YS * ysum) {
#pragma unroll
    for (int k = 0; k < UM; ++k) {
        if (k * NT >= nunits) break;
        const int un = k * NT + t;
        constexpr int GK = PRO == PRO_NORM ? 1 : 0;
        float v[8];
        unit_vals(xv[k][0], xv[k][1], v);
        pro_norm_unit<PRO>(v, gv[GK * k][0], gv[GK * k][1], scale);
        q41_unit_store(v, un, un < nunits, act, dyv, myv, ysum);
    }
}

// PRO_ACTQ: a pre-quantized block b into the table
__device__ __forceinline__ void q40_block_store(uint32_t * act, float * dxp, int b, const uint4 & qs, float d) {
    act_store(act, dxp, b, 0, qs.x, d, true);
    act_store(act, dxp, b, 1, qs.y, 0.0f, false);
    act_store(act, dxp, b, 2, qs.z, 0.0f, false);
    act_store(act, dxp, b, 3, qs.w, 0.0f, false);
}
template <typename YS>
__device__ __forceinline__ void q41_block_store(uint32_t * act, float * dyv, float * myv, YS * ysum, int b,
                                                const uint4 & q, float d, float m) {
    const uint32_t qs[4] = {q.x, q.y, q.z, q.w};
    act41_store(act, dyv, myv, ysum, b, qs, d, m);
}

// ---- epilogues

// RoPE mode 0 of one element (ggml_compute_forward_rope_f32, ggml.c:7209-7223): res is element
// i0 of its head, other its partner i0 ^ 1, cs the pair's {cos, sin}
__device__ __forceinline__ float rope_rot(float res, float other, int i0, float2 cs) {
    if ((i0 & 1) == 0) { const float a = res * cs.x, b = other * cs.y; return a - b; }
    const float a = other * cs.y, b = res * cs.x;
    return a + b;
}

// silu(w1 x) * (w3 x): ggml_vec_silu_f32's f16 table (ggml.c:2495), then ggml_mul (llama.cpp:1096)
__device__ __forceinline__ float silu_mul(float a1, float a3, const uint16_t * silu_tab) {
    const float sl = f16_to_f32(silu_tab[f32_to_f16(a1)]);
    return sl * a3;
}

// QKV epilogue of the single-token matvecs, per output row (lane row r of an 8-row group, chain
// lane j; rows e and e^1 are lanes l and l^8) with the lane's RoPE pair loaded
// (cs: rope[pos * hd / 2 + (e % hd) / 2]): RoPE on q and k, then the q row / K-cache row /
// V-cache column stores (llama.cpp:996-1008)
__device__ __forceinline__ void qkv_epilogue_cs(float res, int row, int j, int E, int hd, int pos, float2 cs,
                                                uint16_t * q16, uint16_t * kc, uint16_t * vc, int n_ctx, int kv32) {
    const int which = row / E;              // 0 q, 1 k, 2 v (uniform per wave: E % 8 == 0)
    const int e = row - which * E;
    const float other = __shfl_xor(res, 8);   // row e^1 lives in lanes of row r^1
    float out = res;
    if (which < 2) out = rope_rot(res, other, e % hd, cs);
    if (j == 0) {
        if (which == 0)      kv_store(q16, e, out, kv32);
        else if (which == 1) kv_store(kc, (size_t) pos * E + e, out, kv32);
        else                 kv_store(vc, (size_t) e * n_ctx + pos, out, kv32);
    }
}

// The single-token epilogue of row grp * 8 + r (k_mv_cu, k_mv_cu41, k_matvec_f16).  mv_pre_epi
// loads its memory operand -- the lane's RoPE pair (pos0 = n_past), or the residual term;
// the CU kernels issue it before the row group's chunk loop: loaded in the epilogue it was a
// full memory round trip in every wave's tail (QKV 7.60 -> 7.45, Wo 4.41 -> 4.25, W2 7.33 ->
// 7.26 us; profiles/r06/decode_ab/epilogue_summary.txt)
struct EpiPre { float2 cs; float rv; };
template <int EPI>
__device__ __forceinline__ EpiPre mv_pre_epi(const MvArgs & P, int row, int pos0) {
    EpiPre e{make_float2(0.0f, 0.0f), 0.0f};
    if constexpr (EPI == EPI_QKV) {
        const int i0 = (row - (row / P.n_embd) * P.n_embd) % P.head_dim;   // V rows: an unused pair
        e.cs = P.rope[(size_t) pos0 * (P.head_dim / 2) + (i0 >> 1)];
    } else if constexpr (EPI == EPI_RESID) {
        e.rv = P.y[row];
    }
    return e;
}
// live: the row exists (the last group of an M % 8 != 0 f16 matrix, EPI_STORE only)
template <int EPI>
__device__ __forceinline__ void mv_epilogue(const MvArgs & P, int grp, int r, int j, float res, int pos0,
                                            const EpiPre & pe, bool live = true) {
    const int row = grp * 8 + r;
    if constexpr (EPI == EPI_STORE) {
        if (j == 0 && live) P.y[row] = res;
    } else if constexpr (EPI == EPI_RESID) {
        if (j == 0 && live) P.y[row] = res + pe.rv;     // ggml_add(cur, inpSA) (llama.cpp:1071,1103)
    } else if constexpr (EPI == EPI_QKV) {
        qkv_epilogue_cs(res, row, j, P.n_embd, P.head_dim, pos0, pe.cs, P.q16, P.kc, P.vc, P.n_ctx, P.kv32);
    } else if constexpr (EPI == EPI_SWIGLU_F32) {
        // fused W1|W3 image interleaved per 4 rows: rows 0-3 of the group are
        // w1 rows 4grp..4grp+3, rows 4-7 the w3 rows (llama.cpp:1085-1096)
        const float a3 = __shfl_xor(res, 32);
        if (r < 4 && j == 0) P.u[grp * 4 + r] = silu_mul(res, a3, P.silu_tab);
    }
}

// The STORE / RESID / QKV epilogue of the generic kernels: results res[tt] of row `row` for
// tokens t0 .. t0 + nt - 1 (chain lane j; y is [N][M])
template <int T, int EPI>
__device__ __forceinline__ void mv_epilogue_rows(const MvArgs & P, const float (&res)[T], int row, int j, int M, int t0,
                                                 int nt) {
    if constexpr (EPI == EPI_STORE) {
#pragma unroll
        for (int tt = 0; tt < T; ++tt)
            if (tt < nt && j == 0) P.y[(size_t) (t0 + tt) * M + row] = res[tt];
    } else if constexpr (EPI == EPI_RESID) {
#pragma unroll
        for (int tt = 0; tt < T; ++tt)
            if (tt < nt && j == 0) {
                float * yp = P.y + (size_t) (t0 + tt) * M + row;
                *yp = res[tt] + *yp;                 // the residual add, as mv_epilogue
            }
    } else if constexpr (EPI == EPI_QKV) {
        const int E = P.n_embd, hd = P.head_dim;
        const int which = row / E;          // 0 q, 1 k, 2 v (uniform per wave: E % 8 == 0)
        const int e = row - which * E;
        const int n_past = P.sp->n_past;
#pragma unroll
        for (int tt = 0; tt < T; ++tt) {
            const float other = __shfl_xor(res[tt], 8);   // row e^1 lives in lanes of row r^1
            if (tt < nt && j == 0) {
                const int pos = n_past + t0 + tt;
                if (which < 2) {
                    const int i0 = e % hd;
                    const float out = rope_rot(res[tt], other, i0, P.rope[(size_t) pos * (hd / 2) + (i0 >> 1)]);
                    if (which == 0) kv_store(P.q16, (size_t) (t0 + tt) * E + e, out, P.kv32);
                    else            kv_store(P.kc, (size_t) pos * E + e, out, P.kv32);
                } else {
                    kv_store(P.vc, (size_t) e * P.n_ctx + pos, res[tt], P.kv32);
                }
            }
        }
    }
}

}  // namespace mv

}  // namespace lvk
