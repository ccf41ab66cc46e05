// mm_mfma.hip -- prompt-eval (N > 1) Q4_0 matmul on the CDNA4 matrix cores,
// bit-faithful to the reference AVX2 arithmetic.
//
// ggml_compute_forward_mul_mat_q_f32 (ggml.c:6510-6696) evaluates every
// (row m, token n) as ggml_vec_dot_q4_0 (ggml.c:1950-2026): 8 fp32 chains
//   acc_j = fmaf(dw_b * da_b, (float) P_bj, acc_j)   over blocks b in order,
//   P_bj  = sum_{e=4j}^{4j+3} (qw_e - 8) * (qa_e - 8)  (exact integer),
// then ((a0+a4)+(a2+a6)) + ((a1+a5)+(a3+a7)).  Those 8.5e11 sequential FMAs
// (7B, 512-token prompt) are the floor of any bit-exact implementation; the
// integer partials are what the matrix cores can take over.
//
// Here v_mfma_f32_32x32x8_f16 produces the partials: in its operand layout
// lane half h holds k = 4h..4h+3, i.e. exactly one chain (2c+h) of a block's
// elements 8c..8c+7.  The B columns are (16 tokens) x (2 chain parities jj);
// lanes with h != jj hold zeros, so output column (n, jj) of the MFMA for
// chain pair c is P_{b,2c+jj}[m, n] for 32 rows m: exact (|products| <= 64,
// sums of 4 in f32).  The VALU then runs exactly the reference's chains:
//   s = dw*da (ggml.c:1968), acc_j = fmaf(s, P_bj, acc_j) (ggml.c:2013),
// and the final AVX2 horizontal order (ggml.c:2019-2024).  Every output is
// bit-identical to ggml_vec_dot_q4_0 (pinned by tests/test_gpu_ops.py).
//
// Operands:
//   A (weights): the decode "octet" image (lvk_kernels.h) read straight into
//     registers: MFMA lane (row, h) loads octet lanes 8r + 2c + h (chains
//     2c+h, c = 0..3) of its row group, 4 x 16 B per 8 blocks; nibbles -> f16
//     with the magic-exponent trick (0x6400|q = 1024+q, 0x4C00|q<<4 = 16+q/4)
//     in the chain order e0 e2 e1 e3.
//   B (activations): Q4_0-quantized tokens as f16 values q-8, written by the
//     activation quantizer straight into the masked fragment image
//       xm[token tile][block][c/2][64 lanes][c%2] x 8 B   (mm_common.h xm_slot)
//     (lane (h, jj, n): chain 2c+h of token n when h == jj, else zero).  The
//     token tile's fragments of one sub-chunk (8 blocks x 2 x 64 lanes x 16 B)
//     are staged once per workgroup in LDS, double-buffered, and every wave
//     reads its fragments from there (one barrier per sub-chunk).
//   Scales: dw (octet image) and da staged per 32-block chunk in LDS (one
//     barrier per chunk); s = dw*da of 32 rows x 16 tokens x 2 blocks comes
//     from one v_mfma_f32_32x32x1f32 outer product (exact f32 products).
// Workgroup = 4 waves, tile 128 rows x 16 tokens (wave w: rows 32w..32w+31,
// all 8 chains: 64 accumulator registers), in the XCD-aware tile order (mm_common.h
// mm_origin).  This file: the kernel, its activation quantizers and its f16 weight image
// builder; the tile, the operand layouts and the epilogue it shares with the Q4_1 kernel
// are in mm_common.h, the interface dispatch in mm_launch.hip.
#include "mm_common.h"

namespace lvk {

namespace {

constexpr int TM = MM_TM, TN = MM_TN, NT = MM_NT;   // the tile (mm_common.h)
constexpr int PDA = 4;      // A16 variant: A blocks in flight per wave

constexpr int DWS = TM + 8;                         // padded row stride of the dw image (conflict-free stores)
constexpr int DAS = TN + 1;                         // padded stride of the da image
constexpr int LDS_DW = 32 * DWS * 4;                // [block of chunk][row]
constexpr int LDS_DA = (32 * DAS * 4 + 15) / 16 * 16;   // [block of chunk][token]
constexpr int OFF_DW0 = 0, OFF_DW1 = LDS_DW;
constexpr int OFF_DA0 = 2 * LDS_DW, OFF_DA1 = OFF_DA0 + LDS_DA;
constexpr int LDS_BSUB = 8 * 128 * 16;               // the B fragments of one sub-chunk: 16 KiB
constexpr int OFF_B0 = OFF_DA1 + LDS_DA, OFF_B1 = OFF_B0 + LDS_BSUB;
constexpr int LDS_TOTAL = OFF_B1 + LDS_BSUB;        // ~69 KiB: two workgroups per CU

struct MmParams {
    const uint4 * nib;
    const float4 * scl;
    const uint2 * a16;       // A16 variant: f16 A-fragment image [M/32][nb][4][64] (QMatrix::a16)
    int M, nb, NC;
    const uint2 * xm;        // masked B fragment image [ntt][nb][4][64]
    const float * da;        // [N][nb]
    MmOut o;                 // tokens N, token tiles ntt, the output y, ...
    uint2 * xq;              // EPI_SWIGLU_Q: the W2 input's fragment image, scales, blocks per token
    float * xqda;
    int nbq;
};

__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t m, uint32_t o) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(m), "v"(o));
    return r;
}

// 16-bit chain field (4 unsigned nibbles e0..e3) selected by sel from X -> f16 e0 e2 e1 e3
__device__ __forceinline__ half4_t unpack_chain(uint32_t X, uint32_t sel) {
    const uint32_t t = __builtin_amdgcn_perm(X, X, sel);            // byte0 | byte1 << 16
    const uint32_t lo = and_or(t, 0x000F000Fu, 0x64006400u);        // (e0, e2) = 1024 + q
    const uint32_t hi = and_or(t, 0x00F000F0u, 0x4C004C00u);        // (e1, e3) = 16 + q/4
    const half2_t c1032 = {(_Float16) -1032.0f, (_Float16) -1032.0f};
    const half2_t c4 = {(_Float16) 4.0f, (_Float16) 4.0f};
    const half2_t c72 = {(_Float16) -72.0f, (_Float16) -72.0f};
    const half2_t h0 = __builtin_bit_cast(half2_t, lo) + c1032;                           // q - 8
    const half2_t h1 = __builtin_elementwise_fma(__builtin_bit_cast(half2_t, hi), c4, c72); // q - 8
    half4_t r;
    r[0] = h0[0]; r[1] = h0[1]; r[2] = h1[0]; r[3] = h1[1];
    return r;
}

// EPI_SWIGLU_Q, the end of the W1|W3 matmul: SwiGLU as EPI_SWIGLU_F32, then quantize_row_q4_0
// of the W2 input (ggml.c:621-685) straight into its fragment image.  The wave's 16 outputs
// (features m0/2 + 16w ..) are half of Q4_0 block b -- groups 2 (w & 1) and 2 (w & 1) + 1 --
// the other half in wave w ^ 1, the amax exchanged through LDS (free after the main loop's
// last barrier)
__device__ __forceinline__ void swiglu_q_store(const MmParams & P, const f32x16_t (&acc)[4], int lane, int w, int m0,
                                               int n0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_e[];
    const int n = n0 + (lane & 15);
    const bool first = (lane >> 4) == 0;              // h = jj = 0: the w1 rows' results
    float res[16];
    mm_hsum(acc, res);
    float uu[16];
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        uu[i] = mv::silu_mul(res[i], __shfl_xor(res[i], 32), P.o.silu_tab);
        const float a = fabsf(uu[i]);
        am = a > am ? a : am;
    }
    __syncthreads();
    float * red = (float *) smem_e;
    if (first) red[w * 16 + (lane & 15)] = am;
    __syncthreads();
    if (first && n < P.o.N) {
        const float ao = red[(w ^ 1) * 16 + (lane & 15)];
        const float amax = (w & 1) ? (am > ao ? am : ao) : (ao > am ? ao : am);
        float d;
        const float id = mv::q40_scale(amax, d);
        const int b = ((m0 >> 1) + 16 * w) >> 5;
#pragma unroll
        for (int g = 0; g < 2; ++g)
            act40_emit(n, P.nbq, b, 2 * (w & 1) + g, mv::q40_pack8(uu + 8 * g, id), d, P.xq, P.xqda);
    }
}

// A16: the A fragments come ready-made from the f16 image (one global_load_dwordx2 per
// MFMA, ring of PD blocks like B) instead of the nibble octet image + unpack (5 VALU per
// MFMA, a third of the loop's VALU work)
template <int EPI, bool A16>
__global__ __launch_bounds__(NT, 2) void k_mm_q40_mfma(MmParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const MmOrigin og = mm_origin(P.o.ntt, P.M / TM);
    const int rt = og.rt, tt = og.tt, m0 = og.m0, n0 = og.n0;
    const int nb = P.nb, NC = P.NC;
    const int G0 = m0 / 8;
    const int U = nb / 8;                      // sub-chunks of 8 blocks

    // ---- scales: chunk c (32 blocks) staged into LDS buffer c & 1 ----
    float rda[2];
    float4 rdw[4];
    auto load_scales = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int Li = i * NT + tid;
            rdw[i] = P.scl[(size_t) (G0 + (Li >> 6)) * NC * 64 + (size_t) c * 64 + (Li & 63)];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int Li = i * NT + tid;
            const int n = Li >> 5, jb = Li & 31;
            const int tok = min(n0 + n, P.o.N - 1);
            rda[i] = P.da[(size_t) tok * nb + min(c * 32 + jb, nb - 1)];
        }
    };
    auto store_scales = [&](int c) {
        float * wl = (float *) (smem + ((c & 1) ? OFF_DW1 : OFF_DW0));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int Li = i * NT + tid;
            const int G = Li >> 6, l = Li & 63;
            const int r = l >> 3, j = l & 7;
            const float v[4] = {rdw[i].x, rdw[i].y, rdw[i].z, rdw[i].w};
#pragma unroll
            for (int m = 0; m < 4; ++m) wl[(8 * m + j) * DWS + 8 * G + r] = v[m];
        }
        float * dl = (float *) (smem + ((c & 1) ? OFF_DA1 : OFF_DA0));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int Li = i * NT + tid;
            dl[(Li & 31) * DAS + (Li >> 5)] = rda[i];
        }
    };

    // ---- A operand: MFMA lane (row rho, half h) <- octet lanes 8r + 2c + h ----
    const int rho = lane & 31, h = lane >> 5;
    const int arow = m0 + 32 * w + rho;
    const uint4 * ap = P.nib + (size_t) (arow >> 3) * NC * 256 + 8 * (arow & 7) + h;
    auto load_a = [&](int u, uint4 (&A)[4]) {              // sub-chunk u = 8 blocks
        const uint4 * p = ap + (size_t) u * 64;            // (c*4 + sb) * 64 == u * 64
#pragma unroll
        for (int c = 0; c < 4; ++c) A[c] = p[2 * c];
    };
    // A16: lane (rho, h) of wave w reads the fragment of rows m0 + 32w + rho, chain 2c + h
    const uint4 * a16p = A16 ? (const uint4 *) P.a16 + (size_t) (rt * TM / 32 + w) * nb * 128 + lane : nullptr;
    uint2 aq[A16 ? PDA : 1][4];
    auto load_aq = [&](int blk, uint2 (&q)[4]) {
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            const uint4 v = a16p[(size_t) blk * 128 + c2 * 64];
            q[2 * c2] = make_uint2(v.x, v.y);
            q[2 * c2 + 1] = make_uint2(v.z, v.w);
        }
    };
    // ---- B operand: masked fragments of this token tile (xm_slot pairs), 4 per block; sub-chunk
    // u of the token tile is 1024 contiguous uint4: thread tid stages 4 of them into LDS ----
    const uint4 * bsp = (const uint4 *) P.xm + (size_t) tt * nb * 128 + tid;
    uint4 bs0, bs1, bs2, bs3;                  // (named: an array of them stays in scratch)
    auto stage_load = [&](int u) {
        const uint4 * g = bsp + (size_t) u * 1024;
        bs0 = g[0]; bs1 = g[NT]; bs2 = g[2 * NT]; bs3 = g[3 * NT];
    };
    auto stage_store = [&](int u) {
        uint4 * bl = (uint4 *) (smem + ((u & 1) ? OFF_B1 : OFF_B0)) + tid;
        bl[0] = bs0; bl[NT] = bs1; bl[2 * NT] = bs2; bl[3 * NT] = bs3;
    };
    auto lds_bq = [&](int u, int jb, uint2 (&q)[4]) {
        const uint4 * bl = (const uint4 *) (smem + ((u & 1) ? OFF_B1 : OFF_B0)) + jb * 128 + lane;
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            const uint4 v = bl[c2 * 64];
            q[2 * c2] = make_uint2(v.x, v.y);
            q[2 * c2 + 1] = make_uint2(v.z, v.w);
        }
    };

    f32x16_t acc[4];
    mm_zero(acc);

    uint32_t X[4][4];                                     // signed octet nibbles -> unsigned q
    auto make_x = [&](const uint4 (&A)[4]) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            X[c][0] = A[c].x ^ 0x88888888u; X[c][1] = A[c].y ^ 0x88888888u;
            X[c][2] = A[c].z ^ 0x88888888u; X[c][3] = A[c].w ^ 0x88888888u;
        }
    };

    uint4 Anext[4];
    load_scales(0);
    if constexpr (A16) {
#pragma unroll
        for (int d = 0; d < PDA; ++d) load_aq(min(d, nb - 1), aq[d]);
    } else {
        load_a(0, Anext);
    }
    stage_load(0);
    stage_store(0);
    store_scales(0);
    if constexpr (!A16) make_x(Anext);
    __syncthreads();

    for (int u = 0; u < U; ++u) {
        const int ch = u >> 2;
        const bool chunk_last = (u & 3) == 3 || u == U - 1;
        const bool scales_next = chunk_last && u + 1 < U;
        if (!A16 && u + 1 < U) load_a(u + 1, Anext);
        if (scales_next) load_scales(ch + 1);
        if (u + 1 < U) stage_load(u + 1);
        const float * wl = (const float *) (smem + ((ch & 1) ? OFF_DW1 : OFF_DW0));
        const float * dl = (const float *) (smem + ((ch & 1) ? OFF_DA1 : OFF_DA0));
        // the block scales s = dw * da (ggml.c:1968) of every (row, token) output come from
        // the matrix core as an outer product, K = 1: each element is one rounded f32
        // multiply, bit-identical to the VALU product.  v_mfma_f32_32x32x1f32 (2 blocks):
        // lane half h feeds block jb + h (dw of row l&31, da of token (l&31)&15); block b
        // lands in registers 16b..16b+15 in the standard 32x32 C/D layout, i.e. exactly the
        // (rows, column) of the chain partials below.
        f32x32_t SC;
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
            const int blk = 8 * u + jb;
            const uint32_t sel = (jb & 1) ? 0x0C030C02u : 0x0C010C00u;
            uint2 bf[4];
            lds_bq(u, jb, bf);
            if ((jb & 1) == 0) {
                const int jc = (u & 3) * 8 + jb + h;        // block of the chunk this lane half feeds
                const float dwa = wl[jc * DWS + 32 * w + rho];
                const float dab = dl[jc * DAS + (lane & 15)];
                SC = __builtin_amdgcn_mfma_f32_32x32x1f32(dwa, dab, (f32x32_t){}, 0, 0, 0);
            }
            float sc[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) sc[i] = SC[16 * (jb & 1) + i];
            // software pipeline: the MFMA of chain pair c+1 is in flight while the VALU runs the
            // chains of pair c (ggml.c:2013: acc_j = fmaf(d, P_j, acc_j))
            f32x16_t Pc[2];
            uint2 (&af)[4] = aq[A16 ? jb % PDA : 0];
            auto afrag = [&](int c) __attribute__((always_inline)) -> half4_t {
                if constexpr (A16) return __builtin_bit_cast(half4_t, af[c]);
                else return unpack_chain(X[c][jb >> 1], sel);
            };
            auto mfma = [&](int c) __attribute__((always_inline)) {
                return __builtin_amdgcn_mfma_f32_32x32x8f16(afrag(c), __builtin_bit_cast(half4_t, bf[c]), (f32x16_t){}, 0, 0, 0);
            };
            Pc[0] = mfma(0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c + 1 < 4) Pc[(c + 1) & 1] = mfma(c + 1);
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[c][i] = __builtin_fmaf(sc[i], Pc[c & 1][i], acc[c][i]);
            }
            // refill this A slot with block blk + PDA (its MFMAs have read the old fragments)
            if constexpr (A16) load_aq(min(blk + PDA, nb - 1), af);
            // block order pinned: unconstrained, hipcc hoists later blocks' MFMAs and spills
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(acc[c]));
        }
        if (!A16 && u + 1 < U) make_x(Anext);
        if (u + 1 < U) stage_store(u + 1);
        if (scales_next) store_scales(ch + 1);
        if (u + 1 < U) __syncthreads();   // chunk ch+1's scales / sub-chunk u+1's B visible; the buffers of
                                          // chunk ch-1 / sub-chunk u-1 free again
    }

    if constexpr (EPI == EPI_SWIGLU_Q) swiglu_q_store(P, acc, lane, w, m0, n0);
    else mm_finish<EPI>(P.o, acc, lane, w, m0, n0);
}

// ---------------------------------------------------------------------------
// Activation quantizer for the MFMA path: x[t] (optionally rms_norm * g, mm_common.h
// act_units) -> quantize_row_q4_0 (AVX2 branch, ggml.c:621-685; mv::q40_quad) -> the
// fragment image + da (act40_emit).  One workgroup per token, one lane quad per block.
// ---------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(256) void k_act_q40_f16(const float * __restrict__ x, const float * __restrict__ g,
                                                     int N, int K, uint2 * __restrict__ xm, float * __restrict__ da) {
    act_units<NORM>(x, g, N, K, [&](int t, int u, bool live, const float (&v)[8]) {
        float d;
        uint32_t qword;
        mv::q40_quad(v, d, qword);
        if (live) act40_emit(t, K / 32, u >> 2, u & 3, qword, d, xm, da);
    });
}

// The quantizer without RMSNorm (the W2 input) by token tiles: a wave takes one 32-block b of
// the tile's 16 tokens (lane quad = token, lane = 8 values), so each of its two stores fills
// whole 256-byte runs of the fragment image (lanes 0-15 | 48-63 of chain pair c/2) instead of
// 16-byte pieces of lines the other 15 tokens' workgroups -- on other XCDs -- also write
// (14 us per 512 x 11008 activation that way).  Same arithmetic per block as k_act_q40_f16.
__global__ __launch_bounds__(256) void k_act_q40_f16_tile(const float * __restrict__ x, int N, int K,
                                                          uint2 * __restrict__ xm, float * __restrict__ da) {
    const int nb = K / 32;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (b >= nb) return;                                     // wave-uniform; no barriers below
    const int tl = lane >> 2, c = lane & 3;
    const int t = blockIdx.x * 16 + tl;
    const bool live = t < N;
    float v[8];
    if (live) {
        const float4 * xp = (const float4 *) (x + (size_t) t * K + b * 32 + c * 8);
        mv::unit_vals(xp[0], xp[1], v);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.0f;
    }
    float d;
    uint32_t qword;
    mv::q40_quad(v, d, qword);
    if (live) act40_emit(t, nb, b, c, qword, d, xm, da);
}

// pre-quantized Q4_0 blocks (ActQ: d + reference nibble qs) -> masked fragment image + da
__global__ void k_actq_to_f16(ActQ q, int N, int K, uint2 * __restrict__ xm, float * __restrict__ da) {
    const int nb = K / 32;
    const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;   // (token, block, group of 8)
    if (idx >= (long) N * nb * 4) return;
    const int c = (int) (idx & 3);
    const long tb = idx >> 2;
    const uint4 qs = q.qs[tb];
    const uint32_t wd[4] = {qs.x, qs.y, qs.z, qs.w};     // word c = elements 8c..8c+7: element 2k = byte k low nibble
    const int t = (int) (tb / nb), b = (int) (tb % nb);
    act40_emit(t, nb, b, c, wd[c], c == 0 ? q.d[tb] : 0.0f, xm, da);
}

// f16 A-fragment image of a Q4_0 octet image (QMatrix::a16, mm_common.h a16_slot): lane
// (rho, h) = row 32 rt + rho, chain 2c + h: its 4 elements as f16 (q - 8) in the fragment
// order e0 e2 e1 e3 (the order the activation image uses).  One thread per 8-byte fragment.
__global__ void k_a16_from_octet(const uint4 * __restrict__ nibi, int M, int K, uint2 * __restrict__ a16) {
    const int nb = K / 32, NC = (nb + 31) / 32;
    const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;     // ((rt * nb + b) * 4 + c) * 64 + lane
    if (idx >= (long) (M / 32) * nb * 256) return;
    const int lane = (int) (idx & 63), c = (int) ((idx >> 6) & 3);
    const long rb = idx >> 8;
    const int b = (int) (rb % nb), rt = (int) (rb / nb);
    // the octet image holds signed nibbles: ^ 8 gives q.  byte0: e0 e1, byte1: e2 e3
    const uint32_t t = octet_chain_field(nibi, rt * 32 + (lane & 31), b, NC, 2 * c + (lane >> 5)) ^ 0x8888u;
    a16[a16_slot(rt, nb, b, c, lane)] = make_uint2(h16m8(nib(t, 0)) | h16m8(nib(t, 2)) << 16,
                                                   h16m8(nib(t, 1)) | h16m8(nib(t, 3)) << 16);
}

}  // namespace

size_t mm_a16_bytes(int M, int K) { return (size_t) (M / 32) * (K / 32) * 256 * 8; }

hipError_t launch_build_a16(const QMatrix & w, void * a16, hipStream_t s) {
    if (w.qtype != Q4_0 || w.M % 32 || w.K % 256) return hipErrorInvalidValue;
    const long n = (long) (w.M / 32) * (w.K / 32) * 256;
    LVK_LAUNCH(k_a16_from_octet, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, w.nib, w.M, w.K, (uint2 *) a16);
    return hipGetLastError();
}

hipError_t mm_q40(const MmLaunch & L, int epi, hipStream_t s) {
    const QMatrix & w = L.w;
    MmParams P{};
    if (epi == EPI_SWIGLU_Q) {
        if (w.M % 64 || !L.silu_tab || !L.out.xm || !L.out.da) return hipErrorInvalidValue;
        P.xq = (uint2 *) L.out.xm; P.xqda = L.out.da; P.nbq = w.M / 64;
    }
    P.nib = w.nib; P.scl = (const float4 *) w.scl; P.a16 = (const uint2 *) w.a16;
    P.M = w.M; P.nb = w.K / 32; P.NC = (P.nb + 31) / 32;
    P.xm = (const uint2 *) L.x.xm; P.da = L.x.da;
    P.o = mm_out(L, epi);
    const dim3 grid((w.M / TM) * P.o.ntt);
    return mm_epi_dispatch<Q4_0>(epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        if (P.a16) LVK_LAUNCH((k_mm_q40_mfma<E, true>), grid, dim3(NT), LDS_TOTAL, s, P);
        else LVK_LAUNCH((k_mm_q40_mfma<E, false>), grid, dim3(NT), LDS_TOTAL, s, P);
        return hipGetLastError();
    });
}

hipError_t act_q40(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s) {
    uint2 * xm = (uint2 *) out.xm;
    if (g)   // one workgroup per token, XCD-grouped token order
        LVK_LAUNCH(k_act_q40_f16<true>, dim3((unsigned) ((N + 127) / 128 * 128)), dim3(256), 0, s, x, g, N, K, xm, out.da);
    else
        LVK_LAUNCH(k_act_q40_f16_tile, dim3((N + 15) / 16, (K / 32 + 3) / 4), dim3(256), 0, s, x, N, K, xm, out.da);
    return hipGetLastError();
}

hipError_t actq_image_q40(const ActQ & q, int N, int K, const ActImage & out, hipStream_t s) {
    const long n = (long) N * (K / 32) * 4;
    LVK_LAUNCH(k_actq_to_f16, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, q, N, K, (uint2 *) out.xm, out.da);
    return hipGetLastError();
}

}  // namespace lvk

// this translation unit's rms_scale_256 counters (k_act_q40_f16<true>), probe build only
LVK_RMS_ACCESSOR(lvk_probe_rms_mm)
