// mm_mfma41.hip -- prompt-eval (N > 1) Q4_1 matmul on the CDNA4 matrix cores,
// bit-faithful to the reference AVX2 arithmetic (the 13B Q4_1 prompt path).
//
// ggml_vec_dot_q4_1 (ggml.c:2188-2258) evaluates every (row m, token n) as 8 fp32
// chains j = 0..7 over the blocks b in order, plus one offset chain:
//   P_bj   = sum of qx_e * qy_e over e in {2j, 2j+1, 16+2j, 17+2j}   (unsigned nibbles)
//   acc_j  = fmaf(dx*dy, P_bj, acc_j)                                 (ggml.c:2244)
//   acc_j  = fmaf(j even ? dx*my : mx*dy, S_bj, acc_j)                (ggml.c:2236-2247)
//            S_bj = j even ? sum(qx_{8q..8q+7}) : sum(qy_{8q..8q+7}),  q = j/2
//   off    = off + mx*my                                              (ggml.c:2226)
// result = hsum8(acc) + off * 32 (ggml.c:2250-2257).  Every integer above is exact in
// f16 operands and f32 MFMA sums, so the matrix cores produce them and the VALU runs
// exactly the reference's chains:
//   * P (4 x v_mfma_f32_32x32x8_f16 per block): as mm_mfma.hip's Q4_0 kernel -- A the
//     weight chain fragments (f16 image, QMatrix::a16), B the masked activation
//     fragments (lane (n, jj, h) holds chain 2c+h of token n when h == jj), output
//     column (n, jj) = chain 2c+jj.
//   * S (4 more v_mfma_f32_32x32x8_f16 per block): the cross term's integer operand in
//     the same output layout -- A lane (row, h): h = 0 the row's 4 weight sums of the
//     block, h = 1 ones; B lane (n, jj, h): (0, 0) the unit vector e_c, (1, 1) the
//     token's activation sum of group c at slot c, else zero.  Output column (n, 0) =
//     S of the even chain 2c (weight sum), (n, 1) = S of the odd chain 2c+1.
//   * the scale products: v_mfma_f32_32x32x1f32 (2 blocks) of A = (d | m of the row by
//     lane half) and B = (d | m of the token) gives dx*dy and mx*my; v_mfma_f32_32x32x2f32
//     of the same A and B = (h == jj ? (m | d) : 0) gives dx*my in the even and mx*dy in
//     the odd columns (one product plus an exact zero: the rounded VALU product, and the
//     chains can never hold -0, so a +-0 product term never changes a sum).
// Operand images (all built so a lane's operand is one 16-byte load):
//   weights a16  [M/32][nb][2][64] x 16 B  chain fragments (as the Q4_0 image, values q)
//           side [M/32][nb][64] x 16 B     {S operand (4 x f16), d | m (f32), 0}
//   tokens  xm   [N/16][nb][2][64] x 16 B  masked chain fragments (mm_common.h xm_slot)
//           xs   [N/16][nb][64] x 16 B     {S operand, d | m, (m | d) masked}
// No LDS and no barrier: every operand streams straight into registers, 3 blocks deep
// (13B 512-token prompt: 1 block 188.7 ms, 2: 172.4, 3: 170.0, 4: 235.8 -- spills).
// Workgroup = 4 waves, tile 128 rows x 16 tokens, XCD-aware tile order (mm_common.h mm_origin).
// Two kernels stream the operands differently (a register ring, an LDS-DMA ring) and share
// the block arithmetic (block41) and, with the Q4_0 kernel, the tile and the epilogue.
#include "mm_common.h"

namespace lvk {

namespace {

constexpr int TM = MM_TM, NT = MM_NT;   // the tile (mm_common.h)
constexpr int PD = 3;       // blocks of every operand in flight per wave

struct Mm41Params {
    const uint4 * a16;       // [M/32][nb][2][64]
    const uint4 * side;      // [M/32][nb][64]
    const uint4 * xm;        // [ntt][nb][2][64]
    const uint4 * xs;        // [ntt][nb][64]
    int M, nb;
    MmOut o;                 // tokens N, token tiles ntt, the output y, ...
};

struct Blk {                 // one block's operands of one lane
    uint4 a[2], b[2], sa, sb;
};

// One block of a lane's chains (both kernels): the scale products, the chain partials P and
// cross-term operands S from the matrix cores, then the reference's fmaf chains and offset
__device__ __forceinline__ void block41(const Blk & o, f32x16_t (&acc)[4], f32x16_t & off) {
    const float sw = __builtin_bit_cast(float, o.sa.z);      // d | m of the row
    const float sb1 = __builtin_bit_cast(float, o.sb.z);     // d | m of the token
    const float sb2 = __builtin_bit_cast(float, o.sb.w);     // (m | d) where h == jj, else 0
    // dx*dy (registers 0..15) and mx*my (16..31); dx*my | mx*dy by column parity
    const f32x32_t SM = __builtin_amdgcn_mfma_f32_32x32x1f32(sw, sb1, (f32x32_t){}, 0, 0, 0);
    const f32x16_t SX = __builtin_amdgcn_mfma_f32_32x32x2f32(sw, sb2, (f32x16_t){}, 0, 0, 0);
    const half4_t ax = __builtin_bit_cast(half4_t, make_uint2(o.sa.x, o.sa.y));
    const uint32_t bfr[8] = {o.b[0].x, o.b[0].y, o.b[0].z, o.b[0].w, o.b[1].x, o.b[1].y, o.b[1].z, o.b[1].w};
    const uint32_t afr[8] = {o.a[0].x, o.a[0].y, o.a[0].z, o.a[0].w, o.a[1].x, o.a[1].y, o.a[1].z, o.a[1].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const half4_t a = __builtin_bit_cast(half4_t, make_uint2(afr[2 * c], afr[2 * c + 1]));
        const half4_t b = __builtin_bit_cast(half4_t, make_uint2(bfr[2 * c], bfr[2 * c + 1]));
        // the S operand's B fragment: slot c of the token's sums (or of e_c)
        const uint32_t yw = (c < 2) ? o.sb.x : o.sb.y;
        const uint32_t ym = yw & ((c & 1) ? 0xFFFF0000u : 0x0000FFFFu);
        const half4_t bs = __builtin_bit_cast(half4_t, (c < 2) ? make_uint2(ym, 0u) : make_uint2(0u, ym));
        const f32x16_t Pc = __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, (f32x16_t){}, 0, 0, 0);
        const f32x16_t Sc = __builtin_amdgcn_mfma_f32_32x32x8f16(ax, bs, (f32x16_t){}, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            acc[c][i] = __builtin_fmaf(SM[i], Pc[i], acc[c][i]);      // ggml.c:2244
            acc[c][i] = __builtin_fmaf(SX[i], Sc[i], acc[c][i]);      // ggml.c:2247
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) off[i] = off[i] + SM[16 + i];      // ggml.c:2226
}

template <int EPI>
__global__ __launch_bounds__(NT, 2) void k_mm_q41_mfma(Mm41Params P) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const MmOrigin og = mm_origin(P.o.ntt, P.M / TM);
    const int tt = og.tt, m0 = og.m0, n0 = og.n0;
    const int nb = P.nb;
    const int rt = m0 / 32 + w;                              // this wave's 32-row tile

    const uint4 * ap = P.a16 + (size_t) rt * nb * 128 + lane;
    const uint4 * sap = P.side + (size_t) rt * nb * 64 + lane;
    const uint4 * bp = P.xm + (size_t) tt * nb * 128 + lane;
    const uint4 * sbp = P.xs + (size_t) tt * nb * 64 + lane;
    auto load = [&](int blk, Blk & o) {
        o.a[0] = ap[(size_t) blk * 128];
        o.a[1] = ap[(size_t) blk * 128 + 64];
        o.b[0] = bp[(size_t) blk * 128];
        o.b[1] = bp[(size_t) blk * 128 + 64];
        o.sa = sap[(size_t) blk * 64];
        o.sb = sbp[(size_t) blk * 64];
    };

    f32x16_t acc[4], off;
    mm_zero(acc);
    mm_zero(off);

    Blk ring[PD];
#pragma unroll
    for (int d = 0; d < PD; ++d) load(min(d, nb - 1), ring[d]);

    for (int b0 = 0; b0 < nb; b0 += PD) {
#pragma unroll
        for (int d = 0; d < PD; ++d) {
            const int blk = b0 + d;
            if (blk >= nb) break;
            Blk & o = ring[d];
            block41(o, acc, off);
            // refill this slot PD blocks ahead (its MFMAs have consumed it)
            load(min(blk + PD, nb - 1), o);
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(acc[c]));
        }
    }

    mm_finish<EPI>(P.o, acc, lane, w, m0, n0, off);
}

// ---------------------------------------------------------------------------
// The same matmul with the operands streamed through a per-wave LDS ring by LDS-DMA
// (global_load_lds_dwordx4).  hipcc's waitcnt pass
// puts a vmcnt(0) at the register-ring loop's header (the refill issued last in a trip
// is waited for at once); the DMAs are invisible to it, so the wave keeps RS blocks in
// flight and waits with its own count.  Per wave RS slots of 6 x 1 KiB (a16 pair halves,
// side, xm pair halves, xs: one 16-byte lane row each, read back with one ds_read_b128
// per lane and operand); 72 KiB per workgroup, two workgroups per CU.
// ---------------------------------------------------------------------------
constexpr int RS = 3;                       // ring slots (blocks in flight) per wave
constexpr int OCC41 = 2;                    // workgroups per CU (LDS: OCC41 * LDS41 <= 160 KiB)
constexpr int SLOT = 6 * 1024;
constexpr int LDS41 = 4 * RS * SLOT;

__device__ __forceinline__ unsigned lds_addr41(const void * p) {
    return (unsigned) (uintptr_t) (const __attribute__((address_space(3))) uint8_t *) p;
}
// one 1 KiB LDS-DMA: lane l's 16 bytes at gsrc land at LDS byte lds_dst + 16 l
__device__ __forceinline__ void dma1k(const void * gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

template <int EPI>
__global__ __launch_bounds__(NT, OCC41) void k_mm_q41_dma(Mm41Params P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const MmOrigin og = mm_origin(P.o.ntt, P.M / TM);
    const int tt = og.tt, m0 = og.m0, n0 = og.n0;
    const int nb = P.nb;
    const int rt = m0 / 32 + w;

    const uint4 * ap = P.a16 + (size_t) rt * nb * 128 + lane;
    const uint4 * sap = P.side + (size_t) rt * nb * 64 + lane;
    const uint4 * bp = P.xm + (size_t) tt * nb * 128 + lane;
    const uint4 * sbp = P.xs + (size_t) tt * nb * 64 + lane;
    uint8_t * ring = smem + w * RS * SLOT;
    const unsigned ring_l = __builtin_amdgcn_readfirstlane(lds_addr41(ring));
    auto issue = [&](int blk, int slot) {
        const unsigned d = ring_l + slot * SLOT;
        dma1k(ap + (size_t) blk * 128, d);
        dma1k(ap + (size_t) blk * 128 + 64, d + 1024);
        dma1k(sap + (size_t) blk * 64, d + 2048);
        dma1k(bp + (size_t) blk * 128, d + 3072);
        dma1k(bp + (size_t) blk * 128 + 64, d + 4096);
        dma1k(sbp + (size_t) blk * 64, d + 5120);
    };

    f32x16_t acc[4], off;
    mm_zero(acc);
    mm_zero(off);

#pragma unroll
    for (int sl = 0; sl < RS; ++sl) issue(min(sl, nb - 1), sl);

    int slot = 0;
    for (int blk = 0; blk < nb; ++blk) {
        // this block's 6 DMAs landed: at most the later RS - 1 blocks' are still in flight
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 * (RS - 1)) : "memory");
        const uint4 * sp = (const uint4 *) (ring + slot * SLOT) + lane;   // ds_read (LDS pointer inferred)
        Blk o;
        o.a[0] = sp[0]; o.a[1] = sp[64]; o.sa = sp[128];
        o.b[0] = sp[192]; o.b[1] = sp[256]; o.sb = sp[320];
        // the slot is free once its reads returned: refill it RS blocks ahead
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        issue(min(blk + RS, nb - 1), slot);
        slot = slot + 1 == RS ? 0 : slot + 1;

        block41(o, acc, off);
#pragma unroll
        for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(acc[c]));
    }
    // the trailing refills must land before the workgroup's LDS is released
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    mm_finish<EPI>(P.o, acc, lane, w, m0, n0, off);
}

// activation quantizer for the Q4_1 MFMA path: x[t] (optionally rms_norm * g, mm_common.h
// act_units) -> quantize_row_q4_1 (AVX2 branch, ggml.c:847-920; mv::q41_quad) -> the
// fragment and side images (act41_emit).  One workgroup per token, one lane quad per block.
template <bool NORM>
__global__ __launch_bounds__(256) void k_act_q41_f16(const float * __restrict__ x, const float * __restrict__ g, int N,
                                                     int K, uint4 * __restrict__ xm, uint4 * __restrict__ xs) {
    act_units<NORM>(x, g, N, K, [&](int t, int u, bool live, const float (&v)[8]) {
        float d, m;
        uint32_t qword;
        mv::q41_quad(v, d, m, qword);
        if (live) act41_emit(t, K / 32, u >> 2, u & 3, qword, d, m, xm, xs);
    });
}

// pre-quantized Q4_1 blocks (ActQ: d, m + reference nibble qs) -> fragment and side images;
// one lane quad per block
__global__ void k_actq41_to_f16(ActQ q, int N, int K, uint4 * __restrict__ xm, uint4 * __restrict__ xs) {
    const int nb = K / 32;
    const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;   // (token, block, quad lane)
    const long tb = idx >> 2;
    const bool live = tb < (long) N * nb;
    const int k = (int) (idx & 3);
    const long tbc = live ? tb : 0;
    const uint4 qs = q.qs[tbc];
    const uint32_t wd[4] = {qs.x, qs.y, qs.z, qs.w};
    if (live) act41_emit((int) (tbc / nb), nb, (int) (tbc % nb), k, wd[k], q.d[tbc], q.m[tbc], xm, xs);
}

// weight images of a Q4_1 octet image (k_repack_q41 layout): one thread per (32-row tile,
// block, lane (rho, h)).  a16: the chain fragments 2c+h (c = 0..3) of row 32 rt + rho as
// f16 q in the order e0 e2 e1 e3, pairs side by side; side: h = 0 {the row's four group
// sums of the block as f16, d}, h = 1 {ones, m}
__global__ void k_mm41_images(const uint4 * __restrict__ nibi, const float * __restrict__ scl, int M, int K,
                              uint2 * __restrict__ a16, uint4 * __restrict__ side) {
    const int nb = K / 32, NC = (nb + 31) / 32;
    const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;     // (rt * nb + b) * 64 + lane
    if (idx >= (long) (M / 32) * nb * 64) return;
    const int lane = (int) (idx & 63), h = lane >> 5;
    const long rb = idx >> 6;
    const int b = (int) (rb % nb), rt = (int) (rb / nb);
    const int row = rt * 32 + (lane & 31);
    uint32_t field[8];                          // chain j: nibbles {2j, 2j+1, 16+2j, 17+2j}
#pragma unroll
    for (int j = 0; j < 8; ++j) field[j] = octet_chain_field(nibi, row, b, NC, j);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t tf = field[2 * c + h];
        a16[a16_slot(rt, nb, b, c, lane)] =
            make_uint2(h16(nib(tf, 0)) | h16(nib(tf, 2)) << 16, h16(nib(tf, 1)) | h16(nib(tf, 3)) << 16);
    }
    // group q = elements 8q..8q+7: the low (q < 2) or high (q >= 2) nibble pairs of chains 4(q&1)..+3
    uint32_t gs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t s = 0;
#pragma unroll
        for (int j = 4 * (q & 1); j < 4 * (q & 1) + 4; ++j) s += nib(field[j], 2 * (q >> 1)) + nib(field[j], 2 * (q >> 1) + 1);
        gs[q] = s;
    }
    // d / m of block b: scl[g][c][dm][8r + j] component mq, b = 32c + 8mq + j
    const size_t sidx = ((((size_t) (row >> 3) * NC + (b >> 5)) * 2 + h) * 64 + 8 * (row & 7) + (b & 7)) * 4 + ((b & 31) >> 3);
    const uint32_t sv = __builtin_bit_cast(uint32_t, scl[sidx]);
    side[idx] = h == 0 ? make_uint4(h16(gs[0]) | h16(gs[1]) << 16, h16(gs[2]) | h16(gs[3]) << 16, sv, 0u)
                       : make_uint4(F16_ONE | F16_ONE << 16, F16_ONE | F16_ONE << 16, sv, 0u);
}

}  // namespace

size_t mm41_side_bytes(int M, int K) { return (size_t) (M / 32) * (K / 32) * 64 * 16; }

hipError_t launch_build_mm41(const QMatrix & w, void * a16, void * side, hipStream_t s) {
    if (w.qtype != Q4_1 || w.M % 32 || w.K % 256) return hipErrorInvalidValue;
    const long n = (long) (w.M / 32) * (w.K / 32) * 64;
    LVK_LAUNCH(k_mm41_images, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, w.nib, (const float *) w.scl, w.M,
               w.K, (uint2 *) a16, (uint4 *) side);
    return hipGetLastError();
}

hipError_t mm_q41(const MmLaunch & L, int epi, hipStream_t s) {
    const QMatrix & w = L.w;
    Mm41Params P{};
    P.a16 = (const uint4 *) w.a16; P.side = (const uint4 *) w.side;
    P.xm = (const uint4 *) L.x.xm; P.xs = (const uint4 *) L.x.xs;
    P.M = w.M; P.nb = w.K / 32;
    P.o = mm_out(L, epi);
    const dim3 grid((w.M / TM) * P.o.ntt);
    // LVK_MM41_DMA=0: the register-ring kernel instead of the LDS-DMA ring
    const char * dma_env = getenv("LVK_MM41_DMA");
    const bool dma = !dma_env || atoi(dma_env) != 0;
    return mm_epi_dispatch<Q4_1>(epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        if (dma) LVK_LAUNCH(k_mm_q41_dma<E>, grid, dim3(NT), LDS41, s, P);
        else LVK_LAUNCH(k_mm_q41_mfma<E>, grid, dim3(NT), 0, s, P);
        return hipGetLastError();
    });
}

hipError_t act_q41(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s) {
    const dim3 gt((unsigned) ((N + 127) / 128 * 128));   // XCD-grouped token order
    if (g) LVK_LAUNCH(k_act_q41_f16<true>, gt, dim3(256), 0, s, x, g, N, K, (uint4 *) out.xm, (uint4 *) out.xs);
    else LVK_LAUNCH(k_act_q41_f16<false>, gt, dim3(256), 0, s, x, g, N, K, (uint4 *) out.xm, (uint4 *) out.xs);
    return hipGetLastError();
}

hipError_t actq_image_q41(const ActQ & q, int N, int K, const ActImage & out, hipStream_t s) {
    const long n = (long) N * (K / 32) * 4;
    LVK_LAUNCH(k_actq41_to_f16, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, q, N, K, (uint4 *) out.xm,
               (uint4 *) out.xs);
    return hipGetLastError();
}

}  // namespace lvk
