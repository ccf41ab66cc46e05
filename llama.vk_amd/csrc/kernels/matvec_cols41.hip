// matvec_cols41.hip -- CU-balanced Q4_1 matmul for a batched decode step of 2 or more activation
// columns (rows of the step): the Q4_1 counterpart of matvec_cols.hip.
//
// Same arithmetic and result bits as matvec_cu41.hip / matvec_q41.hip (ggml_vec_dot_q4_1's AVX2
// form, ggml.c:2188-2258, on columns quantized by quantize_row_q4_1, ggml.c:847-920); per block in
// order and chain j:
//     acc_j = fmaf(dx*dy, (float) p_j, acc_j)                    p_j: exact v_dot8_u32_u4 partial
//     acc_j = fmaf(j even ? dx*my : mx*dy, (float) S_j, acc_j)   S_j: weight / activation sums
//     off   = off + mx*my
//   result = octet_reduce(acc) + off * 32
// The organisation is matvec_cols.hip's (one workgroup per CU with matvec_cu.hip's row-group
// split, lane 8r + j = chain j of row r, a chunk's weights in registers applied to a tile of T
// columns held in LDS, the columns split over CSP waves per row group where a CU has fewer row
// groups than waves).  What differs:
//
//   * the ring.  The Q4_1 row lengths have any number of chunks (4096: 4, 5120: 5, 11008: 10 + 24
//     blocks, 13824: 13 + 16 blocks), so the slots are not named by the chunk's parity: the
//     chunk loop is a runtime loop over one body.  The chunk in flight (nibbles, d, m, weight
//     sums: 28 registers) is moved into the working set (the nibble words split into their
//     half-masked forms) at the top of the body, and the load of the wave's next chunk -- this
//     row group's, the next row group's or the next tile's -- goes out into the freed registers
//     before the chunk's arithmetic: two slots, one code copy, a cursor (row group, chunk)
//     that runs on across row groups and tiles.  The partial last chunk takes the same body
//     with a runtime sub-chunk count (uniform branches); its missing sub-chunks are loaded from
//     the chunk's first one (valid memory, no branch around the issue) and never used;
//   * the column table, per block 16 B of packed nibbles (matvec_cols.hip's 16 bits per (block,
//     chain): half-masked weight words are exact for unsigned nibbles as well), dy, my and the four
//     activation sums of the odd chains as bytes: 28 B per block, chunk-padded.  The tile is the
//     widest that fits 160 KiB with the product slices: 16 columns of K = 4096 / 5120, 12 of
//     11008, 8 of 13824;
//   * the products.  s = dx*dy, dx*my, mx*dy and mx*my of a chunk's 32 blocks go through one
//     per-wave LDS slice of four tables (matvec_cu41.hip's padded layout, 5 KiB per wave), written
//     per column right before that column's chains; no second slice: the ring of matvec_cols.hip
//     would take 80 KiB.
// k_cols41_act converts the step's rows once into a global image that is exactly the table.
// No workgroup waits on another: plain vector loads and stores only.
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

namespace lvk {

namespace {
using namespace mv;

struct Cols41Params : MvArgs {
    const uint4 * nib;
    const float4 * scl;         // [G][NC][2][64]: d, then m
    const uint4 * wsum;         // [G][NC][64]: even-chain weight sums (lvk_kernels.h q41_wsum)
    const uint4 * img;          // the packed column image (k_cols41_act), column t at t * CS16
    int G;                      // row groups (M / 8)
    int M;                      // rows: the column stride of y (u: M / 2)
    int col0, ncols;            // this launch's columns [col0, col0 + ncols)
};

// per-wave product tables (s, dx*my, mx*dy, mx*my) of 8 rows x 32 blocks, matvec_cu41.hip's
// padded row stride: the per-row broadcast float4 reads and the lane stores are conflict free
constexpr int SRS = 40, SPL = 8 * SRS, SWF = 4 * SPL;

// packed column image / LDS table of one column of K = 32 nb elements (NC chunks), in uint4 units:
//   [nb]     nibbles: uint4 (8 u + j), u < nb / 8, chain j: word k = a(8u + 2k, j) | a(8u + 2k + 1, j) << 16,
//            a(i, j) = qs byte j | qs byte 8 + j << 8 of block i (act41_store's 16 bits)
//   [NC * 8] dy: float [c][j][m] = d of block 32 c + 8 m + j (0 past the row's end)
//   [NC * 8] my: the same for m
//   [NC * 8] ys: byte [c][q][i] = the sum of the 8 nibbles of qs word q of block 32 c + i
__host__ __device__ constexpr int cols41_stride16(int K) { return K / 32 + (K / 32 + 31) / 32 * 24; }

// a finished block i of a column (act41_store's values in the packed form)
__device__ __forceinline__ void cols41_block_store(uint4 * col, int nb, int i, const uint32_t (&qs)[4], float d, float m) {
    const int NC = (nb + 31) / 32;
    uint16_t * p16 = (uint16_t *) col;
    float * dyp = (float *) (col + nb);
    float * myp = dyp + NC * 32;
    uint8_t * ys = (uint8_t *) (myp + NC * 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t lo = (qs[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        const uint32_t hi = (qs[2 + (j >> 2)] >> (8 * (j & 3))) & 0xFFu;
        p16[(size_t) (((i >> 3) * 8 + j) * 8 + (i & 7))] = (uint16_t) (lo | (hi << 8));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ys[(size_t) ((i >> 5) * 4 + q) * 32 + (i & 31)] = (uint8_t) udot8(qs[q], 0x11111111u);
    const int o = (i >> 5) * 32 + (i & 7) * 4 + ((i >> 3) & 3);
    dyp[o] = d;
    myp[o] = m;
}

// One workgroup per step row t: the row's packed column.  PRO_NORM: g * rms_norm(x[t]) quantized;
// PRO_ACTF: x[t] quantized; PRO_ACTQ: the blocks of xq row t reshuffled.
template <int PRO>
__global__ __launch_bounds__(256) void k_cols41_act(const float * x, const float * g, ActQ xq, int K, uint4 * img) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int nb = K / 32, NC = (nb + 31) / 32;
    uint4 * col = img + (size_t) t * cols41_stride16(K);
    // the partial last chunk's padding: d = m = 0, sums 0 (written by no block below)
    if (nb % 32) {
        float * dyp = (float *) (col + nb);
        uint32_t * ys32 = (uint32_t *) (dyp + NC * 64);
        for (int i = nb + tid; i < NC * 32; i += 256) {
            const int o = (i >> 5) * 32 + (i & 7) * 4 + ((i >> 3) & 3);
            dyp[o] = 0.0f;
            dyp[NC * 32 + o] = 0.0f;
        }
        // sums of blocks nb .. 32 NC - 1: whole words (nb % 4 == 0) of the last chunk's four rows
        for (int w = tid; w < 4 * 8; w += 256)
            if ((w & 7) * 4 >= nb % 32) ys32[(NC - 1) * 32 + w] = 0u;
    }
    if constexpr (PRO == PRO_ACTQ) {
        for (int b = tid; b < nb; b += 256) {
            const uint4 q = xq.qs[(size_t) t * nb + b];
            const uint32_t qs[4] = {q.x, q.y, q.z, q.w};
            cols41_block_store(col, nb, b, qs, xq.d[(size_t) t * nb + b], xq.m[(size_t) t * nb + b]);
        }
    } else {
        const float * xr = x + (size_t) t * K;
        float scale = 1.0f;
        if constexpr (PRO == PRO_NORM) scale = rms_scale_256(xr, K);
        const int nunits = K / 8;               // a multiple of 4: a block is a whole lane quad
        for (int u0 = 0; u0 < nunits; u0 += 256) {
            const int un = u0 + tid, uc = min(un, nunits - 1);
            const float4 * xp = (const float4 *) (xr + (size_t) uc * 8);
            float4 ga = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gb = ga;
            if constexpr (PRO == PRO_NORM) {
                const float4 * gp = (const float4 *) (g + (size_t) uc * 8);
                ga = gp[0]; gb = gp[1];
            }
            float v[8];
            unit_vals(xp[0], xp[1], v);
            pro_norm_unit<PRO>(v, ga, gb, scale);
            // quantize_row_q4_1 of the quad's block, its 4 qs words gathered into every lane; the
            // quad's first lane stores it (q41_unit_store, with the packed store)
            float d, m;
            uint32_t qw;
            q41_quad(v, d, m, qw);
            uint32_t qs[4];
            qs[0] = __builtin_bit_cast(uint32_t, quad_bcast<0>(__builtin_bit_cast(float, qw)));
            qs[1] = __builtin_bit_cast(uint32_t, quad_bcast<1>(__builtin_bit_cast(float, qw)));
            qs[2] = __builtin_bit_cast(uint32_t, quad_bcast<2>(__builtin_bit_cast(float, qw)));
            qs[3] = __builtin_bit_cast(uint32_t, quad_bcast<3>(__builtin_bit_cast(float, qw)));
            if (un < nunits && (un & 3) == 0) cols41_block_store(col, nb, un >> 2, qs, d, m);
        }
    }
}

// T columns per tile, NW waves, row length KT compiled in.  CSP: the tile's columns are split over
// CSP waves per row group (TW = T / CSP columns each; wave w works on row groups w / CSP,
// w / CSP + NW / CSP, ... and the columns (w % CSP) * TW ...), as in matvec_cols.hip.
template <int T, int CSP, int EPI, int KT, int NW>
__global__ __launch_bounds__(NW * 64) void k_mv_cols41(Cols41Params P) {
    constexpr int NT = NW * 64;
    constexpr int nb = KT / 32;
    constexpr int nsub = nb / 8;                // 8-block sub-chunks of a row
    constexpr int NC = (nb + 31) / 32;          // chunks, the last one partial when nb % 32
    constexpr int TS = (nb % 32) / 8;           // sub-chunks of the partial last chunk (0: none)
    constexpr int CS16 = cols41_stride16(KT);
    constexpr int CPT = (T * CS16 + NT - 1) / NT;       // table uint4 per thread
    constexpr int TW = T / CSP;                 // columns per wave
    constexpr int NWG = NW / CSP;               // row groups in flight per workgroup
    static_assert(nb % 8 == 0 && NC >= 2, "row length");
    static_assert(TW >= 1 && TW * CSP == T && NWG * CSP == NW, "column split");

    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint4 * tab = (uint4 *) smem;                           // T * CS16
    float * sbuf = (float *) (tab + T * CS16);              // NW * SWF

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 7;
    const int r = lane >> 3;
    const int bid = blockIdx.x, nwg = gridDim.x;
    const int g0 = (int) ((unsigned) bid * (unsigned) P.G / (unsigned) nwg);
    const int g1 = (int) ((unsigned) (bid + 1) * (unsigned) P.G / (unsigned) nwg);
    const int wv = wave / CSP, sub = wave % CSP;                // row-group lane, column part
    const int ng = max(0, (g1 - g0 - wv + NWG - 1) / NWG);      // row groups of this wave
    const int gfirst = min(g0 + wv, P.G - 1);
    // a wave without row groups (it only copies the table) issues the ring's first load with
    // every lane on one 16-byte word: no branch around the issue
    const uint32_t loff = ng > 0 ? (uint32_t) lane * 16u : 0u;

    // a tile's columns: a straight copy of the image, through registers.  The barrier between
    // the loads and the stores: every wave is done with the previous tile's table
#define LVK_TABLE_COPY(t0_, nt_, barrier_)                                                              \
    do {                                                                                                \
        const u32x4 * src_ = (const u32x4 *) P.img + (size_t) (t0_) * CS16;                             \
        const int cnt_ = (nt_) * CS16;                                                                  \
        u32x4 tv_[CPT];                                                                                 \
        _Pragma("unroll") for (int k = 0; k < CPT; ++k) tv_[k] = src_[min(k * NT + tid, cnt_ - 1)];     \
        if (barrier_) __syncthreads();                                                                  \
        _Pragma("unroll") for (int k = 0; k < CPT; ++k)                                                 \
            if (k * NT + tid < cnt_) ((u32x4 *) tab)[k * NT + tid] = tv_[k];                            \
        __syncthreads();                                                                                \
    } while (0)

    // the slot in flight: chunk cc of row group grp.  Per chunk the images hold nib [4 sub][1 KiB],
    // d | m [2][1 KiB], wsum [1 KiB]; a lane's slice of each 1 KiB is its 16 bytes.  Sub-chunks
    // past the row's end (the partial chunk's) come from the chunk's first one
    uint4 NW_[4], NWS;
    float4 ND, NM;
#define LVK_ISSUE41(grp, cc)                                                                            \
    do {                                                                                                \
        const size_t ch_ = (size_t) (grp) * NC + (cc);                                                  \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                              \
            const int sq_ = (TS == 0 || (cc) * 4 + sb < nsub) ? sb : 0;                                 \
            NW_[sb] = ld_nt((const uint4 *) ((const char *) P.nib + (ch_ * 4 + sq_) * 1024 + loff));    \
        }                                                                                               \
        ND = ld_nt((const float4 *) ((const char *) P.scl + ch_ * 2048 + loff));                        \
        NM = ld_nt((const float4 *) ((const char *) P.scl + ch_ * 2048 + 1024 + loff));                 \
        NWS = ld_nt((const uint4 *) ((const char *) P.wsum + ch_ * 1024 + loff));                       \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)

    const int ntiles = (P.ncols + T - 1) / T;
    // the weights are in flight under the table copy
    LVK_ISSUE41(gfirst, 0);

    float * sw = sbuf + wave * SWF;
    const uint4 * tabw = tab + sub * TW * CS16;     // this wave's columns
    const bool even = (j & 1) == 0;
    float acc[TW], off[TW];

    for (int tile = 0; tile < ntiles; ++tile) {
        const int t0 = P.col0 + tile * T;
        const int nt = min(T, P.col0 + P.ncols - t0);
        LVK_TABLE_COPY(t0, nt, tile > 0);
        if (ng == 0) continue;
        int gc = gfirst;
        for (int k = 0; k < ng; ++k) {
            // what the ring fetches behind this row group: the wave's next one, or its first
            // again (the next tile's; after the last tile a redundant, valid load)
            const int gn = k + 1 < ng ? gc + NWG : gfirst;
            // the residual terms ahead of the chunk loop for a few columns (mv_pre_epi)
            [[maybe_unused]] float rv[TW];
            if constexpr (EPI == EPI_RESID && TW <= 4) {
#pragma unroll
                for (int tt = 0; tt < TW; ++tt)
                    rv[tt] = P.y[(size_t) min(t0 + sub * TW + tt, t0 + nt - 1) * P.M + gc * 8 + r];
            }
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) { acc[tt] = 0.0f; off[tt] = 0.0f; }
#pragma unroll 1
            for (int c = 0; c < NC; ++c) {
                // the slot in flight becomes the working set: wl / wh, the chunk's weight words
                // split into their low / high 16 bits (blocks 2k / 2k + 1 of a word's pair)
                uint32_t wl[4][4], wh[4][4];
#pragma unroll
                for (int sb = 0; sb < 4; ++sb) {
                    const uint32_t wd[4] = {NW_[sb].x, NW_[sb].y, NW_[sb].z, NW_[sb].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        wl[sb][q] = wd[q] & 0xFFFFu;
                        wh[sb][q] = wd[q] & 0xFFFF0000u;
                    }
                }
                const float dxa[4] = {ND.x, ND.y, ND.z, ND.w};
                const float mxa[4] = {NM.x, NM.y, NM.z, NM.w};
                // the even chains' sums: blocks 0-15 of the chunk in the lane's own words, 16-31 in
                // the odd neighbour's (DPP quad_perm [1,1,3,3]); one byte per block
                uint32_t wsw[8] = {NWS.x, NWS.y, NWS.z, NWS.w, 0u, 0u, 0u, 0u};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    wsw[4 + q] = (uint32_t) __builtin_amdgcn_mov_dpp((int) wsw[q], 0xF5, 0xF, 0xF, false);
                // the working set is pinned before the slot is refilled
#pragma unroll
                for (int sb = 0; sb < 4; ++sb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(wl[sb][q]), "+v"(wh[sb][q]));
#pragma unroll
                for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(wsw[q]));
                const bool own = c + 1 < NC;
                LVK_ISSUE41(own ? gc : gn, own ? c + 1 : 0);
                const int nsb = (TS > 0 && c == NC - 1) ? TS : 4;

                // every column of the tile runs its chains: those past the step's last one (ct >= nt)
                // read table bytes this launch never wrote, and their results are dropped at the epilogue
#pragma unroll
                for (int tt = 0; tt < TW; ++tt) {
                    const uint4 * colp = tabw + tt * CS16;
                    // products of blocks 32c + 8m + j of this lane's row with column tt (ggml.c:2205-2212):
                    // slot 8m + j of the tables s = dx*dy, dx*my, mx*dy, mx*my
                    const float4 dy = *(const float4 *) ((const float *) (colp + nb) + c * 32 + j * 4);
                    const float4 my = *(const float4 *) ((const float *) (colp + nb + NC * 8) + c * 32 + j * 4);
                    const uint4 * ysp = colp + nb + NC * 16 + (c * 4 + (j >> 1)) * 2;
                    const uint4 y0 = ysp[0], y1 = ysp[1];
                    const uint32_t ysw[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
                    const float dya[4] = {dy.x, dy.y, dy.z, dy.w};
                    const float mya[4] = {my.x, my.y, my.z, my.w};
                    __builtin_amdgcn_wave_barrier();        // the previous column's reads are issued
                    float * sl = sw + r * SRS + j;
#pragma unroll
                    for (int mq = 0; mq < 4; ++mq) {
                        sl[mq * 8] = dxa[mq] * dya[mq];
                        sl[SPL + mq * 8] = dxa[mq] * mya[mq];
                        sl[2 * SPL + mq * 8] = mxa[mq] * dya[mq];
                        sl[3 * SPL + mq * 8] = mxa[mq] * mya[mq];
                    }
                    __builtin_amdgcn_wave_barrier();
                    const float * srow = sw + r * SRS;
                    const float * xrow = srow + (even ? SPL : 2 * SPL);
                    const float * mrow = srow + 3 * SPL;
                    float a = acc[tt], o = off[tt];
#pragma unroll
                    for (int sb = 0; sb < 4; ++sb) {
                        if (sb < nsb) {
                            const uint4 A = colp[(c * 4 + sb) * 8 + j];
                            const uint32_t aw[4] = {A.x, A.y, A.z, A.w};
#pragma unroll
                            for (int pp = 0; pp < 2; ++pp) {
                                const int bi = sb * 8 + pp * 4;       // first of 4 blocks within the chunk
                                const float4 s4 = *(const float4 *) (srow + bi);
                                const float4 x4 = *(const float4 *) (xrow + bi);
                                const float4 m4 = *(const float4 *) (mrow + bi);
                                // even chains: the weight sums; odd chains: the activation sums
                                const uint32_t sdw = even ? wsw[sb * 2 + pp] : ysw[sb * 2 + pp];
                                const float S[4] = {(float) (sdw & 0xFFu), (float) ((sdw >> 8) & 0xFFu),
                                                    (float) ((sdw >> 16) & 0xFFu), (float) (sdw >> 24)};
                                const int p[4] = {udot8(wl[sb][2 * pp], aw[2 * pp]), udot8(wh[sb][2 * pp], aw[2 * pp]),
                                                  udot8(wl[sb][2 * pp + 1], aw[2 * pp + 1]),
                                                  udot8(wh[sb][2 * pp + 1], aw[2 * pp + 1])};
                                const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
                                const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
                                const float ms[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    a = __builtin_fmaf(sv[q], (float) p[q], a);
                                    a = __builtin_fmaf(xs[q], S[q], a);
                                    o = o + ms[q];
                                }
                            }
                        }
                    }
                    // keep the columns in program order: the chain values are pinned here, so hipcc
                    // cannot hoist every column's LDS traffic above the first column's arithmetic
                    asm volatile("" : "+v"(a), "+v"(o));
                    acc[tt] = a;
                    off[tt] = o;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // per column: the shared single-token epilogue on that column's outputs;
            // res = hsum(acc) + acc_offset * QK (ggml.c:2249)
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) {
                const float res = octet_reduce(acc[tt]) + off[tt] * 32.0f;
                const int ct = sub * TW + tt;           // column within the tile
                if (ct < nt) {
                    MvArgs A = P;
                    A.y = P.y + (size_t) (t0 + ct) * P.M;
                    A.u = P.u + (size_t) (t0 + ct) * (P.M / 2);
                    EpiPre pe{make_float2(0.0f, 0.0f), 0.0f};
                    if constexpr (EPI == EPI_RESID) {
                        if constexpr (TW <= 4) pe.rv = rv[tt];
                        else pe.rv = A.y[gc * 8 + r];
                    }
                    mv_epilogue<EPI>(A, gc, r, j, res, 0, pe);
                }
            }
            gc += NWG;
        }
    }
#undef LVK_TABLE_COPY
#undef LVK_ISSUE41
}

// -- host -------------------------------------------------------------------

// the widest tile of a row length: what fits 160 KiB of LDS beside the product slices
constexpr int cols41_tmax(int K) { return K == 13824 ? 8 : K == 11008 ? 12 : 16; }

template <int T, int CSP, int EPI, int KT, int NW>
hipError_t go_t(const Cols41Params & P, int nwg, hipStream_t s) {
    constexpr size_t lds = (size_t) T * cols41_stride16(KT) * 16 + (size_t) NW * SWF * 4;
    static_assert(lds <= 160 * 1024, "LDS");
    // more than the default 64 KiB of dynamic LDS: opted in per device and not stream-ordered, so
    // with every launch (as matvec_cols.hip does)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *) k_mv_cols41<T, CSP, EPI, KT, NW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    LVK_LAUNCH((k_mv_cols41<T, CSP, EPI, KT, NW>), dim3(nwg), dim3(NW * 64), lds, s, P);
    return hipGetLastError();
}

// the column split of a tile of T: the one with the least chain work on the busiest wave
// (matvec_cols.hip go_split; a chunk's fixed part -- the split, the sums, the issue -- costs about
// 0.4 of a column here too)
template <int T, int EPI, int KT, int NW>
hipError_t go_split(const Cols41Params & P, hipStream_t s) {
    const int nwg = std::min(cu_count(), P.G);
    const int gpc = (P.G + nwg - 1) / nwg;
    int best = 1;
    float cost = 0.0f;
    for (int csp = 1; csp <= 4 && csp <= T; csp *= 2) {
        const int rounds = (gpc + NW / csp - 1) / (NW / csp);
        const float c = (float) rounds * ((float) (T / csp) + 0.4f);
        if (csp == 1 || c < cost) { best = csp; cost = c; }
    }
    if constexpr (T >= 4)
        if (best == 4) return go_t<T, 4, EPI, KT, NW>(P, nwg, s);
    if (best >= 2) return go_t<T, 2, EPI, KT, NW>(P, nwg, s);
    return go_t<T, 1, EPI, KT, NW>(P, nwg, s);
}

// the columns [col0, col0 + ncols) with the narrowest tile that holds them
template <int EPI, int KT>
hipError_t go_cols(Cols41Params P, int col0, int ncols, hipStream_t s) {
    P.col0 = col0; P.ncols = ncols;
    constexpr int NW = 8, TM = cols41_tmax(KT);
    if (ncols <= 2) return go_split<2, EPI, KT, NW>(P, s);
    if (ncols <= 4) return go_split<4, EPI, KT, NW>(P, s);
    if (ncols <= 8 || TM == 8) return go_split<8, EPI, KT, NW>(P, s);
    return go_split<TM, EPI, KT, NW>(P, s);
}

// a step of n columns: the whole widest tiles in one launch (tiled inside the workgroup), the
// rest in a second one with its own tile width
template <int EPI, int KT>
hipError_t go(const Cols41Params & P, int n, hipStream_t s) {
    constexpr int TM = cols41_tmax(KT);
    const int nfull = n > TM ? n / TM * TM : n;
    if (nfull == n) return go_cols<EPI, KT>(P, 0, n, s);
    EventSplit ev;      // timed as one: the stop event goes to the second launch
    g_launch_events = {nullptr, nullptr};
    const hipError_t e = go_cols<EPI, KT>(P, 0, nfull, s);
    if (e != hipSuccess) return e;
    ev.last();
    return go_cols<EPI, KT>(P, nfull, n - nfull, s);
}

template <int KT>
hipError_t go_epi(const Cols41Params & P, int epi, int n, hipStream_t s) {
    switch (epi) {
        case EPI_STORE: return go<EPI_STORE, KT>(P, n, s);
        case EPI_RESID: return go<EPI_RESID, KT>(P, n, s);
        default: return go<EPI_SWIGLU_F32, KT>(P, n, s);
    }
}

}  // namespace

// row lengths compiled in: n_embd and n_ff of LLaMA 13B and 7B
bool matvec_cols41_supported(int K, int n) {
    return (K == 4096 || K == 5120 || K == 11008 || K == 13824) && n >= 2;
}

size_t matvec_cols41_image_bytes(int K, int n) { return (size_t) n * cols41_stride16(K) * 16; }

hipError_t launch_matvec_cols41(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    const int K = L.w.K, n = L.n_tokens;
    if (L.w.qtype != Q4_1 || !matvec_cols41_supported(K, n) || L.w.M % 8 || L.tok0 != 0) return hipErrorNotSupported;
    const bool ff = K == 11008 || K == 13824;       // n_ff: the W2 role only
    const bool pair = ff ? (pro == PRO_ACTF && epi == EPI_RESID)
                         : ((pro == PRO_NORM && (epi == EPI_STORE || epi == EPI_SWIGLU_F32)) ||
                            (pro == PRO_ACTQ && epi == EPI_RESID));
    if (!pair) return hipErrorNotSupported;
    if (!mv_inputs_set(L, pro) || !L.cols_img || !L.w.nib || !L.w.scl) return hipErrorInvalidValue;
    if (epi == EPI_SWIGLU_F32 ? (!L.u || !L.silu_tab) : !L.y) return hipErrorInvalidValue;
    Cols41Params P{};
    mv_fill(P, L, false);
    P.nib = L.w.nib;
    P.scl = (const float4 *) L.w.scl;
    P.wsum = q41_wsum(L.w);
    P.img = (const uint4 *) L.cols_img;
    P.G = L.w.M / 8;
    P.M = L.w.M;
    // the step's rows, once, into the packed image; timed with the matmul as one launch
    EventSplit ev;
    ev.first();
    uint4 * img = (uint4 *) L.cols_img;
    switch (pro) {
        case PRO_NORM: LVK_LAUNCH((k_cols41_act<PRO_NORM>), dim3(n), dim3(256), 0, s, L.x, L.g, L.xq, K, img); break;
        case PRO_ACTF: LVK_LAUNCH((k_cols41_act<PRO_ACTF>), dim3(n), dim3(256), 0, s, L.x, L.g, L.xq, K, img); break;
        default: LVK_LAUNCH((k_cols41_act<PRO_ACTQ>), dim3(n), dim3(256), 0, s, L.x, L.g, L.xq, K, img); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ev.last();
    switch (K) {
        case 4096: return go_epi<4096>(P, epi, n, s);
        case 5120: return go_epi<5120>(P, epi, n, s);
        case 11008: return go<EPI_RESID, 11008>(P, n, s);
        default: return go<EPI_RESID, 13824>(P, n, s);
    }
}

}  // namespace lvk
