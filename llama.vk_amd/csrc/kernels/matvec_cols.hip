// matvec_cols.hip -- CU-balanced Q4_0 matmul for a batched decode step of 2..64 activation
// columns (rows of the step).
//
// Same arithmetic and result bits as matvec_cu.hip / matvec_q4.hip (ggml_vec_dot_q4_0's AVX2
// chains, ggml.c:1950-2026, on columns quantized by quantize_row_q4_0, ggml.c:621-685): exact
// integer partials from v_dot8_i32_i4, fmaf(dw * dx, P, acc) in block order per chain, the
// octet reduce for the horizontal order.  The organisation is matvec_cu.hip's, widened to a
// tile of T columns:
//
//   * one workgroup per CU, workgroup w owns row groups [w*G/n, (w+1)*G/n); a wave owns a row
//     group at a time, lane 8r + j is chain j of row r; where a CU has fewer row groups than
//     waves, the tile's columns are split over 2 or 4 waves per row group (CSP);
//   * the weights of a chunk (32 blocks of the wave's 8 rows) are loaded once into registers
//     and applied to all T columns of the tile (acc[T] per lane): T times the work per weight
//     byte of the generic multi-row kernel, which re-streams the weights per 4 rows;
//   * the columns sit in LDS in a packed table of 20 B per block (16 B of nibbles + 4 B of
//     dx): a table word holds the 16-bit nibble groups of two blocks, and the weight word is
//     split once per chunk into its two half-masked words (the zero half contributes exact
//     zeros to the dot), instead of the table carrying zero-padded words as matvec_cu.hip's
//     does at 32 B per block.  16 columns of K = 11008 take 108 KiB;
//   * no workgroup builds the table from f32: k_cols_act converts the step's rows once (RMSNorm +
//     quantize, plain quantize, or the attention's blocks reshuffled) into a global image that
//     is exactly the table, and the matmul's prologue is a straight copy of its T columns;
//   * the block-scale products s = dw * dx go through a per-wave LDS slice (matvec_cu.hip's
//     padded, conflict-free layout), one column at a time in a two-slice ring: column t + 1's
//     slice is written before column t's chains run;
//   * a step of more than T columns is handled in tiles inside the workgroup: the table is
//     rebuilt and the workgroup's row groups are streamed again (from L2 / Infinity Cache);
//     the weight ring runs on across row groups and tiles.
// No workgroup waits on another: plain vector loads and stores only.
#include <type_traits>
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"
#include "matvec_cols_common.h"

namespace lvk {

namespace {
using namespace mv;
using namespace cols;

// the packed column image (matvec_cols_common.h): the stores of one block's nibble group and dx
__device__ __forceinline__ void cols_store16(uint16_t * p16, int i, int j, uint32_t v) {
    p16[(size_t) (((i >> 3) * 8 + j) * 8 + (i & 7))] = (uint16_t) v;
}
__device__ __forceinline__ void cols_store_dx(float * dxp, int i, float d) {
    dxp[(size_t) (i >> 5) * 32 + (i & 7) * 4 + ((i >> 3) & 3)] = d;
}

// quantize_row_q4_0 of the block a lane quad holds (unit un = this lane's 8 elements) into the
// packed table: q40_unit_store's arithmetic (matvec_common.h), the packed store
__device__ __forceinline__ void cols_unit_store(const float (&v)[8], int un, bool live, uint16_t * p16, float * dxp) {
    float d;
    uint32_t w;
    q40_quad(v, d, w);
    if (!live) return;
    const uint32_t s = w ^ 0x88888888u;         // elements 8q .. 8q + 7 as signed nibbles: chains 2q, 2q + 1
    const int i = un >> 2, q = un & 3;
    cols_store16(p16, i, 2 * q, s & 0xFFFFu);
    cols_store16(p16, i, 2 * q + 1, s >> 16);
    if (q == 0) cols_store_dx(dxp, i, d);
}

// One workgroup per step row t: the row's packed column.  PRO_NORM: g * rms_norm(x[t]) quantized;
// PRO_ACTF: x[t] quantized; PRO_ACTQ: the blocks of xq row t reshuffled.
template <int PRO>
__global__ __launch_bounds__(256) void k_cols_act(const float * x, const float * g, ActQ xq, int K, uint4 * img) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int nb = K / 32, NC = (nb + 31) / 32;
    uint4 * col = img + (size_t) t * cols_stride16(K);
    uint16_t * p16 = (uint16_t *) col;
    float * dxp = (float *) (col + nb);
    for (int i = nb + tid; i < NC * 32; i += 256) cols_store_dx(dxp, i, 0.0f);
    if constexpr (PRO == PRO_ACTQ) {
        for (int b = tid; b < nb; b += 256) {
            const uint4 qs = xq.qs[(size_t) t * nb + b];
            const uint32_t w[4] = {qs.x, qs.y, qs.z, qs.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t s = w[q] ^ 0x88888888u;
                cols_store16(p16, b, 2 * q, s & 0xFFFFu);
                cols_store16(p16, b, 2 * q + 1, s >> 16);
            }
            cols_store_dx(dxp, b, xq.d[(size_t) t * nb + b]);
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
            cols_unit_store(v, un, un < nunits, p16, dxp);
        }
    }
}

// T columns per tile, NW waves, row length KT compiled in: FC full chunks of 32 blocks through
// a two-slot register ring (FC is even, so a row group always starts on slot 0), the partial
// last chunk of K = 11008 (24 blocks) through a slot of its own.
// CSP: the tile's columns are split over CSP waves per row group (TW = T / CSP columns each; wave
// w works on row groups w / CSP, w / CSP + NW / CSP, ... and the columns (w % CSP) * TW ...).  A
// matrix of 4096 rows is 2 row groups per CU on 256 CUs: unsplit, 2 of the 8 waves would run all
// T columns' chains; split by 4, all 8 run a quarter each (the weights then come 4 times out of
// the CU's cache, once out of memory).
template <int T, int CSP, int EPI, int KT, int NW>
__global__ __launch_bounds__(NW * 64) void k_mv_cols(ColsParams P) {
    constexpr int NT = NW * 64;
    constexpr int nb = KT / 32;
    constexpr int FC = nb / 32;                 // full chunks
    constexpr int TS = (nb % 32) / 8;           // 8-block sub-chunks of the partial last chunk
    constexpr int NC = FC + (TS ? 1 : 0);
    constexpr int CS16 = cols_stride16(KT);
    constexpr int CPT = (T * CS16 + NT - 1) / NT;       // table uint4 per thread
    constexpr int TW = T / CSP;                 // columns per wave
    constexpr int NWG = NW / CSP;               // row groups in flight per workgroup
    static_assert(nb % 8 == 0 && FC >= 2 && FC % 2 == 0, "row length");
    static_assert(TW >= 1 && TW * CSP == T && NWG * CSP == NW, "column split");

    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint4 * tab = (uint4 *) smem;                           // T * CS16
    float * sbuf = (float *) (tab + T * CS16);              // NW * 2 * SPL

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
    // a wave without row groups (it only copies the table) issues the ring's first loads with
    // every lane on one 16-byte word: no branch around the issue, exact wait counts
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

    uint4 W[2][4];
    float4 S[2];
    uint4 WT[TS ? TS : 1];
    float4 ST = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // scales first, then the chunk's nibbles; all streamed once per tile: nt loads
#define LVK_ISSUE(slot, grp, cc)                                                                        \
    do {                                                                                                \
        const size_t ch_ = (size_t) (grp) * NC + (cc);                                                  \
        S[slot] = ld_nt((const float4 *) ((const char *) (P.scl + ch_ * 64) + loff));                   \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb)                                                \
            W[slot][sb] = ld_nt((const uint4 *) ((const char *) (P.nib + (ch_ * 4 + sb) * 64) + loff)); \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)
#define LVK_ISSUE_TAIL(grp)                                                                             \
    do {                                                                                                \
        if constexpr (TS > 0) {                                                                         \
            const size_t ch_ = (size_t) (grp) * NC + FC;                                                \
            ST = ld_nt((const float4 *) ((const char *) (P.scl + ch_ * 64) + loff));                    \
            _Pragma("unroll") for (int sb = 0; sb < TS; ++sb)                                           \
                WT[sb] = ld_nt((const uint4 *) ((const char *) (P.nib + (ch_ * 4 + sb) * 64) + loff));  \
            __builtin_amdgcn_sched_barrier(0);                                                          \
        }                                                                                               \
    } while (0)

    const int ntiles = (P.ncols + T - 1) / T;
    // the weights are in flight under the table copy
    LVK_ISSUE(0, gfirst, 0);
    LVK_ISSUE(1, gfirst, 1);
    LVK_ISSUE_TAIL(gfirst);

    float * sw = sbuf + wave * 2 * SPL;
    float acc[TW];
    const uint4 * tabw = tab + sub * TW * CS16;      // this wave's columns

    // the chains of one chunk (NSB sub-chunks of 8 blocks) on the tile's columns.  wl / wh: the
    // chunk's weight words split into their low / high 16 bits (blocks 2k / 2k + 1 of a word's
    // pair); sc: the chunk's weight scales of this lane (blocks 8m + j)
    auto chunk = [&](auto nsb_c, const uint32_t (&wl)[4][4], const uint32_t (&wh)[4][4], const float4 & sc,
                     int c) __attribute__((always_inline)) {
        constexpr int NSB = decltype(nsb_c)::value;
        auto dx_of = [&](int tt) __attribute__((always_inline)) {
            return *(const float4 *) ((const float *) (tabw + tt * CS16 + nb) + c * 32 + j * 4);
        };
        // s = dw * dx (ggml.c:1968) of column tt into the ring slice tt & 1
        auto write_s = [&](int tt, const float4 & dx) __attribute__((always_inline)) {
            float4 sv;
            sv.x = sc.x * dx.x; sv.y = sc.y * dx.y; sv.z = sc.z * dx.z; sv.w = sc.w * dx.w;
            *(float4 *) (sw + (tt & 1) * SPL + r * SRS + j * 4) = sv;
        };
        float4 dxn = dx_of(0);
        write_s(0, dxn);
        if constexpr (TW > 1) dxn = dx_of(1);
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) {
            __builtin_amdgcn_wave_barrier();
            const float * sl = sw + (tt & 1) * SPL;
            uint4 A[NSB];
#pragma unroll
            for (int sb = 0; sb < NSB; ++sb) A[sb] = tabw[tt * CS16 + (c * 4 + sb) * 8 + j];
            float sa[8][4];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float4 v = *(const float4 *) (sl + r * SRS + jj * 4);
                sa[jj][0] = v.x; sa[jj][1] = v.y; sa[jj][2] = v.z; sa[jj][3] = v.w;
            }
            // the next column's slice goes out under this column's chains
            if (tt + 1 < TW) {
                write_s(tt + 1, dxn);
                if (tt + 2 < TW) dxn = dx_of(tt + 2);
            }
            float a = acc[tt];
#pragma unroll
            for (int sb = 0; sb < NSB; ++sb) {
                const uint32_t aw[4] = {A[sb].x, A[sb].y, A[sb].z, A[sb].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int bi = sb * 8 + 2 * k;          // block within the chunk
                    const int p0 = dot8(wl[sb][k], aw[k]);
                    const int p1 = dot8(wh[sb][k], aw[k]);
                    a = __builtin_fmaf(sa[(bi + 0) & 7][(bi + 0) >> 3], (float) p0, a);
                    a = __builtin_fmaf(sa[(bi + 1) & 7][(bi + 1) >> 3], (float) p1, a);
                }
            }
            // keep the columns in program order: the chain value is pinned here, so hipcc cannot
            // hoist every column's LDS reads above the first column's arithmetic
            asm volatile("" : "+v"(a));
            acc[tt] = a;
            __builtin_amdgcn_sched_barrier(0);
        }
    };
#define LVK_SPLIT(Wc, nsb)                                                                              \
    uint32_t wl[4][4], wh[4][4];                                                                        \
    _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                                  \
        const uint32_t wd_[4] = {Wc[sb < (nsb) ? sb : 0].x, Wc[sb < (nsb) ? sb : 0].y,                  \
                                 Wc[sb < (nsb) ? sb : 0].z, Wc[sb < (nsb) ? sb : 0].w};                 \
        _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                 \
            wl[sb][k] = wd_[k] & 0xFFFFu;                                                               \
            wh[sb][k] = wd_[k] & 0xFFFF0000u;                                                           \
        }                                                                                               \
    }

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
            // the residual terms ahead of the chunk loop for a few columns (mv_pre_epi); a wide
            // tile's row group runs long enough that its epilogue's round trip does not count
            [[maybe_unused]] float rv[TW];
            if constexpr (EPI == EPI_RESID && TW <= 4) {
#pragma unroll
                for (int tt = 0; tt < TW; ++tt)
                    rv[tt] = P.y[(size_t) min(t0 + sub * TW + tt, t0 + nt - 1) * P.M + gc * 8 + r];
            }
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) acc[tt] = 0.0f;
#pragma unroll 1
            for (int cp = 0; cp < FC / 2; ++cp) {
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int c = cp * 2 + d;
                    LVK_SPLIT(W[d], 4)
                    const float4 sc = S[d];
                    // refill the slot two chunks ahead: this row group's, or the next one's
                    const bool own = c + 2 < FC;
                    LVK_ISSUE(d, own ? gc : gn, own ? c + 2 : c + 2 - FC);
                    chunk(std::integral_constant<int, 4>{}, wl, wh, sc, c);
                }
            }
            if constexpr (TS > 0) {
                LVK_SPLIT(WT, TS)
                const float4 sc = ST;
                LVK_ISSUE_TAIL(gn);
                chunk(std::integral_constant<int, TS>{}, wl, wh, sc, FC);
            }
            // per column: the shared single-token epilogue on that column's outputs
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) {
                const float res = octet_reduce(acc[tt]);
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
#undef LVK_SPLIT
#undef LVK_TABLE_COPY
#undef LVK_ISSUE
#undef LVK_ISSUE_TAIL
}

// -- host -------------------------------------------------------------------

template <int T, int CSP, int EPI, int KT, int NW>
hipError_t go_t(const ColsParams & P, int nwg, hipStream_t s) {
    const size_t lds = (size_t) T * cols_stride16(KT) * 16 + (size_t) NW * 2 * SPL * 4;
    static_assert((size_t) T * cols_stride16(KT) * 16 + (size_t) NW * 2 * SPL * 4 <= 160 * 1024, "LDS");
    // more than the default 64 KiB of dynamic LDS: opted in per device and not stream-ordered, so
    // with every launch (as attention_rows.hip does)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *) k_mv_cols<T, CSP, EPI, KT, NW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    LVK_LAUNCH((k_mv_cols<T, CSP, EPI, KT, NW>), dim3(nwg), dim3(NW * 64), lds, s, P);
    return hipGetLastError();
}

// the column split of a tile of T: the one with the least chain work on the busiest wave.  A wave
// runs ceil(gpc / (NW / csp)) row groups of T / csp columns each (gpc: row groups per workgroup);
// a chunk costs about 0.4 of a column besides (the weight split, the ring's start)
template <int T, int EPI, int KT, int NW>
hipError_t go_split(const ColsParams & P, hipStream_t s) {
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

// the columns [col0, col0 + ncols) with the narrowest tile that holds them (16 from 9 on)
template <int EPI, int KT>
hipError_t go_cols(ColsParams P, int col0, int ncols, hipStream_t s) {
    P.col0 = col0; P.ncols = ncols;
    constexpr int NW = 8;
    if (ncols <= 2) return go_split<2, EPI, KT, NW>(P, s);
    if (ncols <= 4) return go_split<4, EPI, KT, NW>(P, s);
    if (ncols <= 8) return go_split<8, EPI, KT, NW>(P, s);
    return go_split<16, EPI, KT, NW>(P, s);
}

// a step of n columns: the whole tiles of 16 in one launch (tiled inside the workgroup), the
// rest in a second one with its own tile width
template <int EPI, int KT>
hipError_t go(const ColsParams & P, int n, hipStream_t s) {
    const int nfull = n > 16 ? n / 16 * 16 : n;
    if (nfull == n) return go_cols<EPI, KT>(P, 0, n, s);
    EventSplit ev;      // timed as one: the stop event goes to the second launch
    g_launch_events = {nullptr, nullptr};
    const hipError_t e = go_cols<EPI, KT>(P, 0, nfull, s);
    if (e != hipSuccess) return e;
    ev.last();
    return go_cols<EPI, KT>(P, nfull, n - nfull, s);
}

}  // namespace

// row lengths compiled in: n_embd and n_ff of LLaMA 7B; those of 13B, 30B and 65B go to
// matvec_cols_long.hip
bool matvec_cols_supported(int qtype, int K, int n) {
    return qtype == Q4_0 && (K == 4096 || K == 11008 || cols_long_supported(K)) && n >= 2;
}

hipError_t launch_matvec_cols(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    const int K = L.w.K, n = L.n_tokens;
    if (!matvec_cols_supported(L.w.qtype, K, n) || L.w.M % 8 || L.tok0 != 0) return hipErrorNotSupported;
    const bool pair = (pro == PRO_NORM && (epi == EPI_STORE || epi == EPI_SWIGLU_F32)) ||
                      ((pro == PRO_ACTQ || pro == PRO_ACTF) && epi == EPI_RESID);
    if (!pair || (K > 8192 && epi != EPI_RESID)) return hipErrorNotSupported;     // an n_ff: the W2 role only
    if (!mv_inputs_set(L, pro) || !L.cols_img || !L.w.nib || !L.w.scl) return hipErrorInvalidValue;
    if (epi == EPI_SWIGLU_F32 ? (!L.u || !L.silu_tab) : !L.y) return hipErrorInvalidValue;
    ColsParams P{};
    mv_fill(P, L, false);
    P.nib = L.w.nib;
    P.scl = (const float4 *) L.w.scl;
    P.img = (const uint4 *) L.cols_img;
    P.G = L.w.M / 8;
    P.M = L.w.M;
    // the step's rows, once, into the packed image; timed with the matmul as one launch
    EventSplit ev;
    ev.first();
    uint4 * img = (uint4 *) L.cols_img;
    switch (pro) {
        case PRO_NORM: LVK_LAUNCH((k_cols_act<PRO_NORM>), dim3(n), dim3(256), 0, s, L.x, L.g, L.xq, K, img); break;
        case PRO_ACTF: LVK_LAUNCH((k_cols_act<PRO_ACTF>), dim3(n), dim3(256), 0, s, L.x, L.g, L.xq, K, img); break;
        default: LVK_LAUNCH((k_cols_act<PRO_ACTQ>), dim3(n), dim3(256), 0, s, L.x, L.g, L.xq, K, img); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ev.last();
    if (cols_long_supported(K)) return launch_cols_long(P, K, epi, n, s);
    if (K == 4096) {
        switch (epi) {
            case EPI_STORE: return go<EPI_STORE, 4096>(P, n, s);
            case EPI_RESID: return go<EPI_RESID, 4096>(P, n, s);
            default: return go<EPI_SWIGLU_F32, 4096>(P, n, s);
        }
    }
    return go<EPI_RESID, 11008>(P, n, s);
}

size_t matvec_cols_image_bytes(int K, int n) { return (size_t) n * cols_stride16(K) * 16; }

}  // namespace lvk
