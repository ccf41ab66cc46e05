// matvec_cols_long.hip -- the CU-balanced Q4_0 matmul of a batched decode step (matvec_cols.hip) for
// row lengths with any number of chunks: n_embd / n_ff of LLaMA 13B (5120 / 13824), 30B (6656 /
// 17920) and 65B (8192 / 22016).
//
// Organisation, column table (the image k_cols_act writes), per-wave two-slice block-scale ring and
// result bits are matvec_cols.hip's: one workgroup per CU, a wave per row group, lane 8r + j = chain
// j of row r, the tile's columns split over CSP waves where a CU has few row groups; exact
// v_dot8_i32_i4 partials, fmaf(dw * dx, P, acc) in block order per chain, the octet reduce.  That
// kernel is unrolled over a compile-time, even number of full chunks; these row lengths have 5, 13,
// 17 and 21 full chunks (odd) or 6 and 8, four of the six end in a 16-block partial chunk, and the
// longest is 21.5 chunks of code if unrolled.  What is new here:
//
//   * the row length is a kernel argument (blocks, chunks, column stride): one kernel per (tile,
//     split, epilogue), whose code does not grow with K;
//   * the weight ring over a chunk stream.  A wave's work in a tile is the stream of its chunks,
//     row group after row group; the loop takes two stream positions per trip, the even one through
//     register slot 0 and the odd one through slot 1, so the slots are named statically and each
//     wait leaves exactly the other slot's five loads in flight.  First and last chunk of a row
//     group are uniform branches in the one body (zero the chains / the epilogue), the partial last
//     chunk a sub-chunk count (its missing sub-chunks are loaded from its first one: the same
//     cache lines, never used).  A stream of odd length is padded with one position that is
//     fetched (the wave's first chunk, which the next tile reads anyway) and not computed, so every
//     tile starts on slot 0 and the ring runs on across row groups and tiles: two positions ahead,
//     as in matvec_cols.hip;
//   * the tile is what fits 160 KiB of LDS beside the 20 KiB of scale slices: 16 columns up to
//     K = 13824 (159 744 B), 12 of 17920, 10 of 22016 (splits 1 / 2 / 4 and 1 / 2);
//   * the table copy is a loop of 4 uint4 per thread and trip, not a register image of the tile.
// No workgroup waits on another: plain vector loads and stores only.
#include <cstdlib>
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"
#include "matvec_cols_common.h"

namespace lvk {

namespace {
using namespace mv;
using namespace cols;

struct LongParams : ColsParams {
    int nb;                     // blocks of a row (K / 32), a multiple of 8
    int NC;                     // chunks of 32 blocks, the last one partial when nb % 32
    int CS16;                   // cols_stride16(K): a column of the image / table in uint4
};

// T columns per tile, NW waves; CSP as in matvec_cols.hip: wave w works on row groups w / CSP,
// w / CSP + NW / CSP, ... and the columns (w % CSP) * TW ...
template <int T, int CSP, int EPI, int NW>
__global__ __launch_bounds__(NW * 64) void k_mv_cols_long(LongParams P) {
    constexpr int NT = NW * 64;
    constexpr int TW = T / CSP;                 // columns per wave
    constexpr int NWG = NW / CSP;               // row groups in flight per workgroup
    static_assert(TW >= 1 && TW * CSP == T && NWG * CSP == NW, "column split");
    const int nb = P.nb, NC = P.NC, CS16 = P.CS16;
    const int nsub = nb >> 3;                   // 8-block sub-chunks of a row

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

    // the ring: scales first, then the chunk's nibbles; all streamed once per tile: nt loads
    uint4 W[2][4];
    float4 S[2];
#define LVK_ISSUE(slot, grp, cc)                                                                        \
    do {                                                                                                \
        const size_t ch_ = (size_t) (grp) * NC + (cc);                                                  \
        S[slot] = ld_nt((const float4 *) ((const char *) (P.scl + ch_ * 64) + loff));                   \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                              \
            const int sq_ = (cc) * 4 + sb < nsub ? sb : 0;                                              \
            W[slot][sb] = ld_nt((const uint4 *) ((const char *) (P.nib + (ch_ * 4 + sq_) * 64) + loff)); \
        }                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)

    // the wave's chunk stream of a tile: ng * NC positions, row group after row group, and one
    // padding position when that is odd.  (fk, fc): the position the ring fetches next, row group
    // fk of the wave (fk == ng: the padding), chunk fc
    const int npos = ng * NC;
    const bool odd = (npos & 1) != 0;
    int fk = 0, fc = 2;
#define LVK_FETCH_ADVANCE()                                                                             \
    do {                                                                                                \
        if (fk == ng) { fk = 0; fc = 0; }                                                               \
        else if (++fc == NC) { fc = 0; ++fk; if (fk == ng && !odd) fk = 0; }                            \
    } while (0)
    // the weights are in flight under the first table copy
    LVK_ISSUE(0, gfirst, 0);
    LVK_ISSUE(1, gfirst, 1);

    float * sw = sbuf + wave * 2 * SPL;
    const uint4 * tabw = tab + sub * TW * CS16;      // this wave's columns
    float acc[TW];
    [[maybe_unused]] float rv[TW];
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) { acc[tt] = 0.0f; rv[tt] = 0.0f; }

    // the chains of chunk c (nsb sub-chunks of 8 blocks) on the wave's columns.  wl / wh: the
    // chunk's weight words split into their low / high 16 bits (blocks 2k / 2k + 1 of a word's
    // pair); sc: the chunk's weight scales of this lane (blocks 8m + j)
    auto chunk = [&](int nsb, const uint32_t (&wl)[4][4], const uint32_t (&wh)[4][4], const float4 & sc,
                     int c) __attribute__((always_inline)) {
        const float * dxb = (const float *) (tabw + nb) + c * 32 + j * 4;
        const uint4 * nbp = tabw + c * 32 + j;
        auto dx_of = [&](int tt) __attribute__((always_inline)) { return *(const float4 *) (dxb + tt * CS16 * 4); };
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
            // the partial chunk's missing sub-chunks read the column's dx words: in the table, unused
            uint4 A[4];
#pragma unroll
            for (int sb = 0; sb < 4; ++sb) A[sb] = nbp[tt * CS16 + sb * 8];
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
            for (int sb = 0; sb < 4; ++sb) {
                if (sb < nsb) {
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
            }
            // keep the columns in program order: the chain value is pinned here, so hipcc cannot
            // hoist every column's LDS reads above the first column's arithmetic
            asm volatile("" : "+v"(a));
            acc[tt] = a;
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    const int ntiles = (P.ncols + T - 1) / T;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int t0 = P.col0 + tile * T;
        const int nt = min(T, P.col0 + P.ncols - t0);
        // the tile's columns: a straight copy of the image.  The barrier ahead of the stores: every
        // wave is done with the previous tile's table
        {
            const u32x4 * src = (const u32x4 *) P.img + (size_t) t0 * CS16;
            const int cnt = nt * CS16;
            if (tile > 0) __syncthreads();
#pragma unroll 1
            for (int b = tid; b < cnt; b += 4 * NT) {
                u32x4 tv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) tv[k] = src[min(b + k * NT, cnt - 1)];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (b + k * NT < cnt) ((u32x4 *) tab)[b + k * NT] = tv[k];
            }
            __syncthreads();
        }
        if (ng == 0) continue;
        int kg = 0, c = 0, gc = gfirst;         // the position consumed: row group kg of the wave (gc), chunk c
        // one stream position through ring slot d
#define LVK_POSITION(d)                                                                                 \
        {                                                                                               \
            const bool live = kg < ng;                                                                  \
            if (live && c == 0) {                                                                       \
                /* the residual terms ahead of the chunk loop for a few columns (mv_pre_epi) */         \
                if constexpr (EPI == EPI_RESID && TW <= 4) {                                            \
                    _Pragma("unroll") for (int tt = 0; tt < TW; ++tt)                                   \
                        rv[tt] = P.y[(size_t) min(t0 + sub * TW + tt, t0 + nt - 1) * P.M + gc * 8 + r]; \
                }                                                                                       \
                _Pragma("unroll") for (int tt = 0; tt < TW; ++tt) acc[tt] = 0.0f;                       \
            }                                                                                           \
            uint32_t wl[4][4], wh[4][4];                                                                \
            _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                          \
                const uint32_t wd_[4] = {W[d][sb].x, W[d][sb].y, W[d][sb].z, W[d][sb].w};               \
                _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                         \
                    wl[sb][k] = wd_[k] & 0xFFFFu;                                                       \
                    wh[sb][k] = wd_[k] & 0xFFFF0000u;                                                   \
                }                                                                                       \
            }                                                                                           \
            /* the scales move to registers of their own (early clobber): left in the slot's, the      \
               refill would land elsewhere and be copied back at the loop's end, behind a full wait */  \
            float4 sc;                                                                                  \
            asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"                  \
                         : "=&v"(sc.x), "=&v"(sc.y), "=&v"(sc.z), "=&v"(sc.w)                             \
                         : "v"(S[d].x), "v"(S[d].y), "v"(S[d].z), "v"(S[d].w));                         \
            /* the working set is pinned ahead of the refill: sunk below it, the split would keep the   \
               slot's old registers live and the ring would turn into copies */                         \
            _Pragma("unroll") for (int sb = 0; sb < 4; ++sb)                                            \
                _Pragma("unroll") for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(wl[sb][k]), "+v"(wh[sb][k])); \
            /* refill the slot two positions ahead: this tile's, or the next one's (after the last    \
               tile redundant, valid loads) */                                                          \
            LVK_ISSUE(d, fk == ng ? gfirst : gfirst + fk * NWG, fc);                                    \
            LVK_FETCH_ADVANCE();                                                                        \
            if (live) {                                                                                 \
                const bool last = c == NC - 1;                                                          \
                chunk(last ? nsub - c * 4 : 4, wl, wh, sc, c);                                          \
                ++c;                                                                                    \
                if (last) {                                                                             \
                    /* per column: the shared single-token epilogue on that column's outputs */        \
                    _Pragma("unroll") for (int tt = 0; tt < TW; ++tt) {                                 \
                        const float res = octet_reduce(acc[tt]);                                        \
                        const int ct = sub * TW + tt;           /* column within the tile */            \
                        if (ct < nt) {                                                                  \
                            MvArgs A = P;                                                               \
                            A.y = P.y + (size_t) (t0 + ct) * P.M;                                       \
                            A.u = P.u + (size_t) (t0 + ct) * (P.M / 2);                                 \
                            EpiPre pe{make_float2(0.0f, 0.0f), 0.0f};                                   \
                            if constexpr (EPI == EPI_RESID) {                                           \
                                if constexpr (TW <= 4) pe.rv = rv[tt];                                  \
                                else pe.rv = A.y[gc * 8 + r];                                           \
                            }                                                                           \
                            mv_epilogue<EPI>(A, gc, r, j, res, 0, pe);                                  \
                        }                                                                               \
                    }                                                                                   \
                    c = 0; ++kg; gc += NWG;                                                             \
                }                                                                                       \
            }                                                                                           \
        }
#pragma unroll 1
        for (int i = 0; i < npos; i += 2) {
            LVK_POSITION(0)
            LVK_POSITION(1)
        }
#undef LVK_POSITION
    }
#undef LVK_FETCH_ADVANCE
#undef LVK_ISSUE
}

// -- host -------------------------------------------------------------------

constexpr size_t LDS_MAX = 160 * 1024;
constexpr int NW = 8;
constexpr size_t lds_bytes(int T, int K) { return (size_t) T * cols_stride16(K) * 16 + (size_t) NW * 2 * SPL * 4; }
static_assert(lds_bytes(16, 13824) <= LDS_MAX && lds_bytes(12, 17920) <= LDS_MAX && lds_bytes(10, 22016) <= LDS_MAX, "LDS");

// the widest tile of a row length: what fits the LDS beside the scale slices.  LVK_COLS_LONG_T8=1
// (read once per process) keeps K = 17920 / 22016 on the tile of 8: the A/B leg of
// profiles/rows_cols_long_speed.json
int tile_max(int K) {
    static const bool t8 = [] { const char * e = getenv("LVK_COLS_LONG_T8"); return e && atoi(e) != 0; }();
    if (K <= 13824) return 16;
    if (t8) return 8;
    return K == 17920 ? 12 : 10;
}

template <int T, int CSP, int EPI>
hipError_t go_t(const LongParams & P, int nwg, hipStream_t s) {
    const size_t lds = (size_t) T * P.CS16 * 16 + (size_t) NW * 2 * SPL * 4;
    if (lds > LDS_MAX) return hipErrorNotSupported;
    // more than the default 64 KiB of dynamic LDS: opted in per device and not stream-ordered, so
    // with every launch (as matvec_cols.hip does)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *) k_mv_cols_long<T, CSP, EPI, NW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    LVK_LAUNCH((k_mv_cols_long<T, CSP, EPI, NW>), dim3(nwg), dim3(NW * 64), lds, s, P);
    return hipGetLastError();
}

// the column split of a tile of T that divides it, by matvec_cols.hip's cost: the least chain work
// on the busiest wave, a chunk's fixed part at 0.4 of a column
template <int T, int EPI>
hipError_t go_split(const LongParams & P, hipStream_t s) {
    const int nwg = std::min(cu_count(), P.G);
    const int gpc = (P.G + nwg - 1) / nwg;
    int best = 1;
    float cost = 0.0f;
    for (int csp = 1; csp <= 4 && T % csp == 0; csp *= 2) {
        const int rounds = (gpc + NW / csp - 1) / (NW / csp);
        const float c = (float) rounds * ((float) (T / csp) + 0.4f);
        if (csp == 1 || c < cost) { best = csp; cost = c; }
    }
    if constexpr (T % 4 == 0)
        if (best == 4) return go_t<T, 4, EPI>(P, nwg, s);
    if (best >= 2) return go_t<T, 2, EPI>(P, nwg, s);
    return go_t<T, 1, EPI>(P, nwg, s);
}

// the columns [col0, col0 + ncols) with the narrowest tile that holds them, up to the row length's
// widest (tm); the tiles of 10 and 12 exist for the n_ff lengths, which take EPI_RESID only
template <int EPI>
hipError_t go_cols(LongParams P, int col0, int ncols, int tm, hipStream_t s) {
    P.col0 = col0; P.ncols = ncols;
    if (ncols <= 2) return go_split<2, EPI>(P, s);
    if (ncols <= 4) return go_split<4, EPI>(P, s);
    if (ncols <= 8 || tm == 8) return go_split<8, EPI>(P, s);
    if constexpr (EPI == EPI_RESID) {
        if (tm == 10) return go_split<10, EPI>(P, s);
        if (tm == 12) return go_split<12, EPI>(P, s);
    }
    return tm == 16 ? go_split<16, EPI>(P, s) : hipErrorNotSupported;
}

// a step of n columns: the whole widest tiles in one launch (tiled inside the workgroup), the
// rest in a second one with its own tile width
template <int EPI>
hipError_t go(const LongParams & P, int n, int tm, hipStream_t s) {
    const int nfull = n > tm ? n / tm * tm : n;
    if (nfull == n) return go_cols<EPI>(P, 0, n, tm, s);
    EventSplit ev;      // timed as one: the stop event goes to the second launch
    g_launch_events = {nullptr, nullptr};
    const hipError_t e = go_cols<EPI>(P, 0, nfull, tm, s);
    if (e != hipSuccess) return e;
    ev.last();
    return go_cols<EPI>(P, nfull, n - nfull, tm, s);
}

}  // namespace

namespace cols {

// n_embd / n_ff of LLaMA 13B, 30B and 65B
bool cols_long_supported(int K) {
    return K == 5120 || K == 13824 || K == 6656 || K == 17920 || K == 8192 || K == 22016;
}

hipError_t launch_cols_long(const ColsParams & P0, int K, int epi, int n, hipStream_t s) {
    if (!cols_long_supported(K) || n < 2) return hipErrorNotSupported;
    LongParams P{};
    static_cast<ColsParams &>(P) = P0;
    P.nb = K / 32;
    P.NC = (P.nb + 31) / 32;
    P.CS16 = cols_stride16(K);
    const int tm = tile_max(K);
    switch (epi) {
        case EPI_STORE: return go<EPI_STORE>(P, n, tm, s);
        case EPI_RESID: return go<EPI_RESID>(P, n, tm, s);
        case EPI_SWIGLU_F32: return go<EPI_SWIGLU_F32>(P, n, tm, s);
    }
    return hipErrorNotSupported;
}

}  // namespace cols

}  // namespace lvk
