// matvec_cu_long.hip -- the CU-balanced single-token Q4_0 matvec (matvec_cu.hip) for the row lengths of
// LLaMA 13B (n_embd 5120, n_ff 13824) and 30B (6656, 17920): 5, 7, 14 and 18 chunks, three of them
// ending in a 16-block chunk.  The kernel's text, the role table and the launcher are the chunk stream of
// matvec_cu_stream.h; this file is its Q4_0 format: k_mv_cu's arithmetic (exact v_dot8_i32_i4 partials,
// fmaf(dw * dx, P, acc) in block order per chain against the per-wave s = dw * dx table in LDS) on the
// two weight images k_mv_cu reads, five nt loads per position.
#include "matvec_common.h"

namespace lvk {
namespace {
struct Q40Stream {
    using Params = mv::CuParams;
    static constexpr int QTYPE = Q4_0;
    static constexpr int KE0 = 5120, KE1 = 6656, KF0 = 13824, KF1 = 17920;
    // waves: QKV 8 (13B) / 12 (30B), W1|W3 and lm_head 16
    static constexpr int nw_qkv(int KE) { return KE == 5120 ? 8 : 12; }
    static constexpr int NW_WIDE = 16;
    static constexpr size_t LDS_MAX = 64 * 1024;
    // the activation table, two s-table buffers per wave, one double per wave: LVK_STREAM_CARVE
    static constexpr size_t lds_bytes(int K, int NW) {
        return (size_t) K + (size_t) ((K / 32 + 31) / 32) * 128 + (size_t) NW * 2 * mv::cu_lds::SPL * 4 + (size_t) NW * 8;
    }
};
}  // namespace
}  // namespace lvk

#define LVK_STREAM_KERNEL k_mv_cu_long
#define LVK_STREAM_FORMAT Q40Stream
#define LVK_STREAM_CARVE                                                                                \
    uint32_t * act = (uint32_t *) smem;                          /* nb * 32 B */                        \
    float * dxp = (float *) (smem + nb * 32);                    /* NC * 128 B */                       \
    float * sbuf = dxp + NC * 32;                                /* NW * 2 * SPL floats */              \
    double * red = (double *) (sbuf + NW * 2 * SPL);             /* NW doubles */
#define LVK_STREAM_STAGED(n) [[maybe_unused]] uint4 qv[n]; [[maybe_unused]] float dv[n];
#define LVK_STREAM_STAGED_LOAD(k, b) qv[k] = P.xq.qs[b]; dv[k] = P.xq.d[b];
#define LVK_STREAM_STAGED_LAND(k) launder(qv[k]); launder(dv[k]);
#define LVK_STREAM_STORE_BLOCK(k, b) q40_block_store(act, dxp, b, qv[k], dv[k])
#define LVK_STREAM_QUANTIZE pro_q40_units<NT, PRO>(xv, gv, scale, nunits, tid, act, dxp)
// the ring: the scales of a position go out before its nibbles.  lo: the lane's byte offset (0: the whole
// wave on one 16-byte word)
#define LVK_STREAM_RING uint4 W[2][4]; float4 S[2];
#define LVK_STREAM_ISSUE(slot, grp, cc, lo)                                                             \
    do {                                                                                                \
        const size_t ch_ = (size_t) (grp) * NC + (cc);                                                  \
        S[slot] = ld_nt((const float4 *) ((const char *) (P.scl + ch_ * 64) + (lo)));                   \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                              \
            const int sq_ = (cc) * 4 + sb < nsub ? sb : 0;                                              \
            W[slot][sb] = ld_nt((const uint4 *) ((const char *) (P.nib + (ch_ * 4 + sq_) * 64) + (lo))); \
        }                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)
// s = dw * dx (ggml.c:1968); chain8: the 8 blocks of sub-chunk sb on the chain
#define LVK_STREAM_TABLES                                                                               \
    float * sw = sbuf + wave * 2 * SPL;                                                                 \
    auto make_table = [&](int buf, const float4 & Sv, int cc) __attribute__((always_inline)) {          \
        const float4 dx = *(const float4 *) (dxp + cc * 32 + j * 4);                                    \
        float4 sv;                                                                                      \
        sv.x = Sv.x * dx.x; sv.y = Sv.y * dx.y; sv.z = Sv.z * dx.z; sv.w = Sv.w * dx.w;                 \
        *(float4 *) (sw + buf * SPL + r * SRS + j * 4) = sv;                                            \
    };                                                                                                  \
    auto chain8 = [&](float acc, const uint4 & w, const uint4 & a0, const uint4 & a1, const float (&sa)[8][4], \
                      int sb) __attribute__((always_inline)) {                                          \
        const uint32_t wd[4] = {w.x, w.y, w.z, w.w};                                                    \
        _Pragma("unroll") for (int pp = 0; pp < 2; ++pp) {                                              \
            const int bi = sb * 8 + pp * 4;                                                             \
            const uint4 a = pp ? a1 : a0;                                                               \
            const int p0 = dot8(wd[2 * pp], a.x);                                                       \
            const int p1 = dot8(wd[2 * pp], a.y);                                                       \
            const int p2 = dot8(wd[2 * pp + 1], a.z);                                                   \
            const int p3 = dot8(wd[2 * pp + 1], a.w);                                                   \
            acc = __builtin_fmaf(sa[(bi + 0) & 7][(bi + 0) >> 3], (float) p0, acc);                     \
            acc = __builtin_fmaf(sa[(bi + 1) & 7][(bi + 1) >> 3], (float) p1, acc);                     \
            acc = __builtin_fmaf(sa[(bi + 2) & 7][(bi + 2) >> 3], (float) p2, acc);                     \
            acc = __builtin_fmaf(sa[(bi + 3) & 7][(bi + 3) >> 3], (float) p3, acc);                     \
        }                                                                                               \
        return acc;                                                                                     \
    };
#define LVK_STREAM_MAKE_TABLE(buf, slot, cc) make_table(buf, S[slot], cc)
#define LVK_STREAM_CHAIN float acc = 0.0f;
#define LVK_STREAM_CHAIN8
#define LVK_STREAM_ZERO acc = 0.0f;
// the chunk's activation words and scale products are read from LDS up front (one exposed LDS latency per
// chunk); the partial chunk's missing sub-chunks read the dx table: in LDS, never used
#define LVK_STREAM_CHUNK(d)                                                                             \
    const float * sl = sw + tbuf * SPL;                                                                 \
    uint4 A[8];                                                                                         \
    _Pragma("unroll") for (int q = 0; q < 8; ++q) A[q] = *(const uint4 *) (act + ((c * 8 + q) * 8 + j) * 4); \
    float sa[8][4];                                                                                     \
    _Pragma("unroll") for (int jj = 0; jj < 8; ++jj) {                                                  \
        const float4 v = *(const float4 *) (sl + r * SRS + jj * 4);                                     \
        sa[jj][0] = v.x; sa[jj][1] = v.y; sa[jj][2] = v.z; sa[jj][3] = v.w;                             \
    }                                                                                                   \
    acc = chain8(acc, W[d][0], A[0], A[1], sa, 0);                                                      \
    acc = chain8(acc, W[d][1], A[2], A[3], sa, 1);                                                      \
    if (TSUB == 4 || c + 1 < NC) {                                                                      \
        acc = chain8(acc, W[d][2], A[4], A[5], sa, 2);                                                  \
        acc = chain8(acc, W[d][3], A[6], A[7], sa, 3);                                                  \
    }
#define LVK_STREAM_RESULT octet_reduce(acc)
#define LVK_STREAM_PIN asm volatile("" : "+v"(acc));
#include "matvec_cu_stream.h"

namespace lvk {

bool matvec_cu_long_supported(int K) { return stream_supported<Q40Stream>(K); }

hipError_t launch_matvec_cu_long(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    return stream_launch<Q40Stream>(L, pro, epi, s);
}

}  // namespace lvk
