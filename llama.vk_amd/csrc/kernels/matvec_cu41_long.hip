// matvec_cu41_long.hip -- the CU-balanced single-token Q4_1 matvec (matvec_cu41.hip) for the row lengths
// of LLaMA 30B (n_embd 6656, n_ff 17920) and 65B (8192, 22016): 7, 8, 18 and 22 chunks, all but 8192
// ending in a 16-block chunk.  The kernel's text, the role table and the launcher are the chunk stream of
// matvec_cu_stream.h; this file is its Q4_1 format: k_mv_cu41's arithmetic, per block in order
//     acc = fmaf(dx*dy, p, acc)                          p: exact v_dot8_u32_u4 partial
//     acc = fmaf(j even ? dx*my : mx*dy, S, acc)         S: weight sums (even j) / activation sums
//     off = off + mx*my
//   result = octet_reduce(acc) + off * 32
// (ggml_vec_dot_q4_1's AVX2 form, ggml.c:2188-2258), on the three weight images k_mv_cu41 reads (nib,
// scl = d | m, q41_wsum) and the activation table act, dyv, myv and the activation-sum bytes ys, seven nt
// loads per position.
//
// The four product tables (s = dx*dy, dx*my, mx*dy, mx*my) are two buffers of 10 KiB per wave.  LDS per
// launch: K bytes of act, K / 8 of ys, 256 B of dyv | myv per chunk, the buffers and one double per
// wave: 49 / 89 KiB (6656, 4 / 8 waves), 51 / 91 KiB (8192), 104 KiB (17920), 110 KiB (22016).  Every
// role fits with two buffers at the wave count it wants, so none is single-buffered; launches above
// 64 KiB raise the kernel's dynamic LDS limit.
#include "matvec_common.h"

namespace lvk {
namespace {
struct Q41Stream {
    using Params = mv::Cu41Params;
    static constexpr int QTYPE = Q4_1;
    static constexpr int KE0 = 6656, KE1 = 8192, KF0 = 17920, KF1 = 22016;
    // waves: 8 (112 KB in flight) wherever a CU has the row groups for them
    static constexpr int nw_qkv(int) { return 8; }
    static constexpr int NW_WIDE = 8;
    static constexpr size_t LDS_MAX = 160 * 1024;
    // the activation table, two buffers of the four product tables per wave, one double per wave:
    // LVK_STREAM_CARVE
    static constexpr size_t lds_bytes(int K, int NW) {
        return (size_t) K + (size_t) ((K / 32 + 31) / 32) * 256 + (size_t) K / 8 + (size_t) NW * 2 * mv::cu_lds::SWF * 4 +
               (size_t) NW * 8;
    }
};
}  // namespace
}  // namespace lvk

#define LVK_STREAM_KERNEL k_mv_cu41_long
#define LVK_STREAM_FORMAT Q41Stream
#define LVK_STREAM_CARVE                                                                                \
    uint32_t * act = (uint32_t *) smem;                          /* nb * 32 B */                        \
    float * dyv = (float *) (smem + nb * 32);                    /* NC * 32 */                          \
    float * myv = dyv + NC * 32;                                 /* NC * 32 */                          \
    uint8_t * ys = (uint8_t *) (myv + NC * 32);                  /* nb * 4 bytes: activation sums */    \
    float * sbuf = (float *) (ys + nb * 4);                      /* NW * 2 * SWF */                     \
    double * red = (double *) (sbuf + NW * 2 * SWF);             /* NW */
#define LVK_STREAM_STAGED(n) [[maybe_unused]] uint4 qv[n]; [[maybe_unused]] float dv[n], mv_[n];
#define LVK_STREAM_STAGED_LOAD(k, b) qv[k] = P.xq.qs[b]; dv[k] = P.xq.d[b]; mv_[k] = P.xq.m[b];
#define LVK_STREAM_STAGED_LAND(k) launder(qv[k]); launder(dv[k]); launder(mv_[k]);
#define LVK_STREAM_STORE_BLOCK(k, b) q41_block_store(act, dyv, myv, ys, b, qv[k], dv[k], mv_[k])
#define LVK_STREAM_QUANTIZE pro_q41_units<NT, PRO>(xv, gv, scale, nunits, tid, act, dyv, myv, ys)
// the ring.  Per chunk cc of row group grp the images hold d | m [2][1 KiB], wsum [1 KiB] and
// nib [4 sub][1 KiB]; a lane's slice of each 1 KiB is its 16 bytes.  d, m and the weight sums of a
// position go out before its nibbles.  lo: the lane's byte offset (0: the whole wave on one 16-byte word)
#define LVK_STREAM_RING uint4 W[2][4], WS[2]; float4 SD[2], SM[2];
#define LVK_STREAM_ISSUE(slot, grp, cc, lo)                                                             \
    do {                                                                                                \
        const size_t ch_ = (size_t) (grp) * NC + (cc);                                                  \
        const char * sc_ = (const char *) P.scl + ch_ * 2048 + (lo);                                    \
        SD[slot] = ld_nt((const float4 *) sc_);                                                         \
        SM[slot] = ld_nt((const float4 *) (sc_ + 1024));                                                \
        WS[slot] = ld_nt((const uint4 *) ((const char *) P.wsum + ch_ * 1024 + (lo)));                  \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                              \
            const int sq_ = (cc) * 4 + sb < nsub ? sb : 0;                                              \
            W[slot][sb] = ld_nt((const uint4 *) ((const char *) P.nib + (ch_ * 4 + sq_) * 1024 + (lo))); \
        }                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)
// ggml.c:2205-2212: slot 8m + j of a table = block 32c + 8m + j of the lane's row.  A tail chunk's slots
// 16..31 multiply dyv / myv words no block wrote: stored, never read
#define LVK_STREAM_TABLES                                                                               \
    const bool even = (j & 1) == 0;                                                                     \
    const uint32_t * ys32 = (const uint32_t *) ys;                                                      \
    float * sw = sbuf + wave * 2 * SWF;                                                                 \
    auto make_table = [&](int buf, const float4 & dxv, const float4 & mxv, int cc) __attribute__((always_inline)) { \
        const float4 dy = *(const float4 *) (dyv + cc * 32 + j * 4);                                    \
        const float4 my = *(const float4 *) (myv + cc * 32 + j * 4);                                    \
        float * sl = sw + buf * SWF + r * SRS + j;                                                      \
        const float dxa[4] = {dxv.x, dxv.y, dxv.z, dxv.w};                                              \
        const float mxa[4] = {mxv.x, mxv.y, mxv.z, mxv.w};                                              \
        const float dya[4] = {dy.x, dy.y, dy.z, dy.w};                                                  \
        const float mya[4] = {my.x, my.y, my.z, my.w};                                                  \
        _Pragma("unroll") for (int mq = 0; mq < 4; ++mq) {                                              \
            sl[mq * 8] = dxa[mq] * dya[mq];                                                             \
            sl[SPL + mq * 8] = dxa[mq] * mya[mq];                                                       \
            sl[2 * SPL + mq * 8] = mxa[mq] * dya[mq];                                                   \
            sl[3 * SPL + mq * 8] = mxa[mq] * mya[mq];                                                   \
        }                                                                                               \
    };
#define LVK_STREAM_MAKE_TABLE(buf, slot, cc) make_table(buf, SD[slot], SM[slot], cc)
#define LVK_STREAM_CHAIN float acc = 0.0f, off = 0.0f;
// the 8 blocks of sub-chunk sb on the chain, read from LDS as they are used.  wsw: the even chains' sums
// of these blocks (one byte per block, exact as floats); odd chains take the activation sums from LDS
// (ggml.c:2236-2240)
#define LVK_STREAM_CHAIN8                                                                               \
    auto chain8 = [&](const uint4 & w, int sb, uint32_t ws0, uint32_t ws1) __attribute__((always_inline)) { \
        const float * srow = sw + tbuf * SWF + r * SRS;                                                 \
        const float * xrow = srow + (even ? SPL : 2 * SPL);                                             \
        const float * mrow = srow + 3 * SPL;                                                            \
        const uint32_t wd[4] = {w.x, w.y, w.z, w.w};                                                    \
        _Pragma("unroll") for (int pp = 0; pp < 2; ++pp) {                                              \
            const int uu = c * 8 + sb * 2 + pp;             /* group of 4 blocks */                     \
            const int bi = sb * 8 + pp * 4;                 /* first block within the chunk */          \
            const uint4 a = *(const uint4 *) (act + ((size_t) uu * 8 + j) * 4);                         \
            const float4 s4 = *(const float4 *) (srow + bi);                                            \
            const float4 x4 = *(const float4 *) (xrow + bi);                                            \
            const float4 m4 = *(const float4 *) (mrow + bi);                                            \
            const uint32_t ydw = ys32[(size_t) uu * 4 + (j >> 1)];                                      \
            const uint32_t sdw = even ? (pp ? ws1 : ws0) : ydw;                                         \
            const float S[4] = {(float) (sdw & 0xFFu), (float) ((sdw >> 8) & 0xFFu), (float) ((sdw >> 16) & 0xFFu), \
                                (float) (sdw >> 24)};                                                   \
            const int p[4] = {udot8(wd[2 * pp], a.x), udot8(wd[2 * pp], a.y), udot8(wd[2 * pp + 1], a.z), \
                              udot8(wd[2 * pp + 1], a.w)};                                              \
            const float sv[4] = {s4.x, s4.y, s4.z, s4.w};                                               \
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w};                                               \
            const float ms[4] = {m4.x, m4.y, m4.z, m4.w};                                               \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                             \
                acc = __builtin_fmaf(sv[k], (float) p[k], acc);                                         \
                acc = __builtin_fmaf(xs[k], S[k], acc);                                                 \
                off = off + ms[k];                                                                      \
            }                                                                                           \
        }                                                                                               \
    };
#define LVK_STREAM_ZERO acc = 0.0f; off = 0.0f;
// blocks 0-15 of the chunk have their weight sums in the lane's own word, 16-31 in the odd neighbour's
// (DPP quad_perm [1,1,3,3]); a 16-block tail chunk ends before those and skips them
#define LVK_STREAM_CHUNK(d)                                                                             \
    const uint4 ws = WS[d];                                                                             \
    chain8(W[d][0], 0, ws.x, ws.y);                                                                     \
    chain8(W[d][1], 1, ws.z, ws.w);                                                                     \
    if (TSUB == 4 || c + 1 < NC) {                                                                      \
        const uint32_t n0 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.x, 0xF5, 0xF, 0xF, false);     \
        const uint32_t n1 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.y, 0xF5, 0xF, 0xF, false);     \
        const uint32_t n2 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.z, 0xF5, 0xF, 0xF, false);     \
        const uint32_t n3 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.w, 0xF5, 0xF, 0xF, false);     \
        chain8(W[d][2], 2, n0, n1);                                                                     \
        chain8(W[d][3], 3, n2, n3);                                                                     \
    }
// res = hsum(acc) + acc_offset * QK (ggml.c:2249)
#define LVK_STREAM_RESULT octet_reduce(acc) + off * 32.0f
// the table buffer is rewritten by the next position: a second wave barrier after the pin
#define LVK_STREAM_PIN asm volatile("" : "+v"(acc), "+v"(off)); __builtin_amdgcn_wave_barrier();
#include "matvec_cu_stream.h"

namespace lvk {

bool matvec_cu41_long_supported(int K) { return stream_supported<Q41Stream>(K); }

hipError_t launch_matvec_cu41_long(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    return stream_launch<Q41Stream>(L, pro, epi, s);
}

}  // namespace lvk
