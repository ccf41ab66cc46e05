// matvec_cu41_long.hip -- the CU-balanced single-token Q4_1 matvec (matvec_cu41.hip) for the row lengths
// of LLaMA 30B (n_embd 6656, n_ff 17920) and 65B (8192, 22016).
//
// Organisation and result bits are k_mv_cu41's: one workgroup per CU, workgroup w owns the row groups
// [w * G / n, (w + 1) * G / n), the activation table (act, dyv, myv and the activation-sum bytes ys:
// RMSNorm + quantize_row_q4_1, a plain quantize, or a quantized input unpacked) is built once per
// workgroup in LDS, lane 8r + j is chain j of row r, and per block in order
//     acc = fmaf(dx*dy, p, acc)                          p: exact v_dot8_u32_u4 partial
//     acc = fmaf(j even ? dx*my : mx*dy, S, acc)         S: weight sums (even j) / activation sums
//     off = off + mx*my
//   result = octet_reduce(acc) + off * 32
// (ggml_vec_dot_q4_1's AVX2 form, ggml.c:2188-2258), on the three weight images k_mv_cu41 reads (nib,
// scl = d | m, q41_wsum), with the shared epilogues.
//
// k_mv_cu41 is unrolled over the whole row and prefetches across row groups only when its depth
// divides the chunk count.  These rows have 7, 8, 18 and 22 chunks (all but 8192 end in a 16-block
// chunk) and a CU owns up to 21.5 row groups of them.  What differs here is k_mv_cu_long's design:
//
//   * one chunk body, and the ring runs over the wave's chunk stream.  A wave's work is the sequence
//     of the chunks of all its row groups; the loop takes two stream positions per trip, the even
//     one through register slot 0 and the odd one through slot 1, so the slots are named statically.
//     A row group's first chunk (zero acc / off, mv_pre_epi) and last chunk (reduce, epilogue) are
//     wave-uniform branches in that body.  The code does not grow with K: the chunk loop is rolled,
//     and K is a template constant only for the prologue's per-thread unit counts, the LDS carve-up
//     and the chunk / tail counts;
//   * seven nt loads per position in program order: the d, m and weight-sum words, then four nibble
//     words per lane.  A slot is refilled two positions ahead as soon as its chains are done,
//     whether that is this row group's chunk or the next one's first: the wait ahead of a slot's
//     nibbles leaves the other slot's seven loads in flight, the wait for the next position's d and m
//     twelve, and no wait in the loop drains the queue.  The 16-block last chunk is a sub-chunk
//     count (2 of 4): its missing nibble words are loaded from its first sub-chunk (the same cache
//     lines) and never used, and having no blocks 16..31 it skips the odd neighbour's half of the
//     weight-sum word (DPP quad_perm [1,1,3,3]).  Past the stream's end the refills go on as loads
//     of one 16-byte word per image (the wave's first chunk, all lanes on one address); a stream of
//     odd length (7 chunks x an odd number of row groups) ends on such a position, fetched and not
//     computed;
//   * the four product tables (s = dx*dy, dx*my, mx*dy, mx*my; 8 rows x 32 blocks, row stride 40
//     floats) of the NEXT position are written while the current one's chains run -- its d and m
//     sit in the other slot -- so no write -> read round trip precedes a chain: two buffers, 10 KiB
//     per wave.  LDS per launch: K bytes of act, K / 8 of ys, 256 B of dyv | myv per chunk, the
//     buffers and one double per wave: 49 / 89 KiB (6656, 4 / 8 waves), 51 / 91 KiB (8192), 104 KiB
//     (17920), 110 KiB (22016).  Every role fits with two buffers at the wave count it wants, so none
//     is single-buffered; launches above 64 KiB raise the kernel's dynamic LDS limit.
// No workgroup waits on another: plain vector loads and stores only.
#include <cstdlib>
#include <type_traits>
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

namespace lvk {

namespace {
using namespace mv;

// (the images lead the block, as in matvec_cu41.hip)
struct Long41Images {
    const uint4 * nib;          // [G][NC][4 sub][64]
    const float4 * scl;         // [G][NC][2][64]: d, then m
    const uint4 * wsum;         // [G][NC][64]: even-chain weight sums (lvk_kernels.h q41_wsum)
    int G;                      // row groups (M / 8)
};
struct Long41Params : Long41Images, MvArgs {};

// per-wave product tables in LDS, matvec_cu41.hip's padded layout (4 tables of 8 rows x 32 blocks,
// the row stride 40 floats: conflict-free broadcast reads and lane stores), two buffers of them
constexpr int SRS = 40, SPL = 8 * SRS, SWF = 4 * SPL;

constexpr size_t lds_bytes(int K, int NW) {
    return (size_t) K + (size_t) ((K / 32 + 31) / 32) * 256 + (size_t) K / 8 + (size_t) NW * 2 * SWF * 4 +
           (size_t) NW * 8;
}

template <int NW, int PRO, int EPI, int KT>
__global__ __launch_bounds__(NW * 64) void k_mv_cu41_long(Long41Params P) {
    constexpr int NT = NW * 64;
    constexpr int nb = KT / 32;                 // blocks per row
    constexpr int nsub = nb / 8;                // 8-block sub-chunks (one uint4 per lane each)
    constexpr int NC = (nb + 31) / 32;          // chunks of 32 blocks, the last one maybe partial
    constexpr int TSUB = nsub - (NC - 1) * 4;   // sub-chunks of the last chunk
    constexpr int nunits = KT / 8;              // f32 prologue work units (8 elements)
    constexpr bool FPRO = PRO == PRO_NORM || PRO == PRO_ACTF;
    static_assert(nb % 8 == 0, "K must be a multiple of 256");
    static_assert(NC >= 3 && (TSUB == 2 || TSUB == 4), "chunk stream");

    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t * act = (uint32_t *) smem;                          // nb * 32 B
    float * dyv = (float *) (smem + nb * 32);                    // NC * 32
    float * myv = dyv + NC * 32;                                 // NC * 32
    uint8_t * ys = (uint8_t *) (myv + NC * 32);                  // nb * 4 bytes: activation sums
    float * sbuf = (float *) (ys + nb * 4);                      // NW * 2 * SWF
    double * red = (double *) (sbuf + NW * 2 * SWF);             // NW

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
    const int j = lane & 7;
    const int r = lane >> 3;
    const int bid = blockIdx.x, nwg = gridDim.x;
    const int g0 = (int) ((unsigned) bid * (unsigned) P.G / (unsigned) nwg);     // G * n_cu < 2^32
    const int g1 = (int) ((unsigned) (bid + 1) * (unsigned) P.G / (unsigned) nwg);
    const int ng = max(0, (g1 - g0 - wave + NW - 1) / NW);      // row groups of this wave: g0 + wave + k * NW
    const int gfirst = min(g0 + wave, P.G - 1);
    // the QKV epilogue's position, an atomic load ahead of the prologue inputs (matvec_cu41.hip)
    [[maybe_unused]] int pos0 = 0;
    if constexpr (EPI == EPI_QKV)
        pos0 = __hip_atomic_load((const __attribute__((address_space(1))) int *) &P.sp->n_past, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);

    // ---- the prologue inputs, then the ring's first two positions behind them (vmcnt retires in
    // order), then the table while the weights are in flight
    constexpr int UM = FPRO ? (nunits + NT - 1) / NT : (nb + NT - 1) / NT;
    [[maybe_unused]] float4 xv[FPRO ? UM : 1][2];
    [[maybe_unused]] float4 gv[PRO == PRO_NORM ? UM : 1][2];
    [[maybe_unused]] uint4 qv[FPRO ? 1 : UM];
    [[maybe_unused]] float dv[FPRO ? 1 : UM], mv_[FPRO ? 1 : UM];
    if constexpr (FPRO) {
        pro_load_units<NT, PRO>(P.x, P.g, nunits, tid, xv, gv);
    } else {
#pragma unroll
        for (int k = 0; k < UM; ++k) {
            const int b = min(k * NT + tid, nb - 1);
            qv[k] = P.xq.qs[b];
            dv[k] = P.xq.d[b];
            mv_[k] = P.xq.m[b];
        }
    }

    // the ring.  Per chunk cc of row group grp the images hold d | m [2][1 KiB], wsum [1 KiB] and
    // nib [4 sub][1 KiB]; a lane's slice of each 1 KiB is its 16 bytes.  d, m and the weight sums of a
    // position go out before its nibbles; all of it is read once per token: nt loads.  lo: the lane's
    // byte offset (0: the whole wave on one 16-byte word)
    uint4 W[2][4], WS[2];
    float4 SD[2], SM[2];
#define LVK_ISSUE(slot, grp, cc, lo)                                                                    \
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
    // a wave without row groups (it only helps build the table) issues the same loads with every
    // lane on one word: no branch around the issue, so the wait counts stay exact on every path
    const uint32_t loff = ng > 0 ? (uint32_t) lane * 16u : 0u;
    LVK_ISSUE(0, gfirst, 0, loff);
    LVK_ISSUE(1, gfirst, 1, loff);
    // the inputs marked landed here, where the count is exact: fourteen weight loads stay in flight
#pragma unroll
    for (int k = 0; k < UM; ++k) {
        if constexpr (FPRO) {
            launder(xv[k][0]); launder(xv[k][1]);
            if constexpr (PRO == PRO_NORM) { launder(gv[k][0]); launder(gv[k][1]); }
        } else {
            launder(qv[k]); launder(dv[k]); launder(mv_[k]);
        }
    }

    if constexpr (FPRO) {
        float scale = 1.0f;
        if constexpr (PRO == PRO_NORM) {
            // per-thread units, a DPP wave tree, then the NW wave sums in order (RMSNorm order)
            double acc = pro_sumsq_units<NT>(xv, nunits, tid);
            acc = wave_sum_d(acc);
            if (lane == 0) red[wave] = acc;
            __syncthreads();
            double sum = red[0];
            for (int w = 1; w < NW; ++w) sum += red[w];
            const float mean = rms_mean_wave(sum, P.x, KT);
            scale = 1.0f / sqrtf(mean + 1e-6f);
        }
        pro_q41_units<NT, PRO>(xv, gv, scale, nunits, tid, act, dyv, myv, ys);
    } else {
#pragma unroll
        for (int k = 0; k < UM; ++k) {
            const int b = k * NT + tid;
            if (b < nb) q41_block_store(act, dyv, myv, ys, b, qv[k], dv[k], mv_[k]);
        }
    }
    __syncthreads();            // activation table ready
    if (ng == 0) return;

    // ---- the chunk stream.  Per position: the chains run against the current table buffer, the slot
    // is refilled two positions ahead, and the products of the NEXT position go to the other buffer
    // (ggml.c:2205-2212: slot 8m + j of a table = block 32c + 8m + j of the lane's row).
    const bool even = (j & 1) == 0;
    const uint32_t * ys32 = (const uint32_t *) ys;
    float * sw = sbuf + wave * 2 * SWF;
    // a tail chunk's slots 16..31 multiply dyv / myv words no block wrote: stored, never read
    auto make_table = [&](int buf, const float4 & dxv, const float4 & mxv, int cc) __attribute__((always_inline)) {
        const float4 dy = *(const float4 *) (dyv + cc * 32 + j * 4);
        const float4 my = *(const float4 *) (myv + cc * 32 + j * 4);
        float * sl = sw + buf * SWF + r * SRS + j;
        const float dxa[4] = {dxv.x, dxv.y, dxv.z, dxv.w};
        const float mxa[4] = {mxv.x, mxv.y, mxv.z, mxv.w};
        const float dya[4] = {dy.x, dy.y, dy.z, dy.w};
        const float mya[4] = {my.x, my.y, my.z, my.w};
#pragma unroll
        for (int mq = 0; mq < 4; ++mq) {
            sl[mq * 8] = dxa[mq] * dya[mq];
            sl[SPL + mq * 8] = dxa[mq] * mya[mq];
            sl[2 * SPL + mq * 8] = mxa[mq] * dya[mq];
            sl[3 * SPL + mq * 8] = mxa[mq] * mya[mq];
        }
    };

    const int npos = ng * NC;               // the stream's positions; an odd count is padded by one
    int pos = 0, c = 0, gc = gfirst;        // the position consumed: chunk c of row group gc
    int fpos = 2, fc = 2, fg = gfirst;      // the position the ring fetches next
    int tbuf = 0;
    float acc = 0.0f, off = 0.0f;
    EpiPre pe{make_float2(0.0f, 0.0f), 0.0f};
    // the 8 blocks of sub-chunk sb on the chain.  wsw: the even chains' sums of these blocks (one byte
    // per block, exact as floats); odd chains take the activation sums from LDS (ggml.c:2236-2240)
    auto chain8 = [&](const uint4 & w, int sb, uint32_t ws0, uint32_t ws1) __attribute__((always_inline)) {
        const float * srow = sw + tbuf * SWF + r * SRS;
        const float * xrow = srow + (even ? SPL : 2 * SPL);
        const float * mrow = srow + 3 * SPL;
        const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int uu = c * 8 + sb * 2 + pp;             // group of 4 blocks
            const int bi = sb * 8 + pp * 4;                 // first block within the chunk
            const uint4 a = *(const uint4 *) (act + ((size_t) uu * 8 + j) * 4);
            const float4 s4 = *(const float4 *) (srow + bi);
            const float4 x4 = *(const float4 *) (xrow + bi);
            const float4 m4 = *(const float4 *) (mrow + bi);
            const uint32_t ydw = ys32[(size_t) uu * 4 + (j >> 1)];
            const uint32_t sdw = even ? (pp ? ws1 : ws0) : ydw;
            const float S[4] = {(float) (sdw & 0xFFu), (float) ((sdw >> 8) & 0xFFu), (float) ((sdw >> 16) & 0xFFu),
                                (float) (sdw >> 24)};
            const int p[4] = {udot8(wd[2 * pp], a.x), udot8(wd[2 * pp], a.y), udot8(wd[2 * pp + 1], a.z),
                              udot8(wd[2 * pp + 1], a.w)};
            const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
            const float ms[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc = __builtin_fmaf(sv[k], (float) p[k], acc);
                acc = __builtin_fmaf(xs[k], S[k], acc);
                off = off + ms[k];
            }
        }
    };
    // one stream position through ring slot d.  The odd slot's may be the padding position: its
    // refill and table go on as everywhere (the wait counts of the even slot stay exact on the way
    // back into the loop), its chunk is not computed
    auto position = [&](auto slot) __attribute__((always_inline)) {
        constexpr int d = decltype(slot)::value;
        const bool live = d == 0 || pos < npos;
        if (live) {
            if (c == 0) {
                // a row group starts: its epilogue's memory operand goes out ahead of its chunks
                acc = 0.0f;
                off = 0.0f;
                pe = mv_pre_epi<EPI>(P, gc * 8 + r, pos0);
            }
            // blocks 0-15 of the chunk have their weight sums in the lane's own word, 16-31 in the odd
            // neighbour's; a 16-block tail chunk ends before those
            const uint4 ws = WS[d];
            chain8(W[d][0], 0, ws.x, ws.y);
            chain8(W[d][1], 1, ws.z, ws.w);
            if (TSUB == 4 || c + 1 < NC) {
                const uint32_t n0 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.x, 0xF5, 0xF, 0xF, false);
                const uint32_t n1 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.y, 0xF5, 0xF, 0xF, false);
                const uint32_t n2 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.z, 0xF5, 0xF, 0xF, false);
                const uint32_t n3 = (uint32_t) __builtin_amdgcn_mov_dpp((int) ws.w, 0xF5, 0xF, 0xF, false);
                chain8(W[d][2], 2, n0, n1);
                chain8(W[d][3], 3, n2, n3);
            }
        }
        // refill the slot two positions ahead: this row group's chunk, the next one's first, or past
        // the end one word of the wave's first chunk
        {
            const bool fl = fpos < npos;
            LVK_ISSUE(d, fl ? fg : gfirst, fl ? fc : 0, fl ? loff : 0u);
            ++fpos;
            if (++fc == NC) { fc = 0; fg += NW; }
        }
        // the next position's product tables: its d and m sit in the other slot
        make_table(tbuf ^ 1, SD[d ^ 1], SM[d ^ 1], c + 1 == NC ? 0 : c + 1);
        __builtin_amdgcn_wave_barrier();
        tbuf ^= 1;
        ++pos;
        if (live && ++c == NC) {
            // res = hsum(acc) + acc_offset * QK (ggml.c:2249)
            const float h = octet_reduce(acc);
            mv_epilogue<EPI>(P, gc, r, j, h + off * 32.0f, pos0, pe);
            c = 0;
            gc += NW;
        }
        // keep the positions in program order: the chain values are pinned here, so this chunk's
        // arithmetic cannot sink below the next one's reads
        asm volatile("" : "+v"(acc), "+v"(off));
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };

    make_table(0, SD[0], SM[0], 0);         // chunk 0 of the first row group
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int i = 0; i < npos; i += 2) {
        position(std::integral_constant<int, 0>{});
        position(std::integral_constant<int, 1>{});
    }
#undef LVK_ISSUE
}

// -- host -------------------------------------------------------------------

template <int NW, int PRO, int EPI, int KT>
hipError_t go(const Long41Params & P, hipStream_t s) {
    constexpr size_t lds = lds_bytes(KT, NW);
    static_assert(lds <= 160 * 1024, "LDS");
    const int nwg = std::min(cu_count(), P.G);
    // more than the default 64 KiB of dynamic LDS: opted in per device and not stream-ordered, so
    // with every launch (as matvec_cols41.hip does)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *) k_mv_cu41_long<NW, PRO, EPI, KT>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    LVK_LAUNCH((k_mv_cu41_long<NW, PRO, EPI, KT>), dim3(nwg), dim3(NW * 64), lds, s, P);
    return hipGetLastError();
}

// launch shapes (waves NW) per row length and role, by matvec_cu_long.hip's rule: a wave keeps two
// positions (14 KB here) in flight and a CU should keep 60-120 KB, so 8 waves (112 KB) wherever a CU
// has the row groups for them: on 256 CUs QKV has 9.75 / 12 row groups per CU (30B / 65B), W1|W3
// 17.5 / 21.5, lm_head 15.6.  Wo and W2 have 3.25 / 4: no more compute waves than that, so Wo takes 4
// (56 KB); the W2 launch takes 8 so that the quantization of u (17920 / 22016 floats per workgroup)
// is spread over 512 threads.  One shape per role, not swept.
template <int KE>       // n_embd
hipError_t go_embd(const Long41Params & P, int pro, int epi, hipStream_t s) {
    if (pro == PRO_NORM) {
        switch (epi) {
            case EPI_QKV: return go<8, PRO_NORM, EPI_QKV, KE>(P, s);
            case EPI_SWIGLU_F32: return go<8, PRO_NORM, EPI_SWIGLU_F32, KE>(P, s);
            case EPI_STORE: return go<8, PRO_NORM, EPI_STORE, KE>(P, s);
        }
    }
    if (pro == PRO_ACTQ && epi == EPI_RESID) return go<4, PRO_ACTQ, EPI_RESID, KE>(P, s);
    // operator API (lvk_mul_mat_q: plain quantize of an f32 input)
    if (pro == PRO_ACTF && epi == EPI_STORE) return go<8, PRO_ACTF, EPI_STORE, KE>(P, s);
    return hipErrorNotSupported;
}
template <int KF>       // n_ff
hipError_t go_ff(const Long41Params & P, int pro, int epi, hipStream_t s) {
    if (pro == PRO_ACTF && epi == EPI_RESID) return go<8, PRO_ACTF, EPI_RESID, KF>(P, s);
    if (pro == PRO_ACTF && epi == EPI_STORE) return go<8, PRO_ACTF, EPI_STORE, KF>(P, s);
    // operator API (lvk_mul_mat_q_norm): the generic kernel has PRO_NORM for even row-group counts only
    if (pro == PRO_NORM && epi == EPI_STORE) return go<8, PRO_NORM, EPI_STORE, KF>(P, s);
    return hipErrorNotSupported;
}

}  // namespace

// LVK_DECODE_LONG=0 (read once per process, the switch of matvec_cu_long.hip) keeps these row lengths
// on the generic kernels, for A/B runs
bool matvec_cu41_long_supported(int K) {
    static const bool on = [] { const char * e = getenv("LVK_DECODE_LONG"); return !e || atoi(e) != 0; }();
    return on && (K == 6656 || K == 8192 || K == 17920 || K == 22016);
}

hipError_t launch_matvec_cu41_long(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    if (L.w.qtype != Q4_1 || L.n_tokens != 1 || L.w.M % 8 || L.w.M < 8 || !matvec_cu41_long_supported(L.w.K))
        return hipErrorNotSupported;
    if (!mv_inputs_set(L, pro)) return hipErrorInvalidValue;
    Long41Params P{};
    mv_fill(P, L, true);
    P.nib = L.w.nib;
    P.scl = (const float4 *) L.w.scl;
    P.wsum = q41_wsum(L.w);
    P.G = L.w.M / 8;
    switch (L.w.K) {
        case 6656: return go_embd<6656>(P, pro, epi, s);
        case 8192: return go_embd<8192>(P, pro, epi, s);
        case 17920: return go_ff<17920>(P, pro, epi, s);
        case 22016: return go_ff<22016>(P, pro, epi, s);
    }
    return hipErrorNotSupported;
}

}  // namespace lvk
