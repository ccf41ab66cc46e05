// matvec_cu_long.hip -- the CU-balanced single-token Q4_0 matvec (matvec_cu.hip) for the row lengths of
// LLaMA 13B (n_embd 5120, n_ff 13824) and 30B (6656, 17920).
//
// Organisation and result bits are k_mv_cu's: one workgroup per CU, workgroup w owns the row groups
// [w * G / n, (w + 1) * G / n), the activation table (RMSNorm + quantize, a plain quantize, or a
// quantized input unpacked) is built once per workgroup in LDS, lane 8r + j is chain j of row r, exact
// v_dot8_i32_i4 partials, fmaf(dw * dx, P, acc) in block order per chain against the per-wave s = dw * dx
// table in LDS (two buffers, row stride SRS), the octet reduce, the shared epilogues.
//
// k_mv_cu is unrolled over the whole row and prefetches across row groups only when the chunk count
// is a multiple of its depth.  These rows have 5, 7, 14 and 18 chunks (three of them end in a
// 16-block chunk), a CU owns up to 17.5 row groups of them, and unrolled they would be up to 18
// chunk bodies per instantiation in the decode step's instruction stream.  What differs here:
//
//   * one chunk body, and the ring runs over the wave's chunk stream.  A wave's work is the sequence
//     of the chunks of all its row groups; the loop takes two stream positions per trip, the even
//     one through register slot 0 and the odd one through slot 1, so the slots are named statically.
//     A row group's first chunk (zero the chain, mv_pre_epi) and last chunk (reduce, epilogue) are
//     wave-uniform branches in that body.  The code does not grow with K: the chunk loop is rolled,
//     and K is a template constant only for the prologue's per-thread unit counts and the LDS
//     carve-up;
//   * exact wait counts.  A slot is refilled two positions ahead as soon as its chains are done,
//     whether that is this row group's chunk or the next one's first, and every position issues
//     five loads (scales, then four nibble words per lane): the wait ahead of a slot's nibbles
//     leaves the other slot's five loads in flight, the wait for the next position's scales nine,
//     and no wait in the loop drains the queue.  The 16-block last chunk is a sub-chunk count (2 of
//     4): its missing sub-chunks are loaded from its first one (the same cache lines) and never
//     used.  Past the stream's end the refills go on as loads of one 16-byte word per wave (the
//     wave's first chunk, all lanes on one address); a stream of odd length ends on such a position,
//     fetched and not computed.
// No workgroup waits on another: plain vector loads and stores only.
#include <cstdlib>
#include <type_traits>
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

namespace lvk {

namespace {
using namespace mv;

// (the images lead the block, as in matvec_cu.hip: the first scalar loads fetch what the
// row-group split and the weight addresses need)
struct LongImages {
    const uint4 * nib;
    const float4 * scl;
    int G;                      // row groups (M / 8)
};
struct LongParams : LongImages, MvArgs {};

// per-wave block-scale table in LDS, as in matvec_cu.hip (two buffers, 8 rows x 32 blocks, the
// row stride padded to 40 floats: bank-conflict free broadcast reads)
constexpr int SRS = 40, SPL = 8 * SRS;

constexpr size_t lds_bytes(int K, int NW) {
    return (size_t) K + (size_t) ((K / 32 + 31) / 32) * 128 + (size_t) NW * 2 * SPL * 4 + (size_t) NW * 8;
}

template <int NW, int PRO, int EPI, int KT>
__global__ __launch_bounds__(NW * 64) void k_mv_cu_long(LongParams P) {
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
    float * dxp = (float *) (smem + nb * 32);                    // NC * 128 B
    float * sbuf = dxp + NC * 32;                                // NW * 2 * SPL floats
    double * red = (double *) (sbuf + NW * 2 * SPL);             // NW doubles

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
    // the QKV epilogue's position, an atomic load ahead of the prologue inputs (matvec_cu.hip)
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
    [[maybe_unused]] float dv[FPRO ? 1 : UM];
    if constexpr (FPRO) {
        pro_load_units<NT, PRO>(P.x, P.g, nunits, tid, xv, gv);
    } else {
#pragma unroll
        for (int k = 0; k < UM; ++k) {
            const int b = min(k * NT + tid, nb - 1);
            qv[k] = P.xq.qs[b];
            dv[k] = P.xq.d[b];
        }
    }

    // the ring: the scales of a position go out before its nibbles; all of it is read once per token:
    // nt loads.  lo: the lane's byte offset (0: the whole wave on one 16-byte word)
    uint4 W[2][4];
    float4 S[2];
#define LVK_ISSUE(slot, grp, cc, lo)                                                                    \
    do {                                                                                                \
        const size_t ch_ = (size_t) (grp) * NC + (cc);                                                  \
        S[slot] = ld_nt((const float4 *) ((const char *) (P.scl + ch_ * 64) + (lo)));                   \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) {                                              \
            const int sq_ = (cc) * 4 + sb < nsub ? sb : 0;                                              \
            W[slot][sb] = ld_nt((const uint4 *) ((const char *) (P.nib + (ch_ * 4 + sq_) * 64) + (lo))); \
        }                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)
    // a wave without row groups (it only helps build the table) issues the same loads with every
    // lane on one word: no branch around the issue, so the wait counts stay exact on every path
    const uint32_t loff = ng > 0 ? (uint32_t) lane * 16u : 0u;
    LVK_ISSUE(0, gfirst, 0, loff);
    LVK_ISSUE(1, gfirst, 1, loff);
    // the inputs marked landed here, where the count is exact: ten weight loads stay in flight
#pragma unroll
    for (int k = 0; k < UM; ++k) {
        if constexpr (FPRO) {
            launder(xv[k][0]); launder(xv[k][1]);
            if constexpr (PRO == PRO_NORM) { launder(gv[k][0]); launder(gv[k][1]); }
        } else {
            launder(qv[k]); launder(dv[k]);
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
        pro_q40_units<NT, PRO>(xv, gv, scale, nunits, tid, act, dxp);
    } else {
#pragma unroll
        for (int k = 0; k < UM; ++k) {
            const int b = k * NT + tid;
            if (b < nb) q40_block_store(act, dxp, b, qv[k], dv[k]);
        }
    }
    __syncthreads();            // activation table ready
    if (ng == 0) return;

    // ---- the chunk stream.  Per position: the chunk's activation words and scale products are read
    // from LDS up front, the chains run, the slot is refilled two positions ahead, and the scale
    // products of the NEXT position go to the other table buffer (s = dw * dx, ggml.c:1968), so no
    // write -> read round trip precedes a chain.
    float * sw = sbuf + wave * 2 * SPL;
    auto make_table = [&](int buf, const float4 & Sv, int cc) __attribute__((always_inline)) {
        const float4 dx = *(const float4 *) (dxp + cc * 32 + j * 4);
        float4 sv;
        sv.x = Sv.x * dx.x; sv.y = Sv.y * dx.y; sv.z = Sv.z * dx.z; sv.w = Sv.w * dx.w;
        *(float4 *) (sw + buf * SPL + r * SRS + j * 4) = sv;
    };
    // the 8 blocks of sub-chunk sb on the chain
    auto chain8 = [&](float acc, const uint4 & w, const uint4 & a0, const uint4 & a1, const float (&sa)[8][4],
                      int sb) __attribute__((always_inline)) {
        const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int bi = sb * 8 + pp * 4;
            const uint4 a = pp ? a1 : a0;
            const int p0 = dot8(wd[2 * pp], a.x);
            const int p1 = dot8(wd[2 * pp], a.y);
            const int p2 = dot8(wd[2 * pp + 1], a.z);
            const int p3 = dot8(wd[2 * pp + 1], a.w);
            acc = __builtin_fmaf(sa[(bi + 0) & 7][(bi + 0) >> 3], (float) p0, acc);
            acc = __builtin_fmaf(sa[(bi + 1) & 7][(bi + 1) >> 3], (float) p1, acc);
            acc = __builtin_fmaf(sa[(bi + 2) & 7][(bi + 2) >> 3], (float) p2, acc);
            acc = __builtin_fmaf(sa[(bi + 3) & 7][(bi + 3) >> 3], (float) p3, acc);
        }
        return acc;
    };

    const int npos = ng * NC;               // the stream's positions; an odd count is padded by one
    int pos = 0, c = 0, gc = gfirst;        // the position consumed: chunk c of row group gc
    int fpos = 2, fc = 2, fg = gfirst;      // the position the ring fetches next
    int tbuf = 0;
    float acc = 0.0f;
    EpiPre pe{make_float2(0.0f, 0.0f), 0.0f};
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
                pe = mv_pre_epi<EPI>(P, gc * 8 + r, pos0);
            }
            // the partial chunk's missing sub-chunks read the dx table: in LDS, never used
            const float * sl = sw + tbuf * SPL;
            uint4 A[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) A[q] = *(const uint4 *) (act + ((c * 8 + q) * 8 + j) * 4);
            float sa[8][4];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float4 v = *(const float4 *) (sl + r * SRS + jj * 4);
                sa[jj][0] = v.x; sa[jj][1] = v.y; sa[jj][2] = v.z; sa[jj][3] = v.w;
            }
            acc = chain8(acc, W[d][0], A[0], A[1], sa, 0);
            acc = chain8(acc, W[d][1], A[2], A[3], sa, 1);
            if (TSUB == 4 || c + 1 < NC) {
                acc = chain8(acc, W[d][2], A[4], A[5], sa, 2);
                acc = chain8(acc, W[d][3], A[6], A[7], sa, 3);
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
        // the next position's scale table: its scales sit in the other slot
        make_table(tbuf ^ 1, S[d ^ 1], c + 1 == NC ? 0 : c + 1);
        __builtin_amdgcn_wave_barrier();
        tbuf ^= 1;
        ++pos;
        if (live && ++c == NC) {
            const float res = octet_reduce(acc);
            mv_epilogue<EPI>(P, gc, r, j, res, pos0, pe);
            c = 0;
            gc += NW;
        }
        // keep the positions in program order: the chain value is pinned here, so this chunk's
        // arithmetic cannot sink below the next one's reads
        asm volatile("" : "+v"(acc));
        __builtin_amdgcn_sched_barrier(0);
    };

    make_table(0, S[0], 0);                 // chunk 0 of the first row group
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
hipError_t go(const LongParams & P, hipStream_t s) {
    static_assert(lds_bytes(KT, NW) <= 64 * 1024, "LDS");
    const int nwg = std::min(cu_count(), P.G);
    LVK_LAUNCH((k_mv_cu_long<NW, PRO, EPI, KT>), dim3(nwg), dim3(NW * 64), lds_bytes(KT, NW), s, P);
    return hipGetLastError();
}

// launch shapes (waves NW) per row length and role, by k_mv_cu's rule: a wave keeps two positions
// (10 KB) in flight, and a CU should keep 60-120 KB.  On 256 CUs QKV has 7.5 / 9.75 row groups per
// CU (13B / 30B), W1|W3 13.5 / 17.5, lm_head 15.6, Wo and W2 2.5 / 3.25: those two cannot use more
// waves than a CU has row groups, the W2 launch takes 8 so that the quantization of u (13824 /
// 17920 floats per workgroup) is spread over 512 threads.  Not swept.
template <int KE>       // n_embd
hipError_t go_embd(const LongParams & P, int pro, int epi, hipStream_t s) {
    constexpr int NWQ = KE == 5120 ? 8 : 12;
    if (pro == PRO_NORM) {
        switch (epi) {
            case EPI_QKV: return go<NWQ, PRO_NORM, EPI_QKV, KE>(P, s);
            case EPI_SWIGLU_F32: return go<16, PRO_NORM, EPI_SWIGLU_F32, KE>(P, s);
            case EPI_STORE: return go<16, PRO_NORM, EPI_STORE, KE>(P, s);
        }
    }
    if (pro == PRO_ACTQ && epi == EPI_RESID) return go<4, PRO_ACTQ, EPI_RESID, KE>(P, s);
    // operator API (lvk_mul_mat_q: plain quantize of an f32 input)
    if (pro == PRO_ACTF && epi == EPI_STORE) return go<8, PRO_ACTF, EPI_STORE, KE>(P, s);
    return hipErrorNotSupported;
}
template <int KF>       // n_ff
hipError_t go_ff(const LongParams & P, int pro, int epi, hipStream_t s) {
    if (pro == PRO_ACTF && epi == EPI_RESID) return go<8, PRO_ACTF, EPI_RESID, KF>(P, s);
    if (pro == PRO_ACTF && epi == EPI_STORE) return go<8, PRO_ACTF, EPI_STORE, KF>(P, s);
    if (pro == PRO_NORM && epi == EPI_STORE) return go<8, PRO_NORM, EPI_STORE, KF>(P, s);
    return hipErrorNotSupported;
}

}  // namespace

// LVK_DECODE_LONG=0 (read once per process) keeps these row lengths on the generic kernels, for A/B runs
bool matvec_cu_long_supported(int K) {
    static const bool on = [] { const char * e = getenv("LVK_DECODE_LONG"); return !e || atoi(e) != 0; }();
    return on && (K == 5120 || K == 6656 || K == 13824 || K == 17920);
}

hipError_t launch_matvec_cu_long(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    if (L.w.qtype != Q4_0 || L.n_tokens != 1 || L.w.M % 8 || L.w.M < 8 || !matvec_cu_long_supported(L.w.K))
        return hipErrorNotSupported;
    if (!mv_inputs_set(L, pro)) return hipErrorInvalidValue;
    LongParams P{};
    mv_fill(P, L, true);
    P.nib = L.w.nib;
    P.scl = (const float4 *) L.w.scl;
    P.G = L.w.M / 8;
    switch (L.w.K) {
        case 5120: return go_embd<5120>(P, pro, epi, s);
        case 6656: return go_embd<6656>(P, pro, epi, s);
        case 13824: return go_ff<13824>(P, pro, epi, s);
        case 17920: return go_ff<17920>(P, pro, epi, s);
    }
    return hipErrorNotSupported;
}

}  // namespace lvk
