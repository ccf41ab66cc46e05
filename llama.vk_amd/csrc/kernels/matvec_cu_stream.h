// matvec_cu_stream.h -- the chunk stream of the CU-balanced single-token matvecs for long rows: the one
// device body, role table and launcher behind k_mv_cu_long (matvec_cu_long.hip, Q4_0) and k_mv_cu41_long
// (matvec_cu41_long.hip, Q4_1).
//
// Organisation and result bits are k_mv_cu's / k_mv_cu41's: one workgroup per CU, workgroup w owns the
// row groups [w * G / n, (w + 1) * G / n), the activation table (RMSNorm + quantize, a plain quantize,
// or a quantized input unpacked) is built once per workgroup in LDS, lane 8r + j is chain j of row r,
// the chain runs in block order against per-wave product tables in LDS (two buffers, row stride SRS),
// then the octet reduce and the shared epilogues.
//
// k_mv_cu and k_mv_cu41 are unrolled over the whole row and prefetch across row groups only when their
// depth divides the chunk count.  The long rows have 5 to 22 chunks (most of them end in a 16-block
// chunk), a CU owns up to 21.5 row groups of them, and unrolled they would be up to 22 chunk bodies per
// instantiation in the decode step's instruction stream.  What differs here:
//
//   * one chunk body, and the ring runs over the wave's chunk stream.  A wave's work is the sequence
//     of the chunks of all its row groups; the loop takes two stream positions per trip, the even
//     one through register slot 0 and the odd one through slot 1, so the slots are named statically.
//     A row group's first chunk (zero the chain, mv_pre_epi) and last chunk (reduce, epilogue) are
//     wave-uniform branches in that body.  The code does not grow with K: the chunk loop is rolled,
//     and K is a template constant only for the prologue's per-thread unit counts, the LDS carve-up
//     and the chunk / tail counts;
//   * exact wait counts.  A slot is refilled two positions ahead as soon as its chains are done,
//     whether that is this row group's chunk or the next one's first, and every position issues the
//     same n nt loads in program order (Q4_0 five: the scales, then four nibble words per lane; Q4_1
//     seven: d, m and the weight sums, then the nibble words): the wait ahead of a slot's nibbles
//     leaves the other slot's n loads in flight, the wait for the next position's scales 2n - 1 (Q4_1:
//     d and m, 2n - 1 and 2n - 2), and no wait in the loop drains the queue.  The 16-block last chunk
//     is a sub-chunk count (2 of 4): its missing nibble words are loaded from its first sub-chunk (the
//     same cache lines) and never used.  Past the stream's end the refills go on as loads of one
//     16-byte word per image (the wave's first chunk, all lanes on one address); a stream of odd
//     length ends on such a position, fetched and not computed;
//   * the product tables of the NEXT position are written while the current one's chains run -- its
//     scales sit in the other slot -- so no write -> read round trip precedes a chain.
// No workgroup waits on another: plain vector loads and stores only.
//
// This header is the kernel's text and is included once by each format file (matvec_cu_long.hip,
// matvec_cu41_long.hip), after the format has defined the kernel's name, its host-side type and the
// pieces that differ between Q4_0 and Q4_1 as macros.  The pieces are macros, not functions of a format
// type, because hipcc compiles the stream differently when they are called pieces (SGPR and VGPR counts
// up by 1..3, another refill arithmetic in the chunk loop, a few roles 0.5..0.9 % slower on the 30B
// shapes): expanded here the kernels compile to the instructions they had as two separate texts
// (profiles/decode_stream_kernel_resources.md).  There is no run-time branch on the format.
//   LVK_STREAM_KERNEL            the __global__ name
//   LVK_STREAM_FORMAT            host type: Params, QTYPE, KE0 / KE1 (n_embd), KF0 / KF1 (n_ff), nw_qkv(KE),
//                                NW_WIDE, LDS_MAX and lds_bytes(K, NW), which sits beside LVK_STREAM_CARVE
//   LVK_STREAM_CARVE             the LDS carve-up of smem: the tables, sbuf, then `double * red`
//   LVK_STREAM_STAGED(n)         the PRO_ACTQ inputs of n blocks, held in registers; _LOAD(k, b), _LAND(k)
//   LVK_STREAM_STORE_BLOCK(k, b), LVK_STREAM_QUANTIZE: staged block k into the table; the FPRO quantizer
//   LVK_STREAM_RING              the ring registers; LVK_STREAM_ISSUE(slot, grp, cc, lo) their loads
//   LVK_STREAM_TABLES            per-wave pointers and the make_table / chain lambdas ahead of the stream
//   LVK_STREAM_CHAIN             the chain state; LVK_STREAM_CHAIN8: a chain lambda that reads c / tbuf
//   LVK_STREAM_ZERO, LVK_STREAM_CHUNK(d), LVK_STREAM_MAKE_TABLE(buf, slot, cc), LVK_STREAM_RESULT,
//   LVK_STREAM_PIN               zero the chain, one chunk through slot d, the tables of chunk cc whose
//                                scales sit in `slot`, the row's result, the pin of the chain values
#pragma once
#include <cstdlib>
#include <type_traits>
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

namespace lvk {

namespace {
using namespace mv;
using namespace mv::cu_lds;

template <int NW, int PRO, int EPI, int KT>
__global__ __launch_bounds__(NW * 64) void LVK_STREAM_KERNEL(LVK_STREAM_FORMAT::Params P) {
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
    LVK_STREAM_CARVE

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
    const int j = lane & 7;
    const int r = lane >> 3;
    const int g0 = row_group0(blockIdx.x, gridDim.x, P.G), g1 = row_group0(blockIdx.x + 1, gridDim.x, P.G);
    const int ng = max(0, (g1 - g0 - wave + NW - 1) / NW);      // row groups of this wave: g0 + wave + k * NW
    const int gfirst = min(g0 + wave, P.G - 1);
    [[maybe_unused]] const int pos0 = mv_pos0<EPI>(P);

    // ---- the prologue inputs, then the ring's first two positions behind them (vmcnt retires in
    // order), then the table while the weights are in flight
    constexpr int UM = FPRO ? (nunits + NT - 1) / NT : (nb + NT - 1) / NT;
    [[maybe_unused]] float4 xv[FPRO ? UM : 1][2];
    [[maybe_unused]] float4 gv[PRO == PRO_NORM ? UM : 1][2];
    LVK_STREAM_STAGED(FPRO ? 1 : UM)
    if constexpr (FPRO) {
        pro_load_units<NT, PRO>(P.x, P.g, nunits, tid, xv, gv);
    } else {
#pragma unroll
        for (int k = 0; k < UM; ++k) {
            const int b = min(k * NT + tid, nb - 1);
            LVK_STREAM_STAGED_LOAD(k, b)
        }
    }

    // the ring: all of a position is read once per token (nt loads).  A wave without row groups (it
    // only helps build the table) issues the same loads with every lane on one word: no branch around
    // the issue, so the wait counts stay exact on every path
    LVK_STREAM_RING
    const uint32_t loff = ng > 0 ? (uint32_t) lane * 16u : 0u;
    LVK_STREAM_ISSUE(0, gfirst, 0, loff);
    LVK_STREAM_ISSUE(1, gfirst, 1, loff);
    // the inputs marked landed here, where the count is exact: the two positions stay in flight
#pragma unroll
    for (int k = 0; k < UM; ++k) {
        if constexpr (FPRO) {
            launder(xv[k][0]); launder(xv[k][1]);
            if constexpr (PRO == PRO_NORM) { launder(gv[k][0]); launder(gv[k][1]); }
        } else {
            LVK_STREAM_STAGED_LAND(k)
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
        LVK_STREAM_QUANTIZE;
    } else {
#pragma unroll
        for (int k = 0; k < UM; ++k) {
            const int b = k * NT + tid;
            if (b < nb) LVK_STREAM_STORE_BLOCK(k, b);
        }
    }
    __syncthreads();            // activation table ready
    if (ng == 0) return;

    // ---- the chunk stream.  Per position: the chains run against the current table buffer, the slot
    // is refilled two positions ahead, and the products of the NEXT position go to the other buffer.
    LVK_STREAM_TABLES
    const int npos = ng * NC;               // the stream's positions; an odd count is padded by one
    int pos = 0, c = 0, gc = gfirst;        // the position consumed: chunk c of row group gc
    int fpos = 2, fc = 2, fg = gfirst;      // the position the ring fetches next
    int tbuf = 0;
    LVK_STREAM_CHAIN
    EpiPre pe{make_float2(0.0f, 0.0f), 0.0f};
    LVK_STREAM_CHAIN8
    // one stream position through ring slot d.  The odd slot's may be the padding position: its
    // refill and table go on as everywhere (the wait counts of the even slot stay exact on the way
    // back into the loop), its chunk is not computed
    auto position = [&](auto slot) __attribute__((always_inline)) {
        constexpr int d = decltype(slot)::value;
        const bool live = d == 0 || pos < npos;
        if (live) {
            if (c == 0) {
                // a row group starts: its epilogue's memory operand goes out ahead of its chunks
                LVK_STREAM_ZERO
                pe = mv_pre_epi<EPI>(P, gc * 8 + r, pos0);
            }
            LVK_STREAM_CHUNK(d)
        }
        // refill the slot two positions ahead: this row group's chunk, the next one's first, or past
        // the end one word of the wave's first chunk
        {
            const bool fl = fpos < npos;
            LVK_STREAM_ISSUE(d, fl ? fg : gfirst, fl ? fc : 0, fl ? loff : 0u);
            ++fpos;
            if (++fc == NC) { fc = 0; fg += NW; }
        }
        // the next position's tables: its scales sit in the other slot
        LVK_STREAM_MAKE_TABLE(tbuf ^ 1, d ^ 1, c + 1 == NC ? 0 : c + 1);
        __builtin_amdgcn_wave_barrier();
        tbuf ^= 1;
        ++pos;
        if (live && ++c == NC) {
            const float res = LVK_STREAM_RESULT;
            mv_epilogue<EPI>(P, gc, r, j, res, pos0, pe);
            c = 0;
            gc += NW;
        }
        // keep the positions in program order: the chain values are pinned here, so this chunk's
        // arithmetic cannot sink below the next one's reads
        LVK_STREAM_PIN
        __builtin_amdgcn_sched_barrier(0);
    };

    LVK_STREAM_MAKE_TABLE(0, 0, 0);         // chunk 0 of the first row group
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int i = 0; i < npos; i += 2) {
        position(std::integral_constant<int, 0>{});
        position(std::integral_constant<int, 1>{});
    }
}

// -- host -------------------------------------------------------------------


template <class F, int NW, int PRO, int EPI, int KT>
hipError_t stream_go(const typename F::Params & P, hipStream_t s) {
    constexpr size_t lds = F::lds_bytes(KT, NW);
    static_assert(lds <= F::LDS_MAX, "LDS");
    const auto kern = &LVK_STREAM_KERNEL<NW, PRO, EPI, KT>;
    const int nwg = std::min(cu_count(), P.G);
    // more than the default 64 KiB of dynamic LDS: opted in per device and not stream-ordered, so
    // with every launch (as matvec_cols41.hip does)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    LVK_LAUNCH(kern, dim3(nwg), dim3(NW * 64), lds, s, P);
    return hipGetLastError();
}

// launch shapes (waves NW) per row length and role, by k_mv_cu's rule: a wave keeps two positions (Q4_0
// 10 KB, Q4_1 14 KB) in flight, and a CU should keep 60-120 KB.  On 256 CUs QKV has 7.5 / 9.75 / 12 row
// groups per CU (13B / 30B / 65B), W1|W3 13.5 / 17.5 / 21.5, lm_head 15.6, Wo and W2 2.5 / 3.25 / 4: those
// two cannot use more waves than a CU has row groups, so Wo takes 4; the W2 launch takes 8 so that the
// quantization of u (13824 .. 22016 floats per workgroup) is spread over 512 threads.  QKV takes
// F::nw_qkv(n_embd) waves, W1|W3 and lm_head F::NW_WIDE; Q4_1 stops at 8 (112 KB) everywhere.  One
// shape per role, not swept.
template <class F, int KE>      // n_embd
hipError_t stream_go_embd(const typename F::Params & P, int pro, int epi, hipStream_t s) {
    constexpr int NWQ = F::nw_qkv(KE), NWW = F::NW_WIDE;
    if (pro == PRO_NORM) {
        switch (epi) {
            case EPI_QKV: return stream_go<F, NWQ, PRO_NORM, EPI_QKV, KE>(P, s);
            case EPI_SWIGLU_F32: return stream_go<F, NWW, PRO_NORM, EPI_SWIGLU_F32, KE>(P, s);
            case EPI_STORE: return stream_go<F, NWW, PRO_NORM, EPI_STORE, KE>(P, s);
        }
    }
    if (pro == PRO_ACTQ && epi == EPI_RESID) return stream_go<F, 4, PRO_ACTQ, EPI_RESID, KE>(P, s);
    // operator API (lvk_mul_mat_q: plain quantize of an f32 input)
    if (pro == PRO_ACTF && epi == EPI_STORE) return stream_go<F, 8, PRO_ACTF, EPI_STORE, KE>(P, s);
    return hipErrorNotSupported;
}
template <class F, int KF>      // n_ff
hipError_t stream_go_ff(const typename F::Params & P, int pro, int epi, hipStream_t s) {
    if (pro == PRO_ACTF && epi == EPI_RESID) return stream_go<F, 8, PRO_ACTF, EPI_RESID, KF>(P, s);
    if (pro == PRO_ACTF && epi == EPI_STORE) return stream_go<F, 8, PRO_ACTF, EPI_STORE, KF>(P, s);
    // operator API (lvk_mul_mat_q_norm): the generic Q4_1 kernel has PRO_NORM for even row-group counts only
    if (pro == PRO_NORM && epi == EPI_STORE) return stream_go<F, 8, PRO_NORM, EPI_STORE, KF>(P, s);
    return hipErrorNotSupported;
}

template <class F>
bool stream_supported(int K) {
    return decode_long_on() && (K == F::KE0 || K == F::KE1 || K == F::KF0 || K == F::KF1);
}

template <class F>
hipError_t stream_launch(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    if (L.w.qtype != F::QTYPE || L.n_tokens != 1 || L.w.M % 8 || L.w.M < 8 || !stream_supported<F>(L.w.K))
        return hipErrorNotSupported;
    if (!mv_inputs_set(L, pro)) return hipErrorInvalidValue;
    typename F::Params P{};
    cu_fill(P, L);
    switch (L.w.K) {
        case F::KE0: return stream_go_embd<F, F::KE0>(P, pro, epi, s);
        case F::KE1: return stream_go_embd<F, F::KE1>(P, pro, epi, s);
        case F::KF0: return stream_go_ff<F, F::KF0>(P, pro, epi, s);
        case F::KF1: return stream_go_ff<F, F::KF1>(P, pro, epi, s);
    }
    return hipErrorNotSupported;
}

}  // namespace

}  // namespace lvk
