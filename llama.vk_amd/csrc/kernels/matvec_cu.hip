// matvec_cu.hip -- CU-balanced single-token Q4_0 matvec (the decode hot path).
//
// Same arithmetic as matvec_q4.hip (bit-faithful ggml_vec_dot_q4_0 AVX2
// chains, ggml.c:1950-2026, on an activation quantized by quantize_row_q4_0,
// ggml.c:621-685), organised for the batch-1 weight stream:
//
//   * A decode matvec reads every weight byte once, so it is bound by how fast
//     each CU can pull bytes (~25-30 GB/s per CU; MI355X_MICROARCH.md, HBM) and
//     by how evenly the bytes are spread over the 256 CUs.  The grid is one
//     workgroup per CU and workgroup w owns row groups [w*G/n, (w+1)*G/n)
//     (a row group = 8 rows = one wavefront's work), so every CU streams the
//     same number of bytes (+-1 row group).
//   * The activation table (RMSNorm + quantize, or a plain quantize) is built
//     once per workgroup in LDS while the first D chunks of weights are
//     already in flight.
//   * Each wave walks its row groups with a D-chunk register prefetch that
//     runs across group boundaries, so a CU's weight stream never drains
//     between groups.  Row length K is a template constant: all loads are
//     exact and static (hipcc's vmcnt accounting stays precise).
#include "lvk_device.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

namespace lvk {

namespace {
using namespace mv;

#ifdef LVK_PROBE_TIMING   // dev probe builds only: per-wave s_memtime trace
__device__ unsigned long long g_trace[256 * 16 * 64];
#define LVK_T(ev)                                                                                  \
    do {                                                                                           \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                \
        if (lane == 0 && (ev) < 64) g_trace[((blockIdx.x & 255) * 16 + (wave & 15)) * 64 + (ev)] = t_; \
    } while (0)
#else
#define LVK_T(ev) do { } while (0)
#endif

// (the images lead the block: the kernel's first scalar loads fetch what the row-group split and
// the weight addresses need)
struct CuImages {
    const uint4 * nib;
    const float4 * scl;
    int G;                      // row groups (M / 8)
};
struct CuParams : CuImages, MvArgs {};

// order of the prologue and the first weight loads (k_mv_cu PF; the values are what the sweep
// build's LVK_MV_PF takes)
enum PfOrder : int {
    PF_ISSUE_FIRST = 0,     // the inputs, then the weights are issued, then the activation table is
                            // built as soon as the inputs land (the weights stay in flight)
    PF_INPUTS_LAND = 1,     // the inputs land, then the weights are issued, then the table is built
    PF_TABLE_FIRST = 2,     // the inputs land and the table is built, then the weights are issued
    PF_SPLIT = 5,           // the inputs land, chunk 0 is issued, the table is built, chunks 1..D-1
                            // go out after the workgroup barrier (the barriers wait for the slowest
                            // wave's issue, which the memory system throttles to the return rate
                            // once the CU's queue is full)
};

// per-wave block-scale table s = dw * dx in LDS (two buffers, 8 rows x 32 blocks): the row
// stride is padded to 40 floats so the rows start on banks 0, 40, 16, 56, 32, 8, 48, 24 of
// the 64 and the per-row broadcast float4 reads are bank-conflict free
constexpr int SRS = 40, SPL = 8 * SRS;

// the workgroup body (bid of nwg workgroups)
template <int NW, int NP, int D, int PRO, int EPI, int KT, int PF>
__device__ __forceinline__ void mv_cu_run(const CuParams & P, const int bid, const int nwg, uint8_t * smem) {
    constexpr int PT = NP * 64;                 // prologue threads
    constexpr int nb = KT / 32;                 // blocks per row
    constexpr int nsub = nb / 8;                // 8-block sub-chunks (one uint4 per lane each)
    constexpr int NC = (nb + 31) / 32;          // chunks of 32 blocks
    constexpr bool XG = (NC % D) == 0;          // prefetch may cross into the next group
    constexpr int nunits = KT / 8;              // f32 prologue work units (8 elements)
    static_assert(D <= NC, "prefetch deeper than a row");
    static_assert(nb % 8 == 0, "K must be a multiple of 256");

    uint32_t * act = (uint32_t *) smem;                          // nb * 32 B
    float * dxp = (float *) (smem + nb * 32);                    // NC * 128 B
    float * sbuf = dxp + NC * 32;                                // NW * 2 * SPL floats

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
    [[maybe_unused]] int tq = 4;   // trace event index (probe builds)
    LVK_T(0);

    if (NP > 0 && wave >= NW) {
        // ---- prologue waves: build the activation table while the compute
        // waves put the CU's weight stream in flight (they never wait on x)
        const int pt = tid - NW * 64;
        constexpr int PT_ = PT > 0 ? PT : 64;   // (NP == 0: branch never taken)
        if constexpr (PRO == PRO_NORM || PRO == PRO_ACTF) {
            constexpr int UMP = (nunits + PT_ - 1) / PT_;
            float4 xv[UMP][2];
            float4 gv[PRO == PRO_NORM ? UMP : 1][2];
            pro_load_units<PT_, PRO>(P.x, P.g, nunits, pt, xv, gv);
            constexpr int XPL = PRO == PRO_NORM ? KT / 4 / 64 : 1;
            float4 xs[XPL];
            if constexpr (PRO == PRO_NORM) {
#pragma unroll
                for (int i = 0; i < XPL; ++i) xs[i] = ((const float4 *) P.x)[i * 64 + lane];
            }
            // barrier A: the inputs enter the CU's texture queue ahead of the weight burst
            __builtin_amdgcn_s_barrier();
            float scale = 1.0f;
            if constexpr (PRO == PRO_NORM) {
                // every prologue wave sums all K squares itself (lane-strided, then a
                // butterfly that leaves the same double in every lane), so no
                // cross-wave reduction is needed
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < XPL; ++i) sumsq4(acc, xs[i]);
                LVK_T(56);
                acc = warp_sum_d(acc);
                const float mean = rms_mean_wave(acc, P.x, KT);
                scale = 1.0f / sqrtf(mean + 1e-6f);
                LVK_T(57);
            }
            pro_q40_units<PT_, PRO>(xv, gv, scale, nunits, pt, act, dxp);
        } else {
            __builtin_amdgcn_s_barrier();       // barrier A (see above)
            constexpr int UMP = (nb + PT_ - 1) / PT_;
#pragma unroll
            for (int k = 0; k < UMP; ++k) {
                const int b = k * PT_ + pt;
                if (b < nb) q40_block_store(act, dxp, b, P.xq.qs[b], P.xq.d[b]);
            }
        }
        LVK_T(2);
        __syncthreads();
        return;
    }

    // ---- compute waves
    const int j = lane & 7;
    const int r = lane >> 3;
    const int g0 = (int) ((unsigned) bid * (unsigned) P.G / (unsigned) nwg);     // G * n_cu < 2^32
    const int g1 = (int) ((unsigned) (bid + 1) * (unsigned) P.G / (unsigned) nwg);
    const int ng = max(0, (g1 - g0 - wave + NW - 1) / NW);      // row groups of this wave
    if (NP > 0 && ng == 0) { __builtin_amdgcn_s_barrier(); __syncthreads(); return; }
    int gc = min(g0 + wave, P.G - 1);
    // the QKV epilogue's position, loaded here ahead of the prologue inputs (vmcnt retires in
    // order: the inputs' wait covers it), so that the RoPE pair can be loaded at a row group's
    // start (mv_pre_epi).  An atomic load: a plain one is sunk to its use; a scalar one sinks
    // too and then holds up the prologue's first barrier, whose lgkmcnt wait covers it.
    [[maybe_unused]] int pos0 = 0;
    if constexpr (EPI == EPI_QKV)
        pos0 = __hip_atomic_load((const __attribute__((address_space(1))) int *) &P.sp->n_past, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);

    // NP == 0: the compute waves build the activation table themselves; its
    // inputs are issued first (vmcnt retires in order)
    constexpr int NT = NW * 64;
    constexpr bool FPRO = (PRO == PRO_NORM || PRO == PRO_ACTF);
    constexpr int UM = NP > 0 ? 1 : (FPRO ? (nunits + NT - 1) / NT : (nb + NT - 1) / NT);
    float4 xv[UM][2];
    float4 gv[UM][2];
    uint4 qv[UM];
    float dv[UM];
    if constexpr (NP == 0) {
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
    }

    // the prologue inputs, marked landed where the wait count is exact (matvec_common.h):
    // hipcc then waits for exactly them, never for weight loads issued behind them
    auto launder_inputs = [&]() __attribute__((always_inline)) {
        if constexpr (NP == 0) {
#pragma unroll
            for (int k = 0; k < UM; ++k) {
                if constexpr (FPRO) {
                    launder(xv[k][0]); launder(xv[k][1]);
                    if constexpr (PRO == PRO_NORM) { launder(gv[k][0]); launder(gv[k][1]); }
                } else {
                    launder(qv[k]); launder(dv[k]);
                }
            }
        }
    };

    // first D chunks of this wave's first row group (wave-uniform base +
    // 32-bit lane offset: the scalar-base load form).  A wave without row groups (it only
    // helps build the table) issues the same loads with every lane on one 16-byte word:
    // no branch around the issue, so hipcc's wait counts stay exact on every path.
    const bool issue = NP > 0 || ng > 0;
    const uint32_t loff = issue ? (uint32_t) lane * 16u : 0u;
    uint4 W[D][4];
    float4 S[D];
    // the scales of a chunk go out before its nibbles: the scale table of chunk c+1 is
    // built while chunk c's nibbles may still be in flight (vmcnt retires in order).  Scales
    // and nibbles are both read once per token: nt loads, all of them (a plain scale load is
    // also free to sink behind the chunk's nt nibble loads, which hipcc did; with plain
    // scales in the Wo matvec alone the next attention launch measured 0.15-0.3 us slower,
    // profiles/nt_helpers_decode_speed.json)
#define LVK_ISSUE(slot, grp, cc)                                                                        \
    do {                                                                                                \
        const uint4 * nb_ = P.nib + ((size_t) (grp) * NC * 4 + (cc) * 4) * 64;                          \
        S[slot] = ld_nt((const float4 *) ((const char *) (P.scl + ((size_t) (grp) * NC + (cc)) * 64) + loff)); \
        _Pragma("unroll") for (int sb = 0; sb < 4; ++sb) if ((cc) * 4 + sb < nsub)                      \
            W[slot][sb] = ld_nt((const uint4 *) ((const char *) (nb_ + sb * 64) + loff));               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
    } while (0)
    // Order of the prologue and the first weight loads: PF (PfOrder).
    // A CU's texture unit takes a 1 KiB wave load in ~16 cycles: issuing 80-160 KiB of
    // weights keeps every wave of the CU in its issue for 1.3-4k cycles, so with
    // PF_ISSUE_FIRST or PF_INPUTS_LAND the table (and the first chain) waits for the wave's own
    // share of the burst to be issued.
    static_assert(PF == PF_ISSUE_FIRST || PF == PF_INPUTS_LAND || PF == PF_TABLE_FIRST || PF == PF_SPLIT, "PfOrder");
    if constexpr (PF != PF_ISSUE_FIRST) launder_inputs();
    // prologue waves (NP > 0): the weight burst goes out behind their inputs (barrier A)
    if constexpr (NP > 0) __builtin_amdgcn_s_barrier();
    LVK_T(58);
    if constexpr (PF == PF_ISSUE_FIRST || PF == PF_INPUTS_LAND) {
#pragma unroll
        for (int d = 0; d < D; ++d) LVK_ISSUE(d, gc, d);
    } else if constexpr (PF == PF_SPLIT) {
        LVK_ISSUE(0, gc, 0);
    }
    if constexpr (PF == PF_ISSUE_FIRST) launder_inputs();
    LVK_T(59);

    if constexpr (NP == 0) {
        double * red = (double *) (sbuf + NW * 2 * SPL); // NW doubles (after the s buffers)
        if constexpr (FPRO) {
            float scale = 1.0f;
            if constexpr (PRO == PRO_NORM) {
                // per-thread units, a DPP wave tree, then the NW wave sums in order
                // (RMSNorm order)
                double acc = pro_sumsq_units<NT>(xv, nunits, tid);
                acc = wave_sum_d(acc);
                if (lane == 0) red[wave] = acc;
                __syncthreads();
                LVK_T(60);
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
    }
    if constexpr (PF == PF_TABLE_FIRST) {
#pragma unroll
        for (int d = 0; d < D; ++d) LVK_ISSUE(d, gc, d);
    }
    LVK_T(1);
    __syncthreads();            // activation table ready
    LVK_T(2);
    if (NP == 0 && ng == 0) return;
    if constexpr (PF == PF_SPLIT) {
#pragma unroll
        for (int d = 1; d < D; ++d) LVK_ISSUE(d, gc, d);
    }

    // 4. row groups: chunk loop with cross-group prefetch.  Per chunk: the chunk's
    // activation words and scale products are read from LDS together up front (one exposed
    // LDS latency per chunk instead of one per 4 blocks), the chains run, the slot is
    // refilled, and the scale products of the NEXT chunk are written to the other table
    // buffer (s = dw * dx, ggml.c:1968), so no write -> read round trip precedes a chain.
    float * sw = sbuf + wave * 2 * SPL;
    int tbuf = 0;
    auto make_table = [&](int buf, const float4 & Sv, int cc) __attribute__((always_inline)) {
        const float4 dx = *(const float4 *) (dxp + cc * 32 + j * 4);
        float4 sv;
        sv.x = Sv.x * dx.x; sv.y = Sv.y * dx.y; sv.z = Sv.z * dx.z; sv.w = Sv.w * dx.w;
        *(float4 *) (sw + buf * SPL + r * SRS + j * 4) = sv;
    };
    auto body = [&](auto has_next, int grp, int gnext) __attribute__((always_inline)) {
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int slot = c % D;
            LVK_T(tq); ++tq;
            constexpr int NQ = 8;                   // 4-block activation groups per chunk
#ifdef LVK_PROBE_NOCOMPUTE   // dev probe builds only: consume the weights trivially
            acc += __uint_as_float(W[slot][0].x ^ W[slot][nsub > 1 ? 1 : 0].y) * S[slot].x;
            if (false) {
#else
            {
#endif
            const float * sl = sw + tbuf * SPL;
            uint4 A[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (c * 4 + q / 2 < nsub) A[q] = *(const uint4 *) (act + ((c * 8 + q) * 8 + j) * 4);
            float sa[8][4];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float4 v = *(const float4 *) (sl + r * SRS + jj * 4);
                sa[jj][0] = v.x; sa[jj][1] = v.y; sa[jj][2] = v.z; sa[jj][3] = v.w;
            }
#pragma unroll
            for (int sb = 0; sb < 4; ++sb) {
                if (c * 4 + sb < nsub) {
                    const uint32_t wd[4] = {W[slot][sb].x, W[slot][sb].y, W[slot][sb].z, W[slot][sb].w};
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) {
                        const int bi = sb * 8 + pp * 4;
                        const uint4 a = A[sb * 2 + pp];
                        const int p0 = dot8(wd[2 * pp], a.x);
                        const int p1 = dot8(wd[2 * pp], a.y);
                        const int p2 = dot8(wd[2 * pp + 1], a.z);
                        const int p3 = dot8(wd[2 * pp + 1], a.w);
                        acc = __builtin_fmaf(sa[(bi + 0) & 7][(bi + 0) >> 3], (float) p0, acc);
                        acc = __builtin_fmaf(sa[(bi + 1) & 7][(bi + 1) >> 3], (float) p1, acc);
                        acc = __builtin_fmaf(sa[(bi + 2) & 7][(bi + 2) >> 3], (float) p2, acc);
                        acc = __builtin_fmaf(sa[(bi + 3) & 7][(bi + 3) >> 3], (float) p3, acc);
                    }
                }
            }
            }
            if (c + D < NC) LVK_ISSUE(slot, grp, c + D);
            else if constexpr (decltype(has_next)::value && XG) LVK_ISSUE(slot, gnext, c + D - NC);
            // the next chunk's scale table: chunk c+1 of this group, or chunk 0 of the next
            // (its scales sit in slot (c+1) % D either way)
            if (c + 1 < NC) make_table(tbuf ^ 1, S[(c + 1) % D], c + 1);
            else if constexpr (decltype(has_next)::value) make_table(tbuf ^ 1, S[(c + 1) % D], 0);
            __builtin_amdgcn_wave_barrier();
            tbuf ^= 1;
            // keep chunks in program order: the chain value is pinned here, so
            // chunk c's arithmetic cannot sink below chunk c+1's reads
            asm volatile("" : "+v"(acc));
            LVK_T(tq); ++tq;
            __builtin_amdgcn_sched_barrier(0);
        }
        return octet_reduce(acc);
    };

    make_table(0, S[0], 0);                 // chunk 0 of the first group
    __builtin_amdgcn_wave_barrier();
    // a row group: its epilogue's memory operand goes out before its chunk loop (mv_pre_epi)
    if constexpr (XG) {
        for (int k = 0; k + 1 < ng; ++k) {
            const EpiPre pe = mv_pre_epi<EPI>(P, gc * 8 + r, pos0);
            const float res = body(std::true_type{}, gc, gc + NW);
            mv_epilogue<EPI>(P, gc, r, j, res, pos0, pe);
            gc += NW;
        }
    }
    const EpiPre pe = mv_pre_epi<EPI>(P, gc * 8 + r, pos0);
    const float res = body(std::false_type{}, gc, gc);
    mv_epilogue<EPI>(P, gc, r, j, res, pos0, pe);
    LVK_T(3);
#undef LVK_ISSUE
}

template <int NW, int NP, int D, int PRO, int EPI, int KT, int PF>
__global__ __launch_bounds__((NW + NP) * 64) void k_mv_cu(CuParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    mv_cu_run<NW, NP, D, PRO, EPI, KT, PF>(P, blockIdx.x, gridDim.x, smem);
}

// -- host -------------------------------------------------------------------

// prologue order (k_mv_cu PF): PFD per launch shape (measured, tools/probe sweeps); the sweep
// probe build (LVK_PROBE_SWEEP) reads LVK_MV_PF (a PfOrder value) to override it for A/B runs, the
// product library carries only the shipped order
#ifdef LVK_PROBE_SWEEP
static int mv_pf_env() {
    static const int v = [] { const char * e = getenv("LVK_MV_PF"); return e ? atoi(e) : -1; }();
    return v;
}
#endif

template <int NW, int NP, int D, int PRO, int EPI, int KT, int PFD = PF_TABLE_FIRST>
hipError_t go(const CuParams & P, hipStream_t s) {
    constexpr int nb = KT / 32, NC = (nb + 31) / 32;
    constexpr bool XG = (NC % D) == 0;
    const int nwg = std::min(cu_count(), P.G);
    // without cross-group prefetch every wave must own at most one group
    if (!XG && (P.G + nwg - 1) / nwg > NW) return hipErrorNotSupported;
    const size_t lds = (size_t) nb * 32 + NC * 128 + NW * 2 * SPL * 4 + NW * 8;
#ifdef LVK_PROBE_SWEEP
    const int pf = mv_pf_env() >= 0 ? mv_pf_env() : PFD;
    switch (pf) {
        case PF_ISSUE_FIRST: LVK_LAUNCH((k_mv_cu<NW, NP, D, PRO, EPI, KT, PF_ISSUE_FIRST>), dim3(nwg), dim3((NW + NP) * 64), lds, s, P); break;
        case PF_INPUTS_LAND: LVK_LAUNCH((k_mv_cu<NW, NP, D, PRO, EPI, KT, PF_INPUTS_LAND>), dim3(nwg), dim3((NW + NP) * 64), lds, s, P); break;
        case PF_TABLE_FIRST: LVK_LAUNCH((k_mv_cu<NW, NP, D, PRO, EPI, KT, PF_TABLE_FIRST>), dim3(nwg), dim3((NW + NP) * 64), lds, s, P); break;
        case PF_SPLIT: LVK_LAUNCH((k_mv_cu<NW, NP, D, PRO, EPI, KT, PF_SPLIT>), dim3(nwg), dim3((NW + NP) * 64), lds, s, P); break;
        default: return hipErrorInvalidValue;
    }
#else
    LVK_LAUNCH((k_mv_cu<NW, NP, D, PRO, EPI, KT, PFD>), dim3(nwg), dim3((NW + NP) * 64), lds, s, P);
#endif
    return hipGetLastError();
}

}  // namespace

// CUs of the current device, cached per device id (a one-process layer split may drive
// devices of different sizes or CU-masked partitions)
int cu_count() {
    constexpr int MAXDEV = 64;
    static int n[MAXDEV] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev < 0 || dev >= MAXDEV) dev = 0;
    if (n[dev] == 0) {
        int v = 0;
        n[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    return n[dev];
}

#ifdef LVK_PROBE_TIMING
void * lvk_probe_trace() { void * p = nullptr; (void) hipGetSymbolAddress(&p, HIP_SYMBOL(g_trace)); return p; }
#endif
// row lengths compiled in: the LLaMA 7B/13B-free Q4_0 shapes (n_embd 4096 / 8192,
// n_ff 11008 / 22016; llama.cpp:771-779)
bool matvec_cu_supported(int K, int qtype) {
    if (qtype == Q4_1) return matvec_cu41_supported(K);
    if (qtype == F16 || qtype == F32) return true;      // matvec_f16.hip / matvec_f32.hip take every row length
    return K == 4096 || K == 11008 || K == 8192 || K == 22016;
}

hipError_t launch_matvec_cu(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    if (L.w.qtype == Q4_1) return launch_matvec_cu41(L, pro, epi, s);
    if (L.w.qtype == F16) return launch_matvec_f16(L, pro, epi, s);
    if (L.w.qtype == F32) return launch_matvec_f32(L, pro, epi, s);
    if (L.w.qtype != Q4_0 || L.n_tokens != 1 || L.w.M % 8) return hipErrorNotSupported;
    if (!mv_inputs_set(L, pro)) return hipErrorInvalidValue;
    CuParams P{};
    mv_fill(P, L, true);
    P.nib = L.w.nib;
    P.scl = (const float4 *) L.w.scl;
    P.G = L.w.M / 8;
    const int K = L.w.K;
#ifdef LVK_PROBE_SWEEP   // dev probe builds only: LVK_CFG selects a launch shape
    {
        static int cfg = getenv("LVK_CFG") ? atoi(getenv("LVK_CFG")) : 0;
#define SW4(E, PR, K_, a0, a1, a2, a3)                                                          \
        switch (cfg) { case 0: return go<a0, PR, E, K_>(P, s); case 1: return go<a1, PR, E, K_>(P, s); \
                       case 2: return go<a2, PR, E, K_>(P, s); default: return go<a3, PR, E, K_>(P, s); }
#define C3(a, b, c) a, b, c
        if (K == 4096 && epi == EPI_QKV) SW4(EPI_QKV, PRO_NORM, 4096, C3(8, 0, 2), C3(8, 0, 4), C3(12, 0, 2), C3(6, 0, 4))
        if (K == 4096 && epi == EPI_SWIGLU_F32) SW4(EPI_SWIGLU_F32, PRO_NORM, 4096, C3(12, 0, 2), C3(12, 0, 4), C3(16, 0, 2), C3(8, 0, 4))
        if (K == 4096 && epi == EPI_STORE) SW4(EPI_STORE, PRO_NORM, 4096, C3(16, 0, 2), C3(16, 0, 4), C3(12, 0, 4), C3(8, 0, 4))
        if (K == 4096 && epi == EPI_RESID) SW4(EPI_RESID, PRO_ACTQ, 4096, C3(2, 0, 2), C3(2, 0, 4), C3(4, 0, 2), C3(4, 0, 4))
        if (K == 11008) SW4(EPI_RESID, PRO_ACTF, 11008, C3(2, 6, 4), C3(2, 6, 2), C3(2, 10, 4), C3(2, 4, 4))
        if (K == 22016 && epi == EPI_RESID) SW4(EPI_RESID, PRO_ACTF, 22016, C3(4, 0, 2), C3(4, 12, 2), C3(4, 4, 2), C3(4, 8, 2))
    }
#endif
    // launch shapes (waves NW, prefetch depth D) per row length and role, measured on
    // the 7B shapes (tools/probe, LVK_PROBE_SWEEP) and scaled for 65B: enough waves that
    // every CU keeps ~60-120 KB of weights in flight
    if (K == 4096) {
        switch (epi) {
            // PF_SPLIT (inputs, chunk 0, table, the rest after the barrier): QKV 7.6 vs
            // 7.7-8.4 us, Wo 4.4 vs 4.5-4.9 over orders 0-2 (profiles/r03_pf_sweep.txt)
            case EPI_QKV: if (pro == PRO_NORM) return go<8, 0, 2, PRO_NORM, EPI_QKV, 4096, PF_SPLIT>(P, s); break;
            case EPI_SWIGLU_F32: if (pro == PRO_NORM) return go<12, 0, 2, PRO_NORM, EPI_SWIGLU_F32, 4096, PF_SPLIT>(P, s); break;
            case EPI_STORE: if (pro == PRO_NORM) return go<16, 0, 2, PRO_NORM, EPI_STORE, 4096, PF_INPUTS_LAND>(P, s); break;
            case EPI_RESID:
                if (pro == PRO_ACTQ) return go<2, 0, 2, PRO_ACTQ, EPI_RESID, 4096, PF_SPLIT>(P, s);
                break;
        }
        // operator API (lvk_mul_mat_q: plain quantize of an f32 input)
        if (epi == EPI_STORE && pro == PRO_ACTF) return go<8, 0, 2, PRO_ACTF, EPI_STORE, 4096>(P, s);
    } else if (K == 8192) {
        switch (epi) {
            // prologue orders on the 65B shapes (round-3 sweep, profiles/r03_pf65.txt): 0 for
            // QKV / W1|W3 (22.4 / 38.6 vs 23.1 / 40.1 us at order 2), 5 for Wo (8.2 vs 8.4)
            case EPI_QKV: if (pro == PRO_NORM) return go<12, 0, 2, PRO_NORM, EPI_QKV, 8192, PF_ISSUE_FIRST>(P, s); break;
            case EPI_SWIGLU_F32: if (pro == PRO_NORM) return go<12, 0, 2, PRO_NORM, EPI_SWIGLU_F32, 8192, PF_ISSUE_FIRST>(P, s); break;
            case EPI_STORE: if (pro == PRO_NORM) return go<12, 0, 2, PRO_NORM, EPI_STORE, 8192>(P, s); break;
            case EPI_RESID: if (pro == PRO_ACTQ) return go<4, 0, 2, PRO_ACTQ, EPI_RESID, 8192, PF_SPLIT>(P, s); break;
        }
        if (epi == EPI_STORE && pro == PRO_ACTF) return go<8, 0, 2, PRO_ACTF, EPI_STORE, 8192>(P, s);
    } else if (K == 11008) {
        // 2 compute waves (one row group each) put the weight burst in flight at once, behind
        // the u loads of 6 prologue waves that quantize u meanwhile (tools/gpu_sweep_np.sh,
        // profiles/r03_np_sweep.txt: 7.0 us against 8.6-9.3 for 8 waves that all quantize u
        // and then issue the weights)
        if (epi == EPI_RESID && pro == PRO_ACTF) {
            // (needs at most 2 row groups per CU: a device with fewer CUs takes 8 waves that
            // all quantize u, then issue the weights)
            const hipError_t e = go<2, 6, 4, PRO_ACTF, EPI_RESID, 11008, PF_ISSUE_FIRST>(P, s);
            if (e != hipErrorNotSupported) return e;
            return go<8, 0, 4, PRO_ACTF, EPI_RESID, 11008, PF_TABLE_FIRST>(P, s);
        }
        if (epi == EPI_STORE && pro == PRO_ACTF) return go<4, 0, 4, PRO_ACTF, EPI_STORE, 11008>(P, s);
        if (epi == EPI_STORE && pro == PRO_NORM) return go<4, 0, 4, PRO_NORM, EPI_STORE, 11008>(P, s);
    } else if (K == 22016) {
        // 4 compute + 8 prologue waves (the 11008 rule): 20.0 vs 22.1 us (profiles/r03_sweep65.txt)
        if (epi == EPI_RESID && pro == PRO_ACTF) return go<4, 8, 2, PRO_ACTF, EPI_RESID, 22016, PF_ISSUE_FIRST>(P, s);
        if (epi == EPI_STORE && pro == PRO_ACTF) return go<4, 0, 2, PRO_ACTF, EPI_STORE, 22016>(P, s);
        if (epi == EPI_STORE && pro == PRO_NORM) return go<4, 0, 2, PRO_NORM, EPI_STORE, 22016>(P, s);
    }
    return hipErrorNotSupported;
}

}  // namespace lvk

LVK_RMS_ACCESSOR(lvk_probe_rms_mv)
