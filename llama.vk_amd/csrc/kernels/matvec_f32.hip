// matvec_f32.hip -- single-token W[M][K] . x for f32 weights, bit-identical to
// ggml_compute_forward_mul_mat_f32 (AVX2), plus the load-time repack of an f32 matrix into its
// step octet image (f32_common.h).
//
// One launch per matrix, the shape of k_matvec_f16.  A workgroup of NW waves stages the f32
// activation row in LDS (rms_norm * g for PRO_NORM, a copy for PRO_ACTF), then every wave
// streams one 8-row group: 1 KiB per global_load_dwordx4, D loads in flight per lane, 4
// v_fma_f32 per load against one ds_read_b128 of the row.  Purely bandwidth-bound; no workgroup
// waits on another.
//
// The staged row takes 4 K bytes.  Rows beyond 64 KiB of LDS (K = 17920, 22016: the 30B / 65B
// W2) run the same kernel: the launch opts it in to the dynamic LDS it needs
// (hipFuncSetAttribute; the CU has 160 KiB), for both prologues.
#include "f32_common.h"
#include "matvec_common.h"

namespace lvk {

namespace {
using namespace f32k;

struct F32Image {
    const uint4 * img;
    int M, K, G;                // G = row groups, ceil(M / 8)
};
struct F32Params : F32Image, mv::MvArgs {};

constexpr int D = 16;           // 16-byte weight loads in flight per lane (16 KiB per wave)
constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_MAX = 160 * 1024;

template <int NW, int PRO, int EPI>
__global__ __launch_bounds__(NW * 64) void k_matvec_f32(F32Params P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int c = lane & 7;
    const int r = lane >> 3;
    const int K = P.K;
    const int S = K / 32;                               // 16-byte units per lane and row
    const int grp = blockIdx.x * NW + wave;
    const bool live = grp < P.G;
    const int nfull = S / D, R = S - nfull * D;

    float4 * xs4 = (float4 *) smem;                     // 4 K bytes: the activation row
    double * red = (double *) (smem + (size_t) 4 * K);  // NW doubles

    // the first D weight loads go out ahead of the prologue (they never depend on x)
    const uint4 * wp = P.img + (size_t) (live ? grp : 0) * S * 64 + lane;
    uint4 W[D];
    if (nfull > 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) W[d] = ld_nt(wp + (size_t) d * 64);
    }

    act_row_f32<NW * 64, PRO == PRO_NORM>(P.x, P.g, K, xs4, red);
    if (!live) return;                                  // wave-uniform, after the last barrier

    const float4 * xs = xs4 + c;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int s0 = 0;
    if (nfull > 0) {
        for (int ch = 0; ch + 1 < nfull; ++ch, s0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                fma4(acc, W[d], xs[(s0 + d) * 8]);
                W[d] = ld_nt(wp + (size_t) (s0 + D + d) * 64);
            }
        }
        // last full chunk; the remainder (R < D units) is loaded behind it
#pragma unroll
        for (int d = 0; d < D; ++d) {
            fma4(acc, W[d], xs[(s0 + d) * 8]);
            if (d < R) W[d] = ld_nt(wp + (size_t) (s0 + D + d) * 64);
        }
        s0 += D;
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d < R) fma4(acc, W[d], xs[(s0 + d) * 8]);
    } else {
        for (int s = 0; s < S; ++s) fma4(acc, ld_nt(wp + (size_t) s * 64), xs[s * 8]);
    }

    const float res = chain_reduce(acc);
    // the epilogue's memory operand (RoPE pair, residual term) is loaded here, in the tail
    [[maybe_unused]] int pos0 = 0;
    if constexpr (EPI == EPI_QKV) pos0 = P.sp->n_past;
    const int row = grp * 8 + r;
    const mv::EpiPre pe = mv::mv_pre_epi<EPI>(P, row, pos0);
    mv::mv_epilogue<EPI>(P, grp, r, c, res, pos0, pe, row < P.M);
}

// file-layout f32 rows -> step octet image, one thread per 16-byte unit.  Rows past M (the last
// group of an M % 8 != 0 matrix) are zero.  interleave4: src holds two (M/2)-row matrices A
// then B; image rows are A0-3, B0-3, A4-7, ... (the fused W1|W3)
__global__ void k_repack_f32(const float * __restrict__ src, int M, int K, uint4 * __restrict__ img, int interleave4) {
    const int S = K / 32;
    const size_t total = (size_t) ((M + 7) / 8) * S * 64;
    const size_t o = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const int lane = (int) (o & 63);
    const size_t gs = o >> 6;
    const int s = (int) (gs % S);
    const int grp = (int) (gs / S);
    const int r = lane >> 3, c = lane & 7;
    int row = grp * 8 + r;
    if (interleave4) row = (r < 4 ? 0 : M / 2) + grp * 4 + (r & 3);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (grp * 8 + r < M) v = *(const uint4 *) (src + (size_t) row * K + (size_t) s * 32 + 4 * c);
    img[o] = v;
}

template <int NW, int PRO, int EPI>
hipError_t go(const F32Params & P, hipStream_t s) {
    const size_t lds = (size_t) 4 * P.K + NW * 8 + 16;
    if (lds > LDS_MAX) return hipErrorInvalidValue;
    if (lds > LDS_DEFAULT) {
        // per device and not stream-ordered, so it is set with every such launch
        const hipError_t e = hipFuncSetAttribute((const void *) k_matvec_f32<NW, PRO, EPI>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    LVK_LAUNCH((k_matvec_f32<NW, PRO, EPI>), dim3((P.G + NW - 1) / NW), dim3(NW * 64), lds, s, P);
    return hipGetLastError();
}

template <int PRO, int EPI>
hipError_t go_nw(const F32Params & P, hipStream_t s) {
    // waves per workgroup, the rule of matvec_f16.hip: 4 when that still gives every CU two
    // workgroups, else 2
    if (P.G >= 8 * cu_count()) return go<4, PRO, EPI>(P, s);
    return go<2, PRO, EPI>(P, s);
}

}  // namespace

hipError_t launch_repack_f32(const void * src_rows, int M, int K, uint4 * img, hipStream_t s, int interleave4) {
    if (K % 256 || M < 1 || (interleave4 && M % 8)) return hipErrorInvalidValue;
    const size_t n = (size_t) ((M + 7) / 8) * (K / 32) * 64;
    hipLaunchKernelGGL(k_repack_f32, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, (const float *) src_rows, M, K,
                       img, interleave4);
    return hipGetLastError();
}

hipError_t launch_matvec_f32(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    if (L.w.qtype != F32 || L.n_tokens != 1) return hipErrorNotSupported;
    if (L.w.K % 256 || L.w.M < 1) return hipErrorInvalidValue;
    if (epi != EPI_STORE && L.w.M % 8) return hipErrorInvalidValue;
    if (pro == PRO_ACTQ) return hipErrorNotSupported;       // f32 weights take f32 rows
    if (!mv::mv_inputs_set(L, pro)) return hipErrorInvalidValue;
    F32Params P{};
    mv::mv_fill(P, L, true);
    P.img = L.w.nib;
    P.M = L.w.M; P.K = L.w.K; P.G = (L.w.M + 7) / 8;
    if (pro == PRO_NORM) {
        switch (epi) {
            case EPI_STORE: return go_nw<PRO_NORM, EPI_STORE>(P, s);
            case EPI_QKV: return go_nw<PRO_NORM, EPI_QKV>(P, s);
            case EPI_SWIGLU_F32: return go_nw<PRO_NORM, EPI_SWIGLU_F32>(P, s);
        }
    } else if (pro == PRO_ACTF) {
        switch (epi) {
            case EPI_STORE: return go_nw<PRO_ACTF, EPI_STORE>(P, s);
            case EPI_RESID: return go_nw<PRO_ACTF, EPI_RESID>(P, s);
        }
    }
    return hipErrorNotSupported;
}

}  // namespace lvk
