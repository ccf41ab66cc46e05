// mm_f32.hip -- batched (2 <= N tokens) W[M][K] . X for f32 weights on the f32 matrix cores,
// bit-identical to ggml_compute_forward_mul_mat_f32 (AVX2).
//
// v_mfma_f32_16x16x4_f32 is a k-ordered chain of four IEEE fmas per output on top of C (one
// rounding per product, no wider accumulation, subnormals kept): with its four k slots the
// steps 4s .. 4s+3 of chain l of ggml_vec_dot_f32 (f32_common.h), one instruction advances that
// chain of 16 rows x 16 tokens by four steps.  A wave owns one 16 x 16 output tile and all 32
// chains of it: 32 independent accumulator tiles of 4 registers.
//   A lane (i = lane % 16, k = lane / 16): W[row i][32 (4s + k) + l]
//   B lane (j = lane % 16, k = lane / 16): x[token j][32 (4s + k) + l]
//   D lane (j, q = lane / 16), register v: chain l of (row 4q + v, token j)
// One 16-byte load gives a lane its operand of four chains, eight give the 32 of a 4-step
// chunk: the weights come from the decode image (the eight loads consume the 128-byte segment
// of step 4s + k of row i), the activations from plain f32 rows [N][K].  After the last chunk
// the 32 chain values of an output sit in one lane and are reduced in the reference's order
// without shuffles.  Rows past M read the image's zero rows or a clamped row, tokens past N a
// clamped token; neither is stored.
// Measured and rejected: whole-line global loads staged through a
// swizzled, double-buffered LDS image shared by the workgroup's four waves -- 326.9 ms against
// this kernel's 235.6 ms on the 7B-shaped 512-token prompt.
#include "f32_common.h"
#include "mm_common.h"

namespace lvk {

namespace {
using namespace f32k;

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct MmParams {
    const uint4 * img;
    int M, K, G;
    const float * x;            // [N][K] f32 rows
    int N;
    float * y;                  // EPI_STORE / EPI_RESID [N][ldy];  EPI_SWIGLU_F32 u [N][M / 2]
    int ldy;
    const uint16_t * silu_tab;
};

constexpr int TM = 16, TN = 16;  // the wave's output tile

struct Chunk {
    uint4 a[8];
    float4 b[8];
};
__device__ __forceinline__ void load_chunk(Chunk & c, const uint4 * wp, const float4 * xp) {
#pragma unroll
    for (int u = 0; u < 8; ++u) c.a[u] = wp[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) c.b[u] = xp[u];
}
__device__ __forceinline__ void mfma_chunk(f32x4_t (&acc)[32], const Chunk & c) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        acc[4 * u + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(c.a[u].x), c.b[u].x, acc[4 * u + 0], 0, 0, 0);
        acc[4 * u + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(c.a[u].y), c.b[u].y, acc[4 * u + 1], 0, 0, 0);
        acc[4 * u + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(c.a[u].z), c.b[u].z, acc[4 * u + 2], 0, 0, 0);
        acc[4 * u + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(c.a[u].w), c.b[u].w, acc[4 * u + 3], 0, 0, 0);
    }
}

template <int EPI>
__global__ __launch_bounds__(256) void k_mm_f32(MmParams P) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int rt = blockIdx.y * 4 + wave;               // 16-row tile
    if (rt * TM >= P.M) return;                         // wave-uniform; the kernel has no barrier
    const int t0 = blockIdx.x * TN;
    const int ij = lane & 15, kq = lane >> 4;
    const int S = P.K / 32;                             // steps; S % 8 == 0
    // operand row and token of this lane, clamped into the image (its rows M .. 8G-1 are zero)
    // and into the N rows of x
    const int arow = min(rt * TM + ij, P.G * 8 - 1);
    const int btok = min(t0 + ij, P.N - 1);
    const uint4 * wp = P.img + ((size_t) (arow >> 3) * S + kq) * 64 + (arow & 7) * 8;
    const float4 * xp = (const float4 *) (P.x + (size_t) btok * P.K) + kq * 8;

    f32x4_t acc[32];
#pragma unroll
    for (int l = 0; l < 32; ++l) acc[l] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    const int nch = S / 4;
    Chunk c0, c1;
    load_chunk(c0, wp, xp);
    for (int s = 0; s < nch; s += 2) {                  // nch is even
        load_chunk(c1, wp + (size_t) (s + 1) * 4 * 64, xp + (s + 1) * 4 * 8);
        mfma_chunk(acc, c0);
        const int sn = s + 2 < nch ? s + 2 : s;         // the last prefetch re-reads a chunk
        load_chunk(c0, wp + (size_t) sn * 4 * 64, xp + sn * 4 * 8);
        mfma_chunk(acc, c1);
    }

    const int t = t0 + ij;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        // GGML_F32x8_REDUCE: chain l = 8a + e is AVX lane e of accumulator a
        float Sx[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float s01 = acc[e][v] + acc[8 + e][v];
            const float s23 = acc[16 + e][v] + acc[24 + e][v];
            Sx[e] = s01 + s23;
        }
        const float u0 = Sx[0] + Sx[4], u1 = Sx[1] + Sx[5], u2 = Sx[2] + Sx[6], u3 = Sx[3] + Sx[7];
        const float u01 = u0 + u1, u23 = u2 + u3;
        const float res = u01 + u23;
        const int row = rt * TM + 4 * kq + v;
        if constexpr (EPI == EPI_STORE) {
            if (t < P.N && row < P.M) P.y[(size_t) t * P.ldy + row] = res;
        } else if constexpr (EPI == EPI_RESID) {
            if (t < P.N && row < P.M) {
                float * yp = P.y + (size_t) t * P.ldy + row;
                *yp = res + *yp;                          // ggml_add(cur, inpSA) (llama.cpp:1071,1103)
            }
        } else if constexpr (EPI == EPI_SWIGLU_F32) {
            // rows 0-3 of an 8-row group are w1 rows 4grp .. 4grp+3, rows 4-7 the w3 rows: the
            // w3 partner of (kq even, v) is (kq + 1, v)
            const float a3 = __shfl_xor(res, 16);
            if (!(kq & 1) && t < P.N && row < P.M) {
                const float sl = f16_to_f32(P.silu_tab[f32_to_f16(res)]);   // ggml_vec_silu_f32 (ggml.c:2495)
                P.y[(size_t) t * P.ldy + (2 * rt + (kq >> 1)) * 4 + v] = sl * a3;   // ggml_mul (llama.cpp:1096)
            }
        }
    }
}

template <bool NORM>
__global__ __launch_bounds__(256) void k_act_f32p(const float * __restrict__ x, const float * __restrict__ g, int K,
                                                  float * __restrict__ out) {
    __shared__ double red[4];
    const size_t t = blockIdx.x;
    act_row_f32<256, NORM>(x + t * K, g, K, (float4 *) (out + t * K), red);
}

template <int EPI>
hipError_t go(const MmParams & P, hipStream_t s) {
    const dim3 grid((P.N + TN - 1) / TN, (P.M + 4 * TM - 1) / (4 * TM));
    if (grid.y > 65535) return hipErrorInvalidValue;
    LVK_LAUNCH((k_mm_f32<EPI>), grid, dim3(256), 0, s, P);
    return hipGetLastError();
}

}  // namespace

hipError_t act_f32(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s) {
    if (g) LVK_LAUNCH((k_act_f32p<true>), dim3(N), dim3(256), 0, s, x, g, K, (float *) out.xm);
    else LVK_LAUNCH((k_act_f32p<false>), dim3(N), dim3(256), 0, s, x, g, K, (float *) out.xm);
    return hipGetLastError();
}

hipError_t mm_f32(const MmLaunch & L, int epi, hipStream_t s) {
    const QMatrix & w = L.w;
    if (epi != EPI_STORE && w.M % 8) return hipErrorInvalidValue;
    MmParams P{};
    P.img = w.nib; P.M = w.M; P.K = w.K; P.G = (w.M + 7) / 8;
    P.x = (const float *) L.x.xm; P.N = L.N; P.y = L.y; P.ldy = L.ldy; P.silu_tab = L.silu_tab;
    return mm_epi_dispatch<F32>(epi, [&](auto e) { return go<decltype(e)::value>(P, s); });
}

}  // namespace lvk
