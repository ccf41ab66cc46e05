// attention_prompt_long.hip -- the prompt-batch attention (N > 1 tokens, f16 KV cache) for
// contexts of up to 2048 positions, bit-faithful to the reference graph (llama.cpp:1010-1061)
// like attention_prompt.hip, whose LDS windows (a whole V slice and T whole score rows of n_ctx
// positions) stop at n_ctx 1024.  Here nothing in LDS is sized by n_ctx:
//
//   k_attn_l_scores  grid (H, ceil(N/T)/2): a pair of mirrored T-token blocks per workgroup.  The
//                    four waves split the 64-position K tiles (wave w: tiles w, w+4, ..), each
//                    tile fetched once per workgroup and applied to all T tokens; the score rows
//                    in LDS are as long as the launch's n_past + N (rounded up to 32), not n_ctx.
//                    T = 16 while such a row is at most 1024 positions, 8 beyond: two workgroups
//                    (two waves per SIMD) fit a CU either way.  Softmax and the f16 P store are
//                    k_attn_p_scores'.
//   k_attn_l_pv      grid (H, ceil(N/32), HD/32), longest blocks first: V rows of one 32-dim slice
//                    and P of 32 tokens go through LDS in tiles of PV_TILE positions, double
//                    buffered (the next tile's global loads are in flight under the current
//                    tile's dots); the 32 accumulators of every (dim, token) dot stay in registers
//                    across the tiles and take the 32-position steps in ascending order, so the
//                    tiled sum is the untiled one bit for bit.  Tail: attn_pv_tail.
#include "attention_common.h"

#include <cstdlib>

namespace lvk {

namespace {

constexpr int HD = ATTN_HD;
constexpr int PV_TILE = 256;              // positions per P.V tile: a multiple of 32, <= 512
constexpr int PV_LD = PV_TILE + 8;        // LDS row pitch in f16: 16 bytes of padding shift the rows' banks
constexpr int SC_LONG = 1024;             // score rows longer than this: 8 tokens per block instead of 16

// ---------------------------------------------------------------------------
// scores + softmax.  A workgroup (4 waves) owns one head and two T-token blocks, the block
// nblk-1-y and its mirror y, one after the other, so every workgroup has about the same count of
// causal K tiles.  Wave w takes the 64-position tiles w, w+4, .. of the block: a lane owns position
// p = pb + lane, its K row packed in 64 VGPRs with the wave's next tile in flight, and runs for each
// of the block's tokens (Q broadcast from LDS) the 32 AVX accumulators of ggml_vec_dot_f16 with
// v_fma_mix, then the F32Cx8 reduce in registers -- k_attn_p_scores' arithmetic; what differs is
// that a K tile is read once per workgroup and used T times (there: once per wave, T/4 times).
// ld: the pitch of the LDS score rows, >= (n_past + N) rounded up to 32 (the launcher's).
// ---------------------------------------------------------------------------
template <int T, int EM>
__global__ __launch_bounds__(256) void k_attn_l_scores(const uint16_t * __restrict__ q16, const uint16_t * __restrict__ kc,
                                                       const uint16_t * __restrict__ exp_tab, const StepParams * sp,
                                                       int E, int n_ctx, int ld, float scale, uint16_t * __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int n_past = sp->n_past, N = sp->n_tokens;
    const int n_kv = n_past + N;
    const int n_pad = (n_kv + 31) & ~31;
    if (n_pad > ld || n_kv > n_ctx) return;                   // the rows would not fit: nothing is touched
    const int nblk = (N + T - 1) / T;
    const int h = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint4 * qs = (uint4 *) smem;                              // [T][16] uint4: Q rows (f16)
    float * sc = (float *) (smem + T * 256);                  // [T][ld] scores, then exp values

    for (int ph = 0; ph < 2; ++ph) {
        const int b = ph == 0 ? nblk - 1 - (int) blockIdx.y : (int) blockIdx.y;
        if (b < 0) break;                                     // a grid larger than the step block's N
        if (ph == 1) {
            if (b >= nblk - 1 - b) break;                    // odd block count: the middle block alone
            __syncthreads();                                  // the first block's rows are read out
        }
        const int t0 = b * T;
        const int nt = min(T, N - t0);
        const int lim_hi = n_past + t0 + nt - 1;              // last unmasked position of the block
        for (int i = tid; i < T * 16; i += 256) {
            const int t = i >> 4;
            qs[i] = t < nt ? *((const uint4 *) (q16 + (size_t) (t0 + t) * E + h * HD) + (i & 15)) : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();

        auto load = [&](uint4 (&kr)[16], int pb) {
            const uint4 * kp = (const uint4 *) (kc + (size_t) min(pb + lane, lim_hi) * E + h * HD);
#pragma unroll
            for (int i = 0; i < 16; ++i) kr[i] = kp[i];
        };
        auto tile = [&](const uint4 (&kr)[16], int pb) {
            const int p = pb + lane;
            const bool live = p <= lim_hi;
            // nt >= 1: the first pass consumes the tile's loads, so the compiler knows them done
            // when the registers are reloaded
            int t = 0;
            do {
                // accumulator (j, l) of ggml_vec_dot_f16 (ggml.c:1781-1815): elements 32 st + 8 j + l,
                // st = 0..3 in order; uint4 4 st + j holds the 8 of (st, j), word w elements 2w, 2w + 1
                float acc[4][8];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int l = 0; l < 8; ++l) acc[j][l] = 0.0f;
#pragma unroll
                for (int st = 0; st < 4; ++st) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint4 q = qs[t * 16 + 4 * st + j];          // wave-uniform: an LDS broadcast
                        const uint4 k = kr[4 * st + j];
                        const uint32_t qw[4] = {q.x, q.y, q.z, q.w}, kw[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            acc[j][2 * w] = fma_mix_hh<0, 0>(kw[w], qw[w], acc[j][2 * w]);
                            acc[j][2 * w + 1] = fma_mix_hh<1, 1>(kw[w], qw[w], acc[j][2 * w + 1]);
                        }
                    }
                }
                // F32Cx8 reduce: accumulator j plays the AVX register j (quad_reduce order)
                float S[8];
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    const float a = acc[0][l] + acc[1][l], c = acc[2][l] + acc[3][l];
                    S[l] = a + c;
                }
                const float kq = f32cx8_hsum(S);
                if (live) sc[t * ld + p] = p <= n_past + t0 + t ? kq * scale : -INFINITY;
                ++t;
            } while (t < nt);
        };
        if (64 * wave <= lim_hi) {
            // the wave's tiles in pairs, its next tile's K loads always in flight (rows clamped
            // to lim_hi): one loop exit, and a skipped second tile drains its loads itself, so the
            // compiler's wait before each tile's first use counts only that tile's loads
            uint4 ka[16], kb[16];
            load(ka, 64 * wave);
            for (int pb = 64 * wave; pb <= lim_hi; pb += 512) {
                load(kb, pb + 256);
                tile(ka, pb);
                load(ka, pb + 512);
                if (pb + 256 <= lim_hi) tile(kb, pb + 256);
                else __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
            }
        }
        __syncthreads();

        // ---- softmax per token row (ggml.c:7099-7121); wave w owns rows w, w+4, ... ----
        for (int t = wave; t < nt; t += 4) {
            float * row = sc + t * ld;
            const int lim = n_past + t0 + t;
            // positions lim+1 .. n_kv-1 are -inf (ggml.c:7028-7031): max over the live ones
            float mx = -INFINITY;
            for (int p = lane; p <= lim; p += 64) { const float v = row[p]; mx = v > mx ? v : mx; }
            mx = wave_max_f(mx);
            double sum = 0.0;      // exact in any order: every term is an fp16 value in [0,1]
            for (int p = lane; p <= lim; p += 64) {
                const float e = f16_to_f32(exp_softmax<EM>(f32_to_f16(row[p] - mx), exp_tab));
                sum += (double) e;
                row[p] = e;
            }
            sum = wave_sum_d(sum);
            const float scl = (float) (1.0 / sum);
            // P rounded to f16 (the mul_mat's src1 conversion), two positions per lane
            uint32_t * prow = (uint32_t *) (P + ((size_t) h * N + t0 + t) * n_ctx);
            for (int p = 2 * lane; p < n_pad; p += 128) {
                const uint32_t lo = p <= lim ? f32_to_f16(row[p] * scl) : 0u;
                const uint32_t hi = p + 1 <= lim ? f32_to_f16(row[p + 1] * scl) : 0u;
                prow[p >> 1] = lo | hi << 16;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// P.V for one 32-dim slice (one Q4 block of the merged heads) and 32 tokens.
// Quad (qd, qt): dims 4qd..4qd+3, tokens 4qt..4qt+3 of the slice / block; quad lane r holds the
// AVX register r (positions 8r..8r+7 of a step) of the quad's 16 dots: 128 accumulators a thread.
// Tile k holds positions PV_TILE k .. of the 32 V rows and the 32 P rows: 8 16-byte pieces a
// thread, fetched into registers before tile k-1's dots and stored to the other LDS buffer after
// them; one barrier per tile.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attn_l_pv(const uint16_t * __restrict__ vc, const uint16_t * __restrict__ P,
                                                   const StepParams * sp, int E, int n_ctx, ActQ out, uint2 * xm,
                                                   float * xda, float * __restrict__ out_f32, int q41,
                                                   uint4 * xs41) {
    __shared__ __attribute__((aligned(16))) uint16_t buf[2][64 * PV_LD];    // rows 0..31 V dims, 32..63 P tokens
    const int n_past = sp->n_past, N = sp->n_tokens;
    const int n_kv = n_past + N;
    if (n_kv > n_ctx) return;
    // the longest blocks (most causal steps) first, so the tail of the launch is short ones
    const int h = blockIdx.x, t0 = (gridDim.y - 1 - blockIdx.y) * 32, ds = blockIdx.z;
    const int nt = min(32, N - t0);
    if (nt < 1) return;
    const int tid = threadIdx.x, r = tid & 3, quad = tid >> 2;
    const int qd = quad & 7, qt = quad >> 3;
    const int n_pad = (n_kv + 31) & ~31;
    const int np = n_kv & ~31;
    const int lim_hi = n_past + t0 + nt - 1;
    const int nsteps = min(np, lim_hi + 1 + 31) / 32;        // steps holding at least one unmasked position
    const int nfill = min(n_pad, (lim_hi + 32) & ~31);        // positions any dot of the block reads
    const int ntile = (nfill + PV_TILE - 1) / PV_TILE;        // >= 1
    const int d0 = h * HD + ds * 32;

    // piece u of a thread: row (tid >> 5) + 8 u of the 64, positions 8 (tid & 31) .. +7 of the tile
    const int prow = tid >> 5, pc = tid & 31;
    auto fetch = [&](uint4 (&g)[8], int tile) {
        const int p = tile * PV_TILE + 8 * pc;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = prow + 8 * u;
            g[u] = make_uint4(0, 0, 0, 0);
            if (p < nfill) {
                if (u < 4) g[u] = *(const uint4 *) (vc + (size_t) (d0 + row) * n_ctx + p);
                else if (row - 32 < nt) g[u] = *(const uint4 *) (P + ((size_t) h * N + t0 + row - 32) * n_ctx + p);
            }
        }
    };
    auto stage = [&](const uint4 (&g)[8], int tile) {
        uint16_t * b = buf[tile & 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) *(uint4 *) (b + (prow + 8 * u) * PV_LD + 8 * pc) = g[u];
    };

    float s[4][4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int l = 0; l < 8; ++l) s[a][b][l] = 0.0f;

    uint4 g[8];
    fetch(g, 0);
    stage(g, 0);
    __syncthreads();
    for (int tile = 0; tile < ntile; ++tile) {
        const bool more = tile + 1 < ntile;
        if (more) fetch(g, tile + 1);
        const uint16_t * vl = buf[tile & 1];
        const uint16_t * pl = vl + 32 * PV_LD;
        const int st1 = min(nsteps, (tile + 1) * (PV_TILE / 32));
        for (int st = tile * (PV_TILE / 32); st < st1; ++st) {
            // the f16 operands straight into v_fma_mix (converted exactly, one rounding = fmaf of the
            // converted values): no separate conversions
            const int o = (st - tile * (PV_TILE / 32)) * 32 + 8 * r;
            uint32_t vw[4][4], pw[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const uint4 v = *(const uint4 *) (vl + (4 * qd + a) * PV_LD + o);
                vw[a][0] = v.x; vw[a][1] = v.y; vw[a][2] = v.z; vw[a][3] = v.w;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint4 v = *(const uint4 *) (pl + (4 * qt + b) * PV_LD + o);
                pw[b][0] = v.x; pw[b][1] = v.y; pw[b][2] = v.z; pw[b][3] = v.w;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        s[a][b][2 * w] = fma_mix_hh<0, 0>(vw[a][w], pw[b][w], s[a][b][2 * w]);
                        s[a][b][2 * w + 1] = fma_mix_hh<1, 1>(vw[a][w], pw[b][w], s[a][b][2 * w + 1]);
                    }
        }
        if (more) {
            // the other buffer: last read in tile - 1's dots, which every thread left before the
            // barrier that ended that iteration
            stage(g, tile + 1);
            __syncthreads();
        }
    }
    // reduce + double leftovers (ggml.c:1806-1808), in position order.  When a token's limit
    // reaches np, nfill = n_pad = np + 32: the last tile staged is the one holding np .. n_kv-1
    const uint16_t * lv = buf[(ntile - 1) & 1];
    const int lo = np - (ntile - 1) * PV_TILE;
    float o[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float res = quad_reduce(s[a][b]);
            const int t = 4 * qt + b;
            const int lim = n_past + t0 + t;
            float v = res;
            if (np < n_kv && np <= lim && t < nt) {
                double sumf = (double) res;
                const uint16_t * vr = lv + (4 * qd + a) * PV_LD + lo;
                const uint16_t * pr = lv + (32 + t) * PV_LD + lo;
                for (int p = 0; p < n_kv - np; ++p) {
                    const float prod = f16_to_f32(vr[p]) * f16_to_f32(pr[p]);
                    sumf += (double) prod;
                }
                v = (float) sumf;
            }
            o[a][b] = v;
        }
    // ---- merged heads: this slice is one Q4 block per token ----
    __syncthreads();
    float * ob = (float *) buf[0];                             // [32 tokens][33]
    if (r == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) ob[(4 * qt + b) * 33 + 4 * qd + a] = o[a][b];
    }
    __syncthreads();
    attn_pv_tail(ob, nt, t0, d0, E, out, xm, xda, out_f32, q41, xs41);
}

}  // namespace

bool attention_prompt_long_supported(int n_embd, int n_head, int n_ctx) {
    return n_head >= 1 && n_embd == n_head * HD && n_ctx % 32 == 0 && n_ctx >= 32 && n_ctx <= 2048;
}

hipError_t launch_attention_prompt_long(const AttnLaunch & A, uint16_t * p_scratch, const ActImage & wo_image,
                                        hipStream_t s) {
    if (!attention_prompt_long_supported(A.n_embd, A.n_head, A.n_ctx) || A.n_tokens < 1 || A.n_tokens > A.n_ctx || A.kv32)
        return hipErrorNotSupported;
    // Q4_1 writes its MFMA operands (xm + xs) or nothing but the ActQ; Q4_0 xm + da
    void * const xm = wo_image.xm;
    float * const xda = wo_image.da;
    void * const xs41 = wo_image.xs;
    if (A.out_qtype == Q4_1 ? (xm != nullptr) != (xs41 != nullptr) || xda : A.out_qtype != Q4_0 || xs41 || (xm != nullptr) != (xda != nullptr))
        return hipErrorNotSupported;
    // the score rows' pitch: the launch's n_past + N where the caller knows it on the host
    const int n_kv = A.n_kv > 0 ? A.n_kv : A.n_ctx;
    if (n_kv < A.n_tokens || n_kv > A.n_ctx) return hipErrorInvalidValue;
    const int ld = (n_kv + 31) & ~31;
    const float scale = attn_scale(A.n_embd, A.n_head);
    EventSplit ev;
    ev.first();
    with_exp_mode(A.exp_computed, [&](auto em) {
        auto go = [&](auto tt) {
            constexpr int T = decltype(tt)::value;
            const size_t lds = (size_t) T * 256 + (size_t) T * ld * 4;
            const int nblk = (A.n_tokens + T - 1) / T;
            LVK_LAUNCH((k_attn_l_scores<T, em()>), dim3(A.n_head, (nblk + 1) / 2), dim3(256), lds, s, A.q16, A.kc,
                       A.exp_tab, A.sp, A.n_embd, A.n_ctx, ld, scale, p_scratch);
        };
        if (ld > SC_LONG) go(std::integral_constant<int, 8>{});
        else go(std::integral_constant<int, 16>{});
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ev.last();
    LVK_LAUNCH(k_attn_l_pv, dim3(A.n_head, (A.n_tokens + 31) / 32, HD / 32), dim3(256), 0, s, A.vc, p_scratch, A.sp,
               A.n_embd, A.n_ctx, A.out, (uint2 *) xm, xda, A.out_f32, A.out_qtype == Q4_1 ? 1 : 0, (uint4 *) xs41);
    return hipGetLastError();
}

}  // namespace lvk
