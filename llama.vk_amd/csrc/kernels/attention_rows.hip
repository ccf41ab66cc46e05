// attention_rows.hip -- one layer of a batched decode step (lvk_decode_batch): n rows, row i a
// single token of KV slot rows[i].slot at position rows[i].pos.  Each row is computed exactly as
// a single-token llama_eval at n_past = pos on that slot's cache would compute it
// (llama.cpp:996-1061): RoPE at pos, K / V appended at pos, attention over n_kv = pos + 1 with
// no position masked, every ggml_vec_dot_f16 over n_kv with its SIMD part n_kv & ~31 and its
// double tail.  (The reference's own N-token batch runs every column over n_past + N; rows of
// different sequences have no common n_past, so the single-token form is the definition.)
//
//   k_rope_kv_rows  k_rope_kv (mm_launch.hip) with the position and the cache per row
//   k_attn_rows     k_attn (attention.hip) on the f16 cache with the mask taken out and n_kv,
//                   K and V per row: grid (H, n, 2), a workgroup pair per (row, head); no
//                   workgroup waits on another
// f16 KV cache only.
#include "attention_common.h"
#include "lvk_kernels.h"
#include "matvec_common.h"

namespace lvk {

namespace {

constexpr int HD = ATTN_HD;

// RoPE mode 0 (ggml.c:7156-7227) + KV append (llama.cpp:996-1008) of the stored Q|K|V rows
// [n][3E] -> q16 [n][E], K [slot][layer][pos][E], V [slot][layer][E][pos]: the stores of
// k_rope_kv for that position
__global__ void k_rope_kv_rows(const float * __restrict__ qkv, int E, int hd, const float2 * __restrict__ rope,
                               const SeqRow * __restrict__ rows, const SeqSlot * __restrict__ slots, size_t layer_off,
                               int n_ctx, uint16_t * __restrict__ q16) {
    const int t = blockIdx.y;
    const int e2 = blockIdx.x * blockDim.x + threadIdx.x;     // pair index over Q|K (E/2 each) then V
    const SeqRow rw = rows[t];
    const int pos = rw.pos;
    const float * row = qkv + (size_t) t * 3 * E;
    if (e2 < E) {
        const int which = e2 / (E / 2);
        const int e = 2 * (e2 - which * (E / 2));
        const float x0 = row[which * E + e], x1 = row[which * E + e + 1];
        const int i0 = e % hd;
        const float2 cs = rope[(size_t) pos * (hd / 2) + (i0 >> 1)];
        const float a0 = x0 * cs.x, b0 = x1 * cs.y;
        const float o0 = a0 - b0;
        const float a1 = x0 * cs.y, b1 = x1 * cs.x;
        const float o1 = a1 + b1;
        if (which == 0) {
            kv_store(q16, (size_t) t * E + e, o0, 0);
            kv_store(q16, (size_t) t * E + e + 1, o1, 0);
        } else {
            uint16_t * kc = slots[rw.slot].kc + layer_off;
            kv_store(kc, (size_t) pos * E + e, o0, 0);
            kv_store(kc, (size_t) pos * E + e + 1, o1, 0);
        }
    } else if (e2 < E + E / 2) {
        const int e = 2 * (e2 - E);
        uint16_t * vc = slots[rw.slot].vc + layer_off;
        kv_store(vc, (size_t) e * n_ctx + pos, row[2 * E + e], 0);
        kv_store(vc, (size_t) (e + 1) * n_ctx + pos, row[2 * E + e + 1], 0);
    }
}

// ---------------------------------------------------------------------------
// One (row t, head h, half of the head dims), the phases of k_attn:
//   1  scores of every position p < n_kv into LDS (quad = one position)
//   2  softmax in LDS, P rounded to f16
//   3  P.V for HD/2 output dims (quad = one dim), V steps 0..15 through LDS by DMA
//   4  quantize the HD/2 outputs (HD/64 weight blocks) for Wo
// grid (H, n, 2), 256 threads.
// ---------------------------------------------------------------------------
template <int QT>
__global__ __launch_bounds__(256) void k_attn_rows(const uint16_t * __restrict__ q16, const SeqRow * __restrict__ rows,
                                                   const SeqSlot * __restrict__ slots, size_t layer_off,
                                                   const uint16_t * __restrict__ exp_tab, ActQ out, int E, int n_ctx,
                                                   float scale, float * __restrict__ out_f32, int exp_computed) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NSTEP = HD / 32;
    const int h = blockIdx.x, t = blockIdx.y, half = blockIdx.z;
    const SeqRow rw = rows[t];
    const int n_kv = rw.pos + 1;
    const uint16_t * __restrict__ kc = slots[rw.slot].kc + layer_off;
    const uint16_t * __restrict__ vc = slots[rw.slot].vc + layer_off;
    const int tid = threadIdx.x, lane = tid & 63, r = tid & 3;
    float * sc = (float *) smem;                                   // n_ctx scores / exp values
    uint16_t * p16 = (uint16_t *) (smem + (size_t) n_ctx * 4);     // n_ctx f16 probabilities
    float * red = (float *) (smem + (size_t) n_ctx * 6);           // 8 floats
    double * redd = (double *) (smem + (size_t) n_ctx * 6 + 32);   // 4 doubles

    // ---- all global loads first: Q, the first 512 positions of K (8 passes of 64 positions, a
    // lane quad per position) and of V (16 steps of 32 positions by DMA into LDS)
    constexpr int KP = 8, VS = 16, PB = KP * 64, VSB = 4096;
    uint4 qv[NSTEP];
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) qv[st] = *(const uint4 *) (q16 + (size_t) t * E + h * HD + st * 32 + r * 8);
    uint4 kv[KP][NSTEP];
    auto load_k = [&](int pb) {
#pragma unroll
        for (int ps = 0; ps < KP; ++ps) {
            if (pb + ps * 64 < n_kv) {          // wave-uniform: no duplicate requests past n_kv
                const int pp = min(pb + ps * 64 + (tid >> 2), n_kv - 1);
#pragma unroll
                for (int st = 0; st < NSTEP; ++st) kv[ps][st] = *(const uint4 *) (kc + (size_t) pp * E + h * HD + st * 32 + r * 8);
            }
        }
    };
    const int d = half * (HD / 2) + (tid >> 2);
    const size_t vrow = (size_t) (h * HD + d) * n_ctx;   // element offset of this thread's V row
    const int np = n_kv & ~31;
    const int nvs = (n_kv + 31) / 32;                  // V steps including a partial one (<= n_ctx / 32)
    uint8_t * vlds = smem + (size_t) n_ctx * 6 + 64;
    load_k(0);
    {
        uint8_t * vl = vlds + (tid & ~63) * 16;       // wave-uniform base; lane l lands at + 16 l
        const int nd = min(nvs, VS);
        for (int st = 0; st < nd; ++st)
            __builtin_amdgcn_global_load_lds((const void *) (vc + vrow + (size_t) st * 32 + r * 8),
                                             (__attribute__((address_space(3))) void *) (vl + st * VSB), 16, 0, 0);
    }

    // ---- phase 1: KQ (ggml_vec_dot_f16 over HD, Q in f16) ----
    for (int pb = 0; pb < n_kv; pb += PB) {
        if (pb > 0) load_k(pb);
#pragma unroll
        for (int ps = 0; ps < KP; ++ps) {
            if (pb + ps * 64 < n_kv) {
                float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int st = 0; st < NSTEP; ++st) {
                    float kf[8], qf[8];
                    unpack8h(kv[ps][st], kf);
                    unpack8h(qv[st], qf);
#pragma unroll
                    for (int l = 0; l < 8; ++l) s[l] = __builtin_fmaf(kf[l], qf[l], s[l]);
                }
                const float kq = quad_reduce(s);
                const int pp = pb + ps * 64 + (tid >> 2);
                if (r == 0 && pp < n_kv) sc[pp] = kq * scale;      // ggml_vec_scale_f32 (llama.cpp:1026)
            }
        }
    }
    __syncthreads();

    // ---- phase 2: softmax (ggml.c:7099-7121); no position is masked ----
    auto bar = [] { __syncthreads(); };
    float mx = -INFINITY;
    for (int p = tid; p < n_kv; p += 256) { const float v = sc[p]; mx = v > mx ? v : mx; }
    mx = wg_max_f(mx, red, bar);
    double sum = 0.0;   // exact in any order: every term is an fp16 value in [0,1]
    for (int p = tid; p < n_kv; p += 256) {
        const float v = sc[p];
        float e = 0.0f;
        if (v != -INFINITY) {
            e = f16_to_f32(exp_f16(f32_to_f16(v - mx), exp_tab, exp_computed));
            sum += (double) e;
        }
        sc[p] = e;
    }
    sum = wg_sum_d(sum, redd, bar);
    const float scl = (float) (1.0 / sum);
    const int n_pad = (n_kv + 31) & ~31;
    for (int p = tid; p < n_pad; p += 256) p16[p] = p < n_kv ? f32_to_f16(sc[p] * scl) : (uint16_t) 0;

    // ---- phase 3: KQV = ggml_vec_dot_f16(n_kv, V row, P) ----
    __syncthreads();     // vmcnt(0) + barrier: P is written and every wave's V DMA has landed
    const int nsteps = np / 32;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto pv_step = [&](const uint4 v8, int st) {
        float vf[8], pf[8];
        unpack8h(v8, vf);
        unpack8h(*((const uint4 *) (p16 + st * 32) + r), pf);
#pragma unroll
        for (int l = 0; l < 8; ++l) s[l] = __builtin_fmaf(vf[l], pf[l], s[l]);
    };
    const int nl = min(nsteps, VS);
    for (int st = 0; st < nl; ++st) pv_step(*((const uint4 *) (vlds + (size_t) st * VSB) + tid), st);
    for (int st = VS; st < nsteps; ++st) pv_step(*(const uint4 *) (vc + vrow + (size_t) st * 32 + r * 8), st);
    const float res = quad_reduce(s);
    float o = res;
    if (np < n_kv) {
        // leftovers in double, in position order (ggml.c:1806-1808), from registers
        const int ts = np / 32;
        uint4 vt[4], pt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pt[k] = *((const uint4 *) (p16 + np) + k);
            if (ts < VS) vt[k] = *((const uint4 *) (vlds + (size_t) ts * VSB) + (tid & ~3) + k);
        }
        if (ts >= VS)
#pragma unroll
            for (int k = 0; k < 4; ++k) vt[k] = *((const uint4 *) (vc + vrow + np) + k);
        if (r == 0) {
            const int nt_ = n_kv - np;
            double sumf = (double) res;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float vf[8], pf[8];
                unpack8h(vt[k], vf);
                unpack8h(pt[k], pf);
#pragma unroll
                for (int l = 0; l < 8; ++l)
                    if (8 * k + l < nt_) { const float pr = vf[l] * pf[l]; sumf += (double) pr; }
            }
            o = (float) sumf;
        }
    }
    if (r == 0 && out_f32) out_f32[(size_t) t * E + h * HD + d] = o;

    // ---- phase 4: quantize HD/2 outputs = HD/64 weight blocks ----
    __syncthreads();
    float * ob = sc;
    if (r == 0) ob[tid >> 2] = o;
    __syncthreads();
    if constexpr (QT == Q4_0) {
        if (tid < HD / 2) {      // wave 0: a 32-lane half per block
            float dd;
            uint4 qs;
            mv::q40_block32(ob[tid], lane, dd, qs);
            if ((lane & 31) == 0) mv::actq_store_block(out, t, (h * HD + half * (HD / 2)) / 32 + (tid >> 5), dd, qs);
        }
    }
    if constexpr (QT == Q4_1) {
        // quantize_row_q4_1 (ggml.c:847-920) of the HD/64 blocks staged in ob
        if (tid < HD / 16) {
            const int bb = tid >> 2, k = tid & 3;
            const int blk = (h * HD + half * (HD / 2)) / 32 + bb;
            float dd, mm;
            uint32_t qw;
            mv::q41_block_lds(ob + bb * 32, k, dd, mm, qw);
            mv::actq_store_block41(out, t, blk, k, dd, mm, qw);
        }
    }
}

}  // namespace

bool attention_rows_supported(int n_embd, int n_head, int n_ctx) {
    return n_head > 0 && n_embd == n_head * HD && n_ctx % 32 == 0 && n_ctx >= 128;
}

hipError_t launch_rope_kv_rows(const float * qkv, int n, int E, int hd, const float2 * rope, const SeqRow * rows,
                               const SeqSlot * slots, size_t layer_off, int n_ctx, uint16_t * q16, hipStream_t s) {
    if (n <= 0 || E % 2 || hd % 2 || !rows || !slots) return hipErrorInvalidValue;
    const int pairs = E + E / 2;
    LVK_LAUNCH(k_rope_kv_rows, dim3((pairs + 255) / 256, n), dim3(256), 0, s, qkv, E, hd, rope, rows, slots, layer_off,
               n_ctx, q16);
    return hipGetLastError();
}

hipError_t launch_attention_rows(const AttnLaunch & A, const SeqRow * rows, const SeqSlot * slots, size_t layer_off,
                                 hipStream_t s) {
    if (!attention_rows_supported(A.n_embd, A.n_head, A.n_ctx) || A.n_tokens <= 0 || A.kv32 || !rows || !slots)
        return hipErrorInvalidValue;
    if (A.out_qtype != Q4_0 && A.out_qtype != Q4_1) return hipErrorNotSupported;
    const float scale = attn_scale(A.n_embd, A.n_head);
    dim3 grid(A.n_head, A.n_tokens, 2);
    // scores, P16, reductions, then V steps 0..15 by DMA (4 KiB each)
    const size_t lds = (size_t) A.n_ctx * 6 + 64 + 16 * 4096;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    // more than the default 64 KiB of dynamic LDS: opted in per device and not stream-ordered,
    // so with every launch (as matvec_f32.hip does)
    const void * fn = A.out_qtype == Q4_1 ? (const void *) k_attn_rows<Q4_1> : (const void *) k_attn_rows<Q4_0>;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
    if (e != hipSuccess) return e;
    if (A.out_qtype == Q4_1)
        LVK_LAUNCH((k_attn_rows<Q4_1>), grid, dim3(256), lds, s, A.q16, rows, slots, layer_off, A.exp_tab, A.out, A.n_embd,
                   A.n_ctx, scale, A.out_f32, A.exp_computed);
    else
        LVK_LAUNCH((k_attn_rows<Q4_0>), grid, dim3(256), lds, s, A.q16, rows, slots, layer_off, A.exp_tab, A.out, A.n_embd,
                   A.n_ctx, scale, A.out_f32, A.exp_computed);
    return hipGetLastError();
}

}  // namespace lvk
