// lvk_kernels.h -- host-visible launch interface of the llama.vk_amd HIP kernels.
//
// Every launcher is stream-ordered and capture-safe (no allocation, no sync),
// so the decode step can be recorded into one hipGraph.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

namespace lvk {

// Profiling hook: when a launcher runs with these set (one kernel per timed
// launch), the kernel is dispatched with hipExtLaunchKernelGGL and the two
// events are stamped by the command processor at its start and end -- the
// same interval rocprofv3's kernel trace reports.
struct LaunchEvents {
    hipEvent_t start = nullptr;
    hipEvent_t stop = nullptr;
};
extern thread_local LaunchEvents g_launch_events;
// a launcher of several kernels times them as one: the start event goes to the
// first kernel, the stop event to the last
struct EventSplit {
    LaunchEvents saved = g_launch_events;
    void first() { g_launch_events = {saved.start, nullptr}; }
    void last() { g_launch_events = {nullptr, saved.stop}; }
    ~EventSplit() { g_launch_events = saved; }
};

#define LVK_LAUNCH(kern, grid, block, lds, stream, ...)                                                        \
    do {                                                                                                       \
        if (::lvk::g_launch_events.start || ::lvk::g_launch_events.stop)                                  \
            hipExtLaunchKernelGGL(kern, grid, block, lds, stream, ::lvk::g_launch_events.start,                \
                                  ::lvk::g_launch_events.stop, 0, __VA_ARGS__);                                \
        else                                                                                                   \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                   \
    } while (0)

// = the model file's tensor type ids; F16 matrices use the paired-step octet image below, F32
// matrices the step octet image
enum QType : int { F32 = 0, F16 = 1, Q4_0 = 2, Q4_1 = 3 };

// error word: kernels whose workgroups wait on each other spin with a bound; a
// spin that gives up stores one of these into the context's host-mapped error
// word (system scope) instead of hanging, and the host fails the eval
enum DevError : unsigned { LVK_ERR_NONE = 0, LVK_ERR_ATTN_SPIN = 1, LVK_ERR_DECODE_SPIN = 2 };

// ---------------------------------------------------------------------------
// Device weight image of one quantized matrix W[M][K] (ggml row-major, K = row
// length) in the "octet" layout: rows are grouped 8 per
// wavefront; lane l = 8*r + j owns row r of the group and the AVX2 accumulator
// chain j of the reference dot product (ggml.c:1950-2026).  NC = ceil(K/1024).
//   nib : [M/8][NC][4][64] uint4   -- nibble slices of 8 blocks per uint4
//   scl : [M/8][NC][64]   float4  -- d of blocks 32c+8m+j, m = 0..3
// Bytes per row equal the file's (20 B per 32 weights; the last chunk of a
// row is zero-padded to 32 blocks when K % 1024 != 0 and never streamed).
// F16 matrices: nib is the paired-step octet image [ceil(M/8)][K/64][64] uint4
// (f16_common.h; f16_image_bytes, launch_repack_f16), scl is unused.
// F32 matrices: nib is the step octet image [ceil(M/8)][K/32][64] uint4 (f32_common.h;
// f32_image_bytes, launch_repack_f32), scl is unused.
struct QMatrix {
    int qtype = Q4_0;
    int M = 0, K = 0;
    const uint4 * nib = nullptr;
    const void * scl = nullptr;
    // optional f16 A-fragment image for the prompt matmul (launch_build_a16): 4x the
    // weight bytes, saves the nibble unpack in k_mm_q40_mfma; nullptr = unpack path
    const void * a16 = nullptr;
    // Q4_1 only: the prompt matmul's per-block side image (launch_build_mm41: weight
    // sums + d / m per lane); with a16 it enables the Q4_1 MFMA path (mm_mfma41.hip)
    const void * side = nullptr;
};

// Activation quantized to the weight format, stored split: d[N][nb] floats,
// m[N][nb] (Q4_1 only), qs[N][nb] uint4 (reference nibble convention).
struct ActQ {
    float * d = nullptr;
    float * m = nullptr;
    uint4 * qs = nullptr;
    int nb = 0;
};

// the runtime scalar block the decode graph reads (so one captured graph
// serves every position): written by a 16-byte H2D copy before each step, or advanced
// on the device by k_argmax_step in a chained greedy decode.
struct StepParams {
    int n_past;
    int n_tokens;
    int pad0;       // the token of a single-token eval (read by the embedding kernel)
    unsigned seq;   // decode step counter: the decode attention's granule epochs are
                    // (seq << 7) + layer + 1, so the granules need no zeroing per token
};

struct RopeTable {            // host-built with glibc powf/cosf/sinf (ggml.c:7209-7213)
    const float2 * cs;        // [n_ctx][hd/2] {cos, sin}
};

// prologue (how the matvec obtains its quantized input)
enum Pro : int { PRO_NORM = 0, PRO_ACTQ = 1, PRO_ACTF = 2 /* f32 input, quantize only */ };
// epilogue (what it does with row results)
enum Epi : int { EPI_STORE = 0, EPI_RESID = 1, EPI_QKV = 2, EPI_SWIGLU = 3, EPI_SWIGLU_F32 = 4, EPI_ROPE_KV = 5, EPI_SWIGLU_Q = 6 };

struct MvLaunch {
    QMatrix w;
    // input
    const float * x = nullptr;       // PRO_NORM: f32 [N][K]
    const float * g = nullptr;       // PRO_NORM: norm weight [K]
    ActQ xq;                         // PRO_ACTQ: quantized input
    const StepParams * sp = nullptr; // device step params (n_past, n_tokens)
    int n_tokens = 1;                // host-known token count of this launch
    int tok0 = 0;                    // first token row of x / xq to use
    // outputs
    float * y = nullptr;             // EPI_STORE: [N][M];  EPI_RESID: residual [N][M] (in place)
    // EPI_QKV
    uint16_t * q16 = nullptr;        // [N][E] f16 (post-rope queries)
    uint16_t * kc = nullptr;         // layer K cache [n_ctx][E]
    uint16_t * vc = nullptr;         // layer V cache [E][n_ctx]
    RopeTable rope{};
    int n_embd = 0, head_dim = 0, n_ctx = 0;
    int kv32 = 0;                    // f32 KV cache and f32 queries (f16_kv = false)
    // EPI_SWIGLU
    const uint16_t * silu_tab = nullptr;   // 64Ki fp16 table
    ActQ out_q;                            // quantized u = silu(w1 x) * (w3 x)
    float * u = nullptr;                   // EPI_SWIGLU_F32: u in f32 [N][M/2]
};

// dispatches on L.w.qtype: Q4_0 here (matvec_q4.hip), Q4_1, F16 and F32 forwarded.  Every matvec
// launcher returns hipErrorNotSupported for a (pro, epi) pair it has no instantiation for and
// hipErrorInvalidValue when the input that pro reads (x, g, or xq.qs / xq.d / xq.m) is null.
hipError_t launch_matvec(const MvLaunch & L, int pro, int epi, hipStream_t s);
// the same for Q4_1 weights (matvec_q41.hip)
hipError_t launch_matvec_q41(const MvLaunch & L, int pro, int epi, hipStream_t s);

// single-token decode matvec, one workgroup per CU (matvec_cu.hip for Q4_0,
// matvec_cu41.hip for Q4_1; F16 and F32 have one single-token kernel each, matvec_f16.hip and
// matvec_f32.hip, for every row length).  Row lengths compiled in: matvec_cu_supported(K, qtype).
// Returns hipErrorNotSupported for anything else (the caller then uses launch_matvec).
bool matvec_cu_supported(int K, int qtype = Q4_0);
hipError_t launch_matvec_cu(const MvLaunch & L, int pro, int epi, hipStream_t s);
// the rule of every caller that takes either: a single token of a compiled-in row length goes
// to the CU-balanced kernel, everything else (and what that has no instantiation for) to the
// generic one
inline hipError_t launch_matvec_auto(const MvLaunch & L, int pro, int epi, hipStream_t s) {
    if (L.n_tokens == 1 && matvec_cu_supported(L.w.K, L.w.qtype)) {
        const hipError_t e = launch_matvec_cu(L, pro, epi, s);
        if (e != hipErrorNotSupported) return e;
    }
    return launch_matvec(L, pro, epi, s);
}
// compute units of the current device (one decode workgroup per CU)
int cu_count();

// token embedding rows: x[t] = dequant(tok_emb[tokens[t]]) (ggml.c:6868-6895)
hipError_t launch_embed(const void * emb, int emb_type, int n_embd, const int * tokens, int n,
                        float * x, hipStream_t s);

// attention, one layer (llama.cpp:1010-1061)
struct AttnLaunch {
    const uint16_t * q16;     // [N][E]
    const uint16_t * kc;      // [n_ctx][E]
    const uint16_t * vc;      // [E][n_ctx]
    float * scores;           // scratch [N][H][n_ctx]
    ActQ out;                 // quantized attention output (Wo input), Q4_0 or Q4_1
    int out_qtype;
    const uint16_t * exp_tab; // 64Ki fp16 exp table
    const StepParams * sp;
    int n_tokens, n_embd, n_head, n_ctx;
    float * out_f32 = nullptr; // optional: also store the unquantized merged heads [N][E]
    uint16_t * p16_out = nullptr; // optional (debug): f16 probabilities [N][H][n_ctx]
    int exp_computed = 0;     // exp mode (lvk_device.h exp_f16): 0 table, 1 double, 2 f32 -- nonzero only after exp_check
    unsigned * err = nullptr; // host-mapped error word (DevError); kernels that spin report a timeout here
    int kv32 = 0;             // f32 K, V and queries (f16_kv = false): launch_attention only
    int seq_epochs = 0;       // decode attention: granule epoch = (sp->seq << 7) + epoch (no per-token zeroing)
};
hipError_t launch_attention(const AttnLaunch & A, hipStream_t s);
// prompt batches (N > 1, Q4_0 / Q4_1 output): scores+softmax per (head, pair of mirrored
// 16-token blocks) then P.V per (head, 32 tokens, 32 dims) with the Wo quantization fused
// (attention_prompt.hip).  p_scratch: H*N*n_ctx f16; wo_image (optional, all of the type's
// parts or none): also write the Wo input as the batched matmul's operand image.
struct ActImage;
bool attention_prompt_supported(int n_embd, int n_head, int n_ctx);
hipError_t launch_attention_prompt(const AttnLaunch & A, uint16_t * p_scratch, const ActImage & wo_image,
                                   hipStream_t s);
// count into bad_d[0] / bad_d[1] the softmax arguments h <= 0 whose exp computed in
// double / with the device expf differs from exp_tab[h]; 0 means that mode
// reproduces the host table exactly
hipError_t exp_check(const uint16_t * exp_tab, int * bad_d, hipStream_t s);
// single-token attention, 4 workgroups per head in one launch (attention_decode.hip):
// the head's scores are exchanged through `gran` (attention_decode_scratch_bytes, zeroed
// at allocation) tagged with `epoch` (layer + 1, never 0) + (sp->seq << 7) when
// A.seq_epochs is set (else the scratch must be zeroed before every token).  Needs
// A.n_tokens == 1.
bool attention_decode_supported(int n_embd, int n_head, int n_ctx);
// score-helper workgroups per head of such a launch on the current device (0 or 4)
int attention_decode_helpers(int n_embd, int n_head, int n_ctx);
size_t attention_decode_scratch_bytes(int n_head, int n_ctx);
hipError_t launch_attention_decode(const AttnLaunch & A, void * gran, unsigned epoch, hipStream_t s);

// Batched decode (lvk_decode_batch; attention_rows.hip): n rows, row i a single token of KV slot
// rows[i].slot at position rows[i].pos, computed as a single-token eval at n_past = pos on that
// slot's f16 cache.  slots[s]: the base of slot s's K [L][n_ctx][E] and V [L][E][n_ctx];
// layer_off: the layer's element offset in both (il * n_ctx * E).
struct SeqRow {
    int slot, pos;
};
struct SeqSlot {
    uint16_t * kc, * vc;
};
// RoPE + KV append of stored Q|K|V rows qkv [n][3E]: q16 [n][E] and, at pos of the row's slot,
// exactly the K / V stores of launch_rope_kv
hipError_t launch_rope_kv_rows(const float * qkv, int n, int E, int hd, const float2 * rope, const SeqRow * rows,
                               const SeqSlot * slots, size_t layer_off, int n_ctx, uint16_t * q16, hipStream_t s);
// one launch for the n rows (A.n_tokens) of a layer: row i attends over n_kv = pos_i + 1 of its
// slot, nothing masked; A.kc / A.vc / A.sp / A.scores are not read.  Writes A.out (and A.out_f32)
// like launch_attention.  Needs head_dim 128, n_ctx % 32 == 0, the f16 cache.
bool attention_rows_supported(int n_embd, int n_head, int n_ctx);
hipError_t launch_attention_rows(const AttnLaunch & A, const SeqRow * rows, const SeqSlot * slots, size_t layer_off,
                                 hipStream_t s);

// one-time weight repack: file-layout rows (ggml blocks) -> quad-sliced image
// interleave4: src_rows holds two (M/2)-row matrices A then B; the image
// interleaves them per 4 rows (A0-3, B0-3, A4-7, ...: the fused W1|W3)
hipError_t launch_repack(const void * src_rows, int qtype, int M, int K, uint4 * nib, void * scl,
                         hipStream_t s, int interleave4 = 0);
// bytes of the two image arrays for an M x K matrix
inline size_t qimage_nib_bytes(int M, int K) { return (size_t) M * ((K / 32 + 31) / 32) * 512; }
// Q4_1: d and m images, then the even-chain weight-sum image (q41_wsum)
inline size_t qimage_scl_bytes(int M, int K, int qtype = Q4_0) {
    return (size_t) M * ((K / 32 + 31) / 32) * 128 * (qtype == Q4_1 ? 3 : 1);
}
// Q4_1 weight sums, precomputed at repack: the AVX2 dot's `sums` term for the even
// chains (ggml.c:2236-2240, _mm256_sad_epu8 of the weight bytes 8k..8k+7 = the nibbles
// of qs[4k..4k+3], chain 2k) as one byte per block.  wsum[g][c][8r+j] (uint4): chain
// 2(j/2) of row 8g+r, blocks 32c + 16(j%2) .. +15 of the chunk, byte t = block +t.
inline const uint4 * q41_wsum(const QMatrix & w) {
    return (const uint4 *) ((const char *) w.scl + (size_t) w.M * ((w.K / 32 + 31) / 32) * 256);
}

// ---------------------------------------------------------------------------
// Batched (N > 1) matmul, bit-exact like launch_matvec.  One interface for the four
// weight types; launch_mm (mm_launch.hip) dispatches on w.qtype:
//   Q4_0 (mm_mfma.hip): the matrix cores produce the per-chain integer partials, the VALU
//     runs the reference fp32 chains.  Weights: the octet image, or QMatrix::a16 when built.
//   Q4_1 (mm_mfma41.hip): the matrix cores also produce the cross-term sums and the scale
//     products.  Weights: QMatrix::a16 + QMatrix::side, both from launch_build_mm41.
//   F16 (mm_f16.hip): the fp32 chains of matvec_f16.hip, tiled over tokens.
//   F32 (mm_f32.hip): the f32 matrix cores run the reference's fp32 chains themselves.
// The activations reach the kernels as an operand image of the weight type:
//   xm : Q4_0 / Q4_1 the masked MFMA B-fragment image (mm_common.h xm_slot);
//        F16 the paired-step f16 rows, N rounded up to MM_F16_TPAD rows;
//        F32 plain f32 rows [N][K] -- any such rows serve as the image, so a caller whose
//        input needs no RMSNorm points xm at it instead of calling launch_act
//   da : Q4_0 the block scales [N][K/32]
//   xs : Q4_1 the side image [N/16][K/32][64] x 16 B (mm_common.h act41_emit)
// xm must be ZEROED once at allocation: the writers only ever store the active fragment
// slots (Q4), and the padding rows' products are computed and dropped (F16).
struct ActImage {
    void * xm = nullptr;
    float * da = nullptr;
    void * xs = nullptr;
};
struct ActImageBytes {
    size_t xm, da, xs;     // 0: the type has no such part
};
constexpr int MM_TN = 16;          // tokens per MFMA tile
constexpr int MM_F16_TPAD = 32;    // the widest token tile of mm_f16.hip
inline ActImageBytes act_image_bytes(int qtype, int N, int K) {
    if (qtype == F16) return {(size_t) ((N + MM_F16_TPAD - 1) / MM_F16_TPAD * MM_F16_TPAD) * K * 2, 0, 0};
    if (qtype == F32) return {(size_t) N * K * 4, 0, 0};
    const size_t tiles = (size_t) (N + MM_TN - 1) / MM_TN, nb = (size_t) K / 32;
    return {tiles * nb * 4 * 64 * 8, qtype == Q4_0 ? (size_t) N * nb * 4 : 0, qtype == Q4_1 ? tiles * nb * 64 * 16 : 0};
}
// f32 rows x[N][K] (rms_norm * g when g != nullptr) -> the operand image: quantize_row_q4_0 /
// quantize_row_q4_1 (AVX2 branches), f32 -> f16 RNE, or (F32) the f32 rows themselves
hipError_t launch_act(int qtype, const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s);
// pre-quantized blocks (ActQ of the same type) -> the operand image; F16 / F32: hipErrorNotSupported
hipError_t launch_actq_to_image(int qtype, const ActQ & q, int N, int K, const ActImage & out, hipStream_t s);

// EPI_ROPE_KV: RoPE + KV append in the QKV matmul's epilogue (f16 KV cache): the f32 Q|K|V
// rows never reach memory; q16 / kc / vc get exactly what launch_rope_kv writes
struct RopeKV {
    const float2 * rope;       // [n_ctx][hd/2] cos, sin
    const StepParams * sp;     // n_past
    int n_ctx, E, hd;
    uint16_t * q16, * kc, * vc;
};
struct MmLaunch {
    QMatrix w;
    ActImage x;                            // the N input rows
    int N = 0;
    float * y = nullptr;                   // EPI_STORE: [N][ldy];  EPI_RESID: y += W x;  EPI_SWIGLU_F32: u [N][ldy]
    int ldy = 0;
    const uint16_t * silu_tab = nullptr;   // EPI_SWIGLU_F32 / EPI_SWIGLU_Q (fused W1|W3 image)
    const RopeKV * rk = nullptr;           // EPI_ROPE_KV (set for that epilogue only)
    // EPI_SWIGLU_Q: u = silu(w1 x) * (w3 x) quantized straight into the W2 input's image (of
    // N x M/2), as launch_act(u, nullptr, ...) would write it
    ActImage out;
};
// which epilogues a type's kernels implement; launch_mm returns hipErrorNotSupported for the others
constexpr bool mm_epi_supported(int qtype, int epi) {
    switch (epi) {
        case EPI_STORE: case EPI_RESID: case EPI_SWIGLU_F32: return qtype == F32 || qtype == F16 || qtype == Q4_0 || qtype == Q4_1;
        case EPI_ROPE_KV: return qtype == Q4_0 || qtype == Q4_1;
        case EPI_SWIGLU_Q: return qtype == Q4_0;
    }
    return false;
}
// the matrix's shape and images fit its type's kernels
bool mm_supported(const QMatrix & w);
hipError_t launch_mm(const MmLaunch & L, int epi, hipStream_t s);
// the per-type halves of launch_act / launch_actq_to_image / launch_mm (reached through them,
// which check the arguments: these only fill their parameter block and launch)
hipError_t act_q40(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s);
hipError_t act_q41(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s);
hipError_t act_f16(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s);
hipError_t act_f32(const float * x, const float * g, int N, int K, const ActImage & out, hipStream_t s);
hipError_t actq_image_q40(const ActQ & q, int N, int K, const ActImage & out, hipStream_t s);
hipError_t actq_image_q41(const ActQ & q, int N, int K, const ActImage & out, hipStream_t s);
hipError_t mm_q40(const MmLaunch & L, int epi, hipStream_t s);
hipError_t mm_q41(const MmLaunch & L, int epi, hipStream_t s);
hipError_t mm_f16(const MmLaunch & L, int epi, hipStream_t s);
hipError_t mm_f32(const MmLaunch & L, int epi, hipStream_t s);

// the f16 A-fragment image of a Q4_0 matrix (QMatrix::a16): bytes, and its build from the
// matrix's octet image (M % 32 == 0)
size_t mm_a16_bytes(int M, int K);
hipError_t launch_build_a16(const QMatrix & w, void * a16, hipStream_t s);
// LVK_PROMPT_A16=0 keeps the prompt matmul on the nibble image (no f16 A image)
inline bool prompt_a16_env() {
    const char * e = getenv("LVK_PROMPT_A16");
    return !e || atoi(e) != 0;
}
// LVK_PROMPT_A16=1: build the Q4_0 images whenever they fit; unset: by capacity (lvk_model.cpp)
inline bool prompt_a16_forced() {
    const char * e = getenv("LVK_PROMPT_A16");
    return e && atoi(e) == 1;
}
// the Q4_1 weight images: QMatrix::a16 (mm_a16_bytes, f16 q values) + QMatrix::side
size_t mm41_side_bytes(int M, int K);
hipError_t launch_build_mm41(const QMatrix & w, void * a16, void * side, hipStream_t s);
// RoPE + KV append of stored Q|K|V rows qkv [N][3E]
hipError_t launch_rope_kv(const float * qkv, int N, int E, int hd, const float2 * rope, const StepParams * sp,
                          int n_ctx, uint16_t * q16, uint16_t * kc, uint16_t * vc, hipStream_t s, int kv32 = 0);

// f16 weights (type 1).  Image: 2 B per weight, rows padded to a multiple of 8.
inline size_t f16_image_bytes(int M, int K) { return (size_t) ((M + 7) / 8 * 8) * K * 2; }
hipError_t launch_repack_f16(const void * src_rows, int M, int K, uint4 * img, hipStream_t s, int interleave4 = 0);
// single-token decode matvec (matvec_f16.hip): PRO_NORM (rms_norm * g -> f16) or PRO_ACTF
// (f32 -> f16) of the f32 row L.x; EPI_STORE, EPI_RESID, EPI_QKV, EPI_SWIGLU_F32.
// launch_matvec and launch_matvec_cu forward here
hipError_t launch_matvec_f16(const MvLaunch & L, int pro, int epi, hipStream_t s);

// f32 weights (type 0).  Image: 4 B per weight, rows padded to a multiple of 8.
inline size_t f32_image_bytes(int M, int K) { return (size_t) ((M + 7) / 8 * 8) * K * 4; }
hipError_t launch_repack_f32(const void * src_rows, int M, int K, uint4 * img, hipStream_t s, int interleave4 = 0);
// single-token decode matvec (matvec_f32.hip): PRO_NORM (rms_norm * g) or PRO_ACTF of the f32
// row L.x, used as it is; EPI_STORE, EPI_RESID, EPI_QKV, EPI_SWIGLU_F32.
// launch_matvec and launch_matvec_cu forward here
hipError_t launch_matvec_f32(const MvLaunch & L, int pro, int epi, hipStream_t s);

// operator-level helpers used by the C ABI tests
hipError_t launch_quantize_act(const float * x, int N, int K, int qtype, ActQ out, hipStream_t s);
// the reference's scalar quantize_row_q4_0/1_reference (roundf, id = 1/d)
hipError_t launch_quantize_ref(const float * x, int N, int K, int qtype, ActQ out, hipStream_t s);

}  // namespace lvk

namespace lvk {
// device half of llama_sample_top_p_top_k (sample.hip): repeat penalty + temperature on the
// logits in HBM, radix select of the k-th largest value, every value >= it written to out
// (host-mapped).  SampleParams lives in device memory (one H2D copy per step).
constexpr int SAMPLE_MAX_VOCAB = 32768;   // values per thread kept in registers
constexpr int SAMPLE_CAP = 1024;          // candidates the host can receive (k <= this)
constexpr int SAMPLE_MAX_LAST = 1024;     // last-n window entries
enum SampleFlags : int { SAMPLE_FLAG_NAN = 1, SAMPLE_FLAG_OVERFLOW = 2 };
struct SampleParams {
    int k;                    // top_k (1..SAMPLE_CAP)
    int n_last;               // entries of last[]
    float scale;              // 1.0f / temp
    float rp;                 // repeat_penalty
    int last[SAMPLE_MAX_LAST];
};
struct SampleOut {
    int count;                // candidates (values >= the k-th largest)
    int flags;                // SampleFlags
    int pad[2];
    float val[SAMPLE_CAP];
    int id[SAMPLE_CAP];
};
hipError_t launch_sample_cand(const float * logits, int n, const SampleParams * P, SampleOut * out, hipStream_t s);
// the same for n_sel rows of logits[.][n] in one launch, one workgroup per record: rec[j] names
// its logits row and holds its parameters (the SampleParams limits per row), its last-n ids are
// pool[last_off .. last_off + n_last), its candidates go to out[j] (host-mapped)
struct SampleRow {
    int row;                  // index into logits[.][n]
    int k;                    // top_k (1..SAMPLE_CAP)
    int n_last;               // entries of its window (0..SAMPLE_MAX_LAST)
    int last_off;             // the window's offset in the pool
    float scale;              // 1.0f / temp
    float rp;                 // repeat_penalty
};
hipError_t launch_sample_cand_rows(const float * logits, int n, const SampleRow * rec, const int * pool, int n_sel,
                                   SampleOut * out, hipStream_t s);

// y[t] = g * rms_norm(x[t]) as f32 (the embeddings output, llama.cpp:1117-1124)
hipError_t launch_rmsnorm_rows(const float * x, const float * g, int K, int n, float * y, hipStream_t s);
// greedy argmax over x[0..n) with the reference's first-maximum rule (llama.cpp:1382-1394); *out on the device
// (out2, optional: a second copy of the token, e.g. host-mapped memory)
hipError_t launch_argmax(const float * x, int n, int * out, hipStream_t s, int * out2 = nullptr);
// the same per row of x[rows][n]: out[r] on the device, one launch
hipError_t launch_argmax_rows(const float * x, int n, int rows, int * out, hipStream_t s);
// one chained decode step's tail (lvk_decode_chain): the same argmax into chain[CHAIN_HDR + i]
// (chain[0] = i counts the steps), the logits digest into digest[i] when chain[2] != 0, the next
// token (forced[i + 1] while i + 1 < chain[1], else the argmax) into the step block (n_past + 1,
// token, seq + 1) and its embedding row (launch_embed's) into x[0..n_embd)
constexpr int CHAIN_HDR = 4;
hipError_t launch_argmax_step(const float * logits, int n, StepParams * sp, int * chain, const int * forced,
                              unsigned long long * digest, const void * emb, int emb_type, int n_embd, float * x,
                              hipStream_t s);
// one chained batched decode step's tail (lvk_decode_batch_chain): launch_argmax_step per row of
// logits [n][n_vocab], one workgroup each.  Row r's step index is i = rows[r].pos - pos0[r]; its
// argmax goes to out_tok[i * n + r], the logits digest to digest[i * n + r] when ctl[1] != 0, the
// next token (forced[(i + 1) * n + r] while i + 1 < ctl[0], else the argmax) to next_tok[r]
// (optional) and, with emb, its embedding row to x[r][0..n_embd); rows[r].pos advances by one.
// No workgroup reads a word another one writes.
hipError_t launch_rows_step(const float * logits, int n_vocab, int n, SeqRow * rows, const int * pos0, const int * ctl,
                            const int * forced, int * out_tok, unsigned long long * digest, int * next_tok,
                            const void * emb, int emb_type, int n_embd, float * x, hipStream_t s);
// the scoring tail (score.hip; lvk_eval_score, lvk_decode_batch_score): probs[i] = the reference's
// softmax(logits[i])[targets[i]] (perplexity.cpp:6-20) for the n rows of logits [n][n_vocab], one
// workgroup each; a row with targets[i] < 0 gets -1.0f.  Every other target must be < n_vocab (the
// host checks it).  The row stays in registers: 1 <= n_vocab <= SCORE_MAX_VOCAB.
constexpr int SCORE_MAX_VOCAB = 32768;
hipError_t launch_score_rows(const float * logits, int n_vocab, int n, const int * targets, float * probs, hipStream_t s);

// ---------------------------------------------------------------------------
// ggml graph operators (graph_ops.hip; include/ggml.h via runtime/ggml_graph.cpp): one
// node per launch on a strided 4-D view of a device buffer
enum GType : int { GT_Q4_0 = 0, GT_Q4_1 = 1, GT_I32 = 4, GT_F16 = 5, GT_F32 = 6 };   // = enum ggml_type
enum GOp : int { GOP_ADD = 0, GOP_SUB, GOP_MUL, GOP_DIV, GOP_REPEAT, GOP_SCALE, GOP_SILU, GOP_DIAG_MASK };
struct GView {
    char * p = nullptr;
    int64_t ne[4] = {1, 1, 1, 1};
    int64_t nb[4] = {0, 0, 0, 0};
    int type = GT_F32;
};
hipError_t launch_g_cpy(const GView & s, const GView & d, hipStream_t st);
hipError_t launch_g_binary(const GView & a, const GView & b, const GView & d, int op, hipStream_t st);
hipError_t launch_g_unary(const GView & s, const GView & d, int op, float v, int n_past, const uint16_t * tab,
                          hipStream_t st);
hipError_t launch_g_rms_norm(const GView & s, const GView & d, hipStream_t st);
hipError_t launch_g_soft_max(const GView & d, const uint16_t * exp_tab, int exp_mode, hipStream_t st);
hipError_t launch_g_rope(const GView & s, const GView & d, const float2 * cs, int n_dims, int i2_0, hipStream_t st);
hipError_t launch_g_get_rows(const GView & s, const int32_t * idx, int64_t n_rows, const GView & d, hipStream_t st);
// y: contiguous rows (f16 when s0 is f16, else f32) [ne13][ne12][ne11][ne00]
hipError_t launch_g_mm_dot(const GView & s0, const void * y, int64_t ne11, const GView & d, hipStream_t st);

}  // namespace lvk
