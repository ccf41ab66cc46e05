// lvk_context.h -- one inference context: device KV cache, scratch, the
// launch sequence of llama_eval on a HIP stream and the captured decode graph.
#pragma once
#include "lvk_buffers.h"

#include <array>
#include <chrono>
#include <functional>
#include <memory>

struct llama_context_params;
struct lvk_row_sample;      // include/lvk_ops.h

namespace lvk {

struct Split;       // lvk_split.h
struct StageLink;
struct SplitDel { void operator()(Split * p) const; };
struct StageLinkDel { void operator()(StageLink * p) const; };

// kernel classes timed by the profiler (events around every launch of a class)
enum KClass : int { K_EMBED = 0, K_QKV, K_ATTN, K_WO, K_W13, K_W2, K_LMHEAD, K_NCLASS };

struct Profile {
    std::array<double, K_NCLASS> ms{};       // accumulated device time
    std::array<long, K_NCLASS> launches{};   // launches accumulated
    std::array<double, K_NCLASS> bytes{};    // algorithmic HBM bytes accumulated
};

// one slice of an eval call: a whole llama_eval, or one micro-batch of a prompt that a
// layer split pipelines through its stages (lvk_split.cpp)
struct EvalPart {
    int tok_off = 0;      // first token of this slice within the call
    int n_total = -1;     // tokens of the whole call (-1: this slice is the call)
    bool head = true;     // run norm + lm_head (last stage: the call's last slice, or logits_all)
    bool copy_out = true; // copy logits / embedding / the greedy token to the host after this slice
    bool greedy = false;  // end in the device argmax (lvk_eval_greedy) instead of the logits D2H
    bool sample = false;  // end in the device top-k candidates (lvk_eval_sample) instead of the logits D2H
    bool score = false;   // lm_head over every row whatever logits_all says, ending in the score kernel over the
                          //   targets staged in sc_tgt_h (lvk_eval_score) instead of the logits D2H
    bool score_argmax = false;   // score: the rows' device argmax as well
};

struct Context {
    Model model;
    int n_ctx = 512;             // allocated positions (the caller's n_ctx rounded up to 32, >= 128)
    int n_ctx_user = 512;        // llama_context_params.n_ctx: the positions an eval may use
    bool logits_all = false;
    bool want_embedding = false;
    // destruction runs upwards: the graphs, events and buffers below go first, then the stream,
    // then the stage link, and the model (whose arena holds the raw pointers below) last
    std::unique_ptr<StageLink, StageLinkDel> link;   // one-stage-per-process link (lvk_stage_connect[_shm])
    Stream stream;

    // device state
    uint16_t * kc = nullptr;     // [L][n_ctx][E] f16, or f32 when kv32
    uint16_t * vc = nullptr;     // [L][E][n_ctx] f16, or f32 when kv32
    bool kv32 = false;           // f32 KV cache and queries (llama_context_params.f16_kv = false)
    size_t kv_elem_bytes() const { return kv32 ? 4 : 2; }
    uint16_t * kc_layer(size_t il) const { return kc + il * (size_t) n_ctx * model.hp.n_embd * (kv_elem_bytes() / 2); }
    uint16_t * vc_layer(size_t il) const { return vc + il * (size_t) n_ctx * model.hp.n_embd * (kv_elem_bytes() / 2); }
    float * x = nullptr;         // residual stream [n_ctx][E]
    uint16_t * q16 = nullptr;    // [n_ctx][E]
    float * scores = nullptr;    // [n_ctx][H][n_ctx]
    ActQ aq_attn;                // [n_ctx][E/32]
    ActQ aq_ffn;                 // [n_ctx][F/32]
    float * u_ffn = nullptr;     // [F] decode: silu(w1 x) * (w3 x) in f32
    float * logits_d = nullptr;  // [n_ctx][V]
    float * emb_d = nullptr;     // [E]
    uint16_t * exp_tab = nullptr;
    int exp_computed = 0;     // softmax exp mode (exp_f16: 0 table, 1 double, 2 f32; verified equal to exp_tab)
    uint16_t * silu_tab = nullptr;
    float2 * rope = nullptr;     // [n_ctx][hd/2]
    StepParams * sp_d = nullptr;
    int * tok_d = nullptr;       // [n_ctx]
    HostPtr<StepParams> sp_h;    // pinned, [1 + n_ctx] step blocks: [0] for the graphs, the
    int sp_next = 1;             //   rest one per eager slice enqueued before the next sync
    HostPtr<int> tok_h;          // pinned [n_ctx]
    HostPtr<unsigned> err_h;     // host-mapped: the kernels' error word (lvk_kernels.h DevError)
    unsigned * err_d = nullptr;  // its device address
    int device = 0;              // the HIP device of this context

    // prompt (N > 1) path: MFMA matmuls with exact block dots (default) or the
    // bit-faithful VALU kernels (prompt_exact; env LVK_PROMPT_EXACT=1)
    bool prompt_exact = false;
    bool old_attention = false;  // env LVK_ATTN_V1=1: single-token evals on the one-kernel attention.hip
    void * attn_gran = nullptr;  // [H][n_ctx] {tag, score} granules of the decode attention
    // batched (N > 1) matmuls: the operand image of the matrix about to run (lvk_kernels.h
    // ActImage, sized for n_ctx rows of max(E, F)), rewritten before every matmul
    ActImage img;
    // Q4_0: the W2 input image written by the W1|W3 epilogue (EPI_SWIGLU_Q; the W1|W3 launch
    // still reads img); LVK_MM_SWIGLU_Q=0: f32 uf + launch_act instead
    ActImage img_w2;
    float * qkv32 = nullptr;     // [C][3E] Q|K|V rows before RoPE (f32-KV prompts, LVK_MM_ROPE=0, f16 models)
    // prompt: RoPE + KV append fused into the QKV matmul (LVK_MM_ROPE=0: separate kernel)
    bool mm_rope_fused = [] { const char * e = getenv("LVK_MM_ROPE"); return !e || atoi(e) != 0; }();
    float * uf = nullptr;        // [C][F] silu(w1 x) * (w3 x)
    // f16 and f32 models only: the attention's f32 output, the Wo input (F16: converted to f16
    // by launch_act / the matvec's prologue; F32: read as it is); nullptr = Wo takes the
    // quantized aq_attn
    float * attn_f32 = nullptr;  // [C][E]

    // the single-token decode graphs, captured on first use (build_graph):
    //   LOGITS  last-token logits (llama_eval)
    //   GREEDY  lvk_eval_greedy: argmax on the device, 4-byte D2H instead of the logits row
    //   SAMPLE  lvk_eval_sample: the sampler block H2D, the forward pass and the device top-k
    //           candidates (sample.hip) into host-mapped memory instead of the logits row
    //   CHAIN   one step of lvk_decode_greedy (below)
    enum class DecodeGraph { LOGITS, GREEDY, SAMPLE, CHAIN };
    std::array<Graph, 4> graphs;
    Graph & graph_of(DecodeGraph k) { return graphs[(size_t) k]; }
    bool use_graph = true;
    HostPtr<SampleParams> samp_h;      // pinned host block, filled per call
    SampleParams * samp_d = nullptr;
    HostPtr<SampleOut> sout_h;         // host-mapped candidates
    SampleOut * sout_d = nullptr;      // its device address
    // one single-token eval + the device half of the sampler (samp_h filled by the caller);
    // the candidates are in *sout_h afterwards
    void eval_sample(int token, int n_past);
    // the last eval's last-token logits row -> host logits (llama_get_logits valid again)
    void fetch_logits();
    int n_sample_fallback = 0;         // lvk_eval_sample calls / lvk_decode_batch_sample rows that took the all-logits host path
    int * greedy_d = nullptr;
    HostPtr<int> greedy_h;       // host-mapped (coherent): the device argmax writes it
    int * greedy_hd = nullptr;   // its device address
    void enqueue_argmax();
    // chained greedy decode (lvk_decode_greedy): one graph per step that reads nothing from
    // the host -- its last kernel (k_argmax_step) picks the token, advances the step block
    // on the device and writes the next step's embedding row -- replayed n times per call
    int * chain_d = nullptr;     // [CHAIN_HDR + n_ctx]: step counter, forced count, digest flag, pad; the argmax tokens
    HostPtr<int> chain_h;        // pinned copy of the tokens
    HostPtr<int> chain_ctl_h;    // pinned header block (CHAIN_HDR ints)
    int * forced_d = nullptr;    // [n_ctx] teacher-forced tokens of a chained decode
    HostPtr<int> forced_h;       // pinned staging of them
    unsigned long long * digest_d = nullptr;   // [n_ctx] per-step logits digests
    HostPtr<unsigned long long> digest_h;      // pinned copy
    int decode_chain(const int * tokens, int n_tokens, int n_past, int n_steps, int * out, unsigned long long * digests);
    // decode attention granule epochs from the step counter (StepParams::seq): no zeroing per
    // token (off for models with more than 126 layers)
    bool seq_epochs = false;
    unsigned seq = 0;            // the last step counter handed to the device
    unsigned next_seq(unsigned k = 1);

    // batched decode (lvk_decode_batch): KV slots beside kc / vc, which are slot 0 with the count
    // kv_n.  seq_kv[s - 1] is slot s >= 1 in the same layout (f16, zeroed at allocation).
    struct SeqKV {
        DevPtr<uint16_t> kc, vc;
        int n = 0;               // positions held
    };
    std::vector<SeqKV> seq_kv;
    DevPtr<SeqSlot> slots_d;     // [seq_count()] base pointers of every slot (empty before seq_init)
    DevPtr<SeqRow> rows_d;       // [n_ctx] {slot, pos} of a call's rows
    HostPtr<SeqRow> rows_h;      // pinned staging of them
    DevPtr<int> amax_d;          // [n_ctx] per-row argmax
    int seq_count() const { return 1 + (int) seq_kv.size(); }
    int & seq_n(int s) { return s == 0 ? kv_n : seq_kv[(size_t) s - 1].n; }
    SeqSlot slot_kv(int s) const {      // the K and V of slot s >= 0
        return s == 0 ? SeqSlot{kc, vc} : SeqSlot{seq_kv[(size_t) s - 1].kc.get(), seq_kv[(size_t) s - 1].vc.get()};
    }
    // allocate slots up to n_seq (fewer than now: nothing); on failure nothing has changed
    void seq_init(int n_seq);
    void seq_copy(int dst, int src, int n_tokens);
    // n rows (token, slot, position), each computed as a single-token eval at its position on
    // its slot; logits [n][V] and argmax [n] are optional host destinations
    void decode_rows(const int * tokens, const int * seqs, const int * pos, int n, float * logits_out, int * argmax_out);
    // n_steps such steps of n rows, one per slot, in one call (state: the end of this struct)
    void decode_rows_chain(const int * forced, int n_forced, const int * seqs, const int * pos, int n, int n_steps,
                           int * out_tokens, unsigned long long * out_digests, float * logits_out);
    void rows_chain_reserve(size_t entries);
    // what the three decode_rows* share: rows_begin takes a step slice, fills its block (pad0 as
    // given) and stages and copies the block, the tokens (nullptr: none) and the rows; rows_finish
    // ends the step with the host logits of llama_get_logits left as they were (an earlier eval's)
    void rows_begin(const int * tokens, const int * seqs, const int * pos, int n, int pad0, unsigned n_seq = 1);
    void rows_finish(const std::vector<int> & next);      // next: rows_check's, the slots' new counts
    // decode_rows' step, then per row with rows[i].sample != 0 the sampler on row i's logits,
    // drawing from the row's slot's generator (lvk_decode_batch_sample; lvk_rows.cpp has the paths)
    void decode_rows_sample(const int * tokens, const int * seqs, const int * pos, int n, const lvk_row_sample * rows,
                            int * out_tokens);
    // the checks of a batched decode step's rows; next[s]: the count slot s has after the step (-1: no row)
    std::vector<int> rows_check(const char * fn, const int * tokens, const int * seqs, const int * pos, int n);
    // scoring (lvk_eval_score, lvk_decode_batch_score): the forward pass with the lm_head over every
    // row, then launch_score_rows over logits_d; only probs (and the rows' argmax) cross PCIe.  The
    // buffers hold n_ctx rows, device and page-locked, allocated by the first call (score_reserve).
    DevPtr<int> sc_tgt_d, sc_amax_d;
    DevPtr<float> sc_prob_d;
    HostPtr<int> sc_tgt_h, sc_amax_h;
    HostPtr<float> sc_prob_h;
    bool score_on_host = false;      // n_vocab > SCORE_MAX_VOCAB (or env LVK_SCORE_HOST=1): score_host over the rows
    void score_reserve();
    // the targets' checks (messages under the caller's name), then the targets into sc_tgt_h
    void score_stage(const char * fn, int n, const int * targets, const float * probs);
    // after the forward pass: targets H2D, the score kernel, probs (and argmax) D2H into the pinned buffers
    void enqueue_score(int n, bool want_argmax);
    // after the stream sync: the pinned results to the caller (score_on_host: the scored rows one
    // by one through score_host)
    void score_collect(int n, float * probs, int * argmax);
    void eval_score(const int * tokens, int n, int n_past, const int * targets, float * probs, int * argmax);
    void decode_rows_score(const int * tokens, const int * seqs, const int * pos, int n, const int * targets, float * probs,
                           int * argmax);
    // per sampled row of a step (sr_cap of them, grown on demand): the candidates (host-mapped)
    // and the kernel's record; sr_pool_cap ints of last-n windows back to back
    size_t sr_cap = 0, sr_pool_cap = 0;
    HostPtr<SampleOut> sr_out_h;        // host-mapped
    SampleOut * sr_out_d = nullptr;     // its device address
    HostPtr<SampleRow> sr_rec_h;        // pinned staging
    DevPtr<SampleRow> sr_rec_d;
    HostPtr<int> sr_pool_h;
    DevPtr<int> sr_pool_d;
    void rows_sample_reserve(size_t rows, size_t pool);
    // the generators of slots >= 1 (slot 0 draws from rng), seeded with `seed` at seq_init
    std::vector<std::mt19937> seq_rng;
    std::mt19937 & seq_gen(int s) { return s == 0 ? rng : seq_rng[(size_t) s - 1]; }

    // host-visible results
    std::vector<float, PinnedAlloc<float>> logits;
    bool logits_valid = false;   // false after lvk_eval_greedy (host logits not refreshed) or a failed eval
    std::vector<float> embedding;
    std::vector<uint8_t> kv_host;
    int kv_n = 0;
    std::mt19937 rng;
    int seed = 0;                // llama_context_params.seed as resolved at init (<= 0: time())

    // timings (llama.cpp:1186-1195)
    int64_t t_start_us = 0, t_load_us = 0, t_sample_us = 0, t_eval_us = 0, t_p_eval_us = 0;
    int n_sample = 0, n_eval = 0, n_p_eval = 0;
    bool has_evaluated_once = false;

    // profiling
    bool profiling = false;
    Profile prof;
    std::vector<std::pair<Event, Event>> ev_pool;
    std::vector<int> ev_class;
    size_t ev_used = 0;

    void init(const llama_context_params & p);
    void eval(const int * tokens, int n, int n_past);
    // eval = begin_eval (everything enqueued on `stream`, no host wait) + end_eval (sync,
    // profile, device error word); a layer split interleaves the stages' begin_evals
    // with the residual-stream hand-offs and ends them together
    void begin_eval(const int * tokens, int n, int n_past, const EvalPart & part);
    void begin_eval_safe(const int * tokens, int n, int n_past, const EvalPart & part);
    // run fn; if it throws, the work already queued drains before the error propagates, with the
    // step slices released (reset_slices) and the host logits marked stale (stale_logits) as asked
    template <class F> void drain_on_error(bool reset_slices, bool stale_logits, F && fn) {
        try {
            fn();
        } catch (...) {
            (void) hipStreamSynchronize(stream);
            if (reset_slices) sp_next = 1;
            if (stale_logits) logits_valid = false;
            throw;
        }
    }
    void end_eval(bool no_host_logits);
    // stage boundary: copy the residual stream x [n][E] to (to_ctx) or from the context
    void x_copy(void * buf, int n, bool to_ctx, bool on_device);
    struct Forward {
        int n = 1;                      // tokens
        bool last_only = true;          // lm_head over the last token only
        const int * tok_src = nullptr;  // device tokens of the embedding (nullptr: tok_d)
        int logit_row = 0;              // first row of logits_d written
        bool head = true;               // run norm + lm_head
        bool embed = true;              // run the embedding (false: x holds the rows already)
        bool rows = false;              // the tokens are a batched decode step's rows (rows_d / slots_d), not
                                        //   n consecutive positions of slot 0
    };
    static Forward rows_forward(int n) {      // a batched decode step over n rows, every row's logits
        Forward f;
        f.n = n;
        f.last_only = false;
        f.rows = true;
        return f;
    }
    void enqueue_forward(const Forward & f);
    bool use_batched(int n) const;
    void build_graph(DecodeGraph kind);
    int eval_greedy(int token, int n_past);
    void kv_get();
    void kv_set(const uint8_t * src, size_t n);
    void kv_copy_from(const Context & src, int n_tokens);
    // positions [0, n_tokens) of every layer's K and V, device to device, then a stream sync
    void copy_kv_prefix(uint16_t * dk, uint16_t * dv, const uint16_t * sk, const uint16_t * sv, int n_tokens);
    size_t kv_bytes() const;
    void timed_launch(int cls, double bytes, const std::function<hipError_t()> & fn);
    void collect_profile();
    // after a stream sync: throw if a kernel raised the error word (and clear it)
    void check_device_error();

    // chained batched decode (lvk_decode_batch_chain): one graph per step of n rows that reads
    // nothing from the host -- the rows' forward pass, then k_rows_step, which picks every row's
    // next token, writes its embedding row and advances rows_d -- replayed n_steps times per call
    Graph graph_rows;
    int graph_rows_n = 0;            // its key: the row count baked into the graph's launches
    bool graph_rows_exact = false;   //   and prompt_exact at capture (it selects the matmul path)
    // per call: [n_steps][n] argmax tokens and digests, [n_forced][n] forced tokens (rc_cap
    // entries each, grown on demand), the rows' start positions and {n_forced, digest flag}
    size_t rc_cap = 0;
    DevPtr<int> rc_tok_d, rc_forced_d, rc_ctl_d;          // rc_ctl: [2 + n_ctx], the two control words, then the
    HostPtr<int> rc_tok_h, rc_forced_h, rc_ctl_h;         //   start positions; allocated once
    DevPtr<unsigned long long> rc_dig_d;
    HostPtr<unsigned long long> rc_dig_h;
};

int64_t now_us();
// the host sampler (llama_api.cpp): llama_sample_top_p_top_k over n_logits values; its part after
// the top-k selection; the same over one row's device candidates (-1: take the all-logits path)
int sample_logits(const float * pl, int n_logits, const int * last, int n_last, int top_k, float top_p, float temp,
                  float repeat_penalty, std::mt19937 & rng);
int sample_from_top_k(std::mt19937 & rng, std::vector<std::pair<float, int>> & cand, float top_p);
int sample_from_candidates(const SampleOut & so, int k, float top_p, std::mt19937 & rng);
// the reference's softmax(row)[target] per row of logits [n][V] on the host (llama_api.cpp; lvk_score_host)
void score_host(const float * logits, int n, int V, const int * targets, float * probs);
// exp mode of the softmax kernels (lvk_device.h exp_f16): 2, 1 or 0 after a device self-check
int pick_exp_mode(const uint16_t * exp_tab_d);
// fp16 exp / silu tables (ggml.c:2915-2927) built with this host's glibc expf
void host_fp16_tables(std::vector<uint16_t> & exp_tab, std::vector<uint16_t> & silu_tab);
// RoPE {cos, sin} table [n_ctx][hd/2] (ggml.c:7209-7213) built with this host's glibc powf / cosf / sinf
void host_rope_table(std::vector<float2> & rt, size_t n_ctx, size_t hd);

}  // namespace lvk

// the opaque handle of the C API (include/llama.h)
struct llama_context {
    lvk::Context c;                                  // the whole model, or the last stage of a split
    std::unique_ptr<lvk::Split, lvk::SplitDel> split;   // layer split over devices (lvk_split.h)
    std::shared_ptr<void> tensor_map;                // llama_internal_get_tensor_map's state (on first use)
    // every stage context in layer order (just &c without a split)
    std::vector<lvk::Context *> stages();
};
