// lvk_rows.cpp -- the batched-decode half of Context: KV slots beside slot 0 (seq_init, seq_copy)
// and the three steps over rows of (token, slot, position); their forward pass is enqueue_forward's
// rows path (lvk_context.cpp).  The buffers grow on demand: seq_init and the two reserves allocate
// into local owners, wait for the stream, and only then move the locals into the members (which
// frees the old buffers), so a throw before that point leaves the context as it was.
#include "lvk_context.h"

#include <cstring>

#include "../../../include/lvk_ops.h"

namespace lvk {

// KV slots 1..n_seq-1 and, on the first call, the row and slot tables of decode_rows.
void Context::seq_init(int n_seq) {
    const HParams & hp = model.hp;
    if (n_seq < 1) throw Error("lvk_seq_init: n_seq must be at least 1");
    if (kv32) throw Error("lvk_seq_init: batched decode needs the f16 KV cache (f16_kv = true)");
    if (!model.has_embed || !model.has_head || link) throw Error("lvk_seq_init: not available on a stage context");
    if (!attention_rows_supported((int) hp.n_embd, (int) hp.n_head, n_ctx))
        throw Error("lvk_seq_init: batched decode needs head_dim 128");
    const int have = seq_count();
    if (n_seq <= have && slots_d) return;
    const int want = std::max(n_seq, have);
    const size_t bytes = kv_bytes() / 2, C = (size_t) n_ctx;
    const char * oom = "lvk_seq_init: out of device memory";
    std::vector<SeqKV> add((size_t) (want - have));
    for (SeqKV & s : add) {
        s.kc = dev_alloc<uint16_t>(bytes / 2, oom);
        s.vc = dev_alloc<uint16_t>(bytes / 2, oom);
        LVK_HIP(hipMemset(s.kc.get(), 0, bytes));
        LVK_HIP(hipMemset(s.vc.get(), 0, bytes));
    }
    // the new slots' generators start from the context's seed; the existing ones stay as they are
    std::vector<std::mt19937> gens;
    gens.reserve((size_t) want - 1);
    gens.assign(seq_rng.begin(), seq_rng.end());
    gens.resize((size_t) want - 1, std::mt19937((unsigned) seed));
    std::vector<SeqSlot> table;
    for (int s = 0; s < have; ++s) table.push_back(slot_kv(s));
    for (const SeqKV & s : add) table.push_back({s.kc.get(), s.vc.get()});
    DevPtr<SeqSlot> table_d = dev_alloc<SeqSlot>(table.size(), oom);
    DevPtr<SeqRow> rd;
    DevPtr<int> ad;
    HostPtr<SeqRow> rh;
    if (!rows_d) {
        rd = dev_alloc<SeqRow>(C, oom);
        ad = dev_alloc<int>(C, oom);
        rh = pinned_alloc<SeqRow>(C);
    }
    seq_kv.reserve((size_t) want - 1);          // the commit below cannot throw
    LVK_HIP(hipStreamSynchronize(stream));      // nothing in flight reads the old table
    LVK_HIP(hipMemcpy(table_d.get(), table.data(), table.size() * sizeof(SeqSlot), hipMemcpyHostToDevice));
    // commit
    graph_rows.reset();     // its launches hold the old slot table
    slots_d = std::move(table_d);
    if (!rows_d) {
        rows_d = std::move(rd);
        amax_d = std::move(ad);
        rows_h = std::move(rh);
    }
    for (SeqKV & s : add) seq_kv.push_back(std::move(s));
    seq_rng.swap(gens);
}

// positions [0, n_tokens) of every layer's K and V from slot src to slot dst
void Context::seq_copy(int dst, int src, int n_tokens) {
    if (dst < 0 || dst >= seq_count() || src < 0 || src >= seq_count()) throw Error("lvk_seq_copy: sequence id out of range");
    if (n_tokens < 0 || n_tokens > seq_n(src)) throw Error("lvk_seq_copy: n_tokens exceeds the source sequence");
    if (dst != src && n_tokens > 0) {
        const SeqSlot d = slot_kv(dst), s = slot_kv(src);
        copy_kv_prefix(d.kc, d.vc, s.kc, s.vc, n_tokens);
    }
    seq_n(dst) = n_tokens;
}

// the argument checks of a batched decode step (decode_rows, decode_rows_sample), messages under
// the caller's name; next[s]: the count slot s has after the step (-1: no row)
std::vector<int> Context::rows_check(const char * fn, const int * tokens, const int * seqs, const int * pos, int n) {
    const int V = (int) model.hp.n_vocab;
    const std::string f = std::string(fn) + ": ";
    if (!tokens || !seqs || !pos) throw Error(f + "null argument");
    if (n < 1 || n > n_ctx_user) throw Error(f + "the row count must be in 1..n_ctx");
    std::vector<int> next((size_t) seq_count(), -1);
    for (int i = 0; i < n; ++i) {
        if (tokens[i] < 0 || tokens[i] >= V) throw Error(f + "token id out of range");
        if (seqs[i] < 0 || seqs[i] >= seq_count()) throw Error(f + "sequence id out of range");
        if (pos[i] < 0 || pos[i] >= n_ctx_user) throw Error(f + "position outside n_ctx");
        int & nx = next[(size_t) seqs[i]];
        if (nx < 0 && pos[i] > seq_n(seqs[i])) throw Error(f + "position past the end of its sequence (a hole)");
        if (nx >= 0 && pos[i] != nx) throw Error(f + "rows of one sequence must have consecutive ascending positions");
        nx = pos[i] + 1;
    }
    return next;
}

void Context::rows_begin(const int * tokens, const int * seqs, const int * pos, int n, int pad0, unsigned n_seq) {
    if (sp_next > n_ctx) throw Error("llama.vk_amd: too many slices before a sync");
    StepParams * sh = &sp_h[sp_next++];
    sh->n_past = 0;             // no kernel of this path takes a position from the step block
    sh->n_tokens = n;
    sh->pad0 = pad0;
    sh->seq = next_seq(n_seq);
    if (tokens) std::memcpy(tok_h.get(), tokens, sizeof(int) * (size_t) n);
    for (int i = 0; i < n; ++i) rows_h[i] = {seqs[i], pos[i]};
    LVK_HIP(hipMemcpyAsync(sp_d, sh, sizeof(StepParams), hipMemcpyHostToDevice, stream));
    if (tokens) LVK_HIP(hipMemcpyAsync(tok_d, tok_h.get(), sizeof(int) * (size_t) n, hipMemcpyHostToDevice, stream));
    LVK_HIP(hipMemcpyAsync(rows_d.get(), rows_h.get(), sizeof(SeqRow) * (size_t) n, hipMemcpyHostToDevice, stream));
}

// the slots' counts move only after the step has completed
void Context::rows_finish(const std::vector<int> & next) {
    const bool valid = logits_valid;
    end_eval(true);
    logits_valid = valid;
    for (int s = 0; s < seq_count(); ++s)
        if (next[(size_t) s] >= 0) seq_n(s) = next[(size_t) s];
}

// One batched decode step (lvk_decode_batch).  Every argument is checked before anything is enqueued.
void Context::decode_rows(const int * tokens, const int * seqs, const int * pos, int n, float * logits_out, int * argmax_out) {
    const int V = (int) model.hp.n_vocab;
    if (!slots_d) seq_init(1);
    const std::vector<int> next = rows_check("lvk_decode_batch", tokens, seqs, pos, n);
    drain_on_error(true, false, [&] {
        rows_begin(tokens, seqs, pos, n, n == 1 ? tokens[0] : 0);
        enqueue_forward(rows_forward(n));
        if (argmax_out) {
            LVK_HIP(launch_argmax_rows(logits_d, V, n, amax_d.get(), stream));
            LVK_HIP(hipMemcpyAsync(argmax_out, amax_d.get(), sizeof(int) * (size_t) n, hipMemcpyDeviceToHost, stream));
        }
        if (logits_out)
            LVK_HIP(hipMemcpyAsync(logits_out, logits_d, sizeof(float) * (size_t) n * V, hipMemcpyDeviceToHost, stream));
    });
    rows_finish(next);
}

// decode_rows' step ending in the score kernel (lvk_decode_batch_score): probs[i] =
// softmax(row i)[targets[i]], -1.0f where targets[i] < 0; only probs (and the rows' argmax) cross
// PCIe.  Every argument is checked before anything is enqueued.
void Context::decode_rows_score(const int * tokens, const int * seqs, const int * pos, int n, const int * targets,
                                float * probs, int * argmax_out) {
    if (!slots_d) seq_init(1);
    const std::vector<int> next = rows_check("lvk_decode_batch_score", tokens, seqs, pos, n);
    score_stage("lvk_decode_batch_score", n, targets, probs);
    drain_on_error(true, false, [&] {
        rows_begin(tokens, seqs, pos, n, n == 1 ? tokens[0] : 0);
        enqueue_forward(rows_forward(n));
        enqueue_score(n, argmax_out != nullptr);
    });
    rows_finish(next);
    score_collect(n, probs, argmax_out);
}

// room for `rows` sampled rows of a step and `pool` last-n ids: the host-mapped candidates, the
// records and the pool, on the device and page-locked on the host; a buffer that is large enough stays
void Context::rows_sample_reserve(size_t rows, size_t pool) {
    const bool grow_rows = rows > sr_cap, grow_pool = pool > sr_pool_cap || !sr_pool_d;
    if (!grow_rows && !grow_pool) return;
    const char * oom = "lvk_decode_batch_sample: out of memory for the sampler's rows";
    const size_t rcap = grow_rows ? std::max(rows, (size_t) 16) : sr_cap;
    const size_t pcap = grow_pool ? std::max(std::max(pool, sr_pool_cap), (size_t) 1024) : sr_pool_cap;
    HostPtr<SampleOut> out_h;
    SampleOut * out_d = nullptr;
    HostPtr<SampleRow> rec_h;
    DevPtr<SampleRow> rec_d;
    HostPtr<int> pool_h;
    DevPtr<int> pool_d;
    if (grow_rows) {
        out_h = mapped_alloc<SampleOut>(rcap, oom);
        out_d = device_address(out_h);
        rec_h = pinned_alloc<SampleRow>(rcap, oom);
        rec_d = dev_alloc<SampleRow>(rcap, oom);
    }
    if (grow_pool) {
        pool_h = pinned_alloc<int>(pcap, oom);
        pool_d = dev_alloc<int>(pcap, oom);
    }
    LVK_HIP(hipStreamSynchronize(stream));      // nothing in flight uses the old buffers
    // commit
    if (grow_rows) {
        sr_out_h = std::move(out_h);
        sr_out_d = out_d;
        sr_rec_h = std::move(rec_h);
        sr_rec_d = std::move(rec_d);
        sr_cap = rcap;
    }
    if (grow_pool) {
        sr_pool_h = std::move(pool_h);
        sr_pool_d = std::move(pool_d);
        sr_pool_cap = pcap;
    }
}

// One batched decode step that ends in the sampler (lvk_decode_batch_sample): decode_rows' forward
// pass, enqueued eagerly; launch_argmax_rows over the span of rows that ask for a greedy token
// (temp <= 0); one launch_sample_cand_rows for the rows that sample within the device limits; one
// stream sync; then, in row order, the host tail of lvk_eval_sample over each row's candidates
// with the generator of the row's slot.  A row with ties, NaN, overflow, top_k <= 0 or >
// SAMPLE_CAP, or a window > SAMPLE_MAX_LAST has its own logits row copied to the host and takes
// sample_logits there with the same generator (n_sample_fallback counts it); no other row notices.
// Every argument is checked before anything is enqueued.  The rows count into the eval timings,
// the sampled rows into the sample timings.
void Context::decode_rows_sample(const int * tokens, const int * seqs, const int * pos, int n, const lvk_row_sample * rows,
                                 int * out_tokens) {
    const int64_t t0 = now_us();
    const int V = (int) model.hp.n_vocab;
    if (!slots_d) seq_init(1);
    const std::vector<int> next = rows_check("lvk_decode_batch_sample", tokens, seqs, pos, n);
    if (!rows || !out_tokens) throw Error("lvk_decode_batch_sample: null argument");
    enum : char { NONE, GREEDY, DEVICE, HOST };
    std::vector<char> kind((size_t) n, NONE);
    std::vector<int> top((size_t) n, 0);      // the reference's k: top_k, or all of them
    size_t n_dev = 0, n_pool = 0;
    int n_samp = 0, g_lo = n, g_hi = -1;
    for (int i = 0; i < n; ++i) {
        const lvk_row_sample & r = rows[i];
        if (!r.sample) continue;
        if (r.n_last < 0 || (r.n_last > 0 && !r.last_n)) throw Error("lvk_decode_batch_sample: bad last-n window");
        ++n_samp;
        const int k = top[(size_t) i] = r.top_k > 0 ? std::min(r.top_k, V) : V;
        if (r.temp <= 0) {                              // llama.cpp:1382-1394
            kind[(size_t) i] = GREEDY;
            g_lo = std::min(g_lo, i);
            g_hi = i;
        } else if (k > SAMPLE_CAP || r.n_last > SAMPLE_MAX_LAST || V > SAMPLE_MAX_VOCAB) {
            kind[(size_t) i] = HOST;
        } else {
            kind[(size_t) i] = DEVICE;
            ++n_dev;
            n_pool += (size_t) r.n_last;
        }
    }
    if (n_dev) rows_sample_reserve(n_dev, n_pool);
    std::vector<int> amax((size_t) n, -1), slot_of((size_t) n, -1);
    drain_on_error(true, false, [&] {
        rows_begin(tokens, seqs, pos, n, n == 1 ? tokens[0] : 0);
        size_t j = 0, off = 0;
        for (int i = 0; i < n; ++i) {
            if (kind[(size_t) i] != DEVICE) continue;
            const lvk_row_sample & r = rows[i];
            sr_rec_h[j] = {i, top[(size_t) i], r.n_last, (int) off, 1.0f / r.temp /* llama.cpp:1398 */, r.repeat_penalty};
            if (r.n_last > 0) std::memcpy(sr_pool_h.get() + off, r.last_n, sizeof(int) * (size_t) r.n_last);
            off += (size_t) r.n_last;
            slot_of[(size_t) i] = (int) j++;
        }
        if (n_dev) {
            LVK_HIP(hipMemcpyAsync(sr_rec_d.get(), sr_rec_h.get(), sizeof(SampleRow) * n_dev, hipMemcpyHostToDevice, stream));
            if (n_pool)
                LVK_HIP(hipMemcpyAsync(sr_pool_d.get(), sr_pool_h.get(), sizeof(int) * n_pool, hipMemcpyHostToDevice, stream));
        }
        enqueue_forward(rows_forward(n));
        if (g_hi >= 0) {
            const size_t m = (size_t) (g_hi - g_lo + 1);
            LVK_HIP(launch_argmax_rows(logits_d + (size_t) g_lo * V, V, (int) m, amax_d.get() + g_lo, stream));
            LVK_HIP(hipMemcpyAsync(amax.data() + g_lo, amax_d.get() + g_lo, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
        }
        if (n_dev)
            LVK_HIP(launch_sample_cand_rows(logits_d, V, sr_rec_d.get(), sr_pool_d.get(), (int) n_dev, sr_out_d, stream));
    });
    rows_finish(next);
    const int64_t t1 = now_us();
    t_eval_us += t1 - t0;       // n decode evals (llama.cpp:1186-1195)
    n_eval += n;
    std::vector<float> row;
    for (int i = 0; i < n; ++i) {
        const lvk_row_sample & r = rows[i];
        int tok = -1;
        if (kind[(size_t) i] == GREEDY) tok = amax[(size_t) i];
        else if (kind[(size_t) i] == DEVICE)
            tok = sample_from_candidates(sr_out_h[(size_t) slot_of[(size_t) i]], top[(size_t) i], r.top_p, seq_gen(seqs[i]));
        if (tok < 0 && (kind[(size_t) i] == DEVICE || kind[(size_t) i] == HOST)) {
            row.resize((size_t) V);
            LVK_HIP(hipMemcpy(row.data(), logits_d + (size_t) i * V, sizeof(float) * (size_t) V, hipMemcpyDeviceToHost));
            tok = sample_logits(row.data(), V, r.last_n, r.n_last, r.top_k, r.top_p, r.temp, r.repeat_penalty, seq_gen(seqs[i]));
            n_sample_fallback++;
        }
        out_tokens[i] = tok;
    }
    t_sample_us += now_us() - t1;
    n_sample += n_samp;
}

// room for `entries` = n_steps * n tokens, digests and forced tokens of a chained batched decode,
// on the device and page-locked on the host, and on the first call the control block.  The step
// graph holds the old addresses, so it goes with them.
void Context::rows_chain_reserve(size_t entries) {
    if (entries <= rc_cap && rc_ctl_d) return;
    const size_t cap = std::max(std::max(entries, rc_cap), (size_t) n_ctx), ctl = 2 + (size_t) n_ctx;
    const char * oom = "lvk_decode_batch_chain: out of memory for the step outputs";
    DevPtr<int> tok_d = dev_alloc<int>(cap, oom);
    HostPtr<int> tok_h = pinned_alloc<int>(cap, oom);
    DevPtr<unsigned long long> dig_d = dev_alloc<unsigned long long>(cap, oom);
    HostPtr<unsigned long long> dig_h = pinned_alloc<unsigned long long>(cap, oom);
    DevPtr<int> for_d = dev_alloc<int>(cap, oom);
    HostPtr<int> for_h = pinned_alloc<int>(cap, oom);
    DevPtr<int> ctl_d = rc_ctl_d ? nullptr : dev_alloc<int>(ctl, oom);
    HostPtr<int> ctl_h = rc_ctl_d ? nullptr : pinned_alloc<int>(ctl, oom);
    LVK_HIP(hipStreamSynchronize(stream));      // nothing in flight uses the old buffers
    // commit
    graph_rows.reset();
    rc_tok_d = std::move(tok_d);
    rc_tok_h = std::move(tok_h);
    rc_dig_d = std::move(dig_d);
    rc_dig_h = std::move(dig_h);
    rc_forced_d = std::move(for_d);
    rc_forced_h = std::move(for_h);
    if (!rc_ctl_d) {
        rc_ctl_d = std::move(ctl_d);
        rc_ctl_h = std::move(ctl_h);
    }
    rc_cap = cap;
}

// n_steps batched decode steps in one call (lvk_decode_batch_chain): step i evaluates, for every
// row r, token t_i[r] at pos[r] + i on slot seqs[r], as decode_rows would with those n rows;
// t_0[r] = forced[r], t_{i+1}[r] = forced[(i + 1) * n + r] while i + 1 < n_forced, else the argmax
// of row r's logits of step i.  The host sets the rows, the forced table and the first embedding
// rows up once; each step is the rows' forward pass followed by k_rows_step, which leaves x and
// rows_d as the next step reads them.  The rows path of enqueue_forward takes positions and slots
// from rows_d / slots_d alone (sp_d is read only by the fused QKV epilogues, which a rows step
// does not run), so the step block needs no advancing on the device.  The steps are replays of
// one captured graph, or the same launches enqueued eagerly when the graph is off or the
// profiler is on.  Every argument is checked before anything is enqueued.
void Context::decode_rows_chain(const int * forced, int n_forced, const int * seqs, const int * pos, int n, int n_steps,
                                int * out_tokens, unsigned long long * out_digests, float * logits_out) {
    const HParams & hp = model.hp;
    const int V = (int) hp.n_vocab, E = (int) hp.n_embd;
    if (!slots_d) seq_init(1);
    if (!forced || !seqs || !pos || !out_tokens) throw Error("lvk_decode_batch_chain: null argument");
    if (n < 1 || n > n_ctx_user) throw Error("lvk_decode_batch_chain: the row count must be in 1..n_ctx");
    if (n_steps < 1 || n_steps > n_ctx_user) throw Error("lvk_decode_batch_chain: n_steps must be in 1..n_ctx");
    if (n_forced < 1 || n_forced > n_steps) throw Error("lvk_decode_batch_chain: n_forced must be in 1..n_steps");
    std::vector<int> next((size_t) seq_count(), -1);      // the count a named slot has after the call
    for (int r = 0; r < n; ++r) {
        if (seqs[r] < 0 || seqs[r] >= seq_count()) throw Error("lvk_decode_batch_chain: sequence id out of range");
        if (next[(size_t) seqs[r]] >= 0) throw Error("lvk_decode_batch_chain: a sequence may have one row only");
        if (pos[r] < 0 || pos[r] > seq_n(seqs[r]))
            throw Error("lvk_decode_batch_chain: position past the end of its sequence (a hole)");
        if (pos[r] > n_ctx_user - n_steps) throw Error("lvk_decode_batch_chain: pos + n_steps exceeds n_ctx");
        next[(size_t) seqs[r]] = pos[r] + n_steps;
    }
    const size_t nf = (size_t) n_forced * n, total = (size_t) n_steps * n;
    for (size_t k = 0; k < nf; ++k)
        if (forced[k] < 0 || forced[k] >= V) throw Error("lvk_decode_batch_chain: token id out of range");
    rows_chain_reserve(total);
    auto step = [&] {
        Forward f = rows_forward(n);
        f.embed = false;
        enqueue_forward(f);
        LVK_HIP(launch_rows_step(logits_d, V, n, rows_d.get(), rc_ctl_d.get() + 2, rc_ctl_d.get(), rc_forced_d.get(),
                                 rc_tok_d.get(), rc_dig_d.get(), nullptr, model.tok_emb, model.emb_type, E, x, stream));
    };
    drain_on_error(true, false, [&] {
        rows_begin(nullptr, seqs, pos, n, 0, (unsigned) n_steps);
        rc_ctl_h[0] = n_forced;
        rc_ctl_h[1] = out_digests ? 1 : 0;
        for (int r = 0; r < n; ++r) rc_ctl_h[2 + r] = pos[r];
        std::memcpy(rc_forced_h.get(), forced, sizeof(int) * nf);
        LVK_HIP(hipMemcpyAsync(rc_ctl_d.get(), rc_ctl_h.get(), sizeof(int) * (2 + (size_t) n), hipMemcpyHostToDevice, stream));
        LVK_HIP(hipMemcpyAsync(rc_forced_d.get(), rc_forced_h.get(), sizeof(int) * nf, hipMemcpyHostToDevice, stream));
        LVK_HIP(launch_embed(model.tok_emb, model.emb_type, E, rc_forced_d.get(), n, x, stream));
        if (use_graph && !profiling) {
            // the row count (and the matmul path it selects) is baked into the graph's launches
            if (graph_rows && (graph_rows_n != n || graph_rows_exact != prompt_exact)) graph_rows.reset();
            if (!graph_rows) {
                capture(stream, graph_rows, step);
                graph_rows_n = n;
                graph_rows_exact = prompt_exact;
            }
            for (int i = 0; i < n_steps; ++i) LVK_HIP(graph_rows.launch(stream));
        } else {
            for (int i = 0; i < n_steps; ++i) step();
        }
        LVK_HIP(hipMemcpyAsync(rc_tok_h.get(), rc_tok_d.get(), sizeof(int) * total, hipMemcpyDeviceToHost, stream));
        if (out_digests) LVK_HIP(hipMemcpyAsync(rc_dig_h.get(), rc_dig_d.get(), 8 * total, hipMemcpyDeviceToHost, stream));
        if (logits_out)
            LVK_HIP(hipMemcpyAsync(logits_out, logits_d, sizeof(float) * (size_t) n * V, hipMemcpyDeviceToHost, stream));
    });
    rows_finish(next);
    std::memcpy(out_tokens, rc_tok_h.get(), sizeof(int) * total);
    if (out_digests) std::memcpy(out_digests, rc_dig_h.get(), 8 * total);
}

}  // namespace lvk
