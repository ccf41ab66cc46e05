// ggml_graph.cpp -- ggml_graph_compute of include/ggml.h on the GPU (the builder: ggml_api.cpp).
//
// ggml_graph_compute mirrors every host buffer the graph touches into HBM, runs each node on
// the GPU in graph order (graph_ops.hip, the Q4 matvec kernels), and copies the bytes the nodes
// wrote back.  The mirrors, the repacked Q4 images and the temporaries' arena persist across
// calls: only host pages that may have been written since the previous call travel again
// (ggml_track.h decides which), so a caller's weights upload once.  An operator without a GPU
// implementation aborts -- there is no CPU fallback.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../../include/lvk_ops.h"
#include "ggml_internal.h"
#include "lvk_context.h"

using namespace ggml_impl;
using namespace lvk::track;

namespace {

uint64_t ns_since(std::chrono::steady_clock::time_point t0) {
    return (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}

// what the tracking asks of HIP: is this (mapped) host address registered or pinned memory
bool is_hip_host(const void * q) {
    hipPointerAttribute_t a{};
    const bool host = hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeHost;
    (void) hipGetLastError();
    return host;
}

// a host range [lo, hi) mirrored in HBM
struct Mirror : PageState {
    lvk::DevPtr<char> dev;
    uint64_t last_call = 0;
};

// a Q4 weight repacked into the decode kernels' octet image, keyed by its host address
struct Repacked {
    const char * lo;
    const char * hi;
    int qt, M, K;
    lvk::DevPtr<char> nib, scl;
    lvk::QMatrix matrix() const {
        lvk::QMatrix q;
        q.qtype = qt; q.M = M; q.K = K; q.nib = (const uint4 *) nib.get(); q.scl = scl.get();
        return q;
    }
};

// grow-only device (or pinned host) arena, reset per call: no allocation per op
template <class Ptr, Ptr (*alloc)(size_t, const char *)>
struct Arena {
    std::vector<std::pair<Ptr, size_t>> chunks;
    size_t cur = 0, off = 0;
    void * get(size_t n) {
        n = (n + 255) & ~(size_t) 255;
        if (n == 0) n = 256;
        while (cur < chunks.size()) {
            if (off + n <= chunks[cur].second) {
                void * p = chunks[cur].first.get() + off;
                off += n;
                return p;
            }
            ++cur;
            off = 0;
        }
        const size_t sz = std::max(n, chunks.empty() ? (size_t) 1 << 20 : chunks.back().second * 2);
        chunks.emplace_back(alloc(sz, nullptr), sz);
        cur = chunks.size() - 1;
        off = n;
        return chunks.back().first.get();
    }
    void reset() { cur = 0; off = 0; }
};

// a contiguous view of ne elements of `es` bytes at p
lvk::GView contiguous_view(void * p, const int64_t * ne, int n_dims, int64_t es, int type) {
    lvk::GView v;
    v.p = (char *) p;
    for (int i = 0; i < n_dims; ++i) v.ne[i] = ne[i];
    v.nb[0] = es;
    for (int i = 1; i < 4; ++i) v.nb[i] = v.nb[i - 1] * v.ne[i - 1];
    v.type = type;
    return v;
}

// f(t) for every tensor node n reads
template <class F> void for_sources(const ggml_tensor * n, F && f) {
    if (n->src0) f(n->src0);
    if (n->src1) f(n->src1);
    for (int k = 0; k < GGML_MAX_OPT; ++k)
        if (n->opt[k]) f(n->opt[k]);
}

struct GraphStats {
    uint64_t h2d = 0, d2h = 0, repack = 0, mirrored = 0;
    uint64_t track_ns = 0, clear_ns = 0;   // host time of the validity bookkeeping / of clear_refs
};

// the persistent device state of ggml_graph_compute on one device
struct GraphEngine {
    lvk::Stream stream;
    std::vector<std::unique_ptr<Mirror>> mirrors;      // sorted by lo, disjoint
    std::vector<Repacked> repacked;
    Arena<lvk::DevPtr<char>, lvk::dev_alloc<char>> dev_arena;
    Arena<lvk::HostPtr<char>, lvk::pinned_alloc<char>> host_arena;
    Tracking track;
    uint64_t calls = 0;
    GraphStats last;
    // this call
    std::vector<Mirror *> used;
    std::vector<Span> written;              // node outputs of this call, in order

    GraphEngine() { LVK_HIP(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)); }

    Mirror & mirror_of(const void * p) {
        const char * c = (const char *) p;
        auto it = std::upper_bound(mirrors.begin(), mirrors.end(), c,
                                   [](const char * v, const std::unique_ptr<Mirror> & m) { return v < m->lo; });
        if (it == mirrors.begin() || c >= (*(it - 1))->hi) gabort("ggml_graph_compute: tensor outside the mapped buffers");
        return **(it - 1);
    }
    char * dev(const void * p) {
        Mirror & m = mirror_of(p);
        return m.dev.get() + ((const char *) p - m.lo);
    }
    void * temp(size_t n) { return dev_arena.get(n); }
    // host bytes that must reach the device in stream order: copied into pinned staging first,
    // so the caller's memory may go away before the copy runs
    void * upload_small(const void * src, size_t n) {
        void * h = host_arena.get(n);
        std::memcpy(h, src, n);
        void * d = temp(n);
        LVK_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream));
        return d;
    }
    void drop_repacked(const char * lo, const char * hi) {
        for (size_t i = 0; i < repacked.size();) {
            if (!overlaps(lo, hi, repacked[i].lo, repacked[i].hi)) { ++i; continue; }
            repacked[i] = std::move(repacked.back());
            repacked.pop_back();
        }
    }

    // one mirror covering [lo, hi): existing overlapping mirrors are merged into it (their
    // device bytes copied over, their fully covered valid pages kept)
    void ensure(char * lo, char * hi) {
        // sorted and disjoint: the mirrors that overlap [lo, hi) are [first, last)
        auto first = std::find_if(mirrors.begin(), mirrors.end(), [&](const auto & m) { return lo < m->hi; });
        auto last = first;
        while (last != mirrors.end() && (*last)->lo < hi) ++last;
        if (last - first == 1 && (*first)->lo <= lo && hi <= (*first)->hi) return;
        for (auto it = first; it != last; ++it) {
            lo = std::min(lo, (*it)->lo);
            hi = std::max(hi, (*it)->hi);
        }
        auto n = std::make_unique<Mirror>();
        n->set_range(lo, hi);
        n->dev = lvk::dev_alloc<char>((size_t) (hi - lo) + 16);
        for (auto it = first; it != last; ++it) {
            const Mirror & m = **it;
            LVK_HIP(hipMemcpyAsync(n->dev.get() + (m.lo - lo), m.dev.get(), (size_t) (m.hi - m.lo), hipMemcpyDeviceToDevice, stream));
            Tracking::adopt(*n, m);
        }
        LVK_HIP(hipStreamSynchronize(stream));
        mirrors.insert(mirrors.erase(first, last), std::move(n));
    }

    // the invalid pages of m that overlap [a, b) travel host -> device
    void upload(Mirror & m, const char * a, const char * b) {
        for (const Span & r : track.invalid_runs(m, a, b)) {
            LVK_HIP(hipMemcpyAsync(m.dev.get() + (r.lo - m.lo), r.lo, (size_t) (r.hi - r.lo), hipMemcpyHostToDevice, stream));
            last.h2d += (uint64_t) (r.hi - r.lo);
            drop_repacked(r.lo, r.hi);
        }
    }

    // true when no node of this call has written [p, p + n) so far: the host bytes are current
    bool host_current(const void * p, size_t n) const {
        const char * a = (const char *) p;
        for (const Span & w : written)
            if (overlaps(a, a + n, w.lo, w.hi)) return false;
        return true;
    }
    template <class T> T read_scalar(const ggml_tensor * t, int i) {
        const char * p = (const char *) t->data + (size_t) i * sizeof(T);
        T v;
        if (host_current(p, sizeof(T))) { std::memcpy(&v, p, sizeof(T)); return v; }
        LVK_HIP(hipMemcpyAsync(&v, dev(p), sizeof(T), hipMemcpyDeviceToHost, stream));
        LVK_HIP(hipStreamSynchronize(stream));
        return v;
    }
    lvk::GView view(const ggml_tensor * t) {
        lvk::GView v;
        v.p = dev(t->data);
        for (int i = 0; i < 4; ++i) { v.ne[i] = t->ne[i]; v.nb[i] = (int64_t) t->nb[i]; }
        v.type = (int) t->type;
        return v;
    }
    // contiguous device copy of a f32 tensor's rows, optionally converted to f16 (RNE)
    void * gather(const ggml_tensor * t, lvk::GType to) {
        const size_t es = to == lvk::GT_F16 ? 2 : 4;
        void * p = temp((size_t) ggml_nelements(t) * es);
        LVK_HIP(lvk::launch_g_cpy(view(t), contiguous_view(p, t->ne, 4, (int64_t) es, to), stream));
        return p;
    }
    // the octet image of the Q4 matrix at host address w (M x K), repacked once and kept
    // until the host bytes change
    lvk::QMatrix qmatrix(const char * w, int qt, int M, int K) {
        for (const Repacked & r : repacked)
            if (r.lo == w && r.qt == qt && r.M == M && r.K == K) return r.matrix();
        const char * hi = w + (size_t) M * (K / 32) * (qt == lvk::Q4_1 ? 24 : 20);
        Repacked r{w, hi, qt, M, K, lvk::dev_alloc<char>(lvk::qimage_nib_bytes(M, K)),
                   lvk::dev_alloc<char>(lvk::qimage_scl_bytes(M, K, qt))};
        LVK_HIP(lvk::launch_repack(dev(w), qt, M, K, (uint4 *) r.nib.get(), r.scl.get(), stream));
        last.repack += (uint64_t) (hi - w);
        repacked.push_back(std::move(r));
        return repacked.back().matrix();
    }

    // ---- the steps of one call, in order (upload_inputs and run_nodes follow run_node below) ----
    void begin_call() {
        last = GraphStats{};
        used.clear(); written.clear();
        dev_arena.reset(); host_arena.reset();
        ++calls;
    }
    // mirrors for the regions: created or merged.  A later region's ensure() may merge (and
    // release) the mirror an earlier region got, so the mirrors this call uses are looked up
    // after all merges
    void map_regions(const std::vector<Span> & regions) {
        for (const Span & r : regions) ensure((char *) r.lo, (char *) r.hi);
        for (const Span & r : regions) {
            Mirror & m = mirror_of(r.lo);
            if (m.last_call != calls) {
                m.last_call = calls;
                used.push_back(&m);
            }
        }
    }
    void refresh_used() {
        const auto t0 = std::chrono::steady_clock::now();
        track.snapshot();
        for (Mirror * m : used) track.refresh(*m, is_hip_host);
        last.track_ns += ns_since(t0);
    }
    // node results back to the host: the written byte ranges only (merged)
    void write_back() {
        for (const Span & w : merge_spans(written)) {
            LVK_HIP(hipMemcpyAsync((void *) w.lo, dev(w.lo), (size_t) (w.hi - w.lo), hipMemcpyDeviceToHost, stream));
            last.d2h += (uint64_t) (w.hi - w.lo);
        }
        LVK_HIP(hipStreamSynchronize(stream));
    }
    // mirrors unused for 8 calls are freed (a caller's per-call scratch contexts)
    void retire() {
        for (size_t i = 0; i < mirrors.size();) {
            if (mirrors[i]->last_call + 8 >= calls) { ++i; continue; }
            drop_repacked(mirrors[i]->lo, mirrors[i]->hi);
            mirrors.erase(mirrors.begin() + (long) i);
        }
    }
    uint64_t resident() const {
        uint64_t n = 0;
        for (const auto & m : mirrors) n += (uint64_t) (m->hi - m->lo);
        return n;
    }
};

// one engine per device, behind one lock (ggml contexts may be used from several threads);
// engines live as long as the process (no HIP object is destroyed from a static destructor)
std::mutex & engine_mutex() {
    static std::mutex m;
    return m;
}
std::map<int, GraphEngine *> & all_engines() {
    static std::map<int, GraphEngine *> per_dev;
    return per_dev;
}
GraphEngine & engine() {
    std::map<int, GraphEngine *> & per_dev = all_engines();
    int d = 0;
    LVK_HIP(hipGetDevice(&d));
    auto it = per_dev.find(d);
    if (it != per_dev.end()) return *it->second;
    return *per_dev.emplace(d, new GraphEngine).first->second;
}
GraphStats g_last_stats;
bool g_have_engine = false;

// the soft-dirty bits are process-wide: every engine's mirrors this call did not use (all those
// of the other devices' engines) note their host writes before the clear
void fold_and_clear(GraphEngine & R) {
    DirtyTracker & T = tracker();
    if (!T.ok) return;
    const auto t_fold0 = std::chrono::steady_clock::now();
    for (auto & kv : all_engines()) {
        GraphEngine & E = *kv.second;
        if (&E != &R) E.track.maps_now = R.track.maps_now;
        for (auto & m : E.mirrors)
            if (&E != &R || m->last_call != R.calls) E.track.refresh(*m, is_hip_host);
    }
    const auto t_clear0 = std::chrono::steady_clock::now();
    if (!T.clear()) {
        T.ok = false;
        for (auto & kv : all_engines())
            for (auto & m : kv.second->mirrors) m->drop_all();
    }
    R.last.clear_ns = ns_since(t_clear0);
    R.last.track_ns += ns_since(t_fold0);
}

// fp16 exp / silu tables of this host's glibc (ggml.c:2915-2927) and the softmax exp mode,
// once per device, for the life of the process
struct Tables {
    uint16_t * exp_tab = nullptr;
    uint16_t * silu_tab = nullptr;
    int exp_mode = 0;
};
const Tables & tables() {
    static std::map<int, Tables> per_dev;
    int dev = 0;
    LVK_HIP(hipGetDevice(&dev));
    auto it = per_dev.find(dev);
    if (it != per_dev.end()) return it->second;
    Tables t;
    std::vector<uint16_t> te, ts;
    lvk::host_fp16_tables(te, ts);
    LVK_HIP(hipMalloc(&t.exp_tab, 65536 * 2));
    LVK_HIP(hipMalloc(&t.silu_tab, 65536 * 2));
    LVK_HIP(hipMemcpy(t.exp_tab, te.data(), 65536 * 2, hipMemcpyHostToDevice));
    LVK_HIP(hipMemcpy(t.silu_tab, ts.data(), 65536 * 2, hipMemcpyHostToDevice));
    t.exp_mode = lvk::pick_exp_mode(t.exp_tab);
    return per_dev.emplace(dev, t).first->second;
}

void run_mul_mat_q(GraphEngine & R, const ggml_tensor * a, const ggml_tensor * b, ggml_tensor * node) {
    // ggml_compute_forward_mul_mat_q_f32 (ggml.c:6510-6696): every src1 row quantized with
    // the AVX2 quantizer, one vec_dot_q per (row, column) -- the matvec kernels' arithmetic
    const int M = (int) a->ne[1], K = (int) a->ne[0], N = (int) b->ne[1];
    const int qt = a->type == GGML_TYPE_Q4_0 ? lvk::Q4_0 : lvk::Q4_1;
    if (M % 8 || K % 256) gabort("ggml_graph_compute: Q4 mul_mat needs ne01 % 8 == 0 and ne00 % 256 == 0");
    G_ASSERT(a->nb[1] == (size_t) (K / 32) * TYPE_SIZE[a->type]);
    for (int64_t i3 = 0; i3 < a->ne[3]; ++i3)
        for (int64_t i2 = 0; i2 < a->ne[2]; ++i2) {
            const lvk::QMatrix q = R.qmatrix((const char *) a->data + i2 * a->nb[2] + i3 * a->nb[3], qt, M, K);
            // this batch's src1 rows, contiguous
            ggml_tensor bs = *b;
            bs.data = (char *) b->data + i2 * b->nb[2] + i3 * b->nb[3];
            bs.ne[2] = bs.ne[3] = 1;
            float * x = (float *) R.gather(&bs, lvk::GT_F32);
            float * y = (float *) R.temp((size_t) N * M * 4);
            const lvk::StepParams sp{0, N, 0, 0};
            lvk::StepParams * spd = (lvk::StepParams *) R.upload_small(&sp, sizeof sp);
            lvk::MvLaunch L;
            L.w = q; L.sp = spd; L.n_tokens = N; L.y = y;
            if (qt == lvk::Q4_1) {
                L.x = x;
                LVK_HIP(lvk::launch_matvec(L, lvk::PRO_ACTF, lvk::EPI_STORE, R.stream));
            } else {
                lvk::ActQ aq;
                aq.nb = K / 32;
                aq.d = (float *) R.temp((size_t) N * aq.nb * 4);
                aq.m = (float *) R.temp((size_t) N * aq.nb * 4);
                aq.qs = (uint4 *) R.temp((size_t) N * aq.nb * 16);
                LVK_HIP(lvk::launch_quantize_act(x, N, K, qt, aq, R.stream));
                L.xq = aq;
                LVK_HIP(lvk::launch_matvec(L, lvk::PRO_ACTQ, lvk::EPI_STORE, R.stream));
            }
            // [N][M] -> the node's (i2, i3) slice
            const int64_t ne[2] = {M, N};
            lvk::GView d = R.view(node);
            d.p += i2 * node->nb[2] + i3 * node->nb[3];
            d.ne[2] = d.ne[3] = 1;
            LVK_HIP(lvk::launch_g_cpy(contiguous_view(y, ne, 2, 4, lvk::GT_F32), d, R.stream));
        }
}

// the ops that only reinterpret their source: they write nothing and launch nothing
bool reinterprets(int op) {
    return op == GGML_OP_NONE || op == GGML_OP_RESHAPE || op == GGML_OP_VIEW || op == GGML_OP_PERMUTE ||
           op == GGML_OP_TRANSPOSE;
}

void run_node(GraphEngine & R, ggml_tensor * n) {
    if (reinterprets(n->op)) return;
    ggml_tensor * a = n->src0;
    ggml_tensor * b = n->src1;
    switch (n->op) {
        case GGML_OP_DUP:
        case GGML_OP_CPY:
            G_ASSERT(a->type == GGML_TYPE_F32 || a->type == GGML_TYPE_F16);
            G_ASSERT(n->type == GGML_TYPE_F32 || n->type == GGML_TYPE_F16);
            LVK_HIP(lvk::launch_g_cpy(R.view(a), R.view(n), R.stream));
            return;
        case GGML_OP_ADD:
        case GGML_OP_SUB:
        case GGML_OP_MUL:
        case GGML_OP_DIV: {
            G_ASSERT(a->type == GGML_TYPE_F32 && b->type == GGML_TYPE_F32 && n->type == GGML_TYPE_F32);
            const int op = n->op == GGML_OP_ADD ? lvk::GOP_ADD : n->op == GGML_OP_SUB ? lvk::GOP_SUB
                         : n->op == GGML_OP_MUL ? lvk::GOP_MUL : lvk::GOP_DIV;
            LVK_HIP(lvk::launch_g_binary(R.view(a), R.view(b), R.view(n), op, R.stream));
            return;
        }
        case GGML_OP_REPEAT:
            G_ASSERT(a->type == GGML_TYPE_F32);
            LVK_HIP(lvk::launch_g_binary(R.view(a), R.view(a), R.view(n), lvk::GOP_REPEAT, R.stream));
            return;
        case GGML_OP_SILU:
            G_ASSERT(a->type == GGML_TYPE_F32);
            LVK_HIP(lvk::launch_g_unary(R.view(a), R.view(n), lvk::GOP_SILU, 0.0f, 0, tables().silu_tab, R.stream));
            return;
        case GGML_OP_SCALE:
            G_ASSERT(a->type == GGML_TYPE_F32 && b->type == GGML_TYPE_F32);
            LVK_HIP(lvk::launch_g_unary(R.view(a), R.view(n), lvk::GOP_SCALE, R.read_scalar<float>(b, 0), 0, nullptr,
                                        R.stream));
            return;
        case GGML_OP_DIAG_MASK_INF:
            G_ASSERT(a->type == GGML_TYPE_F32);
            LVK_HIP(lvk::launch_g_unary(R.view(a), R.view(n), lvk::GOP_DIAG_MASK, 0.0f, R.read_scalar<int32_t>(b, 0),
                                        nullptr, R.stream));
            return;
        case GGML_OP_RMS_NORM:
            G_ASSERT(a->type == GGML_TYPE_F32);
            LVK_HIP(lvk::launch_g_rms_norm(R.view(a), R.view(n), R.stream));
            return;
        case GGML_OP_SOFT_MAX: {
            G_ASSERT(a->type == GGML_TYPE_F32);
            const Tables & T = tables();
            if (n->data != a->data) LVK_HIP(lvk::launch_g_cpy(R.view(a), R.view(n), R.stream));
            LVK_HIP(lvk::launch_g_soft_max(R.view(n), T.exp_tab, T.exp_mode, R.stream));
            return;
        }
        case GGML_OP_ROPE: {
            G_ASSERT(a->type == GGML_TYPE_F32 && a->nb[0] == sizeof(float));
            const int n_past = R.read_scalar<int32_t>(b, 0), n_dims = R.read_scalar<int32_t>(b, 1);
            const int mode = R.read_scalar<int32_t>(b, 2);
            G_ASSERT(n_dims % 2 == 0 && n_dims <= a->ne[0]);
            if (n->data != a->data) LVK_HIP(lvk::launch_g_cpy(R.view(a), R.view(n), R.stream));
            // {cos, sin} of p * theta_i0, theta = powf(10000, -i0 / n_dims) (ggml.c:7209-7213)
            const int i2_0 = mode == 0 ? 0 : n_past;
            const int64_t rows = a->ne[2] - i2_0;
            if (rows <= 0) return;
            std::vector<float2> cs((size_t) rows * (n_dims / 2));
            for (int64_t t = 0; t < rows; ++t) {
                const int p = mode == 0 ? n_past + (int) t : i2_0 + (int) t;
                for (int i0 = 0; i0 < n_dims; i0 += 2) {
                    const float theta = powf(10000.0f, ((float) -i0) / (float) n_dims);
                    const float ang = (float) p * theta;
                    cs[(size_t) t * (n_dims / 2) + i0 / 2] = make_float2(cosf(ang), sinf(ang));
                }
            }
            const float2 * csd = (const float2 *) R.upload_small(cs.data(), cs.size() * sizeof(float2));
            LVK_HIP(lvk::launch_g_rope(R.view(n), R.view(n), csd, n_dims, i2_0, R.stream));
            return;
        }
        case GGML_OP_GET_ROWS:
            G_ASSERT(b->type == GGML_TYPE_I32 && n->type == GGML_TYPE_F32);
            G_ASSERT(a->type == GGML_TYPE_Q4_0 || a->type == GGML_TYPE_Q4_1 || a->type == GGML_TYPE_F16 ||
                     a->type == GGML_TYPE_F32);
            if (b->op == GGML_OP_NONE && R.host_current(b->data, (size_t) b->ne[0] * sizeof(int32_t)))
                for (int64_t i = 0; i < b->ne[0]; ++i) {
                    const int32_t id = ((const int32_t *) b->data)[i];
                    if (id < 0 || id >= a->ne[1]) gabort("ggml_get_rows: row index out of range");
                }
            LVK_HIP(lvk::launch_g_get_rows(R.view(a), (const int32_t *) R.dev(b->data), b->ne[0], R.view(n), R.stream));
            return;
        case GGML_OP_MUL_MAT:
            G_ASSERT(b->type == GGML_TYPE_F32 && b->nb[0] == sizeof(float) && n->nb[0] == sizeof(float));
            if (a->type == GGML_TYPE_Q4_0 || a->type == GGML_TYPE_Q4_1) {
                run_mul_mat_q(R, a, b, n);
            } else if (a->type == GGML_TYPE_F16 || a->type == GGML_TYPE_F32) {
                // ggml.c:6134-6487: src1 to contiguous rows (f16 for an f16 src0: the INIT phase)
                G_ASSERT(a->nb[0] == TYPE_SIZE[a->type]);
                void * y = R.gather(b, a->type == GGML_TYPE_F16 ? lvk::GT_F16 : lvk::GT_F32);
                LVK_HIP(lvk::launch_g_mm_dot(R.view(a), y, b->ne[1], R.view(n), R.stream));
            } else {
                gabort("ggml_graph_compute: mul_mat source type not supported");
            }
            return;
        default: {
            char msg[96];
            snprintf(msg, sizeof msg, "ggml_graph_compute: op %d has no GPU implementation in llama.vk_amd", (int) n->op);
            gabort(msg);
        }
    }
}

bool writes_data(int op) { return !reinterprets(op); }

// every buffer range the graph reads or writes
std::vector<Span> collect_spans(const ggml_cgraph * g) {
    std::vector<Span> sp;
    auto add = [&](const ggml_tensor * t) {
        if (!t->data) gabort("ggml_graph_compute: a tensor has no data (no_alloc context)");
        sp.push_back(span_of(t));
    };
    for (int i = 0; i < g->n_leafs; ++i) add(g->leafs[i]);
    for (int i = 0; i < g->n_nodes; ++i) {
        add(g->nodes[i]);
        for_sources(g->nodes[i], add);
    }
    return sp;
}

// the bytes a node reads before any earlier node of this call wrote them (leaves, the caller's
// inputs, a KV cache) are the only ones that must come from the host
void upload_inputs(GraphEngine & R, const ggml_cgraph * g) {
    std::vector<Span> wr;          // written so far (unsorted; graphs are small)
    std::vector<Span> need;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        for_sources(n, [&](const ggml_tensor * t) {
            const std::vector<Span> parts = subtract(span_of(t), wr);
            need.insert(need.end(), parts.begin(), parts.end());
        });
        if (writes_data(n->op)) wr.push_back(span_of(n));
    }
    for (const Span & p : need) R.upload(R.mirror_of(p.lo), p.lo, p.hi);
}

void run_nodes(GraphEngine & R, const ggml_cgraph * g) {
    // LVK_GGML_SYNC=1: wait for every node and name the one that fails (debugging)
    static const bool sync_each = getenv("LVK_GGML_SYNC") && atoi(getenv("LVK_GGML_SYNC")) != 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        ggml_tensor * n = g->nodes[i];
        run_node(R, n);
        if (writes_data(n->op)) {
            R.written.push_back(span_of(n));
            R.drop_repacked(R.written.back().lo, R.written.back().hi);
        }
        if (!sync_each) continue;
        const hipError_t e = hipStreamSynchronize(R.stream);
        if (e != hipSuccess) {
            fprintf(stderr, "ggml_graph_compute: node %d (op %d, type %d, ne %lld %lld %lld %lld) failed: %s\n", i,
                    (int) n->op, (int) n->type, (long long) n->ne[0], (long long) n->ne[1], (long long) n->ne[2],
                    (long long) n->ne[3], hipGetErrorString(e));
            abort();
        }
    }
}

}  // namespace

extern "C" void ggml_graph_compute(struct ggml_context * ctx, struct ggml_cgraph * cgraph) {
    (void) ctx;
    std::lock_guard<std::mutex> lock(engine_mutex());
    const std::vector<Span> regions = merge_spans(collect_spans(cgraph));
    try {
        GraphEngine & R = engine();
        R.begin_call();
        R.map_regions(regions);
        R.refresh_used();
        upload_inputs(R, cgraph);
        run_nodes(R, cgraph);
        R.write_back();
        R.retire();
        fold_and_clear(R);
        R.last.mirrored = R.resident();
        g_last_stats = R.last;
    } catch (const lvk::Error & e) {
        gabort(e.msg.c_str());
    }
    g_have_engine = true;
    cgraph->perf_runs++;
}

extern "C" int lvk_ggml_stats(uint64_t * out, int n) {
    std::lock_guard<std::mutex> lock(engine_mutex());
    const DirtyTracker & T = tracker();
    const uint64_t v[8] = {g_last_stats.h2d, g_last_stats.d2h, g_last_stats.repack, g_last_stats.mirrored,
                           (uint64_t) (!T.enabled ? 0 : T.ok ? 2 : 1), (uint64_t) (g_have_engine ? 1 : 0),
                           g_last_stats.track_ns / 1000, g_last_stats.clear_ns / 1000};
    if (!out || n < 0) return -1;
    for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
    return 8;
}

// the caller rewrote [p, p + n) in a way the tracking cannot see (ggml_track.h): upload it again
extern "C" int lvk_ggml_invalidate(const void * p, size_t n) {
    std::lock_guard<std::mutex> lock(engine_mutex());
    if (!p) return -1;
    // every device's engine may mirror the range
    const char * a = (const char *) p;
    for (auto & kv : all_engines()) {
        for (auto & m : kv.second->mirrors) Tracking::invalidate(*m, a, a + n);
        kv.second->drop_repacked(a, a + n);
    }
    return 0;
}
