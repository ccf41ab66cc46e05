// ggml_track.cpp -- host change tracking of ggml_graph_compute's device mirrors (ggml_track.h).
// Plain host code: no HIP call; the one question only HIP can answer (is this address pinned
// or registered host memory) comes in as a callable.
#include "ggml_track.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

namespace lvk {
namespace track {

// ---- byte spans ---------------------------------------------------------------------------
std::vector<Span> merge_spans(std::vector<Span> v) {
    std::sort(v.begin(), v.end(), [](const Span & x, const Span & y) { return x.lo < y.lo; });
    std::vector<Span> m;
    for (const Span & s : v) {
        if (!m.empty() && s.lo <= m.back().hi) m.back().hi = std::max(m.back().hi, s.hi);
        else m.push_back(s);
    }
    return m;
}

std::vector<Span> subtract(Span s, const std::vector<Span> & written) {
    std::vector<Span> parts{s};
    for (const Span & w : written) {
        std::vector<Span> next;
        for (const Span & p : parts) {
            if (!overlaps(p.lo, p.hi, w.lo, w.hi)) { next.push_back(p); continue; }
            if (p.lo < w.lo) next.push_back({p.lo, w.lo});
            if (w.hi < p.hi) next.push_back({w.hi, p.hi});
        }
        parts.swap(next);
        if (parts.empty()) break;
    }
    return parts;
}

// ---- /proc/self/maps ----------------------------------------------------------------------
std::vector<MapEnt> read_maps() {
    std::vector<MapEnt> v;
    FILE * f = fopen("/proc/self/maps", "r");
    if (!f) return v;
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        MapEnt e;
        unsigned long lo = 0, hi = 0, off = 0, ino = 0;
        if (sscanf(line, "%lx-%lx %4s %lx %15s %lu", &lo, &hi, e.perms, &off, e.dev, &ino) < 6) continue;
        e.lo = lo; e.hi = hi; e.off = off; e.inode = ino;
        v.push_back(e);
    }
    fclose(f);
    return v;       // the kernel lists mappings in address order
}

const MapEnt * map_of(const std::vector<MapEnt> & v, uintptr_t a) {
    auto it = std::upper_bound(v.begin(), v.end(), a, [](uintptr_t x, const MapEnt & e) { return x < e.lo; });
    if (it == v.begin()) return nullptr;
    --it;
    return a < it->hi ? &*it : nullptr;
}

// ---- soft-dirty bits ----------------------------------------------------------------------
bool DirtyTracker::read(uintptr_t page0, size_t n, std::vector<uint64_t> & e) const {
    e.resize(n);
    const size_t want = n * 8;
    size_t got = 0;
    while (got < want) {
        const ssize_t r = pread(pagemap, (char *) e.data() + got, want - got, (off_t) (page0 * 8 + got));
        if (r <= 0) return false;
        got += (size_t) r;
    }
    return true;
}

bool DirtyTracker::clear() const { return pwrite(clear_refs, "4", 1, 0) == 1; }

DirtyTracker::DirtyTracker() {
    const char * e = getenv("LVK_GGML_CACHE");
    const int mode = e ? atoi(e) : 1;
    if (mode == 0) { enabled = false; return; }
    if (mode != 2) return;
    pagemap = open("/proc/self/pagemap", O_RDONLY | O_CLOEXEC);
    clear_refs = open("/proc/self/clear_refs", O_WRONLY | O_CLOEXEC);
    if (pagemap < 0 || clear_refs < 0) return;
    // self-test on a page of our own: written -> cleared -> written again
    void * p = mmap(nullptr, PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) return;
    volatile char * c = (volatile char *) p;
    std::vector<uint64_t> v;
    const uintptr_t pg = (uintptr_t) p / PAGE;
    c[0] = 1;
    bool good = clear() && read(pg, 1, v) && !written(v[0]);
    c[1] = 2;
    good = good && read(pg, 1, v) && written(v[0]);
    munmap(p, PAGE);
    ok = good;
}

DirtyTracker & tracker() {
    static DirtyTracker t;
    return t;
}

// ---- page state ---------------------------------------------------------------------------
std::pair<size_t, size_t> PageState::page_range(const char * a, const char * b) const {
    a = std::max(a, (const char *) lo);
    b = std::min(b, (const char *) hi);
    if (a > b) return {0, 0};
    // (an empty [a, a) inside a page still names that page, as the callers always had it)
    return {(uintptr_t) a / PAGE - page0(), (uintptr_t) (b - 1) / PAGE - page0() + 1};
}

void Tracking::snapshot() {
    if (!tracker().enabled) return;
    maps_now = read_maps();
    ro_alive.assign(ro_maps.size(), 0);
    for (size_t i = 0; i < ro_maps.size(); ++i) {
        const MapEnt * e = map_of(maps_now, ro_maps[i].lo);
        ro_alive[i] = e && e->same(ro_maps[i]);
    }
}

// the pages [i, j) of a range that lie in one mapping of this call, or in one gap between two
struct Tracking::PageRun {
    size_t i, j;
    const MapEnt * map;       // nullptr: no mapping this call saw
    bool shared() const { return map && map->perms[3] == 's'; }
    bool read_only() const { return map && !strchr(map->perms, 'w') && map->perms[3] == 'p'; }
};

namespace {
// f(run) for the runs of s's pages over the address-ordered mappings, in page order
template <class Run, class F> void for_each_run(const PageState & s, const std::vector<MapEnt> & maps, F && f) {
    const size_t np = s.pages();
    auto it = maps.begin();
    for (size_t i = 0; i < np;) {
        const uintptr_t a = (s.page0() + i) * PAGE;
        while (it != maps.end() && it->hi <= a) ++it;
        const bool inside = it != maps.end() && a >= it->lo;
        const uintptr_t lim = it == maps.end() ? UINTPTR_MAX : inside ? it->hi : it->lo;
        const size_t j = (size_t) std::min<uintptr_t>(np, i + (lim - a - 1) / PAGE + 1);
        f(Run{i, j, inside ? &*it : nullptr});
        i = j;
    }
}
}  // namespace

// Host memory HIP can DMA into (registered or pinned): no CPU-side tracking sees those writes.
// Decided per range from its first and last byte (a range that spans several allocations with
// a pinned one in the middle is not detected: probing the mappings in between can reach driver
// mappings), and decided again whenever the set of mappings over the range changed.  A range
// passed to hipHostRegister after its first use keeps its mappings: the caller says so with
// lvk_ggml_invalidate (lvk_ops.h), which also drops this decision.
void Tracking::decide_pinned(PageState & s, const Probe & is_hip_host) const {
    uint64_t sig = 1469598103934665603ull;
    for (const MapEnt & e : maps_now) {
        if (e.hi <= (uintptr_t) s.lo || e.lo >= (uintptr_t) s.hi) continue;
        for (uint64_t v : {(uint64_t) e.lo, (uint64_t) e.hi, e.inode, e.off}) sig = (sig ^ v) * 1099511628211ull;
    }
    if (sig != s.maps_sig) { s.hip_host = -1; s.maps_sig = sig; }
    if (s.hip_host >= 0) return;
    s.hip_host = 0;
    for (const char * q : {(const char *) s.lo, (const char *) s.hi - 1}) {
        // only addresses mapped now: part of a range may have been unmapped since it was
        // mirrored (a freed scratch buffer), and HIP's pointer query faults on some unmapped
        // host addresses
        if (map_of(maps_now, (uintptr_t) q) && is_hip_host(q)) s.hip_host = 1;
    }
}

// LVK_GGML_CACHE=2: the soft-dirty bits, one read per run.  A page uploaded from a read-only
// private mapping that is still the same mapping (ro_alive: same range, offset, inode, device
// and permissions) is kept without a read -- the process cannot have written it, and a 7B / 65B
// weight mirror is almost all such pages.  A page whose mapping is gone or was replaced (munmap
// + mmap of another file at the same range) is dropped; a page uploaded while writable that now
// sits in a read-only mapping (written, then mprotect'ed) has its bit read like a writable page.
void Tracking::drop_soft_dirty(PageState & s, const PageRun & r, std::vector<uint64_t> & bits) const {
    const bool ro = r.read_only();
    bool need_read = !ro;
    if (ro) {
        for (size_t k = r.i; k < r.j; ++k) {
            if (!s.valid[k]) continue;
            if (s.ro[k] < 0) need_read = true;                        // uploaded writable
            else if (!ro_alive[(size_t) s.ro[k]]) s.valid[k] = 0;     // another mapping
        }
    }
    if (!need_read) return;
    if (!tracker().read(s.page0() + r.i, r.j - r.i, bits)) return s.drop(r.i, r.j);
    for (size_t k = 0; k < bits.size(); ++k)
        if ((!ro || s.ro[r.i + k] < 0) && DirtyTracker::written(bits[k])) s.valid[r.i + k] = 0;
}

// LVK_GGML_CACHE=1: only pages uploaded from a read-only mapping that is still itself are kept
void Tracking::drop_not_read_only(PageState & s, const PageRun & r) const {
    for (size_t k = r.i; k < r.j; ++k)
        if (s.ro[k] < 0 || !ro_alive[(size_t) s.ro[k]]) s.valid[k] = 0;
}

// pages of shared mappings (or of no mapping this call saw) are written behind our back
void Tracking::drop_shared_or_unmapped(PageState & s, const PageRun & r) {
    if (!r.map || r.shared()) s.drop(r.i, r.j);
}

void Tracking::refresh(PageState & s, const Probe & is_hip_host) const {
    const DirtyTracker & T = tracker();
    if (!T.enabled) return s.drop_all();
    decide_pinned(s, is_hip_host);
    if (s.hip_host == 1) return s.drop_all();
    std::vector<uint64_t> bits;
    for_each_run<PageRun>(s, maps_now, [&](const PageRun & r) {
        if (T.ok) drop_soft_dirty(s, r, bits);
        else drop_not_read_only(s, r);
        drop_shared_or_unmapped(s, r);
    });
}

int32_t Tracking::ro_id(uintptr_t page) {
    const MapEnt * e = map_of(maps_now, page * PAGE);
    if (!e || strchr(e->perms, 'w')) return -1;
    for (size_t i = 0; i < ro_maps.size(); ++i)
        if (ro_maps[i].same(*e)) return (int32_t) i;
    ro_maps.push_back(*e);
    ro_alive.push_back(1);
    return (int32_t) ro_maps.size() - 1;
}

std::vector<Span> Tracking::invalid_runs(PageState & s, const char * a, const char * b) {
    std::vector<Span> runs;
    // the mapping identity of every page uploaded from a read-only mapping, in both caching
    // modes (refresh drops the page when that mapping is no longer the same one)
    const bool track_ro = tracker().enabled;
    const auto [i0, i1] = s.page_range(a, b);
    for (size_t i = i0; i < i1;) {
        if (s.valid[i]) { ++i; continue; }
        size_t j = i;
        while (j < i1 && !s.valid[j]) ++j;
        runs.push_back({std::max((const char *) ((s.page0() + i) * PAGE), (const char *) s.lo),
                        std::min((const char *) ((s.page0() + j) * PAGE), (const char *) s.hi)});
        for (size_t k = i; k < j; ++k) {
            s.valid[k] = 1;
            s.ro[k] = track_ro ? ro_id(s.page0() + k) : -1;
        }
        i = j;
    }
    return runs;
}

void Tracking::adopt(PageState & into, const PageState & from) {
    const size_t np = from.pages(), d = from.page0() - into.page0();
    for (size_t i = 0; i < np; ++i) {
        // a page only partly inside the old range holds bytes the old mirror never had
        const char * p0 = (const char *) ((from.page0() + i) * PAGE);
        const bool whole = p0 >= from.lo && p0 + PAGE <= from.hi;
        const bool edge_ok = (p0 < from.lo ? into.lo >= from.lo : true) && (p0 + PAGE > from.hi ? into.hi <= from.hi : true);
        into.valid[d + i] = from.valid[i] && (whole || edge_ok);
        into.ro[d + i] = from.ro[i];
    }
}

void Tracking::invalidate(PageState & s, const char * a, const char * b) {
    if (!overlaps(a, b, s.lo, s.hi)) return;
    const auto [i0, i1] = s.page_range(a, b);
    s.drop(i0, i1);
    s.hip_host = -1;      // e.g. the range was hipHostRegister'ed since its first use
}

}  // namespace track
}  // namespace lvk
