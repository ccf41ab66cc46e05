// track_test.cpp -- the host change tracking of ggml_graph_compute (llama.vk_amd/csrc/runtime/
// ggml_track.cpp) on its own: no library, no GPU.  Built with AddressSanitizer + UBSan linked in
// (Makefile) and run once per case by tests/test_ggml_track.py under LVK_GGML_CACHE=1 and =2.
// "Is this address HIP host memory" is answered by the test: never, except in the pinned case.
// Under LVK_GGML_CACHE=2 the first line says whether the kernel's soft-dirty bits work; where
// they do not, the tracker falls back to mode 1 and every case must behave exactly as there.
// usage: track_test private|ro-kept|remap|mprotect|shared|hole|pinned|edges|adopt|spans
//        (prints "ok <case>" and exits 0)
#ifndef _GNU_SOURCE
#define _GNU_SOURCE 1       // memfd_create
#endif
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../llama.vk_amd/csrc/runtime/ggml_internal.h"

using namespace lvk::track;

#define CHECK(x)                                                                      \
    do {                                                                              \
        if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } \
    } while (0)

static bool never(const void *) { return false; }

static void * map_or_die(void * at, size_t n, int prot, int flags, int fd) {
    void * p = mmap(at, n, prot, flags, fd, 0);
    if (p == MAP_FAILED) { perror("mmap"); exit(2); }
    return p;
}
static char * anon_rw(size_t pages) {
    char * p = (char *) map_or_die(nullptr, pages * PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1);
    memset(p, 1, pages * PAGE);       // every page present
    return p;
}
// a temporary file of `pages` pages (unlinked at once; a mapping keeps it alive)
static int temp_file(size_t pages) {
    char name[] = "/tmp/lvk_track_XXXXXX";
    const int fd = mkstemp(name);
    if (fd < 0) { perror("mkstemp"); exit(2); }
    unlink(name);
    const std::vector<char> v(pages * PAGE, 3);
    if (write(fd, v.data(), v.size()) != (ssize_t) v.size()) { perror("write"); exit(2); }
    return fd;
}
static int shared_fd(size_t pages) {
    const int fd = memfd_create("lvk_track_test", 0);
    if (fd < 0 || ftruncate(fd, (off_t) (pages * PAGE)) != 0) { perror("memfd"); exit(2); }
    return fd;
}

static size_t n_valid(const PageState & s) {
    size_t n = 0;
    for (uint8_t v : s.valid) n += v != 0;
    return n;
}
static PageState state(char * lo, char * hi) {
    PageState s;
    s.set_range(lo, hi);
    CHECK(s.valid.size() == s.pages() && s.ro.size() == s.pages() && n_valid(s) == 0);
    return s;
}
// one call's view of s: everything of [lo, hi) that is invalid travels and becomes valid
static std::vector<Span> upload_all(Tracking & T, PageState & s) {
    T.snapshot();
    std::vector<Span> r = T.invalid_runs(s, s.lo, s.hi);
    CHECK(n_valid(s) == s.pages());
    return r;
}
static void next_call(Tracking & T, PageState & s, const Tracking::Probe & probe = never) {
    T.snapshot();
    T.refresh(s, probe);
}

// a writable anonymous range: dropped on every call; with working soft-dirty bits a page is
// dropped only when it was written since the clear
static void case_private(bool soft) {
    char * p = anon_rw(4);
    PageState s = state(p + 100, p + 4 * PAGE - 100);
    Tracking T;
    const std::vector<Span> r = upload_all(T, s);
    CHECK(r.size() == 1 && r[0].lo == s.lo && r[0].hi == s.hi);
    for (int32_t id : s.ro) CHECK(id == -1);
    if (soft) CHECK(tracker().clear());
    p[2 * PAGE + 7] = 9;
    next_call(T, s);
    if (!soft) CHECK(n_valid(s) == 0);
    else CHECK(s.valid[0] && s.valid[1] && !s.valid[2] && s.valid[3]);
}

// a read-only private file mapping (llama.cpp's weights): kept while it is the same mapping
static void case_ro_kept(bool remap) {
    const size_t n = 4 * PAGE;
    char * p = (char *) map_or_die(nullptr, n, PROT_READ, MAP_PRIVATE, temp_file(4));
    PageState s = state(p + 100, p + n - 100);
    Tracking T;
    CHECK(upload_all(T, s).size() == 1);
    for (int32_t id : s.ro) CHECK(id == 0);
    if (remap) {       // another file at the same address, same permissions
        const int fd = temp_file(4);
        CHECK(munmap(p, n) == 0);
        CHECK(map_or_die(p, n, PROT_READ, MAP_PRIVATE | MAP_FIXED, fd) == p);
    }
    next_call(T, s);
    CHECK(n_valid(s) == (remap ? 0 : s.pages()));
    const std::vector<Span> again = T.invalid_runs(s, s.lo, s.hi);
    CHECK(remap ? again.size() == 1 && again[0].lo == s.lo && again[0].hi == s.hi : again.empty());
}

// uploaded while writable (ro == -1), then written and made read-only: no mapping identity
// vouches for the pages; only the soft-dirty bit can
static void case_mprotect(bool soft) {
    char * p = anon_rw(4);
    PageState s = state(p, p + 4 * PAGE);
    Tracking T;
    upload_all(T, s);
    for (int32_t id : s.ro) CHECK(id == -1);
    if (soft) CHECK(tracker().clear());
    p[PAGE + 1] = 5;
    CHECK(mprotect(p, 4 * PAGE, PROT_READ) == 0);
    next_call(T, s);
    if (!soft) CHECK(n_valid(s) == 0);
    else CHECK(!s.valid[1]);
}

// a MAP_SHARED view: another view may write the pages, never kept, read-only or not
static void case_shared() {
    for (int prot : {PROT_READ | PROT_WRITE, PROT_READ}) {
        char * p = (char *) map_or_die(nullptr, 4 * PAGE, prot, MAP_SHARED, shared_fd(4));
        PageState s = state(p, p + 4 * PAGE);
        Tracking T;
        upload_all(T, s);
        next_call(T, s);
        CHECK(n_valid(s) == 0);
    }
}

// two adjacent mappings in one range, the second unmapped between the calls: its pages are
// dropped, the first mapping's pages follow their own rule (read-only file pages: kept), and
// no address in the hole is looked at
static void case_hole() {
    char * p = (char *) map_or_die(nullptr, 6 * PAGE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1);
    map_or_die(p, 3 * PAGE, PROT_READ, MAP_PRIVATE | MAP_FIXED, temp_file(3));
    map_or_die(p + 3 * PAGE, 3 * PAGE, PROT_READ, MAP_PRIVATE | MAP_FIXED, temp_file(3));
    PageState s = state(p + 10, p + 6 * PAGE - 10);
    Tracking T;
    upload_all(T, s);
    CHECK(munmap(p + 3 * PAGE, 3 * PAGE) == 0);
    std::vector<const void *> asked;
    next_call(T, s, [&](const void * q) { asked.push_back(q); return false; });
    CHECK(asked.size() == 1 && asked[0] == s.lo);       // hi - 1 lies in the hole
    for (size_t i = 0; i < 6; ++i) CHECK(s.valid[i] == (i < 3));
    const std::vector<Span> r = T.invalid_runs(s, s.lo, s.hi);
    CHECK(r.size() == 1 && r[0].lo == p + 3 * PAGE && r[0].hi == s.hi);
}

// HIP host memory: never kept, and HIP is asked again only after the mappings over the range
// changed or after an invalidate -- and only about addresses that are mapped
static void case_pinned() {
    char * p = (char *) map_or_die(nullptr, 4 * PAGE, PROT_READ | PROT_WRITE, MAP_SHARED, shared_fd(4));
    PageState s = state(p + 8, p + 4 * PAGE - 8);
    Tracking T;
    std::vector<const void *> asked;
    const Tracking::Probe pinned = [&](const void * q) { asked.push_back(q); return true; };
    upload_all(T, s);
    next_call(T, s, pinned);
    CHECK(asked.size() == 2 && asked[0] == s.lo && asked[1] == s.hi - 1 && s.hip_host == 1 && n_valid(s) == 0);
    upload_all(T, s);
    next_call(T, s, pinned);                             // same mappings: not asked again
    CHECK(asked.size() == 2 && n_valid(s) == 0);
    CHECK(mprotect(p + PAGE, PAGE, PROT_READ) == 0);     // the mapping splits: asked again
    upload_all(T, s);
    next_call(T, s, pinned);
    CHECK(asked.size() == 4 && n_valid(s) == 0);
    upload_all(T, s);
    Tracking::invalidate(s, s.lo + PAGE, s.lo + PAGE + 1);
    CHECK(s.hip_host == -1 && n_valid(s) == s.pages() - 1 && !s.valid[1]);
    next_call(T, s, pinned);
    CHECK(asked.size() == 6 && n_valid(s) == 0);
    CHECK(munmap(p + 3 * PAGE, PAGE) == 0);              // hi - 1 is no longer mapped
    next_call(T, s, pinned);
    CHECK(asked.size() == 7 && asked[6] == s.lo && n_valid(s) == 0);
}

// invalid_runs against a brute-force restatement: per byte of the (unaligned) range, it travels
// iff its page is invalid and intersects [a, b)
static void case_edges() {
    const size_t np = 5;
    char * p = anon_rw(np);
    char * lo = p + 100;
    char * hi = p + np * PAGE - 300;
    const std::vector<std::pair<char *, char *>> asks = {
        {lo, hi}, {lo, lo + 1}, {hi - 1, hi}, {p + PAGE + 10, p + PAGE + 20}, {p + PAGE + 10, p + 3 * PAGE + 1},
        {p + 2 * PAGE, p + 3 * PAGE}, {p + 2 * PAGE - 1, p + 3 * PAGE + 1}, {lo, p + PAGE}, {p + 4 * PAGE, hi}};
    Tracking T;
    T.snapshot();
    for (unsigned mask = 0; mask < (1u << np); ++mask)
        for (const auto & ab : asks) {
            PageState s = state(lo, hi);
            for (size_t i = 0; i < np; ++i) s.valid[i] = (mask >> i) & 1;
            std::vector<uint8_t> want((size_t) (hi - lo), 0), got(want.size(), 0), valid_after = s.valid;
            for (size_t i = 0; i < np; ++i) {
                char * p0 = p + i * PAGE;
                if (s.valid[i] || !(p0 < ab.second && ab.first < p0 + PAGE)) continue;
                valid_after[i] = 1;
                for (char * c = std::max(p0, lo); c < std::min(p0 + PAGE, hi); ++c) want[(size_t) (c - lo)] = 1;
            }
            const char * prev = nullptr;
            for (const Span & r : T.invalid_runs(s, ab.first, ab.second)) {
                CHECK(r.lo < r.hi && r.lo >= lo && r.hi <= hi && (!prev || prev < r.lo));   // clipped, ordered, merged
                prev = r.hi;
                for (const char * c = r.lo; c < r.hi; ++c) got[(size_t) (c - lo)] = 1;
            }
            CHECK(got == want && s.valid == valid_after);
        }
    const PageState s = state(lo, hi);
    CHECK(s.page_range(lo, hi) == std::make_pair((size_t) 0, np));
    CHECK(s.page_range(lo - 64, hi + 64) == std::make_pair((size_t) 0, np));                // clamped
    CHECK(s.page_range(p + PAGE, p + PAGE + 1) == std::make_pair((size_t) 1, (size_t) 2));
}

// validity carried into a wider range: interior pages keep it; a page only partly inside the
// old range keeps it only when the new range does not reach beyond the old one on that side
static void case_adopt() {
    char * p = anon_rw(8);
    PageState old = state(p + PAGE + 100, p + 4 * PAGE - 100);       // pages 1..3 of the buffer
    old.valid = {1, 1, 1};
    old.ro = {7, 8, 9};
    for (bool below : {false, true})
        for (bool above : {false, true}) {
            PageState n = state(old.lo - (below ? 50 : 0), old.hi + (above ? 50 : 0));
            Tracking::adopt(n, old);
            CHECK(n.valid[0] == !below && n.valid[1] == 1 && n.valid[2] == !above);
            CHECK(n.ro[0] == 7 && n.ro[1] == 8 && n.ro[2] == 9);
        }
    // two old ranges into one wider one, across pages neither had: an invalid page stays invalid,
    // and page 3, which b covers only from byte 5 on, is not carried (n begins below b)
    PageState a = state(p, p + 2 * PAGE), b = state(p + 3 * PAGE + 5, p + 6 * PAGE);
    a.valid = {1, 0};
    b.valid = {1, 1, 1};
    PageState n = state(p, p + 8 * PAGE);
    Tracking::adopt(n, a);
    Tracking::adopt(n, b);
    CHECK(n.valid == std::vector<uint8_t>({1, 0, 0, 0, 1, 1, 0, 0}));
}

static bool same(const std::vector<Span> & a, const std::vector<Span> & b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].lo != b[i].lo || a[i].hi != b[i].hi) return false;
    return true;
}
static void case_spans() {
    static char m[512];
    auto S = [&](int lo, int hi) { return Span{m + lo, m + hi}; };
    CHECK(same(merge_spans({S(30, 40), S(0, 10), S(10, 20)}), {S(0, 20), S(30, 40)}));        // touching, disjoint
    CHECK(same(merge_spans({S(20, 30), S(0, 100), S(90, 120)}), {S(0, 120)}));                // nested, overlapping
    CHECK(merge_spans({}).empty());
    CHECK(same(subtract(S(100, 200), {S(0, 100), S(200, 300)}), {S(100, 200)}));              // before, after
    CHECK(same(subtract(S(100, 200), {S(120, 130)}), {S(100, 120), S(130, 200)}));            // inside
    CHECK(subtract(S(100, 200), {S(50, 250)}).empty());                                       // covering
    CHECK(same(subtract(S(100, 200), {S(50, 110), S(190, 300)}), {S(110, 190)}));             // straddling both ends
    CHECK(same(subtract(S(100, 200), {S(120, 130), S(125, 150), S(100, 105)}), {S(105, 120), S(150, 200)}));
    // a transposed f32 view of a 5 x 3 matrix: nb[0] > nb[1], and still the matrix's 60 bytes
    ggml_tensor t;
    memset(&t, 0, sizeof t);
    t.type = GGML_TYPE_F32;
    t.data = m;
    const int64_t ne[4] = {3, 5, 1, 1};
    const size_t nb[4] = {20, 4, 60, 60};
    for (int i = 0; i < 4; ++i) { t.ne[i] = ne[i]; t.nb[i] = nb[i]; }
    CHECK(ggml_impl::span_bytes(&t) == 60);
    CHECK(ggml_impl::span_of(&t).lo == m && ggml_impl::span_of(&t).hi == m + 60);
    // three Q4_0 rows of two blocks, rows padded to 48 bytes
    t.type = GGML_TYPE_Q4_0;
    const int64_t qne[4] = {64, 3, 1, 1};
    const size_t qnb[4] = {20, 48, 144, 144};
    for (int i = 0; i < 4; ++i) { t.ne[i] = qne[i]; t.nb[i] = qnb[i]; }
    CHECK(ggml_impl::span_bytes(&t) == 40 + 2 * 48);
}

int main(int argc, char ** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    const char * e = getenv("LVK_GGML_CACHE");
    const int mode = e ? atoi(e) : 1;
    const DirtyTracker & D = tracker();
    CHECK(D.enabled == (mode != 0) && (mode == 2 || !D.ok));
    if (mode == 2) printf("soft-dirty: %s\n", D.ok ? "working" : "not working, tracking as under LVK_GGML_CACHE=1");
    if (c == "private") case_private(D.ok);
    else if (c == "ro-kept") case_ro_kept(false);
    else if (c == "remap") case_ro_kept(true);
    else if (c == "mprotect") case_mprotect(D.ok);
    else if (c == "shared") case_shared();
    else if (c == "hole") case_hole();
    else if (c == "pinned") case_pinned();
    else if (c == "edges") case_edges();
    else if (c == "adopt") case_adopt();
    else if (c == "spans") case_spans();
    else { fprintf(stderr, "usage: track_test <case>\n"); return 2; }
    printf("ok %s\n", c.c_str());
    return 0;
}
