// ggml_track.h -- which host pages of ggml_graph_compute's device mirrors must travel again.
// Host code only (no HIP): ggml_graph.cpp owns the device side, tools/ggml_graph/track_test.cpp
// runs this unit alone on a CPU.
//
// A graph's tensors live in caller memory that the caller may rewrite between calls (the next
// token ids, a KV cache it restored ...), while most of it -- the weights -- never changes.
// The mirrors keep host ranges in HBM across calls and upload a page again only when the host
// may have written it since it was uploaded:
//   * pages inside a mapping this process cannot write (llama.cpp's PROT_READ model-file
//     mapping, or a buffer the caller made read-only with mprotect) stay valid while that
//     mapping (address range, offset, device, inode, permissions in /proc/self/maps) is
//     unchanged -- a caller that re-enables writes, writes and protects again between two
//     calls must say so with lvk_ggml_invalidate;
//   * writable pages are uploaded again on every call.  LVK_GGML_CACHE=2 tracks them with
//     the kernel's soft-dirty bits instead (/proc/self/pagemap bit 55, cleared by "4" into
//     /proc/self/clear_refs; a new mapping reads dirty, a page that is neither present nor
//     swapped counts as written).  That is opt-in: the clear is process-wide, and in a HIP
//     process the call after it stalls for ~0.2 s (tools/ggml_graph/track_cost.c, DESIGN.md
//     section 5), more than re-uploading gigabytes of writable pages costs;
//   * pages the CPU-side tracking cannot see written are never kept: pages of shared mappings
//     (another mapping or process may write them; HIP's pinned host allocations are shared
//     mappings of the driver's device file) and host memory registered with HIP (a DMA into
//     it, e.g. hipMemcpy D2H, bypasses this process's page tables) are uploaded on every call;
//   * only bytes a node reads before any node of the call writes them are uploaded at all
//     (a node's output buffer never travels host -> device), and only the bytes the nodes
//     wrote travel back.
// The soft-dirty bits are per process: before a call clears them, every engine (one per
// device) folds the bits into the validity of all its mirrors.
// LVK_GGML_CACHE=0 turns the caching off (every needed page uploaded on every call); 1 (the
// default) keeps pages of read-only mappings; 2 adds the soft-dirty tracking of writable pages.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

namespace lvk {
namespace track {

constexpr size_t PAGE = 4096;

// ---- byte spans ---------------------------------------------------------------------------
struct Span {
    const char * lo;
    const char * hi;
};
inline bool overlaps(const char * a0, const char * a1, const char * b0, const char * b1) { return a0 < b1 && b0 < a1; }
// sorted by lo, overlapping and touching spans merged
std::vector<Span> merge_spans(std::vector<Span> v);
// the parts of s that no span of `written` covers
std::vector<Span> subtract(Span s, const std::vector<Span> & written);

// ---- /proc/self/maps ----------------------------------------------------------------------
struct MapEnt {
    uintptr_t lo = 0, hi = 0;
    uint64_t off = 0, inode = 0;
    char perms[5] = {0};
    char dev[16] = {0};
    bool same(const MapEnt & o) const {
        return lo == o.lo && hi == o.hi && off == o.off && inode == o.inode && !strcmp(perms, o.perms) &&
               !strcmp(dev, o.dev);
    }
};
std::vector<MapEnt> read_maps();      // in address order, as the kernel lists them
const MapEnt * map_of(const std::vector<MapEnt> & v, uintptr_t a);

// ---- soft-dirty bits (LVK_GGML_CACHE) -----------------------------------------------------
struct DirtyTracker {
    int pagemap = -1, clear_refs = -1;
    bool enabled = true;       // LVK_GGML_CACHE != 0
    bool ok = false;           // LVK_GGML_CACHE=2 and the soft-dirty bits work (self-test)
    DirtyTracker();
    bool read(uintptr_t page0, size_t n, std::vector<uint64_t> & e) const;
    static bool written(uint64_t e) {
        const bool present = (e >> 63) & 1, swapped = (e >> 62) & 1, soft_dirty = (e >> 55) & 1;
        return soft_dirty || (!present && !swapped);
    }
    bool clear() const;
};
DirtyTracker & tracker();

// ---- per-page state of one mirrored host range --------------------------------------------
// valid[i]: the bytes of host page (lo / PAGE + i) inside [lo, hi) equal the device copy
struct PageState {
    char * lo = nullptr;
    char * hi = nullptr;
    std::vector<uint8_t> valid;
    std::vector<int32_t> ro;       // per page: the read-only mapping it was uploaded from, or -1
    int hip_host = -1;             // 1: HIP-registered / pinned host memory (never cached); -1 unknown
    uint64_t maps_sig = 0;         // the mappings over [lo, hi) when hip_host was decided
    uintptr_t page0() const { return (uintptr_t) lo / PAGE; }
    size_t pages() const { return (uintptr_t) (hi - 1) / PAGE - page0() + 1; }
    // [lo_, hi_) with every page invalid
    void set_range(char * lo_, char * hi_) {
        lo = lo_;
        hi = hi_;
        valid.assign(pages(), 0);
        ro.assign(pages(), -1);
    }
    // the pages [i0, i1) that [a, b) touches, clamped to the range (empty: i0 == i1)
    std::pair<size_t, size_t> page_range(const char * a, const char * b) const;
    void drop(size_t i0, size_t i1) { std::memset(valid.data() + i0, 0, i1 - i0); }
    void drop_all() { drop(0, valid.size()); }
};

// the mappings of this call and the identities of the read-only mappings pages came from
struct Tracking {
    std::vector<MapEnt> ro_maps;           // identities of the read-only mappings pages came from
    std::vector<uint8_t> ro_alive;         // this call: is ro_maps[i] still mapped, unchanged
    std::vector<MapEnt> maps_now;          // /proc/self/maps of this call

    using Probe = std::function<bool(const void *)>;   // is this (mapped) address HIP host memory

    // read /proc/self/maps and see which read-only mappings are still themselves
    void snapshot();
    // pages the host may have written since they were uploaded lose their validity
    void refresh(PageState & s, const Probe & is_hip_host) const;
    // the byte ranges of the invalid pages of s that [a, b) touches, clipped to [lo, hi): they
    // must travel host -> device.  Marks those pages valid and records their mapping identity
    std::vector<Span> invalid_runs(PageState & s, const char * a, const char * b);
    // `from` lies inside `into`: its fully covered valid pages stay valid
    static void adopt(PageState & into, const PageState & from);
    // the caller rewrote [a, b) where the tracking cannot see it; also drops the pinned decision
    static void invalidate(PageState & s, const char * a, const char * b);

private:
    struct PageRun;
    void decide_pinned(PageState & s, const Probe & is_hip_host) const;
    void drop_soft_dirty(PageState & s, const PageRun & r, std::vector<uint64_t> & bits) const;
    void drop_not_read_only(PageState & s, const PageRun & r) const;
    static void drop_shared_or_unmapped(PageState & s, const PageRun & r);
    int32_t ro_id(uintptr_t page);
};

}  // namespace track
}  // namespace lvk
