// ggml_internal.h -- what the units behind include/ggml.h share: ggml_api.cpp (the builder),
// ggml_graph.cpp (ggml_graph_compute on the GPU) and ggml_track.cpp (host change tracking).
// Host code only (no HIP).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../../include/ggml.h"
#include "ggml_track.h"

namespace lvk {
int64_t now_us();       // lvk_context.cpp: the runtime's one clock
}

namespace ggml_impl {

// bytes per block and elements per block (ggml.c GGML_TYPE_SIZE / GGML_BLCK_SIZE)
constexpr size_t TYPE_SIZE[GGML_TYPE_COUNT] = {20, 24, 1, 2, 4, 2, 4};
constexpr int BLCK_SIZE[GGML_TYPE_COUNT] = {32, 32, 1, 1, 1, 1, 1};

[[noreturn]] inline void gabort(const char * what) {
    fprintf(stderr, "llama.vk_amd ggml: %s\n", what);
    abort();
}
#define G_ASSERT(x)                                                                             \
    do {                                                                                        \
        if (!(x)) ggml_impl::gabort("GGML_ASSERT: " #x);                                        \
    } while (0)

// bytes a strided tensor spans from its data pointer
inline size_t span_bytes(const ggml_tensor * t) {
    // quantized rows are contiguous blocks; other types may have any stride in any
    // dimension (a transpose swaps nb[0] and nb[1])
    const bool quant = BLCK_SIZE[t->type] > 1;
    size_t s = quant ? (size_t) (t->ne[0] / BLCK_SIZE[t->type]) * TYPE_SIZE[t->type] : TYPE_SIZE[t->type];
    for (int d = quant ? 1 : 0; d < GGML_MAX_DIMS; ++d)
        if (t->ne[d] > 1) s += (size_t) (t->ne[d] - 1) * t->nb[d];
    return s;
}
inline lvk::track::Span span_of(const ggml_tensor * t) {
    return {(const char *) t->data, (const char *) t->data + span_bytes(t)};
}

}  // namespace ggml_impl
