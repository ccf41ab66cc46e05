// ggml_api.cpp -- the ggml builder of include/ggml.h on llama.vk_amd: contexts, tensors, operator
// nodes and graphs.  Host code only (no HIP).
//
// The reference builds llama_eval_internal (llama.cpp:927-1197) as a ggml graph over host
// tensors and runs it with ggml_graph_compute (ggml.h:660; dispatch ggml.c:8562-8716).
// This library keeps that API for callers that drive ggml themselves:
//   * contexts are real memory pools with the reference's accounting (an object header,
//     the tensor, its data, 16-byte aligned; scratch buffers), so callers that size their
//     pools like llama.cpp does fit;
//   * struct ggml_tensor is the reference's layout, views / permutes / reshapes are
//     metadata only, as in ggml;
//   * ggml_graph_compute runs the graph on the GPU (ggml_graph.cpp).
#include <immintrin.h>

#include <algorithm>
#include <cinttypes>
#include <cstring>

#include "ggml_internal.h"

using namespace ggml_impl;

namespace {

constexpr size_t MEM_ALIGN = 16;
static_assert(sizeof(ggml_object) % MEM_ALIGN == 0, "ggml_object size");
static_assert(sizeof(ggml_tensor) % MEM_ALIGN == 0, "ggml_tensor size");

__attribute__((target("f16c"))) uint16_t h_f32_to_f16(float f) { return _cvtss_sh(f, 0); }
__attribute__((target("f16c"))) float h_f16_to_f32(uint16_t h) { return _cvtsh_ss(h); }

// element i of a non-quantized tensor as T (int32_t or float), with C's conversions
template <class T> T get_1d(const ggml_tensor * t, int i, const char * quantized) {
    switch (t->type) {
        case GGML_TYPE_I8: return (T) ((int8_t *) t->data)[i];
        case GGML_TYPE_I16: return (T) ((int16_t *) t->data)[i];
        case GGML_TYPE_I32: return (T) ((int32_t *) t->data)[i];
        case GGML_TYPE_F16: return (T) h_f16_to_f32(((uint16_t *) t->data)[i]);
        case GGML_TYPE_F32: return (T) ((float *) t->data)[i];
        default: gabort(quantized);
    }
}
template <class T> void set_1d(const ggml_tensor * t, int i, T v, const char * quantized) {
    switch (t->type) {
        case GGML_TYPE_I8: ((int8_t *) t->data)[i] = (int8_t) v; break;
        case GGML_TYPE_I16: ((int16_t *) t->data)[i] = (int16_t) v; break;
        case GGML_TYPE_I32: ((int32_t *) t->data)[i] = (int32_t) v; break;
        case GGML_TYPE_F16: ((uint16_t *) t->data)[i] = h_f32_to_f16((float) v); break;
        case GGML_TYPE_F32: ((float *) t->data)[i] = (float) v; break;
        default: gabort(quantized);
    }
}

}  // namespace

struct ggml_context {
    size_t mem_size = 0;
    char * mem_buffer = nullptr;
    bool mem_owned = false;
    bool no_alloc = false;
    ggml_object * objects_begin = nullptr;
    ggml_object * objects_end = nullptr;
    ggml_scratch scratch{0, 0, nullptr};
    ggml_scratch scratch_save{0, 0, nullptr};
};

namespace {

bool is_contiguous(const ggml_tensor * t) {
    return t->nb[0] == TYPE_SIZE[t->type] && t->nb[1] == (t->nb[0] * t->ne[0]) / BLCK_SIZE[t->type] &&
           t->nb[2] == t->nb[1] * t->ne[1] && t->nb[3] == t->nb[2] * t->ne[2];
}
bool same_shape(const ggml_tensor * a, const ggml_tensor * b) {
    return a->ne[0] == b->ne[0] && a->ne[1] == b->ne[1] && a->ne[2] == b->ne[2] && a->ne[3] == b->ne[3];
}

ggml_tensor * new_tensor_impl(ggml_context * ctx, ggml_type type, int n_dims, const int64_t * ne, void * data) {
    G_ASSERT(type < GGML_TYPE_COUNT && n_dims >= 1 && n_dims <= GGML_MAX_DIMS);
    ggml_object * cur = ctx->objects_end;
    const size_t cur_end = cur ? cur->offs + cur->size : 0;
    size_t need = 0;
    if (!data && !ctx->no_alloc) {
        need = TYPE_SIZE[type] * (ne[0] / BLCK_SIZE[type]);
        for (int i = 1; i < n_dims; ++i) need *= ne[i];
        need = (need + MEM_ALIGN - 1) / MEM_ALIGN * MEM_ALIGN;
    }
    ggml_object * obj = (ggml_object *) (ctx->mem_buffer + cur_end);
    if (!ctx->scratch.data || data) {
        need += sizeof(ggml_tensor);
        if (cur_end + need + GGML_OBJECT_SIZE > ctx->mem_size) {
            fprintf(stderr, "%s: not enough space in the context's memory pool (needed %zu, available %zu)\n", __func__,
                    cur_end + need + GGML_OBJECT_SIZE, ctx->mem_size);
            gabort("out of context memory");
        }
        *obj = ggml_object{cur_end + GGML_OBJECT_SIZE, need, nullptr, {0}};
    } else {
        if (ctx->scratch.offs + need > ctx->scratch.size) gabort("not enough space in the scratch memory");
        if (cur_end + sizeof(ggml_tensor) + GGML_OBJECT_SIZE > ctx->mem_size) gabort("out of context memory");
        data = (char *) ctx->scratch.data + ctx->scratch.offs;
        *obj = ggml_object{cur_end + GGML_OBJECT_SIZE, sizeof(ggml_tensor), nullptr, {0}};
        ctx->scratch.offs += need;
    }
    if (cur) cur->next = obj;
    else ctx->objects_begin = obj;
    ctx->objects_end = obj;
    ggml_tensor * t = (ggml_tensor *) (ctx->mem_buffer + obj->offs);
    std::memset(t, 0, sizeof(*t));
    t->type = type;
    t->n_dims = n_dims;
    for (int i = 0; i < GGML_MAX_DIMS; ++i) t->ne[i] = 1;
    for (int i = 0; i < n_dims; ++i) t->ne[i] = ne[i];
    t->op = GGML_OP_NONE;
    t->data = (!data && !ctx->no_alloc) ? (void *) (t + 1) : data;
    t->nb[0] = TYPE_SIZE[type];
    t->nb[1] = t->nb[0] * (t->ne[0] / BLCK_SIZE[type]);
    for (int i = 2; i < GGML_MAX_DIMS; ++i) t->nb[i] = t->nb[i - 1] * t->ne[i - 1];
    return t;
}

// a 1-element tensor outside any scratch buffer (ggml_new_i32 / ggml_new_f32 and the
// parameter tensors of rope / diag_mask_inf)
ggml_tensor * new_param_tensor(ggml_context * ctx, ggml_type type, int64_t n) {
    ctx->scratch_save = ctx->scratch;
    ctx->scratch.data = nullptr;
    ggml_tensor * t = new_tensor_impl(ctx, type, 1, &n, nullptr);
    ctx->scratch = ctx->scratch_save;
    return t;
}

// the fresh tensor r becomes the node op(a, b)
ggml_tensor * node(ggml_tensor * r, ggml_op op, ggml_tensor * a, ggml_tensor * b = nullptr) {
    r->op = op;
    r->src0 = a;
    r->src1 = b;
    return r;
}
ggml_tensor * unary_node(ggml_context * ctx, ggml_tensor * a, ggml_op op) { return node(ggml_dup_tensor(ctx, a), op, a); }
ggml_tensor * binary_node(ggml_context * ctx, ggml_tensor * a, ggml_tensor * b, ggml_op op) {
    G_ASSERT(same_shape(a, b));
    return node(ggml_dup_tensor(ctx, a), op, a, b);
}
// a node of a's type over existing bytes (reshape, view): metadata only
ggml_tensor * view_node(ggml_context * ctx, ggml_tensor * a, int n_dims, const int64_t * ne, void * data, ggml_op op) {
    return node(new_tensor_impl(ctx, a->type, n_dims, ne, data), op, a);
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// timing, fp16, sizes
// ---------------------------------------------------------------------------
static int64_t g_t0_us = 0;
void ggml_time_init(void) { g_t0_us = lvk::now_us(); }
int64_t ggml_time_ms(void) { return (lvk::now_us() - g_t0_us) / 1000; }
int64_t ggml_time_us(void) { return lvk::now_us() - g_t0_us; }
int64_t ggml_cycles(void) { return (int64_t) __rdtsc(); }
int64_t ggml_cycles_per_ms(void) {
    static int64_t c = 0;
    if (!c) {
        const int64_t t0 = lvk::now_us(), c0 = ggml_cycles();
        while (lvk::now_us() - t0 < 2000) {}
        c = (ggml_cycles() - c0) / 2;
    }
    return c;
}

float ggml_fp16_to_fp32(ggml_fp16_t x) { return h_f16_to_f32(x); }
ggml_fp16_t ggml_fp32_to_fp16(float x) { return h_f32_to_f16(x); }

int64_t ggml_nelements(const struct ggml_tensor * t) { return t->ne[0] * t->ne[1] * t->ne[2] * t->ne[3]; }
size_t ggml_nbytes(const struct ggml_tensor * t) {
    return (size_t) ggml_nelements(t) * TYPE_SIZE[t->type] / BLCK_SIZE[t->type];
}
int ggml_blck_size(enum ggml_type type) { return BLCK_SIZE[type]; }
size_t ggml_type_size(enum ggml_type type) { return TYPE_SIZE[type]; }
float ggml_type_sizef(enum ggml_type type) { return (float) TYPE_SIZE[type] / BLCK_SIZE[type]; }
size_t ggml_element_size(const struct ggml_tensor * t) { return TYPE_SIZE[t->type]; }

void ggml_print_object(const struct ggml_object * obj) {
    fprintf(stderr, " - ggml_object: offset = %zu, size = %zu, next = %p\n", obj->offs, obj->size, (void *) obj->next);
}
void ggml_print_objects(const struct ggml_context * ctx) {
    fprintf(stderr, "%s: objects in context %p:\n", __func__, (const void *) ctx);
    for (const ggml_object * o = ctx->objects_begin; o; o = o->next) ggml_print_object(o);
}

// ---------------------------------------------------------------------------
// contexts
// ---------------------------------------------------------------------------
struct ggml_context * ggml_init(struct ggml_init_params params) {
    ggml_context * c = new ggml_context;
    c->mem_size = params.mem_size;
    c->no_alloc = params.no_alloc;
    if (params.mem_buffer) {
        c->mem_buffer = (char *) params.mem_buffer;
    } else if (params.mem_size) {
        void * p = nullptr;
        if (posix_memalign(&p, MEM_ALIGN, params.mem_size) != 0) {
            delete c;
            return nullptr;
        }
        c->mem_buffer = (char *) p;
        c->mem_owned = true;
    }
    return c;
}

void ggml_free(struct ggml_context * ctx) {
    if (!ctx) return;
    if (ctx->mem_owned) free(ctx->mem_buffer);
    delete ctx;
}

size_t ggml_used_mem(const struct ggml_context * ctx) {
    return ctx->objects_end ? ctx->objects_end->offs + ctx->objects_end->size : 0;
}

size_t ggml_set_scratch(struct ggml_context * ctx, struct ggml_scratch scratch) {
    const size_t used = ctx->scratch.offs;
    ctx->scratch = scratch;
    return used;
}

// ---------------------------------------------------------------------------
// tensors
// ---------------------------------------------------------------------------
struct ggml_tensor * ggml_new_tensor(struct ggml_context * ctx, enum ggml_type type, int n_dims, const int64_t * ne) {
    return new_tensor_impl(ctx, type, n_dims, ne, nullptr);
}
struct ggml_tensor * ggml_new_tensor_1d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0) {
    return new_tensor_impl(ctx, type, 1, &ne0, nullptr);
}
struct ggml_tensor * ggml_new_tensor_2d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0, int64_t ne1) {
    const int64_t ne[2] = {ne0, ne1};
    return new_tensor_impl(ctx, type, 2, ne, nullptr);
}
struct ggml_tensor * ggml_new_tensor_3d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0, int64_t ne1,
                                        int64_t ne2) {
    const int64_t ne[3] = {ne0, ne1, ne2};
    return new_tensor_impl(ctx, type, 3, ne, nullptr);
}
struct ggml_tensor * ggml_new_tensor_4d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0, int64_t ne1,
                                        int64_t ne2, int64_t ne3) {
    const int64_t ne[4] = {ne0, ne1, ne2, ne3};
    return new_tensor_impl(ctx, type, 4, ne, nullptr);
}
struct ggml_tensor * ggml_new_i32(struct ggml_context * ctx, int32_t value) {
    ggml_tensor * t = new_param_tensor(ctx, GGML_TYPE_I32, 1);
    ggml_set_i32(t, value);
    return t;
}
struct ggml_tensor * ggml_new_f32(struct ggml_context * ctx, float value) {
    ggml_tensor * t = new_param_tensor(ctx, GGML_TYPE_F32, 1);
    ggml_set_f32(t, value);
    return t;
}
struct ggml_tensor * ggml_dup_tensor(struct ggml_context * ctx, const struct ggml_tensor * src) {
    return new_tensor_impl(ctx, src->type, src->n_dims, src->ne, nullptr);
}
struct ggml_tensor * ggml_view_tensor(struct ggml_context * ctx, const struct ggml_tensor * src) {
    ggml_tensor * t = new_tensor_impl(ctx, src->type, src->n_dims, src->ne, src->data);
    for (int i = 0; i < GGML_MAX_DIMS; ++i) t->nb[i] = src->nb[i];
    return t;
}

struct ggml_tensor * ggml_set_zero(struct ggml_tensor * t) {
    std::memset(t->data, 0, ggml_nbytes(t));
    return t;
}

int32_t ggml_get_i32_1d(const struct ggml_tensor * t, int i) {
    return get_1d<int32_t>(t, i, "ggml_get_i32_1d: quantized tensor");
}
void ggml_set_i32_1d(const struct ggml_tensor * t, int i, int32_t v) {
    set_1d(t, i, v, "ggml_set_i32_1d: quantized tensor");
}
float ggml_get_f32_1d(const struct ggml_tensor * t, int i) {
    return get_1d<float>(t, i, "ggml_get_f32_1d: quantized tensor");
}
void ggml_set_f32_1d(const struct ggml_tensor * t, int i, float v) { set_1d(t, i, v, "ggml_set_f32_1d: quantized tensor"); }
struct ggml_tensor * ggml_set_i32(struct ggml_tensor * t, int32_t v) {
    const int64_t n = ggml_nelements(t);
    for (int64_t i = 0; i < n; ++i) ggml_set_i32_1d(t, (int) i, v);
    return t;
}
struct ggml_tensor * ggml_set_f32(struct ggml_tensor * t, float v) {
    const int64_t n = ggml_nelements(t);
    for (int64_t i = 0; i < n; ++i) ggml_set_f32_1d(t, (int) i, v);
    return t;
}
void * ggml_get_data(const struct ggml_tensor * t) { return t->data; }
float * ggml_get_data_f32(const struct ggml_tensor * t) {
    G_ASSERT(t->type == GGML_TYPE_F32);
    return (float *) t->data;
}

// ---------------------------------------------------------------------------
// operators (graph nodes)
// ---------------------------------------------------------------------------
struct ggml_tensor * ggml_dup(struct ggml_context * ctx, struct ggml_tensor * a) { return unary_node(ctx, a, GGML_OP_DUP); }
struct ggml_tensor * ggml_add(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    return binary_node(ctx, a, b, GGML_OP_ADD);
}
struct ggml_tensor * ggml_sub(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    return binary_node(ctx, a, b, GGML_OP_SUB);
}
struct ggml_tensor * ggml_mul(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    return binary_node(ctx, a, b, GGML_OP_MUL);
}
struct ggml_tensor * ggml_div(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    return binary_node(ctx, a, b, GGML_OP_DIV);
}
struct ggml_tensor * ggml_repeat(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    G_ASSERT(b->ne[0] % a->ne[0] == 0 && b->ne[1] % a->ne[1] == 0 && b->ne[2] % a->ne[2] == 0 &&
             b->ne[3] % a->ne[3] == 0);
    if (same_shape(a, b) && !a->is_param) return a;
    return node(new_tensor_impl(ctx, a->type, b->n_dims, b->ne, nullptr), GGML_OP_REPEAT, a, b);
}
struct ggml_tensor * ggml_silu(struct ggml_context * ctx, struct ggml_tensor * a) { return unary_node(ctx, a, GGML_OP_SILU); }
struct ggml_tensor * ggml_rms_norm(struct ggml_context * ctx, struct ggml_tensor * a) {
    return unary_node(ctx, a, GGML_OP_RMS_NORM);
}
struct ggml_tensor * ggml_mul_mat(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    G_ASSERT(a->ne[0] == b->ne[0] && a->ne[2] == b->ne[2] && a->ne[3] == b->ne[3]);
    const int64_t ne[4] = {a->ne[1], b->ne[1], a->ne[2], b->ne[3]};
    return node(new_tensor_impl(ctx, GGML_TYPE_F32, std::min(a->n_dims, b->n_dims), ne, nullptr), GGML_OP_MUL_MAT, a, b);
}
struct ggml_tensor * ggml_scale(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    G_ASSERT(ggml_nelements(b) == 1);
    G_ASSERT(a->nb[0] == TYPE_SIZE[a->type] && a->nb[1] == a->nb[0] * a->ne[0]);   // padded 1d rows
    return node(ggml_view_tensor(ctx, a), GGML_OP_SCALE, a, b);
}
struct ggml_tensor * ggml_cpy(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    G_ASSERT(ggml_nelements(a) == ggml_nelements(b));
    return node(ggml_view_tensor(ctx, b), GGML_OP_CPY, a, b);
}
struct ggml_tensor * ggml_reshape(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    G_ASSERT(is_contiguous(a) && is_contiguous(b) && ggml_nelements(a) == ggml_nelements(b));
    return view_node(ctx, a, b->n_dims, b->ne, a->data, GGML_OP_RESHAPE);
}
struct ggml_tensor * ggml_reshape_2d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1) {
    G_ASSERT(is_contiguous(a) && ggml_nelements(a) == ne0 * ne1);
    const int64_t ne[2] = {ne0, ne1};
    return view_node(ctx, a, 2, ne, a->data, GGML_OP_RESHAPE);
}
struct ggml_tensor * ggml_reshape_3d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1,
                                     int64_t ne2) {
    G_ASSERT(is_contiguous(a) && ggml_nelements(a) == ne0 * ne1 * ne2);
    const int64_t ne[3] = {ne0, ne1, ne2};
    return view_node(ctx, a, 3, ne, a->data, GGML_OP_RESHAPE);
}
struct ggml_tensor * ggml_view_1d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, size_t offset) {
    return view_node(ctx, a, 1, &ne0, (char *) a->data + offset, GGML_OP_VIEW);
}
struct ggml_tensor * ggml_view_2d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1,
                                  size_t nb1, size_t offset) {
    const int64_t ne[2] = {ne0, ne1};
    ggml_tensor * r = view_node(ctx, a, 2, ne, (char *) a->data + offset, GGML_OP_VIEW);
    r->nb[1] = nb1;
    r->nb[2] = r->nb[1] * ne1;
    r->nb[3] = r->nb[2];
    return r;
}
struct ggml_tensor * ggml_view_3d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1,
                                  int64_t ne2, size_t nb1, size_t nb2, size_t offset) {
    const int64_t ne[3] = {ne0, ne1, ne2};
    ggml_tensor * r = view_node(ctx, a, 3, ne, (char *) a->data + offset, GGML_OP_VIEW);
    r->nb[1] = nb1;
    r->nb[2] = nb2;
    r->nb[3] = r->nb[2] * ne2;
    return r;
}
struct ggml_tensor * ggml_permute(struct ggml_context * ctx, struct ggml_tensor * a, int axis0, int axis1, int axis2,
                                  int axis3) {
    const int ax[4] = {axis0, axis1, axis2, axis3};
    for (int i = 0; i < 4; ++i) {
        G_ASSERT(ax[i] >= 0 && ax[i] < GGML_MAX_DIMS);
        for (int k = 0; k < i; ++k) G_ASSERT(ax[i] != ax[k]);
    }
    ggml_tensor * r = node(ggml_view_tensor(ctx, a), GGML_OP_PERMUTE, a);
    for (int i = 0; i < 4; ++i) {
        r->ne[ax[i]] = a->ne[i];
        r->nb[ax[i]] = a->nb[i];
    }
    return r;
}
struct ggml_tensor * ggml_transpose(struct ggml_context * ctx, struct ggml_tensor * a) {
    ggml_tensor * r = node(ggml_view_tensor(ctx, a), GGML_OP_TRANSPOSE, a);
    std::swap(r->ne[0], r->ne[1]);
    std::swap(r->nb[0], r->nb[1]);
    return r;
}
struct ggml_tensor * ggml_get_rows(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b) {
    G_ASSERT(a->ne[2] == 1 && a->ne[3] == 1 && b->ne[1] == 1 && b->ne[2] == 1 && b->ne[3] == 1 &&
             b->type == GGML_TYPE_I32);
    return node(ggml_new_tensor_2d(ctx, GGML_TYPE_F32, a->ne[0], b->ne[0]), GGML_OP_GET_ROWS, a, b);
}
// diag_mask_inf and rope: the view is created before the parameter tensor, as in ggml.c
struct ggml_tensor * ggml_diag_mask_inf(struct ggml_context * ctx, struct ggml_tensor * a, int n_past) {
    ggml_tensor * r = ggml_view_tensor(ctx, a);
    ggml_tensor * b = new_param_tensor(ctx, GGML_TYPE_I32, 1);
    ((int32_t *) b->data)[0] = n_past;
    return node(r, GGML_OP_DIAG_MASK_INF, a, b);
}
struct ggml_tensor * ggml_soft_max(struct ggml_context * ctx, struct ggml_tensor * a) {
    return node(ggml_view_tensor(ctx, a), GGML_OP_SOFT_MAX, a);
}
struct ggml_tensor * ggml_rope(struct ggml_context * ctx, struct ggml_tensor * a, int n_past, int n_dims, int mode) {
    G_ASSERT(n_past >= 0);
    ggml_tensor * r = ggml_view_tensor(ctx, a);
    ggml_tensor * b = new_param_tensor(ctx, GGML_TYPE_I32, 3);
    ((int32_t *) b->data)[0] = n_past;
    ((int32_t *) b->data)[1] = n_dims;
    ((int32_t *) b->data)[2] = mode;
    return node(r, GGML_OP_ROPE, a, b);
}

void ggml_set_param(struct ggml_context * ctx, struct ggml_tensor * tensor) {
    tensor->is_param = true;
    G_ASSERT(tensor->grad == nullptr);
    tensor->grad = ggml_dup_tensor(ctx, tensor);
}

// ---------------------------------------------------------------------------
// graphs: depth-first over src0, src1, opt[], leaves before their users (ggml.c
// ggml_visit_parents / ggml_build_forward_impl)
// ---------------------------------------------------------------------------
static void visit_parents(ggml_cgraph * g, ggml_tensor * node) {
    for (int i = 0; i < g->n_nodes; ++i)
        if (g->nodes[i] == node) return;
    for (int i = 0; i < g->n_leafs; ++i)
        if (g->leafs[i] == node) return;
    if (node->src0) visit_parents(g, node->src0);
    if (node->src1) visit_parents(g, node->src1);
    for (int i = 0; i < GGML_MAX_OPT; ++i)
        if (node->opt[i]) visit_parents(g, node->opt[i]);
    if (node->op == GGML_OP_NONE && node->grad == nullptr) {
        G_ASSERT(g->n_leafs < GGML_MAX_NODES);
        g->leafs[g->n_leafs++] = node;
    } else {
        G_ASSERT(g->n_nodes < GGML_MAX_NODES);
        g->nodes[g->n_nodes] = node;
        g->grads[g->n_nodes] = node->grad;
        g->n_nodes++;
    }
}

void ggml_build_forward_expand(struct ggml_cgraph * cgraph, struct ggml_tensor * tensor) {
    const int n0 = cgraph->n_nodes;
    visit_parents(cgraph, tensor);
    if (cgraph->n_nodes > n0) G_ASSERT(cgraph->nodes[cgraph->n_nodes - 1] == tensor);
}

struct ggml_cgraph ggml_build_forward(struct ggml_tensor * tensor) {
    ggml_cgraph g;
    std::memset(&g, 0, sizeof(g));
    ggml_build_forward_expand(&g, tensor);
    return g;
}

void ggml_graph_reset(struct ggml_cgraph * cgraph) {
    for (int i = 0; i < cgraph->n_nodes; ++i)
        if (cgraph->grads[i]) ggml_set_zero(cgraph->grads[i]);
}

void ggml_graph_print(const struct ggml_cgraph * cgraph) {
    fprintf(stderr, "=== GRAPH ===\nn_nodes = %d\n", cgraph->n_nodes);
    for (int i = 0; i < cgraph->n_nodes; ++i) {
        const ggml_tensor * n = cgraph->nodes[i];
        fprintf(stderr, " - %3d: [ %" PRId64 ", %" PRId64 ", %" PRId64 "] op %d\n", i, n->ne[0], n->ne[1], n->ne[2], (int) n->op);
    }
    fprintf(stderr, "n_leafs = %d\n", cgraph->n_leafs);
    for (int i = 0; i < cgraph->n_leafs; ++i) {
        const ggml_tensor * n = cgraph->leafs[i];
        fprintf(stderr, " - %3d: [ %" PRId64 ", %" PRId64 "]\n", i, n->ne[0], n->ne[1]);
    }
    fprintf(stderr, "========================================\n");
}

int ggml_cpu_has_avx(void) { return __builtin_cpu_supports("avx") ? 1 : 0; }
int ggml_cpu_has_avx2(void) { return __builtin_cpu_supports("avx2") ? 1 : 0; }
int ggml_cpu_has_avx512(void) { return __builtin_cpu_supports("avx512f") ? 1 : 0; }
int ggml_cpu_has_fma(void) { return __builtin_cpu_supports("fma") ? 1 : 0; }
int ggml_cpu_has_neon(void) { return 0; }
int ggml_cpu_has_arm_fma(void) { return 0; }
int ggml_cpu_has_f16c(void) { return 1; }
int ggml_cpu_has_fp16_va(void) { return 0; }
int ggml_cpu_has_wasm_simd(void) { return 0; }
int ggml_cpu_has_blas(void) { return 0; }
int ggml_cpu_has_sse3(void) { return __builtin_cpu_supports("sse3") ? 1 : 0; }
int ggml_cpu_has_vsx(void) { return 0; }

}  // extern "C"
