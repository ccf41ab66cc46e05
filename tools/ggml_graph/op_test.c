/* op_test.c -- one case per edge of every ggml graph operator this library runs on the GPU
 * (dup, cpy, add, sub, mul, div, repeat, silu, scale, diag_mask_inf, rms_norm, soft_max,
 * rope, get_rows, mul_mat), through the public ggml.h API only.
 *
 * The same source is compiled twice (tools/ggml_graph/Makefile): against include/ggml.h +
 * libllama_vk_amd.so (every node on the GPU) and against the reference ggml.c (oracle/_ref,
 * its CPU AVX2 build, -DNDEBUG).  tests/test_ggml_ops.py and tests/test_gpu_ggml_ops.py
 * compare the two builds case by case.
 *
 * usage: op_test <dump.bin>    run every case, write one record per case
 *        op_test --list        print the case names
 *        OP_TEST_BUILD_ONLY=1 op_test
 *                              build every case's graph and print its result tensor (op, type,
 *                              ne, nb, whether its data is its sources' data, ggml_used_mem);
 *                              nothing is computed
 *
 * Every case fills its inputs from a xorshift generator seeded from the case's name (plus a
 * per-case salt), so both builds see identical bytes.  A record is
 *     u32 name length, name, u32 n_in, u32 n_out, then n_in + n_out tensors, each
 *     i32 type, i64 ne[4], the elements in logical order (i0 fastest) read through nb[]
 * (a Q4 tensor: its rows' blocks as stored).  An input is the operand as the operator gets it
 * (the transposed or strided view, not its parent).  Inputs are written before the graph runs --
 * scale, diag_mask_inf, soft_max and rope write into their source.
 *
 * The reference is built with -DNDEBUG, so its asserts are off and some of its loops only
 * address certain layouts; each group of cases below names the reference loop and the
 * layouts it handles, and no case leaves them.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ggml.h"

#define F32 GGML_TYPE_F32
#define F16 GGML_TYPE_F16

enum { MAX_IN = 4, MAX_OUT = 2, MAX_ARG = 8 };

struct rec {
    struct ggml_context * ctx;
    struct ggml_tensor * in[MAX_IN];
    int n_in;
    struct ggml_tensor * res;          /* the node the graph is built for */
    struct ggml_tensor * out[MAX_OUT]; /* dumped after the run; default: res */
    int n_out;
};

/* ---- the generator ---------------------------------------------------------------- */
static uint32_t rng = 1u;
static uint32_t next_u32(void) {
    rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5;
    return rng;
}
static void seed_case(const char * name, int salt) {
    uint32_t h = 2166136261u;
    for (const char * p = name; *p; ++p) { h ^= (uint8_t) *p; h *= 16777619u; }
    h ^= (uint32_t) salt * 0x9E3779B9u;
    rng = h ? h : 1u;
    for (int i = 0; i < 8; ++i) next_u32();
}
static float uni(float lo, float hi) { return lo + (hi - lo) * (float) (next_u32() >> 8) / 16777216.0f; }
/* mixed sign and magnitude: +-[1, 2) * 2^[-6, 6) */
static float mixed(void) {
    const uint32_t r = next_u32();
    const int e = (int) ((r >> 8) % 12u) - 6;
    const float v = ldexpf(1.0f + (float) (next_u32() >> 9) / 8388608.0f, e);
    return (r & 1u) ? -v : v;
}

/* ---- tensors ---------------------------------------------------------------------- */
/* n_dims: up to the last extent above 1, at least nd_min (a [K, 1] matrix stays 2-D) */
static struct ggml_tensor * newtn(struct rec * r, enum ggml_type type, int nd_min, int64_t ne0, int64_t ne1,
                                  int64_t ne2, int64_t ne3) {
    const int64_t ne[4] = {ne0, ne1, ne2, ne3};
    int nd = nd_min;
    for (int d = 1; d < 4; ++d)
        if (ne[d] > 1) nd = d + 1;
    struct ggml_tensor * t = ggml_new_tensor(r->ctx, type, nd, ne);
    memset(t->data, 0, ggml_nbytes(t));
    return t;
}
static struct ggml_tensor * newt(struct rec * r, enum ggml_type type, int64_t ne0, int64_t ne1, int64_t ne2,
                                 int64_t ne3) {
    return newtn(r, type, 1, ne0, ne1, ne2, ne3);
}
/* element i of a contiguous f32 / f16 tensor */
static void set_el(struct ggml_tensor * t, int64_t i, float v) {
    if (t->type == F16) ((ggml_fp16_t *) t->data)[i] = ggml_fp32_to_fp16(v);
    else ((float *) t->data)[i] = v;
}
static void fill_uni(struct ggml_tensor * t, float lo, float hi) {
    for (int64_t i = 0; i < ggml_nelements(t); ++i) set_el(t, i, uni(lo, hi));
}
static void fill_mixed(struct ggml_tensor * t) {
    for (int64_t i = 0; i < ggml_nelements(t); ++i) set_el(t, i, mixed());
}
static void fill_list(struct ggml_tensor * t, const float * v, int n) {
    for (int i = 0; i < n; ++i) set_el(t, i, v[i]);
}
/* a Q4_0 / Q4_1 tensor quantized from mixed values by the file quantizers both builds export */
static struct ggml_tensor * new_q4(struct rec * r, enum ggml_type type, int64_t K, int64_t M, int64_t ne2) {
    struct ggml_tensor * t = newtn(r, type, 2, K, M, ne2, 1);
    const int n = (int) (K * M * ne2);
    float * f = (float *) malloc(sizeof(float) * (size_t) n);
    int64_t hist[16] = {0};
    for (int i = 0; i < n; ++i) f[i] = mixed() * 0.25f;
    if (type == GGML_TYPE_Q4_0) ggml_quantize_q4_0(f, t->data, n, (int) K, hist);
    else ggml_quantize_q4_1(f, t->data, n, (int) K, hist);
    free(f);
    return t;
}
static void add_in(struct rec * r, struct ggml_tensor * t) { r->in[r->n_in++] = t; }
static void add_out(struct rec * r, struct ggml_tensor * t) { r->out[r->n_out++] = t; }

/* ---- dup / cpy ---------------------------------------------------------------------
 * ggml_compute_forward_dup_f32 (ggml.c:4918-5010) walks the source through its strides and
 * the destination through its own, with destination counters that wrap at the destination's
 * extents (4965-4976, 4991-5002): any layout and any reshape is handled.
 * ggml_compute_forward_dup_f16 (4804-4916) wraps its destination counters at the SOURCE's
 * extents (4871-4881, 4897-4907): right only when both shapes are equal, so every f16-source
 * case here keeps the shape (a reshaping f16-source copy leaves holes or writes outside the
 * destination in the reference and is left out).  Same type, same ne0 and unit nb0 on both
 * sides copies by rows (4835-4851); both contiguous is one memcpy (4830-4833). */
static const float f16_edges[] = {
    65504.0f, 65519.99f, 65520.0f, 65536.0f, 1e-8f, 6.1e-5f, 5.96e-8f, 0.0f, -0.0f, INFINITY, -INFINITY,
    1.0f + 0x1p-11f, 1.0f + 3 * 0x1p-11f, -(1.0f + 0x1p-11f), -(1.0f + 3 * 0x1p-11f), -65519.99f, -65520.0f,
    0x1p-24f, 0x1p-25f, 0x1.000002p-25f, 3 * 0x1p-25f, -0x1p-25f, 0x1p-14f, 0x1.ffcp-15f, 0x1.ffep-15f, 1e-39f,
    -1e-39f, 1e-45f, 3.4e38f, 0.1f, 1.0f / 3.0f, 2049.0f, 2051.0f, 1e-7f, -1e-7f};
#define N_F16_EDGES ((int) (sizeof(f16_edges) / sizeof(f16_edges[0])))

static void c_cpy_f32_f16_edges(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 70, 3, 1, 1);
    fill_mixed(s);
    fill_list(s, f16_edges, N_F16_EDGES);
    add_in(r, s);
    r->res = ggml_cpy(r->ctx, s, newt(r, F16, 70, 3, 1, 1));
}
/* a[0]: source type, a[1]: destination type; source transpose([7,5]) -> contiguous [5,7] */
static void c_cpy_transposed(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, (enum ggml_type) a[0], 7, 5, 1, 1);
    fill_mixed(s);
    s = ggml_transpose(r->ctx, s);
    add_in(r, s);
    r->res = ggml_cpy(r->ctx, s, newt(r, (enum ggml_type) a[1], 5, 7, 1, 1));
}
static void c_cpy_f32_permute_reshape(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 4, 3, 5, 1);
    fill_mixed(s);
    s = ggml_permute(r->ctx, s, 0, 2, 1, 3);
    add_in(r, s);
    r->res = ggml_cpy(r->ctx, s, newt(r, F32, 12, 5, 1, 1));
}
static void c_cpy_f32_4d(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 3, 2, 4, 2);
    fill_mixed(s);
    s = ggml_permute(r->ctx, s, 1, 0, 3, 2);
    add_in(r, s);
    r->res = ggml_cpy(r->ctx, s, newt(r, F16, 2, 3, 2, 4));
}
/* the V-cache layout: 3 columns of 8 rows 16 elements apart, at element 5 of an f16 cache.
 * a[0]: source type (f32: a transposed [8,3], as llama.cpp's Vcur; f16: contiguous [3,8],
 * the by-rows path).  The whole cache is dumped too: the gaps keep their bytes. */
static void c_cpy_into_vcache(struct rec * r, const int * a) {
    struct ggml_tensor * cache = newt(r, F16, 128, 1, 1, 1);
    fill_uni(cache, 100.0f, 200.0f);
    struct ggml_tensor * s;
    if (a[0] == F32) {
        s = newt(r, F32, 8, 3, 1, 1);
        fill_mixed(s);
        s = ggml_transpose(r->ctx, s);
        add_in(r, s);
    } else {
        s = newt(r, F16, 3, 8, 1, 1);
        fill_mixed(s);
        add_in(r, s);
    }
    add_in(r, cache);
    r->res = ggml_cpy(r->ctx, s, ggml_view_2d(r->ctx, cache, 3, 8, 16 * sizeof(ggml_fp16_t), 5 * sizeof(ggml_fp16_t)));
    add_out(r, r->res);
    add_out(r, cache);
}
/* f16 rows 16 apart -> contiguous f16 (by rows, strided source) */
static void c_cpy_from_vcache(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * cache = newt(r, F16, 128, 1, 1, 1);
    fill_mixed(cache);
    struct ggml_tensor * s = ggml_view_2d(r->ctx, cache, 3, 8, 16 * sizeof(ggml_fp16_t), 5 * sizeof(ggml_fp16_t));
    add_in(r, s);
    r->res = ggml_cpy(r->ctx, s, newt(r, F16, 3, 8, 1, 1));
}
static void c_cpy_f16_contig(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F16, 70, 3, 1, 1);
    fill_mixed(s);
    fill_list(s, f16_edges, N_F16_EDGES);
    add_in(r, s);
    r->res = ggml_cpy(r->ctx, s, newt(r, (enum ggml_type) a[0], 70, 3, 1, 1));
}
/* a[0]: type, a[1]: 1 = dup of the transpose */
static void c_dup(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, (enum ggml_type) a[0], 7, 5, 1, 1);
    fill_mixed(s);
    if (a[1]) s = ggml_transpose(r->ctx, s);
    add_in(r, s);
    r->res = ggml_dup(r->ctx, s);
}

/* ---- add / sub / mul / div ---------------------------------------------------------
 * ggml_compute_forward_{sub,mul,div}_f32 (ggml.c:5117-5142, 5169-5194, 5221-5246) and add's
 * contiguous-src1 branch (5068-5077) step row j of all three tensors by j * nb[1] alone over
 * ggml_nrows rows: right for 2-D tensors of any row stride and for contiguous 3-D ones
 * (nb[2] == nb[1] * ne[1]).  add with nb10 != 4 (5078-5088) also steps rows by nb11 alone:
 * a 2-D transposed src1.  The result is a new contiguous tensor. */
static struct ggml_tensor * binary(struct rec * r, int op, struct ggml_tensor * x, struct ggml_tensor * y) {
    switch (op) {
        case 0: return ggml_add(r->ctx, x, y);
        case 1: return ggml_sub(r->ctx, x, y);
        case 2: return ggml_mul(r->ctx, x, y);
        default: return ggml_div(r->ctx, x, y);
    }
}
static void c_bin_contig(struct rec * r, const int * a) {
    struct ggml_tensor * x = newt(r, F32, 33, 5, 2, 1);
    struct ggml_tensor * y = newt(r, F32, 33, 5, 2, 1);
    fill_mixed(x);
    fill_mixed(y);
    add_in(r, x);
    add_in(r, y);
    r->res = binary(r, a[0], x, y);
}
/* a[1]: which operand is rows 33 of a [40,5] tensor, from column 3 */
static void c_bin_view(struct rec * r, const int * a) {
    struct ggml_tensor * w = newt(r, F32, 40, 5, 1, 1);
    struct ggml_tensor * c = newt(r, F32, 33, 5, 1, 1);
    fill_mixed(w);
    fill_mixed(c);
    struct ggml_tensor * v = ggml_view_2d(r->ctx, w, 33, 5, 40 * sizeof(float), 3 * sizeof(float));
    struct ggml_tensor * x = a[1] == 0 ? v : c;
    struct ggml_tensor * y = a[1] == 0 ? c : v;
    add_in(r, x);
    add_in(r, y);
    r->res = binary(r, a[0], x, y);
}
static void c_add_src1_transposed(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * x = newt(r, F32, 5, 7, 1, 1);
    struct ggml_tensor * y = newt(r, F32, 7, 5, 1, 1);
    fill_mixed(x);
    fill_mixed(y);
    y = ggml_transpose(r->ctx, y);
    add_in(r, x);
    add_in(r, y);
    r->res = ggml_add(r->ctx, x, y);
}
/* denormal operands and results (1e-39 + 1e-39, 1e-20 * 1e-20, 1e-30 / 1e10), x / 0, 0 / 0,
 * inf - inf, inf * 0, overflow, signed zeros: all four operators over the same pairs */
static void c_bin_special(struct rec * r, const int * a) {
    static const float xs[] = {1e-39f, 1e-20f,   1e-30f, 1.0f,  -1.0f, 0.0f,  INFINITY, -0.0f, 1e38f, 3e38f,
                               1e-38f, 1.5e-45f, 5.0f,   -7.0f, 1e-39f, 16777216.0f, INFINITY, -0.0f, 2e-38f, 3e-39f};
    static const float ys[] = {1e-39f, 1e-20f, 1e10f, 0.0f, 0.0f,   0.0f, INFINITY,  0.0f,  1e38f, -3e38f,
                               0.5f,   2.0f,   0.1f,  3.0f, -1e-39f, 1.0f, -INFINITY, -0.0f, 1.5e-38f, 7.0f};
    const int n = (int) (sizeof(xs) / sizeof(xs[0]));
    struct ggml_tensor * x = newt(r, F32, n, 1, 1, 1);
    struct ggml_tensor * y = newt(r, F32, n, 1, 1, 1);
    fill_list(x, xs, n);
    fill_list(y, ys, n);
    add_in(r, x);
    add_in(r, y);
    r->res = binary(r, a[0], x, y);
}

/* ---- repeat -------------------------------------------------------------------------
 * ggml_compute_forward_repeat_f32 (ggml.c:5504-5542) is 2-D (ne2 == ne3 == 1 on both sides)
 * with unit nb0; it tiles src0's nr0 rows of nc0 values over the destination. */
static void c_repeat(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F32, a[0], a[1], 1, 1);
    fill_mixed(s);
    add_in(r, s);
    const int64_t ne[2] = {a[2], a[3]};
    struct ggml_tensor * shape = ggml_new_tensor(r->ctx, F32, 2, ne);
    memset(shape->data, 0, ggml_nbytes(shape));
    r->res = ggml_repeat(r->ctx, s, shape);
}

/* ---- silu, scale --------------------------------------------------------------------
 * ggml_compute_forward_silu_f32 (ggml.c:5875-5914) and ggml_compute_forward_scale_f32
 * (6757-6790) want contiguous tensors (GGML_ASSERT, live under NDEBUG) and step rows by
 * nb[1] over ggml_nrows rows.  scale writes into its source. */
static void c_silu_sweep(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 300, 1, 1, 1);
    for (int i = 0; i < 300; ++i) set_el(s, i, -20.0f + 40.0f * (float) i / 299.0f);
    add_in(r, s);
    r->res = ggml_silu(r->ctx, s);
}
static void c_silu_special(struct rec * r, const int * a) {
    (void) a;
    static const float v[] = {70000.0f, -70000.0f, 65504.0f, 65520.0f, 1e-8f, -0.0f, 0.0f, -65504.0f,
                              -65520.0f, 1e-39f, 88.0f, -88.0f, 11.09f, -11.09f, 6.1e-5f, -17.5f};
    const int n = (int) (sizeof(v) / sizeof(v[0]));
    struct ggml_tensor * s = newt(r, F32, n / 2, 2, 1, 1);
    fill_list(s, v, n);
    add_in(r, s);
    r->res = ggml_silu(r->ctx, s);
}
static void c_silu_3d(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 33, 3, 2, 1);
    fill_uni(s, -8.0f, 8.0f);
    add_in(r, s);
    r->res = ggml_silu(r->ctx, s);
}
/* a[0..2]: shape, a[3]: 0 = 1/sqrt(128) on mixed values, 1 = 1e-10 on values near 1e-30 */
static void c_scale(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F32, a[0], a[1], a[2], 1);
    if (a[3]) fill_uni(s, -2e-30f, 2e-30f);
    else fill_mixed(s);
    struct ggml_tensor * f = ggml_new_f32(r->ctx, a[3] ? 1e-10f : 1.0f / sqrtf(128.0f));
    add_in(r, s);
    add_in(r, f);
    r->res = ggml_scale(r->ctx, s, f);
}

/* ---- diag_mask_inf -------------------------------------------------------------------
 * ggml_compute_forward_diag_mask_inf_f32 (ggml.c:7001-7035) steps planes by nb[2] alone over
 * nrows / ne1 planes: contiguous tensors of up to 3 dims.  It writes -inf into its source. */
static void c_diag_mask(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F32, a[0], a[1], a[2], 1);
    fill_mixed(s);
    r->res = ggml_diag_mask_inf(r->ctx, s, a[3]);
    add_in(r, s);
    add_in(r, r->res->src1);
}

/* ---- rms_norm ------------------------------------------------------------------------
 * ggml_compute_forward_rms_norm_f32 (ggml.c:6024-6080) addresses rows through nb[1..3] of
 * source and destination: any row layout with unit nb0.  The result is a new contiguous
 * tensor.  a[3]: 0 plain, 1 row 1 all zero, 2 terms near 1e4 among terms near 1e-3 (the
 * index-order double sum differs from a float one) */
static void fill_rms(struct ggml_tensor * s, int kind) {
    const int64_t ne0 = s->ne[0];
    for (int64_t i = 0; i < ggml_nelements(s); ++i) {
        float v = uni(-2.0f, 2.0f);
        if (kind == 1 && i / ne0 == 1) v = 0.0f;
        if (kind == 2) v = (next_u32() % 3u == 0u) ? uni(0.5e4f, 1.5e4f) : uni(-2e-3f, 2e-3f);
        set_el(s, i, v);
    }
}
static void c_rms_norm(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F32, a[0], a[1], a[2], 1);
    fill_rms(s, a[3]);
    add_in(r, s);
    r->res = ggml_rms_norm(r->ctx, s);
}
static void c_rms_norm_view(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * w = newt(r, F32, 40, 3, 1, 1);
    fill_rms(w, 0);
    struct ggml_tensor * v = ggml_view_2d(r->ctx, w, 33, 3, 40 * sizeof(float), 5 * sizeof(float));
    add_in(r, v);
    r->res = ggml_rms_norm(r->ctx, v);
}

/* ---- soft_max ------------------------------------------------------------------------
 * ggml_compute_forward_soft_max_f32 (ggml.c:7062-7130) wants contiguous tensors (GGML_ASSERT)
 * and steps rows by nb[1]; it works in place on its source.  A row of only -inf is left out:
 * the reference divides by a zero sum there (its assert is off). */
static void c_soft_max_len(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F32, a[0], 2, 1, 1);
    fill_uni(s, -6.0f, 6.0f);
    add_in(r, s);
    r->res = ggml_soft_max(r->ctx, s);
}
static void c_soft_max_masked(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 9, 4, 3, 1);
    fill_uni(s, -6.0f, 6.0f);
    add_in(r, s);
    r->res = ggml_soft_max(r->ctx, ggml_diag_mask_inf(r->ctx, s, 5));
}
static void c_soft_max_wide(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * s = newt(r, F32, 201, 2, 1, 1);
    for (int i = 0; i < 201; ++i) {
        set_el(s, i, -100.0f + (float) i);
        set_el(s, 201 + i, 100.0f - (float) ((i * 67) % 201) + uni(0.0f, 0.5f));
    }
    add_in(r, s);
    r->res = ggml_soft_max(r->ctx, s);
}
/* p - max below -65504 (fp16 -inf, exp 0), at the fp16 overflow boundary, and a literal -inf */
static void c_soft_max_underflow(struct rec * r, const int * a) {
    (void) a;
    static const float v[] = {0.0f,  -70000.0f, -65504.0f, -65520.0f, -1e5f,    -3.0f,    -1e30f,    -11.0f, -65519.0f,
                              1e5f,  0.0f,      5e4f,      99999.0f,  34464.0f, 34496.0f, -INFINITY, 34480.0f, 99990.0f};
    struct ggml_tensor * s = newt(r, F32, 9, 2, 1, 1);
    fill_list(s, v, 18);
    add_in(r, s);
    r->res = ggml_soft_max(r->ctx, s);
}

/* ---- rope ----------------------------------------------------------------------------
 * ggml_compute_forward_rope_f32 (ggml.c:7156-7227) addresses source and destination (a view
 * of the source) through the source's nb[1..3], unit nb0; pairs below n_dims only; mode != 0
 * starts at slice n_past with p = i2.  a: ne0..ne3, n_past, n_dims, mode */
static void c_rope(struct rec * r, const int * a) {
    struct ggml_tensor * s = newt(r, F32, a[0], a[1], a[2], a[3]);
    fill_uni(s, -2.0f, 2.0f);
    r->res = ggml_rope(r->ctx, s, a[4], a[5], a[6]);
    add_in(r, s);
    add_in(r, r->res->src1);
}
/* rows 8 of a [10,3,4] tensor from column 1; the whole tensor is dumped too */
static void c_rope_view(struct rec * r, const int * a) {
    (void) a;
    struct ggml_tensor * w = newt(r, F32, 10, 3, 4, 1);
    fill_uni(w, -2.0f, 2.0f);
    struct ggml_tensor * v = ggml_view_3d(r->ctx, w, 8, 3, 4, 10 * sizeof(float), 30 * sizeof(float), sizeof(float));
    r->res = ggml_rope(r->ctx, v, 3, 8, 0);
    add_in(r, w);
    add_in(r, r->res->src1);
    add_out(r, r->res);
    add_out(r, w);
}

/* ---- get_rows ------------------------------------------------------------------------
 * ggml_compute_forward_get_rows_{q,f16,f32} (ggml.c:6868-6950): row ids[i] of a 2-D src0
 * (by nb[1]) to row i of a new contiguous f32 tensor.  a: type, K, rows, id set */
static void c_get_rows(struct rec * r, const int * a) {
    static const int32_t ids4[] = {9, 0, 0, 3};
    static const int32_t ids1[] = {4};
    const enum ggml_type type = (enum ggml_type) a[0];
    struct ggml_tensor * s;
    if (type == GGML_TYPE_Q4_0 || type == GGML_TYPE_Q4_1) {
        s = new_q4(r, type, a[1], a[2], 1);
    } else {
        s = newt(r, type, a[1], a[2], 1, 1);
        fill_mixed(s);
    }
    const int n = a[3] ? 1 : 4;
    struct ggml_tensor * ids = ggml_new_tensor_1d(r->ctx, GGML_TYPE_I32, n);
    memcpy(ids->data, a[3] ? ids1 : ids4, sizeof(int32_t) * (size_t) n);
    add_in(r, s);
    add_in(r, ids);
    r->res = ggml_get_rows(r->ctx, s, ids);
}

/* ---- mul_mat f16 x f32, f32 x f32 ----------------------------------------------------
 * ggml_compute_forward_mul_mat_f32 (ggml.c:6134-6297) reads src0 rows through nb01..nb03 and
 * src1 rows through nb11..nb13 (unit nb00 / nb10) and writes through the destination's
 * strides; ggml_compute_forward_mul_mat_f16_f32 (6299-6487) first converts src1 through all
 * four of its strides to contiguous f16 rows (6412-6428), then reads src0 rows through
 * nb01..nb03.  The destination is a new contiguous tensor.  ggml_vec_dot_f32 (1713-1748)
 * sums its n & ~31 part in 4 x 8 lanes and the tail in float, ggml_vec_dot_f16 (1781-1815)
 * the tail in double.  a: type, K, M, N, ne2, ne3, salt */
static void c_mm(struct rec * r, const int * a) {
    struct ggml_tensor * x = newtn(r, (enum ggml_type) a[0], 2, a[1], a[2], a[4], a[5]);
    struct ggml_tensor * y = newtn(r, F32, 2, a[1], a[3], a[4], a[5]);
    fill_mixed(x);
    fill_mixed(y);
    add_in(r, x);
    add_in(r, y);
    r->res = ggml_mul_mat(r->ctx, x, y);
}
/* src0: 37 of 48 cached positions, [37, 4, 2] with rows 48 apart (llama.cpp's V view) */
static void c_mm_vcache(struct rec * r, const int * a) {
    const enum ggml_type type = (enum ggml_type) a[0];
    const size_t es = type == F16 ? sizeof(ggml_fp16_t) : sizeof(float);
    struct ggml_tensor * cache = newt(r, type, 48 * 4 * 2, 1, 1, 1);
    fill_mixed(cache);
    struct ggml_tensor * x = ggml_view_3d(r->ctx, cache, 37, 4, 2, 48 * es, 48 * es * 4, 0);
    struct ggml_tensor * y = newt(r, F32, 37, 3, 2, 1);
    fill_mixed(y);
    add_in(r, x);
    add_in(r, y);
    r->res = ggml_mul_mat(r->ctx, x, y);
}
/* src1: a [40, 2, 3] tensor permuted to [40, 3, 2] (rows of a plane 2 rows apart) */
static void c_mm_src1_permuted(struct rec * r, const int * a) {
    struct ggml_tensor * x = newt(r, (enum ggml_type) a[0], 40, 5, 2, 1);
    struct ggml_tensor * y = newt(r, F32, 40, 2, 3, 1);
    fill_mixed(x);
    fill_mixed(y);
    y = ggml_permute(r->ctx, y, 0, 2, 1, 3);
    add_in(r, x);
    add_in(r, y);
    r->res = ggml_mul_mat(r->ctx, x, y);
}

/* ---- mul_mat Q4_0 / Q4_1 x f32 -------------------------------------------------------
 * ggml_compute_forward_mul_mat_q_f32 (ggml.c:6510-6696): src1 rows quantized through
 * nb11..nb13, src0 rows read through nb01..nb03, a new contiguous destination.
 * a: type, M, K, N, ne2 */
static void c_mmq(struct rec * r, const int * a) {
    struct ggml_tensor * x = new_q4(r, (enum ggml_type) a[0], a[2], a[1], a[4]);
    struct ggml_tensor * y = newtn(r, F32, 2, a[2], a[3], a[4], 1);
    fill_mixed(y);
    add_in(r, x);
    add_in(r, y);
    r->res = ggml_mul_mat(r->ctx, x, y);
}

/* ---- the table ---------------------------------------------------------------------- */
struct op_case {
    const char * name;
    void (*build)(struct rec *, const int *);
    int a[MAX_ARG];
    int salt;
};

enum { ADD = 0, SUB, MUL, DIV };
#define Q40 GGML_TYPE_Q4_0
#define Q41 GGML_TYPE_Q4_1

/* K in {1, 31, 32, 33, 64, 95, 128} x M in {1, 5} x N in {1, 3}; the salts of the
 * single-column cases were chosen so that a left-to-right float sum differs from the
 * reference's order (tests/test_ggml_ops.py) */
#define MM_K(T, t, K, s11, s13, s51, s53)                       \
    {"mm_" t "_k" #K "_m1_n1", c_mm, {T, K, 1, 1, 1, 1}, s11},  \
    {"mm_" t "_k" #K "_m1_n3", c_mm, {T, K, 1, 3, 1, 1}, s13},  \
    {"mm_" t "_k" #K "_m5_n1", c_mm, {T, K, 5, 1, 1, 1}, s51},  \
    {"mm_" t "_k" #K "_m5_n3", c_mm, {T, K, 5, 3, 1, 1}, s53}
#define MMQ(T, t)                                                  \
    {"mmq_" t "_m8_k256_n1", c_mmq, {T, 8, 256, 1, 1}, 0},         \
    {"mmq_" t "_m8_k256_n2", c_mmq, {T, 8, 256, 2, 1}, 0},         \
    {"mmq_" t "_m8_k256_n9", c_mmq, {T, 8, 256, 9, 1}, 0},         \
    {"mmq_" t "_m16_k512_n33", c_mmq, {T, 16, 512, 33, 1}, 0},     \
    {"mmq_" t "_m16_k512_n70", c_mmq, {T, 16, 512, 70, 1}, 0},     \
    {"mmq_" t "_m8_k256_n3_batched", c_mmq, {T, 8, 256, 3, 2}, 0}

static const struct op_case cases[] = {
    {"cpy_f32_f16_edges", c_cpy_f32_f16_edges, {0}, 0},
    {"cpy_f32_f32_transposed", c_cpy_transposed, {F32, F32}, 0},
    {"cpy_f32_f16_transposed", c_cpy_transposed, {F32, F16}, 0},
    {"cpy_f16_f32_transposed", c_cpy_transposed, {F16, F32}, 0},
    {"cpy_f16_f16_transposed", c_cpy_transposed, {F16, F16}, 0},
    {"cpy_f32_permute_reshape", c_cpy_f32_permute_reshape, {0}, 0},
    {"cpy_f32_f16_4d_permuted", c_cpy_f32_4d, {0}, 0},
    {"cpy_f32_f16_into_vcache", c_cpy_into_vcache, {F32}, 0},
    {"cpy_f16_f16_into_vcache", c_cpy_into_vcache, {F16}, 0},
    {"cpy_f16_f16_from_vcache", c_cpy_from_vcache, {0}, 0},
    {"cpy_f16_f16_contig", c_cpy_f16_contig, {F16}, 0},
    {"cpy_f16_f32_contig", c_cpy_f16_contig, {F32}, 0},
    {"dup_f32_transposed", c_dup, {F32, 1}, 0},
    {"dup_f16_contig", c_dup, {F16, 0}, 0},
    {"dup_f16_transposed", c_dup, {F16, 1}, 0},
    {"dup_f32_contig", c_dup, {F32, 0}, 0},

    {"add_contig", c_bin_contig, {ADD}, 0},
    {"sub_contig", c_bin_contig, {SUB}, 0},
    {"mul_contig", c_bin_contig, {MUL}, 0},
    {"div_contig", c_bin_contig, {DIV}, 0},
    {"add_view_src0", c_bin_view, {ADD, 0}, 0},
    {"sub_view_src1", c_bin_view, {SUB, 1}, 0},
    {"mul_view_src0", c_bin_view, {MUL, 0}, 0},
    {"div_view_src1", c_bin_view, {DIV, 1}, 0},
    {"sub_view_src0", c_bin_view, {SUB, 0}, 0},
    {"add_view_src1", c_bin_view, {ADD, 1}, 0},
    {"add_src1_transposed", c_add_src1_transposed, {0}, 0},
    {"add_special", c_bin_special, {ADD}, 0},
    {"sub_special", c_bin_special, {SUB}, 0},
    {"mul_special", c_bin_special, {MUL}, 0},
    {"div_special", c_bin_special, {DIV}, 0},

    {"repeat_8x1_8x5", c_repeat, {8, 1, 8, 5}, 0},
    {"repeat_1x5_8x5", c_repeat, {1, 5, 8, 5}, 0},
    {"repeat_2x3_6x9", c_repeat, {2, 3, 6, 9}, 0},
    {"repeat_1x1_7x3", c_repeat, {1, 1, 7, 3}, 0},

    {"silu_sweep", c_silu_sweep, {0}, 0},
    {"silu_special", c_silu_special, {0}, 0},
    {"silu_3d", c_silu_3d, {0}, 0},

    {"scale_33x4", c_scale, {33, 4, 1, 0}, 0},
    {"scale_7x3x2", c_scale, {7, 3, 2, 0}, 0},
    {"scale_denormal", c_scale, {33, 4, 1, 1}, 0},

    {"diag_mask_9x4x3_p5", c_diag_mask, {9, 4, 3, 5}, 0},
    {"diag_mask_6x6x1_p0", c_diag_mask, {6, 6, 1, 0}, 0},
    {"diag_mask_9x1x2_p8", c_diag_mask, {9, 1, 2, 8}, 0},
    {"diag_mask_300x2x1_p297", c_diag_mask, {300, 2, 1, 297}, 0},

    {"rms_norm_256x3", c_rms_norm, {256, 3, 1, 0}, 0},
    {"rms_norm_100x2x2", c_rms_norm, {100, 2, 2, 0}, 0},
    {"rms_norm_1x4", c_rms_norm, {1, 4, 1, 0}, 0},
    {"rms_norm_257x2", c_rms_norm, {257, 2, 1, 0}, 0},
    {"rms_norm_1000x2", c_rms_norm, {1000, 2, 1, 0}, 0},
    {"rms_norm_zero_row", c_rms_norm, {40, 3, 1, 1}, 0},
    {"rms_norm_view", c_rms_norm_view, {0}, 0},
    {"rms_norm_mixed_magnitude", c_rms_norm, {300, 3, 1, 2}, 0},

    {"soft_max_len1", c_soft_max_len, {1}, 0},
    {"soft_max_len2", c_soft_max_len, {2}, 0},
    {"soft_max_len63", c_soft_max_len, {63}, 0},
    {"soft_max_len64", c_soft_max_len, {64}, 0},
    {"soft_max_len255", c_soft_max_len, {255}, 0},
    {"soft_max_len256", c_soft_max_len, {256}, 0},
    {"soft_max_len257", c_soft_max_len, {257}, 0},
    {"soft_max_len1000", c_soft_max_len, {1000}, 0},
    {"soft_max_masked", c_soft_max_masked, {0}, 0},
    {"soft_max_wide", c_soft_max_wide, {0}, 0},
    {"soft_max_underflow", c_soft_max_underflow, {0}, 0},

    {"rope_m0_p0", c_rope, {8, 3, 4, 1, 0, 8, 0}, 0},
    {"rope_m0_p5", c_rope, {8, 3, 4, 1, 5, 8, 0}, 0},
    {"rope_m0_p2000", c_rope, {8, 3, 4, 1, 2000, 8, 0}, 0},
    {"rope_m0_ndims4", c_rope, {8, 3, 4, 1, 3, 4, 0}, 0},
    {"rope_m0_4d", c_rope, {8, 2, 3, 2, 7, 8, 0}, 0},
    {"rope_m0_view", c_rope_view, {0}, 0},
    {"rope_m1_p2", c_rope, {8, 3, 6, 1, 2, 8, 1}, 0},
    {"rope_m1_p2_4d_ndims4", c_rope, {8, 2, 5, 2, 2, 4, 1}, 0},
    {"rope_m1_noop_p4", c_rope, {8, 3, 4, 1, 4, 8, 1}, 0},
    {"rope_m1_noop_p6", c_rope, {8, 3, 4, 1, 6, 8, 1}, 0},

    {"get_rows_q4_0", c_get_rows, {Q40, 64, 10, 0}, 0},
    {"get_rows_q4_1", c_get_rows, {Q41, 64, 10, 0}, 0},
    {"get_rows_f16_k50", c_get_rows, {F16, 50, 10, 0}, 0},
    {"get_rows_f32_k33", c_get_rows, {F32, 33, 10, 0}, 0},
    {"get_rows_f32_k300", c_get_rows, {F32, 300, 10, 0}, 0},
    {"get_rows_f32_single", c_get_rows, {F32, 33, 10, 1}, 0},
    {"get_rows_f16_single", c_get_rows, {F16, 50, 10, 1}, 0},
    {"get_rows_q4_0_single", c_get_rows, {Q40, 64, 10, 1}, 0},

    MM_K(F16, "f16", 1, 0, 0, 0, 0),
    MM_K(F16, "f16", 31, 0, 0, 0, 0),
    MM_K(F16, "f16", 32, 0, 0, 0, 0),
    MM_K(F16, "f16", 33, 0, 0, 0, 0),
    MM_K(F16, "f16", 64, 1, 0, 0, 0),
    MM_K(F16, "f16", 95, 0, 0, 0, 0),
    MM_K(F16, "f16", 128, 0, 0, 0, 0),
    MM_K(F32, "f32", 1, 0, 0, 0, 0),
    MM_K(F32, "f32", 31, 0, 0, 0, 0),
    MM_K(F32, "f32", 32, 0, 0, 0, 0),
    MM_K(F32, "f32", 33, 3, 0, 0, 0),
    MM_K(F32, "f32", 64, 0, 0, 0, 0),
    MM_K(F32, "f32", 95, 1, 0, 0, 0),
    MM_K(F32, "f32", 128, 1, 0, 0, 0),
    {"mm_f16_k40_batched", c_mm, {F16, 40, 3, 2, 3, 2}, 0},
    {"mm_f32_k40_batched", c_mm, {F32, 40, 3, 2, 3, 2}, 0},
    {"mm_f16_vcache", c_mm_vcache, {F16}, 0},
    {"mm_f32_vcache", c_mm_vcache, {F32}, 0},
    {"mm_f16_src1_permuted", c_mm_src1_permuted, {F16}, 0},
    {"mm_f32_src1_permuted", c_mm_src1_permuted, {F32}, 0},

    MMQ(Q40, "q4_0"),
    MMQ(Q41, "q4_1"),
};
#define N_CASES ((int) (sizeof(cases) / sizeof(cases[0])))

/* ---- dump --------------------------------------------------------------------------- */
static void dump_tensor(FILE * f, const struct ggml_tensor * t) {
    const int32_t type = (int32_t) t->type;
    fwrite(&type, sizeof type, 1, f);
    fwrite(t->ne, sizeof(int64_t), 4, f);
    const int blck = ggml_blck_size(t->type);
    const size_t es = ggml_type_size(t->type);
    for (int64_t i3 = 0; i3 < t->ne[3]; ++i3)
        for (int64_t i2 = 0; i2 < t->ne[2]; ++i2)
            for (int64_t i1 = 0; i1 < t->ne[1]; ++i1) {
                const char * row = (const char *) t->data + i1 * t->nb[1] + i2 * t->nb[2] + i3 * t->nb[3];
                if (blck > 1) {
                    fwrite(row, es, (size_t) (t->ne[0] / blck), f);
                } else {
                    for (int64_t i0 = 0; i0 < t->ne[0]; ++i0) fwrite(row + i0 * t->nb[0], es, 1, f);
                }
            }
}

int main(int argc, char ** argv) {
    if (argc > 1 && strcmp(argv[1], "--list") == 0) {
        for (int i = 0; i < N_CASES; ++i) printf("%s\n", cases[i].name);
        return 0;
    }
    const int build_only = getenv("OP_TEST_BUILD_ONLY") != NULL;
    FILE * fo = NULL;
    if (!build_only) {
        if (argc < 2) {
            fprintf(stderr, "usage: %s dump.bin | --list   (OP_TEST_BUILD_ONLY=1: print the result tensors)\n", argv[0]);
            return 2;
        }
        fo = fopen(argv[1], "wb");
        if (!fo) return 1;
    }
    ggml_time_init();
    static struct ggml_cgraph gf;
    for (int ci = 0; ci < N_CASES; ++ci) {
        const struct op_case * c = &cases[ci];
        struct ggml_init_params ip = {8u << 20, NULL, false};
        struct rec r;
        memset(&r, 0, sizeof r);
        r.ctx = ggml_init(ip);
        if (!r.ctx) return 1;
        seed_case(c->name, c->salt);
        c->build(&r, c->a);
        if (r.n_out == 0) add_out(&r, r.res);
        if (build_only) {
            const struct ggml_tensor * t = r.res;
            printf("%s: op %d type %d ne %lld %lld %lld %lld nb %zu %zu %zu %zu src0 %d src1 %d used %zu\n", c->name,
                   (int) t->op, (int) t->type, (long long) t->ne[0], (long long) t->ne[1], (long long) t->ne[2],
                   (long long) t->ne[3], t->nb[0], t->nb[1], t->nb[2], t->nb[3],
                   (int) (t->src0 && t->data == t->src0->data), (int) (t->src1 && t->data == t->src1->data),
                   ggml_used_mem(r.ctx));
            ggml_free(r.ctx);
            continue;
        }
        const uint32_t nl = (uint32_t) strlen(c->name), ni = (uint32_t) r.n_in, no = (uint32_t) r.n_out;
        fwrite(&nl, sizeof nl, 1, fo);
        fwrite(c->name, 1, nl, fo);
        fwrite(&ni, sizeof ni, 1, fo);
        fwrite(&no, sizeof no, 1, fo);
        for (int i = 0; i < r.n_in; ++i) dump_tensor(fo, r.in[i]);
        memset(&gf, 0, sizeof gf);
        gf.n_threads = 1;
        ggml_build_forward_expand(&gf, r.res);
        ggml_graph_compute(r.ctx, &gf);
        for (int i = 0; i < r.n_out; ++i) dump_tensor(fo, r.out[i]);
        ggml_free(r.ctx);
    }
    if (fo && fclose(fo) != 0) return 1;
    return 0;
}
