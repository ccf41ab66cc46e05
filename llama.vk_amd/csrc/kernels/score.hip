// score.hip -- the device half of scoring a token (examples/perplexity/perplexity.cpp:6-20, 70).
//
// The reference copies every logits row to the host, runs softmax over all n_vocab entries and
// keeps one of them: probs[target].  Here one workgroup per row does that over the logits in
// HBM and only the probability crosses PCIe.  The arithmetic is the reference's:
//   mx   = the row maximum, started at x[0] with std::max's rule (a NaN in x[0] stays, a NaN
//          elsewhere is not taken)
//   e_i  = expf(x_i - mx), the subtraction and the result in float
//   S    = sum of the e_i, in double
//   prob = (float) ((double) e_target / S)
// so NaN rows, a +inf maximum (inf - inf), an all -inf row, a target far below the maximum (0,
// or a denormal, which the default kernel mode keeps) come out as on the host.  expf itself is
// the double-precision exp of the float argument rounded to float: within half an ulp of the true
// value, so within one ulp of glibc's expf (documented at 0.502 ulp) for every argument.  S is
// a tree of non-negative doubles, far below float resolution away from the host's index-order sum.
//
// The row is read from memory once: 16-byte loads from the first 16-byte boundary of the row on,
// up to 3 single floats in front of it and up to 3 behind, everything held in registers
// (SCORE_MAX_VOCAB / 1024 floats per thread) across the maximum and the sum.
#include "lvk_device.h"
#include "lvk_kernels.h"

namespace lvk {

namespace {

constexpr int ST = 1024;                          // threads (one workgroup)
constexpr int PER4 = SCORE_MAX_VOCAB / 4 / ST;    // float4 per thread

__device__ __forceinline__ float exp_f32(float d) { return (float) exp((double) d); }

// workgroup i: row i of logits[.][V] and targets[i] -> probs[i] (-1.0f for a target < 0)
__global__ __launch_bounds__(ST) void k_score_rows(const float * __restrict__ logits, int V,
                                                   const int * __restrict__ targets, float * __restrict__ probs) {
    __shared__ float red_mx[ST / 64];
    __shared__ double red_s[ST / 64];
    __shared__ float s_et;
    const int tid = threadIdx.x, row = blockIdx.x;
    const int target = targets[row];
    if (target < 0) {       // uniform over the workgroup: nobody reaches a barrier
        if (tid == 0) probs[row] = -1.0f;
        return;
    }
    const float * __restrict__ x = logits + (size_t) row * V;
    // x[0 .. head) singles, then n4 float4 from the 16-byte boundary, then tail singles
    const int head = min(V, (int) ((16u - (unsigned) ((uintptr_t) x & 15u)) & 15u) >> 2);
    const int n4 = (V - head) >> 2;
    const int tail0 = head + n4 * 4;
    const float4 * __restrict__ x4 = (const float4 *) (x + head);
    float4 v[PER4];
#pragma unroll
    for (int j = 0; j < PER4; ++j) {
        const int k = j * ST + tid;
        v[j] = k < n4 ? x4[k] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
    // the singles: thread t < head holds x[t], the next V - tail0 threads the tail
    const int xi = tid < head ? tid : tail0 + (tid - head);
    const bool has_x = tid < head + (V - tail0);
    const float xv = has_x ? x[xi] : -INFINITY;
    const float x0 = x[0];

    // maximum: a NaN never compares greater, a padding -inf never wins over a real entry
    float m = xv;
    if (!(m == m)) m = -INFINITY;
#pragma unroll
    for (int j = 0; j < PER4; ++j) {
        if (v[j].x > m) m = v[j].x;
        if (v[j].y > m) m = v[j].y;
        if (v[j].z > m) m = v[j].z;
        if (v[j].w > m) m = v[j].w;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off, 64);
        if (o > m) m = o;
    }
    if ((tid & 63) == 0) red_mx[tid >> 6] = m;
    __syncthreads();
    float mx = red_mx[0];
#pragma unroll
    for (int w = 1; w < ST / 64; ++w)
        if (red_mx[w] > mx) mx = red_mx[w];
    if (!(x0 == x0)) mx = x0;       // max_logit = logits[0] stays when it is NaN

    // e_i and their sum; the thread that holds the target publishes e_target
    double s = 0.0;
    if (has_x) {
        const float e = exp_f32(xv - mx);
        s += (double) e;
        if (xi == target) s_et = e;
    }
#pragma unroll
    for (int j = 0; j < PER4; ++j) {
        const int k = j * ST + tid;
        if (k < n4) {
            const int i = head + 4 * k;
            const float e0 = exp_f32(v[j].x - mx), e1 = exp_f32(v[j].y - mx);
            const float e2 = exp_f32(v[j].z - mx), e3 = exp_f32(v[j].w - mx);
            s += ((double) e0 + (double) e1) + ((double) e2 + (double) e3);
            if ((unsigned) (target - i) < 4u) s_et = target == i ? e0 : target == i + 1 ? e1 : target == i + 2 ? e2 : e3;
        }
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((tid & 63) == 0) red_s[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double S = red_s[0];
#pragma unroll
        for (int w = 1; w < ST / 64; ++w) S += red_s[w];
        probs[row] = (float) ((double) s_et / S);
    }
}

}  // namespace

hipError_t launch_score_rows(const float * logits, int V, int n, const int * targets, float * probs, hipStream_t s) {
    if (!logits || !targets || !probs || n <= 0 || V <= 0 || V > SCORE_MAX_VOCAB) return hipErrorInvalidValue;
    LVK_LAUNCH(k_score_rows, dim3(n), dim3(ST), 0, s, logits, V, targets, probs);
    return hipGetLastError();
}

}  // namespace lvk
