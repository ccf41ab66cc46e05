// matvec_cols_common.h -- what the two Q4_0 columns kernels share (matvec_cols.hip: the row lengths
// 4096 / 11008 compiled in; matvec_cols_long.hip: any chunk count): the parameter block, the packed
// column image that k_cols_act writes, the per-wave block-scale slices.
#pragma once
#include "matvec_common.h"

namespace lvk {
namespace cols {

struct ColsParams : mv::MvArgs {
    const uint4 * nib;
    const float4 * scl;
    const uint4 * img;          // the packed column image (k_cols_act), column t at t * CS16
    int G;                      // row groups (M / 8)
    int M;                      // rows: the column stride of y (u: M / 2)
    int col0, ncols;            // this launch's columns [col0, col0 + ncols)
};

// per-wave block-scale slice (8 rows x 32 blocks), row stride padded as in matvec_cu.hip: the
// per-row broadcast float4 reads are bank-conflict free
constexpr int SRS = 40, SPL = 8 * SRS;

// packed column image / LDS table of one column of K = 32 nb elements, in uint4 units:
//   [nb]     nibbles: uint4 (8 u + j), u < nb / 8, chain j: word k = a(8u + 2k, j) | a(8u + 2k + 1, j) << 16,
//            a(i, j) = the signed nibbles of elements 4j .. 4j + 3 of block i (16 bits)
//   [NC * 8] dx: float [c][j][m] = dx of block 32 c + 8 m + j (0 past the row's end)
__host__ __device__ constexpr int cols_stride16(int K) { return K / 32 + (K / 32 + 31) / 32 * 8; }

// matvec_cols_long.hip: the row lengths it takes, and the matmul of a step of n columns on the image
// that launch_matvec_cols has written (P filled but for col0 / ncols)
bool cols_long_supported(int K);
hipError_t launch_cols_long(const ColsParams & P, int K, int epi, int n, hipStream_t s);

}  // namespace cols
}  // namespace lvk
