// mm41_common.h -- what the Q4_1 prompt matmul kernels share (mm_mfma41.hip: the two kernels on
// the f16 + side images; mm_mfma41_nib.hip: the kernel on the octet image): one block's operands
// of a lane, the block arithmetic, and the 1 KiB LDS-DMA.
#pragma once
#include "mm_common.h"

namespace lvk {
namespace {

struct Blk {                 // one block's operands of one lane
    uint4 a[2], b[2], sa, sb;
};

// One block of a lane's chains (every kernel): the scale products, the chain partials P and
// cross-term operands S from the matrix cores, then the reference's fmaf chains and offset
__device__ __forceinline__ void block41(const Blk & o, f32x16_t (&acc)[4], f32x16_t & off) {
    const float sw = __builtin_bit_cast(float, o.sa.z);      // d | m of the row
    const float sb1 = __builtin_bit_cast(float, o.sb.z);     // d | m of the token
    const float sb2 = __builtin_bit_cast(float, o.sb.w);     // (m | d) where h == jj, else 0
    // dx*dy (registers 0..15) and mx*my (16..31); dx*my | mx*dy by column parity
    const f32x32_t SM = __builtin_amdgcn_mfma_f32_32x32x1f32(sw, sb1, (f32x32_t){}, 0, 0, 0);
    const f32x16_t SX = __builtin_amdgcn_mfma_f32_32x32x2f32(sw, sb2, (f32x16_t){}, 0, 0, 0);
    const half4_t ax = __builtin_bit_cast(half4_t, make_uint2(o.sa.x, o.sa.y));
    const uint32_t bfr[8] = {o.b[0].x, o.b[0].y, o.b[0].z, o.b[0].w, o.b[1].x, o.b[1].y, o.b[1].z, o.b[1].w};
    const uint32_t afr[8] = {o.a[0].x, o.a[0].y, o.a[0].z, o.a[0].w, o.a[1].x, o.a[1].y, o.a[1].z, o.a[1].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const half4_t a = __builtin_bit_cast(half4_t, make_uint2(afr[2 * c], afr[2 * c + 1]));
        const half4_t b = __builtin_bit_cast(half4_t, make_uint2(bfr[2 * c], bfr[2 * c + 1]));
        // the S operand's B fragment: slot c of the token's sums (or of e_c)
        const uint32_t yw = (c < 2) ? o.sb.x : o.sb.y;
        const uint32_t ym = yw & ((c & 1) ? 0xFFFF0000u : 0x0000FFFFu);
        const half4_t bs = __builtin_bit_cast(half4_t, (c < 2) ? make_uint2(ym, 0u) : make_uint2(0u, ym));
        const f32x16_t Pc = __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, (f32x16_t){}, 0, 0, 0);
        const f32x16_t Sc = __builtin_amdgcn_mfma_f32_32x32x8f16(ax, bs, (f32x16_t){}, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            acc[c][i] = __builtin_fmaf(SM[i], Pc[i], acc[c][i]);      // ggml.c:2244
            acc[c][i] = __builtin_fmaf(SX[i], Sc[i], acc[c][i]);      // ggml.c:2247
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) off[i] = off[i] + SM[16 + i];      // ggml.c:2226
}

__device__ __forceinline__ unsigned lds_addr41(const void * p) {
    return (unsigned) (uintptr_t) (const __attribute__((address_space(3))) uint8_t *) p;
}
// one 1 KiB LDS-DMA: lane l's 16 bytes at gsrc (any address per lane) land at LDS byte lds_dst + 16 l
__device__ __forceinline__ void dma1k(const void * gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

}  // namespace
}  // namespace lvk
