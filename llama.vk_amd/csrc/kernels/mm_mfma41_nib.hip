// mm_mfma41_nib.hip -- the Q4_1 prompt matmul of mm_mfma41.hip on the weights the model already
// holds: the A-side operands come from the decode "octet" image (k_repack_q41, misc.hip) instead
// of the f16 + side images (3 B per weight).  Same tile, same block arithmetic (block41), same
// epilogues and tile order; bit-identical results.  Per row and 32-block chunk it streams
// 512 B of nibbles + 128 B d + 128 B m + 128 B weight sums = 896 B where a16 + side take 3072 B.
//
// Where block41's A-side operands of MFMA lane (rho, h) of wave w come from (row = m0 + 32w + rho,
// g = row >> 3, r = row & 7, block b of chunk c = b >> 5, sub-chunk sb = (b & 31) >> 3):
//   chain fragments   nib[g][c][sb][8r + 2cp + h] (uint4 = chain 2cp + h of the sub-chunk's 8
//                     blocks), cp = 0..3: 4 x 16 B per lane and sub-chunk, one sub-chunk ahead.
//                     Unsigned nibbles -> f16 q by the magic-exponent trick
//                     (0x6400 | q = 1024 + q, 0x4C00 | q << 4 = 16 + q/4) in the order e0 e2 e1 e3.
//   d | m (sa.z)      scl[g][c][h][8r + (b & 7)], component sb
//   S operand         h = 1: ones.  h = 0: the row's four group sums of the block, bytes of
//                     wsum[g][c][8r + 2k + ((b & 31) >> 4)] (k = 0..3), byte b & 15; at most 120, so
//                     (byte | 0x6400) - 1024 is an exact f16 conversion.
// The side data (d, m, sums) is in [row][block of chunk] order in memory and wanted per block.  It is
// staged once per chunk in a wave-private LDS area by LDS-DMA (dma1k), and the transpose is done by
// the DMA's source addresses -- a lane of a DMA may fetch any 16 bytes -- not by LDS stores:
//   DM  8 DMAs: DMA j, lane (h, rho) <- scl[g][c][h][8r + j]   (d | m of blocks j, 8+j, 16+j, 24+j)
//   WS  4 DMAs: DMA k, lane (hf, rho) <- wsum[g][c][8r + 2k + hf]  (group k, blocks 16hf .. 16hf+15)
// so DM is [j][lane] x 16 B and WS [k][hf][rho] x 16 B.  A sub-chunk then takes 8 ds_read_b32 (dword
// sb of DM[j][lane], j = its 8 blocks) and 4 ds_read_b64 (the sub-chunk's 8 sum bytes of group k)
// into 16 registers; a block's d | m is one of them and its packed sums two v_perm_b32.  The DMA
// writes are 1 KiB runs (no bank conflicts); the reads stride 16 B across lanes (4 lanes per bank),
// 12 LDS reads per 8 blocks against their 80 MFMAs and 1168 FMAs: off the critical path.
// The area is single-buffered: once the reads of a chunk's last sub-chunk have returned
// (lgkmcnt(0)), the next chunk's 12 DMAs are issued and land under that sub-chunk's 8 blocks.
// The nibbles take the same road: 4 DMAs per sub-chunk into one of two 4 KiB buffers ([cp][lane] x
// 16 B), issued one sub-chunk ahead; a pair of blocks reads its 4 words (ds_read_b32) from there.
// Held in registers instead (16 for the sub-chunk + 16 in flight) the kernel spilled 18 registers.
// Every DMA is followed by the 24 token-ring loads of the sub-chunk it lands under, and loads
// return in order, so vmcnt(3 PDN) at a sub-chunk's start -- the ring's last refills, nothing older --
// covers its DMAs (DESIGN section 4 rules 2 and 8); hipcc's own counts do not see the DMAs and are
// therefore only stricter.  No workgroup barrier anywhere.
// LDS: 4 waves x (8 KiB DM + 4 KiB WS + 2 x 4 KiB nibbles) = 80 KiB per workgroup: two workgroups
// fill a CU's 160 KiB, and __launch_bounds__(256, 2) keeps the registers for two waves per SIMD.
// The token images xm / xs stream 2 blocks deep in registers (24), as k_mm_q41_mfma's ring does
// 3 deep: a depth that divides the 8 unrolled blocks keeps the slot index static
// (profiles/q41_nib_kernel_resources.md has the register, LDS and scratch figures).
// K % 256 == 0: the last chunk may hold 8, 16 or 24 blocks; the loop runs nb / 8 sub-chunks and
// stops there, so no zero-filled block enters a chain.  The DMAs of a partial chunk read the
// zero fill k_repack_q41 wrote (the images are allocated by whole chunks).
#include "mm41_common.h"

namespace lvk {

namespace {

constexpr int TM = MM_TM, NT = MM_NT;
constexpr int PDN = 2;                        // blocks of the token images in flight per wave
constexpr int SIDE_DM = 8 * 1024;             // [8 j][64 lanes] x 16 B
constexpr int SIDE_WS = 4 * 1024;             // [4 k][2 hf][32 rho] x 16 B
constexpr int NIB_SUB = 4 * 1024;              // [4 cp][64 lanes] x 16 B, one sub-chunk; two buffers
constexpr int WAVE_LDS = SIDE_DM + SIDE_WS + 2 * NIB_SUB;
constexpr int LDSN = 4 * WAVE_LDS;

struct Mm41NibParams {
    const uint4 * nib;       // [M/8][NC][4][64]
    const uint4 * scl;       // [M/8][NC][2][64] (d, m)
    const uint4 * wsum;      // [M/8][NC][64]
    const uint4 * xm;        // [ntt][nb][2][64]
    const uint4 * xs;        // [ntt][nb][64]
    int M, nb;
    MmOut o;
};

struct XBlk {                // one block's token-side operands of one lane
    uint4 b[2], sb;
};

// 16-bit chain field (4 unsigned nibbles e0..e3) selected by sel from X -> f16 q: e0 e2 e1 e3
__device__ __forceinline__ uint2 unpack_chain41(uint32_t X, uint32_t sel) {
    const uint32_t t = __builtin_amdgcn_perm(X, X, sel);            // byte0 | byte1 << 16
    const uint32_t lo = (t & 0x000F000Fu) | 0x64006400u;            // (e0, e2) = 1024 + q
    const uint32_t hi = (t & 0x00F000F0u) | 0x4C004C00u;            // (e1, e3) = 16 + q/4
    const half2_t c1024 = {(_Float16) -1024.0f, (_Float16) -1024.0f};
    const half2_t c4 = {(_Float16) 4.0f, (_Float16) 4.0f};
    const half2_t c64 = {(_Float16) -64.0f, (_Float16) -64.0f};
    const half2_t h0 = __builtin_bit_cast(half2_t, lo) + c1024;
    const half2_t h1 = __builtin_elementwise_fma(__builtin_bit_cast(half2_t, hi), c4, c64);
    return make_uint2(__builtin_bit_cast(uint32_t, h0), __builtin_bit_cast(uint32_t, h1));
}

// bytes `sel & 3` of lo and of hi (sums <= 120) as two f16: (byte | 0x6400) - 1024
__device__ __forceinline__ uint32_t sums_f16(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint32_t t = __builtin_amdgcn_perm(hi, lo, sel) | 0x64006400u;
    const half2_t c1024 = {(_Float16) -1024.0f, (_Float16) -1024.0f};
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2_t, t) + c1024);
}

template <int EPI>
__global__ __launch_bounds__(NT, 2) void k_mm_q41_nib(Mm41NibParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const MmOrigin og = mm_origin(P.o.ntt, P.M / TM);
    const int tt = og.tt, m0 = og.m0, n0 = og.n0;
    const int nb = P.nb, NC = (nb + 31) / 32;
    const int U = nb / 8;                                    // sub-chunks of 8 blocks
    const int rho = lane & 31, h = lane >> 5;
    const int row = m0 + 32 * w + rho;
    const size_t g = (size_t) (row >> 3);
    const int r = row & 7;

    // ---- side data of chunk c -> this wave's LDS area, transposed by the DMA's source addresses
    const uint4 * dmp = P.scl + g * NC * 128 + h * 64 + 8 * r;       // + c * 128 + j
    const uint4 * wsp = P.wsum + g * NC * 64 + 8 * r + h;            // + c * 64 + 2k  (hf = h)
    uint8_t * side = smem + w * WAVE_LDS;
    const unsigned side_l = __builtin_amdgcn_readfirstlane(lds_addr41(side));
    auto issue_side = [&](int c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dma1k(dmp + (size_t) c * 128 + j, side_l + j * 1024);
#pragma unroll
        for (int k = 0; k < 4; ++k) dma1k(wsp + (size_t) c * 64 + 2 * k, side_l + SIDE_DM + k * 1024);
    };
    const uint32_t * dml = (const uint32_t *) side + lane * 4;         // + j * 256 + sb
    const uint2 * wsl = (const uint2 *) (side + SIDE_DM) + rho * 2;    // + (k * 64 + hf * 32) * 2 + (sb & 1)

    // ---- chain fragments: octet lanes 8r + 2cp + h, one uint4 per chain pair and sub-chunk, by
    // DMA into buffer u & 1 as [cp][lane] x 16 B; word jb >> 1 of it serves blocks jb, jb + 1
    const uint4 * ap = P.nib + g * NC * 256 + 8 * r + h;
    auto issue_nib = [&](int u) {
        const uint4 * p = ap + (size_t) u * 64;                        // (c * 4 + sb) * 64 == u * 64
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) dma1k(p + 2 * cp, side_l + SIDE_DM + SIDE_WS + (u & 1) * NIB_SUB + cp * 1024);
    };
    const uint32_t * nibl = (const uint32_t *) (side + SIDE_DM + SIDE_WS) + lane * 4;   // + (u & 1) * 1024 + cp * 256 + word
    // ---- token side: as k_mm_q41_mfma, PDN blocks deep
    const uint4 * bp = P.xm + (size_t) tt * nb * 128 + lane;
    const uint4 * sbp = P.xs + (size_t) tt * nb * 64 + lane;
    auto load_x = [&](int blk, XBlk & x) {
        x.b[0] = bp[(size_t) blk * 128];
        x.b[1] = bp[(size_t) blk * 128 + 64];
        x.sb = sbp[(size_t) blk * 64];
    };

    f32x16_t acc[4], off;
    mm_zero(acc);
    mm_zero(off);

    XBlk ring[PDN];
    issue_side(0);
    issue_nib(0);
#pragma unroll
    for (int d = 0; d < PDN; ++d) load_x(min(d, nb - 1), ring[d]);

    for (int u = 0; u < U; ++u) {
        const int sb = u & 3;
        // this sub-chunk's 4 nibble DMAs (and, first of a chunk, its 12 side DMAs) are older than
        // the token ring's 3 PDN refills in flight
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(3 * PDN) : "memory");
        uint32_t dm[8];
        uint2 ws[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) dm[j] = dml[j * 256 + sb];
#pragma unroll
        for (int k = 0; k < 4; ++k) ws[k] = wsl[(k * 64 + (sb >> 1) * 32) * 2 + (sb & 1)];
        if (u + 1 < U) {
            // these reads and sub-chunk u - 1's nibble reads have returned: the side area is free after
            // a chunk's last sub-chunk (the next chunk lands under it), nibble buffer (u + 1) & 1 always
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (sb == 3) issue_side((u >> 2) + 1);
            issue_nib(u + 1);
        }
        const uint32_t * nl = nibl + (u & 1) * (NIB_SUB / 4);
        uint32_t X[4];
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
            const int blk = 8 * u + jb;
            XBlk & x = ring[jb % PDN];
            const uint32_t sel = (jb & 1) ? 0x0C030C02u : 0x0C010C00u;
            if ((jb & 1) == 0) {
#pragma unroll
                for (int cp = 0; cp < 4; ++cp) X[cp] = nl[cp * 256 + (jb >> 1)];
            }
            uint2 f[4];
#pragma unroll
            for (int cp = 0; cp < 4; ++cp) f[cp] = unpack_chain41(X[cp], sel);
            // byte jb of the sub-chunk's sums: group k from ws[k], pairs (0, 1) and (2, 3)
            const uint32_t bsel = 0x0C040C00u | (uint32_t) (jb & 3) | (uint32_t) (jb & 3) << 16;
            const uint32_t w0 = jb < 4 ? ws[0].x : ws[0].y, w1 = jb < 4 ? ws[1].x : ws[1].y;
            const uint32_t w2 = jb < 4 ? ws[2].x : ws[2].y, w3 = jb < 4 ? ws[3].x : ws[3].y;
            const uint32_t ones = F16_ONE | F16_ONE << 16;
            Blk o;
            o.a[0] = make_uint4(f[0].x, f[0].y, f[1].x, f[1].y);
            o.a[1] = make_uint4(f[2].x, f[2].y, f[3].x, f[3].y);
            o.b[0] = x.b[0]; o.b[1] = x.b[1]; o.sb = x.sb;
            o.sa = make_uint4(h ? ones : sums_f16(w1, w0, bsel), h ? ones : sums_f16(w3, w2, bsel), dm[jb], 0u);
            block41(o, acc, off);
            // refill this slot PDN blocks ahead (its MFMAs have consumed it)
            load_x(min(blk + PDN, nb - 1), x);
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(acc[c]));
        }
    }

    mm_finish<EPI>(P.o, acc, lane, w, m0, n0, off);
}

}  // namespace

hipError_t mm_q41_nib(const MmLaunch & L, int epi, hipStream_t s) {
    const QMatrix & w = L.w;
    Mm41NibParams P{};
    P.nib = w.nib; P.scl = (const uint4 *) w.scl; P.wsum = q41_wsum(w);
    P.xm = (const uint4 *) L.x.xm; P.xs = (const uint4 *) L.x.xs;
    P.M = w.M; P.nb = w.K / 32;
    P.o = mm_out(L, epi);
    const dim3 grid((w.M / TM) * P.o.ntt);
    return mm_epi_dispatch<Q4_1>(epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        LVK_LAUNCH(k_mm_q41_nib<E>, grid, dim3(NT), LDSN, s, P);
        return hipGetLastError();
    });
}

}  // namespace lvk
