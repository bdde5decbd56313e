// hvc_mixed_encode.hip -- the FORWARD block stage over frames of DIFFERENT geometry and quantiser tables in one launch.
//
// k_encode (hvc_kernels.hip) takes one EncodeParams: up to four planes and four tables in the kernarg segment, grid = tiles x
// frames.  Here the decomposition comes from device memory: hvc_mixed_dev.h says how (the block stage's, and the forward
// tail); a table entry (hvc_mixed_encode_plan.h) holds the 64 reciprocals of the plane's quantiser.
//
// Per lane: k_encode's block in its shipped form (its HVC_ENCODE_MULHI = 1, HVC_ENCODE_QMAGIC = 1, non-temporal loads and
// stores; none of its experiment switches exists here) -- eight 8-byte row loads at the descriptor's stride, the column
// pass from the bytes with the level shift riding in fdct_tail<true>, the row pass, the quantiser as one v_fma_f32 per
// coefficient against fl((1 + 2^-16) / (4 t)) with v_perm_b32 packing the pairs (tests/test_quant_division.py proves the
// quotient; the host makes the reciprocals with the expression k_encode's are made with, encode_quant_reciprocal), then
// the forward tail.  LDS per workgroup: 32 KiB, as k_encode with HVC_TILE 256.  No scratch
// (profiles/mixed_encode_rocprofv3.txt).
//
// (The Huffman coder on the GPU for mixed sets is hvc_huff_mixed.hip, behind hvc_jpeg_encode_batch_mixed_gpu; RGB input for
// mixed sets is k_rgb_to_ycc_mixed, hvc_mixed_rgb.hip, in front of this block stage, behind hvc_jpeg_encode_batch_mixed_rgb.)
// Out of scope, each a step of its own:
//   - the Hardcaml encode arithmetic (hvc_set_encode_arithmetic): the entry points return HVC_E_INVALID_ARG under it
//   - monochrome files
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_mixed_dev.h"
#include "hvc_mixed_encode.h"

namespace hvc {
namespace {

// zig-zag position -> natural position (zigzag.ml:5-69)
__device__ constexpr int EZI[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// dct.ml:109-112.  The multiplies are issued explicitly, constant in an SGPR, operands < 2^15 (k_encode says why).
__device__ __forceinline__ int e_mul24(int k, int x) {
    int d;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(d) : "s"(k), "v"(x));
    return d;
}
__device__ __forceinline__ int e_mad24(int k, int x, int acc) {
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "s"(k), "v"(x), "v"(acc));
    return d;
}
// c4 without its shift: (362 x) >> 9 = the high dword of (x << 9) * (362 << 14) as a 24 x 24 -> 48 bit product, exact
// while |x| < 2^14 (the sums c4 sees are <= 1024 in the column pass, <= 5792 in the row pass: tests/test_guard_bounds.py)
__device__ __forceinline__ int e_mulhi24(int k, int x) {
    int d;
    asm("v_mul_hi_i32_i24 %0, %1, %2" : "=v"(d) : "s"(k), "v"(x));
    return d;
}
__device__ __forceinline__ int e_c62(int f, int g) { return e_mad24(473, g, e_mul24(196, f)) >> 9; }
__device__ __forceinline__ int e_c71(int f, int g) { return e_mad24(502, g, e_mul24(100, f)) >> 9; }
__device__ __forceinline__ int e_c35(int f, int g) { return e_mad24(284, g, e_mul24(426, f)) >> 9; }
// c62 b3 (-b2), c35 a2 (-a1), c71 a3 (-a0): the negation rides in the constant
__device__ __forceinline__ int e_c62n(int f, int g) { return e_mad24(-473, g, e_mul24(196, f)) >> 9; }
__device__ __forceinline__ int e_c71n(int f, int g) { return e_mad24(-502, g, e_mul24(100, f)) >> 9; }
__device__ __forceinline__ int e_c35n(int f, int g) { return e_mad24(-284, g, e_mul24(426, f)) >> 9; }

// dct.ml:114-149 (dct_col) / :151-187 (dct_row) share one butterfly: here after its first stage, from the sums a0..a3
// and the differences c0..c3.  LS = the sums still carry the +256 of two un-shifted pixels: only b0 + b1 sees it.
template <bool LS>
__device__ __forceinline__ void fdct_tail(int a0, int a1, int a2, int a3, int c0, int c1, int c2, int c3, int &p0, int &p1,
                                          int &p2, int &p3, int &p4, int &p5, int &p6, int &p7) {
    constexpr int C4S = 362 << 14;
    const int b0s = (a0 + a3) << 9, b1s = (a1 + a2) << 9, b2 = a1 - a2, b3 = a0 - a3;
    p0 = e_mulhi24(C4S, LS ? b0s + b1s - (1024 << 9) : b0s + b1s);
    p4 = e_mulhi24(C4S, b0s - b1s); // c4 b0 (-b1): the level shift cancels
    p2 = e_c62(b2, b3);
    p6 = e_c62n(b3, b2);            // c62 b3 (-b2)
    const int c2s = c2 << 9;
    const int b0 = e_mulhi24(C4S, e_mad24(-512, c1, c2s)); // c4 c2 (-c1)
    const int b1 = e_mulhi24(C4S, e_mad24(512, c1, c2s));
    a0 = c0 + b0;
    a1 = c0 - b0;
    a2 = c3 - b1;
    a3 = c3 + b1;
    p1 = e_c71(a0, a3);
    p5 = e_c35(a1, a2);
    p3 = e_c35n(a2, a1); // c35 a2 (-a1)
    p7 = e_c71n(a3, a0); // c71 a3 (-a0)
}

// byte BYTE of a  +/-  byte BYTE of b: the unpacking of the pixel bytes rides in the SDWA source selectors
template <int BYTE>
__device__ __forceinline__ int e_add_bytes(unsigned a, unsigned b) {
    int d;
    if (BYTE == 0) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:BYTE_0" : "=v"(d) : "v"(a), "v"(b));
    if (BYTE == 1) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:BYTE_1" : "=v"(d) : "v"(a), "v"(b));
    if (BYTE == 2) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:BYTE_2" : "=v"(d) : "v"(a), "v"(b));
    if (BYTE == 3) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:BYTE_3" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
template <int BYTE>
__device__ __forceinline__ int e_sub_bytes(unsigned a, unsigned b) {
    int d;
    if (BYTE == 0) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:BYTE_0" : "=v"(d) : "v"(a), "v"(b));
    if (BYTE == 1) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:BYTE_1" : "=v"(d) : "v"(a), "v"(b));
    if (BYTE == 2) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:BYTE_2" : "=v"(d) : "v"(a), "v"(b));
    if (BYTE == 3) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:BYTE_3" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// Column pass (dct.ml:114-149) of column C from the eight packed pixel rows (two dwords each).  level_shifted_input_block
// (encoder.ml:87) subtracts 128 from every pixel: differences do not see it, sums carry +256, and past the first stage
// only b0 + b1 uses sums -- so the shift is one "- 1024" (fdct_tail<true>) instead of 64 subtractions.
template <int C>
__device__ __forceinline__ void fdct_col_bytes(const unsigned (&px)[8][2], int (&v)[64]) {
    constexpr int D = C >> 2, B = C & 3;
    const int a0 = e_add_bytes<B>(px[0][D], px[7][D]), c3 = e_sub_bytes<B>(px[0][D], px[7][D]);
    const int a1 = e_add_bytes<B>(px[1][D], px[6][D]), c2 = e_sub_bytes<B>(px[1][D], px[6][D]);
    const int a2 = e_add_bytes<B>(px[2][D], px[5][D]), c1 = e_sub_bytes<B>(px[2][D], px[5][D]);
    const int a3 = e_add_bytes<B>(px[3][D], px[4][D]), c0 = e_sub_bytes<B>(px[3][D], px[4][D]);
    fdct_tail<true>(a0, a1, a2, a3, c0, c1, c2, c3, v[C], v[8 + C], v[16 + C], v[24 + C], v[32 + C], v[40 + C], v[48 + C],
                    v[56 + C]);
}

__global__ __launch_bounds__(HVC_MIXED_LANES) void k_encode_mixed(MixedEncodeParams P) {
    unsigned wf, wt;
    xcd_work(P.xcd_map, P.xcd_magic, wf, wt); // gridDim.y == 1: a permutation of the groups (or the plain order)
    const unsigned group = wf * gridDim.x + wt;
    const int wv = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & (HVC_MIXED_UNIT - 1));
    const unsigned unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(group * HVC_MIXED_GROUP + (unsigned)wv));
    if (unit >= P.n_units) return; // (the whole wavefront: the last group's spare units; no barrier below)
    const MixedPlaneK &K = P.planes[P.map[unit]];
    const float *__restrict__ qr = P.tables[K.table].qrcp;
    const int wave_b0 = (int)(unit - K.unit0) * HVC_MIXED_UNIT; // block (inside the plane) of lane 0
    const int nblk = K.nblk; // (read once, here: behind the stores below the compiler would load it again, per store)
    int b = wave_b0 + l;
    b = b < nblk ? b : nblk - 1; // an inactive lane computes the plane's last block and stores nothing
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const size_t stride = (size_t)K.stride;
    const uint8_t *pix = P.pixels + (size_t)K.pix_base + (size_t)by * 8 * stride + (size_t)bx * 8;
    // 8 rows x 8 B per lane, read once
    typedef unsigned u2l __attribute__((ext_vector_type(2)));
    unsigned px[8][2];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u2l w = __builtin_nontemporal_load(reinterpret_cast<const u2l *>(pix + (size_t)j * stride));
        px[j][0] = w.x;
        px[j][1] = w.y;
    }
    // Dct.Chen.forward_8x8 (dct.ml:189-196): columns first, then rows
    int v[64];
    fdct_col_bytes<0>(px, v);
    fdct_col_bytes<1>(px, v);
    fdct_col_bytes<2>(px, v);
    fdct_col_bytes<3>(px, v);
    fdct_col_bytes<4>(px, v);
    fdct_col_bytes<5>(px, v);
    fdct_col_bytes<6>(px, v);
    fdct_col_bytes<7>(px, v);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int *p = v + r * 8;
        fdct_tail<false>(p[0] + p[7], p[1] + p[6], p[2] + p[5], p[3] + p[4], p[3] - p[4], p[2] - p[5], p[1] - p[6], p[0] - p[7],
                         p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
    }
    // Encoder.quant (encoder.ml:103-108): quant[zz] = quant_and_scale fdct[ZI[zz]] table[zz], as ONE fused multiply-add per
    // coefficient: float(f) * r + 1.5 * 2^23 rounds (to nearest, once, at an ulp of 1) to 1.5 * 2^23 + q, whose low 16 bits
    // ARE q in two's complement; the int16 pair is one v_perm_b32 of the two bit patterns.  The wave's 64 records go
    // through its own LDS region -- XOR-swizzled 16-byte slots, conflict-free for the ds_write_b128 (lane l writes slot
    // 8 l + (c ^ (l & 7))) and for the ds_read_b128 -- and leave as whole 1 KiB runs (k_encode says what that buys).
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    __shared__ u4v lds[HVC_MIXED_GROUP][512];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        unsigned w[4];
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const int k = j * 8 + h * 2;
            const float plo = __builtin_fmaf((float)v[EZI[k]], qr[k], 12582912.f);
            const float phi = __builtin_fmaf((float)v[EZI[k + 1]], qr[k + 1], 12582912.f);
            w[h] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, phi), __builtin_bit_cast(unsigned, plo), 0x05040100u);
        }
        const u4v t = {w[0], w[1], w[2], w[3]};
        lds[wv][l * 8 + (j ^ (l & 7))] = t;
    }
    // (wave-private LDS region: the wave's own ds ops are ordered, no barrier needed)
    u4v *dst = reinterpret_cast<u4v *>(P.coefs + (size_t)K.coef_base + (size_t)wave_b0 * 64);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int blk = 8 * j + (l >> 3), ch = l & 7;
        const u4v t = lds[wv][blk * 8 + (ch ^ (blk & 7))];
        if (wave_b0 + blk < nblk) __builtin_nontemporal_store(t, dst + j * 64 + l);
    }
}

} // namespace

hipError_t launch_encode_mixed(const MixedEncodeParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch_xcd(k_encode_mixed, P, s, k0, k1);
}

} // namespace hvc
