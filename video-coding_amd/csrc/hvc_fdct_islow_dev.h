// hvc_fdct_islow_dev.h -- one block of the libjpeg-exact encoder on the device: jfdctint.c's forward DCT as the operation list
// of hvc_fdct_islow_spec.h, and libjpeg's rounded division by 8 q through the host-made multipliers of
// hvc_libjpeg_encode_plan.h.  Shared by the kernels of hvc_libjpeg_encode.hip.
//
// Every product of the list is v_mul_i32_i24's: the constants are below 2^15, the data operand below 2^23 and no value leaves
// int32 (tests/test_fdct_islow_bounds.py, for 8-bit samples: no guard and no wide path).  The quotient is one v_mul_hi_u32_u24 per
// coefficient (tests/host_harness/libjpeg_encode_plan_harness.cpp exhausts it against C's /).
#ifndef HVC_FDCT_ISLOW_DEV_H
#define HVC_FDCT_ISLOW_DEV_H

#include <hip/hip_runtime.h>

#include "hvc_fdct_islow_spec.h"
#include "hvc_libjpeg_encode_plan.h"

namespace hvc {

// the step of pass PASS (1: along a row, 2: down a column) on v0 .. v7 -> o[0 .. 7], scaled as the spec says
template <int PASS>
__device__ __forceinline__ void fdct_islow_step(int v0, int v1, int v2, int v3, int v4, int v5, int v6, int v7, int (&o)[8]) {
    constexpr int HI = PASS == 1 ? HVC_FI_PASS1_HI_SHIFT : HVC_FI_PASS2_HI_SHIFT;
#define HVC_FI_MUL(d, a, k) const int d = __mul24(a, (k));
#define HVC_FI_ADD(d, a, b) const int d = (a) + (b);
#define HVC_FI_SUB(d, a, b) const int d = (a) - (b);
#define HVC_FI_OUTLO(i, a) \
    o[i] = PASS == 1 ? (a) << HVC_FI_PASS1_LO_SHL : ((a) + (1 << (HVC_FI_PASS2_LO_SHIFT - 1))) >> HVC_FI_PASS2_LO_SHIFT;
#define HVC_FI_OUTHI(i, a) o[i] = ((a) + (1 << (HI - 1))) >> HI;
    HVC_FDCT_ISLOW_STEP(HVC_FI_MUL, HVC_FI_ADD, HVC_FI_SUB, HVC_FI_OUTLO, HVC_FI_OUTHI)
#undef HVC_FI_MUL
#undef HVC_FI_ADD
#undef HVC_FI_SUB
#undef HVC_FI_OUTLO
#undef HVC_FI_OUTHI
}

// the high dword of a 24 x 24 bit product, full rate (v_mul_hi_u32 takes four passes)
__device__ __forceinline__ unsigned fdct_islow_mul_hi_u24(unsigned a, unsigned b) {
    unsigned d;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// zig-zag position -> natural position (jpeg/model/src/zigzag.ml:3-69)
constexpr unsigned char FDCT_ISLOW_ZI[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One block: pixel rows px[r] (8 bytes each, two dwords) -> the record's 32 dwords (zig-zag int16 pairs, DC absolute).
// magic / half: the table's 64 words in natural order (libjpeg_encode_tables), uniform over the wave (scalar loads).
__device__ __forceinline__ void fdct_islow_block(const unsigned (&px)[8][2], const unsigned *__restrict__ magic,
                                                 const unsigned *__restrict__ half, unsigned (&out)[32]) {
    int w[8][8]; // w[r][i]: result i of row r
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int x[8];
#pragma unroll
        for (int c = 0; c < 8; c++) x[c] = (int)((px[r][c >> 2] >> (8 * (c & 3))) & 0xffu) - HVC_FI_LEVEL;
        fdct_islow_step<1>(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], w[r]);
    }
    int z[64]; // the quantised coefficients, natural order
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int t[8];
        fdct_islow_step<2>(w[0][c], w[1][c], w[2][c], w[3][c], w[4][c], w[5][c], w[6][c], w[7][c], t);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int k = 8 * i + c;
            const unsigned a = (unsigned)abs(t[i]);
            const int q = (int)fdct_islow_mul_hi_u24((a + half[k]) << HVC_LJE_NUMERATOR_SHIFT, magic[k]); // = libjpeg_quant_divide
            z[k] = t[i] < 0 ? -q : q;
        }
    }
#pragma unroll
    for (int i = 0; i < 32; i++)
        out[i] = ((unsigned)z[FDCT_ISLOW_ZI[2 * i]] & 0xffffu) | ((unsigned)z[FDCT_ISLOW_ZI[2 * i + 1]] << 16);
}

} // namespace hvc
#endif
