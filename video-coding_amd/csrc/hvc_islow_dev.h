// hvc_islow_dev.h -- device side of libjpeg's jidctint.c inverse DCT (internal): the block code k_islow (hvc_libjpeg.hip, one
// geometry per launch, tables in the kernarg segment) and k_islow_mixed (hvc_mixed_libjpeg.hip, geometry and tables per
// wavefront from device memory) share.  The arithmetic is the operation list of hvc_islow_spec.h, which
// tests/test_islow_guard.py proves; what each path is and why is said at the top of hvc_libjpeg.hip.  Everything here has
// internal linkage: include it in a .hip file only.
#ifndef HVC_ISLOW_DEV_H
#define HVC_ISLOW_DEV_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvc_islow_spec.h"
#include "hvc_rgb_dev.h" /* u2v */

namespace hvc {
namespace {

// natural position -> zig-zag position (hvc_kernels.h HVC_ZF, for device code)
__device__ constexpr int IZF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// v_pk_mul_lo_u16: the low 16 bits of both halves' products
__device__ __forceinline__ unsigned pk_mul_lo(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b));
}
// |lo|, |hi| of an int16 pair as uint16 (-32768 -> 32768)
__device__ __forceinline__ unsigned pk_abs(unsigned a) {
    const u16x2 n = (u16x2)(0) - __builtin_bit_cast(u16x2, a);
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, n)));
}
// half (z & 1) of dword z / 2, sign-extended
__device__ __forceinline__ int half_of(const unsigned (&w)[32], int z) {
    return (z & 1) ? (int)w[z >> 1] >> 16 : (int)(short)(w[z >> 1] & 0xffffu);
}

// value * constant: the int path's multiplicands fit 24 signed bits under the guard (hvc_islow_spec.h)
__device__ __forceinline__ int mulc(int v, int k) { return __mul24(v, k); }

// a result of a step: descaled by SH, or (SH = 0) left to the caller's saturating pack
template <class T, int SH>
__device__ __forceinline__ T result(T x) {
    if constexpr (SH == 0) return x;
    else return (x + ((T)1 << (SH - 1))) >> SH;
}

// The step of hvc_islow_spec.h on int
template <int SH>
__device__ __forceinline__ void islow_step(int v0, int v1, int v2, int v3, int v4, int v5, int v6, int v7, int (&o)[8]) {
    typedef int T;
#define HVC_IS_OP_MUL(d, a, k) const T d = mulc(a, (k));
#define HVC_IS_OP_ADD(d, a, b) const T d = a + b;
#define HVC_IS_OP_SUB(d, a, b) const T d = a - b;
#define HVC_IS_OP_SHL(d, a, n) const T d = a * (T)(1 << (n));
#define HVC_IS_OP_OUTADD(i, a, b) o[i] = result<T, SH>(a + b);
#define HVC_IS_OP_OUTSUB(i, a, b) o[i] = result<T, SH>(a - b);
    HVC_ISLOW_STEP(HVC_IS_OP_MUL, HVC_IS_OP_ADD, HVC_IS_OP_SUB, HVC_IS_OP_SHL, HVC_IS_OP_OUTADD, HVC_IS_OP_OUTSUB)
#undef HVC_IS_OP_MUL
#undef HVC_IS_OP_ADD
#undef HVC_IS_OP_SUB
#undef HVC_IS_OP_SHL
#undef HVC_IS_OP_OUTADD
#undef HVC_IS_OP_OUTSUB
}

// pixel bytes of a, b, c, d: (v >> HVC_IS_PASS2_SHIFT) saturated to [0, 255] (v_ashr_pk_u8_i32)
static_assert(HVC_IS_PASS2_SHIFT == 18, "the pack's shift is spelled in its assembly");
__device__ __forceinline__ unsigned ashr18_sat_pack4(int a, int b, int c, int d) {
    unsigned r;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, 18" : "=v"(r) : "v"(a), "v"(b));
    asm("v_ashr_pk_u8_i32 %0, %1, %2, 18 op_sel:[0,0,0,1]" : "+v"(r) : "v"(c), "v"(d));
    return r;
}

__device__ __forceinline__ void store_row8_nt(uint8_t *p, unsigned lo, unsigned hi) {
    const u2v t = {lo, hi};
    __builtin_nontemporal_store(t, reinterpret_cast<u2v *>(p));
}

// the guard sum S = SUM |coefficient| * table entry over the record w and the table pairs qq, exact and saturating
// (v_dot2_u32_u16 with clamp); a block with S <= HVC_IS_GUARD_SUM takes the int path
__device__ __forceinline__ unsigned islow_guard_sum(const unsigned (&w)[32], const unsigned *__restrict__ qq) {
    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < 32; i++)
        sum = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, pk_abs(w[i])), __builtin_bit_cast(u16x2, qq[i]), sum, true);
    return sum;
}

// the int path: the record w and the table pairs qq -> out[row][0..1] = the row's 8 pixels
__device__ __forceinline__ void islow_block_int(const unsigned (&w)[32], const unsigned *__restrict__ qq, unsigned (&out)[8][2]) {
    unsigned dd[32]; // the dequantised record: int16 pairs, exact under the guard
#pragma unroll
    for (int i = 0; i < 32; i++) dd[i] = pk_mul_lo(w[i], qq[i]);
    int ws[8][8]; // ws[row][col]
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int o[8];
        islow_step<HVC_IS_PASS1_SHIFT>(half_of(dd, IZF[c]), half_of(dd, IZF[8 + c]), half_of(dd, IZF[16 + c]),
                                            half_of(dd, IZF[24 + c]), half_of(dd, IZF[32 + c]), half_of(dd, IZF[40 + c]),
                                            half_of(dd, IZF[48 + c]), half_of(dd, IZF[56 + c]), o);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r][c] = o[r];
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int o[8];
        islow_step<0>(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][4], ws[r][5], ws[r][6], ws[r][7], o);
        constexpr int ADD = (1 << (HVC_IS_PASS2_SHIFT - 1)) + (HVC_IS_LEVEL << HVC_IS_PASS2_SHIFT);
        out[r][0] = ashr18_sat_pack4(o[0] + ADD, o[1] + ADD, o[2] + ADD, o[3] + ADD);
        out[r][1] = ashr18_sat_pack4(o[4] + ADD, o[5] + ADD, o[6] + ADD, o[7] + ADD);
    }
}

__device__ __forceinline__ unsigned sample64(long long x) {
    x += HVC_IS_LEVEL;
    return (unsigned)(x < 0 ? 0ll : x > 255 ? 255ll : x);
}

// The step as a matrix: within a step every value is an exact integer combination of the inputs, so result i is
// D(SUM over k of M[i][k] v[k], sh) with M[i][k] = result i of the undescaled step on the k-th unit vector.
struct IslowMatrix {
    int m[8][8];
};
constexpr IslowMatrix islow_matrix() {
    IslowMatrix M{};
    for (int k = 0; k < 8; k++) {
        const long long v0 = k == 0, v1 = k == 1, v2 = k == 2, v3 = k == 3, v4 = k == 4, v5 = k == 5, v6 = k == 6, v7 = k == 7;
#define HVC_IS_OP_MUL(d, a, c) const long long d = a * (c);
#define HVC_IS_OP_ADD(d, a, b) const long long d = a + b;
#define HVC_IS_OP_SUB(d, a, b) const long long d = a - b;
#define HVC_IS_OP_SHL(d, a, n) const long long d = a * (1 << (n));
#define HVC_IS_OP_OUTADD(i, a, b) M.m[i][k] = (int)(a + b);
#define HVC_IS_OP_OUTSUB(i, a, b) M.m[i][k] = (int)(a - b);
        HVC_ISLOW_STEP(HVC_IS_OP_MUL, HVC_IS_OP_ADD, HVC_IS_OP_SUB, HVC_IS_OP_SHL, HVC_IS_OP_OUTADD, HVC_IS_OP_OUTSUB)
#undef HVC_IS_OP_MUL
#undef HVC_IS_OP_ADD
#undef HVC_IS_OP_SUB
#undef HVC_IS_OP_SHL
#undef HVC_IS_OP_OUTADD
#undef HVC_IS_OP_OUTSUB
    }
    return M;
}
__device__ constexpr IslowMatrix ISM = islow_matrix();
static_assert(ISM.m[0][0] == 1 << HVC_IS_CONST_BITS && ISM.m[7][1] == -ISM.m[0][1], "the step's matrix");

// the int64 path: the block's 8 rows at dst from its record `rec` (coefficient 0 replaced by dc) and the table pairs qq, in
// the matrix form and in real loops -- row r of the workspace is made and used one column at a time, the record is read
// again from memory (it is in the cache) -- so that the path holds 8 sums and little else: the kernel's registers are the
// int path's.  Some five times the butterfly's multiplications, for blocks that no real image has.
__device__ __forceinline__ void islow_block_wide(const int16_t *__restrict__ rec, int dc, const unsigned *__restrict__ qq, uint8_t *dst,
                                                 size_t stride, bool active) {
#pragma unroll 1
    for (int r = 0; r < 8; r++) {
        long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
        for (int c = 0; c < 8; c++) {
            long long t = 0;
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                const int z = IZF[8 * k + c];
                const unsigned q = (z & 1) ? qq[z >> 1] >> 16 : qq[z >> 1] & 0xffffu;
                const int cf = z == 0 ? dc : (int)rec[z];
                t += (long long)ISM.m[r][k] * (long long)(cf * (int)q); // (|int16| * uint16 < 2^31)
            }
            const long long wsv = result<long long, HVC_IS_PASS1_SHIFT>(t);
#pragma unroll
            for (int i = 0; i < 8; i++) acc[i] += (long long)ISM.m[i][c] * wsv;
        }
        unsigned px[8];
#pragma unroll
        for (int i = 0; i < 8; i++) px[i] = sample64(result<long long, HVC_IS_PASS2_SHIFT>(acc[i]));
        if (active)
            store_row8_nt(dst + (size_t)r * stride, px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24, px[4] | px[5] << 8 | px[6] << 16 | px[7] << 24);
    }
}

} // namespace
} // namespace hvc
#endif
