// hvc_scaled_dev.h -- device side of the reduced-size inverse DCT (internal): what k_decode_scaled (hvc_scaled.hip, one
// geometry per launch) and k_decode_mixed_scaled (hvc_mixed_scaled.hip, geometry per wavefront from device memory) share --
// one block per lane from its loaded record to its N x N samples, the int32 guard, and the stores that join the lanes of a
// pair / quad into one dword.  Constants and guard: hvc_scaled_spec.h; the definition: include/hvc_jpeg.h ("Decoding at
// reduced size").  Everything here has internal linkage: include it in a .hip file only.
#ifndef HVC_SCALED_DEV_H
#define HVC_SCALED_DEV_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvc_scaled_spec.h"

namespace {

// natural position -> zig-zag position (hvc_kernels.h HVC_ZF, for device code)
__device__ constexpr int SZF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// d[k] of the definition: coefficient at natural position k (halfword SZF[k] of the record) times its table entry; both
// factors fit 24 signed bits, the product fits int32
__device__ __forceinline__ int dequant(const unsigned (&w)[32], const int *__restrict__ q, int k) {
    const int z = SZF[k];
    const int c = (z & 1) ? (int)w[z >> 1] >> 16 : (int)(short)(w[z >> 1] & 0xffffu);
    return __mul24(c, q[z]);
}

// constant * value: the int32 path's multiplicands fit 24 signed bits under the guard (hvc_scaled_spec.h)
__device__ __forceinline__ int mulc(int k, int v) { return __mul24(k, v); }
__device__ __forceinline__ long long mulc(int k, long long v) { return (long long)k * v; }

template <class T>
__device__ __forceinline__ T descale(T x, int n) { return (x + ((T)1 << (n - 1))) >> n; }

template <class T>
__device__ __forceinline__ unsigned sample(T x) {
    x += 128;
    return (unsigned)(x < 0 ? (T)0 : x > 255 ? (T)255 : x);
}

template <class T>
__device__ __forceinline__ void step4(T v0, T v1, T v2, T v3, T v5, T v6, T v7, int sh, T (&o)[4]) {
    const T t0 = v0 * (T)(1 << HVC_S4_V0_SHIFT);
    const T t2 = mulc(HVC_S4_V2, v2) - mulc(HVC_S4_V6, v6);
    const T t10 = t0 + t2, t12 = t0 - t2;
    const T o0 = mulc(HVC_S4_O0_V5, v5) - mulc(HVC_S4_O0_V7, v7) - mulc(HVC_S4_O0_V3, v3) + mulc(HVC_S4_O0_V1, v1);
    const T o2 = mulc(HVC_S4_O2_V3, v3) - mulc(HVC_S4_O2_V7, v7) - mulc(HVC_S4_O2_V5, v5) + mulc(HVC_S4_O2_V1, v1);
    o[0] = descale(t10 + o2, sh);
    o[1] = descale(t12 + o0, sh);
    o[2] = descale(t12 - o0, sh);
    o[3] = descale(t10 - o2, sh);
}

template <class T>
__device__ __forceinline__ void step2(T v0, T v1, T v3, T v5, T v7, int sh, T (&o)[2]) {
    const T t10 = v0 * (T)(1 << HVC_S2_V0_SHIFT);
    const T t0 = mulc(HVC_S2_V5, v5) - mulc(HVC_S2_V7, v7) - mulc(HVC_S2_V3, v3) + mulc(HVC_S2_V1, v1);
    o[0] = descale(t10 + t0, sh);
    o[1] = descale(t10 - t0, sh);
}

// out[r] = row r of the block's N x N samples, first sample in the low byte
template <class T>
__device__ __forceinline__ void idct4(const int (&d)[64], unsigned (&out)[4]) {
    T ws[4][8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        if (c == 4) continue;
        T o[4];
        step4<T>(d[c], d[8 + c], d[16 + c], d[24 + c], d[40 + c], d[48 + c], d[56 + c], HVC_S4_PASS1_SHIFT, o);
#pragma unroll
        for (int r = 0; r < 4; r++) ws[r][c] = o[r];
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        T o[4];
        step4<T>(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][5], ws[r][6], ws[r][7], HVC_S4_PASS2_SHIFT, o);
        out[r] = sample(o[0]) | sample(o[1]) << 8 | sample(o[2]) << 16 | sample(o[3]) << 24;
    }
}

template <class T>
__device__ __forceinline__ void idct2(const int (&d)[64], unsigned (&out)[2]) {
    T ws[2][8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        if (c != 0 && !(c & 1)) continue;
        T o[2];
        step2<T>(d[c], d[8 + c], d[24 + c], d[40 + c], d[56 + c], HVC_S2_PASS1_SHIFT, o);
        ws[0][c] = o[0];
        ws[1][c] = o[1];
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        T o[2];
        step2<T>(ws[r][0], ws[r][1], ws[r][3], ws[r][5], ws[r][7], HVC_S2_PASS2_SHIFT, o);
        out[r] = sample(o[0]) | sample(o[1]) << 8;
    }
}

// does the definition for N use natural row / column i?
template <int N>
__device__ __forceinline__ constexpr bool uses(int i) { return N == 4 ? i != 4 : (i == 0 || (i & 1)); }

// The lane's 128-byte record as eight 16-byte loads into W[32].  This and the two macros below are spelled inline in their
// kernels (hvc_kernels.hip HVC_DECODE_BLOCK_PACKED says why a macro: the kernels keep the register figures of the spelled-out
// form).
#define HVC_SCALED_LOAD_RECORD(REC, W)                                                              \
    do {                                                                                            \
        const uint4 *src_ = reinterpret_cast<const uint4 *>(REC);                                   \
        _Pragma("unroll") for (int j = 0; j < 8; j++) {                                             \
            const uint4 v = src_[j];                                                                \
            (W)[4 * j] = v.x, (W)[4 * j + 1] = v.y, (W)[4 * j + 2] = v.z, (W)[4 * j + 3] = v.w;     \
        }                                                                                           \
    } while (0)

// N = 1: the sample of a block with DC coefficient c0 and table entry q0  (|d[0]| + 4 < 2^31)
__device__ __forceinline__ unsigned block1(int c0, int q0) { return sample(descale(__mul24(c0, q0), HVC_S1_SHIFT)); }

// N = 4, 2 (a constant expression): the loaded record W, table Q -> OUT[N]: only the positions the definition uses are
// multiplied, then the guard of hvc_scaled_spec.h, the int32 path under it and the int64 path (same formulas, same lane)
// outside; NARROW (a bool lvalue): the block took the int32 path
#define HVC_SCALED_BLOCK(N, W, Q, OUT, NARROW)                                                                                   \
    do {                                                                                                                         \
        int d[64];                                                                                                               \
        unsigned ac = 0;                                                                                                         \
        _Pragma("unroll") for (int r = 0; r < 8; r++) {                                                                          \
            if (!uses<N>(r)) continue;                                                                                           \
            _Pragma("unroll") for (int c = 0; c < 8; c++) {                                                                      \
                if (!uses<N>(c)) continue;                                                                                       \
                const int v = dequant((W), (Q), 8 * r + c);                                                                      \
                d[8 * r + c] = v;                                                                                                \
                if (r | c) ac = max(ac, (unsigned)abs(v));                                                                       \
            }                                                                                                                    \
        }                                                                                                                        \
        const unsigned dc = (unsigned)abs(d[0]);                                                                                 \
        const unsigned long long g = N == 4 ? (unsigned long long)HVC_S4_GUARD_WD * dc + (unsigned long long)HVC_S4_GUARD_WA * ac \
                                            : (unsigned long long)HVC_S2_GUARD_WD * dc + (unsigned long long)HVC_S2_GUARD_WA * ac; \
        (NARROW) = g <= (N == 4 ? HVC_S4_GUARD_LIMIT : HVC_S2_GUARD_LIMIT);                                                      \
        if constexpr (N == 4) {                                                                                                  \
            if (NARROW) idct4<int>(d, (OUT));                                                                                    \
            else idct4<long long>(d, (OUT));                                                                                     \
        } else {                                                                                                                 \
            if (NARROW) idct2<int>(d, (OUT));                                                                                    \
            else idct2<long long>(d, (OUT));                                                                                     \
        }                                                                                                                        \
    } while (0)

template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }

__device__ __forceinline__ void store_bytes(uint8_t *p, unsigned v, int n) {
    for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// the byte form: rows that do not start on 4-byte boundaries
#define HVC_SCALED_STORE_BYTES(N, DST, STRIDE, OUT, ACTIVE)                                                \
    do {                                                                                                   \
        if (ACTIVE) {                                                                                      \
            _Pragma("unroll") for (int r = 0; r < N; r++) store_bytes((DST) + (size_t)r * (STRIDE), (OUT)[r], N); \
        }                                                                                                  \
    } while (0)

// The dword form (every row of the plane starts on a 4-byte boundary): N = 4 one dword per lane and row; N = 2 joins the
// two lanes of a pair, N = 1 the four lanes of a quad by DPP where the pair / quad lies in one block row on a 4-byte
// boundary (it starts on an even / multiple-of-4 BX and does not run past BW), and stores 2 / 1 bytes where it does not.
// Run by every lane of the wavefront (the DPP reads its neighbours); LANE = the lane's number in a run of lanes that hold
// consecutive blocks of the plane, the run starting at a multiple of 4 blocks.
#define HVC_SCALED_STORE_DWORDS(N, DST, STRIDE, OUT, LANE, BX, BW, ACTIVE)                                                                   \
    do {                                                                                                                                     \
        if constexpr (N == 4) {                                                                                                              \
            if (ACTIVE) {                                                                                                                    \
                _Pragma("unroll") for (int r = 0; r < 4; r++)                                                                                \
                    __builtin_nontemporal_store((OUT)[r], reinterpret_cast<unsigned *>((DST) + (size_t)r * (STRIDE)));                       \
            }                                                                                                                                \
        } else if constexpr (N == 2) {                                                                                                       \
            /* the pair (lane, lane ^ 1) holds blocks (bx0, bx0 + 1) of one block row with bx0 even: its 4 bytes are one dword */           \
            const int lp = (LANE) & 1, bx0 = (BX) - lp;                                                                                      \
            const bool joined = (BX) >= lp && !(bx0 & 1) && bx0 + 1 < (BW);                                                                  \
            const unsigned o0 = (OUT)[0] | dpp<0xB1>((OUT)[0]) << 16, o1 = (OUT)[1] | dpp<0xB1>((OUT)[1]) << 16; /* quad_perm:[1,0,3,2] */   \
            if (ACTIVE) {                                                                                                                    \
                if (joined) {                                                                                                                \
                    if (!lp) {                                                                                                               \
                        __builtin_nontemporal_store(o0, reinterpret_cast<unsigned *>(DST));                                                  \
                        __builtin_nontemporal_store(o1, reinterpret_cast<unsigned *>((DST) + (STRIDE)));                                     \
                    }                                                                                                                        \
                } else {                                                                                                                     \
                    *reinterpret_cast<unsigned short *>(DST) = (unsigned short)(OUT)[0];                                                     \
                    *reinterpret_cast<unsigned short *>((DST) + (STRIDE)) = (unsigned short)(OUT)[1];                                        \
                }                                                                                                                            \
            }                                                                                                                                \
        } else {                                                                                                                             \
            /* the quad holds blocks bx0 .. bx0 + 3 of one block row with bx0 a multiple of 4: one dword */                                  \
            const int lq = (LANE) & 3, bx0 = (BX) - lq;                                                                                      \
            const bool joined = (BX) >= lq && !(bx0 & 3) && bx0 + 3 < (BW);                                                                  \
            const unsigned o = dpp<0x00>((OUT)[0]) | dpp<0x55>((OUT)[0]) << 8 | dpp<0xAA>((OUT)[0]) << 16 | dpp<0xFF>((OUT)[0]) << 24;       \
            if (ACTIVE) {                                                                                                                    \
                if (joined) {                                                                                                                \
                    if (!lq) __builtin_nontemporal_store(o, reinterpret_cast<unsigned *>(DST));                                              \
                } else {                                                                                                                     \
                    (DST)[0] = (uint8_t)(OUT)[0];                                                                                            \
                }                                                                                                                            \
            }                                                                                                                                \
        }                                                                                                                                    \
    } while (0)

} // namespace
#endif
