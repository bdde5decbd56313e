// hvc_scaled.hip -- k_decode_scaled: coefficient records -> planes at 1/2, 1/4 or 1/8 size (N = 4, 2, 1 samples per block
// side) by the reduced-size inverse DCT of include/hvc_jpeg.h ("Decoding at reduced size"; constants and the int32
// guard: hvc_scaled_spec.h; numpy restatement: tools/scaled_reference.py).
//
// One block per lane with k_decode_packed's geometry (tiles of HVC_TILE consecutive blocks of one plane, grid = tiles x
// frames, the same XCD work map): consecutive lanes hold horizontally consecutive blocks of one block row, so the N bytes
// per lane of an output row are contiguous across the wavefront.  N = 4 stores one dword per lane and row; N = 2 joins the
// two lanes of a pair, N = 1 the four lanes of a quad into one dword by DPP where the pair / quad lies in one block row on a
// 4-byte boundary, and falls back to 2-byte / 1-byte stores where it does not.  The byte form (DW = false) serves planes
// whose rows do not start on 4-byte boundaries.  N = 4 and 2 read the lane's 128-byte record as eight 16-byte loads and
// multiply only the positions the definition uses; N = 1 reads the dword that holds the DC -- or, DCP, nothing but the
// compact DC array.  No LDS, no scratch.
//
// Blocks outside the int32 guard run the same formulas in int64 in the same lane (a rare divergent branch); their number
// goes to P.wide_total with one atomic per wavefront that has such a block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_scaled_spec.h"

namespace hvc {
namespace {

// natural position -> zig-zag position (hvc_kernels.h HVC_ZF, for device code)
__device__ constexpr int SZF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct ScaledRef {
    size_t coef_idx; // int16 element index of the block's 64 coefficients
    size_t rel_blk;  // block index inside the frame's coefficient record (the compact DC array's index)
    size_t pix_idx;  // byte index of the block's top-left output sample
    size_t stride;
    int qtab, bx, bw;
    bool active;
};

// locate() of hvc_kernels.hip with N bytes and N rows per block
template <int N>
__device__ __forceinline__ ScaledRef locate_scaled(const DecodeParams &P, unsigned frame, int tile, int lane) {
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && tile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    int b = (tile - K.tile0) * HVC_TILE + lane;
    ScaledRef r;
    r.active = b < K.nblk;
    b = r.active ? b : K.nblk - 1;
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    r.rel_blk = (K.coef_off >> 6) + (size_t)b;
    r.coef_idx = (size_t)frame * P.coef_fs + K.coef_off + (size_t)b * 64;
    r.pix_idx = (size_t)frame * P.pixel_fs + K.plane_off + (size_t)by * N * K.stride + (size_t)bx * N;
    r.stride = K.stride;
    r.qtab = K.qtab;
    r.bx = (int)bx;
    r.bw = K.bw;
    return r;
}

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

template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }

__device__ __forceinline__ void store_bytes(uint8_t *p, unsigned v, int n) {
    for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}

template <int N, bool DCP, bool DW>
__global__ __launch_bounds__(HVC_TILE) void k_decode_scaled(DecodeParams P) {
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    const ScaledRef br = locate_scaled<N>(P, wframe, (int)wtile, lane);
    const int *__restrict__ q = P.qt + br.qtab * 64; // wave-uniform, kernarg segment
    int16_t dcv = 0;
    if (DCP) dcv = P.dc_plane[(size_t)wframe * P.dc_fs + br.rel_blk];
    unsigned out[N];
    bool wide = false;
    if constexpr (N == 1) {
        int c0 = dcv;
        if (!DCP) c0 = (int)(short)(*reinterpret_cast<const unsigned *>(P.coefs + br.coef_idx) & 0xffffu);
        out[0] = sample(descale(__mul24(c0, q[0]), HVC_S1_SHIFT)); // (|d[0]| + 4 < 2^31)
    } else {
        const uint4 *src = reinterpret_cast<const uint4 *>(P.coefs + br.coef_idx);
        unsigned w[32];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint4 v = src[j];
            w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
        }
        if (DCP) w[0] = (w[0] & 0xffff0000u) | (unsigned)(unsigned short)dcv;
        int d[64];
        unsigned ac = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (!uses<N>(r)) continue;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                if (!uses<N>(c)) continue;
                const int v = dequant(w, q, 8 * r + c);
                d[8 * r + c] = v;
                if (r | c) ac = max(ac, (unsigned)abs(v));
            }
        }
        const unsigned dc = (unsigned)abs(d[0]);
        const unsigned long long g = N == 4 ? (unsigned long long)HVC_S4_GUARD_WD * dc + (unsigned long long)HVC_S4_GUARD_WA * ac
                                            : (unsigned long long)HVC_S2_GUARD_WD * dc + (unsigned long long)HVC_S2_GUARD_WA * ac;
        const bool narrow = g <= (N == 4 ? HVC_S4_GUARD_LIMIT : HVC_S2_GUARD_LIMIT);
        if constexpr (N == 4) {
            if (narrow) idct4<int>(d, out);
            else idct4<long long>(d, out);
        } else {
            if (narrow) idct2<int>(d, out);
            else idct2<long long>(d, out);
        }
        wide = br.active && !narrow;
    }

    uint8_t *dst = P.pixels + br.pix_idx;
    if constexpr (!DW) {
        if (br.active) {
#pragma unroll
            for (int r = 0; r < N; r++) store_bytes(dst + (size_t)r * br.stride, out[r], N);
        }
    } else if constexpr (N == 4) {
        if (br.active) {
#pragma unroll
            for (int r = 0; r < 4; r++) __builtin_nontemporal_store(out[r], reinterpret_cast<unsigned *>(dst + (size_t)r * br.stride));
        }
    } else if constexpr (N == 2) {
        // the pair (lane, lane ^ 1) holds blocks (bx0, bx0 + 1) of one block row with bx0 even: its 4 bytes are one dword
        const int lp = lane & 1, bx0 = br.bx - lp;
        const bool joined = br.bx >= lp && !(bx0 & 1) && bx0 + 1 < br.bw;
        const unsigned o0 = out[0] | dpp<0xB1>(out[0]) << 16, o1 = out[1] | dpp<0xB1>(out[1]) << 16; // quad_perm:[1,0,3,2]
        if (br.active) {
            if (joined) {
                if (!lp) {
                    __builtin_nontemporal_store(o0, reinterpret_cast<unsigned *>(dst));
                    __builtin_nontemporal_store(o1, reinterpret_cast<unsigned *>(dst + br.stride));
                }
            } else {
                *reinterpret_cast<unsigned short *>(dst) = (unsigned short)out[0];
                *reinterpret_cast<unsigned short *>(dst + br.stride) = (unsigned short)out[1];
            }
        }
    } else {
        // the quad holds blocks bx0 .. bx0 + 3 of one block row with bx0 a multiple of 4: one dword
        const int lq = lane & 3, bx0 = br.bx - lq;
        const bool joined = br.bx >= lq && !(bx0 & 3) && bx0 + 3 < br.bw;
        const unsigned o = dpp<0x00>(out[0]) | dpp<0x55>(out[0]) << 8 | dpp<0xAA>(out[0]) << 16 | dpp<0xFF>(out[0]) << 24; // quad_perm:[k,k,k,k]
        if (br.active) {
            if (joined) {
                if (!lq) __builtin_nontemporal_store(o, reinterpret_cast<unsigned *>(dst));
            } else {
                dst[0] = (uint8_t)out[0];
            }
        }
    }

    if constexpr (N > 1) {
        const unsigned long long m = __ballot(wide);
        if (m && (lane & 63) == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

template <int N>
void launch_n(const DecodeParams &Q, bool dwords, dim3 grid, hipStream_t s) {
    if (Q.dc_plane) {
        if (dwords) hipLaunchKernelGGL((k_decode_scaled<N, true, true>), grid, dim3(HVC_TILE), 0, s, Q);
        else hipLaunchKernelGGL((k_decode_scaled<N, true, false>), grid, dim3(HVC_TILE), 0, s, Q);
    } else {
        if (dwords) hipLaunchKernelGGL((k_decode_scaled<N, false, true>), grid, dim3(HVC_TILE), 0, s, Q);
        else hipLaunchKernelGGL((k_decode_scaled<N, false, false>), grid, dim3(HVC_TILE), 0, s, Q);
    }
}

} // namespace

hipError_t launch_decode_scaled(const DecodeParams &P, int n, bool dwords, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (n != 4 && n != 2 && n != 1) return hipErrorInvalidValue;
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    DecodeParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic); // (xcd_work: every XCD takes runs of consecutive tiles)
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (n == 4) launch_n<4>(Q, dwords, grid, s);
    else if (n == 2) launch_n<2>(Q, dwords, grid, s);
    else launch_n<1>(Q, dwords, grid, s);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc
