// hvc_libjpeg.hip -- the two kernels of hvc_set_arithmetic(HVC_ARITH_LIBJPEG): the decoder of include/hvc_jpeg.h
// ("Bit-exact to libjpeg"; numpy restatement: tools/libjpeg_reference.py).
//
// k_islow: coefficient records -> planes by libjpeg's jidctint.c inverse DCT.  Mapping: k_hardcaml's / k_decode_packed's --
// one 8x8 block per lane, a tile of HVC_TILE consecutive blocks of one plane per workgroup, grid = tiles x frames,
// workgroups -> (frame, tile) by xcd_work.  A lane loads its 128-byte record (8 x 16 B), keeps all 64 values in VGPRs and
// stores 8 rows of 8 bytes: the kernel moves the model path's bytes.  No LDS, no scratch.
//   guard       S = SUM |coefficient| * table entry, exact and saturating: v_pk_sub_i16 + v_pk_max_i16 for the magnitudes,
//               v_dot2_u32_u16 with clamp against the table pair of each record dword (hvc_islow_spec.h)
//   int path    (S <= HVC_IS_GUARD_SUM) dequantisation by v_pk_mul_lo_u16 per record dword -- every product fits int16 --,
//               the step of hvc_islow_spec.h on int with v_mul_i32_i24 products in both passes (tests/test_islow_guard.py
//               proves the bounds); pass 2's rounding and the level shift ride in one addend, shift and saturation by
//               v_ashr_pk_u8_i32
//   int64 path  every other block, in the same lane (a rare divergent branch): the same step as its 8 x 8 integer matrix
//               (made from the list at compile time) on long long, in real loops over a record read again from the cache,
//               so that the path needs no registers beyond the int path's; counted in P.wide_total with one atomic per
//               wavefront that has such a block
// Both paths give the definition's value for every int16 coefficient and every 16-bit table entry.
//
// k_ycc_to_rgb_fancy: k_ycc_to_rgb's lane (hvc_rgb.hip: 8 columns of one row, of two rows for 4:2:0) with libjpeg's
// "fancy" triangle filter in place of the model's supersampling; loads of Y, colour matrix and stores are the shared
// code of hvc_rgb_dev.h (8-byte and byte-wise paths, interleaved and planar, strides).  A lane reads its four chroma
// samples of a row as one dword where alignment allows and its two neighbours, clamped to the chroma WINDOW, as byte LOADS
// (not DPP: the neighbours of a wavefront's end lanes and of a lane row's ends would need the loads anyway, and the bytes
// sit in lines the adjacent lanes have just fetched); 4:2:0 reads three window rows.  The clamp gives libjpeg's edge
// rules by itself: (3 s + s + 1) >> 2 = s, (3 t + t + 8) >> 4 = (4 t + 8) >> 4.  Windows at most 2 samples wide are replicated
// (libjpeg picks its plain routine there): an image-uniform branch.
#include "hvc_ctx.h"
#include "hvc_islow_spec.h"
#include "hvc_libjpeg.h"
#include "hvc_rgb_dev.h"

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

// DCP: the DC comes from P.dc_plane
template <bool DCP>
__global__ __launch_bounds__(HVC_TILE) void k_islow(IslowParams P) {
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && (int)wtile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    int b = ((int)wtile - K.tile0) * HVC_TILE + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1; // (inactive lanes compute the plane's last block and store nothing)
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const size_t coef_idx = (size_t)wframe * P.coef_fs + K.coef_off + (size_t)b * 64;
    uint8_t *dst = P.pixels + (size_t)wframe * P.pixel_fs + K.plane_off + (size_t)by * 8 * K.stride + (size_t)bx * 8;
    const unsigned *__restrict__ qq = P.qq + K.qtab * 32; // wave-uniform, kernarg segment

    unsigned w[32];
    const uint4 *src = reinterpret_cast<const uint4 *>(P.coefs + coef_idx);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 t = src[j];
        w[4 * j + 0] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
    }
    if (DCP) w[0] = (w[0] & 0xffff0000u) | (unsigned)(unsigned short)P.dc_plane[(size_t)wframe * P.dc_fs + (K.coef_off >> 6) + (size_t)b];

    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < 32; i++)
        sum = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, pk_abs(w[i])), __builtin_bit_cast(u16x2, qq[i]), sum, true);
    const bool narrow = !P.all_wide && sum <= (unsigned)HVC_IS_GUARD_SUM;
    if (narrow) {
        unsigned out[8][2];
        islow_block_int(w, qq, out);
        if (active) {
#pragma unroll
            for (int j = 0; j < 8; j++) store_row8_nt(dst + (size_t)j * K.stride, out[j][0], out[j][1]);
        }
    } else {
        islow_block_wide(P.coefs + coef_idx, half_of(w, 0), qq, dst, K.stride, active);
    }
    if (!P.all_wide) {
        const unsigned long long m = __ballot(active && !narrow);
        if (m && (lane & 63) == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

} // namespace

void prepare_islow_tables(const uint16_t *qtabs, int n_qtabs, unsigned *qq) {
    for (int t = 0; t < n_qtabs; t++)
        for (int i = 0; i < 32; i++) qq[t * 32 + i] = (unsigned)qtabs[t * 64 + 2 * i] | (unsigned)qtabs[t * 64 + 2 * i + 1] << 16;
}

hipError_t launch_islow(const IslowParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    IslowParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic);
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (P.dc_plane) hipLaunchKernelGGL(k_islow<true>, grid, dim3(HVC_TILE), 0, s, Q);
    else hipLaunchKernelGGL(k_islow<false>, grid, dim3(HVC_TILE), 0, s, Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc

// ---------------------------------------------------------------------------
// The colour pass with libjpeg's fancy upsampling
namespace {

// samples c0 - 1 .. c0 + 4 of a chroma row of n valid samples, clamped to the row's window [0, n - 1]; c0 < n
__device__ __forceinline__ void load6(const uint8_t *row, int c0, int n, bool vec, int (&s)[6]) {
    unsigned a, nb;
    load4n(row, c0, n, vec, a, nb);
    s[0] = (int)row[max(c0 - 1, 0)];
#pragma unroll
    for (int i = 0; i < 4; i++) s[1 + i] = (int)((a >> (8 * i)) & 0xffu);
    s[5] = (int)(nb >> 24);
}
// the triangle filter along a row: t[0..5] = positions c0 - 1 .. c0 + 4 -> the 8 samples 2 c0 .. 2 c0 + 7
__device__ __forceinline__ void fancy_h(const int (&t)[6], int r0, int r1, int sh, unsigned &lo, unsigned &hi) {
    unsigned o[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned e = (unsigned)((3 * t[i + 1] + t[i] + r0) >> sh), d = (unsigned)((3 * t[i + 1] + t[i + 2] + r1) >> sh);
        o[i >> 1] |= (e | d << 8) << (16 * (i & 1));
    }
    lo = o[0], hi = o[1];
}

// S: 420, 422, 444 or 400 (luma only).  Lanes: ceil(w / 8) per lane row; a lane row is one image row (4:2:0: two).
template <int S, int PLANAR>
__global__ __launch_bounds__(256) void k_ycc_to_rgb_fancy(RgbOp P) {
    constexpr int ROWS = S == 420 ? 2 : 1;
    const unsigned groups = (unsigned)(P.w + 7) >> 3, lrows = S == 420 ? (unsigned)(P.h + 1) >> 1 : (unsigned)P.h;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * lrows) return;
    const unsigned lr = t / groups, g = t - lr * groups;
    const size_t f = blockIdx.y;
    const int x0 = (int)(8 * g);
    const bool full = x0 + 8 <= P.w;
    unsigned cb[ROWS][2], cr[ROWS][2];
    if (S == 444) {
        load8(P.cb + f * P.yuv_fs + (size_t)lr * P.cb_stride, x0, P.cw, P.vec_c && full, cb[0][0], cb[0][1]);
        load8(P.cr + f * P.yuv_fs + (size_t)lr * P.cr_stride, x0, P.cw, P.vec_c && full, cr[0][0], cr[0][1]);
    } else if (S != 400) {
        const int c0 = (int)(4 * g); // (8 g < w, so c0 < ceil(w / 2) <= cw)
        const bool vc = P.vec_c && c0 + 4 <= P.cw;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint8_t *plane = (k ? P.cr : P.cb) + f * P.yuv_fs;
            const size_t stride = k ? P.cr_stride : P.cb_stride;
            unsigned(*out)[2] = k ? cr : cb;
            const uint8_t *row = plane + (size_t)lr * stride;
            if (P.cw <= 2) { // plain replication, 2x or 2x2
                unsigned a, an;
                load4n(row, c0, P.cw, vc, a, an);
                interleave(a, a, out[0][0], out[0][1]);
                out[ROWS - 1][0] = out[0][0], out[ROWS - 1][1] = out[0][1];
                continue;
            }
            int s[6];
            load6(row, c0, P.cw, vc, s);
            if (S == 422) {
                fancy_h(s, 1, 2, 2, out[0][0], out[0][1]);
            } else {
                int up[6], dn[6];
                load6(plane + (size_t)(lr ? lr - 1u : 0u) * stride, c0, P.cw, vc, up);
                load6(plane + (size_t)min(lr + 1u, (unsigned)P.ch - 1u) * stride, c0, P.cw, vc, dn);
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    up[i] += 3 * s[i];
                    dn[i] += 3 * s[i];
                }
                fancy_h(up, 8, 7, 4, out[0][0], out[0][1]);
                fancy_h(dn, 8, 7, 4, out[ROWS - 1][0], out[ROWS - 1][1]);
            }
        }
    }
    uint8_t *frame = P.rgb + f * P.frame_stride;
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++) {
        const int row = (int)lr * ROWS + rr;
        if (row >= P.h) break;
        unsigned y[2], r[2], gg[2], b[2];
        load8(P.y + f * P.yuv_fs + (size_t)row * P.y_stride, x0, P.w, P.vec_y && full, y[0], y[1]);
        if (S == 400) {
            r[0] = gg[0] = b[0] = y[0];
            r[1] = gg[1] = b[1] = y[1];
        } else {
            ycc4_to_rgb(y[0], cb[rr][0], cr[rr][0], r[0], gg[0], b[0]);
            ycc4_to_rgb(y[1], cb[rr][1], cr[rr][1], r[1], gg[1], b[1]);
        }
        store_rgb<PLANAR>(P, frame, row, x0, P.vec_rgb && full, r, gg, b);
    }
}

template <int PLANAR>
void launch_fancy(int sampling, dim3 grid, hipStream_t s, const RgbOp &P) {
    switch (sampling) {
    case HVC_YUV_420: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<420, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_422: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<422, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_444: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<444, PLANAR>), grid, dim3(256), 0, s, P); break;
    default: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<400, PLANAR>), grid, dim3(256), 0, s, P); break;
    }
}

} // namespace

// ycc_to_rgb_device (hvc_rgb.hip) with k_ycc_to_rgb_fancy: the same arguments, the same launches of at most 65535 frames
hipError_t ycc_to_rgb_fancy_device(const uint8_t *d_yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int w, int h, int cw,
                                   int ch, int n_frames, uint8_t *d_rgb, const RgbImage &im, hipStream_t s) {
    if (n_frames <= 0 || w <= 0 || h <= 0) return hipSuccess;
    const bool grey = sampling == HVC_YUV_400;
    RgbOp P;
    std::memset(&P, 0, sizeof P);
    P.w = w, P.h = h, P.cw = cw, P.ch = ch;
    P.y_stride = comps[0].stride;
    P.cb_stride = grey ? 0 : comps[1].stride, P.cr_stride = grey ? 0 : comps[2].stride;
    P.yuv_fs = yuv_fs;
    P.row_stride = im.row_stride, P.frame_stride = im.frame_stride, P.plane_stride = im.row_stride * (size_t)h;
    const unsigned lrows = sampling == HVC_YUV_420 ? (unsigned)(h + 1) >> 1 : (unsigned)h;
    const unsigned long long lanes = (unsigned long long)((w + 7) >> 3) * lrows;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {
        const int cnt = n_frames - f0 < 65535 ? n_frames - f0 : 65535;
        uint8_t *base = const_cast<uint8_t *>(d_yuv) + (size_t)f0 * yuv_fs;
        P.y = base + comps[0].plane_offset;
        P.cb = grey ? nullptr : base + comps[1].plane_offset;
        P.cr = grey ? nullptr : base + comps[2].plane_offset;
        P.rgb = d_rgb + (size_t)f0 * im.frame_stride;
        const size_t ca = sampling == HVC_YUV_444 ? 8 : 4;
        P.vec_y = ((uintptr_t)P.y | P.y_stride | yuv_fs) % 8 == 0;
        P.vec_c = !grey && ((uintptr_t)P.cb | (uintptr_t)P.cr | P.cb_stride | P.cr_stride | yuv_fs) % ca == 0;
        P.vec_rgb = ((uintptr_t)P.rgb | P.row_stride | P.frame_stride | (im.layout == HVC_RGB_PLANAR ? P.plane_stride : 0)) % 8 == 0;
        const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)cnt, 1);
        if (im.layout == HVC_RGB_PLANAR) launch_fancy<1>(sampling, grid, s, P);
        else launch_fancy<0>(sampling, grid, s, P);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
