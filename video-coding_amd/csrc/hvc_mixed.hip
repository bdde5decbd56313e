// hvc_mixed.hip -- the block stage over frames of DIFFERENT geometry and quantiser tables in one launch.
//
// k_decode_packed takes one DecodeParams: up to four planes and four tables in the kernarg segment, grid = tiles x frames.
// Here the decomposition comes from device memory: hvc_mixed_dev.h says how (work map, plane descriptor, one wavefront per
// work unit); a table entry (hvc_mixed_plan.h) holds the plane's quantiser in the forms the arithmetic wants.  No LDS.
//
// Per lane: K1's block -- eight 16-byte loads of the 128-byte record, the Chen-Wang row and column passes as the operation
// list of hvc_idct_spec.h (HVC_IDCT_PASS, expanded with this file's own primitives: operation for operation the form
// tests/test_guard_bounds.py proves under HVC_GUARD_D_PACKED / HVC_GUARD_RE / HVC_GUARD_Y), v_ashr_pk_u8_i32 for >> 14 /
// clip / + 128, eight 8-byte non-temporal row stores at the descriptor's stride.
//
// Blocks outside the proven int32 range -- a guard that trips, and every block of a plane whose table has an entry above
// 255 (a wave-uniform flag) -- are appended to the context's fix-up list as unit * 64 + lane, and k_decode_mixed_wide
// recomputes them in the model's arithmetic in int64, finding them through the same tables.  hvc_set_decode_kernel(ctx, 2)
// sends every block that way (MixedParams::all_wide).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_idct_spec.h"
#include "hvc_mixed.h"
#include "hvc_mixed_dev.h"

namespace hvc {
namespace {

// natural position -> zig-zag position (zigzag.ml:71-137)
__device__ constexpr int MZF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

typedef short m_short2 __attribute__((ext_vector_type(2)));
typedef unsigned short m_ushort2 __attribute__((ext_vector_type(2)));
typedef unsigned m_uint2 __attribute__((ext_vector_type(2)));

// pair.lo * k.lo + pair.hi * k.hi + ADD, the constant pair in an SGPR and the addend an inline constant (VOP3P)
template <int ADD>
__device__ __forceinline__ int m_dot2(unsigned pair, unsigned k) {
    static_assert(ADD == 0 || ADD == 4, "inline constants only");
    int d;
    if (ADD == 0)
        asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(pair), "s"(k));
    else
        asm("v_dot2_i32_i16 %0, %1, %2, 4" : "=v"(d) : "v"(pair), "s"(k));
    return d;
}
__device__ __forceinline__ int m_dot2v(unsigned pair, unsigned k, int add) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(pair), "s"(k), "v"(add));
    return d;
}
__device__ __forceinline__ int m_dot2_sat(unsigned pair, unsigned k, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(m_short2, pair), __builtin_bit_cast(m_short2, k), acc, true);
}
constexpr unsigned m_pk(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }

// raster coefficients PA (low half) and PB (high half) out of the 32 loaded dwords: one v_perm_b32
template <int PA, int PB>
__device__ __forceinline__ unsigned m_gather(const unsigned (&w)[32]) {
    constexpr int za = MZF[PA], zb = MZF[PB];
    constexpr int ha = za & 1, hb = zb & 1;
    constexpr unsigned sel = ((unsigned)(4 + 2 * hb + 1) << 24) | ((unsigned)(4 + 2 * hb) << 16) | ((unsigned)(2 * ha + 1) << 8) |
                             (unsigned)(2 * ha);
    return __builtin_amdgcn_perm(w[zb >> 1], w[za >> 1], sel);
}
__device__ __forceinline__ unsigned m_pk_mul(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, (m_ushort2)(__builtin_bit_cast(m_ushort2, a) * __builtin_bit_cast(m_ushort2, b)));
}

struct MGuard {
    int energy = 0;  // sum of squared quantised coefficients (saturating)
    int renergy = 0; // sum of squared saturated row outputs (saturating)
    int ymax = 0, ymin = 0;
    int k128 = HVC_ROW_ZADD, kcol = HVC_COL_ZADD;
    __device__ __forceinline__ void y2(int a, int b) { ymax = max(max(ymax, a), b); ymin = min(min(ymin, a), b); }
    __device__ __forceinline__ bool failed(int ethr) const {
        return (energy > ethr) | (renergy >= HVC_GUARD_RE) | (ymax > HVC_GUARD_Y) | (ymin < -HVC_GUARD_Y);
    }
};

// the statements of a pass = the expansion of HVC_IDCT_PASS (hvc_idct_spec.h)
#define HVC_MX_PASS(PASS)                                                                                              \
    HVC_IDCT_PASS(HVC_MX_ROT_##PASS, HVC_MX_ZDOT_##PASS, HVC_MX_ADD, HVC_MX_SUB, HVC_MX_GUARDY, HVC_MX_M181,           \
                  HVC_MX_OUTADD_##PASS, HVC_MX_OUTSUB_##PASS)
#define HVC_MX_ROT_ROW(d, P, klo, khi) const int d = m_dot2<HVC_ROW_RADD>(P, m_pk(klo, khi)) >> HVC_ROW_RSHIFT;
#define HVC_MX_ROT_COL(d, P, klo, khi) const int d = m_dot2<HVC_COL_RADD>(P, m_pk(klo, khi)) >> HVC_COL_RSHIFT;
#define HVC_MX_ZDOT_ROW(d, P, slo, shi) const int d = m_dot2v(P, m_pk((slo) * HVC_ROW_ZSCALE, (shi) * HVC_ROW_ZSCALE), g.k128);
#define HVC_MX_ZDOT_COL(d, P, slo, shi) const int d = m_dot2v(P, m_pk((slo) * HVC_COL_ZSCALE, (shi) * HVC_COL_ZSCALE), g.kcol);
#define HVC_MX_ADD(d, a, b) const int d = a + b;
#define HVC_MX_SUB(d, a, b) const int d = a - b;
#define HVC_MX_GUARDY(a, b) g.y2(a, b);
#define HVC_MX_M181(d, a) const int d = (__mul24(HVC_M181_MUL, a) + HVC_M181_ADD) >> HVC_M181_SHIFT;
#define HVC_MX_OUTADD_ROW(i, a, b) o[i] = (a + b) >> HVC_ROW_OSHIFT;
#define HVC_MX_OUTSUB_ROW(i, a, b) o[i] = (a - b) >> HVC_ROW_OSHIFT;
#define HVC_MX_OUTADD_COL(i, a, b) o[i] = (a + b) >> HVC_COL_OSHIFT;
#define HVC_MX_OUTSUB_COL(i, a, b) o[i] = (a - b) >> HVC_COL_OSHIFT;

// row pass (dct.ml:11-54) of row R; qp = the row's four operand pairs of the table entry, order A, B, C, Z
template <int R>
__device__ __forceinline__ void m_row(const unsigned (&w)[32], const unsigned *__restrict__ qp, int (&o)[8], MGuard &g) {
    const unsigned A = m_pk_mul(m_gather<8 * R + HVC_PAIR_A_LO, 8 * R + HVC_PAIR_A_HI>(w), qp[0]);
    const unsigned B = m_pk_mul(m_gather<8 * R + HVC_PAIR_B_LO, 8 * R + HVC_PAIR_B_HI>(w), qp[1]);
    const unsigned C = m_pk_mul(m_gather<8 * R + HVC_PAIR_C_LO, 8 * R + HVC_PAIR_C_HI>(w), qp[2]);
    const unsigned Z = m_pk_mul(m_gather<8 * R + HVC_PAIR_Z_LO, 8 * R + HVC_PAIR_Z_HI>(w), qp[3]);
    HVC_MX_PASS(ROW)
}
// two row outputs saturated into one column operand pair, with their share of the row-output energy
__device__ __forceinline__ unsigned m_pack_rows(int lo, int hi, MGuard &g) {
    const unsigned p = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(lo, hi));
    g.renergy = m_dot2_sat(p, p, g.renergy);
    return p;
}
// column pass (dct.ml:56-98): outputs unshifted, recon's + 128 rides in the rounding constant (HVC_COL_ZADD)
__device__ __forceinline__ void m_col(unsigned A, unsigned B, unsigned C, unsigned Z, int (&o)[8], MGuard &g) {
    HVC_MX_PASS(COL)
}
// sat_u8(a >> 14) | sat_u8(b >> 14) << 8 into one half of dst (the other half is kept: a 16-bit write)
template <int HALF>
__device__ __forceinline__ void m_pack2(unsigned &dst, int a, int b) {
    if (HALF == 0)
        asm("v_ashr_pk_u8_i32 %0, %1, %2, %3" : "=v"(dst) : "v"(a), "v"(b), "n"(HVC_COL_PACK_SHIFT));
    else
        asm("v_ashr_pk_u8_i32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(dst) : "v"(a), "v"(b), "n"(HVC_COL_PACK_SHIFT));
}
__device__ __forceinline__ void m_store_row(uint8_t *p, unsigned lo, unsigned hi) {
    m_uint2 t = {lo, hi};
    __builtin_nontemporal_store(t, reinterpret_cast<m_uint2 *>(p));
}

// One block per lane, spelled inline in the kernel (hvc_kernels.hip HVC_DECODE_BLOCK_PACKED says why a macro): the loaded
// dwords W -> the block's 8 rows as byte-packed dword pairs OUT[8][2]; QP = the table entry's 32 operand pairs.
#define HVC_MX_DECODE_BLOCK(W, QP, OUT, G)                                                                 \
    do {                                                                                                   \
        _Pragma("unroll") for (int d = 0; d < 32; d++) (G).energy = m_dot2_sat((W)[d], (W)[d], (G).energy); \
        unsigned cA[8], cB[8], cC[8], cZ[8];                                                               \
        {                                                                                                  \
            int ra[8], rb[8];                                                                              \
            m_row<HVC_PAIR_A_LO>((W), (QP) + 4 * HVC_PAIR_A_LO, ra, (G));                                  \
            m_row<HVC_PAIR_A_HI>((W), (QP) + 4 * HVC_PAIR_A_HI, rb, (G));                                  \
            _Pragma("unroll") for (int c = 0; c < 8; c++) cA[c] = m_pack_rows(ra[c], rb[c], (G));          \
            m_row<HVC_PAIR_B_LO>((W), (QP) + 4 * HVC_PAIR_B_LO, ra, (G));                                  \
            m_row<HVC_PAIR_B_HI>((W), (QP) + 4 * HVC_PAIR_B_HI, rb, (G));                                  \
            _Pragma("unroll") for (int c = 0; c < 8; c++) cB[c] = m_pack_rows(ra[c], rb[c], (G));          \
            m_row<HVC_PAIR_C_LO>((W), (QP) + 4 * HVC_PAIR_C_LO, ra, (G));                                  \
            m_row<HVC_PAIR_C_HI>((W), (QP) + 4 * HVC_PAIR_C_HI, rb, (G));                                  \
            _Pragma("unroll") for (int c = 0; c < 8; c++) cC[c] = m_pack_rows(ra[c], rb[c], (G));          \
            m_row<HVC_PAIR_Z_LO>((W), (QP) + 4 * HVC_PAIR_Z_LO, ra, (G));                                  \
            m_row<HVC_PAIR_Z_HI>((W), (QP) + 4 * HVC_PAIR_Z_HI, rb, (G));                                  \
            _Pragma("unroll") for (int c = 0; c < 8; c++) cZ[c] = m_pack_rows(ra[c], rb[c], (G));          \
        }                                                                                                  \
        _Pragma("unroll") for (int c = 0; c < 8; c += 2) {                                                 \
            int ca[8], cb[8];                                                                              \
            m_col(cA[c], cB[c], cC[c], cZ[c], ca, (G));                                                    \
            m_col(cA[c + 1], cB[c + 1], cC[c + 1], cZ[c + 1], cb, (G));                                    \
            _Pragma("unroll") for (int j = 0; j < 8; j++) {                                                \
                if ((c & 2) == 0)                                                                          \
                    m_pack2<0>((OUT)[j][c >> 2], ca[j], cb[j]);                                            \
                else                                                                                       \
                    m_pack2<1>((OUT)[j][c >> 2], ca[j], cb[j]);                                            \
            }                                                                                              \
        }                                                                                                  \
    } while (0)

__global__ __launch_bounds__(HVC_MIXED_LANES, 4) void k_decode_mixed(MixedParams P) {
    const MixedWave W = mixed_wave_xcd(P.xcd_map, P.xcd_magic);
    if (W.unit >= P.n_units) return;
    const MixedPlaneK &K = P.planes[P.map[W.unit]];
    const MixedTableK &T = P.tables[K.table];
    const auto B = mixed_block<8>(K, W.unit, W.lane, P.coefs, P.pixels);
    bool flag = B.active;
    if (!(P.all_wide | T.wide)) { // wave-uniform
        unsigned w[32];
        mixed_load_record(B.rec, w);
        MGuard g;
        unsigned out[8][2];
        const unsigned *__restrict__ qp = T.qpair;
        HVC_MX_DECODE_BLOCK(w, qp, out, g);
        const bool bad = g.failed(T.ethr_packed);
        if (B.active && !bad) {
#pragma unroll
            for (int j = 0; j < 8; j++) m_store_row(B.pix + (size_t)j * B.stride, out[j][0], out[j][1]);
        }
        flag = B.active && bad;
    }
    const unsigned long long m = __ballot(flag);
    if (m) {
        unsigned base = 0;
        if (W.lane == 0) base = atomicAdd(P.fix_count, (unsigned)__popcll(m));
        base = __shfl(base, 0);
        if (flag) P.fix_list[base + (unsigned)__popcll(m & ((1ull << W.lane) - 1ull))] = W.unit * HVC_MIXED_UNIT + (unsigned)W.lane;
    }
}

// The model's pass as it writes it (dct.ml:11-98) in 64 bits.  OCaml's int has 63 bits; for an int16 coefficient times a
// 16-bit table entry no value of either pass reaches 2^57 (tests/test_guard_bounds.py::
// test_wide_kernel_without_the_63_bit_reading), so the 63-bit reading is the identity and `asr` is one 64-bit shift.
// Sums and products are kept unsigned (modulo 2^64); a value is read as signed where the model shifts or compares it.
template <bool COL>
__device__ __forceinline__ void m_idct8_wide(const uint64_t (&b)[8], int64_t (&o)[8]) {
    typedef uint64_t u64;
    constexpr u64 w1 = HVC_W1, w2 = HVC_W2, w3 = HVC_W3, w5 = HVC_W5, w6 = HVC_W6, w7 = HVC_W7;
    constexpr u64 R = COL ? 4 : 0;
    constexpr int RS = COL ? 3 : 0, S = COL ? 14 : 8;
    auto asr = [](u64 x, int s) { return (u64)((int64_t)x >> s); };
    u64 x0 = COL ? b[0] * 256u + 8192u : b[0] * 2048u + 128u;
    u64 x1 = COL ? b[4] * 256u : b[4] * 2048u;
    u64 x2 = b[6], x3 = b[2], x4 = b[1], x5 = b[7], x6 = b[5], x7 = b[3];
    u64 x8 = w7 * (x4 + x5) + R;
    x4 = asr(x8 + (w1 - w7) * x4, RS);
    x5 = asr(x8 - (w1 + w7) * x5, RS);
    x8 = w3 * (x6 + x7) + R;
    x6 = asr(x8 - (w3 - w5) * x6, RS);
    x7 = asr(x8 - (w3 + w5) * x7, RS);
    x8 = x0 + x1;
    x0 = x0 - x1;
    x1 = w6 * (x3 + x2) + R;
    x2 = asr(x1 - (w2 + w6) * x2, RS);
    x3 = asr(x1 + (w2 - w6) * x3, RS);
    x1 = x4 + x6;
    x4 = x4 - x6;
    x6 = x5 + x7;
    x5 = x5 - x7;
    x7 = x8 + x3;
    x8 = x8 - x3;
    x3 = x0 + x2;
    x0 = x0 - x2;
    x2 = asr(181u * (x4 + x5) + 128u, 8);
    x4 = asr(181u * (x4 - x5) + 128u, 8);
    o[0] = (int64_t)asr(x7 + x1, S);
    o[1] = (int64_t)asr(x3 + x2, S);
    o[2] = (int64_t)asr(x0 + x4, S);
    o[3] = (int64_t)asr(x8 + x6, S);
    o[4] = (int64_t)asr(x8 - x6, S);
    o[5] = (int64_t)asr(x0 - x4, S);
    o[6] = (int64_t)asr(x3 - x2, S);
    o[7] = (int64_t)asr(x7 - x1, S);
}

// decoder.ml:142-149 (dequantise + inverse zig-zag), dct.ml:11-107 (rows, then columns), decoder.ml:213-224 (clip, + 128)
__device__ __forceinline__ void m_block_wide(const unsigned (&w)[32], const int *__restrict__ q, unsigned (&out)[8][2]) {
    int64_t v[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        uint64_t in[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int zz = MZF[8 * r + i];
            const int c = (zz & 1) ? (int)w[zz >> 1] >> 16 : (int)(short)(w[zz >> 1] & 0xffffu);
            in[i] = (uint64_t)((int64_t)c * (int64_t)q[zz]);
        }
        int64_t o[8];
        m_idct8_wide<false>(in, o);
#pragma unroll
        for (int i = 0; i < 8; i++) v[8 * r + i] = o[i];
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[j][0] = out[j][1] = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        uint64_t in[8];
#pragma unroll
        for (int j = 0; j < 8; j++) in[j] = (uint64_t)v[8 * j + c];
        int64_t o[8];
        m_idct8_wide<true>(in, o);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t y = (uint64_t)o[j] + 128u;
            const unsigned px = y <= 255u ? (unsigned)y : ((int64_t)y < 0 ? 0u : 255u);
            out[j][c >> 2] |= px << (8 * (c & 3));
        }
    }
}

// The listed blocks, one per lane, in a grid-stride loop over the (normally empty) list: a fixed grid, since the list's
// length is known on the device only.  An id that does not name a block of THIS launch's tables never becomes an address.
#define HVC_MIXED_WIDE_WGS 512
#define HVC_MIXED_WIDE_LANES 256
__global__ __launch_bounds__(HVC_MIXED_WIDE_LANES) void k_decode_mixed_wide(MixedParams P) {
    const unsigned long long n = (unsigned long long)*P.fix_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) { // the counters alternate between launches, the call's total adds up (k_decode_wide)
        if (P.fix_count_next) *P.fix_count_next = 0;
        if (P.wide_total) *P.wide_total = P.wide_first ? n : *P.wide_total + n;
    }
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned id = P.fix_list[i];
        const unsigned unit = id / HVC_MIXED_UNIT, lane = id % HVC_MIXED_UNIT;
        if (unit >= P.n_units) continue;
        const MixedPlaneK K = P.planes[P.map[unit]];
        if (unit < K.unit0) continue;
        const unsigned long long b = (unsigned long long)(unit - K.unit0) * HVC_MIXED_UNIT + lane;
        if (b >= (unsigned long long)K.nblk) continue;
        const auto br = mixed_block_at<8>(K, (int)b, P.coefs, P.pixels);
        unsigned w[32], out[8][2];
        mixed_load_record(br.rec, w);
        m_block_wide(w, P.tables[K.table].qt, out);
#pragma unroll
        for (int j = 0; j < 8; j++) m_store_row(br.pix + (size_t)j * br.stride, out[j][0], out[j][1]);
    }
}

} // namespace

hipError_t launch_decode_mixed(const MixedParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (P.n_units == 0) return hipSuccess;
    const hipError_t e = mixed_launch_xcd(k_decode_mixed, P, s, k0, k1);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode_mixed_wide, dim3(HVC_MIXED_WIDE_WGS), dim3(HVC_MIXED_WIDE_LANES), 0, s, P);
    return hipGetLastError();
}

} // namespace hvc
