// hvc_hardcaml.hip -- gfx950 kernel of the Hardcaml RTL decoder's block datapath (hvc_set_arithmetic HVC_ARITH_HARDCAML):
// 12-bit dequantisation, the 12-bit fixed-point matrix IDCT of jpeg/hardcaml/src/dct.ml, saturation, level shift -- bit
// exact to the RTL for every int16 record and every 16-bit table (hvc_hardcaml_spec.h states the arithmetic and the
// schedule; tests/test_hardcaml_twin.py proves the int32 bounds over it).
//
// Mapping: k_decode_packed's -- one 8x8 block per lane, a tile of HVC_TILE consecutive blocks of one plane per
// workgroup, grid = tiles x frames, workgroups -> (frame, tile) by xcd_work.  A lane loads its 128-byte record (8 x 16 B),
// keeps all 64 values in VGPRs and stores 8 rows of 8 bytes: the twin moves the model path's bytes.
//   dequantise  v_pk_mul_lo_u16 per record dword (two zig-zag coefficients) with the pre-shifted table pair: 16 x the
//               12-bit product as int16, exact (hvc_hardcaml_spec.h)
//   pass 1      the column operand pairs (x0,x2) (x4,x6) (x1,x3) (x5,x7) gathered by v_perm_b32 (the inverse zig-zag is
//               compile-time), then v_dot2_i32_i16 against ROM pairs: 16 dot2 per column for 8 outputs (butterfly)
//   pass 2      T needs 18 bits: v_mul_i32_i24 / v_mad_i32_i24 against ROM constants, 32 per row for 8 outputs
//   output      RND + level shift in one v_add3, shift and saturation by v_ashr_pk_u8_i32
// Why not MFMA: pass 1's sums reach 2^24.4, beyond f32's exact integers, and the i8 form would need the 12-bit operands
// split; the VALU form is exact in int32 with no fix-up path, and its ~1 060 instructions per block stay below the
// memory time of the block's 192 bytes.
//
// k_hardcaml_encode, the encoder twin (hvc_set_encode_arithmetic HVC_ARITH_HARDCAML): the RTL encoder's forward DCT
// (Dct_config) and reciprocal quantiser, bit exact for every 8-bit pixel and every table in 1..255
// (hvc_hardcaml_fwd_spec.h; tests/test_hardcaml_encoder_twin.py proves its bounds).  Mapping: k_encode's -- one block per
// lane, xcd_work, 8-byte non-temporal row loads, the wave's records transposed through LDS into 1 KiB non-temporal runs.
//   pass 1      v_perm_b32 gathers two rows' pixel bytes of a column as an int16 pair, v_pk_add_u16 / v_pk_sub_u16 form
//               the butterfly (the level shift rides in the accumulator), 2 v_dot2_i32_i16 per output; RND without its
//               final shift: bytes 1-2 of the rounded sum ARE T, and one v_perm_b32 packs two of them
//   pass 2      the same butterfly on the int16 pairs of T, 2 v_dot2_i32_i16 per output, RND by 16
//   quantiser   v_mul_i32_i24 by the reciprocal << 4 and one rounding add: the quotient is the product's high half, and
//               one v_perm_b32 packs two in zig-zag order
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_hardcaml.h"
#include "hvc_hardcaml_fwd_spec.h"
#include "hvc_hardcaml_spec.h"

namespace hvc {

namespace {

constexpr int ROM[8][8] = {{HVC_HC_ROM_R0}, {HVC_HC_ROM_R1}, {HVC_HC_ROM_R2}, {HVC_HC_ROM_R3},
                           {HVC_HC_ROM_R4}, {HVC_HC_ROM_R5}, {HVC_HC_ROM_R6}, {HVC_HC_ROM_R7}};

constexpr bool rom_is_symmetric() {
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 8; k++)
            if (ROM[7 - r][k] != ((k & 1) ? -ROM[r][k] : ROM[r][k])) return false;
    return true;
}
static_assert(rom_is_symmetric(), "the butterfly needs C[7-r][k] = (-1)^k C[r][k]");

// jpeg/model/src/zigzag.ml:71-137  forward[raster] = zz
constexpr unsigned char ZF[64] = {
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

constexpr unsigned pk16(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }

// v_perm_b32 selector: low half = half (a & 1) of source 1, high half = half (b & 1) of source 0
constexpr unsigned perm_sel(int a, int b) {
    const unsigned lo = 2u * (unsigned)(a & 1), hi = 4u + 2u * (unsigned)(b & 1);
    return lo | (lo + 1u) << 8 | hi << 16 | (hi + 1u) << 24;
}

} // namespace

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}

// v_pk_mul_lo_u16: the low 16 bits of both halves' products
__device__ __forceinline__ unsigned pk_mul_lo(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b));
}

// round half away from zero by P bits, ADD added in the same instruction (a multiple of 2^P)
template <int P, int ADD>
__device__ __forceinline__ int rnd(int v) {
    return (v + ((1 << (P - 1)) + ADD) + (v >> 31)) >> P;
}

// pixel bytes of a, b, c, d: (v >> 16) saturated to [0, 255] (v_ashr_pk_u8_i32)
__device__ __forceinline__ unsigned ashr16_sat_pack4(int a, int b, int c, int d) {
    unsigned r;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, 16" : "=v"(r) : "v"(a), "v"(b));
    asm("v_ashr_pk_u8_i32 %0, %1, %2, 16 op_sel:[0,0,0,1]" : "+v"(r) : "v"(c), "v"(d));
    return r;
}

__device__ __forceinline__ void store_row8_nt(uint8_t *p, unsigned lo, unsigned hi) {
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    u2v t = {lo, hi};
    __builtin_nontemporal_store(t, reinterpret_cast<u2v *>(p));
}

// One block: record dwords w (zig-zag pairs), table pairs qq -> out[row][0..1] = the row's 8 pixels.
__device__ __forceinline__ void hardcaml_block(const unsigned (&w)[32], const unsigned *__restrict__ qq, unsigned (&out)[8][2]) {
    unsigned d[32];
#pragma unroll
    for (int i = 0; i < 32; i++) d[i] = pk_mul_lo(w[i], qq[i]);

    int T[8][8]; // T[x][y], 4 fractional bits
#pragma unroll
    for (int y = 0; y < 8; y++) {
        // operand pairs of column y: raster (8k + y) sits at zig-zag ZF[8k + y] = half (zz & 1) of dword zz / 2
        unsigned P[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            constexpr int KS[4][2] = {{0, 2}, {4, 6}, {1, 3}, {5, 7}};
            const int a = ZF[8 * KS[j][0] + y], b = ZF[8 * KS[j][1] + y];
            P[j] = __builtin_amdgcn_perm(d[b >> 1], d[a >> 1], perm_sel(a, b));
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int e = dot2(P[1], pk16(ROM[r][4], ROM[r][6]), dot2(P[0], pk16(ROM[r][0], ROM[r][2]), 0));
            const int o = dot2(P[3], pk16(ROM[r][5], ROM[r][7]), dot2(P[2], pk16(ROM[r][1], ROM[r][3]), 0));
            T[r][y] = rnd<HVC_HC_P1_SHIFT, 0>(e + o);
            T[7 - r][y] = rnd<HVC_HC_P1_SHIFT, 0>(e - o);
        }
    }
#pragma unroll
    for (int x = 0; x < 8; x++) {
        int R[8];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int e = __mul24(T[x][0], ROM[r][0]) + __mul24(T[x][2], ROM[r][2]) + __mul24(T[x][4], ROM[r][4]) +
                          __mul24(T[x][6], ROM[r][6]);
            const int o = __mul24(T[x][1], ROM[r][1]) + __mul24(T[x][3], ROM[r][3]) + __mul24(T[x][5], ROM[r][5]) +
                          __mul24(T[x][7], ROM[r][7]);
            constexpr int L = HVC_HC_LEVEL << HVC_HC_P2_SHIFT;
            R[r] = e + o + ((1 << (HVC_HC_P2_SHIFT - 1)) + L);
            R[7 - r] = e - o + ((1 << (HVC_HC_P2_SHIFT - 1)) + L);
            R[r] += (e + o) >> 31;
            R[7 - r] += (e - o) >> 31;
        }
        out[x][0] = ashr16_sat_pack4(R[0], R[1], R[2], R[3]);
        out[x][1] = ashr16_sat_pack4(R[4], R[5], R[6], R[7]);
    }
}

struct HcRef {
    size_t coef_idx, pix_idx, stride;
    int qtab, comp, b;
};

__device__ __forceinline__ bool hc_locate(const HardcamlParams &P, int frame, int tile, int lane, HcRef &br) {
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && tile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    int b = (tile - K.tile0) * HVC_TILE + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1;
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    br.coef_idx = (size_t)frame * P.coef_fs + K.coef_off + (size_t)b * 64;
    br.pix_idx = (size_t)frame * P.pixel_fs + K.plane_off + (size_t)by * 8 * K.stride + (size_t)bx * 8;
    br.stride = K.stride;
    br.qtab = K.qtab;
    br.comp = c;
    br.b = b;
    return active;
}

__device__ __forceinline__ void load_record(const int16_t *cf, unsigned (&w)[32]) {
    const uint4 *src = reinterpret_cast<const uint4 *>(cf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 t = src[j];
        w[4 * j + 0] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
    }
}

__device__ __forceinline__ unsigned with_dc(unsigned w0, unsigned dc) { return (w0 & 0xffff0000u) | (dc & 0xffffu); }

// largest |a - b| over the bytes of two dwords
__device__ __forceinline__ unsigned max_abs_diff4(unsigned a, unsigned b, unsigned m) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = (int)((a >> (8 * k)) & 0xffu), y = (int)((b >> (8 * k)) & 0xffu);
        m = max(m, (unsigned)abs(x - y));
    }
    return m;
}

// DCP: the DC comes from P.dc_plane; CMP: the divergence form (P.pixels holds the model's pixels, P.diff gets a byte
// per block)
template <bool DCP, bool CMP>
__global__ __launch_bounds__(HVC_TILE) void k_hardcaml(HardcamlParams P) {
    HcRef br;
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    const bool active = hc_locate(P, (int)wframe, (int)wtile, lane, br);
    unsigned w[32], out[8][2];
    load_record(P.coefs + br.coef_idx, w);
    if (DCP) w[0] = with_dc(w[0], (unsigned short)P.dc_plane[(size_t)wframe * P.dc_fs + ((br.coef_idx - (size_t)wframe * P.coef_fs) >> 6)]);
    hardcaml_block(w, P.qq + br.qtab * 32, out);
    if (!active) return;
    if (CMP) {
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            typedef unsigned u2v __attribute__((ext_vector_type(2)));
            const u2v ref = *reinterpret_cast<const u2v *>(P.pixels + br.pix_idx + (size_t)j * br.stride);
            m = max_abs_diff4(out[j][0], ref.x, m);
            m = max_abs_diff4(out[j][1], ref.y, m);
        }
        P.diff[(size_t)wframe * P.diff_fs + (size_t)P.blk0[br.comp] + (size_t)br.b] = (uint8_t)m;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) store_row8_nt(P.pixels + br.pix_idx + (size_t)j * br.stride, out[j][0], out[j][1]);
    }
}

// The listed blocks, one per lane of a small grid-stride loop, coefficient 0 replaced by the true DC (only its low 12
// bits matter to the RTL: the record's saturated value would not do).
__global__ __launch_bounds__(64) void k_hardcaml_dcfix(HardcamlParams P, const unsigned *count, const unsigned *list,
                                                        const long long *dcs) {
    const unsigned n = *count;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned id = list[i];
        const int lane = (int)(id % HVC_TILE);
        const unsigned t = id / HVC_TILE;
        const int tile = (int)(t % (unsigned)P.tiles_per_frame);
        const int frame = (int)(t / (unsigned)P.tiles_per_frame);
        if (frame >= P.n_frames) continue; // an id from another geometry must never turn into an address
        HcRef br;
        if (!hc_locate(P, frame, tile, lane, br)) continue;
        unsigned w[32], out[8][2];
        load_record(P.coefs + br.coef_idx, w);
        w[0] = with_dc(w[0], (unsigned)(unsigned long long)dcs[i]);
        hardcaml_block(w, P.qq + br.qtab * 32, out);
#pragma unroll
        for (int j = 0; j < 8; j++) store_row8_nt(P.pixels + br.pix_idx + (size_t)j * br.stride, out[j][0], out[j][1]);
    }
}

void prepare_hardcaml_tables(const uint16_t *qtabs, int n_qtabs, unsigned *qq) {
    for (int t = 0; t < n_qtabs; t++)
        for (int i = 0; i < 32; i++) {
            const unsigned lo = (qtabs[t * 64 + 2 * i] & ((1u << HVC_HC_Q_BITS) - 1)) << HVC_HC_QSHIFT;
            const unsigned hi = (qtabs[t * 64 + 2 * i + 1] & ((1u << HVC_HC_Q_BITS) - 1)) << HVC_HC_QSHIFT;
            qq[t * 32 + i] = lo | hi << 16;
        }
}

hipError_t launch_hardcaml(const HardcamlParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    HardcamlParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic);
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (P.diff) {
        if (P.dc_plane) hipLaunchKernelGGL((k_hardcaml<true, true>), grid, dim3(HVC_TILE), 0, s, Q);
        else hipLaunchKernelGGL((k_hardcaml<false, true>), grid, dim3(HVC_TILE), 0, s, Q);
    } else {
        if (P.dc_plane) hipLaunchKernelGGL((k_hardcaml<true, false>), grid, dim3(HVC_TILE), 0, s, Q);
        else hipLaunchKernelGGL((k_hardcaml<false, false>), grid, dim3(HVC_TILE), 0, s, Q);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

hipError_t launch_hardcaml_dcfix(const HardcamlParams &P, const unsigned *count, const unsigned *ids, const long long *dcs,
                                 hipStream_t s) {
    hipLaunchKernelGGL(k_hardcaml_dcfix, dim3(64), dim3(64), 0, s, P, count, ids, dcs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The encoder twin (hvc_hardcaml_fwd_spec.h)

namespace {

constexpr int FROM[8][8] = {{HVC_HCE_ROM_R0}, {HVC_HCE_ROM_R1}, {HVC_HCE_ROM_R2}, {HVC_HCE_ROM_R3},
                            {HVC_HCE_ROM_R4}, {HVC_HCE_ROM_R5}, {HVC_HCE_ROM_R6}, {HVC_HCE_ROM_R7}};

constexpr bool fwd_rom_is_symmetric() {
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 4; x++)
            if (FROM[u][7 - x] != ((u & 1) ? -FROM[u][x] : FROM[u][x])) return false;
    return true;
}
static_assert(fwd_rom_is_symmetric(), "the butterfly needs C[u][7-x] = (-1)^u C[u][x]");
static_assert(HVC_HCE_P1_SHIFT == 8, "pass 1: T is bytes 1-2 of the rounded sum");
static_assert(HVC_HCE_QZ_SHIFT == 16, "quantiser: q is the high half of the rounded product");

// pass 1's accumulator: the level shift of the sums p + p' = X + X' + 2 LEVEL (the differences do not see it)
constexpr int fwd_level_acc(int u) {
    return (u & 1) ? 0 : -2 * HVC_HCE_LEVEL * (FROM[u][0] + FROM[u][1] + FROM[u][2] + FROM[u][3]);
}

// jpeg/model/src/zigzag.ml:3-69  inverse[zz] = raster
constexpr unsigned char ZI[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// v_perm_b32 selector: low half = byte b of source 1 zero-extended, high half = byte b of source 0 zero-extended
constexpr unsigned byte_pair_sel(int b) { return (unsigned)b | 0x0cu << 8 | (4u + (unsigned)b) << 16 | 0x0cu << 24; }
constexpr unsigned SEL_T = 0x06050201u; // bytes 1-2 of source 1 | bytes 1-2 of source 0 << 16
constexpr unsigned SEL_Q = 0x07060302u; // the high halves: source 1's low, source 0's high

} // namespace

__device__ __forceinline__ unsigned pk_add16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ unsigned pk_sub16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}

// One block: pixel rows px[x] (8 bytes each) -> the record's 32 dwords (zig-zag int16 pairs).
__device__ __forceinline__ void hardcaml_encode_block(const unsigned (&px)[8][2], const int *__restrict__ qr,
                                                      unsigned (&out)[32]) {
    int w[8][8]; // w[u][y] = T[u][y] << 8 + the rounding remainder (hvc_hardcaml_fwd_spec.h)
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const int D = y >> 2;
        const unsigned sel = byte_pair_sel(y & 3);
        const unsigned a0 = __builtin_amdgcn_perm(px[1][D], px[0][D], sel); // (p0, p1)
        const unsigned b0 = __builtin_amdgcn_perm(px[6][D], px[7][D], sel); // (p7, p6)
        const unsigned a1 = __builtin_amdgcn_perm(px[3][D], px[2][D], sel); // (p2, p3)
        const unsigned b1 = __builtin_amdgcn_perm(px[4][D], px[5][D], sel); // (p5, p4)
        const unsigned S0 = pk_add16(a0, b0), S1 = pk_add16(a1, b1), D0 = pk_sub16(a0, b0), D1 = pk_sub16(a1, b1);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned X0 = (u & 1) ? D0 : S0, X1 = (u & 1) ? D1 : S1;
            const int v = dot2(X1, pk16(FROM[u][2], FROM[u][3]), dot2(X0, pk16(FROM[u][0], FROM[u][1]), fwd_level_acc(u)));
            w[u][y] = v + (1 << (HVC_HCE_P1_SHIFT - 1)) + (v >> 31);
        }
    }
    int z[64]; // z[8u + v] = q << 16 + the rounding remainder, natural order
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const unsigned P0 = __builtin_amdgcn_perm(w[u][1], w[u][0], SEL_T); // (T0, T1)
        const unsigned P1 = __builtin_amdgcn_perm(w[u][3], w[u][2], SEL_T); // (T2, T3)
        const unsigned Q0 = __builtin_amdgcn_perm(w[u][6], w[u][7], SEL_T); // (T7, T6)
        const unsigned Q1 = __builtin_amdgcn_perm(w[u][4], w[u][5], SEL_T); // (T5, T4)
        const unsigned E0 = pk_add16(P0, Q0), E1 = pk_add16(P1, Q1), O0 = pk_sub16(P0, Q0), O1 = pk_sub16(P1, Q1);
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const unsigned X0 = (v & 1) ? O0 : E0, X1 = (v & 1) ? O1 : E1;
            const int s = dot2(X1, pk16(FROM[v][2], FROM[v][3]), dot2(X0, pk16(FROM[v][0], FROM[v][1]), 0));
            const int R = rnd<HVC_HCE_P2_SHIFT, 0>(s);
            z[8 * u + v] = __mul24(R, qr[8 * u + v]) + (1 << (HVC_HCE_QZ_SHIFT - 1)) + (R >> 31);
        }
    }
#pragma unroll
    for (int i = 0; i < 32; i++) out[i] = __builtin_amdgcn_perm(z[ZI[2 * i + 1]], z[ZI[2 * i]], SEL_Q);
}

// largest |a - b| over the int16 halves of two dwords
__device__ __forceinline__ unsigned max_abs_diff_i16x2(unsigned a, unsigned b, unsigned m) {
    const int alo = (int)(short)(a & 0xffffu), ahi = (int)a >> 16;
    const int blo = (int)(short)(b & 0xffffu), bhi = (int)b >> 16;
    return max(m, max((unsigned)abs(alo - blo), (unsigned)abs(ahi - bhi)));
}

// CMP: the divergence form (P.coefs holds the model's records, P.diff gets min(255, max |model - rtl|) per block)
template <bool CMP>
__global__ __launch_bounds__(HVC_TILE) void k_hardcaml_encode(HardcamlEncodeParams P) {
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && (int)wtile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    const int tile_b0 = ((int)wtile - K.tile0) * HVC_TILE;
    int b = tile_b0 + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1; // (inactive lanes read the plane's last block and store nothing)
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const uint8_t *pix = P.pixels + (size_t)wframe * P.pixel_fs + K.plane_off + (size_t)by * 8 * K.stride + (size_t)bx * 8;
    const size_t plane_coef_idx = (size_t)wframe * P.coef_fs + K.coef_off;
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    unsigned px[8][2];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u2v t = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(pix + (size_t)j * K.stride));
        px[j][0] = t.x;
        px[j][1] = t.y;
    }
    unsigned out[32];
    hardcaml_encode_block(px, P.qr + K.qtab * 64, out);
    if (CMP) {
        unsigned ref[32];
        load_record(P.coefs + plane_coef_idx + (size_t)b * 64, ref);
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < 32; i++) m = max_abs_diff_i16x2(ref[i], out[i], m);
        if (active) P.diff[(size_t)wframe * P.diff_fs + (size_t)P.blk0[c] + (size_t)b] = (uint8_t)min(m, 255u);
        return;
    }
    // k_encode's store: the wave's 64 records through LDS (XOR-swizzled 16-byte slots, conflict-free both ways), out as
    // whole 1 KiB runs (lane i of store j writes byte 1024 j + 16 i of the wave's coefficient run)
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    __shared__ u4v lds[HVC_TILE / 64][512];
    const int wv = lane >> 6, l = lane & 63;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u4v t = {out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]};
        lds[wv][l * 8 + (j ^ (l & 7))] = t;
    }
    // (wave-private LDS region: the wave's own ds ops are ordered, no barrier needed)
    const int wave_b0 = tile_b0 + (lane & ~63);
    u4v *dst = reinterpret_cast<u4v *>(P.coefs + plane_coef_idx + (size_t)wave_b0 * 64);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int blk = 8 * j + (l >> 3), ch = l & 7;
        const u4v t = lds[wv][blk * 8 + (ch ^ (blk & 7))];
        if (wave_b0 + blk < K.nblk) __builtin_nontemporal_store(t, dst + j * 64 + l);
    }
}

void prepare_hardcaml_encode_tables(const uint16_t *qtabs, int n_qtabs, int *qr) {
    for (int t = 0; t < n_qtabs; t++)
        for (int k = 0; k < 64; k++) {
            const int q = qtabs[t * 64 + ZF[k]];
            qr[t * 64 + k] = q > 0 ? (HVC_HCE_QR_NUM / q) << HVC_HCE_QR_SCALE : 0;
        }
}

hipError_t launch_hardcaml_encode(const HardcamlEncodeParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    HardcamlEncodeParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic);
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (P.diff) hipLaunchKernelGGL(k_hardcaml_encode<true>, grid, dim3(HVC_TILE), 0, s, Q);
    else hipLaunchKernelGGL(k_hardcaml_encode<false>, grid, dim3(HVC_TILE), 0, s, Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc
