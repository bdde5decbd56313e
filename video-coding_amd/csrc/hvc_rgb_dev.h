// hvc_rgb_dev.h -- device side of the RGB colour pass (internal): what k_ycc_to_rgb / k_rgb_to_ycc (hvc_rgb.hip, one geometry
// per launch) and k_ycc_to_rgb_mixed / k_rgb_to_ycc_mixed (hvc_mixed_rgb.hip, geometry per wavefront from device memory) share.  The definition of
// every byte is the one at the top of hvc_rgb.hip.  Everything here has internal linkage: include it in a .hip file only.
#ifndef HVC_RGB_DEV_H
#define HVC_RGB_DEV_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

struct RgbOp {
    uint8_t *y, *cb, *cr; // frame 0's planes (source: k_ycc_to_rgb, destination: k_rgb_to_ycc)
    uint8_t *rgb;
    size_t y_stride, cb_stride, cr_stride, yuv_fs; // bytes per row of each plane, from frame to frame
    size_t row_stride, plane_stride, frame_stride; // of the RGB image (plane_stride: planar layout)
    int w, h, cw, ch;                              // frame size; valid chroma samples (k_ycc_to_rgb: where the neighbours clamp)
    int vec_y, vec_c, vec_rgb;                     // bases and strides allow the 8 / 4-byte forms
};

typedef unsigned u2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned avg2x4(unsigned a, unsigned b) { // (a + b + 1) >> 1 on four bytes (planar_444.ml:4-8)
    return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu);
}
// avg4 on four samples at once (tests/test_guard_bounds.py::test_avg4_by_lerp_identity, as in hvc_yuv.hip)
__device__ __forceinline__ unsigned avg4x4(unsigned a, unsigned b, unsigned c, unsigned d) {
    return __builtin_amdgcn_lerp(__builtin_amdgcn_lerp(a, b, 0x01010101u), __builtin_amdgcn_lerp(c, d, 0u), ~(a ^ b) | (c ^ d));
}
__device__ __forceinline__ unsigned pairsum(unsigned x) { return (x & 0x00ff00ffu) + ((x >> 8) & 0x00ff00ffu); }
__device__ __forceinline__ unsigned pack_even(unsigned lo, unsigned hi) { // bytes 0 and 2 of lo, then of hi
    return __builtin_amdgcn_perm(hi, lo, 0x06040200u);
}

// samples x0 .. x0 + 7 of a row of n valid samples (columns past the last one repeat it: never read, or never used)
__device__ __forceinline__ void load8(const uint8_t *row, int x0, int n, bool vec, unsigned &lo, unsigned &hi) {
    if (vec) {
        const u2v v = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(row + x0));
        lo = v.x, hi = v.y;
        return;
    }
    lo = hi = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        lo |= (unsigned)row[min(x0 + i, n - 1)] << (8 * i);
        hi |= (unsigned)row[min(x0 + 4 + i, n - 1)] << (8 * i);
    }
}
// samples c0 .. c0 + 3 of a chroma row of n valid samples and every one's right neighbour (the last column's: itself)
__device__ __forceinline__ void load4n(const uint8_t *row, int c0, int n, bool vec, unsigned &a, unsigned &nb) {
    if (vec) {
        a = *reinterpret_cast<const unsigned *>(row + c0);
    } else {
        a = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) a |= (unsigned)row[min(c0 + i, n - 1)] << (8 * i);
    }
    nb = (a >> 8) | ((unsigned)row[min(c0 + 4, n - 1)] << 24);
}
// (e0 o0 e1 o1) (e2 o2 e3 o3): the even and odd columns of a supersampled row, side by side
__device__ __forceinline__ void interleave(unsigned even, unsigned odd, unsigned &lo, unsigned &hi) {
    lo = __builtin_amdgcn_perm(odd, even, 0x05010400u);
    hi = __builtin_amdgcn_perm(odd, even, 0x07030602u);
}
__device__ __forceinline__ void store8(uint8_t *row, int x0, int n, bool vec, unsigned lo, unsigned hi) {
    if (vec) {
        const u2v v = {lo, hi};
        __builtin_nontemporal_store(v, reinterpret_cast<u2v *>(row + x0));
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (x0 + i < n) row[x0 + i] = (uint8_t)((i < 4 ? lo >> (8 * i) : hi >> (8 * (i - 4))) & 0xffu);
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// four pixels: packed Y, Cb, Cr -> packed R, G, B
__device__ __forceinline__ void ycc4_to_rgb(unsigned y, unsigned cb, unsigned cr, unsigned &r, unsigned &g, unsigned &b) {
    r = g = b = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int Y = (int)((y >> (8 * i)) & 0xffu), u = (int)((cb >> (8 * i)) & 0xffu) - 128, v = (int)((cr >> (8 * i)) & 0xffu) - 128;
        r |= (unsigned)clamp255(Y + ((91881 * v + 32768) >> 16)) << (8 * i);
        g |= (unsigned)clamp255(Y + ((-22554 * u - 46802 * v + 32768) >> 16)) << (8 * i);
        b |= (unsigned)clamp255(Y + ((116130 * u + 32768) >> 16)) << (8 * i);
    }
}
__device__ __forceinline__ void rgb4_to_ycc(unsigned r, unsigned g, unsigned b, unsigned &y, unsigned &cb, unsigned &cr) {
    y = cb = cr = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int R = (int)((r >> (8 * i)) & 0xffu), G = (int)((g >> (8 * i)) & 0xffu), B = (int)((b >> (8 * i)) & 0xffu);
        y |= (unsigned)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) << (8 * i);
        cb |= (unsigned)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) << (8 * i);
        cr |= (unsigned)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) << (8 * i);
    }
}

// four pixels R G B R | G B R G | B R G B <-> packed R, G, B (v_perm_b32: selector bytes 0 .. 3 = the second operand)
__device__ __forceinline__ void rgb_interleave(unsigned r, unsigned g, unsigned b, unsigned &d0, unsigned &d1, unsigned &d2) {
    d0 = __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x01000400u), 0x03040100u);
    d1 = __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x06020005u), 0x03020500u);
    d2 = __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x00070300u), 0x07020106u);
}
__device__ __forceinline__ void rgb_deinterleave(unsigned d0, unsigned d1, unsigned d2, unsigned &r, unsigned &g, unsigned &b) {
    r = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00060300u), 0x05020100u);
    g = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00070401u), 0x06020100u);
    b = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00000502u), 0x07040100u);
}

// columns x0 .. x0 + 7 of one RGB row
template <int PLANAR>
__device__ __forceinline__ void store_rgb(const RgbOp &P, uint8_t *frame, int row, int x0, bool vec, const unsigned r[2], const unsigned g[2],
                                          const unsigned b[2]) {
    uint8_t *line = frame + (size_t)row * P.row_stride;
    if (PLANAR) {
        store8(line, x0, P.w, vec, r[0], r[1]);
        store8(line + P.plane_stride, x0, P.w, vec, g[0], g[1]);
        store8(line + 2 * P.plane_stride, x0, P.w, vec, b[0], b[1]);
        return;
    }
    if (vec) {
        unsigned d[6];
        rgb_interleave(r[0], g[0], b[0], d[0], d[1], d[2]);
        rgb_interleave(r[1], g[1], b[1], d[3], d[4], d[5]);
        u2v *o = reinterpret_cast<u2v *>(line + 3 * (size_t)x0);
        const u2v o0 = {d[0], d[1]}, o1 = {d[2], d[3]}, o2 = {d[4], d[5]};
        __builtin_nontemporal_store(o0, o);
        __builtin_nontemporal_store(o1, o + 1);
        __builtin_nontemporal_store(o2, o + 2);
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (x0 + i < P.w) {
            uint8_t *px = line + 3 * (size_t)(x0 + i);
            px[0] = (uint8_t)((r[i >> 2] >> (8 * (i & 3))) & 0xffu);
            px[1] = (uint8_t)((g[i >> 2] >> (8 * (i & 3))) & 0xffu);
            px[2] = (uint8_t)((b[i >> 2] >> (8 * (i & 3))) & 0xffu);
        }
}
template <int PLANAR>
__device__ __forceinline__ void load_rgb(const RgbOp &P, const uint8_t *frame, int row, int x0, bool vec, unsigned r[2], unsigned g[2], unsigned b[2]) {
    const uint8_t *line = frame + (size_t)row * P.row_stride;
    if (PLANAR) {
        load8(line, x0, P.w, vec, r[0], r[1]);
        load8(line + P.plane_stride, x0, P.w, vec, g[0], g[1]);
        load8(line + 2 * P.plane_stride, x0, P.w, vec, b[0], b[1]);
        return;
    }
    if (vec) {
        const u2v *s = reinterpret_cast<const u2v *>(line + 3 * (size_t)x0);
        const u2v a0 = __builtin_nontemporal_load(s), a1 = __builtin_nontemporal_load(s + 1), a2 = __builtin_nontemporal_load(s + 2);
        rgb_deinterleave(a0.x, a0.y, a1.x, r[0], g[0], b[0]);
        rgb_deinterleave(a1.y, a2.x, a2.y, r[1], g[1], b[1]);
        return;
    }
    r[0] = r[1] = g[0] = g[1] = b[0] = b[1] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t *px = line + 3 * (size_t)min(x0 + i, P.w - 1);
        r[i >> 2] |= (unsigned)px[0] << (8 * (i & 3));
        g[i >> 2] |= (unsigned)px[1] << (8 * (i & 3));
        b[i >> 2] |= (unsigned)px[2] << (8 * (i & 3));
    }
}

// One lane of planes -> RGB, spelled inline in its kernel (a macro for the reason hvc_kernels.hip gives at
// HVC_DECODE_BLOCK_PACKED: as a function taking the parameter block, k_ycc_to_rgb no longer reads its kernarg segment the way
// it did and its register figures move): columns 8 g .. 8 g + 7 of lane row lr of frame f of P (one frame per P: f = 0).
// S (420, 422, 444 or 400 = luma only) and PLANAR are compile-time constants of the scope that expands it.  A lane row is
// one image row (4:2:0: two, so that a chroma row is loaded once).
#define HVC_YCC_LANE_TO_RGB(P, f, lr, g) \
    do { \
        constexpr int ROWS = S == 420 ? 2 : 1; \
        const int x0 = (int)(8 * (g)); \
        const bool full = x0 + 8 <= (P).w; \
        unsigned cb[ROWS][2], cr[ROWS][2]; \
        if (S == 444) { \
            load8((P).cb + (f) * (P).yuv_fs + (size_t)(lr) * (P).cb_stride, x0, (P).cw, (P).vec_c && full, cb[0][0], cb[0][1]); \
            load8((P).cr + (f) * (P).yuv_fs + (size_t)(lr) * (P).cr_stride, x0, (P).cw, (P).vec_c && full, cr[0][0], cr[0][1]); \
        } else if (S != 400) { \
            const int c0 = (int)(4 * (g)); \
            const bool vc = (P).vec_c && c0 + 4 <= (P).cw; \
            _Pragma("unroll") for (int k = 0; k < 2; k++) { \
                const uint8_t *plane = (k ? (P).cr : (P).cb) + (f) * (P).yuv_fs; \
                const size_t stride = k ? (P).cr_stride : (P).cb_stride; \
                unsigned(*out)[2] = k ? cr : cb; \
                unsigned a, an; \
                load4n(plane + (size_t)(lr) * stride, c0, (P).cw, vc, a, an); \
                interleave(a, avg2x4(a, an), out[0][0], out[0][1]); \
                if (S == 420) { \
                    unsigned c, cn; \
                    load4n(plane + (size_t)min((lr) + 1u, (unsigned)(P).ch - 1u) * stride, c0, (P).cw, vc, c, cn); \
                    interleave(avg2x4(a, c), avg4x4(a, an, c, cn), out[ROWS - 1][0], out[ROWS - 1][1]); \
                } \
            } \
        } \
        uint8_t *frame = (P).rgb + (f) * (P).frame_stride; \
        _Pragma("unroll") for (int rr = 0; rr < ROWS; rr++) { \
            const int row = (int)(lr) * ROWS + rr; \
            if (row >= (P).h) break; \
            unsigned y[2], r[2], gg[2], b[2]; \
            load8((P).y + (f) * (P).yuv_fs + (size_t)row * (P).y_stride, x0, (P).w, (P).vec_y && full, y[0], y[1]); \
            if (S == 400) { \
                r[0] = gg[0] = b[0] = y[0]; \
                r[1] = gg[1] = b[1] = y[1]; \
            } else { \
                ycc4_to_rgb(y[0], cb[rr][0], cr[rr][0], r[0], gg[0], b[0]); \
                ycc4_to_rgb(y[1], cb[rr][1], cr[rr][1], r[1], gg[1], b[1]); \
            } \
            store_rgb<PLANAR>((P), frame, row, x0, (P).vec_rgb && full, r, gg, b); \
        } \
    } while (0)

// One lane of RGB -> planes, the way back, spelled inline in its kernel for the same reason: columns 8 g .. 8 g + 7 of lane row
// lr of frame f of P.  w is even for 4:2:2 and 4:2:0, h even for 4:2:0 (the launch / the plan checks), so a lane row of 4:2:0
// is two whole image rows and a lane's 8 columns give 4 chroma samples of a row of w / 2.
#define HVC_RGB_LANE_TO_YCC(P, f, lr, g) \
    do { \
        constexpr int ROWS = S == 420 ? 2 : 1; \
        const int x0 = (int)(8 * (g)); \
        const bool full = x0 + 8 <= (P).w; \
        const uint8_t *frame = (P).rgb + (f) * (P).frame_stride; \
        unsigned cb[ROWS][2], cr[ROWS][2]; \
        _Pragma("unroll") for (int rr = 0; rr < ROWS; rr++) { \
            const int row = (int)(lr) * ROWS + rr; \
            unsigned r[2], gg[2], b[2], y[2]; \
            load_rgb<PLANAR>((P), frame, row, x0, (P).vec_rgb && full, r, gg, b); \
            rgb4_to_ycc(r[0], gg[0], b[0], y[0], cb[rr][0], cr[rr][0]); \
            rgb4_to_ycc(r[1], gg[1], b[1], y[1], cb[rr][1], cr[rr][1]); \
            store8((P).y + (f) * (P).yuv_fs + (size_t)row * (P).y_stride, x0, (P).w, (P).vec_y && full, y[0], y[1]); \
        } \
        if (S == 400) break; \
        uint8_t *pcb = (P).cb + (f) * (P).yuv_fs + (size_t)(lr) * (P).cb_stride, *pcr = (P).cr + (f) * (P).yuv_fs + (size_t)(lr) * (P).cr_stride; \
        if (S == 444) { \
            store8(pcb, x0, (P).w, (P).vec_c && full, cb[0][0], cb[0][1]); \
            store8(pcr, x0, (P).w, (P).vec_c && full, cr[0][0], cr[0][1]); \
            break; \
        } \
        unsigned ob, orr; \
        if (S == 422) { /* subsample_h2: avg2 of the pair */ \
            ob = pack_even(((pairsum(cb[0][0]) + 0x00010001u) >> 1) & 0x00ff00ffu, ((pairsum(cb[0][1]) + 0x00010001u) >> 1) & 0x00ff00ffu); \
            orr = pack_even(((pairsum(cr[0][0]) + 0x00010001u) >> 1) & 0x00ff00ffu, ((pairsum(cr[0][1]) + 0x00010001u) >> 1) & 0x00ff00ffu); \
        } else { /* subsample_hv2: avg4 of the 2 x 2 */ \
            ob = pack_even(((pairsum(cb[0][0]) + pairsum(cb[ROWS - 1][0]) + 0x00020002u) >> 2) & 0x00ff00ffu, \
                           ((pairsum(cb[0][1]) + pairsum(cb[ROWS - 1][1]) + 0x00020002u) >> 2) & 0x00ff00ffu); \
            orr = pack_even(((pairsum(cr[0][0]) + pairsum(cr[ROWS - 1][0]) + 0x00020002u) >> 2) & 0x00ff00ffu, \
                            ((pairsum(cr[0][1]) + pairsum(cr[ROWS - 1][1]) + 0x00020002u) >> 2) & 0x00ff00ffu); \
        } \
        const int c0 = (int)(4 * (g)), cw = (P).w >> 1; \
        if ((P).vec_c && full) { \
            __builtin_nontemporal_store(ob, reinterpret_cast<unsigned *>(pcb + c0)); \
            __builtin_nontemporal_store(orr, reinterpret_cast<unsigned *>(pcr + c0)); \
            break; \
        } \
        _Pragma("unroll") for (int i = 0; i < 4; i++) \
            if (c0 + i < cw) { \
                pcb[c0 + i] = (uint8_t)((ob >> (8 * i)) & 0xffu); \
                pcr[c0 + i] = (uint8_t)((orr >> (8 * i)) & 0xffu); \
            } \
    } while (0)

} // namespace
#endif
