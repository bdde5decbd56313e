// hvc_resize.hip -- the resampling step over RGB images of DIFFERENT size, each to a size of its own, in one launch per pass:
// k_resize_h_mixed (rows: source -> an 8-bit intermediate of out_w x h) and k_resize_v_mixed (columns: intermediate ->
// destination).  The definition is include/hvc_jpeg.h, Resizing -- Pillow's Image.resize on 8-bit images, bit for bit: 22-bit
// integer taps made on the host (hvc_resize_plan.cpp), clip_0_255((2^21 + SUM k[i] * in[xmin + i]) >> 22) per sample here.
//
// Both kernels work under the image passes' decomposition of hvc_mixed_dev.h; an image descriptor says where the pass reads and
// writes and which axis table it uses.  No LDS.
//
// k_resize_h_mixed: a unit = 64 consecutive lanes of one image; a lane makes one output sample position of one source row
// in all its channels (3 interleaved, 1 for a plane of a planar image: the plan emits a planar image as three one-channel
// images).  Its (xmin, count, first tap) record and its taps come from the table, stored transposed so that the 64 lanes read
// consecutive words; the source row is read as bytes that the neighbouring lanes share (their windows overlap: the lines
// come from L1 / L2 once).
//
// k_resize_v_mixed does not know channels: an output row is a run of bytes, each byte a tap sum over the same byte of `count`
// source rows.  A lane makes 4 consecutive bytes of one output row, with dword loads and stores where the image's `vec` flag
// allows (the branch is wave-uniform; the last lane of a row whose byte count is no multiple of 4 takes the byte path for
// what is left).  The lane mapping differs from the horizontal pass in one point, on purpose: a unit = 64 consecutive lanes of
// ONE ROW of one image rather than of the image, so that the row's record and taps are wave-uniform as well and come through
// scalar loads; the price is idle lanes at the end of every row (224 x 3 bytes: 168 of 192 lanes work).
//
// k_resize_v_mixed_lut<ELEM> (below, at the kernel): the vertical pass under a typed output -- the same lanes and samples, each
// sample looked up in a caller's table of 2- or 4-byte elements and stored as such.
//
// The multiply: every tap fits 24 signed bits and every sample 8, the plan checks both, so a multiply-add is one
// v_mad_i32_i24 (__mul24); the accumulator stays inside int32 by the plan's check of 255 * SUM |k| + 2^21 < 2^31.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hvc_jpeg.h"
#include "hvc_mixed_dev.h"
#include "hvc_resize.h"

namespace hvc {
namespace {

#define HVC_RESIZE_ROUND (1 << (HVC_RESIZE_PRECISION_BITS - 1))

__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = acc >> HVC_RESIZE_PRECISION_BITS; // arithmetic
    return (unsigned)min(max(v, 0), 255);
}

template <int CH>
__device__ __forceinline__ void resize_h_lane(const ResizeImageK &K, const ResizeParams &P, unsigned row, unsigned xx) {
    const ResizeRecK rec = P.recs[K.rec0 + xx];
    const uint8_t *s = P.src[0] + K.src_base + (size_t)row * K.src_stride + (size_t)rec.xmin * CH;
    const int *k = P.taps + rec.first;
    int acc[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) acc[c] = HVC_RESIZE_ROUND;
    for (unsigned i = 0; i < rec.count; i++) { // xmin + count <= n_in: every byte read is the row's own
        const int t = k[(size_t)i * K.tap_stride];
#pragma unroll
        for (int c = 0; c < CH; c++) acc[c] += __mul24(t, (int)s[(size_t)i * CH + c]);
    }
    uint8_t *d = (K.dst_sel ? P.dst[1] : P.dst[0]) + K.dst_base + (size_t)row * K.dst_stride + (size_t)xx * CH;
#pragma unroll
    for (int c = 0; c < CH; c++) d[c] = (uint8_t)clip8(acc[c]);
}

__global__ __launch_bounds__(HVC_MIXED_LANES) void k_resize_h_mixed(ResizeParams P) {
    const MixedWave W = mixed_wave_plain();
    if (W.unit >= P.n_units) return;
    const ResizeImageK K = P.images[P.map[W.unit]]; // wave-uniform: read once, before any store
    MixedImageLane L;
    if (!mixed_image_lane(K, W.unit, W.lane, L)) return;
    if (K.ch == 3) resize_h_lane<3>(K, P, L.row, L.group); // wave-uniform
    else resize_h_lane<1>(K, P, L.row, L.group);
}

__global__ __launch_bounds__(HVC_MIXED_LANES) void k_resize_v_mixed(ResizeParams P) {
    const MixedWave W = mixed_wave_plain();
    if (W.unit >= P.n_units) return;
    const ResizeImageK K = P.images[P.map[W.unit]]; // wave-uniform
    MixedImageLane L;
    if (!mixed_image_row_lane(K, W.unit, W.lane, L)) return;
    const unsigned l = L.t, row = L.row;
    const unsigned b = l * 4;                                   // the lane's first byte of the row
    const unsigned nb = min(4u, K.row_bytes - b);               // (l < lanes: b < row_bytes)
    const ResizeRecK rec = P.recs[K.rec0 + row];                // wave-uniform: the row's record and taps are scalar loads
    const int *k = P.taps + rec.first;
    const uint8_t *s = (K.src_sel ? P.src[1] : P.src[0]) + K.src_base + (size_t)rec.xmin * K.src_stride + b;
    uint8_t *d = P.dst[0] + K.dst_base + (size_t)row * K.dst_stride + b;
    int a0 = HVC_RESIZE_ROUND, a1 = HVC_RESIZE_ROUND, a2 = HVC_RESIZE_ROUND, a3 = HVC_RESIZE_ROUND;
    if (K.vec && nb == 4) { // K.vec: wave-uniform; nb < 4 only in the last lane of a row
        for (unsigned i = 0; i < rec.count; i++) { // xmin + count <= the source's rows
            const int t = k[(size_t)i * K.tap_stride];
            const unsigned v = *reinterpret_cast<const unsigned *>(s + (size_t)i * K.src_stride);
            a0 += __mul24(t, (int)(v & 255u));
            a1 += __mul24(t, (int)((v >> 8) & 255u));
            a2 += __mul24(t, (int)((v >> 16) & 255u));
            a3 += __mul24(t, (int)(v >> 24));
        }
        // Bytes 0, 2 and bytes 1, 3 are joined first: written as b0 | b1 << 8 | ..., the compiler turns the first pair into
        // v_ashr_pk_u8_i32, which writes 16 bits and leaves the upper half of its destination as it was -- on the GPU bytes 2
        // and 3 of every dword then held what the register held before (profiles/resize_rocprofv3.txt).
        const unsigned even = clip8(a0) | clip8(a2) << 16, odd = clip8(a1) | clip8(a3) << 16;
        *reinterpret_cast<unsigned *>(d) = even | odd << 8;
        return;
    }
    for (unsigned i = 0; i < rec.count; i++) {
        const int t = k[(size_t)i * K.tap_stride];
        const uint8_t *q = s + (size_t)i * K.src_stride;
        a0 += __mul24(t, (int)q[0]);
        if (nb > 1) a1 += __mul24(t, (int)q[1]);
        if (nb > 2) a2 += __mul24(t, (int)q[2]);
        if (nb > 3) a3 += __mul24(t, (int)q[3]);
    }
    d[0] = (uint8_t)clip8(a0);
    if (nb > 1) d[1] = (uint8_t)clip8(a1);
    if (nb > 2) d[2] = (uint8_t)clip8(a2);
    if (nb > 3) d[3] = (uint8_t)clip8(a3);
}

// k_resize_v_mixed_lut<ELEM>: the vertical pass under a typed output (include/hvc_jpeg.h, Typed output).  The decomposition,
// the record, the taps and the 4 samples of a lane are k_resize_v_mixed's, to the letter; the samples are then looked up in
// the caller's table -- sample v of channel c becomes lut[c * 256 + v], ELEM bytes of raw bits -- and 4 ELEMENTS are stored: one
// 8- or 16-byte store where the descriptor's `dvec` says every destination row starts on 4 * ELEM bytes (wave-uniform), element
// stores otherwise and for what the tail lane of a row has left.  `vec` speaks of the source rows alone here.  The channel:
// a plane of a planar image has one (K.chan, wave-uniform); in an interleaved row sample j of lane l is sample 4 l + j of the
// row, and 4 = 1 (mod 3), so its channel is (l + j) % 3 -- l counts through the row's 64-lane units, so this holds across them.
//
// The table (1.5 or 3 KiB) is read through the caches, not staged in LDS: every workgroup of the launch reads the same few
// lines, so they stay in L1 / L2, while a workgroup makes only 1024 samples -- staging 768 elements per group would cost about
// as many loads as the group has lookups, plus a barrier that every lane would have to reach before the early returns below
// (the last group's spare units).  No LDS, no barrier, no scratch.
template <int ELEM> struct LutElem;
template <> struct LutElem<2> { typedef uint16_t type; };
template <> struct LutElem<4> { typedef uint32_t type; };

template <int ELEM>
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_resize_v_mixed_lut(ResizeParams P, const typename LutElem<ELEM>::type *__restrict__ lut) {
    typedef typename LutElem<ELEM>::type E;
    const MixedWave W = mixed_wave_plain();
    if (W.unit >= P.n_units) return;
    const ResizeImageK K = P.images[P.map[W.unit]]; // wave-uniform
    MixedImageLane L;
    if (!mixed_image_row_lane(K, W.unit, W.lane, L)) return;
    const unsigned l = L.t, row = L.row;
    const unsigned b = l * 4;                                   // the lane's first sample of the row
    const unsigned nb = min(4u, K.row_bytes - b);               // (l < lanes: b < row_bytes)
    const ResizeRecK rec = P.recs[K.rec0 + row];                // wave-uniform
    const int *k = P.taps + rec.first;
    const uint8_t *s = (K.src_sel ? P.src[1] : P.src[0]) + K.src_base + (size_t)rec.xmin * K.src_stride + b;
    uint8_t *d = P.dst[0] + K.dst_base + (size_t)row * K.dst_stride + (size_t)b * ELEM;
    int a0 = HVC_RESIZE_ROUND, a1 = HVC_RESIZE_ROUND, a2 = HVC_RESIZE_ROUND, a3 = HVC_RESIZE_ROUND;
    if (K.vec && nb == 4) { // K.vec: wave-uniform; nb < 4 only in the last lane of a row
        for (unsigned i = 0; i < rec.count; i++) { // xmin + count <= the source's rows
            const int t = k[(size_t)i * K.tap_stride];
            const unsigned v = *reinterpret_cast<const unsigned *>(s + (size_t)i * K.src_stride);
            a0 += __mul24(t, (int)(v & 255u));
            a1 += __mul24(t, (int)((v >> 8) & 255u));
            a2 += __mul24(t, (int)((v >> 16) & 255u));
            a3 += __mul24(t, (int)(v >> 24));
        }
    } else {
        for (unsigned i = 0; i < rec.count; i++) {
            const int t = k[(size_t)i * K.tap_stride];
            const uint8_t *q = s + (size_t)i * K.src_stride;
            a0 += __mul24(t, (int)q[0]);
            if (nb > 1) a1 += __mul24(t, (int)q[1]);
            if (nb > 2) a2 += __mul24(t, (int)q[2]);
            if (nb > 3) a3 += __mul24(t, (int)q[3]);
        }
    }
    // the channels of the 4 samples, times 256 (a sample past the row's end looks up a valid entry and is not stored)
    unsigned c0, c1, c2;
    if (K.chan < 3) { // wave-uniform
        c0 = c1 = c2 = K.chan << 8;
    } else {
        const unsigned m = l % 3;
        c0 = m << 8, c1 = (m == 2 ? 0 : m + 1) << 8, c2 = (m == 0 ? 2 : m - 1) << 8;
    }
    const E e0 = lut[c0 + clip8(a0)], e1 = lut[c1 + clip8(a1)], e2 = lut[c2 + clip8(a2)], e3 = lut[c0 + clip8(a3)];
    if (K.dvec && nb == 4) { // K.dvec: wave-uniform
        if (ELEM == 2)
            *reinterpret_cast<uint2 *>(d) = make_uint2((unsigned)e0 | (unsigned)e1 << 16, (unsigned)e2 | (unsigned)e3 << 16);
        else
            *reinterpret_cast<uint4 *>(d) = make_uint4((unsigned)e0, (unsigned)e1, (unsigned)e2, (unsigned)e3);
        return;
    }
    E *q = reinterpret_cast<E *>(d);
    q[0] = e0;
    if (nb > 1) q[1] = e1;
    if (nb > 2) q[2] = e2;
    if (nb > 3) q[3] = e3;
}

} // namespace

hipError_t launch_resize_h_mixed(const ResizeParams &P, hipStream_t s) { return mixed_launch(k_resize_h_mixed, P, s, nullptr, nullptr); }

hipError_t launch_resize_v_mixed(const ResizeParams &P, hipStream_t s) { return mixed_launch(k_resize_v_mixed, P, s, nullptr, nullptr); }

hipError_t launch_resize_v_mixed_lut(const ResizeParams &P, const void *lut, int elem, hipStream_t s) {
    if ((elem != 2 && elem != 4) || !lut) return hipErrorInvalidValue;
    if (elem == 2) return mixed_launch(k_resize_v_mixed_lut<2>, P, s, nullptr, nullptr, static_cast<const uint16_t *>(lut));
    return mixed_launch(k_resize_v_mixed_lut<4>, P, s, nullptr, nullptr, static_cast<const uint32_t *>(lut));
}

} // namespace hvc
