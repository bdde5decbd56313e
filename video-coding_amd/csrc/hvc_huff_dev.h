// hvc_huff_dev.h -- device code shared by the GPU Huffman coders (internal): the uniform coder (hvc_huff.hip, one geometry
// per launch from HuffParams) and the mixed coder (hvc_huff_mixed.hip, the geometry of every work unit from device memory).
// ONE copy of the symbol walk over a block and of the three sinks it feeds, and the load of a block's record.  Everything is
// __forceinline__ and lives in an anonymous namespace of the including translation unit, as hvc_rgb_dev.h, hvc_scaled_dev.h
// and hvc_hdec_dev.h do it.
#ifndef HVC_HUFF_DEV_H
#define HVC_HUFF_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hvc {
namespace {

// The walk over one block, shared by the histogram, the length and the emit pass.  It hands the sink every symbol as
// SINK::sym(slot, magnitude, size): slot = the symbol's entry of a table set (DC category, or 16 + ((run << 4) | size) for
// AC, 16 + 0xf0 ZRL, 16 EOB), magnitude = its size low bits (encoder.ml:155-160).
template <class SINK>
__device__ __forceinline__ void walk_block(const unsigned (&w)[32], int pred, SINK &sink, unsigned &err) {
    const int dc = (int)(short)(w[0] & 0xffffu);
    const int diff = dc - pred;
    {
        const unsigned a = (unsigned)(diff < 0 ? -diff : diff);
        const int size = a ? 32 - __clz((int)a) : 0;
        if (size > 11) err = 1; // no code in the default DC tables (the host coder returns HVC_E_RANGE)
        const unsigned mag = (unsigned)(diff >= 0 ? diff : diff - 1) & ((1u << size) - 1u);
        sink.sym(size & 15, mag, size);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
        const int v = (k & 1) ? (int)w[k >> 1] >> 16 : (int)(short)(w[k >> 1] & 0xffffu);
        if (v == 0) {
            run++;
        } else {
            while (run >= 16) { // ZRL (encoder.ml:162-187)
                sink.sym(16 + 0xf0, 0u, 0);
                run -= 16;
            }
            const unsigned a = (unsigned)(v < 0 ? -v : v);
            const int size = 32 - __clz((int)a);
            if (size > 10) err = 1; // no code in the default AC tables
            const unsigned mag = (unsigned)(v >= 0 ? v : v - 1) & ((1u << size) - 1u);
            sink.sym(16 + ((run << 4) | (size & 15)), mag, size);
            run = 0;
        }
    }
    if (run) sink.sym(16, 0u, 0); // EOB
}

// the length and the emit pass look their codes up in LDS: (code << 5) | length
struct LenSink {
    const unsigned *tab; // LDS: 16 dc + 256 ac
    unsigned bits = 0;
    __device__ __forceinline__ void sym(int slot, unsigned, int size) { bits += (tab[slot] & 31u) + (unsigned)size; }
};

// Writes a bit string at an arbitrary bit offset of a zero-initialised big-endian bit buffer.  The
// first and the last word of the string may be shared with the neighbouring blocks: atomicOr; the
// words in between belong to this block alone: plain stores.
struct EmitSink {
    const unsigned *tab;     // LDS: 16 dc + 256 ac
    unsigned *wp;            // next 32-bit word of the frame's buffer
    unsigned long long acc;  // pending bits, right-aligned
    int n;                   // number of pending bits (including the `lead` bits of the first word)
    bool first;
    __device__ __forceinline__ void init(unsigned *buf, unsigned long long bitpos) {
        wp = buf + (bitpos >> 5);
        acc = 0;
        n = (int)(bitpos & 31u); // the leading bits of the first word are somebody else's: zeros here
        first = n != 0;
    }
    __device__ __forceinline__ void sym(int slot, unsigned mag, int size) {
        const unsigned e = tab[slot];
        put(((e >> 5) << size) | mag, (int)(e & 31u) + size);
    }
    __device__ __forceinline__ void put(unsigned code, int len) { // len <= 27
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const unsigned word = (unsigned)(acc >> (n - 32));
            n -= 32;
            const unsigned be = __builtin_bswap32(word);
            if (first)
                atomicOr(wp, be);
            else
                *wp = be;
            first = false;
            wp++;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(wp, __builtin_bswap32((unsigned)(acc << (32 - n))));
    }
};

// the histogram pass counts symbols into LDS bins of the block's table set; EOB (at most one per block, the symbol every
// block shares) is left to a wave ballot
struct HistSink {
    unsigned *bins; // LDS: 16 dc + 256 ac
    bool eob = false;
    __device__ __forceinline__ void sym(int slot, unsigned, int) {
        if (slot == 16)
            eob = true;
        else
            atomicAdd(bins + slot, 1u);
    }
};

// the 64 coefficients of a block's record (on 16 bytes) as 32 pairs
__device__ __forceinline__ void load_record(const int16_t *rec, unsigned (&w)[32]) {
    const uint4 *src = reinterpret_cast<const uint4 *>(rec);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 t = src[j];
        w[4 * j + 0] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
    }
}

} // namespace
} // namespace hvc
#endif
