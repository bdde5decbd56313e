// hvc_hdec_dev.h -- device code the GPU Huffman readers share (internal): the uniform-geometry reader of hvc_hdec.hip and the
// mixed-geometry reader of hvc_hdec_mixed.hip walk the same symbol loops over the same table formats.
#ifndef HVC_HDEC_DEV_H
#define HVC_HDEC_DEV_H

#include "hvc_hdec.h"

namespace hvc {
namespace hd_dev {

constexpr int S = HVC_HD_SUBSEQ_BITS;

// per subsequence: state = bit position | k << 32 | block-in-MCU << 40
__device__ __forceinline__ unsigned long long pack_state(unsigned p, int k, int b) {
    return (unsigned long long)p | ((unsigned long long)(unsigned)k << 32) | ((unsigned long long)(unsigned)b << 40);
}

// A staged subsequence: its S / 32 dwords and one more.  A symbol starts before bit S and is at most 32 bits long
// (code <= 16, magnitude <= 16), so bit S + 31 is the last one any walk looks at.  S / 32 + 1 is odd: lanes reading
// the same dword index of their rows hit different LDS banks.
constexpr int SROW = S / 32 + 1;
static_assert((SROW & 1) == 1, "odd row stride");
__device__ __forceinline__ void stage_row(unsigned *row, const uint8_t *seg) {
    const uint4 *src = reinterpret_cast<const uint4 *>(seg);
#pragma unroll
    for (int q = 0; q < S / 128; q++) {
        const uint4 v = src[q];
        row[4 * q + 0] = __builtin_bswap32(v.x);
        row[4 * q + 1] = __builtin_bswap32(v.y);
        row[4 * q + 2] = __builtin_bswap32(v.z);
        row[4 * q + 3] = __builtin_bswap32(v.w);
    }
    row[S / 32] = __builtin_bswap32(reinterpret_cast<const unsigned *>(seg)[S / 32]); // the segment buffer has 16 bytes past every frame
}
constexpr int SPEC_T = HVC_HD_SPEC_T;

// 2-bit fields of a PF selmask with component 2 renamed 1 (its tables are component 1's: HdFrameTabs::flags)
__device__ __forceinline__ unsigned selmask_c2_as_c1(unsigned sel) {
    const unsigned hi = sel & 0xaaaaaaaau;
    return (sel & ~hi) | (hi >> 1);
}

// A code under a prefix that has no sub-table (HVC_HD_OVF): the canonical search of ITU-T T.81 F.2.2.3 over the lengths
// 11..16 in the table's overflow record (device memory; rare by construction -- the prefixes without a sub-table hold
// the table's least frequent symbols).  w = the next 32 bits; VAL picks the entry format.  "No such code" = entry 1.
template <bool VAL>
__device__ __noinline__ unsigned ovf_lookup(const HdOvf *o, unsigned w) {
    const unsigned w16 = w >> 16;
    for (int i = 0; i < 6; i++) {
        const unsigned d = (w16 >> (5 - i)) - (unsigned)o->mincode[i];
        if (d < (unsigned)o->count[i]) return (VAL ? o->val : o->spec)[(unsigned)o->valptr[i] + d];
    }
    return 1u;
}

// rd(i) = dword i of the subsequence, big-endian order restored (i <= S / 32: one dword past it).  sp = the tables of
// the frame: [slot or component][DC, AC][SPEC_T] -- in LDS (one set for the whole batch) or, in PF mode, in device
// memory (this frame's record); sel = HdParams::selmask.
// The loop body is straight-line code but for the second-level look-up: in a wavefront of 64 walks SOME lane refills
// its window or ends a block in nine iterations out of ten, so a branch around either is paid every time, plus its
// mask bookkeeping -- and a refill inside a branch made the wavefront wait for its LDS read on the spot.  Selects
// instead; with RD_FREE (rows in LDS) the dword after the window is simply read again in every iteration (rd(ni) is a
// function of ni), and nothing waits for it before the next table look-up has come back anyway.
// RD_FREE: the row sits in LDS at `row` (SROW dwords and two more that may be read, whatever they hold).
// SEL1: sel has one bit per block of an MCU (HdParams::slotmask: the two slots of HdSpec); otherwise two (selmask).
// ovf = the overflow records of the same tables, [slot or component][DC, AC] (device memory).
template <bool RD_FREE, bool SEL1, class RD>
__device__ __forceinline__ void spec_walk(RD rd, const unsigned *row, const uint16_t *sp, const HdOvf *ovf, unsigned sel, int B, unsigned base,
                                          unsigned &p, int &k, int &b, unsigned &nb) {
    // The bit position is kept as mm = ~(P + 31), P = bits consumed since the start of the row (P < 32 + S at the
    // start): its low five bits are what v_alignbit has to shift {hi, lo} by, the window moves on by a dword when mm
    // changes above bit 4, and "p < limit" is "mm > ~(S + 31)" -- one subtraction per symbol keeps all of that current.
    // lo = dword (P + 31) >> 5 of the row, hi the one before (not looked at when P is a multiple of 32), nx the one
    // after -- read from *np, which moves with the window (up to two dwords past the row: nothing looks at those).
    const unsigned P0 = p - base;
    unsigned mm = ~(P0 + 31u);
    const unsigned mm_limit = ~((unsigned)S + 31u);
    const unsigned l0 = (P0 + 31u) >> 5;
    unsigned hi = l0 ? rd(l0 - 1u) : 0u;
    unsigned lo = rd(min(l0, (unsigned)(SROW - 1)));
    unsigned nx = rd(min(l0 + 1u, (unsigned)(SROW - 1)));
    const unsigned *np = row + l0 + 1u;
    auto tables_of = [&](int bb) -> const uint16_t * {
        return sp + __umul24(SEL1 ? __builtin_amdgcn_ubfe(sel, (unsigned)bb, 1u) : (sel >> (2 * bb)) & 3u, 2u * SPEC_T); // (a 32-bit multiply runs at a quarter of the rate)
    };
    const uint16_t *bt = tables_of(b);
    while (mm > mm_limit) {
        const unsigned w = __builtin_amdgcn_alignbit(hi, lo, mm); // the next 32 bits
        const uint16_t *t = bt + (k ? SPEC_T : 0);
        unsigned e = t[w >> 22];
        unsigned used = e & 63u;
        if (used == 0u) { // the code is longer than the first level's 10 bits
            const unsigned sn = e >> 6;
            if (sn != HVC_HD_OVF) e = t[1024u + sn * 64u + ((w >> 16) & 63u)];
            else e = ovf_lookup<false>(ovf + ((SEL1 ? __builtin_amdgcn_ubfe(sel, (unsigned)b, 1u) : (sel >> (2 * b)) & 3u) * 2u + (k ? 1u : 0u)), w);
            used = e & 63u;
        }
        k += (int)((e >> 6) & 127u); // an EOB advances by 64
#ifdef HVC_HD_STATS
        nb += 1u << 16; // experiments: symbols of this walk in the upper half (the caller takes it out again)
#endif
        const unsigned mn = mm - used;
        const bool refill = ((mn ^ mm) >> 5) != 0u; // the window's first dword is used up (<= 32 bits a symbol: one step is enough)
        mm = mn;
        if (RD_FREE) {
            hi = refill ? lo : hi;
            lo = refill ? nx : lo;
            np += refill ? 1 : 0;
            nx = *np;
        } else if (refill) {
            hi = lo;
            lo = nx;
            nx = rd(min((31u - mn) >> 5, (unsigned)(SROW - 1)));
        }
        // EOB, index 63 written, or past it (the model raises: the true parse never gets here)
        const bool end = k >= 64;
        const int b1 = b + 1 == B ? 0 : b + 1;
        k = end ? 0 : k;
        b = end ? b1 : b;
        nb += end ? 1u : 0u;
        bt = tables_of(b);
    }
    p = base + ~mm - 31u;
}

// One entry of a value table (k_hd_write2; HdFrameTabs::val), from HdTable's (length << 8) | value:
//   bits 0-4   bits the symbol takes: code + magnitude, 1..31;  0 = (first level only) the code is longer: bits 5-15
//              hold the number of the sub-table that has it
//   bits 5-8   magnitude bits (0..15)
//   bits 9-13  index advance: run of zeros + 1 (1 for a DC symbol; an EOB's does not matter);  0 marks what the model
//              raises on -- no code with this prefix (the walk steps one bit) or a DC category whose magnitude
//              decoder.ml:73-79 cannot hold; for the DC that is category 16 as well: its differences (|d| >= 32768, or
//              -32768) leave int16 or the range a JPEG DC can have, so the stream goes to the host reader either way
//              and the loop needs no range check
//   bit 15     EOB
__host__ __device__ inline unsigned val_entry(unsigned e, bool dc, bool second_level) {
    if (e & 0x8000u) return second_level ? 1u : (e & 0x7fffu) << 5; // (a pointer inside a sub-table: no such code)
    if (!e) return 1u;
    const unsigned len = e >> 8, v = e & 0xffu;
    if (dc) return v >= 16u ? len : (len + v) | (v << 5) | (1u << 9);
    const unsigned size = v & 15u, run = v >> 4;
    return (len + size) | (size << 5) | ((run + 1u) << 9) | (v ? 0u : 0x8000u);
}

// One symbol of the WRITE passes (k_hd_write2, k_hdm_write), from val_entry's tables: what it consumes, the coefficient it
// carries and where the zig-zag index goes.  w = the next 32 bits; t = the table of the symbol's class (DC for k == 0, AC
// otherwise) of block b's component: first level, then the sub-tables; ovf = the overflow records of the file's tables,
// [slot or component][DC, AC]; selmask: 2 bits per block of an MCU (which tables it reads).
// Straight-line code but for the second-level look-up; one path for DC and AC symbols (a DC symbol advances the index from 0 to 1).
struct HdSymbol {
    unsigned used;  // bits the symbol takes: code + magnitude, 1..31
    int mag;        // its coefficient (decoder.ml:73-79 mag'); |mag| < 2^15: size <= 15
    int kn;         // one past the index the coefficient has: k + run + 1
    bool wrong;     // what the model raises on: "Can't find dc / ac code" (one bit further), a DC category of 16 and above (the
                    // code is skipped), "coefficient index out of range"
    bool end_block; // EOB, or index 63 written (what is wrong for its code advances by 0 and is no EOB)
};
__device__ __forceinline__ HdSymbol val_symbol(unsigned w, const uint16_t *t, const HdOvf *ovf, unsigned selmask, int b, int k) {
    unsigned e = t[__builtin_amdgcn_ubfe(w, 22u, 10u)];
    if ((e & 31u) == 0u) { // a longer code: its prefix's sub-table, or (no sub-table: HVC_HD_OVF) the canonical search
        const unsigned sn = e >> 5;
        if (sn != HVC_HD_OVF) e = t[1024u + sn * 64u + __builtin_amdgcn_ubfe(w, 16u, 6u)];
        else e = ovf_lookup<true>(ovf + (((selmask >> (2 * b)) & 3u) * 2u + (k ? 1u : 0u)), w);
    }
    const unsigned used = e & 31u, size = __builtin_amdgcn_ubfe(e, 5u, 4u), adv = __builtin_amdgcn_ubfe(e, 9u, 5u);
    const bool eob = (int16_t)e < 0;
    const bool bad = adv == 0u;
    // mag': `size` bits after the code; a leading 0 bit means negative, i.e. the field minus (2^size - 1).  As a signed
    // field x that is x - full where the leading bit is 0, x - ~full where it is 1.
    const int x = __builtin_amdgcn_sbfe((int)w, 32u - used, size);
    const int full = (int)__builtin_amdgcn_ubfe(0xffffffffu, 0u, size);
    HdSymbol s;
    s.used = used;
    s.mag = x - (full ^ (x >> 31));
    s.kn = k + (int)adv;
    s.wrong = bad || (s.kn > 64 && !eob);
    s.end_block = eob || s.kn > 63;
    return s;
}

} // namespace hd_dev
} // namespace hvc
#endif
