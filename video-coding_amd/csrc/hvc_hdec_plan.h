// hvc_hdec_plan.h -- the host plan of the UNIFORM GPU Huffman reader (internal): what hvc_capi_reader.hip decides and lays out
// before a launch of hvc_hdec.hip, for files that share one geometry.  Plain C++, no device code: the stand-alone program
// tests/host_harness/hdec_plan_harness.cpp runs it under sanitizers.
//
//   restart units      whether the reader's frames are the files or their restart intervals (hd_restart_units)
//   subsequence counts of a file's segment and of an interval (hd_file_subs beside hvc_hdec.h's hd_unit_subs)
//   chunk layout       one ring slot of the batch pipeline (HdChunkLayout): bytes per file in the segment ring and the named
//                      word offsets of the slot's index arrays, pinned and on the device alike
//   index fill         the words of one chunk that travel up (hd_chunk_fill)
#ifndef HVC_HDEC_PLAN_H
#define HVC_HDEC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "hvc_hdec.h"

namespace hvc {

constexpr size_t HD_SB = HVC_HD_SUBSEQ_BITS / 8; // bytes of a subsequence

// Restart intervals honoured (hvc_set_restart_markers) and the first file's scan has more than one: every interval of every
// file is a reader frame of its own (hvc_hdec.h HdParams::rst_*), ipf of them per file; else ipf = 1, frame = file.
struct HdRestart {
    bool host;             // more intervals per file than the caller takes: the host reader's
    unsigned interval, ipf; // MCUs per interval (0: none), reader frames per file
    // the capacity of a reader frame's DC-difference row (HdParams::blocks_per_frame); (< the file's blocks: no overflow)
    unsigned blocks_per_frame(unsigned blocks_per_mcu) const { return interval * blocks_per_mcu; }
};
// mcus: of one file's scan; dri: the first file's restart interval; max_ipf: the caller's ceiling on intervals per file
inline HdRestart hd_restart_units(unsigned long long mcus, bool honour, unsigned dri, unsigned long long max_ipf) {
    if (!honour || !dri || mcus <= dri) return {false, 0, 1};
    const unsigned long long q = (mcus + dri - 1) / dri;
    if (q > max_ipf) return {true, 0, 1};
    return {false, dri, (unsigned)q};
}

// Subsequences of a FILE's segment of `bytes` bytes: its own and one of zeros behind them (an interval: hd_unit_subs, which
// has none -- hvc_hdec.h)
inline size_t hd_file_subs(size_t bytes) { return (bytes + HD_SB - 1) / HD_SB + 1; }

// One ring slot of the batch pipeline, for chunks of C files of at most max_file bytes each, ipf reader frames per file.
// An entropy-coded segment is shorter than its file; every frame has one subsequence of zeros behind its bytes and 16 bytes
// of overshoot, its bytes start on a subsequence boundary (intervals: hd_unit_slot for each).
// Index arrays of a slot, in 32-bit words: [ecs_off CU][sub_off CU + 1][tabset_of CU] travel up, [frame_of C * nsub_max] is
// filled on the device, [frame_blocks CU][changed, status] are written there; the last two come back.
struct HdChunkLayout {
    size_t C, ipf;
    size_t CU;        // reader frames of a full chunk
    size_t nsub_max;  // the most subsequences a file can have
    size_t R;         // bytes per FILE in the segment ring (a multiple of 16)
    size_t ecs_bytes; // the segment ring's slot
    size_t ecs_off, sub_off, tabset_of, frame_of, frame_blocks, changed, status; // first word of each array
    size_t meta_words, upload_words; // all of them / those that travel up: ecs_off | sub_off | tabset_of
    size_t state_subs; // subsequences the reader's per-subsequence state is carved for

    // the sizes the reader's 32-bit indices cannot hold: such a batch is the host reader's
    bool fits() const { return C * nsub_max < (1ull << 31) && C * R < (1ull << 31); }
    size_t file_at(size_t i) const { return i * R; } // where file i of the chunk is unstuffed to, in bytes from the slot
    // ... and the room the unstuffing is given there (without intervals: the extra subsequence and the overshoot stay free)
    size_t file_cap() const { return ipf > 1 ? R : (nsub_max - 1) * HD_SB; }
};
inline HdChunkLayout hd_chunk_layout(size_t C, size_t ipf, size_t max_file) {
    HdChunkLayout L;
    L.C = C, L.ipf = ipf, L.CU = C * ipf;
    const size_t whole = (max_file + HD_SB - 1) / HD_SB;
    L.nsub_max = ipf > 1 ? whole + 2 * ipf : whole + 1;
    L.R = ipf > 1 ? whole * HD_SB + ipf * (2 * HD_SB + 16) : L.nsub_max * HD_SB + 16;
    L.ecs_bytes = C * L.R;
    L.state_subs = C * L.nsub_max;
    L.ecs_off = 0;
    L.sub_off = L.ecs_off + L.CU;
    L.tabset_of = L.sub_off + L.CU + 1;
    L.frame_of = L.upload_words = L.tabset_of + L.CU;
    L.frame_blocks = L.frame_of + L.state_subs;
    L.changed = L.frame_blocks + L.CU;
    L.status = L.changed + 1;
    L.meta_words = L.status + 1;
    return L;
}

// The words of a chunk of cnt <= C files that travel up, into the slot's pinned words hm[0, L.upload_words): where every
// reader frame's bytes start (ecs_off), its first subsequence (sub_off, and the total behind the last), its table record
// (tabset_of: 0 = the first file's, 1 + f = file f's own).  ecs_size / frame_pf: [cnt] of the chunk's files; unit_off /
// unit_len: [cnt][ipf] their intervals' places inside the file's region and bytes (read when L.ipf > 1 only).
struct HdChunkFill {
    unsigned subs;   // subsequences of the chunk
    bool own_tables; // a file of the chunk carries tables of its own
};
inline HdChunkFill hd_chunk_fill(const HdChunkLayout &L, unsigned *hm, int cnt, const unsigned *ecs_size, const unsigned *unit_off,
                                 const unsigned *unit_len, const char *frame_pf) {
    HdChunkFill r{0, false};
    for (int f = 0; f < cnt; f++) {
        r.own_tables |= frame_pf[f] != 0;
        for (size_t q = 0; q < L.ipf; q++) { // the file's reader frames: itself, or its restart intervals
            const size_t u = (size_t)f * L.ipf + q;
            hm[L.tabset_of + u] = frame_pf[f] ? 1u + (unsigned)f : 0u;
            hm[L.ecs_off + u] = (unsigned)(L.file_at((size_t)f) + (L.ipf > 1 ? unit_off[u] : 0u));
            hm[L.sub_off + u] = r.subs;
            r.subs += (unsigned)(L.ipf > 1 ? hd_unit_subs(unit_len[u]) : hd_file_subs(ecs_size[f]));
        }
    }
    hm[L.sub_off + (size_t)cnt * L.ipf] = r.subs;
    return r;
}

} // namespace hvc
#endif
