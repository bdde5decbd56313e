// hvc_huff.hip -- baseline Huffman coding of quantised coefficient records ON THE GPU (gfx950).
//
// The encoder's back end (Encoder.rle + write_bits + Bitstream_writer with byte stuffing,
// jpeg/model/src/encoder.ml:127-193, common/src/bitstream_writer.ml) is sequential in the model, but
// nothing in it depends on earlier OUTPUT: every block's bit string is a function of its own 64
// coefficients and of one other DC value (the predictor = the previous block of the same component
// in scan order).  So the scan is rebuilt as data-parallel passes over device-resident records:
//   1  k_huff_len     one block per lane: bit length of the block's code -> lens[scan index]
//   2  k_scan_u32     per frame exclusive prefix sum (one workgroup per frame)   -> bit offsets
//   3  k_huff_emit    one block per lane: the same walk, now writing the bits at the block's offset
//                     (big-endian bit order; words shared with a neighbour by atomicOr)
//   4  k_ff_count / k_scan_u32 / k_frame_offsets / k_stuff_write: 0xFF -> 0xFF 0x00 and packing of the
//                     frames' segments back to back
// The bytes equal hvc_jpeg_entropy_encode's scan data (tests/test_gpu_huffman.py), hence the model's.
// The default (Annex K) tables, as Encoder.Parameters.c420/c422/c444 use (encoder.ml:306-349), are one pair for every
// frame.  With per-frame optimised tables (hvc_huffman_encode_frames_optimised, hvc_set_huffman_tables) two passes run
// first, over the same walk:
//   0a k_huff_hist    symbol counts per frame and table set (LDS bins per workgroup, one flush of the non-zero bins)
//   0b k_huff_build   one wavefront per (frame, table): ITU-T T.81 Annex K.2 -> code table + DHT body per frame
// and passes 1 and 3 read frame f's tables at tables + f * table_stride.
// With a restart interval Ri (hvc_set_restart_interval; ITU-T T.81 B.2.4.4, E.1.4) the frame is cut every Ri MCUs: each
// interval starts on a byte, with no DC predictor, behind an RSTn marker.  The passes above run as their *_rst twins
// (the same bodies, template <bool RST>; the plain kernels are the RST = false instantiations, unchanged), and
//   2b k_ivl_bytes    one interval per lane: its bytes = ceil(bits / 8) from the bit offsets of pass 2; a second
//                     k_scan_u32 gives every interval's byte base in the unstuffed segment
// follows pass 2.  Pass 3 writes a block at 8 * base[interval] + its offset inside the interval and pads every
// interval's last block with ones.  The markers never enter the bit buffer (they must not be stuffed): behind pass 4a
// k_ff_marks adds 2 bytes per interval boundary to the count of the piece that holds the boundary, so the scan leaves
// room for them, and pass 4d's byte-wise path writes FF Dn when it crosses one.
#include <vector>

#include "hvc_huff.h"
#include "hvc_huff_dev.h"

namespace hvc {

namespace {

constexpr int HT = 256; // blocks (lanes) per workgroup, one component plane tile like K1 / K3
constexpr int HIST_GROUPS = 2048; // k_huff_hist: workgroups per launch to aim at (each walks several tiles of its frame)

struct BlockPos {
    int comp, bx, by;
    bool active;
    unsigned scan;     // index of the block in scan order inside its frame
    unsigned mcu;      // index of its MCU (read by the RST passes only)
    size_t coef_idx;   // int16 element index of the block's coefficients
    size_t pred_idx;   // ... of the block whose DC is the predictor (valid when has_pred)
    bool has_pred;
};

template <bool RST>
__device__ __forceinline__ BlockPos locate_block(const HuffParams &P, int frame, int tile, int lane) {
    BlockPos r;
    int c = 0;
#pragma unroll
    for (int i = 1; i < 3; i++)
        if (tile >= P.comp[i].tile0) c = i;
    const HuffComp &K = P.comp[c];
    int b = (tile - K.tile0) * HT + lane;
    r.active = b < K.nblk;
    b = r.active ? b : K.nblk - 1;
    const int by = b / K.bw, bx = b - by * K.bw;
    r.comp = c;
    r.bx = bx;
    r.by = by;
    const size_t base = (size_t)frame * P.coef_fs + K.coef_off;
    r.coef_idx = base + (size_t)b * 64;
    // scan order (encoder.ml:476-505): MCU rows, MCUs, components, v x h blocks inside the MCU
    const int mx = bx / K.h, sx = bx - mx * K.h, my = by / K.v, sy = by - my * K.v;
    // blocks outside the MCU grid (planes larger than the grid) are never coded
    if (mx >= P.mbs_wide || my >= P.mbs_high) r.active = false;
    r.scan = (unsigned)(my * P.mbs_wide + mx) * (unsigned)P.blocks_per_mcu + (unsigned)(K.mcu_base + sy * K.h + sx);
    // predictor: the block coded just before this one in the same component
    const int hv = K.h * K.v;
    const int ord = (my * P.mbs_wide + mx) * hv + sy * K.h + sx;
    r.has_pred = ord > 0;
    r.mcu = (unsigned)(my * P.mbs_wide + mx);
    // a component has no predictor at its first block of a restart interval
    if (RST && sy == 0 && sx == 0 && r.mcu % (unsigned)P.restart == 0) r.has_pred = false;
    const int po = r.has_pred ? ord - 1 : 0;
    const int pm = po / hv, pr = po - pm * hv;
    const int psy = pr / K.h, psx = pr - psy * K.h;
    const int pmy = pm / P.mbs_wide, pmx = pm - pmy * P.mbs_wide;
    r.pred_idx = base + ((size_t)(pmy * K.v + psy) * K.bw + (size_t)(pmx * K.h + psx)) * 64;
    return r;
}

// walk_block, LenSink / EmitSink / HistSink and load_record: hvc_huff_dev.h (shared with the mixed coder, hvc_huff_mixed.hip)

__device__ __forceinline__ void load_tables(const HuffParams &P, int frame, unsigned *lds) {
    const unsigned *t = P.tables + (size_t)frame * P.table_stride; // table_stride 0: the default tables of every frame
    for (int i = threadIdx.x; i < 2 * 272; i += HT) lds[i] = t[i]; // both table sets
}

__device__ __forceinline__ void load_block(const HuffParams &P, const BlockPos &b, unsigned (&w)[32]) {
    load_record(P.coefs + b.coef_idx, w);
}

} // namespace

// pass 1 ---------------------------------------------------------------------------------------
namespace {
template <bool RST>
__device__ __forceinline__ void huff_len_body(const HuffParams &P) {
    __shared__ unsigned tabs[2 * 272];
    const int lane = threadIdx.x, frame = blockIdx.y;
    load_tables(P, frame, tabs);
    __syncthreads();
    const BlockPos b = locate_block<RST>(P, frame, blockIdx.x, lane);
    unsigned w[32];
    load_block(P, b, w);
    const int pred = b.has_pred ? (int)P.coefs[b.pred_idx] : 0;
    LenSink s;
    s.tab = tabs + 272 * P.comp[b.comp].table;
    unsigned err = 0;
    walk_block(w, pred, s, err);
    if (b.active) {
        P.lens[(size_t)frame * P.blocks_per_frame + b.scan] = s.bits;
        if (err) atomicOr(P.status, 1u);
    }
}
} // namespace
__global__ __launch_bounds__(HT) void k_huff_len(HuffParams P) { huff_len_body<false>(P); }
__global__ __launch_bounds__(HT) void k_huff_len_rst(HuffParams P) { huff_len_body<true>(P); }

// pass 3 ---------------------------------------------------------------------------------------
namespace {
template <bool RST>
__device__ __forceinline__ void huff_emit_body(const HuffParams &P) {
    __shared__ unsigned tabs[2 * 272];
    const int lane = threadIdx.x, frame = blockIdx.y;
    load_tables(P, frame, tabs);
    __syncthreads();
    const BlockPos b = locate_block<RST>(P, frame, blockIdx.x, lane);
    if (!b.active) return;
    if ((size_t)((P.frame_bits[frame] + 31u) >> 5) + 1 > P.bitbuf_words) return; // flagged by k_frame_sizes
    unsigned w[32];
    load_block(P, b, w);
    const int pred = b.has_pred ? (int)P.coefs[b.pred_idx] : 0;
    const size_t li = (size_t)frame * P.blocks_per_frame + b.scan;
    unsigned bitpos = P.lens[li]; // exclusive offset after pass 2
    const unsigned per_ivl = RST ? (unsigned)P.restart * (unsigned)P.blocks_per_mcu : 0u; // blocks per interval
    if (RST) { // the interval's byte base (pass 2b) + the block's offset inside its interval
        const unsigned j = b.mcu / (unsigned)P.restart;
        bitpos = 8u * P.ivl[(size_t)frame * P.n_intervals + j] + (bitpos - P.lens[li - b.scan + j * per_ivl]);
    }
    EmitSink s;
    s.tab = tabs + 272 * P.comp[b.comp].table;
    s.init(P.bitbuf + (size_t)frame * P.bitbuf_words, bitpos);
    unsigned err = 0;
    walk_block(w, pred, s, err);
    if (RST) {
        // the last block of every interval pads to a byte with ones (T.81 B.2.4.4 in front of RSTn, flush_with_1s at the
        // end); the sink's pending bits say where in its byte the block ended (words are whole bytes)
        if (b.scan + 1 == P.blocks_per_frame || (b.scan + 1) % per_ivl == 0) {
            const int pad = (8 - (s.n & 7)) & 7;
            if (pad) s.put((1u << pad) - 1u, pad);
        }
    } else if (b.scan == P.blocks_per_frame - 1) {
        // Bitstream_writer.flush_with_1s (bitstream_writer.ml:45-49): pad the last byte with ones
        const unsigned total = P.frame_bits[frame];
        const int pad = (int)((8u - (total & 7u)) & 7u);
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
}
} // namespace
__global__ __launch_bounds__(HT) void k_huff_emit(HuffParams P) { huff_emit_body<false>(P); }
__global__ __launch_bounds__(HT) void k_huff_emit_rst(HuffParams P) { huff_emit_body<true>(P); }

// optimised tables, pass 0a: symbol counts per frame and table set.  A workgroup walks every gridDim.x-th tile of its frame
// and counts into LDS bins; at the end it adds its non-zero bins to the frame's counters (zeroed by hipMemsetAsync).
namespace {
template <bool RST>
__device__ __forceinline__ void huff_hist_body(const HuffParams &P) {
    __shared__ unsigned bins[2 * 272];
    const int lane = threadIdx.x, frame = blockIdx.y;
    for (int i = lane; i < 2 * 272; i += HT) bins[i] = 0;
    __syncthreads();
    for (int tile = blockIdx.x; tile < P.tiles_per_frame; tile += gridDim.x) {
        const BlockPos b = locate_block<RST>(P, frame, tile, lane);
        HistSink s;
        s.bins = bins + 272 * P.comp[b.comp].table; // (one component per tile: the same for the whole workgroup)
        if (b.active) {
            unsigned w[32];
            load_block(P, b, w);
            const int pred = b.has_pred ? (int)P.coefs[b.pred_idx] : 0;
            unsigned err = 0; // (k_huff_len reports it)
            walk_block(w, pred, s, err);
        }
        const unsigned long long eob = __ballot(s.eob);
        if ((lane & 63) == 0 && eob) atomicAdd(s.bins + 16, (unsigned)__popcll(eob));
    }
    __syncthreads();
    unsigned *h = P.hist + (size_t)frame * HUFF_TABLE_WORDS;
    for (int i = lane; i < 2 * 272; i += HT)
        if (bins[i]) atomicAdd(h + i, bins[i]);
}
} // namespace
__global__ __launch_bounds__(HT) void k_huff_hist(HuffParams P) { huff_hist_body<false>(P); }
__global__ __launch_bounds__(HT) void k_huff_hist_rst(HuffParams P) { huff_hist_body<true>(P); }

namespace {
// the two smallest keys of the wave, (lo, hi) per lane -> every lane
__device__ __forceinline__ void wave_min2(unsigned long long &lo, unsigned long long &hi) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long ol = __shfl_xor(lo, o), oh = __shfl_xor(hi, o);
        const unsigned long long nl = lo < ol ? lo : ol, mx = lo < ol ? ol : lo;
        const unsigned long long m2 = hi < oh ? hi : oh;
        hi = mx < m2 ? mx : m2;
        lo = nl;
    }
}
} // namespace

// optimised tables, pass 0b: one wavefront per (frame, table), table = blockIdx.x: 0 DC0, 1 DC1, 2 AC0, 3 AC1.
// ITU-T T.81 Annex K.2 as hvc_huffman_spec_from_counts computes it.  Lane l holds symbols l, l + 64, ... l + 256 (256 = the
// reserved symbol, count 1).  Merge step: the smallest key (count << 9) | (511 - index) is c1 (the largest index among the
// smallest counts), the next smallest c2.  Code sizes: a symbol is labelled with the root of its subtree, the one symbol
// of it whose count is non-zero; every member of both groups gets + 1 and c2's group becomes c1's -- what K.2's `others`
// chains do, without walking them.  Then figure K.3 on lane 0, HUFFVAL by (unadjusted size, symbol), canonical codes.
// Counts fit in 32 bits: huffman_prepare bounds a frame at 2^32 bits, and every symbol takes at least one.
__global__ __launch_bounds__(64) void k_huff_build(HuffParams P) {
    __shared__ unsigned cs_s[260];   // unadjusted code sizes (257 used)
    __shared__ int bits[64], maxlen_s, cum[18];
    __shared__ unsigned firstcode[18];
    __shared__ unsigned spec_w[sizeof(hvc_huff_spec) / 4];
    const int lane = threadIdx.x, t = blockIdx.x, frame = blockIdx.y;
    const int set = t & 1, ac = t >> 1, nsym = ac ? 256 : 16;
    const unsigned *h = P.hist + (size_t)frame * HUFF_TABLE_WORDS + 272 * set + (ac ? 16 : 0);
    unsigned f[5], lab[5], cs[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int i = lane + 64 * k;
        f[k] = i < nsym ? h[i] : (i == 256 ? 1u : 0u);
        lab[k] = (unsigned)i;
        cs[k] = 0;
    }
    for (;;) {
        unsigned long long lo = ~0ull, hi = ~0ull;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const unsigned long long key = f[k] ? ((unsigned long long)f[k] << 9) | (unsigned)(511 - (lane + 64 * k)) : ~0ull;
            if (key < lo) {
                hi = lo;
                lo = key;
            } else if (key < hi) {
                hi = key;
            }
        }
        wave_min2(lo, hi);
        if (hi == ~0ull) break; // one tree left
        const unsigned c1 = 511u - (unsigned)(lo & 511u), c2 = 511u - (unsigned)(hi & 511u);
        const unsigned f2 = (unsigned)(hi >> 9);
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const unsigned i = (unsigned)(lane + 64 * k);
            if (lab[k] == c1 || lab[k] == c2) {
                cs[k]++;
                lab[k] = c1;
            }
            if (i == c1) f[k] += f2;
            if (i == c2) f[k] = 0;
        }
    }
    bits[lane] = 0;
    if (lane == 0) maxlen_s = 0;
    for (int i = lane; i < (int)(sizeof spec_w / 4); i += 64) spec_w[i] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int i = lane + 64 * k;
        if (i < 257) {
            cs_s[i] = cs[k];
            if (cs[k]) {
                atomicAdd(&bits[cs[k] < 63 ? cs[k] : 63], 1); // (sizes stay below 50 for 32-bit counts)
                atomicMax(&maxlen_s, (int)cs[k]);
            }
        }
    }
    __syncthreads();
    // HUFFVAL position of each symbol < 256: the coded symbols of smaller size, and those of equal size and smaller index
    unsigned pos[4] = {0, 0, 0, 0};
    for (int i = 0; i < 256; i++) {
        const unsigned c = cs_s[i];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned mine = cs[k];
            pos[k] += (c && (c < mine || (c == mine && i < lane + 64 * k))) ? 1u : 0u;
        }
    }
    uint8_t *sb = reinterpret_cast<uint8_t *>(spec_w);
    if (lane == 0) {
        // figure K.3: no code longer than 16 bits; then the reserved symbol's code leaves the longest length
        for (int i = maxlen_s < 63 ? maxlen_s : 63; i > 16; i--)
            while (bits[i] > 0) {
                int j = i - 2;
                while (bits[j] == 0) j--;
                bits[i] -= 2;
                bits[i - 1]++;
                bits[j + 1] += 2;
                bits[j]--;
            }
        int i = 16;
        while (i > 0 && bits[i] == 0) i--; // (i = 0: no symbol counted at all, which huffman_prepare does not let through)
        if (i) bits[i]--;
        // canonical codes (tables.ml:27-45)
        int n = 0;
        unsigned code = 0;
        cum[0] = 0;
        for (int l = 1; l <= 16; l++) {
            sb[l - 1] = (uint8_t)bits[l];
            firstcode[l] = code;
            n += bits[l];
            cum[l] = n;
            code = (code + (unsigned)bits[l]) << 1;
        }
        sb[offsetof(hvc_huff_spec, n_vals)] = (uint8_t)(n & 255);
        sb[offsetof(hvc_huff_spec, n_vals) + 1] = (uint8_t)(n >> 8);
    }
    __syncthreads();
    unsigned *tab = P.opt_tables + (size_t)frame * HUFF_TABLE_WORDS + 272 * set + (ac ? 16 : 0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = lane + 64 * k;
        unsigned e = 0;
        if (cs[k] && i < 256) {
            const int p = (int)pos[k];
            sb[offsetof(hvc_huff_spec, vals) + p] = (uint8_t)i;
            int l = 1;
            while (l < 16 && p >= cum[l]) l++;
            e = ((firstcode[l] + (unsigned)(p - cum[l - 1])) << 5) | (unsigned)l;
        }
        if (i < nsym) tab[i] = e;
    }
    __syncthreads();
    unsigned *dst = reinterpret_cast<unsigned *>(P.specs + (size_t)frame * 4 + t);
    for (int i = lane; i < (int)(sizeof spec_w / 4); i += 64) dst[i] = spec_w[i];
}

// pass 2 / 4b: per-frame exclusive scan of n[frame] 32-bit values (in place), total -> totals[frame].
// One workgroup of 1024 lanes per frame; 4 values per lane per round.
__global__ __launch_bounds__(1024) void k_scan_u32(unsigned *data, size_t stride, const unsigned *counts, unsigned fixed_count,
                                                   unsigned *totals) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned carry_s;
    const int frame = blockIdx.x, lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
    unsigned *d = data + (size_t)frame * stride;
    const unsigned n = counts ? counts[frame] : fixed_count;
    if (lane == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < n; base += 4096) {
        const unsigned i0 = base + 4u * (unsigned)lane;
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (i0 + k < n) ? d[i0 + k] : 0u;
        const unsigned mine = v[0] + v[1] + v[2] + v[3];
        // inclusive scan of `mine` inside the wave
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(incl, o);
            if (wl >= o) incl += t;
        }
        if (wl == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned wbase = 0;
        for (int k = 0; k < wave; k++) wbase += wsum[k];
        unsigned run = carry_s + wbase + incl - mine;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) d[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (lane == 1023) carry_s = run; // run of the last lane = carry + everything of this round
        __syncthreads();
    }
    if (lane == 0) totals[frame] = carry_s;
}

// After pass 2: bytes of every frame's unstuffed segment and the number of 64-byte pieces.
__global__ void k_frame_sizes(HuffParams P) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= P.n_frames) return;
    const unsigned bits = P.frame_bits[f];
    const unsigned bytes = (bits + 7u) >> 3;
    P.frame_bytes[f] = bytes;
    P.frame_pieces[f] = (bytes + 63u) >> 6;
    if ((size_t)((bits + 31u) >> 5) + 1 > P.bitbuf_words) atomicOr(P.status, 2u); // cannot happen: worst case sized
}

// restart intervals, pass 2b: bytes of every interval from the frame-wide bit offsets of pass 2; one interval per lane
__global__ __launch_bounds__(256) void k_ivl_bytes(HuffParams P) {
    const int frame = blockIdx.y;
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= P.n_intervals) return;
    const unsigned per_ivl = (unsigned)P.restart * (unsigned)P.blocks_per_mcu;
    const unsigned *l = P.lens + (size_t)frame * P.blocks_per_frame;
    const unsigned first = j * per_ivl, next = first + per_ivl;
    const unsigned end = next < P.blocks_per_frame ? l[next] : P.frame_bits[frame];
    P.ivl[(size_t)frame * P.n_intervals + j] = (end - l[first] + 7u) >> 3;
}

// ... and behind the scan over them (frame_bytes = the sum): the padded segment's bits and pieces
__global__ void k_frame_sizes_rst(HuffParams P) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= P.n_frames) return;
    const unsigned bytes = P.frame_bytes[f];
    P.frame_bits[f] = bytes * 8u; // (huffman_prepare bounds it below 2^32)
    P.frame_pieces[f] = (bytes + 63u) >> 6;
    if ((size_t)((bytes + 3u) >> 2) + 1 > P.bitbuf_words) atomicOr(P.status, 2u); // cannot happen: worst case sized
}

namespace {
// the first interval j in [1, n) whose byte base is >= key (n when there is none): base[1 ..] is strictly increasing,
// every interval holding at least one byte
__device__ __forceinline__ unsigned ivl_lower_bound(const unsigned *base, unsigned n, unsigned key) {
    unsigned lo = 1, hi = n;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (base[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

} // namespace

// pass 4a: number of 0xFF bytes in every 64-byte piece
__global__ __launch_bounds__(256) void k_ff_count(HuffParams P) {
    const int frame = blockIdx.y;
    const unsigned piece = blockIdx.x * 256u + threadIdx.x;
    if (piece >= P.frame_pieces[frame]) return;
    const unsigned bytes = P.frame_bytes[frame];
    const uint4 *src = reinterpret_cast<const uint4 *>(P.bitbuf + (size_t)frame * P.bitbuf_words) + (size_t)piece * 4;
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 t = src[j];
        const unsigned ws[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned pos = piece * 64u + (unsigned)(j * 16 + k * 4);
#pragma unroll
            for (int bb = 0; bb < 4; bb++)
                cnt += (pos + bb < bytes && ((ws[k] >> (8 * bb)) & 0xffu) == 0xffu) ? 1u : 0u;
        }
    }
    P.ff[(size_t)frame * P.ff_stride + piece] = cnt;
}

// restart intervals, pass 4a: behind k_ff_count (left as it is), + 2 for every interval boundary inside the piece (the
// marker in front of the interval's first byte)
__global__ __launch_bounds__(256) void k_ff_marks(HuffParams P) {
    const int frame = blockIdx.y;
    const unsigned piece = blockIdx.x * 256u + threadIdx.x;
    if (piece >= P.frame_pieces[frame]) return;
    const unsigned *base = P.ivl + (size_t)frame * P.n_intervals;
    const unsigned marks = ivl_lower_bound(base, P.n_intervals, piece * 64u + 64u) - ivl_lower_bound(base, P.n_intervals, piece * 64u);
    if (marks) P.ff[(size_t)frame * P.ff_stride + piece] += 2u * marks;
}

// pass 4c: offsets of the frames' stuffed segments inside the packed output (n_frames is small)
__global__ void k_frame_offsets(HuffParams P) {
    if (blockIdx.x || threadIdx.x) return;
    unsigned long long off = 0;
    for (int f = 0; f < P.n_frames; f++) {
        P.out_offsets[f] = off;
        off += (unsigned long long)P.frame_bytes[f] + P.frame_ff[f];
    }
    P.out_offsets[P.n_frames] = off;
    if (off > P.out_cap) atomicOr(P.status, 4u);
}

// pass 4d: copy with stuffing; one 64-byte piece per lane.  RST: ff counts the markers' bytes too, so the straight copy
// is taken by pieces without an 0xFF and without a boundary, and the byte-wise path writes FF Dn in front of every
// interval's first byte (D0 + (j - 1) mod 8 in front of interval j)
namespace {
template <bool RST>
__device__ __forceinline__ void stuff_write_body(const HuffParams &P) {
    const int frame = blockIdx.y;
    const unsigned piece = blockIdx.x * 256u + threadIdx.x;
    if (piece >= P.frame_pieces[frame]) return;
    if (P.out_offsets[P.n_frames] > P.out_cap) return;
    const unsigned bytes = P.frame_bytes[frame];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(P.bitbuf + (size_t)frame * P.bitbuf_words) + (size_t)piece * 64;
    uint8_t *dst = P.out + P.out_offsets[frame] + (size_t)piece * 64 + P.ff[(size_t)frame * P.ff_stride + piece];
    const unsigned n = min(64u, bytes - piece * 64u);
    const unsigned nff = (piece + 1 < P.frame_pieces[frame] ? P.ff[(size_t)frame * P.ff_stride + piece + 1]
                                                            : P.frame_ff[frame]) -
                         P.ff[(size_t)frame * P.ff_stride + piece];
    if (nff == 0 && n == 64) {
        // four out of five pieces hold no 0xFF: a straight copy, dwords at whatever alignment the
        // earlier stuffing bytes left (global memory takes unaligned dwords)
        typedef unsigned unaligned_u32 __attribute__((aligned(1)));
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        unaligned_u32 *d = reinterpret_cast<unaligned_u32 *>(dst);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint4 t = s4[j];
            d[4 * j + 0] = t.x;
            d[4 * j + 1] = t.y;
            d[4 * j + 2] = t.z;
            d[4 * j + 3] = t.w;
        }
        return;
    }
    const unsigned *base = RST ? P.ivl + (size_t)frame * P.n_intervals : nullptr;
    unsigned jb = RST ? ivl_lower_bound(base, P.n_intervals, piece * 64u) : 0u;
    unsigned nextb = RST && jb < P.n_intervals ? base[jb] - piece * 64u : ~0u; // the next boundary, relative to the piece
    for (unsigned i = 0; i < n; i++) {
        if (RST && i == nextb) {
            *dst++ = 0xff;
            *dst++ = (uint8_t)(0xd0u + ((jb - 1u) & 7u));
            jb++;
            nextb = jb < P.n_intervals ? base[jb] - piece * 64u : ~0u;
        }
        const uint8_t v = src[i];
        *dst++ = v;
        if (v == 0xff) *dst++ = 0;
    }
}
} // namespace
__global__ __launch_bounds__(256) void k_stuff_write(HuffParams P) { stuff_write_body<false>(P); }
__global__ __launch_bounds__(256) void k_stuff_write_rst(HuffParams P) { stuff_write_body<true>(P); }

// the passes with a restart interval (the memsets of status and bitbuf are the caller's, launch_huffman_encode)
static hipError_t launch_huffman_encode_rst(const HuffParams &P, const dim3 grid, hipStream_t s) {
    if (P.hist) {
        const hipError_t e = hipMemsetAsync(P.hist, 0, (size_t)P.n_frames * HUFF_TABLE_WORDS * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        int per = HIST_GROUPS / P.n_frames;
        per = per < 1 ? 1 : (per > P.tiles_per_frame ? P.tiles_per_frame : per);
        hipLaunchKernelGGL(k_huff_hist_rst, dim3((unsigned)per, (unsigned)P.n_frames, 1), dim3(HT), 0, s, P);
        hipLaunchKernelGGL(k_huff_build, dim3(4, (unsigned)P.n_frames, 1), dim3(64), 0, s, P);
    }
    hipLaunchKernelGGL(k_huff_len_rst, grid, dim3(HT), 0, s, P);
    hipLaunchKernelGGL(k_scan_u32, dim3((unsigned)P.n_frames), dim3(1024), 0, s, P.lens, (size_t)P.blocks_per_frame,
                       (const unsigned *)nullptr, P.blocks_per_frame, P.frame_bits);
    hipLaunchKernelGGL(k_ivl_bytes, dim3((P.n_intervals + 255u) / 256u, (unsigned)P.n_frames, 1), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_scan_u32, dim3((unsigned)P.n_frames), dim3(1024), 0, s, P.ivl, (size_t)P.n_intervals,
                       (const unsigned *)nullptr, P.n_intervals, P.frame_bytes);
    hipLaunchKernelGGL(k_frame_sizes_rst, dim3((unsigned)((P.n_frames + 63) / 64)), dim3(64), 0, s, P);
    hipLaunchKernelGGL(k_huff_emit_rst, grid, dim3(HT), 0, s, P);
    const unsigned max_pieces = (unsigned)((P.bitbuf_words * 4 + 63) / 64);
    const dim3 pgrid((max_pieces + 255u) / 256u, (unsigned)P.n_frames, 1);
    hipLaunchKernelGGL(k_ff_count, pgrid, dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_ff_marks, pgrid, dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_scan_u32, dim3((unsigned)P.n_frames), dim3(1024), 0, s, P.ff, P.ff_stride,
                       (const unsigned *)P.frame_pieces, 0u, P.frame_ff);
    hipLaunchKernelGGL(k_frame_offsets, dim3(1), dim3(1), 0, s, P);
    hipLaunchKernelGGL(k_stuff_write_rst, pgrid, dim3(256), 0, s, P);
    return hipGetLastError();
}

// k_huff_build alone, for the mixed coder (hvc_huff_mixed.hip): it reads P.hist, P.opt_tables, P.specs and P.n_frames only
hipError_t launch_huffman_build(const HuffParams &P, hipStream_t s) {
    if (P.n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_huff_build, dim3(4, (unsigned)P.n_frames, 1), dim3(64), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_huffman_encode(const HuffParams &P, hipStream_t s) {
    if (P.n_frames <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(P.status, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(P.bitbuf, 0, (size_t)P.n_frames * P.bitbuf_words * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    if (P.restart > 0) return launch_huffman_encode_rst(P, grid, s);
    if (P.hist) { // the frames' own tables
        e = hipMemsetAsync(P.hist, 0, (size_t)P.n_frames * HUFF_TABLE_WORDS * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        int per = HIST_GROUPS / P.n_frames;
        per = per < 1 ? 1 : (per > P.tiles_per_frame ? P.tiles_per_frame : per);
        hipLaunchKernelGGL(k_huff_hist, dim3((unsigned)per, (unsigned)P.n_frames, 1), dim3(HT), 0, s, P);
        hipLaunchKernelGGL(k_huff_build, dim3(4, (unsigned)P.n_frames, 1), dim3(64), 0, s, P);
    }
    hipLaunchKernelGGL(k_huff_len, grid, dim3(HT), 0, s, P);
    hipLaunchKernelGGL(k_scan_u32, dim3((unsigned)P.n_frames), dim3(1024), 0, s, P.lens, (size_t)P.blocks_per_frame,
                       (const unsigned *)nullptr, P.blocks_per_frame, P.frame_bits);
    hipLaunchKernelGGL(k_frame_sizes, dim3((unsigned)((P.n_frames + 63) / 64)), dim3(64), 0, s, P);
    hipLaunchKernelGGL(k_huff_emit, grid, dim3(HT), 0, s, P);
    const unsigned max_pieces = (unsigned)((P.bitbuf_words * 4 + 63) / 64);
    const dim3 pgrid((max_pieces + 255u) / 256u, (unsigned)P.n_frames, 1);
    hipLaunchKernelGGL(k_ff_count, pgrid, dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_scan_u32, dim3((unsigned)P.n_frames), dim3(1024), 0, s, P.ff, P.ff_stride,
                       (const unsigned *)P.frame_pieces, 0u, P.frame_ff);
    hipLaunchKernelGGL(k_frame_offsets, dim3(1), dim3(1), 0, s, P);
    hipLaunchKernelGGL(k_stuff_write, pgrid, dim3(256), 0, s, P);
    return hipGetLastError();
}

} // namespace hvc
