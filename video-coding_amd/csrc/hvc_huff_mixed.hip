// hvc_huff_mixed.hip -- baseline Huffman coding of the coefficient records of frames of DIFFERENT geometry in one chain of
// launches (gfx950): hvc_huff.hip's passes with the geometry taken from device memory instead of HuffParams.
//
// The decomposition is k_encode_mixed's / k_decode_mixed's (hvc_huff_mixed_plan.h): a work unit is 64 consecutive blocks of
// ONE plane of one file = one wavefront, HVC_MIXED_GROUP units per workgroup.  map[unit] names the plane, the plane
// descriptor its file; the unit index goes through readfirstlane, so both descriptors are wave-uniform and come through
// scalar loads.  The symbol walk and its sinks are the uniform coder's own (hvc_huff_dev.h), locate()'s arithmetic is
// locate_block's: scan index, predictor block, blocks outside the MCU grid inactive.
//   0a k_hm_hist        (optimised tables) symbol counts: LDS bins per WAVEFRONT (the four units of a workgroup may belong
//                       to four files), EOB by ballot, one flush of the non-zero bins to the file's counters
//   0b k_huff_build     hvc_huff.hip's, as it stands: one wavefront per (file, table)
//   1  k_hm_len         bit length of every block's code -> lens[file's base + scan index]; a value without a code flags
//                       the FILE (file_status bit 0).  Each wavefront stages the one table set of its plane.
//   2  k_hm_scan<0>     per file (one workgroup each, base and count from the descriptor; rounds of 1024 values) the
//                       exclusive scan of its lengths, then its bits, bytes and pieces; a flagged file gets 0 bits
//   2c k_hm_file_scan<0> exclusive scan of the files' piece counts -> piece_base (one workgroup, 1024 files per round)
//   3  k_hm_emit        the walk again, writing the bits at the block's offset of the file's own bit buffer (which starts on
//                       a 64-byte piece: no word is shared between files); the last coded block pads with ones; a flagged
//                       file is skipped
//   4a k_hm_ff_count    0xFF bytes of every 64-byte piece         4b k_hm_scan<1>  their scan per file
//   4c k_hm_file_scan<1> the packed output offsets of the files: a scan over the files' byte totals (a chunk of thumbnails
//                       holds thousands of files; k_frame_offsets walks them on one lane)
//   4d k_hm_stuff       the stuffed copy, one piece per lane
// The piece passes (4a, 4d) run over the chunk's pieces, not over a (pieces, files) grid: how many pieces a file has is known
// only on the device, behind pass 2, so a piece map like the unit map would have to be sized for the worst case (216 bytes per
// block against the ten or twenty a block takes) or built by one more kernel.  Instead pass 2c makes the DENSE piece bases of
// the files, lane p of the piece grid takes piece p of the chunk and finds its file by a binary search over those bases
// (at most 16 steps over an array that stays in cache), and the lanes past the chunk's last piece -- the grid is sized from
// the buffer -- leave after one load.  No grid row per file, no idle row for a file of one piece.
// Status is one word per file; the launch's own word only says that `out` is too small (nothing is written then).
// Not here: restart intervals (the entry points hand such calls to the host coder).
// LDS per workgroup: 4352 bytes (k_hm_hist, k_hm_len, k_hm_emit: 4 x 272 words), 20 (k_hm_scan), 136 (k_hm_file_scan); no
// scratch; registers: profiles/mixed_coder_rocprofv3.txt.
#include <cstring>

#include "hvc_huff_mixed.h"
#include "hvc_huff_dev.h"

namespace hvc {
namespace {

constexpr int HM_LANES = HVC_MIXED_UNIT * HVC_MIXED_GROUP;
constexpr int HM_SET = 16 + 256; // words of one table set

struct BlockPosM {
    bool active;
    unsigned scan;   // index of the block in scan order inside its file
    size_t coef_idx; // int16 element index of the block's coefficients
    size_t pred_idx; // ... of the block whose DC is the predictor (valid when has_pred)
    bool has_pred;
};

// locate_block of hvc_huff.hip with the plane and the file from their descriptors; b = the block inside the plane
__device__ __forceinline__ BlockPosM locate(const HuffMixedFileK &F, const HuffMixedPlaneK &K, int b) {
    BlockPosM r;
    r.active = b < K.nblk;
    b = r.active ? b : K.nblk - 1;
    const int by = b / K.bw, bx = b - by * K.bw;
    r.coef_idx = (size_t)K.coef_base + (size_t)b * 64;
    // scan order (encoder.ml:476-505): MCU rows, MCUs, components, v x h blocks inside the MCU
    const int mx = bx / K.h, sx = bx - mx * K.h, my = by / K.v, sy = by - my * K.v;
    // blocks outside the MCU grid (planes larger than the grid) are never coded
    if (mx >= F.mbs_wide || my >= F.mbs_high) r.active = false;
    r.scan = (unsigned)(my * F.mbs_wide + mx) * (unsigned)F.blocks_per_mcu + (unsigned)(K.mcu_base + sy * K.h + sx);
    // predictor: the block coded just before this one in the same component
    const int hv = K.h * K.v;
    const int ord = (my * F.mbs_wide + mx) * hv + sy * K.h + sx;
    r.has_pred = ord > 0;
    const int po = r.has_pred ? ord - 1 : 0;
    const int pm = po / hv, pr = po - pm * hv;
    const int psy = pr / K.h, psx = pr - psy * K.h;
    const int pmy = pm / F.mbs_wide, pmx = pm - pmy * F.mbs_wide;
    r.pred_idx = (size_t)K.coef_base + ((size_t)(pmy * K.v + psy) * K.bw + (size_t)(pmx * K.h + psx)) * 64;
    return r;
}

// the wavefront's own LDS region is written by some lanes and read by others: the wave's ds operations complete in order,
// the compiler is told not to move anything across
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the work unit of this wavefront, wave-uniform; false: a spare unit of the last workgroup (the whole wavefront leaves)
__device__ __forceinline__ bool unit_of_wave(const HuffMixedParams &P, unsigned &unit, int &wv, int &l) {
    wv = (int)(threadIdx.x >> 6);
    l = (int)(threadIdx.x & (HVC_MIXED_UNIT - 1));
    unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * HVC_MIXED_GROUP + (unsigned)wv));
    return unit < P.n_units;
}

// the table set of plane K's file into the wavefront's LDS region
__device__ __forceinline__ void stage_tables(const HuffMixedParams &P, const HuffMixedPlaneK &K, unsigned *lds, int l) {
    const unsigned *t = P.tables + (size_t)K.file * P.table_stride + (size_t)(HM_SET * K.table);
    for (int i = l; i < HM_SET; i += HVC_MIXED_UNIT) lds[i] = t[i];
    wave_sync();
}

} // namespace

// pass 0a ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_LANES) void k_hm_hist(HuffMixedParams P) {
    __shared__ unsigned bins[HVC_MIXED_GROUP][HM_SET];
    unsigned unit;
    int wv, l;
    if (!unit_of_wave(P, unit, wv, l)) return; // (no workgroup barrier below)
    const HuffMixedPlaneK K = P.planes[P.map[unit]];
    const HuffMixedFileK F = P.files[K.file];
    unsigned *mine = bins[wv];
    for (int i = l; i < HM_SET; i += HVC_MIXED_UNIT) mine[i] = 0;
    wave_sync();
    const BlockPosM b = locate(F, K, (int)(unit - K.unit0) * HVC_MIXED_UNIT + l);
    HistSink s;
    s.bins = mine;
    if (b.active) {
        unsigned w[32];
        load_record(P.coefs + b.coef_idx, w);
        const int pred = b.has_pred ? (int)P.coefs[b.pred_idx] : 0;
        unsigned err = 0; // (k_hm_len reports it)
        walk_block(w, pred, s, err);
    }
    const unsigned long long eob = __ballot(s.eob);
    if (l == 0 && eob) atomicAdd(mine + 16, (unsigned)__popcll(eob));
    wave_sync();
    unsigned *h = P.hist + (size_t)K.file * HUFF_TABLE_WORDS + (size_t)(HM_SET * K.table);
    for (int i = l; i < HM_SET; i += HVC_MIXED_UNIT)
        if (mine[i]) atomicAdd(h + i, mine[i]);
}

// pass 1 ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_LANES) void k_hm_len(HuffMixedParams P) {
    __shared__ unsigned tabs[HVC_MIXED_GROUP][HM_SET];
    unsigned unit;
    int wv, l;
    if (!unit_of_wave(P, unit, wv, l)) return;
    const HuffMixedPlaneK K = P.planes[P.map[unit]];
    const HuffMixedFileK F = P.files[K.file];
    stage_tables(P, K, tabs[wv], l);
    const BlockPosM b = locate(F, K, (int)(unit - K.unit0) * HVC_MIXED_UNIT + l);
    if (!b.active) return;
    unsigned w[32];
    load_record(P.coefs + b.coef_idx, w);
    const int pred = b.has_pred ? (int)P.coefs[b.pred_idx] : 0;
    LenSink s;
    s.tab = tabs[wv];
    unsigned err = 0;
    walk_block(w, pred, s, err);
    P.lens[(size_t)F.lens_base + b.scan] = s.bits; // (scan < F.blocks: the block lies inside the MCU grid)
    if (err) atomicOr(P.file_status + K.file, 1u);
}

// pass 3 ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_LANES) void k_hm_emit(HuffMixedParams P) {
    __shared__ unsigned tabs[HVC_MIXED_GROUP][HM_SET];
    unsigned unit;
    int wv, l;
    if (!unit_of_wave(P, unit, wv, l)) return;
    const HuffMixedPlaneK K = P.planes[P.map[unit]];
    const HuffMixedFileK F = P.files[K.file];
    if (P.file_status[K.file]) return; // a flagged file contributes nothing (its bit total is 0: k_hm_scan)
    stage_tables(P, K, tabs[wv], l);
    const BlockPosM b = locate(F, K, (int)(unit - K.unit0) * HVC_MIXED_UNIT + l);
    if (!b.active) return;
    unsigned w[32];
    load_record(P.coefs + b.coef_idx, w);
    const int pred = b.has_pred ? (int)P.coefs[b.pred_idx] : 0;
    const unsigned bitpos = P.lens[(size_t)F.lens_base + b.scan]; // exclusive offset after pass 2
    EmitSink s;
    s.tab = tabs[wv];
    s.init(P.bitbuf + (size_t)F.bitbuf_base, bitpos);
    unsigned err = 0;
    walk_block(w, pred, s, err);
    if (b.scan == F.blocks - 1) {
        // Bitstream_writer.flush_with_1s (bitstream_writer.ml:45-49): pad the last byte with ones
        const unsigned total = P.file_bits[K.file];
        const int pad = (int)((8u - (total & 7u)) & 7u);
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
}

// pass 2 / 4b: per-file exclusive scan (in place), one workgroup of 256 lanes per file, 4 values per lane per round.
// MODE 0: the file's lengths -> bit offsets; total -> its bits, bytes, pieces (0 for a flagged file).
// MODE 1: the 0xFF counts of its pieces -> offsets; total -> file_ff.
template <int MODE>
__global__ __launch_bounds__(256) void k_hm_scan(HuffMixedParams P) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned carry_s;
    const unsigned f = blockIdx.x;
    const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
    const HuffMixedFileK F = P.files[f];
    unsigned *d = MODE == 0 ? P.lens + (size_t)F.lens_base : P.ff + P.piece_base[f];
    const unsigned n = MODE == 0 ? F.blocks : P.file_pieces[f];
    if (lane == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < n; base += 1024) {
        const unsigned i0 = base + 4u * (unsigned)lane;
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (i0 + k < n) ? d[i0 + k] : 0u;
        const unsigned mine = v[0] + v[1] + v[2] + v[3];
        unsigned incl = mine; // inclusive scan of `mine` inside the wave
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
        if (lane == 255) carry_s = run; // run of the last lane = carry + everything of this round
        __syncthreads();
    }
    if (lane != 0) return;
    unsigned total = carry_s;
    if (MODE == 0) {
        unsigned st = P.file_status[f];
        if ((unsigned long long)((total + 31u) >> 5) + 1 > F.bitbuf_words) { // cannot happen: worst case sized
            st |= 2u;
            P.file_status[f] = st;
        }
        if (st) total = 0; // a flagged file holds no bytes: its neighbours close up
        const unsigned bytes = (total + 7u) >> 3;
        P.file_bits[f] = total;
        P.file_bytes[f] = bytes;
        P.file_pieces[f] = (bytes + 63u) >> 6;
    } else {
        P.file_ff[f] = total;
    }
}

// pass 2c / 4c: exclusive scan over the FILES, one workgroup of 1024 lanes, one file per lane per round.
// MODE 0: piece counts -> piece_base[0 .. n_files] (the sum stays below 2^32: every file's pieces lie inside its buffer).
// MODE 1: bytes + 0xFF bytes -> out_offsets[0 .. n_files]; past out_cap: bit 2 of the launch's status.
template <int MODE>
__global__ __launch_bounds__(1024) void k_hm_file_scan(HuffMixedParams P) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry_s;
    const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
    if (lane == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < P.n_files; base += 1024) {
        const unsigned f = base + (unsigned)lane;
        unsigned long long mine = 0;
        if (f < P.n_files) mine = MODE == 0 ? (unsigned long long)P.file_pieces[f] : (unsigned long long)P.file_bytes[f] + P.file_ff[f];
        unsigned long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(incl, o);
            if (wl >= o) incl += t;
        }
        if (wl == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long wbase = 0;
        for (int k = 0; k < wave; k++) wbase += wsum[k];
        const unsigned long long excl = carry_s + wbase + incl - mine;
        if (f < P.n_files) {
            if (MODE == 0)
                P.piece_base[f] = (unsigned)excl;
            else
                P.out_offsets[f] = excl;
        }
        __syncthreads();
        if (lane == 1023) carry_s = excl + mine;
        __syncthreads();
    }
    if (lane != 0) return;
    if (MODE == 0) {
        P.piece_base[P.n_files] = (unsigned)carry_s;
    } else {
        P.out_offsets[P.n_files] = carry_s;
        if (carry_s > P.out_cap) atomicOr(P.status, 4u);
    }
}

namespace {
// the file of piece p of the chunk (p < piece_base[n_files]): the one with piece_base[f] <= p < piece_base[f + 1]
__device__ __forceinline__ unsigned file_of_piece(const unsigned *piece_base, unsigned n_files, unsigned p) {
    unsigned lo = 0, hi = n_files; // the first f whose piece_base[f + 1] is above p
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (piece_base[mid + 1] <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
} // namespace

// pass 4a: number of 0xFF bytes in every 64-byte piece of the chunk
__global__ __launch_bounds__(256) void k_hm_ff_count(HuffMixedParams P) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= P.piece_base[P.n_files]) return; // (<= pieces_cap, what ff holds)
    const unsigned f = file_of_piece(P.piece_base, P.n_files, p);
    const unsigned piece = p - P.piece_base[f];
    const unsigned bytes = P.file_bytes[f];
    const uint4 *src = reinterpret_cast<const uint4 *>(P.bitbuf + (size_t)P.files[f].bitbuf_base) + (size_t)piece * 4;
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
    P.ff[p] = cnt;
}

// pass 4d: copy with stuffing; one 64-byte piece per lane (k_stuff_write's body without the restart markers)
__global__ __launch_bounds__(256) void k_hm_stuff(HuffMixedParams P) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= P.piece_base[P.n_files]) return;
    const unsigned f = file_of_piece(P.piece_base, P.n_files, p);
    // out too small: nothing is written (partial = 0), or only the files that end inside it (the batch pipeline hands the
    // others to the host coder: huff_mixed_hand_back)
    if (P.out_offsets[P.partial ? f + 1 : P.n_files] > P.out_cap) return;
    const unsigned piece = p - P.piece_base[f], pieces = P.file_pieces[f];
    const unsigned bytes = P.file_bytes[f];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(P.bitbuf + (size_t)P.files[f].bitbuf_base) + (size_t)piece * 64;
    const unsigned before = P.ff[p];
    uint8_t *dst = P.out + P.out_offsets[f] + (size_t)piece * 64 + before;
    const unsigned n = min(64u, bytes - piece * 64u);
    const unsigned nff = (piece + 1 < pieces ? P.ff[p + 1] : P.file_ff[f]) - before;
    if (nff == 0 && n == 64) {
        // most pieces hold no 0xFF: a straight copy, dwords at whatever alignment the earlier stuffing bytes left
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
    for (unsigned i = 0; i < n; i++) {
        const uint8_t v = src[i];
        *dst++ = v;
        if (v == 0xff) *dst++ = 0;
    }
}

hipError_t launch_huffman_encode_mixed(const HuffMixedParams &P, hipStream_t s) {
    if (P.n_files == 0 || P.n_units == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(P.status, 0, sizeof(unsigned), s);
    if (e == hipSuccess) e = hipMemsetAsync(P.file_status, 0, (size_t)P.n_files * sizeof(unsigned), s);
    if (e == hipSuccess) e = hipMemsetAsync(P.bitbuf, 0, (size_t)P.bitbuf_words * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const dim3 ugrid((P.n_units + HVC_MIXED_GROUP - 1) / HVC_MIXED_GROUP), pgrid((P.pieces_cap + 255u) / 256u);
    if (P.hist) { // the files' own tables
        e = hipMemsetAsync(P.hist, 0, (size_t)P.n_files * HUFF_TABLE_WORDS * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_hm_hist, ugrid, dim3(HM_LANES), 0, s, P);
        HuffParams B;
        std::memset(&B, 0, sizeof B);
        B.n_frames = (int)P.n_files; // (<= HVC_HUFF_MIXED_MAX_FILES: the plan)
        B.hist = P.hist;
        B.opt_tables = P.opt_tables;
        B.specs = P.specs;
        if ((e = launch_huffman_build(B, s)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_hm_len, ugrid, dim3(HM_LANES), 0, s, P);
    hipLaunchKernelGGL(k_hm_scan<0>, dim3(P.n_files), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_hm_file_scan<0>, dim3(1), dim3(1024), 0, s, P);
    hipLaunchKernelGGL(k_hm_emit, ugrid, dim3(HM_LANES), 0, s, P);
    hipLaunchKernelGGL(k_hm_ff_count, pgrid, dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_hm_scan<1>, dim3(P.n_files), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_hm_file_scan<1>, dim3(1), dim3(1024), 0, s, P);
    hipLaunchKernelGGL(k_hm_stuff, pgrid, dim3(256), 0, s, P);
    return hipGetLastError();
}

} // namespace hvc
