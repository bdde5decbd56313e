// hvc_ctx.h -- what the translation units of the C ABI share (internal; nothing here is exported): the context, the
// helpers every entry point uses, and the few functions one part of the ABI calls in another.
//   hvc_capi.hip         context, streams, timers, memory; the block stage (decode_frames_impl, decode_frames_yuv444_impl,
//                        encode_frames_impl behind the entry points; the staging steps they share) and its divergence calls
//   hvc_capi_jpeg.hip    files: one at a time (hvc_jpeg_decode, _yuv444, _rgb on one skeleton; _scaled, _scaled_rgb; hvc_jpeg_encode,
//                        _encode_rgb) and the batch pipeline with the host reader (hvc_jpeg_decode_batch, _yuv444, _scaled, _rgb)
//   hvc_capi_reader.hip  the GPU Huffman reader's entry point and the batch pipeline built on it (its per-chunk driver:
//                        hvc_uniform_reader.h; what both lay out on the host: hvc_hdec_plan.h)
//   hvc_capi_files.hip   the GPU Huffman coder's entry point and the batch pipelines that write files
//   hvc_rgb.hip          the RGB colour pass (kernels and launches; its entry points live with their families in the files above)
//   hvc_capi_mixed.hip   batches of frames / files of different geometry and tables (hvc_decode_frames_mixed, hvc_jpeg_decode_batch_mixed,
//                        their RGB forms: hvc_yuv_to_rgb_mixed, hvc_decode_frames_mixed_rgb, hvc_jpeg_decode_batch_mixed_rgb, and the
//                        reduced-size forms hvc_decode_frames_mixed_scaled, hvc_jpeg_decode_batch_mixed_scaled, _scaled_rgb); under
//                        hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG) the full-size ones launch the kernels of hvc_mixed_libjpeg.hip
//                        (the file pipeline's chunk cut and download runs: hvc_mixed_decode_chunks.h, plain C++)
//   hvc_capi_mixed_encode.hip  the same in the other direction: raw frames of different geometry, sampling and quality to records
//                        and files (behind hvc_encode_frames_mixed, hvc_jpeg_encode_batch_mixed), and the same from RGB images
//                        (behind hvc_rgb_to_yuv_mixed, hvc_encode_frames_mixed_rgb, hvc_jpeg_encode_batch_mixed_rgb[_gpu]); the part
//                        of the file pipeline that the one with the GPU coder runs too (encode_mixed_chunks, hvc_batch.h; its
//                        chunk cut and the padding workers' host parts: hvc_mixed_encode_chunks.h, plain C++)
//   hvc_capi_mixed_coder.hip   the mixed GPU Huffman coder alone and the file pipeline built on it (behind
//                        hvc_huffman_encode_frames_mixed, hvc_jpeg_encode_batch_mixed_gpu): what stands behind the block stage
//   hvc_capi_mixed_reader.hip  the mixed GPU Huffman reader's driver (hvc_mixed_reader.h) and hvc_jpeg_entropy_decode_gpu_mixed
//   hvc_capi_resize.hip  the resampling step over a mixed set (hvc_rgb_resize_mixed) and the launch of its two passes, which
//                        hvc_jpeg_decode_batch_mixed_resized ends in
//   hvc_capi_async.hip   pinned host memory and the slots of the asynchronous seam (hvc_decode_frames_submit / hvc_wait)
#ifndef HVC_CTX_H
#define HVC_CTX_H

#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <deque>
#include <functional>
#include <initializer_list>
#include <vector>

#include "../../include/hvc_jpeg.h"
#include "hvc_hdec.h"
#include "hvc_hardcaml.h"
#include "hvc_libjpeg.h"
#include "hvc_libjpeg_encode.h"
#include "hvc_libjpeg_encode_plan.h"
#include "hvc_huff.h"
#include "hvc_kernels.h"
#include "hvc_mixed_plan.h"
#include "hvc_mixed_encode_plan.h"
#include "hvc_mixed_encode_chunks.h"
#include "hvc_mixed_decode_chunks.h"
#include "hvc_pool.h"
#include "hvc_scaled_spec.h"

#define HVC_PROF_RING 64
#define HVC_FIX_WORDS 8 /* d_fix_count: [0] [1] counters, [2..3] the 64-bit total, [4] [5] the fused path's luma counters */

// ---------------------------------------------------------------------------
// What a context owns.  Three types, each a member that can be neither copied nor moved and whose destructor releases
// what it holds; hvc_destroy drains the streams and deletes the context, nothing else.

struct Pinned { // pinned host memory with these hipHostMalloc flags (a Buf declared without one is device memory)
    unsigned flags;
};
// A buffer: pointer and capacity in bytes.  Filled by grow (below), or by ring_ensure for the slots of a ring.
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    const bool pinned = false;
    const unsigned flags = 0;
    Buf() = default;
    Buf(Pinned k) : pinned(true), flags(k.flags) {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { (void)release(); }
    template <class T = void>
    T *as() const { return static_cast<T *>(p); }
    explicit operator bool() const { return p != nullptr; }
    hipError_t release() {
        const hipError_t e = !p ? hipSuccess : pinned ? hipHostFree(p) : hipFree(p);
        p = nullptr;
        cap = 0;
        return e;
    }
    void adopt(Buf &from) { // (of the same kind) a local that is complete becomes the context's
        (void)release();
        p = from.p, cap = from.cap;
        from.p = nullptr, from.cap = 0;
    }
};
// An event, created by the first ensure() with the flags given there.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
    hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};
// A stream of the context's own, created by the first ensure(): non-blocking, with a priority where one is given.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
    hipError_t ensure() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t ensure(int priority) { return s ? hipSuccess : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
};

// A plan's image in a device buffer, the pinned image it was uploaded from (a call whose plan is the same bytes uploads
// nothing) and the event behind the last upload (upload_image, hvc_capi_mixed.hip)
struct PlanBuf {
    Buf d, h{Pinned{hipHostMallocDefault}};
    size_t len = 0; // bytes of the image d holds, 0 = none
    Event ev;
};

// pinned rings the host only ever writes (unstuffed segments, padded raw frames) and the copy engine reads
#ifndef HVC_UPLOAD_RING_FLAGS
#define HVC_UPLOAD_RING_FLAGS hipHostMallocDefault
#endif
#define HVC_RING3(kind) {kind, kind, kind} /* the RING slots of a ring, all of one kind */
#define HVC_PINNED_RING HVC_RING3(Pinned{hipHostMallocDefault})
#define HVC_UPLOAD_RING HVC_RING3(Pinned{HVC_UPLOAD_RING_FLAGS})

// Members are destroyed in reverse order of declaration: the streams come FIRST, so that every buffer and event below
// them is released before the streams are destroyed (hvc_destroy has drained them by then).  Adding a buffer is one line:
// declare it here, as a Buf (device), a Buf{Pinned{flags}} or a ring of them, and grow it where it is used.
struct hvc_ctx {
    int device = -1;
    Stream own_stream;
    hipStream_t stream = nullptr; // own_stream, or the caller's (hvc_set_stream): never destroyed here
    Stream side_stream;           // the fused 4:4:4 path's side-by-side form: the stream the luma kernel runs on
    Stream down_stream, copy_stream; // hvc_jpeg_decode_batch: copy stream + ring of pinned host / device coefficient chunks
    Stream rd_stream[3];          // hvc_jpeg_decode_batch_gpu: the Huffman reader of even / odd chunks
    Event ev0, ev1;
    // ring of event pairs around the dominant kernel of the last HVC_PROF_RING profiled calls
    Event k0[HVC_PROF_RING], k1[HVC_PROF_RING];
    unsigned long long k_calls = 0;
    bool profiling = false;
    int mixed_reader = HVC_READER_HOST; // hvc_set_mixed_reader: who reads the files of the mixed batch calls
    unsigned long long mixed_gpu_files = 0, mixed_host_files = 0; // hvc_last_mixed_reader_files: the last mixed batch call's split
    bool honour_restart = false; // hvc_set_restart_markers: restart intervals honoured by the file-level entry points (an extension)
    int decode_kernel = 0; // hvc_set_decode_kernel: 0 packed (default), 1 unpacked int32, 2 int64 for every block, 3 q16
    int arith = HVC_ARITH_MODEL; // hvc_set_arithmetic: the block stage's arithmetic (HARDCAML: k_hardcaml, hvc_hardcaml.hip;
                                 // LIBJPEG: k_islow and, in the colour pass, k_ycc_to_rgb_fancy, hvc_libjpeg.hip)
    int mixed_arith = HVC_ARITH_MODEL; // hvc_set_mixed_arithmetic: the mixed decode calls' own setting (LIBJPEG: k_islow_mixed and
                                       // k_ycc_to_rgb_fancy_mixed, hvc_mixed_libjpeg.hip; they then do not look at `arith`)
    int enc_arith = HVC_ARITH_MODEL; // hvc_set_encode_arithmetic: the encoder's (HARDCAML: k_hardcaml_encode, hvc_hardcaml.hip)
    int enc_libjpeg = 0; // hvc_set_encode_libjpeg: the encoder of "Encoding bit-exact to libjpeg" (k_fdct_islow and k_dummy_blocks,
                         // hvc_libjpeg_encode.hip; replicated edges); enc_arith is then not consulted, HARDCAML beside it is refused
    int huff_tables = HVC_HUFF_DEFAULT; // hvc_set_huffman_tables: the files' Huffman tables (OPTIMISED: k_huff_hist / k_huff_build)
    int restart_interval = 0; // hvc_set_restart_interval: MCUs per restart interval of the files written, 0 = no DRI / RSTn
    Buf d_fix_count; // two counters, used alternately (see k_decode_wide); behind them (+ 8 bytes) the 64-bit
                     // total of the last call's fix-up blocks over all its launches (hvc_last_wide_blocks)
    // [4], [5]: a second pair of counters, for the luma planes of the fused 4:4:4 path when they run through
    // k_decode_packed beside (or before) the chroma tiles' kernel, which uses the first pair
    int fix_phase_l = 0;
    Event ev_fork, ev_join; // ... and the side stream's fork / join events
    bool wide_total_started = false; // the current call has enqueued a launch that stores (rather than adds to) that total
    long long wide_host = -1;        // >= 0: the last call sent every block through the int64 kernel (no list): this many
    int fix_phase = 0;               // index of the counter the NEXT decode call appends to
    int fix_last = 0;                // index of the counter the last decode call used
    Buf d_fix_list; // unsigned entries
    Buf d_in, d_out, d_sums, d_aux, d_aux2;
    // hvc_decode_frames_divergence / hvc_encode_frames_divergence: the model's output (pixels / records), and (host memory
    // calls) the input and the divergence bytes
    Buf d_div_px, d_div_in, d_div_out;
    // hvc_dct_*: the tables (uploaded at the first call) with k_dct_fixed's range flag, and two scratch buffers
    Buf d_dct_tab, d_dct_a, d_dct_b;
    int last_hip = 0;
    static constexpr int RING = 3;
    static_assert(RING == 3, "HVC_RING3 names the slots of a ring one by one");
    Event ev_rd[3]; // the Huffman reader's "records complete" per ring slot (RING entries)
    Buf h_ring[RING] = HVC_PINNED_RING, d_ring[RING], d_oring[RING];
    size_t ring_bytes = 0, oring_bytes = 0;
    Event ev_h2d[RING], ev_kern[RING], ev_t[4];
    // hvc_jpeg_encode_batch: pinned / device rings of padded pixel chunks (in) and coefficient chunks (out)
    Buf eh_in[RING] = HVC_UPLOAD_RING, ed_in[RING], eh_out[RING] = HVC_PINNED_RING, ed_out[RING];
    size_t e_in_bytes = 0, e_out_bytes = 0;
    Event ev_up[RING], ev_down[RING], ev_et[RING][3], ev_gpu[RING];
    Buf ed_seg[RING], ed_off[RING], eh_off[RING] = HVC_PINNED_RING; // hvc_jpeg_encode_batch_gpu: packed segments + offsets
    size_t e_seg_bytes = 0, e_off_bytes = 0;
    Buf eh_specs[RING] = HVC_PINNED_RING; // ... and, with optimised tables, each frame's four specs
    size_t e_specs_bytes = 0;
    // hvc_jpeg_encode_batch_mixed_rgb[_gpu]: the device slots the chunks' RGB images are uploaded into (eh_in holds them pinned,
    // ed_in the planes k_rgb_to_ycc_mixed makes of them)
    Buf ed_rgb[RING];
    size_t e_rgb_bytes = 0;
    // hvc_jpeg_decode_batch_gpu: pinned / device rings of unstuffed segments and their index arrays
    Buf gp_h_ecs[RING] = HVC_UPLOAD_RING, gp_d_ecs[RING], gp_h_meta[RING] = HVC_PINNED_RING, gp_d_meta[RING];
    Buf gp_h_ftabs[RING] = HVC_UPLOAD_RING, gp_d_ftabs[RING]; // ... and of per-frame Huffman tables (hvc::HdFrameTabs, PF mode)
    size_t gp_ecs_bytes = 0, gp_meta_bytes = 0, gp_ftabs_bytes = 0;
    // GPU Huffman decoder (hvc_jpeg_entropy_decode_gpu): device scratch, grown on demand
    Buf gd_ecs, gd_meta, gd_state, gd_tables, gd_coefs, gd_dcd;
    Buf gd_h_ecs{Pinned{HVC_UPLOAD_RING_FLAGS}}; // the batch's unstuffed segments on their way to gd_ecs
    Buf gd_fcnt;  // PF mode: per-frame list lengths per round (hvc::HdParams::list_fn)
    Buf gd_ftabs; // per-frame tables of hvc_jpeg_entropy_decode_gpu (PF mode)
    Buf gd_dcv;   // batch pipeline: the blocks' DC values as a compact array (hvc::DecodeParams::dc_plane)
    Buf d_dcfix;  // blocks with a DC beyond int16 (hvc::WideDc): ids, true DCs, count
    // hvc_decode_frames_mixed (hvc_capi_mixed.hip): the block stage's plan, and the plan of the colour pass over a mixed batch
    // (k_ycc_to_rgb_mixed): a buffer of its own, so that the colour plan of a chunk never overwrites the block-stage plan of
    // that chunk
    PlanBuf mixed_plan, mixed_rgb_plan;
    PlanBuf mixed_enc_plan; // hvc_encode_frames_mixed / hvc_jpeg_encode_batch_mixed (hvc_capi_mixed_encode.hip): k_encode_mixed's plan
    PlanBuf mixed_huff_plan; // hvc_huffman_encode_frames_mixed / hvc_jpeg_encode_batch_mixed_gpu (hvc_capi_mixed_coder.hip): the mixed coder's plan
    unsigned long long mixed_coder_gpu_files = 0, mixed_coder_host_files = 0; // hvc_last_mixed_coder_files
    // hvc_jpeg_decode_batch_mixed_rgb: the ring of device slots the chunks' decoded planes live in (they never leave the GPU)
    Buf d_pring[RING];
    size_t pring_bytes = 0;
    // hvc_rgb_resize_mixed / hvc_jpeg_decode_batch_mixed_resized (hvc_capi_resize.hip): the plan of the two resampling passes, and
    // the pipeline's rings of device slots for the chunks' RGB images at decoded size and for the passes' intermediates
    PlanBuf resize_plan;
    Buf d_rring[RING], d_mring[RING];
    size_t rring_bytes = 0, mring_bytes = 0;
    // hvc_set_host_cpus: the CPUs the batch pipelines' host threads may run on (empty = no restriction)
    bool have_cpus = false;
    cpu_set_t cpus;
    char cpulist[256] = "";
    bool have_default_cpus = false; // the process's own mask when the context was created: what the pool's threads go
    cpu_set_t default_cpus;         // back to when a restriction is lifted (they outlive the call that pinned them)
    hvc::WorkerPool pool;           // the batch pipelines' host threads (hvc_pool.h): persistent, joined in hvc_destroy
    std::unique_ptr<hvc::HdTables> gd_tables_host; // what gd_tables holds (value tables; the HdSpec behind them follows from these)
    bool gd_tables_valid = false;
    int gd_tables_ncomp = 0;
    // GPU Huffman coder (hvc_huffman_encode_frames): tables + scratch, grown on demand
    Buf hd_tables; // (unsigned words)
    Buf hd_opt;    // optimised tables: per-frame counts, code tables and specs (HuffParams hist / opt_tables / specs)
    Buf hd_lens, hd_meta, hd_bitbuf, hd_ff, hd_out;
    Buf hd_ivl; // restart intervals: bytes / byte bases per interval (HuffParams ivl)
    // The asynchronous seam (hvc_capi_async.hip): one batch in flight per slot.  Uploads run on copy_stream, the block stage
    // on `stream`, downloads on down_stream; a slot's device buffers are its own (grown while the slot is free).
    struct Slot {
        Buf d_in, d_out;
        // up0 / up1 around the upload, k0 / k1 around the block stage, dn0 / dn1 around the download; `done` = the last of them
        Event up0, up1, k0, k1, dn0, dn1;
        bool busy = false, has_down = false, timed = false;
        unsigned long long h2d_bytes = 0, d2h_bytes = 0;
    } slots[HVC_SLOTS];
};

// The pipelines' rings: RING pinned / device buffers per member, members that are (re)allocated together as a set.
struct RingMember {
    Buf (*ring)[hvc_ctx::RING];
    size_t *recorded; // the bytes it was last allocated for (members of the same size share one)
    size_t slack;     // a device member is allocated with this many bytes more
};
struct RingSet {
    RingMember m[6];
    int n;
    bool drain_copy; // copy_stream is drained as well as `stream` before the old buffers go
};
inline RingSet coef_rings(hvc_ctx *c) { return {{{&c->h_ring, &c->ring_bytes, 0}, {&c->d_ring, &c->ring_bytes, 0}}, 2, true}; } // coefficient chunks of the decode pipelines
inline RingSet out_rings(hvc_ctx *c) { return {{{&c->d_oring, &c->oring_bytes, 0}}, 1, false}; } // decoded chunks on their way to the host
inline RingSet plane_rings(hvc_ctx *c) { return {{{&c->d_pring, &c->pring_bytes, 0}}, 1, false}; }
inline RingSet resize_rings(hvc_ctx *c) { return {{{&c->d_rring, &c->rring_bytes, 0}, {&c->d_mring, &c->mring_bytes, 0}}, 2, false}; } // decoded-size RGB chunks and the passes' intermediates
inline RingSet reader_rings(hvc_ctx *c) { // hvc_jpeg_decode_batch_gpu: segments, index arrays, per-frame tables
    return {{{&c->gp_h_ecs, &c->gp_ecs_bytes, 0}, {&c->gp_d_ecs, &c->gp_ecs_bytes, HVC_HD_ECS_SLACK}, {&c->gp_h_meta, &c->gp_meta_bytes, 0},
             {&c->gp_d_meta, &c->gp_meta_bytes, 0}, {&c->gp_h_ftabs, &c->gp_ftabs_bytes, 0}, {&c->gp_d_ftabs, &c->gp_ftabs_bytes, 0}},
            6, true};
}
inline RingSet enc_rings(hvc_ctx *c) { // hvc_jpeg_encode_batch: padded pixel chunks in, coefficient chunks out
    return {{{&c->eh_in, &c->e_in_bytes, 0}, {&c->eh_out, &c->e_out_bytes, 0}, {&c->ed_in, &c->e_in_bytes, 0}, {&c->ed_out, &c->e_out_bytes, 0}},
            4, true};
}
inline RingSet enc_seg_rings(hvc_ctx *c) { // hvc_jpeg_encode_batch_gpu: packed segments + offsets
    return {{{&c->ed_seg, &c->e_seg_bytes, 0}, {&c->ed_off, &c->e_off_bytes, 0}, {&c->eh_off, &c->e_off_bytes, 0}}, 3, false};
}
inline RingSet enc_spec_rings(hvc_ctx *c) { return {{{&c->eh_specs, &c->e_specs_bytes, 0}}, 1, false}; }
inline RingSet enc_rgb_rings(hvc_ctx *c) { return {{{&c->ed_rgb, &c->e_rgb_bytes, 0}}, 1, true}; } // RGB chunks of the mixed encode pipelines
// A set grows when any member wants more than it has (`want`: bytes per member, in the set's order), and is then allocated
// at the sizes wanted now.  HVC_OK, HVC_E_HIP (a stream did not drain) or HVC_E_OUT_OF_MEMORY.
int ring_ensure(hvc_ctx *c, const RingSet &s, std::initializer_list<size_t> want);

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

inline int fail_hip(hvc_ctx *c, hipError_t e) {
    c->last_hip = (int)e;
    return HVC_E_HIP;
}
#define HIPCHK(c, call)                                 \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return fail_hip((c), e_); \
    } while (0)

// Every host thread a batch pipeline starts calls this first (hvc_set_host_cpus); false = the restriction could not
// be applied (the batch call then fails rather than run somewhere it was told not to).
bool pin_to_ctx_cpus(const hvc_ctx *c);

// `n` pool threads for a pipeline call (+ `extra` for its downloader): HVC_OK, or HVC_E_SYSTEM when the system refuses one
inline int pool_ready(hvc_ctx *c, int n, int extra = 0) { return c->pool.ensure(n + extra); }

// Linux cpulist format ("0-15,32-47") -> cpu_set_t; false on a syntax error, an empty set or a CPU beyond CPU_SETSIZE
bool parse_cpulist(const char *s, cpu_set_t &set);

// How a buffer grows: to need + need / spare_div + spare_add bytes (spare_div 0: no fraction), and whether c->stream is
// drained before the old allocation goes.  Growth sizes are behaviour: they decide the resident footprint and when a
// reallocation, with its drain, happens.
struct GrowRule {
    unsigned spare_div;
    size_t spare_add;
    enum { NO_DRAIN, DRAIN_HELD, DRAIN_ALWAYS } drain; // never / when there is an old allocation / whenever it grows
    bool clear_error; // a refused allocation's error is taken off the runtime (hipGetLastError)
};
constexpr GrowRule GROW_SCRATCH{4, 4096, GrowRule::DRAIN_HELD, false};      // the context's device scratch: the default
constexpr GrowRule GROW_SLOT{8, 4096, GrowRule::NO_DRAIN, false};           // a slot of the asynchronous seam, grown while it is free
constexpr GrowRule GROW_PLAN_IMAGE{4, 4096, GrowRule::DRAIN_ALWAYS, false}; // PlanBuf::h
constexpr GrowRule GROW_READER_STAGE{2, 0, GrowRule::NO_DRAIN, true};       // gd_h_ecs
constexpr GrowRule GROW_EXACT{0, 0, GrowRule::NO_DRAIN, false};             // tables of a fixed size, allocated once
// `b` of at least `need` bytes: HVC_OK, HVC_E_HIP (the stream did not drain, the old device allocation could not be freed) or
// HVC_E_OUT_OF_MEMORY (device memory: with last_hip set)
int grow(hvc_ctx *c, Buf &b, size_t need, const GrowRule &rule = GROW_SCRATCH);

// The two fix-up counters alternate between launches: a launch appends to counter fix_phase and its wide kernel
// clears the other one for the launch after it (no memset node).  The roles change hands only once a launch has
// been enqueued: a call that fails before or while launching leaves fix_phase where it was and, if anything may
// have reached the stream, both counters are cleared -- the next call must never find a stale count (its wide kernel
// would re-process old list entries under the new geometry).
template <class Params>
inline void fix_assign(const hvc_ctx *c, Params &P) {
    P.fix_count = c->d_fix_count.as<unsigned>() + c->fix_phase;
    P.fix_count_next = c->d_fix_count.as<unsigned>() + (c->fix_phase ^ 1);
    P.fix_list = c->d_fix_list.as<unsigned>();
    P.wide_total = reinterpret_cast<unsigned long long *>(c->d_fix_count.as<unsigned>() + 2);
    P.wide_first = c->wide_total_started ? 0 : 1;
}
inline void fix_commit(hvc_ctx *c) {
    c->fix_last = c->fix_phase;
    c->fix_phase ^= 1;
    c->wide_total_started = true; // the call's next launches add to the total
}
// at the start of every decode call: its first launch starts the total over
inline void wide_total_begin(hvc_ctx *c) {
    c->wide_total_started = false;
    c->wide_host = -1;
}
inline void fix_reset(hvc_ctx *c) { // after a failed launch: all counters to zero, in stream order
    (void)hipMemsetAsync(c->d_fix_count.p, 0, HVC_FIX_WORDS * sizeof(unsigned), c->stream); // (and the total behind the first pair)
}
// The total for a block stage that only ADDS to it (k_decode_mixed_scaled, k_islow_mixed: no fix-up list): the call's first
// launch has it cleared in front of it, in stream order
inline hipError_t wide_total_for_adding(hvc_ctx *c, unsigned long long *&total) {
    total = reinterpret_cast<unsigned long long *>(c->d_fix_count.as<unsigned>() + 2);
    const hipError_t e = c->wide_total_started ? hipSuccess : hipMemsetAsync(total, 0, sizeof *total, c->stream);
    if (e == hipSuccess) c->wide_total_started = true;
    return e;
}

// A launch that takes the next entry of the profiling ring (hvc_kernel_ms_history) when `profile`: launch(k0, k1) is given the
// entry's two events to record around its kernels, or two null events; the entry counts once the launch is enqueued.
template <class Launch>
inline hipError_t profiled_launch(hvc_ctx *c, bool profile, Launch launch) {
    const int slot = (int)(c->k_calls % HVC_PROF_RING);
    const hipError_t e = launch(profile ? (hipEvent_t)c->k0[slot] : nullptr, profile ? (hipEvent_t)c->k1[slot] : nullptr);
    if (e == hipSuccess && profile) c->k_calls++;
    return e;
}

// Launches longer than about 3 ms lose 2-3 % against back-to-back shorter ones (measured on MI355X: 1080p batches of
// 2048 / 4096 frames per launch run at 71.9 / 71.6 % of the HBM peak, 1024-frame launches -- even 1900 of them back to
// back over 3 s, or sixteen of them over a 154 GB resident set -- at 74.4 %; the counters show a lower clock and more
// DRAM read-credit stalls late in a long launch, not TLB misses: DESIGN.md section 5).  So a device-memory batch is cut
// into launches of at most this many algorithmic bytes (192 B per block); HVC_LAUNCH_BYTES overrides (experiments).
size_t launch_bytes_limit();
// The fused 4:4:4 path's block stage (decode_frames_yuv444_impl): 0 = one kernel for luma and chroma tiles, 1 = the luma
// planes through k_decode_packed, then the chroma tiles, 2 = the two side by side on two streams.  HVC_444_MODE
// overrides the default (A/B measurements).
#ifndef HVC_444_MODE_DEFAULT
#define HVC_444_MODE_DEFAULT 0
#endif
int fused444_mode();
// frames per launch for a batch of n_frames frames of blocks_per_frame blocks: equal parts, each within the limit
int frames_per_launch(int n_frames, unsigned long long blocks_per_frame);

// Geometry of one call -> CompK[]; shared by decode and encode.
struct Layout {
    hvc::CompK comp[HVC_MAX_COMP];
    int n_comp = 0, tiles_per_frame = 0;
    size_t coef_span = 0;  // elements covered by one frame record
    size_t pixel_span = 0; // bytes covered by one frame record
    unsigned long long blocks_per_frame = 0;
};
// n: samples per block side of the pixel planes -- 8, or 4 / 2 / 1 for the scaled block stage, whose planes (bw * n bytes
// per row) may lie at any offset with any stride >= that
int make_layout(const hvc_component *comps, int n_comp, int n_qtabs, Layout &L, int n = 8);
int check_qtabs(const uint16_t *qtabs, int n_qtabs, bool divides); // divides: the encoder (an entry of zero is HVC_E_RANGE)

// A component without a block (blocks_w or blocks_h of zero: the model's empty Plane.t) has no part in the block stage: the
// decoding entry points drop such components from the list they work on; *n_kept == 0: nothing to decode at all.
int drop_empty_components(const hvc_component *comps, int n_comp, hvc_component *kept, int *n_kept);

// What comes back to a host caller is what the kernels wrote, never the padding between planes.  Planes (pixel planes:
// decode; coefficient planes: encode) that follow one another tightly -- the usual record -- are ONE stretch per frame:
// [first, first + len) in bytes from the frame record; len == 0: they are not, every plane is copied by itself.
struct RecordRun {
    size_t first = 0, len = 0;
};
RecordRun pixel_run(const hvc_component *comps, int n_comp);
RecordRun coef_run(const hvc_component *comps, int n_comp); // (bytes, like pixel_run)
// frames [f0, f0 + cnt) of a batch laid out alike on the device (d_base) and on the host (h_base), frame stride `fs` bytes,
// device -> host on stream `st`: one copy (stretches that touch), one 2D copy, or one 2D copy per plane
hipError_t download_pixels(const hvc_component *comps, int n_comp, const RecordRun &run, int f0, int cnt, size_t fs,
                           const uint8_t *d_base, uint8_t *h_base, hipStream_t st);
hipError_t download_coefs(const hvc_component *comps, int n_comp, const RecordRun &run, int f0, int cnt, size_t fs_bytes,
                          const uint8_t *d_base, uint8_t *h_base, hipStream_t st);

// The batch pipelines' orchestrating thread waits most of the call (an upload's end, a chunk's kernels).
// hipEventSynchronize spins -- also on an event created with hipEventBlockingSync, on this ROCm (measured: CPU time =
// wall time) -- and on a box whose processes own a fixed share of CPU time (16 CPUs for one GPU here) a spinning thread
// takes its CPU from the workers that are the bound of the pipeline.  So: poll and sleep, 20 us at first, 200 us from
// the tenth poll on (the waits are milliseconds long).  HVC_EVENT_SPIN=1: hipEventSynchronize (A/B).
hipError_t wait_event(hipEvent_t e);

// Host buffers, large batches: four parts; while part k + 1 is uploaded (c->stream), part k runs through the kernels
// (c->stream) and is downloaded (a second thread on c->down_stream: copies to and from pageable memory hold
// their caller), so the link carries both directions at once.  up(f0, cnt) / run(k, f0, cnt) enqueue on c->stream,
// down(f0, cnt, stream) on the stream it is given.
template <class Up, class Run, class Down>
inline int overlapped_parts(hvc_ctx *c, int n_frames, Up up, Run run, Down down) {
    constexpr int K = 4;
    HIPCHK(c, c->down_stream.ensure());
    for (int i = 0; i < K; i++) HIPCHK(c, c->ev_t[i].ensure());
    std::atomic<int> launched{0}, herr{0};
    auto part = [&](int k, int &f0, int &cnt) {
        f0 = (int)((long long)n_frames * k / K);
        cnt = (int)((long long)n_frames * (k + 1) / K) - f0;
    };
    int pr = pool_ready(c, 1);
    if (pr) return pr;
    hvc::PoolScope scope(c->pool, [&] { if (launched.load() < K) herr.store(herr.load() ? herr.load() : (int)hipErrorUnknown); });
    pr = c->pool.submit([&] {
        (void)pin_to_ctx_cpus(c);
        if (hipSetDevice(c->device) != hipSuccess) { herr.store((int)hipErrorInvalidDevice); return; }
        for (int k = 0; k < K; k++) {
            while (launched.load(std::memory_order_acquire) <= k && !herr.load()) std::this_thread::yield();
            if (herr.load()) return;
            int f0, cnt;
            part(k, f0, cnt);
            hipError_t e = hipStreamWaitEvent(c->down_stream, c->ev_t[k], 0);
            if (e == hipSuccess) e = down(f0, cnt, c->down_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->down_stream);
            if (e != hipSuccess) { herr.store((int)e); return; }
        }
    }, 1);
    if (pr) return pr;
    hipError_t e = hipSuccess;
    for (int k = 0; k < K && e == hipSuccess && !herr.load(); k++) {
        int f0, cnt;
        part(k, f0, cnt);
        e = up(f0, cnt);
        if (e == hipSuccess) e = run(k, f0, cnt);
        if (e == hipSuccess) e = hipEventRecord(c->ev_t[k], c->stream);
        if (e == hipSuccess) launched.store(k + 1, std::memory_order_release);
    }
    if (e != hipSuccess) herr.store((int)e);
    pr = scope.finish();
    (void)hipStreamSynchronize(c->stream);
    if (pr) return pr;
    if (herr.load()) return fail_hip(c, (hipError_t)herr.load());
    return HVC_OK;
}

// ---------------------------------------------------------------------------
// What one part of the ABI calls in another

// A block of a batch whose true DC does not fit the int16 record (hvc::WideDc of frame `frame` of the batch): after
// the batch's launches it is recomputed in int64 with that DC -- what the model's 63-bit arithmetic gives.
struct WideFix {
    int frame;
    uint32_t block;
    long long dc;
};

// What one call of the block stage is to do beyond its records: stated by the caller with the call, never by changing the
// context's settings around it.  The public entry points take the context's settings (the constructors); an internal
// caller starts from those and overrides what it decides itself.
struct DecodeOpts {
    int arith = HVC_ARITH_MODEL;         // hvc_set_arithmetic
    bool profile = false;                // a device-memory call takes an entry of the profiling ring (hvc_set_profiling)
    const int16_t *dc_plane = nullptr;   // (device memory calls only, default kernels only): see hvc::DecodeParams::dc_plane
    size_t dc_fs = 0;
    const std::vector<WideFix> *wide = nullptr; // (device memory calls only): blocks to recompute with their true DC once the launches are enqueued
    explicit DecodeOpts(const hvc_ctx *c) : arith(c ? c->arith : HVC_ARITH_MODEL), profile(c && c->profiling) {}
};
struct EncodeOpts {
    int arith = HVC_ARITH_MODEL; // hvc_set_encode_arithmetic
    bool libjpeg = false;        // hvc_set_encode_libjpeg: k_fdct_islow whatever `arith` (HARDCAML beside it: HVC_E_INVALID_ARG)
    bool profile = false;
    // (libjpeg only) the frames' sizes, where the caller knows them: comp[i].actual_width / actual_height and hscale of the
    // components the records are laid out for -- blocks past ceil(actual / 8) are dummy blocks (k_dummy_blocks behind every
    // launch, same stream).  nullptr: every block is real.
    const hvc_jpeg_info *edges = nullptr;
    explicit EncodeOpts(const hvc_ctx *c)
        : arith(c ? c->enc_arith : HVC_ARITH_MODEL), libjpeg(c && c->enc_libjpeg), profile(c && c->profiling) {}
};
// the rule of hvc_set_encode_libjpeg for the entry points that have no libjpeg form (hvc_encode_frames_recon, _divergence): refused,
// never the model's form in silence
inline bool encode_libjpeg_refused(const hvc_ctx *c) { return c && c->enc_libjpeg; }

// hvc_capi.hip: the block stage behind hvc_decode_frames / hvc_decode_frames_yuv444 / hvc_encode_frames
int decode_frames_impl(hvc_ctx *c, const int16_t *coefs, size_t coef_fs, const uint16_t *qtabs, int n_qtabs,
                       const hvc_component *comps, int n_comp, int n_frames, uint8_t *pixels, size_t pixel_fs, int where,
                       const DecodeOpts &o);
int decode_frames_yuv444_impl(hvc_ctx *c, const int16_t *coefs, size_t coef_fs, const uint16_t *qtabs, int n_qtabs,
                              const hvc_component *comps, int n_comp, int n_frames, int width, int height, uint8_t *frames,
                              size_t frame_stride, int where, const DecodeOpts &o);
// the block stage at 1 / scale_denom size (k_decode_scaled, hvc_scaled.hip) behind hvc_decode_frames_scaled and the file-level
// scaled entry points; scale_denom = 1 is decode_frames_impl.  Of `o` it takes arith (anything but MODEL: HVC_E_INVALID_ARG), profile,
// dc_plane and dc_fs.
int decode_frames_scaled_impl(hvc_ctx *c, const int16_t *coefs, size_t coef_fs, const uint16_t *qtabs, int n_qtabs,
                              const hvc_component *comps, int n_comp, int n_frames, int scale_denom, uint8_t *pixels, size_t pixel_fs,
                              int where, const DecodeOpts &o);
// scaled_side(scale_denom) and scaled_info (hvc_jpeg_scaled_info's arithmetic): hvc_mixed_plan.h, plain C++ for the host plans too
int encode_frames_impl(hvc_ctx *c, const uint8_t *pixels, size_t pixel_fs, const uint16_t *qtabs, int n_qtabs,
                       const hvc_component *comps, int n_comp, int n_frames, int16_t *coefs, size_t coef_fs, int where,
                       const EncodeOpts &o);

// after_reader (optional): called once the reader's launches are enqueued and BEFORE its verdict is known -- the caller
// enqueues what consumes the records (block stage, download) on the same stream, so that one call costs one host
// synchronisation instead of two; *speculated tells whether what it enqueued ran on valid records.
struct AfterReader {
    std::function<int()> enqueue; // an hvc_status
    bool speculated = false;      // out: enqueue() ran, and behind a reader run whose verdict was good
    // The consumer is the block stage: the reader's DC pass then writes the DC values to this compact array
    // (hvc::DecodeParams::dc_plane, one per block of the frame record) instead of 2 bytes into each 128-byte record --
    // a partial-line write apiece, 35 of a single file's 430 us -- and the records keep the DC difference.
    int16_t *dc_plane = nullptr;
    size_t dc_fs = 0;
};
// hvc_capi_reader.hip: Huffman decoding on the GPU (hvc_hdec.hip) of a batch of files that share a geometry.  HVC_OK with
// *used_gpu = 1 when the coefficient records at d_coefs are complete; HVC_OK with *used_gpu = 0 when a stream needs the
// host reader (nothing usable was written); or the error the host reader would report while parsing headers.
int gpu_entropy_decode(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, const hvc_jpeg_info &info0,
                       int16_t *d_coefs, size_t coef_fs, int *used_gpu, AfterReader *after = nullptr);

inline bool is_420_scan(const hvc_jpeg_info &info) { // Y 2x2, Cb / Cr 1x1 (frame.ml:42-61)
    return info.n_comp == 3 && info.comp[0].hscale == 2 && info.comp[0].vscale == 2 && info.comp[1].hscale == 1 &&
           info.comp[1].vscale == 1 && info.comp[2].hscale == 1 && info.comp[2].vscale == 1;
}

// What the records of a file become, for the file-level decoders (hvc_capi_jpeg.hip, hvc_capi_reader.hip).  An entry point
// states the kind (and scale_denom); of() adds the geometry once the first file's header is read.
struct OutputForm {
    enum Kind {
        PLANES, // padded component planes (hvc_jpeg_decode, hvc_jpeg_decode_batch)
        YUV444, // a 4:2:0 scan as a tight 4:4:4 frame through the fused kernel (hvc_jpeg_decode_yuv444, _batch_yuv444)
        SCALED, // the planes of hvc_jpeg_scaled_info, tight, through the scaled block stage: scale_denom = 2, 4, 8
    } kind;
    int scale_denom;
    hvc_jpeg_info info, sinfo; // the first file's, and the output's geometry: the same, or its scaled form
    size_t out_bytes = 0;      // per frame
    explicit OutputForm(Kind k, int denom = 1) : kind(denom == 1 && k == SCALED ? PLANES : k), scale_denom(denom) {}
    bool known() const { return kind == SCALED ? scaled_side(scale_denom) != 0 : scale_denom == 1; }
    void of(const hvc_jpeg_info &first) {
        info = sinfo = first;
        if (kind == SCALED) scaled_info(first, scaled_side(scale_denom), sinfo);
        out_bytes = kind == YUV444 ? (size_t)3 * first.width * first.height : sinfo.pixel_bytes;
    }
    // a batch into frames `frame_stride` bytes apart: 4:4:4 frames need a 4:2:0 scan of even size, full-size planes a stride
    // that keeps every frame's rows 8-byte aligned
    int batch_check(size_t frame_stride) const {
        if (kind == YUV444 && (!is_420_scan(info) || (info.width & 1) || (info.height & 1))) return HVC_E_INVALID_ARG;
        return frame_stride < out_bytes || (kind == PLANES && (frame_stride & 7)) ? HVC_E_INVALID_ARG : HVC_OK;
    }
    // a batch pipeline's chunk takes a profiling-ring entry only through the scaled block stage (hvc_jpeg_decode_batch_scaled)
    bool chunk_profile(const hvc_ctx *c) const { return kind == SCALED && c->profiling; }
    // the block stage of n_frames records (info.coef_count apart) to dst; o.wide: HVC_E_RANGE where the form has no int64
    // fix-up (the scaled block stage) and the list names a block
    int run(hvc_ctx *c, const int16_t *coefs, int n_frames, uint8_t *dst, size_t dst_fs, int where, const DecodeOpts &o) const {
        const uint16_t *q = &info.qtabs[0][0];
        switch (kind) {
        case SCALED:
            if (o.wide && !o.wide->empty()) return HVC_E_RANGE;
            return decode_frames_scaled_impl(c, coefs, info.coef_count, q, info.n_qtabs, sinfo.layout, info.n_comp, n_frames, scale_denom,
                                             dst, dst_fs, where, o);
        case YUV444:
            return decode_frames_yuv444_impl(c, coefs, info.coef_count, q, info.n_qtabs, info.layout, info.n_comp, n_frames, info.width,
                                             info.height, dst, dst_fs, where, o);
        default:
            return decode_frames_impl(c, coefs, info.coef_count, q, info.n_qtabs, info.layout, info.n_comp, n_frames, dst, dst_fs, where, o);
        }
    }
};

// hvc_capi_jpeg.hip: the batch pipeline with the host reader (hvc_jpeg_decode_batch / _yuv444 / _scaled) -- also where the
// pipeline with the GPU reader sends a batch, or the chunks, it cannot take (with the form it was given)
int decode_batch_impl(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads,
                      int frames_per_chunk, uint8_t *pixels, size_t pixel_fs, int where, hvc_batch_stats *stats, OutputForm form);
// hvc_capi_reader.hip: the same with the GPU reader (behind hvc_jpeg_decode_batch_gpu)
int decode_batch_gpu(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads, int frames_per_chunk,
                     uint8_t *pixels, size_t pixel_fs, int where, hvc_batch_stats *stats, OutputForm form);

// hvc_capi_mixed.hip: frames / files of different geometry and tables in one call (behind hvc_decode_frames_mixed in hvc_capi.hip
// and hvc_jpeg_decode_batch_mixed in hvc_capi_jpeg.hip)
int decode_frames_mixed_impl(hvc_ctx *c, const int16_t *coefs, const size_t *coef_offsets, const hvc_jpeg_info *infos, int n_frames,
                             uint8_t *pixels, const size_t *pixel_offsets, int where, int scale_denom = 1);
// (MixedForm -- what the files of a mixed batch become -- and the pipeline's chunk cut: hvc_mixed_decode_chunks.h, plain C++)
// Which arithmetic a mixed decode call runs in, or that it is refused (the one rule of hvc_set_mixed_arithmetic).  At the
// default the calls do what they did before there was such a setting: the model's arithmetic, and HVC_E_INVALID_ARG unless
// hvc_set_arithmetic is the model's too (the RTL arithmetic has no mixed form, as it has no scaled one).  Under
// HVC_ARITH_LIBJPEG hvc_set_arithmetic is not looked at; the reduced-size forms have no libjpeg form (libjpeg decodes the
// chroma of a subsampled file at another size there) and are refused.
inline int mixed_arith_of(const hvc_ctx *c, int scale_denom, bool &libjpeg) {
    libjpeg = c->mixed_arith == HVC_ARITH_LIBJPEG;
    if (libjpeg) return scale_denom == 1 ? HVC_OK : HVC_E_INVALID_ARG;
    return c->arith != HVC_ARITH_MODEL ? HVC_E_INVALID_ARG : HVC_OK;
}
int decode_batch_mixed_impl(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads, size_t chunk_bytes,
                            const hvc_jpeg_info *infos, int *status, const size_t *pixel_offsets, uint8_t *pixels, size_t pixel_cap,
                            int where, hvc_batch_stats *stats, const MixedForm &form = MixedForm(), bool host_reader_only = false);
// A plan's image in a device buffer of the context, in stream order on c->stream: uploaded from the pinned copy unless the
// device already holds these bytes (hvc_capi_mixed.hip; the mixed encode plans of hvc_capi_mixed_encode.hip go the same way)
int upload_image(hvc_ctx *c, PlanBuf &b, const std::vector<unsigned char> &img);
// ... made of parts one after another, each on 16 bytes; at[i] = where part i starts (a part of no bytes takes no room)
struct ImagePart {
    const void *p;
    size_t bytes;
};
int upload_parts(hvc_ctx *c, PlanBuf &b, std::initializer_list<ImagePart> parts, size_t *at);
// hvc_capi_mixed_encode.hip: frames of different geometry, sampling and quality ENCODED in one call (behind
// hvc_encode_frames_mixed and hvc_jpeg_encode_batch_mixed in hvc_capi_files.hip)
int encode_frames_mixed_impl(hvc_ctx *c, const uint8_t *pixels, const size_t *pixel_offsets, const hvc_jpeg_info *infos, int n_frames,
                             int16_t *coefs, const size_t *coef_offsets, int where);
// (MixedEncodeInput -- what frames[f] of a mixed encode batch is -- and the host-only parts of the padding workers:
// hvc_mixed_encode_chunks.h; what the pipeline shares with the one behind the GPU coder: MixedEncodeFront, hvc_batch.h)
int encode_batch_mixed_impl(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                            size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes, hvc_batch_stats *stats,
                            const MixedEncodeInput &in = MixedEncodeInput());
// hvc_capi_mixed.hip, for both directions: the mixed colour pass of a plan on device memory, enqueued on c->stream (to_ycc:
// k_rgb_to_ycc_mixed, d_rgb read and the planes at d_yuv written); where the records of a host-memory call go in device scratch
namespace hvc {
struct MixedRgbPlan;
}
int mixed_rgb_launch_plan(hvc_ctx *c, const hvc::MixedRgbPlan &plan, int layout, const uint8_t *d_yuv, uint8_t *d_rgb, bool profile,
                          bool to_ycc = false);
size_t stage_offsets(const size_t *offsets, const std::vector<size_t> &spans, std::vector<size_t> &d_off);
// hvc_capi_resize.hip: the two resampling passes of a plan on device memory, enqueued on c->stream (d_mid: the intermediate, at
// least plan.mid_bytes, on 64 bytes)
namespace hvc {
struct ResizePlan;
}
// lut: a plan with out_elem 2 / 4 (typed output): the caller's table, HOST memory, 3 * 256 elements
int resize_launch_plan(hvc_ctx *c, const hvc::ResizePlan &plan, const uint8_t *d_src, uint8_t *d_dst, uint8_t *d_mid, bool profile,
                       const void *lut = nullptr);
// what every call reads of an hvc_resize_opts before anything else (NULL: all zero): out_elem is 0, 2 or 4, and a table comes with 2 / 4
inline int resize_opts_check(const hvc_resize_opts *o) {
    if (!o) return HVC_OK;
    if (o->out_elem != 0 && o->out_elem != 2 && o->out_elem != 4) return HVC_E_INVALID_ARG;
    return o->out_elem && !o->lut ? (int)HVC_E_INVALID_ARG : (int)HVC_OK;
}
// ... and the resampling step alone (behind hvc_rgb_resize_mixed and hvc_rgb_resize_mixed_opts in hvc_yuv.hip)
int rgb_resize_mixed_impl(hvc_ctx *c, const uint8_t *src, const size_t *src_offsets, const size_t *src_row_strides, const int *widths,
                          const int *heights, int n_images, uint8_t *dst, const size_t *dst_offsets, const size_t *dst_row_strides,
                          const int *out_widths, const int *out_heights, int layout, int filter, int where,
                          const hvc_resize_opts *opts = nullptr);
// hvc_normalize_lut.cpp (plain C++, -ffp-contract=off): the table behind hvc_normalize_lut (hvc_yuv.hip)
namespace hvc {
int normalize_lut(const float *mean, const float *std, int elem, void *lut);
}
// the colour pass alone / in front of the block stage (behind hvc_rgb_to_yuv_mixed in hvc_yuv.hip, hvc_encode_frames_mixed_rgb in
// hvc_capi_files.hip)
int rgb_to_yuv_mixed_impl(hvc_ctx *c, uint8_t *yuv, const size_t *yuv_offsets, const hvc_jpeg_info *infos, int n_frames, const uint8_t *rgb,
                          const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout, int where);
int encode_frames_mixed_rgb_impl(hvc_ctx *c, const uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout,
                                 const hvc_jpeg_info *infos, int n_frames, int16_t *coefs, const size_t *coef_offsets, int where);
// hvc_capi_mixed_encode.hip: k_encode_mixed over a plan on device memory, enqueued on c->stream
// lje (hvc_set_encode_libjpeg; nullptr: the model's block stage): the frames the plan was built of -- k_fdct_islow_mixed in
// place of k_encode_mixed and, from the infos' sizes, k_dummy_blocks_mixed behind it (hvc_libjpeg_encode.hip)
struct MixedLibjpeg {
    const hvc_jpeg_info *infos;
    const size_t *coef_offsets; // as the plan was built with
    const int *frames;          // the plan's list (nullptr: 0 .. n_list - 1)
    int n_list;
};
int encode_mixed_launch_plan(hvc_ctx *c, const hvc::MixedEncodePlan &plan, const uint8_t *d_pixels, int16_t *d_coefs, bool profile,
                             const MixedLibjpeg *lje = nullptr);
// hvc_capi_mixed_coder.hip: the mixed GPU Huffman coder alone and behind the block stage (behind
// hvc_huffman_encode_frames_mixed and hvc_jpeg_encode_batch_mixed_gpu in hvc_capi_files.hip)
int huffman_encode_frames_mixed_impl(hvc_ctx *c, const hvc_jpeg_info *infos, const int16_t *coefs, const size_t *coef_offsets, int n_frames,
                                     int tables, uint8_t *out, size_t out_cap, uint64_t *offsets, int *status, hvc_huff_spec *specs, int where);
int encode_batch_mixed_gpu_impl(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                                size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes, hvc_batch_stats *stats,
                                const MixedEncodeInput &in = MixedEncodeInput());
// hvc_capi_mixed_reader.hip: the mixed GPU Huffman reader over one chunk on the calling thread (behind hvc_jpeg_entropy_decode_gpu_mixed
// in hvc_capi_jpeg.hip)
int entropy_decode_gpu_mixed_impl(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, const hvc_jpeg_info *infos,
                                  int *status, int16_t *coefs, const size_t *coef_offsets, size_t coef_cap, int where, int *used_gpu);
// the colour pass alone / behind the block stage (behind hvc_yuv_to_rgb_mixed in hvc_yuv.hip, hvc_decode_frames_mixed_rgb in hvc_capi.hip)
int yuv_to_rgb_mixed_impl(hvc_ctx *c, const uint8_t *yuv, const size_t *yuv_offsets, const hvc_jpeg_info *infos, int n_frames, uint8_t *rgb,
                          const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout, int where);
int decode_frames_mixed_rgb_impl(hvc_ctx *c, const int16_t *coefs, const size_t *coef_offsets, const hvc_jpeg_info *infos, int n_frames,
                                 uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout, int where);

// hvc_rgb.hip: the colour pass (k_ycc_to_rgb / k_rgb_to_ycc) on device memory, for the entry points that end or begin with it
struct RgbImage { // an RGB image as the caller laid it out (hvc_rgb_layout; strides of 0 resolved to tight)
    int layout = 0;
    size_t row_bytes = 0, rows = 0; // what a row holds, rows from the first to the last (planar: 3 * height, the planes follow one another)
    size_t row_stride = 0, frame_stride = 0;
};
bool rgb_image(int layout, int width, int height, size_t row_stride, size_t frame_stride, RgbImage &im); // false: a bad layout or stride
size_t rgb_bytes(const RgbImage &im, int n_frames); // from the first byte of frame 0 to the last byte written
int rgb_sampling_of(const hvc_jpeg_info &info);     // HVC_YUV_420 / 422 / 444 / 400 by the scan's sampling factors, 0 = none of them
void rgb_chroma_window(int sampling, int width, int height, int &cw, int &ch); // ceil(width / 2) x ceil(height / 2) for 4:2:0, ...
// arith: the context's hvc_set_arithmetic -- HVC_ARITH_LIBJPEG takes k_ycc_to_rgb_fancy (hvc_libjpeg.hip), anything else k_ycc_to_rgb
hipError_t ycc_to_rgb_device(const uint8_t *d_yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int width, int height, int cw,
                             int ch, int n_frames, uint8_t *d_rgb, const RgbImage &im, hipStream_t s, int arith);
hipError_t ycc_to_rgb_fancy_device(const uint8_t *d_yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int width, int height,
                                   int cw, int ch, int n_frames, uint8_t *d_rgb, const RgbImage &im, hipStream_t s);
// hvc_set_encode_libjpeg: k_rgb_to_ycc_libjpeg (hvc_libjpeg_encode.hip) -- libjpeg's chroma averaging; pad: every component written up to
// ceil(actual / 8) * 8 both ways (the encode pipelines' replicated edge; the planes must be whole blocks), else the frame's own samples
hipError_t rgb_to_ycc_libjpeg_device(const uint8_t *d_rgb, const RgbImage &im, int width, int height, int sampling, int n_frames, uint8_t *d_yuv,
                                     size_t yuv_fs, const hvc_component *comps, bool pad, hipStream_t s);
// the mixed colour pass RGB -> planes over a plan of mixed_rgb_encode_plan_build: k_rgb_to_ycc_mixed, or under hvc_set_encode_libjpeg
// k_rgb_to_ycc_libjpeg_mixed on the plan's images with libjpeg_rgb_plan_lanes' lane grid (pad, infos: as there)
int rgb_to_ycc_mixed_launch(hvc_ctx *c, hvc::MixedRgbPlan &plan, int layout, uint8_t *d_planes, const uint8_t *d_rgb, bool profile, bool pad,
                            const hvc_jpeg_info *infos);
hipError_t rgb_to_ycc_device(const uint8_t *d_rgb, const RgbImage &im, int width, int height, int sampling, int n_frames, uint8_t *d_yuv,
                             size_t yuv_fs, const hvc_component *comps, hipStream_t s);
size_t rgb_yuv_span(const hvc_component *comps, int sampling, int w, int h, int cw, int ch); // bytes of a frame record the pass touches
// the arguments every RGB entry point shares; HVC_OK with nothing = true: a width, height or n_frames of 0
int rgb_check_args(const hvc_ctx *c, int sampling, int width, int height, int n_frames, int layout, int where, size_t rgb_row_stride,
                   size_t rgb_frame_stride, RgbImage &im, bool &nothing);
hipError_t rgb_download(const uint8_t *d_rgb, uint8_t *h_rgb, const RgbImage &im, int n_frames, hipStream_t s); // only the bytes written

// hvc_capi_files.hip: the default code tables in c->hd_tables (uploaded by the first call)
int upload_enc_tables(hvc_ctx *c);
// hvc_capi_files.hip: geometry + scratch + tables of one GPU Huffman coder call (hvc_huff.hip)
int huffman_prepare(hvc_ctx *c, const hvc_jpeg_info *info, const int16_t *d_coefs, size_t coef_fs, int n_frames, uint8_t *d_out,
                    size_t out_cap, unsigned long long *d_offsets, hvc::HuffParams &P, bool optimised = false, int restart = 0);

#endif
