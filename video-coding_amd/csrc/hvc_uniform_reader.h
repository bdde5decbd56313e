// hvc_uniform_reader.h -- the uniform GPU Huffman reader (hvc_hdec.hip) as the batch pipeline of hvc_jpeg_decode_batch_gpu drives
// it, and the thread that brings a host caller's chunks home (internal; defined in hvc_capi_reader.hip).
//
// A chunk is a run of C files of one geometry; chunk k lives in slot k % RING of the context's reader rings (reader_rings:
// pinned / device segments, index arrays, per-frame table records; the slot's layout: hvc_hdec_plan.h).  Per call:
//   begin(...)     the first file's probe, restart units, chunk size, layout; streams, events, rings and device scratch; the
//                  first file's tables on the device and as record 0 of every slot.  Nothing of a chunk is enqueued.
//   prepare(f)     any thread, once per file: header and geometry check, the segment unstuffed into the pinned slot, the
//                  record of a file with tables of its own; marks the chunk of a file the reader cannot take
//   enqueue(k)     the orchestrating thread, once the chunk's files are prepared: the index arrays, the uploads on the copy
//                  stream, the reader's launches and the read-back of its two flags on rd_stream[k % NRD]; c->stream waits
//                  for them
//   verdict(k)     once the slot's consumers are through: the flags of the chunk, its stage times
// Chunks the GPU reader cannot or must not do (a file with tables that are no prefix code, a stream the model raises on or
// that ends early, rounds that do not settle) are marked (host_chunk) and left to the host-reader pipeline by the caller.
#ifndef HVC_UNIFORM_READER_H
#define HVC_UNIFORM_READER_H

#include <atomic>
#include <mutex>
#include <optional>
#include <vector>

#include "hvc_ctx.h"
#include "hvc_feed.h"
#include "hvc_hdec_plan.h"

class UniformGpuReader {
  public:
    struct Chunk { // what the block stage reads
        const int16_t *coefs;
        const int16_t *dc_plane; // the chunk's compact DC array, or null: the DC values are in the records
        size_t dc_fs;
    };
    // HVC_OK with *host_pipeline = false: ready.  HVC_OK with *host_pipeline = true: the whole call is the host-reader
    // pipeline's (no chunk was enqueued).  form: of() the first file's header on return.  *frames_per_chunk: the caller's wish
    // (< 1: none) in, the chunk size in use out -- also what the host-reader pipeline is given when the call goes there.
    // The device is the context's from here until the reader goes.
    int begin(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int *frames_per_chunk, int where, size_t pixel_fs,
              OutputForm &form, bool *host_pipeline);
    int n_chunks() const { return n_chunks_; }
    int first_of(int k) const { return k * (int)L_.C; }
    int count_of(int k) const { return first_of(k) + (int)L_.C <= n_frames_ ? (int)L_.C : n_frames_ - first_of(k); }
    int prepare(int f, std::mutex &mu); // the status for the feed's report; mu guards the chunks' marks
    hipError_t enqueue(int k, Chunk &out);
    void verdict(int k);
    bool host_chunk(int k) const { return chunk_host_[(size_t)k] != 0; } // (under the mutex while workers run)
    double h2d_ms() const { return h2d_ms_; }
    double kernel_ms() const { return k_ms_; }
    uint64_t ecs_total() const { return ecs_total_; } // bytes uploaded: the unstuffed segments of the chunks enqueued

  private:
    hvc_ctx *c_ = nullptr;
    std::optional<DeviceGuard> guard_;
    const uint8_t *const *jpegs_ = nullptr;
    const size_t *sizes_ = nullptr;
    int n_frames_ = 0, n_chunks_ = 0;
    hvc_jpeg_info info0_;
    hvc::HdParams G_;        // geometry, restart units and the first file's tables: what every chunk's parameters start from
    hvc::HdTables tables0_;
    hvc::HdRestart units_{false, 0, 1};
    hvc::HdChunkLayout L_;
    bool uniform_ok_ = false, pf_fits_ = false, dc_compact_ = false;
    size_t state_bytes_ = 0, dcd_elems_ = 0, dcv_fs_ = 0, dcv_elems_ = 0;
    std::vector<char> frame_pf_, chunk_host_; // the frame has tables of its own; the chunk is the host reader's
    std::vector<unsigned> ecs_size_;
    std::vector<unsigned> unit_off_, unit_len_; // restart intervals: [file][interval] place inside the file's ring region, bytes
    double h2d_ms_ = 0, k_ms_ = 0;
    uint64_t ecs_total_ = 0;
};

// Host output: a thread of its own downloads chunk after chunk on c->down_stream (copies to pageable memory hold their
// caller -- issued from the orchestrating loop they kept the next chunk's launches waiting, and on the block stage's stream
// its kernels too: 18 Gpixel/s, 33 with this).  Its state is guarded by the feed's mutex and waited for on the feed's
// condition variable; a pool task reads it, so it is declared BEFORE the feed (hvc_feed.h).
class ChunkDownloader {
  public:
    explicit ChunkDownloader(int n_chunks) : downloaded_((size_t)n_chunks, 0), skipped_((size_t)n_chunks, 0) {}
    void abort() { abort_.store(1); } // the feed's on_leave (under the lock)
    void attach(hvc::ChunkFeed &feed) { feed_ = &feed; }
    // the pool task (submitted before the workers: it must run beside them, never queue behind them); an hvc_status
    int start(hvc_ctx *c, const UniformGpuReader &rd, uint8_t *pixels, size_t pixel_fs, size_t out_bytes);
    // Chunk k's block stage is enqueued (its end: ev_et[slot][2]).  skipped: nothing was decoded -- the host-reader pipeline
    // fills the chunk in later -- and its pinned slot goes to chunk k + RING under the same lock.
    void hand_over(int k, bool skipped);
    bool skipped(int k) const { return skipped_[(size_t)k] != 0; } // (the orchestrating thread's, which alone writes it)
    hipError_t wait_downloaded(int k); // the chunk's frames have left the device, or the downloader's error
  private:
    hvc::ChunkFeed *feed_ = nullptr;
    std::atomic<int> stage_done_{0}, abort_{0}, err_{0}; // chunks whose block stage is enqueued
    std::vector<char> downloaded_, skipped_;
};

#endif
