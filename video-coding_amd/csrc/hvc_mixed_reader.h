// hvc_mixed_reader.h -- the mixed GPU Huffman reader (hvc_hdec_mixed.hip) as the batch pipeline of hvc_capi_mixed.hip and
// hvc_jpeg_entropy_decode_gpu_mixed drive it (internal; defined in hvc_capi_mixed_reader.hip).
//
// A chunk is a run of files; chunk k lives in slot k % RING of the context's reader rings (reader_rings: pinned / device
// segments, descriptors + map + verdicts, table records).  Per chunk:
//   prepare(k, t)   any thread, once per file: the file's segment unstuffed into the pinned slot at a place known from the
//                   file's size alone, its table set found among the chunk's (make_frame_tabs for one not seen yet)
//   upload(k, s)    the orchestrating thread, once the chunk's files are prepared: the plan (hvc_hdec_mixed_plan.h), then
//                   segments, descriptors, map and table records on stream s
//   read(k, d, s)   the reader's launches into the coefficient records at d on stream s, the per-file verdict read back
//                   (the one host synchronisation of the chunk); names the files that go to the host reader
// A file goes to the host reader when its verdict is not clean, when the reader cannot take it (hdm_geometry, tables that
// are no prefix code), when its segment or its table set does not fit the chunk's slot, or when it carries restart
// intervals while they are honoured.
#ifndef HVC_MIXED_READER_H
#define HVC_MIXED_READER_H

#include <memory>
#include <mutex>
#include <vector>

#include "hvc_ctx.h"
#include "hvc_hdec_mixed_plan.h"

// table records a chunk's slot has room for (62 KB each, pinned and on the device, per ring slot): a chunk of more distinct
// table sets sends the files of the later ones to the host reader
#define HVC_HDM_MAX_TABLE_SETS 512

class MixedGpuReader {
  public:
    // files[first_of(k) .. + count_of(k)) of `take` (indices into jpegs / sizes / infos / coef_base) are chunk k.  Sizes
    // the rings and the reader's device scratch; nothing is enqueued.  coef_base: int16 elements from the pointer read() is given.
    int begin(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, const hvc_jpeg_info *infos, const size_t *coef_base,
              const std::vector<int> &take, const std::vector<int> &chunk_first, const std::vector<int> &chunk_count);
    void prepare(int k, int t);
    hipError_t upload(int k, hipStream_t s);
    // back[f] = 1 for every file of the chunk the host reader must take; *gpu_files: the others
    int read(int k, int16_t *d_coefs, hipStream_t s, std::vector<char> &back, int *gpu_files);

  private:
    struct SlotFile {
        size_t seg_bytes = 0;
        int set = -1;
        bool ok = false;
    };
    struct Slot {
        std::mutex mu;
        int chunk = -1;
        std::vector<hvc::HdTables> sets;
        std::vector<SlotFile> files; // by position in the chunk
        hvc::HdmPlan plan;
        size_t status_at = 0;        // bytes from the slot's device meta buffer
    };
    hvc_ctx *c_ = nullptr;
    const uint8_t *const *jpegs_ = nullptr;
    const size_t *sizes_ = nullptr, *coef_base_ = nullptr;
    const hvc_jpeg_info *infos_ = nullptr;
    const std::vector<int> *take_ = nullptr, *first_ = nullptr, *count_ = nullptr;
    std::vector<size_t> ecs_off_;   // by position in `take`: where the file's segment goes in its chunk's slot
    std::vector<int> geo_;          // by position in `take`: hdm_geometry's answer
    size_t ecs_cap_ = 0, sets_cap_ = 0;
    std::unique_ptr<Slot[]> slots_;
    std::vector<unsigned> verdict_;
};

#endif
