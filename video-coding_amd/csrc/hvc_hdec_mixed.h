// hvc_hdec_mixed.h -- the GPU Huffman reader for files of DIFFERENT geometry in one chain of launches (internal).
// Everything a lane needs about its file comes from a descriptor in device memory (hvc_hdec_mixed_plan.h), not from kernel
// arguments; the verdict is one status word per FILE.
#ifndef HVC_HDEC_MIXED_H
#define HVC_HDEC_MIXED_H

#include <hip/hip_runtime.h>

#include "hvc_hdec_mixed_plan.h"

namespace hvc {

// Synchronisation launches of one run.  After round r the exits of a file's first r + 1 subsequences are the true ones
// (subsequence 0 starts from the truth), so a file of at most HVC_HDM_ROUNDS + 1 subsequences is settled whatever it holds;
// a longer one is settled when its content falls into step within that many hand-overs, and is handed back when not.
#define HVC_HDM_ROUNDS 22
// device bytes of the per-subsequence state for n subsequences
#define HVC_HDM_STATE_BYTES(n) ((size_t)(n) * (3 * sizeof(unsigned long long) + sizeof(unsigned)) + 64)

struct HdmParams {
    const uint8_t *ecs;        // the chunk's segment buffer (HVC_HD_ECS_SLACK readable bytes behind plan.seg_bytes)
    const HdmFileK *files;     // [n_files]
    const unsigned *map;       // [n_units] file of every work unit
    const HdFrameTabs *ftabs;  // the chunk's distinct table records
    unsigned n_files, n_units;
    int16_t *coefs;            // what HdmFileK::coef_base counts from (16-byte aligned)
    int16_t *dcd;              // [plan.dcd_entries] DC differences in scan order (write pass -> DC pass)
    // per subsequence: state = bit position | k << 32 | block-in-MCU << 40
    unsigned long long *start_used, *exit_a, *exit_b; // exits of even rounds go to exit_a, of odd rounds to exit_b
    unsigned *nblk;            // blocks completed inside the subsequence, then (scan) index of its first block
    // [n_files] bit 0: invalid code / index out of range / DC category beyond 15 inside the coded blocks, bit 1: a DC outside
    // int16, bit 2: fewer blocks than the file needs, bit 3: hand-overs inconsistent (not settled).  Zero: the records count.
    unsigned *status;
};

inline void hdm_carve_state(HdmParams &P, void *mem, size_t n) {
    unsigned long long *sp = (unsigned long long *)mem;
    P.start_used = sp;
    P.exit_a = sp + n;
    P.exit_b = sp + 2 * n;
    P.nblk = (unsigned *)(sp + 3 * n);
}

// Enqueue the whole run on `s`: HVC_HDM_ROUNDS synchronisation launches, the per-file scan, the write pass, the DC pass --
// kernels only.  Afterwards P.status holds every file's verdict; no host round trip in between.
hipError_t launch_hd_mixed(const HdmParams &P, hipStream_t s);

} // namespace hvc
#endif
