// hvc_libjpeg.h -- the libjpeg-exact forms of the block stage and the colour pass (hvc_libjpeg.hip; hvc_set_arithmetic
// HVC_ARITH_LIBJPEG): parameters and launchers (internal).
#ifndef HVC_LIBJPEG_H
#define HVC_LIBJPEG_H

#include "hvc_kernels.h"

namespace hvc {

struct IslowParams {
    const int16_t *coefs;
    uint8_t *pixels;
    size_t coef_fs;   // int16 elements between frames
    size_t pixel_fs;  // bytes between frames
    int n_frames, n_comp, tiles_per_frame;
    int xcd_map;       // as in DecodeParams
    unsigned xcd_magic;
    CompK comp[HVC_MAX_COMP];
    // per table and record dword i: q[2i] | q[2i+1] << 16, zig-zag order, all 16 bits of every entry
    unsigned qq[HVC_MAX_QTABS * 32];
    const int16_t *dc_plane; // as in DecodeParams (absolute DC read instead of the record's coefficient 0)
    size_t dc_fs;
    unsigned long long *wide_total; // receives the number of blocks that took the int64 path (cleared by the caller)
    int all_wide;                   // hvc_set_decode_kernel(ctx, 2): every block takes the int64 path (nothing is counted)
};

void prepare_islow_tables(const uint16_t *qtabs, int n_qtabs, unsigned *qq);
// every block of P (grid = tiles x frames, one block per lane)
hipError_t launch_islow(const IslowParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
