// hvc_hardcaml.h -- the Hardcaml RTL twin of the block stage (hvc_hardcaml.hip): parameters and launchers (internal).
#ifndef HVC_HARDCAML_H
#define HVC_HARDCAML_H

#include "hvc_kernels.h"

namespace hvc {

struct HardcamlParams {
    const int16_t *coefs;
    uint8_t *pixels;  // the twin's output (store form), or the model's pixels to compare with (divergence form)
    size_t coef_fs;   // int16 elements between frames
    size_t pixel_fs;  // bytes between frames
    int n_frames, n_comp, tiles_per_frame;
    int xcd_map;       // as in DecodeParams
    unsigned xcd_magic;
    CompK comp[HVC_MAX_COMP];
    // per table and record dword i: ((q[2i] & 0xff) << 4) | ((q[2i+1] & 0xff) << 4) << 16, zig-zag order (hvc_hardcaml_spec.h)
    unsigned qq[HVC_MAX_QTABS * 32];
    const int16_t *dc_plane; // as in DecodeParams (absolute DC read instead of the record's coefficient 0)
    size_t dc_fs;
    // divergence form: one byte per block, diff[frame * diff_fs + blk0[component] + block index inside the plane]
    uint8_t *diff;
    size_t diff_fs;
    int blk0[HVC_MAX_COMP];
};

// the kernel-side table of hvc_hardcaml_spec.h's dequantisation from 16-bit zig-zag tables
void prepare_hardcaml_tables(const uint16_t *qtabs, int n_qtabs, unsigned *qq);
// every block of P (grid = tiles x frames, one block per lane): pixels, or (P.diff set) divergence bytes
hipError_t launch_hardcaml(const HardcamlParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);
// the listed blocks (fix-list ids of P's geometry, *count entries) again, coefficient 0 = dcs[i] (hvc_hdec.h WideDc)
hipError_t launch_hardcaml_dcfix(const HardcamlParams &P, const unsigned *count, const unsigned *ids, const long long *dcs,
                                 hipStream_t s);

// The encoder twin (k_hardcaml_encode, hvc_hardcaml_fwd_spec.h): the Hardcaml RTL encoder's forward DCT and quantiser.
struct HardcamlEncodeParams {
    const uint8_t *pixels;
    int16_t *coefs;   // the twin's records (store form), or the model's records to compare with (divergence form)
    size_t coef_fs;   // int16 elements between frames
    size_t pixel_fs;  // bytes between frames
    int n_frames, n_comp, tiles_per_frame;
    int xcd_map;      // as in EncodeParams
    unsigned xcd_magic;
    CompK comp[HVC_MAX_COMP];
    // per table, natural position k: (QR_NUM / table[Zigzag.forward[k]]) << QR_SCALE (hvc_hardcaml_fwd_spec.h)
    int qr[HVC_MAX_QTABS * 64];
    // divergence form: one byte per block, diff[frame * diff_fs + blk0[component] + block index inside the plane]
    uint8_t *diff;
    size_t diff_fs;
    int blk0[HVC_MAX_COMP];
};

// the kernel-side reciprocals of hvc_hardcaml_fwd_spec.h from zig-zag tables with entries in 1..255
void prepare_hardcaml_encode_tables(const uint16_t *qtabs, int n_qtabs, int *qr);
// every block of P (grid = tiles x frames, one block per lane): coefficient records, or (P.diff set) divergence bytes
hipError_t launch_hardcaml_encode(const HardcamlEncodeParams &P, hipStream_t s, hipEvent_t k0 = nullptr,
                                  hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
