// hvc_dct_fixed.h -- the parametric fixed-point DCT of the model (hvc_dct_fixed.hip): tables, the block generator and
// the launchers (internal).
#ifndef HVC_DCT_FIXED_H
#define HVC_DCT_FIXED_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_dct_spec.h"

namespace hvc {

constexpr int DCT_N_ROMS = HVC_DCT_ROM_PREC_MAX + 1;

// What the kernels read, one device buffer: the forward ROM of every rom_prec, then the float64 matrix.
struct DctTables {
    int32_t rom[DCT_N_ROMS][64]; // round_nearest(M[r][c] * 2^p), row-major; the inverse reads it transposed
    double m[64];                // M, the static x86 forward matrix (dct.ml:255-337)
};

// The block generator (hvc_dct_blocks).  Block i, element j (row-major, j = 8 row + col), for seed s and range R:
// u = the (32 i + j / 2)-th output of SplitMix64 seeded with s, i.e. mix(s + 0x9E3779B97F4A7C15 * (32 i + j / 2 + 1))
// (arithmetic mod 2^64); w = its low 32 bits for even j, its high 32 bits for odd j; x = ((w * 2R) >> 32) - R, in [-R, R).
__host__ __device__ inline uint64_t dct_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline void dct_block(uint64_t seed, int range, uint64_t i, int32_t *x) {
    const uint64_t r2 = 2 * (uint64_t)range;
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const uint64_t u = dct_mix64(seed + 0x9E3779B97F4A7C15ull * (32 * i + k + 1));
        x[2 * k] = (int32_t)(((u & 0xffffffffull) * r2) >> 32) - range;
        x[2 * k + 1] = (int32_t)(((u >> 32) * r2) >> 32) - range;
    }
}

// One entry of a search: mode 0 forward, 1 inverse (the error against the float64 reference), 2 round trip (the
// integer error max |x - inverse(forward(x))|).
struct DctCfg {
    int mode, fwd_rom, fwd_tp, inv_rom, inv_tp;
};
// The worst block of one configuration: key = the bit pattern of the error (a non-negative double, so the order of the
// keys is the order of the errors), idx = the block index.  Larger key wins, then the smaller index.
struct DctWorst {
    unsigned long long key, idx;
};

constexpr int DCT_SEARCH_WG = 256;  // lanes per workgroup, one block each
constexpr int DCT_SEARCH_CFGS = 64; // configurations per workgroup (grid y)

// explicit blocks: out = the fixed-point transform of in, one block per lane; a block with an input outside the
// accepted range is not written and sets *bad
hipError_t launch_dct_fixed(const DctTables *tab, int inverse, int rom, int tp, const int32_t *in, int32_t *out,
                            size_t n_blocks, unsigned *bad, hipStream_t s);
// explicit blocks: out = fmul(fmul(F, in), F^T) in float64, F = M (forward) or M^T (inverse)
hipError_t launch_dct_reference(const DctTables *tab, int inverse, const int32_t *in, double *out, size_t n_blocks,
                                hipStream_t s);
// generated blocks [first, first + n) x configurations, all of one mode: slab[cfg * grid_x + x] per workgroup column
// (dct_search_grid_x(n, n_cfg) columns), then worst[cfg]
size_t dct_search_grid_x(uint64_t n_blocks, int n_cfg);
hipError_t launch_dct_search(const DctTables *tab, int mode, const DctCfg *cfg, int n_cfg, uint64_t seed, int range,
                             uint64_t first, uint64_t n_blocks, DctWorst *slab, DctWorst *worst, hipStream_t s,
                             hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
