// hvc_mixed_scaled.hip -- k_decode_mixed_scaled: the block stage at 1/2, 1/4 or 1/8 size (N = 4, 2, 1 samples per block
// side) over frames of DIFFERENT geometry and quantiser tables in one launch.
//
// The decomposition is the block stage's of hvc_mixed_dev.h (tables of hvc_mixed_plan.h built for N).  Per lane it is
// k_decode_scaled's block (hvc_scaled_dev.h, shared with hvc_scaled.hip): N = 4 and 2 read the 128-byte record as eight
// 16-byte loads, multiply only the positions the definition uses, and run the int32 path under the guard of
// hvc_scaled_spec.h or the int64 path in the same lane; N = 1 reads the dword that holds the DC.  No LDS, no scratch, no
// fix-up list: the blocks of the int64 branch are counted into P.wide_total, one atomic per wavefront that has any.
//
// Where k_decode_scaled chooses dword or byte stores for a whole launch, here the descriptor says it per plane
// (MixedPlaneK::dwords, a wave-uniform branch): a plane whose first byte and stride are multiples of 4 leaves as dwords (N =
// 2 and 1 join pairs / quads by DPP), every other plane as 2-byte / 1-byte stores.  A unit starts at a multiple of 64
// blocks of its plane, so the lane number within the unit decides pairs and quads exactly as the lane of a tile does in
// k_decode_scaled.  Inactive lanes stay clamped to the plane's last block and never store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_mixed.h"
#include "hvc_mixed_dev.h"
#include "hvc_scaled_dev.h"

namespace hvc {
namespace {

template <int N>
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_decode_mixed_scaled(MixedParams P) {
    const MixedWave W = mixed_wave_xcd(P.xcd_map, P.xcd_magic);
    if (W.unit >= P.n_units) return;
    const MixedPlaneK &K = P.planes[P.map[W.unit]];
    const int *__restrict__ q = P.tables[K.table].qt; // wave-uniform
    const auto B = mixed_block<N>(K, W.unit, W.lane, P.coefs, P.pixels);

    unsigned out[N];
    bool wide = false;
    if constexpr (N == 1) {
        out[0] = block1((int)(short)(*reinterpret_cast<const unsigned *>(B.rec) & 0xffffu), q[0]);
    } else {
        unsigned w[32];
        HVC_SCALED_LOAD_RECORD(B.rec, w);
        bool narrow;
        HVC_SCALED_BLOCK(N, w, q, out, narrow);
        wide = B.active && !narrow;
    }

    if (K.dwords) { // wave-uniform
        HVC_SCALED_STORE_DWORDS(N, B.pix, B.stride, out, W.lane, (int)B.bx, B.bw, B.active);
    } else {
        HVC_SCALED_STORE_BYTES(N, B.pix, B.stride, out, B.active);
    }

    if constexpr (N > 1) {
        const unsigned long long m = __ballot(wide);
        if (m && W.lane == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

} // namespace

hipError_t launch_decode_mixed_scaled(const MixedParams &P, int n, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (n != 4 && n != 2 && n != 1) return hipErrorInvalidValue;
    return mixed_launch_xcd(n == 4 ? k_decode_mixed_scaled<4> : n == 2 ? k_decode_mixed_scaled<2> : k_decode_mixed_scaled<1>, P, s, k0, k1);
}

} // namespace hvc
