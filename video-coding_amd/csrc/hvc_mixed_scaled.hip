// hvc_mixed_scaled.hip -- k_decode_mixed_scaled: the block stage at 1/2, 1/4 or 1/8 size (N = 4, 2, 1 samples per block
// side) over frames of DIFFERENT geometry and quantiser tables in one launch.
//
// The decomposition is k_decode_mixed's (hvc_mixed.hip, tables of hvc_mixed_plan.h built for N): a work unit is 64
// consecutive blocks of ONE plane = one wavefront, a workgroup is four units, the map entry, the plane descriptor and the
// table entry are wave-uniform and come through scalar loads, the groups go over the XCDs by xcd_work.  Per lane it is
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

#include "hvc_kernels.h" /* xcd_work, xcd_map_for */
#include "hvc_mixed.h"
#include "hvc_scaled_dev.h"

namespace hvc {
namespace {

#define HVC_MIXED_LANES (HVC_MIXED_UNIT * HVC_MIXED_GROUP)

template <int N>
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_decode_mixed_scaled(MixedParams P) {
    unsigned wf, wt;
    xcd_work(P.xcd_map, P.xcd_magic, wf, wt); // gridDim.y == 1: a permutation of the groups (or the plain order)
    const unsigned group = wf * gridDim.x + wt;
    const int lane = threadIdx.x & (HVC_MIXED_UNIT - 1);
    const unsigned unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(group * HVC_MIXED_GROUP + (threadIdx.x >> 6)));
    if (unit >= P.n_units) return; // (the whole wavefront: the last group's spare units)
    const MixedPlaneK &K = P.planes[P.map[unit]];
    const int *__restrict__ q = P.tables[K.table].qt; // wave-uniform
    int b = (int)(unit - K.unit0) * HVC_MIXED_UNIT + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1;
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const int bx = (int)((unsigned)b - by * (unsigned)K.bw);
    const int bw = K.bw;
    const size_t stride = (size_t)K.stride;
    const int16_t *rec = P.coefs + (size_t)K.coef_base + (size_t)b * 64;
    uint8_t *dst = P.pixels + (size_t)K.pix_base + (size_t)by * N * stride + (size_t)bx * N;

    unsigned out[N];
    bool wide = false;
    if constexpr (N == 1) {
        out[0] = block1((int)(short)(*reinterpret_cast<const unsigned *>(rec) & 0xffffu), q[0]);
    } else {
        unsigned w[32];
        HVC_SCALED_LOAD_RECORD(rec, w);
        bool narrow;
        HVC_SCALED_BLOCK(N, w, q, out, narrow);
        wide = active && !narrow;
    }

    if (K.dwords) { // wave-uniform
        HVC_SCALED_STORE_DWORDS(N, dst, stride, out, lane, bx, bw, active);
    } else {
        HVC_SCALED_STORE_BYTES(N, dst, stride, out, active);
    }

    if constexpr (N > 1) {
        const unsigned long long m = __ballot(wide);
        if (m && lane == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

} // namespace

hipError_t launch_decode_mixed_scaled(const MixedParams &P, int n, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (n != 4 && n != 2 && n != 1) return hipErrorInvalidValue;
    if (P.n_units == 0) return hipSuccess;
    hipError_t e;
    const unsigned groups = (P.n_units + HVC_MIXED_GROUP - 1) / HVC_MIXED_GROUP;
    MixedParams Q = P;
    Q.xcd_map = xcd_map_for(groups, 1, Q.xcd_magic); // (0 beyond 65535 groups: the plain order)
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (n == 4) hipLaunchKernelGGL(k_decode_mixed_scaled<4>, dim3(groups), dim3(HVC_MIXED_LANES), 0, s, Q);
    else if (n == 2) hipLaunchKernelGGL(k_decode_mixed_scaled<2>, dim3(groups), dim3(HVC_MIXED_LANES), 0, s, Q);
    else hipLaunchKernelGGL(k_decode_mixed_scaled<1>, dim3(groups), dim3(HVC_MIXED_LANES), 0, s, Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc
