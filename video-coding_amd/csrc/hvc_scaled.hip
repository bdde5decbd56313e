// hvc_scaled.hip -- k_decode_scaled: coefficient records -> planes at 1/2, 1/4 or 1/8 size (N = 4, 2, 1 samples per block
// side) by the reduced-size inverse DCT of include/hvc_jpeg.h ("Decoding at reduced size"; constants and the int32
// guard: hvc_scaled_spec.h; numpy restatement: tools/scaled_reference.py).
//
// One block per lane with k_decode_packed's geometry (tiles of HVC_TILE consecutive blocks of one plane, grid = tiles x
// frames, the same XCD work map): consecutive lanes hold horizontally consecutive blocks of one block row, so the N bytes
// per lane of an output row are contiguous across the wavefront.  N = 4 stores one dword per lane and row; N = 2 joins the
// two lanes of a pair, N = 1 the four lanes of a quad into one dword by DPP where the pair / quad lies in one block row on a
// 4-byte boundary, and falls back to 2-byte / 1-byte stores where it does not.  The byte form (DW = false) serves planes
// whose rows do not start on 4-byte boundaries.  N = 4 and 2 read the lane's 128-byte record as eight 16-byte loads and
// multiply only the positions the definition uses; N = 1 reads the dword that holds the DC -- or, DCP, nothing but the
// compact DC array.  No LDS, no scratch.
//
// Blocks outside the int32 guard run the same formulas in int64 in the same lane (a rare divergent branch); their number
// goes to P.wide_total with one atomic per wavefront that has such a block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_scaled_dev.h"
#include "hvc_scaled_spec.h"

namespace hvc {
namespace {

struct ScaledRef {
    size_t coef_idx; // int16 element index of the block's 64 coefficients
    size_t rel_blk;  // block index inside the frame's coefficient record (the compact DC array's index)
    size_t pix_idx;  // byte index of the block's top-left output sample
    size_t stride;
    int qtab, bx, bw;
    bool active;
};

// locate() of hvc_kernels.hip with N bytes and N rows per block
template <int N>
__device__ __forceinline__ ScaledRef locate_scaled(const DecodeParams &P, unsigned frame, int tile, int lane) {
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && tile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    int b = (tile - K.tile0) * HVC_TILE + lane;
    ScaledRef r;
    r.active = b < K.nblk;
    b = r.active ? b : K.nblk - 1;
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    r.rel_blk = (K.coef_off >> 6) + (size_t)b;
    r.coef_idx = (size_t)frame * P.coef_fs + K.coef_off + (size_t)b * 64;
    r.pix_idx = (size_t)frame * P.pixel_fs + K.plane_off + (size_t)by * N * K.stride + (size_t)bx * N;
    r.stride = K.stride;
    r.qtab = K.qtab;
    r.bx = (int)bx;
    r.bw = K.bw;
    return r;
}

template <int N, bool DCP, bool DW>
__global__ __launch_bounds__(HVC_TILE) void k_decode_scaled(DecodeParams P) {
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    const ScaledRef br = locate_scaled<N>(P, wframe, (int)wtile, lane);
    const int *__restrict__ q = P.qt + br.qtab * 64; // wave-uniform, kernarg segment
    int16_t dcv = 0;
    if (DCP) dcv = P.dc_plane[(size_t)wframe * P.dc_fs + br.rel_blk];
    unsigned out[N];
    bool wide = false;
    if constexpr (N == 1) {
        int c0 = dcv;
        if (!DCP) c0 = (int)(short)(*reinterpret_cast<const unsigned *>(P.coefs + br.coef_idx) & 0xffffu);
        out[0] = block1(c0, q[0]);
    } else {
        unsigned w[32];
        HVC_SCALED_LOAD_RECORD(P.coefs + br.coef_idx, w);
        if (DCP) w[0] = (w[0] & 0xffff0000u) | (unsigned)(unsigned short)dcv;
        bool narrow;
        HVC_SCALED_BLOCK(N, w, q, out, narrow);
        wide = br.active && !narrow;
    }

    uint8_t *dst = P.pixels + br.pix_idx;
    if constexpr (!DW) HVC_SCALED_STORE_BYTES(N, dst, br.stride, out, br.active);
    else HVC_SCALED_STORE_DWORDS(N, dst, br.stride, out, lane, br.bx, br.bw, br.active);

    if constexpr (N > 1) {
        const unsigned long long m = __ballot(wide);
        if (m && (lane & 63) == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

template <int N>
void launch_n(const DecodeParams &Q, bool dwords, dim3 grid, hipStream_t s) {
    if (Q.dc_plane) {
        if (dwords) hipLaunchKernelGGL((k_decode_scaled<N, true, true>), grid, dim3(HVC_TILE), 0, s, Q);
        else hipLaunchKernelGGL((k_decode_scaled<N, true, false>), grid, dim3(HVC_TILE), 0, s, Q);
    } else {
        if (dwords) hipLaunchKernelGGL((k_decode_scaled<N, false, true>), grid, dim3(HVC_TILE), 0, s, Q);
        else hipLaunchKernelGGL((k_decode_scaled<N, false, false>), grid, dim3(HVC_TILE), 0, s, Q);
    }
}

} // namespace

hipError_t launch_decode_scaled(const DecodeParams &P, int n, bool dwords, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (n != 4 && n != 2 && n != 1) return hipErrorInvalidValue;
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    DecodeParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic); // (xcd_work: every XCD takes runs of consecutive tiles)
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (n == 4) launch_n<4>(Q, dwords, grid, s);
    else if (n == 2) launch_n<2>(Q, dwords, grid, s);
    else launch_n<1>(Q, dwords, grid, s);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc
