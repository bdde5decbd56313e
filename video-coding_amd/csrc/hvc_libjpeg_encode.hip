// hvc_libjpeg_encode.hip -- the kernels of hvc_set_encode_libjpeg: the encoder of include/hvc_jpeg.h ("Encoding bit-exact to
// libjpeg"), gfx950.  A translation unit of its own, as hvc_libjpeg.hip is for the decoder: the measured kernels of
// hvc_kernels.hip keep their build id.
//
// k_fdct_islow: k_encode's launch geometry and record layout (grid = tiles of HVC_TILE blocks x frames, XCD workgroup order,
// one block per lane, the component from the tile index), with jfdctint.c's forward DCT (hvc_fdct_islow_spec.h expanded by
// hvc_fdct_islow_dev.h) and libjpeg's rounded division (one host-made 24-bit multiplier per table entry, kernarg segment -> scalar
// loads).  Mapping: one block per lane, both passes in registers -- a lane's eight row loads are its own block's, so no
// exchange is needed before the store; the store is k_encode's: the wave's 64 records through LDS (XOR-swizzled 16-byte
// slots) and out as whole 1 KiB runs.  LDS per workgroup: 32 KiB, as k_encode.  8-bit input: no guard, no wide path.
//
// k_dummy_blocks: the dummy blocks of libjpeg's padded layout (blocks past ceil(actual / 8) in either direction), one lane
// per dummy block, after k_fdct_islow on the same stream: it reads the DC of its source block (a REAL block: the host-proved
// closed form of hvc_libjpeg_encode_plan.h resolves the chain, so no lane waits for another) and writes the 64 coefficients.
// A pass of its own leaves k_fdct_islow's registers and its whole-run stores alone; a frame has at most one column and one
// row of MCUs' worth of dummies, so the pass is small.
//
// k_rgb_to_ycc_libjpeg: the colour pass in front of the block stage with libjpeg's chroma averaging; its lane, the edges it
// writes and why are in hvc_rgb_libjpeg_dev.h.  The three kernels' mixed twins expand the same device code under the
// decomposition of hvc_mixed_dev.h.
#include "hvc_libjpeg_encode.h"

#include "hvc_fdct_islow_dev.h"
#include "hvc_mixed_dev.h"
#include "hvc_rgb_libjpeg_dev.h"

namespace hvc {

__global__ __launch_bounds__(HVC_TILE) void k_fdct_islow(FdctIslowParams P) {
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && (int)wtile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    const int tile_b0 = ((int)wtile - K.tile0) * HVC_TILE;
    int b = tile_b0 + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1; // (inactive lanes read the plane's last block and store nothing)
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const uint8_t *pix = P.pixels + (size_t)wframe * P.pixel_fs + K.plane_off + (size_t)by * 8 * K.stride + (size_t)bx * 8;
    const size_t plane_coef_idx = (size_t)wframe * P.coef_fs + K.coef_off;
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    unsigned px[8][2];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u2v t = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(pix + (size_t)j * K.stride));
        px[j][0] = t.x;
        px[j][1] = t.y;
    }
    unsigned out[32];
    fdct_islow_block(px, P.magic + K.qtab * 64, P.half + K.qtab * 64, out);
    // k_encode's store: the wave's 64 records through LDS (XOR-swizzled 16-byte slots, conflict-free both ways), out as
    // whole 1 KiB runs (lane i of store j writes byte 1024 j + 16 i of the wave's coefficient run)
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    __shared__ u4v lds[HVC_TILE / 64][512];
    const int wv = lane >> 6, l = lane & 63;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u4v t = {out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]};
        lds[wv][l * 8 + (j ^ (l & 7))] = t;
    }
    // (wave-private LDS region: the wave's own ds ops are ordered, no barrier needed)
    const int wave_b0 = tile_b0 + (lane & ~63);
    u4v *dst = reinterpret_cast<u4v *>(P.coefs + plane_coef_idx + (size_t)wave_b0 * 64);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int blk = 8 * j + (l >> 3), ch = l & 7;
        const u4v t = lds[wv][blk * 8 + (ch ^ (blk & 7))];
        if (wave_b0 + blk < K.nblk) __builtin_nontemporal_store(t, dst + j * 64 + l);
    }
}

hipError_t launch_fdct_islow(const FdctIslowParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    FdctIslowParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic);
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_fdct_islow, grid, dim3(HVC_TILE), 0, s, Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

// ---------------------------------------------------------------------------
constexpr int DUMMY_LANES = 256;

__global__ __launch_bounds__(DUMMY_LANES) void k_dummy_blocks(DummyBlocksParams P) {
    int i = (int)(blockIdx.x * DUMMY_LANES + threadIdx.x);
    if (i >= P.total) return;
    int c = 0;
#pragma unroll
    for (int k = 1; k < HVC_MAX_COMP; k++)
        if (k < P.n_comp && i >= P.comp[k].first) c = k;
    const int bw = P.comp[c].bw, real_w = P.comp[c].real_w, real_h = P.comp[c].real_h, h = P.comp[c].h;
    i -= P.comp[c].first;
    int bx, by;
    libjpeg_dummy_at(i, bw, real_w, real_h, bx, by);
    const int src = libjpeg_dummy_source(bx, by, bw, real_w, real_h, h);
    int16_t *plane = P.coefs + (size_t)blockIdx.y * P.coef_fs + P.comp[c].coef_off;
    const unsigned dc = (unsigned short)plane[(size_t)src * 64];
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    u4v *dst = reinterpret_cast<u4v *>(plane + (size_t)(bx + by * bw) * 64);
    const u4v first = {dc, 0u, 0u, 0u}, zero = {0u, 0u, 0u, 0u};
    dst[0] = first;
#pragma unroll
    for (int j = 1; j < 8; j++) dst[j] = zero;
}

// ---------------------------------------------------------------------------
// The mixed twins: the decomposition of hvc_mixed_dev.h, the block of hvc_fdct_islow_dev.h
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_fdct_islow_mixed(FdctIslowMixedParams P) {
    unsigned wf, wt;
    xcd_work(P.xcd_map, P.xcd_magic, wf, wt); // gridDim.y == 1: a permutation of the groups (or the plain order)
    const unsigned group = wf * gridDim.x + wt;
    const int wv = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & (HVC_MIXED_UNIT - 1));
    const unsigned unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(group * HVC_MIXED_GROUP + (unsigned)wv));
    if (unit >= P.n_units) return; // (the whole wavefront: the last group's spare units; no barrier below)
    const MixedPlaneK &K = P.planes[P.map[unit]];
    const FdctIslowTableK &T = P.tables[K.table];
    const int wave_b0 = (int)(unit - K.unit0) * HVC_MIXED_UNIT; // block (inside the plane) of lane 0
    const int nblk = K.nblk;
    int b = wave_b0 + l;
    b = b < nblk ? b : nblk - 1; // an inactive lane computes the plane's last block and stores nothing
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const size_t stride = (size_t)K.stride;
    const uint8_t *pix = P.pixels + (size_t)K.pix_base + (size_t)by * 8 * stride + (size_t)bx * 8;
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    unsigned px[8][2];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u2v t = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(pix + (size_t)j * stride));
        px[j][0] = t.x;
        px[j][1] = t.y;
    }
    unsigned out[32];
    fdct_islow_block(px, T.magic, T.half, out);
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    __shared__ u4v lds[HVC_MIXED_GROUP][512];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u4v t = {out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]};
        lds[wv][l * 8 + (j ^ (l & 7))] = t;
    }
    // (wave-private LDS region: the wave's own ds ops are ordered, no barrier needed)
    u4v *dst = reinterpret_cast<u4v *>(P.coefs + (size_t)K.coef_base + (size_t)wave_b0 * 64);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int blk = 8 * j + (l >> 3), ch = l & 7;
        const u4v t = lds[wv][blk * 8 + (ch ^ (blk & 7))];
        if (wave_b0 + blk < nblk) __builtin_nontemporal_store(t, dst + j * 64 + l);
    }
}

hipError_t launch_fdct_islow_mixed(const FdctIslowMixedParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch_xcd(k_fdct_islow_mixed, P, s, k0, k1);
}

__global__ __launch_bounds__(DUMMY_LANES) void k_dummy_blocks_mixed(int16_t *coefs, const DummyPairK *pairs, unsigned n) {
    const unsigned i = blockIdx.x * DUMMY_LANES + threadIdx.x;
    if (i >= n) return;
    const DummyPairK p = pairs[i];
    const unsigned dc = (unsigned short)coefs[p.src];
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    u4v *dst = reinterpret_cast<u4v *>(coefs + p.dst);
    const u4v first = {dc, 0u, 0u, 0u}, zero = {0u, 0u, 0u, 0u};
    dst[0] = first;
#pragma unroll
    for (int j = 1; j < 8; j++) dst[j] = zero;
}

hipError_t launch_dummy_blocks_mixed(int16_t *coefs, const DummyPairK *pairs, unsigned n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dummy_blocks_mixed, dim3((n + DUMMY_LANES - 1) / DUMMY_LANES), dim3(DUMMY_LANES), 0, s, coefs, pairs, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The colour pass in front of the block stage (hvc_rgb_libjpeg_dev.h)
__global__ __launch_bounds__(256) void k_rgb_to_ycc_libjpeg(RgbLibjpegParams P) {
    const unsigned lane = blockIdx.x * 256u + threadIdx.x;
    if (lane >= P.image.lanes) return;
    rgb_to_ycc_libjpeg_lane(P.image, lane, P.rgb + (size_t)blockIdx.y * P.rgb_fs, P.yuv + (size_t)blockIdx.y * P.yuv_fs, P.planar != 0, P.pad != 0);
}

hipError_t launch_rgb_to_ycc_libjpeg(const RgbLibjpegParams &P, hipStream_t s) {
    if (P.n_frames <= 0 || P.image.lanes == 0) return hipSuccess;
    for (int f0 = 0; f0 < P.n_frames; f0 += 65535) { // (the grid's y dimension)
        RgbLibjpegParams Q = P;
        Q.n_frames = P.n_frames - f0 < 65535 ? P.n_frames - f0 : 65535;
        Q.rgb = P.rgb + (size_t)f0 * P.rgb_fs;
        Q.yuv = P.yuv + (size_t)f0 * P.yuv_fs;
        hipLaunchKernelGGL(k_rgb_to_ycc_libjpeg, dim3((P.image.lanes + 255) / 256, (unsigned)Q.n_frames), dim3(256), 0, s, Q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

__global__ __launch_bounds__(HVC_MIXED_LANES) void k_rgb_to_ycc_libjpeg_mixed(RgbLibjpegMixedParams P) {
    const MixedWave W = mixed_wave_plain();
    if (W.unit >= P.n_units) return;
    const MixedRgbImageK &K = P.images[P.map[W.unit]];
    MixedImageLane L;
    if (!mixed_image_lane(K, W.unit, W.lane, L)) return;
    rgb_to_ycc_libjpeg_lane(K, L.t, P.rgb, P.yuv, P.planar != 0, P.pad != 0); // (it splits t into row and group itself)
}

hipError_t launch_rgb_to_ycc_libjpeg_mixed(const RgbLibjpegMixedParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch(k_rgb_to_ycc_libjpeg_mixed, P, s, k0, k1);
}

bool dummy_blocks_geometry(DummyBlocksParams &P, int n_comp, const int *bw, const int *bh, const int *real_w, const int *real_h,
                           const int *h, const size_t *coef_off) {
    P = DummyBlocksParams();
    if (n_comp < 1 || n_comp > HVC_MAX_COMP) return false;
    P.n_comp = n_comp;
    for (int i = 0; i < n_comp; i++) {
        if (real_w[i] < 1 || real_w[i] > bw[i] || real_h[i] < 1 || real_h[i] > bh[i] || h[i] < 1) return false;
        DummyCompK &K = P.comp[i];
        K.bw = bw[i];
        K.real_w = real_w[i];
        K.real_h = real_h[i];
        K.h = h[i];
        K.first = P.total;
        K.coef_off = coef_off[i];
        P.total += libjpeg_dummy_count(bw[i], bh[i], real_w[i], real_h[i]);
    }
    return true;
}

hipError_t launch_dummy_blocks(const DummyBlocksParams &P, hipStream_t s) {
    if (P.n_frames <= 0 || P.total <= 0) return hipSuccess;
    const dim3 grid((unsigned)((P.total + DUMMY_LANES - 1) / DUMMY_LANES), (unsigned)P.n_frames, 1);
    hipLaunchKernelGGL(k_dummy_blocks, grid, dim3(DUMMY_LANES), 0, s, P);
    return hipGetLastError();
}

} // namespace hvc
