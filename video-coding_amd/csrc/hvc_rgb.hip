// hvc_rgb.hip -- JFIF colour conversion (ITU-T T.871) in both directions, fused with the chroma resampling in front of /
// behind it: decoded planes -> RGB (k_ycc_to_rgb) and RGB -> the encoder's planes (k_rgb_to_ycc).  The definition every
// byte is tested against (tools/rgb_reference.py):
//     full-size chroma   Planar_444.supersample_hv2 (4:2:0) / supersample_h2 (4:2:2) of the cw x ch window of the chroma
//                        planes (tools/src/planar_444.ml:25-33, 82-103: avg2 / avg4, last column and row repeated)
//     colour             libjpeg's 16-bit fixed-point form of the JFIF matrix, cb = Cb - 128, cr = Cr - 128, >> arithmetic:
//                          R = clamp(Y + ((  91881 cr              + 32768) >> 16))
//                          G = clamp(Y + (( -22554 cb - 46802 cr   + 32768) >> 16))
//                          B = clamp(Y + (( 116130 cb              + 32768) >> 16))
//                        and back (every output is in 0 .. 255 already):
//                          Y  = ( 19595 R + 38470 G +  7471 B               + 32768) >> 16
//                          Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//                          Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//     sub-sampling       Planar_444.subsample_hv2 / subsample_h2 (planar_444.ml:18-23, 69-80)
// Three components are always Y, Cb, Cr (no Adobe APP14 transform flag, no CMYK).  Both kernels are byte traffic: a lane
// owns 8 columns of one row (4:2:0: of two rows, so that a chroma row is loaded once for both); the full-size chroma planes
// exist in registers only.  Rows whose bases and strides allow it move as 8-byte pieces, everything else through the
// bounds-checked byte path.  The entry points live with their families: hvc_yuv_to_rgb / hvc_rgb_to_yuv in hvc_yuv.hip,
// hvc_decode_frames_rgb in hvc_capi.hip, the file-level ones in hvc_capi_jpeg.hip.
#include "hvc_ctx.h"
#include "hvc_rgb_dev.h"

namespace {

// S: 420, 422, 444 or 400 (luma only).  Lanes: ceil(w / 8) per lane row; a lane row is one image row (4:2:0: two).
template <int S, int PLANAR>
__global__ __launch_bounds__(256) void k_ycc_to_rgb(RgbOp P) {
    const unsigned groups = (unsigned)(P.w + 7) >> 3, lrows = S == 420 ? (unsigned)(P.h + 1) >> 1 : (unsigned)P.h;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * lrows) return;
    const unsigned lr = t / groups, g = t - lr * groups;
    const size_t f = blockIdx.y;
    HVC_YCC_LANE_TO_RGB(P, f, lr, g);
}

// The way back; w even for 4:2:2 and 4:2:0, h even for 4:2:0 (the launch checks).  A lane's 8 columns give 4 chroma samples.
template <int S, int PLANAR>
__global__ __launch_bounds__(256) void k_rgb_to_ycc(RgbOp P) {
    const unsigned groups = (unsigned)(P.w + 7) >> 3, lrows = S == 420 ? (unsigned)P.h >> 1 : (unsigned)P.h;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * lrows) return;
    const unsigned lr = t / groups, g = t - lr * groups;
    const size_t f = blockIdx.y;
    HVC_RGB_LANE_TO_YCC(P, f, lr, g);
}

template <int PLANAR>
void launch_to_rgb(int sampling, dim3 grid, hipStream_t s, const RgbOp &P) {
    switch (sampling) {
    case HVC_YUV_420: hipLaunchKernelGGL((k_ycc_to_rgb<420, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_422: hipLaunchKernelGGL((k_ycc_to_rgb<422, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_444: hipLaunchKernelGGL((k_ycc_to_rgb<444, PLANAR>), grid, dim3(256), 0, s, P); break;
    default: hipLaunchKernelGGL((k_ycc_to_rgb<400, PLANAR>), grid, dim3(256), 0, s, P); break;
    }
}
template <int PLANAR>
void launch_to_ycc(int sampling, dim3 grid, hipStream_t s, const RgbOp &P) {
    switch (sampling) {
    case HVC_YUV_420: hipLaunchKernelGGL((k_rgb_to_ycc<420, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_422: hipLaunchKernelGGL((k_rgb_to_ycc<422, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_444: hipLaunchKernelGGL((k_rgb_to_ycc<444, PLANAR>), grid, dim3(256), 0, s, P); break;
    default: hipLaunchKernelGGL((k_rgb_to_ycc<400, PLANAR>), grid, dim3(256), 0, s, P); break;
    }
}

bool is_sampling(int s) { return s == HVC_YUV_420 || s == HVC_YUV_422 || s == HVC_YUV_444 || s == HVC_YUV_400; }

// either direction on device memory, in launches of at most 65535 frames (the grid's second dimension)
hipError_t launch_colour(bool to_rgb, const uint8_t *yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int w, int h, int cw,
                         int ch, int n_frames, const uint8_t *rgb, const RgbImage &im, hipStream_t s) {
    if (n_frames <= 0 || w <= 0 || h <= 0) return hipSuccess;
    const bool grey = sampling == HVC_YUV_400;
    RgbOp P;
    std::memset(&P, 0, sizeof P);
    P.w = w, P.h = h, P.cw = cw, P.ch = ch;
    P.y_stride = comps[0].stride;
    P.cb_stride = grey ? 0 : comps[1].stride, P.cr_stride = grey ? 0 : comps[2].stride;
    P.yuv_fs = yuv_fs;
    P.row_stride = im.row_stride, P.frame_stride = im.frame_stride, P.plane_stride = im.row_stride * (size_t)h;
    const unsigned lrows = sampling == HVC_YUV_420 ? (unsigned)(to_rgb ? (h + 1) >> 1 : h >> 1) : (unsigned)h;
    const unsigned long long lanes = (unsigned long long)((w + 7) >> 3) * lrows;
    if (lanes == 0) return hipSuccess;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {
        const int cnt = n_frames - f0 < 65535 ? n_frames - f0 : 65535;
        uint8_t *base = const_cast<uint8_t *>(yuv) + (size_t)f0 * yuv_fs;
        P.y = base + comps[0].plane_offset;
        P.cb = grey ? nullptr : base + comps[1].plane_offset;
        P.cr = grey ? nullptr : base + comps[2].plane_offset;
        P.rgb = const_cast<uint8_t *>(rgb) + (size_t)f0 * im.frame_stride;
        const size_t ca = sampling == HVC_YUV_444 ? 8 : 4;
        P.vec_y = ((uintptr_t)P.y | P.y_stride | yuv_fs) % 8 == 0;
        P.vec_c = !grey && ((uintptr_t)P.cb | (uintptr_t)P.cr | P.cb_stride | P.cr_stride | yuv_fs) % ca == 0;
        P.vec_rgb = ((uintptr_t)P.rgb | P.row_stride | P.frame_stride | (im.layout == HVC_RGB_PLANAR ? P.plane_stride : 0)) % 8 == 0;
        const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)cnt, 1);
        if (to_rgb) {
            if (im.layout == HVC_RGB_PLANAR) launch_to_rgb<1>(sampling, grid, s, P);
            else launch_to_rgb<0>(sampling, grid, s, P);
        } else {
            if (im.layout == HVC_RGB_PLANAR) launch_to_ycc<1>(sampling, grid, s, P);
            else launch_to_ycc<0>(sampling, grid, s, P);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

// bytes of the planes of one frame record that the colour pass touches: [0, span)
size_t rgb_yuv_span(const hvc_component *comps, int sampling, int w, int h, int cw, int ch) {
    size_t span = comps[0].plane_offset + (size_t)(h - 1) * comps[0].stride + (size_t)w;
    for (int k = 1; k < 3 && sampling != HVC_YUV_400; k++)
        span = std::max(span, comps[k].plane_offset + (size_t)(ch - 1) * comps[k].stride + (size_t)cw);
    return span;
}

// the arguments every entry point shares: HVC_OK with *nothing = true when there is nothing to write
int rgb_check_args(const hvc_ctx *c, int sampling, int width, int height, int n_frames, int layout, int where, size_t rgb_row_stride,
                 size_t rgb_frame_stride, RgbImage &im, bool &nothing) {
    if (!c || !is_sampling(sampling) || width < 0 || height < 0 || n_frames < 0) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    if (!rgb_image(layout, width, height, rgb_row_stride, rgb_frame_stride, im)) return HVC_E_INVALID_ARG;
    if (width > (1 << 24) || height > (1 << 24) || (unsigned long long)((width + 7) / 8) * (unsigned long long)height >= (1ull << 31)) return HVC_E_TOO_LARGE;
    nothing = width == 0 || height == 0 || n_frames == 0;
    return HVC_OK;
}


bool rgb_image(int layout, int width, int height, size_t row_stride, size_t frame_stride, RgbImage &im) {
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return false;
    const size_t tight_row = layout == HVC_RGB_PLANAR ? (size_t)width : (size_t)3 * width;
    im.layout = layout;
    im.row_bytes = tight_row;
    im.rows = layout == HVC_RGB_PLANAR ? (size_t)3 * height : (size_t)height; // (planar planes are row_stride * height apart: 3 h rows)
    im.row_stride = row_stride ? row_stride : tight_row;
    if (im.row_stride < tight_row) return false;
    const size_t tight_frame = im.row_stride * im.rows;
    im.frame_stride = frame_stride ? frame_stride : tight_frame;
    return im.frame_stride >= tight_frame;
}

// (rgb_sampling_of and rgb_chroma_window are host rules without HIP: hvc_mixed_rgb_plan.cpp)

hipError_t ycc_to_rgb_device(const uint8_t *d_yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int width, int height, int cw,
                             int ch, int n_frames, uint8_t *d_rgb, const RgbImage &im, hipStream_t s, int arith) {
    if (arith == HVC_ARITH_LIBJPEG) return ycc_to_rgb_fancy_device(d_yuv, yuv_fs, comps, sampling, width, height, cw, ch, n_frames, d_rgb, im, s);
    return launch_colour(true, d_yuv, yuv_fs, comps, sampling, width, height, cw, ch, n_frames, d_rgb, im, s);
}
hipError_t rgb_to_ycc_device(const uint8_t *d_rgb, const RgbImage &im, int width, int height, int sampling, int n_frames, uint8_t *d_yuv,
                             size_t yuv_fs, const hvc_component *comps, hipStream_t s) {
    return launch_colour(false, d_yuv, yuv_fs, comps, sampling, width, height, 0, 0, n_frames, d_rgb, im, s);
}
hipError_t rgb_download(const uint8_t *d_rgb, uint8_t *h_rgb, const RgbImage &im, int n_frames, hipStream_t s) {
    if (im.row_stride == im.row_bytes && im.frame_stride == im.row_stride * im.rows)
        return hipMemcpyAsync(h_rgb, d_rgb, im.frame_stride * (size_t)n_frames, hipMemcpyDeviceToHost, s);
    for (int f = 0; f < n_frames; f++) { // (only what was written: the caller's padding stays)
        const hipError_t e = hipMemcpy2DAsync(h_rgb + (size_t)f * im.frame_stride, im.row_stride, d_rgb + (size_t)f * im.frame_stride,
                                              im.row_stride, im.row_bytes, im.rows, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
size_t rgb_bytes(const RgbImage &im, int n_frames) { // from the first byte to the last one written
    return n_frames < 1 || !im.rows ? 0 : (size_t)(n_frames - 1) * im.frame_stride + (im.rows - 1) * im.row_stride + im.row_bytes;
}
