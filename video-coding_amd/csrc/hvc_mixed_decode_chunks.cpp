// hvc_mixed_decode_chunks.cpp -- the chunk cut of the mixed decode file pipeline and the copies that take a chunk's output
// back to host memory (hvc_mixed_decode_chunks.h).  Plain C++ (no HIP), usable without a GPU.
#include "hvc_mixed_decode_chunks.h"

#include <algorithm>

#include "hvc_mixed_plan.h"
#include "hvc_mixed_rgb_plan.h"

namespace hvc {

namespace {

size_t up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

} // namespace

int mixed_decode_chunks_build(const hvc_jpeg_info *infos, int *status, const uint8_t *const *jpegs, const size_t *pixel_offsets,
                              size_t pixel_cap, bool have_pixels, int n_files, size_t chunk_bytes, int where, const MixedForm &form,
                              MixedDecodeChunks &plan) {
    plan = MixedDecodeChunks();
    const int N = scaled_side(form.scale_denom);
    if (!N || n_files < 0) return HVC_E_INVALID_ARG;
    if (n_files == 0) return HVC_OK;
    if (!infos || !status || !jpegs || !pixel_offsets) return HVC_E_INVALID_ARG;
    if (form.resized() && (!form.out_heights || (form.filter != HVC_RESIZE_BOX && form.filter != HVC_RESIZE_BILINEAR && form.filter != HVC_RESIZE_BICUBIC)))
        return HVC_E_INVALID_ARG;
    if (chunk_bytes == 0) chunk_bytes = (size_t)64 << 20;
    const bool host = where == HVC_MEM_HOST;
    const size_t n = (size_t)n_files;
    plan.chunk_of.assign(n, -1);
    plan.coef_rel.assign(n, 0);
    plan.pix_rel.assign(n, 0);
    plan.out_bytes.assign(n, 0);
    if (form.rgb()) plan.plane_rel.assign(n, 0), plan.row_bytes.assign(n, 0), plan.rows.assign(n, 0);
    if (form.resized()) plan.rgb_rel.assign(n, 0), plan.rimg.resize(n);
    if (N != 8) plan.scaled.resize(n);
    std::vector<MixedDecodeChunk> &chunks = plan.chunks;
    bool need_pixels = false;
    for (int f = 0; f < n_files; f++) {
        if (status[f] != HVC_OK) continue;
        const hvc_jpeg_info &fi = infos[f];
        if (!jpegs[f] || fi.n_comp < 0 || fi.n_comp > 4) return HVC_E_INVALID_ARG;
        if (N != 8) scaled_info(fi, N, plan.scaled[(size_t)f]);
        const hvc_jpeg_info &oi = plan.out_infos(infos)[f];
        size_t &ob = plan.out_bytes[(size_t)f];
        if (form.rgb()) {
            if (!rgb_sampling_of(fi)) { // as hvc_jpeg_decode_rgb answers it: the file's own result
                status[f] = HVC_E_INVALID_ARG;
                continue;
            }
            if (oi.width < 0 || oi.height < 0) return HVC_E_INVALID_ARG;
            // the size of the file's record in `pixels`: its image's, or (resized) the size the caller names for it
            const int ow = form.resized() ? form.out_widths[f] : oi.width, oh = form.resized() ? form.out_heights[f] : oi.height;
            const size_t stride = form.rgb_row_strides ? form.rgb_row_strides[f] : 0;
            if (form.resized()) { // whether its image can be taken to its size is the file's own result too
                const int rr = resize_image_status_box(oi.width, oi.height, ow, oh, form.filter, form.boxes ? form.boxes + 4 * (size_t)f : nullptr,
                                                       form.mirror ? form.mirror[f] : 0);
                if (rr || (stride && stride < mixed_rgb_row_bytes(form.layout, ow) * form.elem())) {
                    status[f] = rr ? rr : (int)HVC_E_INVALID_ARG;
                    continue;
                }
            }
            const size_t tight = mixed_rgb_row_bytes(form.layout, ow) * (form.resized() ? form.elem() : 1);
            if (stride && stride < tight) return HVC_E_INVALID_ARG;
            plan.row_bytes[(size_t)f] = tight;
            plan.rows[(size_t)f] = mixed_rgb_rows(form.layout, oh);
            ob = mixed_rgb_span(form.layout, ow, oh, stride ? stride : tight);
            if (ob && form.resized() && form.out_elem) ob = (plan.rows[(size_t)f] - 1) * (stride ? stride : tight) + tight; // (typed rows)
        } else {
            ob = oi.pixel_bytes;
            if (N == 8 && ob && (pixel_offsets[f] & 7)) return HVC_E_ALIGNMENT; // (scaled planes: any offset)
        }
        if (ob) {
            if (pixel_offsets[f] > pixel_cap || ob > pixel_cap - pixel_offsets[f]) return HVC_E_INVALID_ARG;
            need_pixels = true;
        }
        const size_t cb = fi.coef_count * sizeof(int16_t);
        if (chunks.empty() || (chunks.back().count > 0 && chunks.back().coef_bytes + cb > chunk_bytes)) {
            chunks.emplace_back();
            chunks.back().first = (int)plan.take.size();
        }
        MixedDecodeChunk &k = chunks.back();
        plan.coef_rel[(size_t)f] = k.coef_bytes / sizeof(int16_t);
        plan.chunk_of[(size_t)f] = (int)chunks.size() - 1;
        if (ob) { // (an image may start anywhere: the slot keeps its offset modulo 8)
            const size_t lo = pixel_offsets[f] & ~(size_t)7;
            k.pix_lo = k.pix_hi ? std::min(k.pix_lo, lo) : lo;
            k.pix_hi = std::max(k.pix_hi, pixel_offsets[f] + ob);
        }
        if (form.rgb()) {
            plan.plane_rel[(size_t)f] = k.plane_bytes;
            k.plane_bytes += up(oi.pixel_bytes, 64);
        }
        if (form.resized()) {
            ResizeImage &im = plan.rimg[(size_t)f];
            im.w = oi.width, im.h = oi.height, im.out_w = form.out_widths[f], im.out_h = form.out_heights[f];
            im.src_offset = plan.rgb_rel[(size_t)f] = k.rgb_bytes, im.src_row_stride = 0;
            im.dst_offset = pixel_offsets[f]; // (host output: from the chunk's pix_lo, below)
            im.dst_row_stride = form.rgb_row_strides ? form.rgb_row_strides[f] : 0;
            const size_t planes = form.layout == HVC_RGB_PLANAR ? 3 : 1;
            k.rgb_bytes += up(mixed_rgb_span(form.layout, oi.width, oi.height, mixed_rgb_row_bytes(form.layout, oi.width)), 64);
            // (an upper bound of what resize_plan_build gives it: rows on 4 bytes, the image on 64)
            k.mid_bytes += 64 + up(mixed_rgb_row_bytes(form.layout, im.out_w), 4) * (size_t)im.h * planes;
        }
        k.coef_bytes += cb;
        k.count++;
        plan.take.push_back(f);
    }
    if (need_pixels && !have_pixels) return HVC_E_INVALID_ARG;
    for (const MixedDecodeChunk &k : chunks) {
        plan.chunk_first.push_back(k.first);
        plan.chunk_count.push_back(k.count);
        plan.coef_ring = std::max(plan.coef_ring, k.coef_bytes);
        if (host) plan.out_ring = std::max(plan.out_ring, k.pix_hi - k.pix_lo);
        plan.plane_ring = std::max(plan.plane_ring, k.plane_bytes);
        plan.rgb_ring = std::max(plan.rgb_ring, k.rgb_bytes);
        plan.mid_ring = std::max(plan.mid_ring, k.mid_bytes);
        plan.largest = std::max(plan.largest, k.count);
    }
    if (host)
        for (int f : plan.take) {
            plan.pix_rel[(size_t)f] = plan.out_bytes[(size_t)f] ? pixel_offsets[f] - chunks[(size_t)plan.chunk_of[(size_t)f]].pix_lo : 0;
            if (form.resized()) plan.rimg[(size_t)f].dst_offset = plan.pix_rel[(size_t)f];
        }
    return HVC_OK;
}

void mixed_decode_download_runs(const MixedDecodeChunks &plan, int k, const int *status, const char *back, const MixedForm &form,
                                bool scaled, bool host_reader_only, std::vector<MixedDecodeRun> &runs) {
    runs.clear();
    const MixedDecodeChunk &ch = plan.chunks[(size_t)k];
    const size_t reach = !scaled && !host_reader_only && !form.resized() ? 4096 : 1; // a run takes a file that starts less than this behind it
    MixedDecodeRun run;
    auto flush = [&]() {
        if (run.bytes) runs.push_back(run);
        run = MixedDecodeRun();
    };
    int prev_t = -2;
    for (int t = ch.first; t < ch.first + ch.count; t++) {
        const int f = plan.take[(size_t)t];
        if (status[f] != HVC_OK || !plan.out_bytes[(size_t)f] || (back && back[f])) continue;
        const size_t lo = plan.pix_rel[(size_t)f], hi = lo + plan.out_bytes[(size_t)f];
        if (form.rgb() && form.rgb_row_strides && form.rgb_row_strides[f] > plan.row_bytes[(size_t)f]) {
            flush(); // rows with room between them: the image row by row, the caller's bytes between rows stay
            MixedDecodeRun rows;
            rows.lo = lo, rows.row_stride = form.rgb_row_strides[f], rows.row_bytes = plan.row_bytes[(size_t)f], rows.rows = plan.rows[(size_t)f];
            runs.push_back(rows);
            continue;
        }
        const size_t run_hi = run.lo + run.bytes;
        const bool joins = run.bytes && t == prev_t + 1 && lo >= run_hi && lo - run_hi < reach;
        if (!joins) flush();
        if (!run.bytes) run.lo = lo;
        run.bytes = hi - run.lo;
        prev_t = t;
    }
    flush();
}

} // namespace hvc
