// Stand-alone driver of csrc/hvc_mixed_decode_chunks.cpp for tests/test_mixed_decode_chunks.py, built by
// Makefile.mixed_decode_chunks with -fsanitize=address,undefined (CPU only, no device code):
//   mixed_decode_chunks_harness FILE    FILE = int64 n_files, chunk_bytes, where, pixel_cap, have_pixels, rgb, layout, has_strides,
//                                       scale_denom, resized, filter, has_heights, host_reader_only, has_back;
//                                       hvc_jpeg_info[n_files]; int32 status[n_files]; uint8 has_jpeg[n_files];
//                                       uint64 pixel_offsets[n_files]; uint64 rgb_row_strides[n_files] (if has_strides);
//                                       int32 out_widths[n_files], out_heights[n_files] (if resized);
//                                       int32 later[n_files] (every file's status once its chunk was decoded);
//                                       uint8 back[n_files] (if has_back).
//                                       Prints what hvc::mixed_decode_chunks_build answers, the plan it leaves and, per chunk,
//                                       the copies of hvc::mixed_decode_download_runs under the later statuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hvc_mixed_decode_chunks.h"

namespace {

bool read_all(const char *path, std::vector<unsigned char> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

template <class T>
void print_list(const char *name, const std::vector<T> &v) {
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

// n values of type T at raw[at ...], exactly sized: a read beyond is a report
template <class T>
std::vector<T> take(const std::vector<unsigned char> &raw, size_t &at, size_t n) {
    std::vector<T> v(n);
    if (n) std::memcpy(v.data(), raw.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
}

} // namespace

int main(int argc, char **argv) {
    std::vector<unsigned char> raw;
    long long head[14];
    if (argc != 2 || !read_all(argv[1], raw) || raw.size() < sizeof head) {
        std::fprintf(stderr, "usage: mixed_decode_chunks_harness FILE\n");
        return 2;
    }
    std::memcpy(head, raw.data(), sizeof head);
    const long long n = head[0];
    const bool rgb = head[5] != 0, strides = head[7] != 0, resized = head[9] != 0, heights = head[11] != 0, has_back = head[13] != 0;
    if (n < 0 || raw.size() != sizeof head + (size_t)n * (sizeof(hvc_jpeg_info) + 4 + 1 + 8 + (strides ? 8 : 0) + (resized ? 8 : 0) + 4 + (has_back ? 1 : 0)))
        return 2;
    size_t at = sizeof head;
    std::vector<hvc_jpeg_info> infos = take<hvc_jpeg_info>(raw, at, (size_t)n);
    std::vector<int> status = take<int>(raw, at, (size_t)n);
    const std::vector<unsigned char> has_jpeg = take<unsigned char>(raw, at, (size_t)n);
    const std::vector<unsigned long long> offsets64 = take<unsigned long long>(raw, at, (size_t)n);
    const std::vector<unsigned long long> strides64 = take<unsigned long long>(raw, at, strides ? (size_t)n : 0);
    const std::vector<int> out_w = take<int>(raw, at, resized ? (size_t)n : 0), out_h = take<int>(raw, at, resized ? (size_t)n : 0);
    const std::vector<int> later = take<int>(raw, at, (size_t)n);
    const std::vector<char> back = take<char>(raw, at, has_back ? (size_t)n : 0);
    const std::vector<size_t> offsets(offsets64.begin(), offsets64.end()), rs(strides64.begin(), strides64.end());
    // the build function only asks whether a pointer is null: one byte stands for every file
    static const uint8_t file_byte = 0;
    std::vector<const uint8_t *> jpegs((size_t)n);
    for (long long i = 0; i < n; i++) jpegs[(size_t)i] = has_jpeg[(size_t)i] ? &file_byte : nullptr;
    MixedForm form;
    if (rgb) form.rgb_offsets = offsets.data(); // (as the entry points: the images' offsets are the call's pixel offsets)
    form.rgb_row_strides = strides ? rs.data() : nullptr;
    form.layout = (int)head[6];
    form.scale_denom = (int)head[8];
    form.out_widths = resized ? out_w.data() : nullptr;
    form.out_heights = resized && heights ? out_h.data() : nullptr;
    form.filter = (int)head[10];
    hvc::MixedDecodeChunks plan;
    const int r = hvc::mixed_decode_chunks_build(infos.data(), status.data(), jpegs.data(), offsets.data(), (size_t)head[3], head[4] != 0, (int)n,
                                                 (size_t)head[1], (int)head[2], form, plan);
    std::printf("status %d\n", r);
    print_list("statuses", status);
    if (r) return 0;
    print_list("take", plan.take);
    print_list("chunk_of", plan.chunk_of);
    print_list("chunk_first", plan.chunk_first);
    print_list("chunk_count", plan.chunk_count);
    for (size_t k = 0; k < plan.chunks.size(); k++) {
        const hvc::MixedDecodeChunk &c = plan.chunks[k];
        std::printf("chunk %zu %d %d %zu %zu %zu %zu %zu %zu\n", k, c.first, c.count, c.coef_bytes, c.pix_lo, c.pix_hi, c.plane_bytes, c.rgb_bytes,
                    c.mid_bytes);
    }
    print_list("coef_rel", plan.coef_rel);
    print_list("pix_rel", plan.pix_rel);
    print_list("out_bytes", plan.out_bytes);
    print_list("plane_rel", plan.plane_rel);
    print_list("row_bytes", plan.row_bytes);
    print_list("rows", plan.rows);
    print_list("rgb_rel", plan.rgb_rel);
    for (size_t f = 0; f < plan.rimg.size(); f++) {
        const hvc::ResizeImage &im = plan.rimg[f];
        std::printf("rimg %zu %d %d %d %d %zu %zu %zu %zu\n", f, im.w, im.h, im.out_w, im.out_h, im.src_offset, im.src_row_stride, im.dst_offset,
                    im.dst_row_stride);
    }
    for (size_t f = 0; f < plan.scaled.size(); f++) // (what the pipeline reads of a file's output info)
        std::printf("scaled %zu %d %d %zu\n", f, plan.scaled[f].width, plan.scaled[f].height, (size_t)plan.scaled[f].pixel_bytes);
    std::printf("wants %zu %zu %zu %zu %zu %d\n", plan.coef_ring, plan.out_ring, plan.plane_ring, plan.rgb_ring, plan.mid_ring, plan.largest);
    if ((int)head[2] != HVC_MEM_HOST) return 0;
    std::vector<hvc::MixedDecodeRun> runs;
    for (size_t k = 0; k < plan.chunks.size(); k++) {
        hvc::mixed_decode_download_runs(plan, (int)k, later.data(), has_back ? back.data() : nullptr, form, form.scale_denom != 1, head[12] != 0, runs);
        for (const hvc::MixedDecodeRun &run : runs)
            std::printf("run %zu %zu %zu %zu %zu %zu\n", k, run.lo, run.bytes, run.row_stride, run.row_bytes, run.rows);
    }
    return 0;
}
