// Stand-alone driver of csrc/hvc_mixed_encode_chunks.cpp for tests/test_mixed_encode_chunks.py, built by
// Makefile.mixed_encode_chunks with -fsanitize=address,undefined (CPU only, no device code):
//   mixed_encode_chunks_harness plan FILE    FILE = int64 n_frames, chunk_bytes, max_files_per_chunk, rgb, layout, has_strides;
//                                            hvc_jpeg_info[n_frames]; int32 status[n_frames]; uint8 has_frame[n_frames];
//                                            uint8 has_jpeg[n_frames]; uint64 rgb_row_strides[n_frames] (if has_strides).
//                                            Prints what hvc::mixed_encode_chunks_build answers and the plan it leaves.
//   mixed_encode_chunks_harness pad W H CHROMA   hvc_jpeg_encoder_layout's actual plane sizes next to the uniform pipeline's
//                                            (width, height, chroma) rule, and pad_frame of the frame src[i] = i % 251 + 1
//                                            into a record filled with 0xA5 with 64 guard bytes behind it, in hex
//   mixed_encode_chunks_harness rule MAXW MAXH   the same comparison over every size up to MAXW x MAXH under 4:2:0, 4:2:2 and
//                                            4:4:4: "rule <laid out> <passing hvc_jpeg_encoder_check> <differing>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hvc_mixed_encode_chunks.h"

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

int cmd_plan(const char *path) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 48) return 2;
    long long head[6];
    std::memcpy(head, raw.data(), sizeof head);
    const long long n = head[0];
    const bool strides = head[5] != 0;
    if (n < 0 || raw.size() != 48 + (size_t)n * (sizeof(hvc_jpeg_info) + 4 + 2 + (strides ? 8 : 0))) return 2;
    size_t at = 48;
    std::vector<hvc_jpeg_info> infos((size_t)n);
    std::vector<int> status((size_t)n);
    std::vector<size_t> rs((size_t)n, 0);
    if (n) std::memcpy(infos.data(), raw.data() + at, (size_t)n * sizeof(hvc_jpeg_info));
    at += (size_t)n * sizeof(hvc_jpeg_info);
    if (n) std::memcpy(status.data(), raw.data() + at, (size_t)n * 4);
    at += (size_t)n * 4;
    const unsigned char *has_frame = raw.data() + at, *has_jpeg = raw.data() + at + n;
    at += 2 * (size_t)n;
    for (long long i = 0; strides && i < n; i++) {
        unsigned long long v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)i, 8);
        rs[(size_t)i] = (size_t)v;
    }
    // the build function only asks whether a pointer is null: one byte stands for every frame and every file
    static const uint8_t frame_byte = 0;
    static uint8_t jpeg_byte = 0;
    std::vector<const uint8_t *> frames((size_t)n);
    std::vector<uint8_t *> jpegs((size_t)n);
    for (long long i = 0; i < n; i++) {
        frames[(size_t)i] = has_frame[i] ? &frame_byte : nullptr;
        jpegs[(size_t)i] = has_jpeg[i] ? &jpeg_byte : nullptr;
    }
    MixedEncodeInput in;
    in.rgb = head[3] != 0;
    in.layout = (int)head[4];
    in.rgb_row_strides = strides ? rs.data() : nullptr;
    hvc::MixedEncodeChunks plan;
    const int r = hvc::mixed_encode_chunks_build(infos.data(), status.data(), frames.data(), jpegs.data(), (int)n, (size_t)head[1], in,
                                                 (int)head[2], plan);
    std::printf("status %d\n", r);
    print_list("statuses", status);
    if (r) return 0;
    print_list("take", plan.take);
    print_list("chunk_of", plan.chunk_of);
    for (size_t k = 0; k < plan.chunks.size(); k++) {
        const hvc::MixedEncodeChunk &c = plan.chunks[k];
        std::printf("chunk %zu %d %d %zu %zu %zu\n", k, c.first, c.count, c.pix_bytes, c.coef_elems, c.rgb_bytes);
    }
    print_list("pix_rel", plan.pix_rel);
    print_list("coef_rel", plan.coef_rel);
    print_list("rgb_rel", plan.rgb_rel);
    std::printf("wants %zu %zu %zu %d %llu\n", plan.in_bytes, plan.out_bytes, plan.rgb_bytes, plan.largest, (unsigned long long)plan.coef_total);
    return 0;
}

int cmd_pad(int width, int height, int chroma) {
    hvc_jpeg_info info;
    const int r = hvc_jpeg_encoder_layout(width, height, chroma, 75, &info);
    std::printf("layout %d check %d\n", r, r ? 0 : hvc_jpeg_encoder_check(&info));
    if (r) return 0;
    // what hvc_jpeg_encode_batch derives from width, height and chroma for its padding workers
    const int cw = chroma == 444 ? width : width / 2, ch = chroma == 420 ? height / 2 : height;
    const int sw[3] = {width, cw, cw}, sh[3] = {height, ch, ch};
    size_t total = 0;
    for (int i = 0; i < 3; i++) {
        std::printf("plane %d actual %d %d rule %d %d decoded %d %d offset %zu stride %zu\n", i, info.comp[i].actual_width,
                    info.comp[i].actual_height, sw[i], sh[i], info.comp[i].decoded_width, info.comp[i].decoded_height,
                    (size_t)info.layout[i].plane_offset, (size_t)info.layout[i].stride);
        total += (size_t)info.comp[i].actual_width * info.comp[i].actual_height;
    }
    std::vector<uint8_t> src(total), rec(info.pixel_bytes + 64, 0xA5); // (exactly sized: a byte read or written beyond is a report)
    for (size_t i = 0; i < total; i++) src[i] = (uint8_t)(i % 251 + 1);
    pad_frame(info, src.data(), rec.data());
    std::printf("pixel_bytes %zu\nrecord ", (size_t)info.pixel_bytes);
    for (uint8_t b : rec) std::printf("%02x", b);
    std::printf("\n");
    return 0;
}

// every size up to max_w x max_h under the three samplings: where hvc_jpeg_encoder_layout answers, are its actual plane sizes
// the rule's?
int cmd_rule(int max_w, int max_h) {
    int laid_out = 0, checked = 0, differ = 0;
    for (int chroma : {420, 422, 444})
        for (int width = 1; width <= max_w; width++)
            for (int height = 1; height <= max_h; height++) {
                hvc_jpeg_info info;
                if (hvc_jpeg_encoder_layout(width, height, chroma, 75, &info)) continue;
                laid_out++;
                if (!hvc_jpeg_encoder_check(&info)) checked++;
                const int cw = chroma == 444 ? width : width / 2, ch = chroma == 420 ? height / 2 : height;
                const int sw[3] = {width, cw, cw}, sh[3] = {height, ch, ch};
                bool same = info.n_comp == 3;
                for (int i = 0; i < 3; i++) same = same && info.comp[i].actual_width == sw[i] && info.comp[i].actual_height == sh[i];
                if (!same) {
                    differ++;
                    std::printf("differs %d %d %d\n", width, height, chroma);
                }
            }
    std::printf("rule %d %d %d\n", laid_out, checked, differ);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !std::strcmp(argv[1], "rule")) return cmd_rule(std::atoi(argv[2]), std::atoi(argv[3]));
    if (argc == 3 && !std::strcmp(argv[1], "plan")) return cmd_plan(argv[2]);
    if (argc == 5 && !std::strcmp(argv[1], "pad")) return cmd_pad(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
    std::fprintf(stderr, "usage: mixed_encode_chunks_harness plan FILE | pad W H CHROMA | rule MAXW MAXH\n");
    return 2;
}
