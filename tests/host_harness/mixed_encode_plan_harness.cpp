// Stand-alone driver of csrc/hvc_mixed_encode_plan.cpp for tests/test_mixed_encode_plan.py, built by Makefile.mixed_encode
// with -fsanitize=address,undefined (CPU only, no device code):
//   mixed_encode_plan_harness dump FILE          FILE = int64 n_frames, int64 n_list (-1: no list), hvc_jpeg_info[n_frames],
//                                                uint64 coef_offsets[n_frames], uint64 pixel_offsets[n_frames], int32
//                                                list[n_list]; prints the plan hvc::mixed_encode_plan_build makes of it, whether
//                                                its planes and map are hvc::mixed_plan_build's for the same set, and whether
//                                                its reciprocals are hvc::encode_quant_reciprocal's
//   mixed_encode_plan_harness layout ALIGN W H CHROMA QUALITY ...   hvc::encoder_mixed_layout (what
//                                                hvc_jpeg_encoder_mixed_layout forwards to) next to hvc_jpeg_encoder_layout +
//                                                hvc_jpeg_encoder_check frame by frame
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hvc_mixed_encode_plan.h"

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

int cmd_dump(const char *path) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 16) return 2;
    long long n = 0, nl = 0;
    std::memcpy(&n, raw.data(), 8);
    std::memcpy(&nl, raw.data() + 8, 8);
    size_t at = 16;
    if (n < 0 || raw.size() != at + (size_t)n * (sizeof(hvc_jpeg_info) + 16) + (nl > 0 ? (size_t)nl * 4 : 0)) return 2;
    std::vector<hvc_jpeg_info> infos((size_t)n);
    std::vector<size_t> coef((size_t)n), pix((size_t)n);
    std::vector<int> list;
    std::memcpy(infos.data(), raw.data() + at, (size_t)n * sizeof(hvc_jpeg_info));
    at += (size_t)n * sizeof(hvc_jpeg_info);
    for (long long i = 0; i < n; i++) {
        unsigned long long v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)i, 8);
        coef[(size_t)i] = (size_t)v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)(n + i), 8);
        pix[(size_t)i] = (size_t)v;
    }
    at += 16 * (size_t)n;
    if (nl >= 0) {
        list.resize((size_t)nl);
        if (nl) std::memcpy(list.data(), raw.data() + at, (size_t)nl * 4);
        for (int f : list)
            if (f < 0 || f >= n) return 2;
    }
    const int *lp = nl >= 0 ? list.data() : nullptr;
    const int n_list = nl >= 0 ? (int)nl : (int)n;
    hvc::MixedEncodePlan plan;
    const int r = hvc::mixed_encode_plan_build(infos.data(), coef.data(), pix.data(), lp, n_list, plan);
    std::printf("status %d\n", r);
    if (r) {
        std::printf("left %zu %zu %zu %llu\n", plan.planes.size(), plan.tables.size(), plan.map.size(), plan.blocks);
        return 0;
    }
    // units and map: the decode plan's for the same geometry, descriptor for descriptor
    hvc::MixedPlan d;
    const int rd = hvc::mixed_plan_build(infos.data(), coef.data(), pix.data(), lp, n_list, d);
    bool same = rd == HVC_OK && d.planes.size() == plan.planes.size() && d.map == plan.map && d.blocks == plan.blocks &&
                d.tables.size() == plan.tables.size();
    for (size_t i = 0; same && i < d.planes.size(); i++) same = !std::memcmp(&d.planes[i], &plan.planes[i], sizeof d.planes[i]);
    std::printf("decode_plan %s\n", same ? "same" : "differs");
    bool recip = same;
    for (size_t k = 0; recip && k < plan.tables.size(); k++)
        for (int i = 0; i < 64; i++) {
            const float want = hvc::encode_quant_reciprocal((unsigned)d.tables[k].qt[i]);
            if (std::memcmp(&want, &plan.tables[k].qrcp[i], sizeof want)) recip = false;
        }
    std::printf("reciprocals %s\n", recip ? "shared" : "differ");
    std::printf("blocks %llu\n", plan.blocks);
    for (size_t i = 0; i < plan.planes.size(); i++) {
        const hvc::MixedPlaneK &p = plan.planes[i];
        std::printf("plane %zu %llu %llu %llu %d %d %u %d %u\n", i, p.coef_base, p.pix_base, p.stride, p.bw, p.nblk, p.magic, p.table, p.unit0);
    }
    for (size_t k = 0; k < plan.tables.size(); k++) { // the float bit patterns
        std::printf("table %zu", k);
        for (int i = 0; i < 64; i++) {
            unsigned bits;
            std::memcpy(&bits, &plan.tables[k].qrcp[i], 4);
            std::printf(" %u", bits);
        }
        std::printf("\n");
    }
    std::printf("map");
    for (unsigned u : plan.map) std::printf(" %u", u);
    std::printf("\n");
    return 0;
}

int cmd_layout(size_t align, int argc, char **argv) {
    if (argc % 4) return 2;
    const int n = argc / 4;
    std::vector<int> w((size_t)n), h((size_t)n), c((size_t)n), q((size_t)n), status((size_t)n, 77);
    for (int f = 0; f < n; f++) {
        w[(size_t)f] = std::atoi(argv[4 * f]);
        h[(size_t)f] = std::atoi(argv[4 * f + 1]);
        c[(size_t)f] = std::atoi(argv[4 * f + 2]);
        q[(size_t)f] = std::atoi(argv[4 * f + 3]);
    }
    std::vector<hvc_jpeg_info> infos((size_t)n);
    std::vector<size_t> poff((size_t)n), coff((size_t)n);
    size_t ptot = 0, ctot = 0;
    const int r = hvc::encoder_mixed_layout(w.data(), h.data(), c.data(), q.data(), n, align, infos.data(), status.data(), poff.data(),
                                            coff.data(), &ptot, &ctot);
    std::printf("status %d totals %zu %zu\n", r, ptot, ctot);
    if (r) return 0;
    for (int f = 0; f < n; f++) {
        hvc_jpeg_info one;
        int want = hvc_jpeg_encoder_layout(w[(size_t)f], h[(size_t)f], c[(size_t)f], q[(size_t)f], &one);
        if (!want) want = hvc_jpeg_encoder_check(&one);
        const bool info_same = status[(size_t)f] || !std::memcmp(&one, &infos[(size_t)f], sizeof one);
        std::printf("frame %d %d %d %d %zu %zu %zu %zu\n", f, status[(size_t)f], want, info_same ? 1 : 0, poff[(size_t)f], coff[(size_t)f],
                    status[(size_t)f] ? (size_t)0 : infos[(size_t)f].pixel_bytes, status[(size_t)f] ? (size_t)0 : infos[(size_t)f].coef_count);
    }
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "dump")) return cmd_dump(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "layout")) return cmd_layout((size_t)std::strtoull(argv[2], nullptr, 10), argc - 3, argv + 3);
    std::fprintf(stderr, "usage: mixed_encode_plan_harness dump FILE | layout ALIGN W H CHROMA QUALITY ...\n");
    return 2;
}
