// Stand-alone driver of csrc/hvc_huff_mixed_plan.cpp for tests/test_huff_mixed_plan.py, built by Makefile.huff_mixed with
// -fsanitize=address,undefined (CPU only, no device code):
//   huff_mixed_plan_harness dump FILE OPTIMISED     FILE = int64 n_frames, int64 n_list (-1: no list), hvc_jpeg_info[n_frames],
//                                                   uint64 coef_offsets[n_frames], int32 list[n_list]; prints the plan
//                                                   hvc::huff_mixed_plan_build makes of it
//   huff_mixed_plan_harness handback CAPACITY N OFFSET{N + 1} STATUS{N}    hvc::huff_mixed_hand_back
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hvc_huff_mixed_plan.h"

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

int cmd_dump(const char *path, bool optimised) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 16) return 2;
    long long n = 0, nl = 0;
    std::memcpy(&n, raw.data(), 8);
    std::memcpy(&nl, raw.data() + 8, 8);
    size_t at = 16;
    if (n < 0 || raw.size() != at + (size_t)n * (sizeof(hvc_jpeg_info) + 8) + (nl > 0 ? (size_t)nl * 4 : 0)) return 2;
    std::vector<hvc_jpeg_info> infos((size_t)n);
    std::vector<size_t> coef((size_t)n);
    std::vector<int> list;
    if (n) std::memcpy(infos.data(), raw.data() + at, (size_t)n * sizeof(hvc_jpeg_info));
    at += (size_t)n * sizeof(hvc_jpeg_info);
    for (long long i = 0; i < n; i++) {
        unsigned long long v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)i, 8);
        coef[(size_t)i] = (size_t)v;
    }
    at += 8 * (size_t)n;
    if (nl >= 0) {
        list.resize((size_t)nl);
        if (nl) std::memcpy(list.data(), raw.data() + at, (size_t)nl * 4);
        for (int f : list)
            if (f >= n) return 2; // (a negative entry is the builder's to refuse)
    }
    static const int no_frames[1] = {0};
    const int *lp = nl >= 0 ? (nl ? list.data() : no_frames) : nullptr;
    const int n_list = nl >= 0 ? (int)nl : (int)n;
    hvc::HuffMixedPlan plan;
    const int r = hvc::huff_mixed_plan_build(infos.data(), coef.data(), lp, n_list, optimised, plan);
    std::printf("status %d\n", r);
    std::printf("sizes %zu %zu %zu %zu %zu\n", plan.files.size(), plan.file_of.size(), plan.status.size(), plan.planes.size(), plan.map.size());
    std::printf("totals %llu %llu %llu %llu\n", plan.lens_total, plan.bitbuf_words, plan.pieces_cap, plan.coef_elems);
    if (r) return 0;
    std::printf("codes");
    for (int s : plan.status) std::printf(" %d", s);
    std::printf("\nfile_of");
    for (int f : plan.file_of) std::printf(" %d", f);
    std::printf("\n");
    for (size_t i = 0; i < plan.files.size(); i++) {
        const hvc::HuffMixedFileK &k = plan.files[i];
        std::printf("file %zu %d %d %d %u %llu %llu %u\n", i, k.mbs_wide, k.mbs_high, k.blocks_per_mcu, k.blocks, k.lens_base, k.bitbuf_base,
                    k.bitbuf_words);
    }
    for (size_t i = 0; i < plan.planes.size(); i++) {
        const hvc::HuffMixedPlaneK &p = plan.planes[i];
        std::printf("plane %zu %llu %d %d %d %d %d %d %u %u\n", i, p.coef_base, p.bw, p.nblk, p.h, p.v, p.mcu_base, p.table, p.unit0, p.file);
    }
    std::printf("map");
    for (unsigned u : plan.map) std::printf(" %u", u);
    std::printf("\n");
    return 0;
}

int cmd_handback(int argc, char **argv) {
    if (argc < 2) return 2;
    const unsigned long long cap = std::strtoull(argv[0], nullptr, 10);
    const int n = std::atoi(argv[1]);
    if (n < 0 || argc != 2 + (n + 1) + n) return 2;
    std::vector<unsigned long long> off((size_t)n + 1);
    std::vector<unsigned> st((size_t)n + 1, 0); // (+ 1: never an empty array)
    for (int i = 0; i <= n; i++) off[(size_t)i] = std::strtoull(argv[2 + i], nullptr, 10);
    for (int i = 0; i < n; i++) st[(size_t)i] = (unsigned)std::strtoul(argv[3 + n + i], nullptr, 10);
    std::vector<int> complete{-7}, back{-7}; // (what was there before must go)
    hvc::huff_mixed_hand_back(off.data(), st.data(), n, cap, complete, back);
    std::printf("complete");
    for (int k : complete) std::printf(" %d", k);
    std::printf("\nback");
    for (int k : back) std::printf(" %d", k);
    std::printf("\n");
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "dump")) return cmd_dump(argv[2], std::atoi(argv[3]) != 0);
    if (argc >= 3 && !std::strcmp(argv[1], "handback")) return cmd_handback(argc - 2, argv + 2);
    std::fprintf(stderr, "usage: huff_mixed_plan_harness dump FILE OPTIMISED | handback CAPACITY N OFFSETS... STATUS...\n");
    return 2;
}
