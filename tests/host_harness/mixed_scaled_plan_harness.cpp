// Stand-alone driver of the SCALED host plans (csrc/hvc_mixed_plan.cpp with n = 4, 2, 1; csrc/hvc_mixed_rgb_plan.cpp over
// scaled planes) for tests/test_mixed_scaled_plan.py, built by Makefile.mixed_scaled with -fsanitize=address,undefined (CPU
// only, no device code):
//   mixed_scaled_plan_harness shapes               for N in 4, 2, 1 and three placements (tight, on 4 bytes, shifted by one
//                                                  byte): planes of 1, 63, 64, 65, 256, 257 blocks, bw in 1, 5, 6, 9, an empty
//                                                  plane; every property below is checked here
//   mixed_scaled_plan_harness random SEED COUNT    COUNT seeded random sets, each at a random N, placement and base address
//   mixed_scaled_plan_harness window               the colour plan over scaled planes refuses a window beyond N * blocks_w / _h
//   mixed_scaled_plan_harness layout S ALIGN F...  hvc::mixed_scaled_layout over the files
// The properties: every block's N x N square lies inside its frame's record; the squares of a plane are disjoint and cover
// blocks_w * N x blocks_h * N; the planes of a record do not overlap; `dwords` is set exactly when base address and stride
// are multiples of 4; units, map and tables (and every descriptor field but pix_base / stride / dwords) equal those of the
// full-size plan of the same frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hvc_mixed_plan.h"
#include "hvc_mixed_rgb_plan.h"

namespace {

struct Set {
    std::vector<hvc_jpeg_info> infos; // layout[].plane_offset / .stride: the SCALED planes
    std::vector<size_t> coef, pix, rec; // rec[f]: bytes of frame f's pixel record
    std::vector<int> list;
    bool has_list = false;
};

unsigned long long rng_state;
unsigned rnd(unsigned n) { // splitmix64
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) % n);
}

// the same frames with full-size tight planes (what mixed_plan_build takes for n = 8)
Set full_size(const Set &s) {
    Set o = s;
    size_t pix = 0;
    for (size_t f = 0; f < o.infos.size(); f++) {
        size_t po = 0;
        for (int i = 0; i < o.infos[f].n_comp; i++) {
            hvc_component &c = o.infos[f].layout[i];
            c.stride = (size_t)c.blocks_w * 8;
            c.plane_offset = po;
            po += (size_t)c.blocks_w * c.blocks_h * 64;
        }
        o.pix[f] = pix;
        pix += po;
    }
    return o;
}

int build(const Set &s, hvc::MixedPlan &plan, int n, uintptr_t addr) {
    return hvc::mixed_plan_build(s.infos.data(), s.coef.data(), s.pix.data(), s.has_list ? s.list.data() : nullptr,
                                 s.has_list ? (int)s.list.size() : (int)s.infos.size(), plan, n, addr);
}

std::string check_scaled(const Set &s, int n, uintptr_t addr) {
    hvc::MixedPlan plan, full;
    int r = build(s, plan, n, addr);
    if (r) return "status " + std::to_string(r);
    if ((r = build(full_size(s), full, 8, 0))) return "full-size status " + std::to_string(r);
    if (plan.map != full.map) return "map differs from the full-size plan";
    if (plan.blocks != full.blocks || plan.planes.size() != full.planes.size() || plan.tables.size() != full.tables.size()) return "totals";
    if (!plan.tables.empty() && std::memcmp(plan.tables.data(), full.tables.data(), plan.tables.size() * sizeof(hvc::MixedTableK)))
        return "tables differ from the full-size plan";
    const int n_list = s.has_list ? (int)s.list.size() : (int)s.infos.size();
    size_t pi = 0;
    for (int l = 0; l < n_list; l++) {
        const size_t f = (size_t)(s.has_list ? s.list[(size_t)l] : l);
        const hvc_jpeg_info &fi = s.infos[f];
        std::vector<unsigned char> bytes(s.rec[f], 0); // the record: who wrote which byte
        for (int i = 0; i < fi.n_comp; i++) {
            const hvc_component &c = fi.layout[i];
            if (c.blocks_w == 0 || c.blocks_h == 0) continue;
            if (pi >= plan.planes.size()) return "a plane without a descriptor";
            const hvc::MixedPlaneK &p = plan.planes[pi], &q = full.planes[pi];
            if (p.bw != q.bw || p.nblk != q.nblk || p.magic != q.magic || p.table != q.table || p.unit0 != q.unit0 || p.coef_base != q.coef_base)
                return "descriptor differs from the full-size plan";
            if (q.dwords) return "the full-size plan sets the dword flag";
            if (p.pix_base != s.pix[f] + c.plane_offset || p.stride != c.stride) return "bases";
            if ((p.dwords != 0) != ((((unsigned long long)addr + p.pix_base) % 4 == 0) && p.stride % 4 == 0)) return "dword flag";
            const size_t W = (size_t)c.blocks_w * n, H = (size_t)c.blocks_h * n;
            std::vector<unsigned char> cover(W * H, 0);
            const unsigned long long nu = ((unsigned long long)p.nblk + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
            for (unsigned long long u = p.unit0; u < p.unit0 + nu; u++)
                for (int lane = 0; lane < HVC_MIXED_UNIT; lane++) { // the kernel's arithmetic
                    const unsigned long long b = (u - p.unit0) * HVC_MIXED_UNIT + (unsigned)lane;
                    if (b >= (unsigned long long)p.nblk) continue;
                    const unsigned by = p.bw == 1 ? (unsigned)b : (unsigned)(((unsigned long long)(unsigned)b * p.magic) >> 32);
                    const unsigned bx = (unsigned)b - by * (unsigned)p.bw;
                    for (int row = 0; row < n; row++)
                        for (int col = 0; col < n; col++) {
                            const unsigned long long at = p.pix_base + ((unsigned long long)by * n + row) * p.stride + (unsigned long long)bx * n + col;
                            if (at < s.pix[f] || at - s.pix[f] >= s.rec[f]) return "a sample outside its record";
                            if (bytes[(size_t)(at - s.pix[f])]++) return "a byte of the record written twice";
                            const unsigned long long off = at - p.pix_base, y = off / p.stride, x = off % p.stride;
                            if (x >= W || y >= H) return "a sample outside its plane";
                            cover[(size_t)(y * W + x)]++;
                        }
                }
            for (unsigned char v : cover)
                if (v != 1) return "the squares do not cover the plane";
            pi++;
        }
    }
    if (pi != plan.planes.size()) return "descriptor count";
    return "";
}

// placement: 0 tight (hvc_jpeg_scaled_info's), 1 strides and plane offsets on 4 bytes, 2 as 1 with everything shifted by a byte
void place(Set &s, int n, int placement) {
    size_t coef = 0, pix = placement == 2 ? 1 : 0;
    s.coef.clear(), s.pix.clear(), s.rec.clear();
    for (hvc_jpeg_info &fi : s.infos) {
        size_t co = 0, po = 0;
        for (int i = 0; i < fi.n_comp; i++) {
            hvc_component &c = fi.layout[i];
            const size_t row = (size_t)c.blocks_w * n;
            c.stride = placement ? (row + 3) & ~(size_t)3 : row;
            if (c.blocks_w == 0) c.stride = 0;
            c.coef_offset = co;
            c.plane_offset = po;
            co += (size_t)c.blocks_w * c.blocks_h * 64;
            po += c.stride * (size_t)c.blocks_h * n;
            if (placement) po = (po + 3) & ~(size_t)3;
        }
        fi.coef_count = co;
        fi.pixel_bytes = po;
        s.coef.push_back(coef);
        s.pix.push_back(pix);
        s.rec.push_back(po);
        coef += co;
        pix += placement ? (po + 7) & ~(size_t)7 : po;
    }
}

hvc_jpeg_info frame(std::initializer_list<std::pair<int, int>> planes, int table_kind) {
    hvc_jpeg_info fi;
    std::memset(&fi, 0, sizeof fi);
    fi.n_qtabs = 2;
    for (int k = 0; k < 64; k++) fi.qtabs[0][k] = (uint16_t)(1 + table_kind * 16 + k % 5), fi.qtabs[1][k] = (uint16_t)(table_kind == 2 ? 300 : 9 + k);
    for (auto &p : planes) {
        hvc_component &c = fi.layout[fi.n_comp];
        c.blocks_w = p.first, c.blocks_h = p.second, c.qtab = fi.n_comp ? 1 : 0;
        fi.n_comp++;
    }
    return fi;
}

int cmd_shapes() {
    Set s;
    s.infos = {frame({{1, 1}}, 0),                      // 1 block
               frame({{9, 7}, {8, 8}, {5, 13}}, 1),     // 63, 64, 65; bw 9 and 5
               frame({{16, 16}, {0, 4}, {1, 257}}, 0),  // 256, an empty plane, bw 1 with 257
               frame({{6, 11}, {4, 0}}, 2),             // bw 6; a plane without rows
               frame({{5, 1}, {6, 1}, {9, 1}, {1, 1}}, 1)};
    int checked = 0;
    for (int n : {4, 2, 1})
        for (int placement = 0; placement < 3; placement++)
            for (uintptr_t addr : {(uintptr_t)0x1000, (uintptr_t)0x1002}) {
                place(s, n, placement);
                const std::string bad = check_scaled(s, n, addr);
                if (!bad.empty()) {
                    std::printf("N %d placement %d addr %zu: %s\n", n, placement, (size_t)addr, bad.c_str());
                    return 1;
                }
                // the flag by the placements' own construction: all planes on 4 bytes, or none
                hvc::MixedPlan plan;
                build(s, plan, n, addr);
                for (const hvc::MixedPlaneK &p : plan.planes) {
                    if (placement == 1 && addr == 0x1000 && !p.dwords) return std::printf("N %d: an aligned plane without the flag\n", n), 1;
                    if (placement == 2 && addr == 0x1000 && p.dwords) return std::printf("N %d: a shifted plane with the flag\n", n), 1;
                }
                checked++;
            }
    // the rules: a stride below the row, a coefficient plane off 16 bytes, n outside 8 4 2 1
    place(s, 2, 0);
    hvc::MixedPlan plan;
    Set t = s;
    t.infos[1].layout[0].stride = 17; // 9 blocks of 2 bytes
    if (build(t, plan, 2, 0) != HVC_E_INVALID_ARG) return std::printf("a stride below the row was accepted\n"), 1;
    t = s;
    t.coef[1] += 4;
    if (build(t, plan, 2, 0) != HVC_E_ALIGNMENT) return std::printf("a coefficient plane off 16 bytes was accepted\n"), 1;
    if (build(s, plan, 3, 0) != HVC_E_INVALID_ARG || build(s, plan, 0, 0) != HVC_E_INVALID_ARG) return std::printf("a bad n was accepted\n"), 1;
    if (build(s, plan, 8, 0) != HVC_E_INVALID_ARG && build(s, plan, 8, 0) != HVC_E_ALIGNMENT) return std::printf("full size took scaled strides\n"), 1;
    std::printf("ok %d\n", checked);
    return 0;
}

int cmd_random(unsigned long long seed, int count) {
    rng_state = seed;
    static const int SIDES[] = {0, 1, 1, 2, 3, 5, 6, 7, 8, 9, 16, 63, 64, 65, 255, 256, 257};
    static const int NS[] = {4, 2, 1};
    for (int it = 0; it < count; it++) {
        Set s;
        const int frames = 1 + (int)rnd(8);
        for (int f = 0; f < frames; f++) {
            hvc_jpeg_info fi = frame({}, (int)rnd(3));
            fi.n_comp = 1 + (int)rnd(4);
            for (int i = 0; i < fi.n_comp; i++) {
                hvc_component &c = fi.layout[i];
                c.blocks_w = SIDES[rnd(sizeof SIDES / sizeof SIDES[0])];
                c.blocks_h = rnd(3) ? SIDES[rnd(12)] : 1;
                c.qtab = (int)rnd(2);
            }
            s.infos.push_back(fi);
        }
        const int n = NS[rnd(3)];
        place(s, n, (int)rnd(3));
        if (rnd(2)) {
            s.has_list = true;
            for (int f = 0; f < frames; f++)
                if (rnd(4)) s.list.push_back(f);
        }
        const std::string bad = check_scaled(s, n, (uintptr_t)(0x2000 + rnd(8)));
        if (!bad.empty()) {
            std::printf("set %d (N %d): %s\n", it, n, bad.c_str());
            return 1;
        }
    }
    std::printf("ok %d\n", count);
    return 0;
}

// one 4:2:0 frame of 4 x 3 luma blocks as the scaled block stage leaves it, an image of w x h inside
int rgb_status(int n, int w, int h) {
    hvc_jpeg_info fi;
    std::memset(&fi, 0, sizeof fi);
    fi.n_comp = 3;
    fi.width = w, fi.height = h;
    for (int i = 0; i < 3; i++) {
        fi.comp[i].hscale = fi.comp[i].vscale = i ? 1 : 2;
        hvc_component &c = fi.layout[i];
        c.blocks_w = i ? 2 : 4, c.blocks_h = i ? 2 : 3;
        c.stride = 64; // (rows longer than any window tried here: what refuses is the window check, not the stride check)
        c.plane_offset = (size_t)i * 64 * 24;
    }
    const size_t zero = 0;
    hvc::MixedRgbPlan plan;
    return hvc::mixed_rgb_plan_build(&fi, &zero, &zero, nullptr, HVC_RGB_INTERLEAVED, nullptr, 1, 0, 0, true, plan, n);
}

int cmd_window() {
    for (int n : {8, 4, 2, 1}) {
        if (rgb_status(n, 4 * n, 3 * n) != HVC_OK) return std::printf("N %d: the whole plane refused\n", n), 1;
        if (rgb_status(n, 4 * n + 1, 3 * n) != HVC_E_INVALID_ARG) return std::printf("N %d: a window wider than N * blocks_w accepted\n", n), 1;
        if (rgb_status(n, 4 * n, 3 * n + 1) != HVC_E_INVALID_ARG) return std::printf("N %d: a window taller than N * blocks_h accepted\n", n), 1;
        // what passes at full size must not pass over scaled planes: a hand-made info with the full-size window
        if (n != 8 && rgb_status(n, 32, 24) != HVC_E_INVALID_ARG) return std::printf("N %d: the full-size window accepted\n", n), 1;
    }
    if (rgb_status(3, 4, 3) != HVC_E_INVALID_ARG) return std::printf("a bad n accepted\n"), 1;
    std::printf("ok\n");
    return 0;
}

bool read_all(const char *path, std::vector<unsigned char> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int cmd_layout(int scale, size_t align, int n, char **paths) {
    std::vector<std::vector<unsigned char>> files((size_t)n);
    std::vector<const uint8_t *> ptrs((size_t)n);
    std::vector<size_t> sizes((size_t)n), offs((size_t)n);
    std::vector<hvc_jpeg_info> infos((size_t)n), scaled((size_t)n);
    std::vector<int> status((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!read_all(paths[i], files[(size_t)i])) return 2;
        ptrs[(size_t)i] = files[(size_t)i].data();
        sizes[(size_t)i] = files[(size_t)i].size();
    }
    size_t total = 0;
    const int r = hvc::mixed_scaled_layout(ptrs.data(), sizes.data(), n, scale, align, infos.data(), scaled.data(), status.data(), offs.data(), &total);
    std::printf("status %d total %zu\n", r, total);
    if (r) return 0;
    for (int i = 0; i < n; i++)
        std::printf("file %d %d %zu %zu\n", i, status[(size_t)i], offs[(size_t)i], status[(size_t)i] ? (size_t)0 : scaled[(size_t)i].pixel_bytes);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "shapes")) return cmd_shapes();
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "window")) return cmd_window();
    if (argc >= 4 && !std::strcmp(argv[1], "layout"))
        return cmd_layout(std::atoi(argv[2]), (size_t)std::strtoull(argv[3], nullptr, 10), argc - 4, argv + 4);
    std::fprintf(stderr, "usage: mixed_scaled_plan_harness shapes | random SEED COUNT | window | layout S ALIGN FILE...\n");
    return 2;
}
