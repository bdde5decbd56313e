// Stand-alone driver of csrc/hvc_mixed_plan.cpp for tests/test_mixed_plan.py, built by Makefile.mixed with
// -fsanitize=address,undefined (CPU only, no device code):
//   mixed_plan_harness dump FILE            FILE = int64 n_frames, int64 n_list (-1: no list), hvc_jpeg_info[n_frames],
//                                           uint64 coef_offsets[n_frames], uint64 pixel_offsets[n_frames], int32 list[n_list];
//                                           prints the plan hvc::mixed_plan_build makes of it
//   mixed_plan_harness random SEED COUNT    COUNT seeded random sets, each checked here: every block of every listed plane
//                                           lies in exactly one (unit, lane), equal tables share an entry, unequal ones do not
//   mixed_plan_harness layout ALIGN F...    hvc::mixed_layout (what hvc_jpeg_mixed_layout forwards to) over the files
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "hvc_mixed_plan.h"

namespace {

struct Set {
    std::vector<hvc_jpeg_info> infos;
    std::vector<size_t> coef, pix;
    std::vector<int> list;
    bool has_list = false;
};

bool read_all(const char *path, std::vector<unsigned char> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

// the properties every plan must have; returns an empty string or what is wrong
std::string check_plan(const Set &s, const hvc::MixedPlan &plan) {
    const int n_list = s.has_list ? (int)s.list.size() : (int)s.infos.size();
    size_t pi = 0;
    unsigned long long units = 0, blocks = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = s.has_list ? s.list[(size_t)l] : l;
        const hvc_jpeg_info &fi = s.infos[(size_t)f];
        for (int i = 0; i < fi.n_comp; i++) {
            const hvc_component &c = fi.layout[i];
            if (c.blocks_w == 0 || c.blocks_h == 0) continue;
            if (pi >= plan.planes.size()) return "a plane without a descriptor";
            const hvc::MixedPlaneK &p = plan.planes[pi];
            const unsigned long long nblk = (unsigned long long)c.blocks_w * c.blocks_h;
            if (p.bw != c.blocks_w || (unsigned long long)p.nblk != nblk || p.stride != c.stride) return "geometry";
            if (p.coef_base != s.coef[(size_t)f] + c.coef_offset || p.pix_base != s.pix[(size_t)f] + c.plane_offset) return "bases";
            if (p.unit0 != units) return "unit0";
            if (p.table < 0 || (size_t)p.table >= plan.tables.size()) return "table index";
            const hvc::MixedTableK &t = plan.tables[(size_t)p.table];
            bool wide = false;
            for (int k = 0; k < 64; k++) {
                if (t.qt[k] != (int)fi.qtabs[c.qtab][k]) return "table content";
                wide |= fi.qtabs[c.qtab][k] > 255;
            }
            if ((t.wide != 0) != wide) return "wide flag";
            // every block in exactly one (unit, lane): the kernel's b = (unit - unit0) * 64 + lane, by = umulhi(b, magic)
            std::vector<unsigned char> seen((size_t)nblk, 0);
            const unsigned long long nu = (nblk + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
            for (unsigned long long u = units; u < units + nu; u++) {
                if (u >= plan.map.size() || plan.map[(size_t)u] != pi) return "map entry";
                for (int lane = 0; lane < HVC_MIXED_UNIT; lane++) {
                    const unsigned long long b = (u - p.unit0) * HVC_MIXED_UNIT + (unsigned)lane;
                    if (b >= nblk) continue;
                    const unsigned by = p.bw == 1 ? (unsigned)b : (unsigned)(((unsigned long long)(unsigned)b * p.magic) >> 32);
                    const unsigned bx = (unsigned)b - by * (unsigned)p.bw;
                    if (bx >= (unsigned)c.blocks_w || by >= (unsigned)c.blocks_h) return "block position";
                    if (seen[(size_t)by * c.blocks_w + bx]++) return "a block twice";
                }
            }
            for (unsigned char v : seen)
                if (v != 1) return "a block without a lane";
            units += nu;
            blocks += nblk;
            pi++;
        }
    }
    if (pi != plan.planes.size() || units != plan.map.size() || blocks != plan.blocks) return "totals";
    for (size_t a = 0; a < plan.tables.size(); a++)
        for (size_t b = a + 1; b < plan.tables.size(); b++)
            if (!std::memcmp(plan.tables[a].qt, plan.tables[b].qt, sizeof plan.tables[a].qt)) return "equal tables not shared";
    return "";
}

int build(const Set &s, hvc::MixedPlan &plan) {
    return hvc::mixed_plan_build(s.infos.data(), s.coef.data(), s.pix.data(), s.has_list ? s.list.data() : nullptr,
                                 s.has_list ? (int)s.list.size() : (int)s.infos.size(), plan);
}

int cmd_dump(const char *path) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 16) return 2;
    long long n = 0, nl = 0;
    std::memcpy(&n, raw.data(), 8);
    std::memcpy(&nl, raw.data() + 8, 8);
    Set s;
    size_t at = 16;
    const size_t need = at + (size_t)n * (sizeof(hvc_jpeg_info) + 16) + (nl > 0 ? (size_t)nl * 4 : 0);
    if (n < 0 || raw.size() != need) return 2;
    s.infos.resize((size_t)n);
    s.coef.resize((size_t)n);
    s.pix.resize((size_t)n);
    std::memcpy(s.infos.data(), raw.data() + at, (size_t)n * sizeof(hvc_jpeg_info));
    at += (size_t)n * sizeof(hvc_jpeg_info);
    for (long long i = 0; i < n; i++) {
        unsigned long long v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)i, 8);
        s.coef[(size_t)i] = (size_t)v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)(n + i), 8);
        s.pix[(size_t)i] = (size_t)v;
    }
    at += 16 * (size_t)n;
    if (nl >= 0) {
        s.has_list = true;
        s.list.resize((size_t)nl);
        if (nl) std::memcpy(s.list.data(), raw.data() + at, (size_t)nl * 4);
        for (int f : s.list)
            if (f < 0 || f >= n) return 2;
    }
    hvc::MixedPlan plan;
    const int r = build(s, plan);
    std::printf("status %d\n", r);
    if (r) return 0;
    const std::string bad = check_plan(s, plan);
    std::printf("check %s\n", bad.empty() ? "ok" : bad.c_str());
    std::printf("blocks %llu\n", plan.blocks);
    for (size_t i = 0; i < plan.planes.size(); i++) {
        const hvc::MixedPlaneK &p = plan.planes[i];
        std::printf("plane %zu %llu %llu %llu %d %d %u %d %u\n", i, p.coef_base, p.pix_base, p.stride, p.bw, p.nblk, p.magic, p.table, p.unit0);
    }
    for (size_t i = 0; i < plan.tables.size(); i++) {
        const hvc::MixedTableK &t = plan.tables[i];
        std::printf("table %zu %d %d", i, t.wide, t.ethr_packed);
        for (int k = 0; k < 64; k++) std::printf(" %d", t.qt[k]);
        for (int k = 0; k < 32; k++) std::printf(" %u", t.qpair[k]);
        std::printf("\n");
    }
    std::printf("map");
    for (unsigned u : plan.map) std::printf(" %u", u);
    std::printf("\n");
    return 0;
}

unsigned long long rng_state;
unsigned rnd(unsigned n) { // splitmix64
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) % n);
}

int cmd_random(unsigned long long seed, int count) {
    rng_state = seed;
    static const int SIDES[] = {0, 1, 1, 2, 3, 7, 8, 9, 16, 63, 64, 65, 255, 256, 257};
    int refused = 0;
    for (int it = 0; it < count; it++) {
        Set s;
        const int n = 1 + (int)rnd(12);
        size_t coef = 0, pix = 0;
        for (int f = 0; f < n; f++) {
            hvc_jpeg_info fi;
            std::memset(&fi, 0, sizeof fi);
            fi.n_comp = 1 + (int)rnd(4);
            fi.n_qtabs = 1 + (int)rnd(4);
            for (int t = 0; t < fi.n_qtabs; t++) {
                const unsigned kind = rnd(4); // a few contents, so that tables repeat across frames
                for (int k = 0; k < 64; k++) fi.qtabs[t][k] = (uint16_t)(kind == 3 ? 200 + 2 * k : 1 + kind * 16 + (unsigned)k % (kind + 2));
            }
            size_t co = 0, po = 0;
            for (int i = 0; i < fi.n_comp; i++) {
                hvc_component &c = fi.layout[i];
                c.blocks_w = SIDES[rnd(sizeof SIDES / sizeof SIDES[0])];
                c.blocks_h = SIDES[rnd(sizeof SIDES / sizeof SIDES[0])];
                if (rnd(3) == 0) c.blocks_h = 1;
                c.qtab = (int)rnd((unsigned)fi.n_qtabs);
                c.stride = (size_t)c.blocks_w * 8 + 8 * rnd(3);
                c.coef_offset = co;
                c.plane_offset = po;
                co += (size_t)c.blocks_w * c.blocks_h * 64;
                po += c.stride * (size_t)c.blocks_h * 8;
            }
            fi.coef_count = co;
            fi.pixel_bytes = po;
            s.infos.push_back(fi);
            s.coef.push_back(coef);
            s.pix.push_back(pix);
            coef += co;
            pix += (po + 255) & ~(size_t)255;
        }
        if (rnd(2)) { // a list with holes
            s.has_list = true;
            for (int f = 0; f < n; f++)
                if (rnd(4)) s.list.push_back(f);
        }
        const bool misalign = rnd(10) == 0 && !s.pix.empty();
        if (misalign) s.pix[rnd((unsigned)n)] += 4;
        hvc::MixedPlan plan;
        const int r = build(s, plan);
        if (r) {
            if (!(misalign && r == HVC_E_ALIGNMENT)) {
                std::printf("set %d: status %d\n", it, r);
                return 1;
            }
            refused++;
            continue;
        }
        const std::string bad = check_plan(s, plan);
        if (!bad.empty()) {
            std::printf("set %d: %s\n", it, bad.c_str());
            return 1;
        }
    }
    std::printf("ok %d refused %d\n", count, refused);
    return 0;
}

int cmd_layout(size_t align, int n, char **paths) {
    std::vector<std::vector<unsigned char>> files((size_t)n);
    std::vector<const uint8_t *> ptrs((size_t)n);
    std::vector<size_t> sizes((size_t)n), offs((size_t)n);
    std::vector<hvc_jpeg_info> infos((size_t)n);
    std::vector<int> status((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!read_all(paths[i], files[(size_t)i])) return 2;
        ptrs[(size_t)i] = files[(size_t)i].data();
        sizes[(size_t)i] = files[(size_t)i].size();
    }
    size_t total = 0;
    const int r = hvc::mixed_layout(ptrs.data(), sizes.data(), n, align, infos.data(), status.data(), offs.data(), &total);
    std::printf("status %d total %zu\n", r, total);
    if (r) return 0;
    for (int i = 0; i < n; i++) std::printf("file %d %d %zu %zu\n", i, status[(size_t)i], offs[(size_t)i], status[(size_t)i] ? (size_t)0 : infos[(size_t)i].pixel_bytes);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "dump")) return cmd_dump(argv[2]);
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 3 && !std::strcmp(argv[1], "layout")) return cmd_layout((size_t)std::strtoull(argv[2], nullptr, 10), argc - 3, argv + 3);
    std::fprintf(stderr, "usage: mixed_plan_harness dump FILE | random SEED COUNT | layout ALIGN FILE...\n");
    return 2;
}
