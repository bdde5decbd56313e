// Stand-alone driver of hvc::mixed_islow_pairs_build (csrc/hvc_mixed_plan.cpp) for tests/test_mixed_islow_plan.py, built by
// Makefile.mixed_islow with -fsanitize=address,undefined (CPU only, no device code): the table records of the libjpeg-exact
// mixed block stage (k_islow_mixed), made from the plan hvc::mixed_plan_build gives.
//   mixed_islow_plan_harness random SEED COUNT    COUNT seeded sets of frames whose tables have entries from 1 to 65535, with
//                                                 duplicates within and across frames: one record of 32 words per table of the
//                                                 plan, in plan.tables order, word i = q[2i] | q[2i+1] << 16 of the table the
//                                                 plane's FRAME holds; prints "ok COUNT tables T shared S"
//   mixed_islow_plan_harness distinct SEED N      one set with N distinct tables (N may exceed 512): N records, each its table's
//   mixed_islow_plan_harness empty                an empty plan and a set without a block: no record
//   mixed_islow_plan_harness dump Q0 .. Q63       the record of one table, 32 words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hvc_mixed_plan.h"

namespace {

unsigned long long rng_state;
unsigned rnd(unsigned n) { // splitmix64
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) % n);
}

struct Set {
    std::vector<hvc_jpeg_info> infos;
    std::vector<size_t> coef, pix;
};

// a frame of n_comp one-row planes over its n_qtabs tables (already filled in)
void lay_out(hvc_jpeg_info &fi, Set &s, size_t &coef, size_t &pix) {
    size_t co = 0, po = 0;
    for (int i = 0; i < fi.n_comp; i++) {
        hvc_component &c = fi.layout[i];
        c.blocks_w = 1 + (int)rnd(3);
        c.blocks_h = (int)rnd(5) == 0 ? 0 : 1 + (int)rnd(2); // (some planes are empty: they name no table)
        c.qtab = (int)rnd((unsigned)fi.n_qtabs);
        c.stride = (size_t)c.blocks_w * 8;
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

// what every set of records must be; tables_out / shared_out: how many records, how many planes found their table there already
std::string check(const Set &s, size_t *tables_out, size_t *shared_out) {
    hvc::MixedPlan plan;
    const int r = hvc::mixed_plan_build(s.infos.data(), s.coef.data(), s.pix.data(), nullptr, (int)s.infos.size(), plan);
    if (r) return "plan status " + std::to_string(r);
    std::vector<unsigned> pairs(7, 0xdeadbeefu); // (stale content must go)
    hvc::mixed_islow_pairs_build(plan, pairs);
    if (pairs.size() != plan.tables.size() * HVC_ISLOW_PAIR_WORDS) return "record count";
    // through the planes: the record a plane's `table` names holds the pairs of the table its frame gives it
    std::vector<char> named(plan.tables.size(), 0);
    size_t pi = 0, shared = 0;
    for (const hvc_jpeg_info &fi : s.infos)
        for (int i = 0; i < fi.n_comp; i++) {
            const hvc_component &c = fi.layout[i];
            if (c.blocks_w == 0 || c.blocks_h == 0) continue;
            if (pi >= plan.planes.size()) return "a plane without a descriptor";
            const int t = plan.planes[pi++].table;
            if (t < 0 || (size_t)t >= plan.tables.size()) return "table index";
            const uint16_t *q = fi.qtabs[c.qtab];
            for (int w = 0; w < HVC_ISLOW_PAIR_WORDS; w++)
                if (pairs[(size_t)t * HVC_ISLOW_PAIR_WORDS + w] != ((unsigned)q[2 * w] | (unsigned)q[2 * w + 1] << 16)) return "pair word";
            shared += named[(size_t)t];
            named[(size_t)t] = 1;
        }
    // one record per DISTINCT table, in plan.tables order: record t is plan.tables[t]'s, no two tables are equal
    for (size_t t = 0; t < plan.tables.size(); t++) {
        if (!named[t]) return "a record no plane names";
        for (int w = 0; w < HVC_ISLOW_PAIR_WORDS; w++)
            if (pairs[t * HVC_ISLOW_PAIR_WORDS + w] != ((unsigned)plan.tables[t].qt[2 * w] | (unsigned)plan.tables[t].qt[2 * w + 1] << 16))
                return "record order";
        for (size_t u = t + 1; u < plan.tables.size(); u++)
            if (!std::memcmp(&pairs[t * HVC_ISLOW_PAIR_WORDS], &pairs[u * HVC_ISLOW_PAIR_WORDS], HVC_ISLOW_PAIR_WORDS * sizeof(unsigned)))
                return "two records of one table";
    }
    if (tables_out) *tables_out = plan.tables.size();
    if (shared_out) *shared_out = shared;
    return "";
}

// entries from 1 to 65535: the ends, small and large ones
uint16_t entry() {
    switch (rnd(6)) {
    case 0: return 1;
    case 1: return 65535;
    case 2: return (uint16_t)(1 + rnd(255));
    case 3: return (uint16_t)(256 + rnd(65280));
    case 4: return (uint16_t)(32768 + rnd(3) - 1);
    default: return (uint16_t)(1 + rnd(65535));
    }
}

int cmd_random(unsigned long long seed, int count) {
    rng_state = seed;
    size_t tables = 0, shared = 0;
    for (int it = 0; it < count; it++) {
        // a pool of contents the frames draw from, so that tables repeat within and across frames
        std::vector<std::vector<uint16_t>> pool(1 + rnd(6), std::vector<uint16_t>(64));
        for (auto &q : pool)
            for (auto &v : q) v = entry();
        if (pool.size() > 1 && rnd(2)) { // two contents that differ in one entry only
            pool[1] = pool[0];
            const unsigned k = rnd(64);
            pool[1][k] = (uint16_t)(pool[1][k] == 65535 ? 1 : pool[1][k] + 1);
        }
        Set s;
        size_t coef = 0, pix = 0;
        const int n = 1 + (int)rnd(10);
        for (int f = 0; f < n; f++) {
            hvc_jpeg_info fi;
            std::memset(&fi, 0, sizeof fi);
            fi.n_comp = 1 + (int)rnd(4);
            fi.n_qtabs = 1 + (int)rnd(4);
            for (int t = 0; t < fi.n_qtabs; t++) std::memcpy(fi.qtabs[t], pool[rnd((unsigned)pool.size())].data(), 64 * sizeof(uint16_t));
            lay_out(fi, s, coef, pix);
        }
        size_t t = 0, sh = 0;
        const std::string bad = check(s, &t, &sh);
        if (!bad.empty()) {
            std::printf("set %d: %s\n", it, bad.c_str());
            return 1;
        }
        tables += t;
        shared += sh;
    }
    std::printf("ok %d tables %zu shared %zu\n", count, tables, shared);
    return 0;
}

int cmd_distinct(unsigned long long seed, int n_tables) {
    rng_state = seed;
    Set s;
    size_t coef = 0, pix = 0;
    for (int t0 = 0; t0 < n_tables; t0 += 4) {
        hvc_jpeg_info fi;
        std::memset(&fi, 0, sizeof fi);
        fi.n_qtabs = n_tables - t0 < 4 ? n_tables - t0 : 4;
        fi.n_comp = fi.n_qtabs;
        for (int t = 0; t < fi.n_qtabs; t++) {
            for (int k = 0; k < 64; k++) fi.qtabs[t][k] = entry();
            fi.qtabs[t][0] = (uint16_t)(1 + (t0 + t) % 65535), fi.qtabs[t][63] = (uint16_t)(1 + (t0 + t) / 65535); // distinct by construction
        }
        lay_out(fi, s, coef, pix);
        hvc_jpeg_info &back = s.infos.back(); // every table named by exactly one plane with a block
        size_t co = 0, po = 0;
        for (int i = 0; i < back.n_comp; i++) {
            hvc_component &c = back.layout[i];
            c.blocks_w = c.blocks_h = 1, c.qtab = i, c.stride = 8, c.coef_offset = co, c.plane_offset = po;
            co += 64, po += 64;
        }
        back.coef_count = co, back.pixel_bytes = po;
        coef = s.coef.back() + co, pix = s.pix.back() + 256;
    }
    size_t t = 0, sh = 0;
    const std::string bad = check(s, &t, &sh);
    if (!bad.empty() || t != (size_t)n_tables || sh != 0) {
        std::printf("distinct: %s (%zu tables, %zu shared)\n", bad.c_str(), t, sh);
        return 1;
    }
    std::printf("ok tables %zu\n", t);
    return 0;
}

int cmd_empty() {
    hvc::MixedPlan plan;
    std::vector<unsigned> pairs(3, 1u);
    hvc::mixed_islow_pairs_build(plan, pairs);
    if (!pairs.empty()) return 1;
    hvc_jpeg_info fi; // a frame without a block: its tables reach no plane
    std::memset(&fi, 0, sizeof fi);
    fi.n_comp = 2, fi.n_qtabs = 1;
    for (int k = 0; k < 64; k++) fi.qtabs[0][k] = 65535;
    fi.layout[0].blocks_w = 4, fi.layout[1].blocks_h = 4;
    const size_t zero = 0;
    pairs.assign(5, 2u);
    if (hvc::mixed_plan_build(&fi, &zero, &zero, nullptr, 1, plan) != HVC_OK || !plan.tables.empty()) return 1;
    hvc::mixed_islow_pairs_build(plan, pairs);
    if (!pairs.empty()) return 1;
    std::printf("ok empty\n");
    return 0;
}

int cmd_dump(char **q) {
    hvc_jpeg_info fi;
    std::memset(&fi, 0, sizeof fi);
    fi.n_comp = fi.n_qtabs = 1;
    for (int k = 0; k < 64; k++) fi.qtabs[0][k] = (uint16_t)std::strtoul(q[k], nullptr, 10);
    fi.layout[0].blocks_w = fi.layout[0].blocks_h = 1, fi.layout[0].stride = 8;
    const size_t zero = 0;
    hvc::MixedPlan plan;
    std::vector<unsigned> pairs;
    if (hvc::mixed_plan_build(&fi, &zero, &zero, nullptr, 1, plan) != HVC_OK) return 1;
    hvc::mixed_islow_pairs_build(plan, pairs);
    std::printf("pairs");
    for (unsigned w : pairs) std::printf(" %u", w);
    std::printf("\n");
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 4 && !std::strcmp(argv[1], "distinct")) return cmd_distinct(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "empty")) return cmd_empty();
    if (argc >= 66 && !std::strcmp(argv[1], "dump")) return cmd_dump(argv + 2);
    std::fprintf(stderr, "usage: mixed_islow_plan_harness random SEED COUNT | distinct SEED N | empty | dump Q0 .. Q63\n");
    return 2;
}
