// Stand-alone driver of csrc/hvc_hdec_mixed_plan.cpp for tests/test_hdec_mixed_plan.py, built by Makefile.hdec_mixed with
// -fsanitize=address,undefined (CPU only, no device code):
//   hdec_mixed_plan_harness files LIST F...   the files' headers (hvc_jpeg_read_header) and segments (prepare_gpu_decode_to, into
//                                             one buffer at places known from the files' sizes) -> hvc::hdm_plan_build over
//                                             LIST ("all", "none", or positions "3,0,2"); prints the plan and checks it
//   hdec_mixed_plan_harness random SEED COUNT COUNT seeded random sets of synthetic geometries, each checked here
//   hdec_mixed_plan_harness limits            the 32-bit limits (HDM_TOO_LARGE) from both sides, per file and per chunk
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hvc_hdec_mixed_plan.h"

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

// the properties every plan must have; returns an empty string or what is wrong
std::string check_plan(const std::vector<hvc::HdmFileIn> &in, const std::vector<int> &list, const hvc::HdmPlan &plan) {
    if (plan.refusal.size() != list.size() || plan.files.size() != plan.file_of.size()) return "sizes";
    size_t at = 0;
    unsigned long long subs = 0, units = 0, dcd = 0;
    for (size_t l = 0; l < list.size(); l++) {
        if (plan.refusal[l] != hvc::HDM_TAKEN) continue;
        if (at >= plan.files.size() || plan.file_of[at] != list[l]) return "order";
        const hvc::HdmFileK &k = plan.files[at];
        const hvc::HdmFileIn &f = in[(size_t)list[l]];
        if (k.sub0 != subs || k.unit0 != units || k.dcd0 != dcd) return "prefix sums";
        if (k.n_sub != hvc::hdm_file_subs(f.seg_bytes) || (size_t)k.n_sub * (HVC_HD_SUBSEQ_BITS / 8) < f.seg_bytes + 1) return "subsequences";
        if (k.ecs_off != f.ecs_off || k.coef_base != f.coef_base) return "places";
        if (k.need == 0 || k.blocks_per_mcu == 0 || k.blocks_per_mcu > HVC_HD_MAX_MCU_BLOCKS || k.need % k.blocks_per_mcu) return "need";
        const unsigned long long nu = ((unsigned long long)k.n_sub + HVC_HDM_UNIT - 1) / HVC_HDM_UNIT;
        for (unsigned long long u = units; u < units + nu; u++)
            if (u >= plan.map.size() || plan.map[(size_t)u] != at) return "map entry";
        // every block of an MCU: inside its component's plane at every MCU of the grid, component and position consistent
        if (k.mbs_wide == 0) return "grid";
        const unsigned mcus = k.need / k.blocks_per_mcu, mbs_high = mcus / k.mbs_wide;
        if (mcus % k.mbs_wide) return "grid";
        for (unsigned b = 0; b < k.blocks_per_mcu; b++) {
            const unsigned c = k.b2comp[b];
            if (c >= k.n_comp || ((k.selmask >> (2 * b)) & 3u) != c) return "component of a block";
            if (k.b2sx[b] >= k.h[c] || k.b2sy[b] >= k.v[c] || b != k.mcu_base[c] + k.b2sy[b] * k.h[c] + k.b2sx[b]) return "position of a block";
            const hvc_component &L = f.info->layout[c];
            const unsigned long long bx = (unsigned long long)(k.mbs_wide - 1) * k.h[c] + k.b2sx[b], by = (unsigned long long)(mbs_high - 1) * k.v[c] + k.b2sy[b];
            if (bx >= (unsigned long long)L.blocks_w || by >= (unsigned long long)L.blocks_h) return "a block outside its plane";
            if (k.coef_off[c] + (by * k.bw[c] + bx + 1) * 64 > f.info->coef_count) return "a block outside the record";
        }
        if (k.tabrec >= plan.tab_src.size() || plan.tab_src[k.tabrec] < 0 || (f.tabrec >= 0 && k.tabrec != (unsigned)f.tabrec) || std::memcmp(in[(size_t)plan.tab_src[k.tabrec]].tables, f.tables, sizeof(hvc::HdTables))) return "table record";
        subs += k.n_sub;
        units += nu;
        dcd += k.need;
        if (f.ecs_off + hvc::hdm_file_room(f.seg_bytes) > plan.seg_bytes) return "segment buffer";
        at++;
    }
    if (at != plan.files.size() || subs != plan.total_sub || units != plan.map.size() || dcd != plan.dcd_entries) return "totals";
    for (size_t a = 0; a < plan.tab_src.size(); a++) // (a caller's own record indices may leave some unused: -1)
        for (size_t b = a + 1; b < plan.tab_src.size(); b++)
            if (plan.tab_src[a] >= 0 && plan.tab_src[b] >= 0 && !std::memcmp(in[(size_t)plan.tab_src[a]].tables, in[(size_t)plan.tab_src[b]].tables, sizeof(hvc::HdTables))) return "equal tables not shared";
    return "";
}

void print_plan(const hvc::HdmPlan &plan) {
    std::printf("totals %u %zu %zu %zu %zu\n", plan.total_sub, plan.seg_bytes, plan.dcd_entries, plan.tab_src.size(), plan.map.size());
    std::printf("refusal");
    for (int r : plan.refusal) std::printf(" %d", r);
    std::printf("\ntabsrc");
    for (int t : plan.tab_src) std::printf(" %d", t);
    std::printf("\n");
    for (size_t i = 0; i < plan.files.size(); i++) {
        const hvc::HdmFileK &k = plan.files[i];
        std::printf("file %d %u %u %u %u %llu %u %u %u %u %u %u %u", plan.file_of[i], k.ecs_off, k.sub0, k.n_sub, k.unit0, k.coef_base, k.need,
                    k.blocks_per_mcu, k.mbs_wide, k.n_comp, k.selmask, k.tabrec, k.dcd0);
        for (int c = 0; c < 4; c++) std::printf(" %u %u %u %u %u", k.h[c], k.v[c], k.bw[c], k.mcu_base[c], k.coef_off[c]);
        for (int b = 0; b < HVC_HD_MAX_MCU_BLOCKS; b++) std::printf(" %u %u %u", k.b2comp[b], k.b2sx[b], k.b2sy[b]);
        std::printf("\n");
    }
    std::printf("map");
    for (unsigned u : plan.map) std::printf(" %u", u);
    std::printf("\n");
}

int cmd_files(const char *list_arg, int n, char **paths) {
    std::vector<std::vector<unsigned char>> files((size_t)n);
    std::vector<hvc_jpeg_info> infos((size_t)n);
    std::vector<std::unique_ptr<hvc::HdTables>> tabs((size_t)n);
    std::vector<hvc::HdmFileIn> in((size_t)n);
    const size_t SB = HVC_HD_SUBSEQ_BITS / 8;
    size_t room = 0, coef = 0;
    for (int i = 0; i < n; i++) {
        if (!read_all(paths[i], files[(size_t)i])) return 2;
        room += hvc::hdm_file_room(files[(size_t)i].size());
    }
    std::vector<uint8_t> ecs(room + HVC_HD_ECS_SLACK, 0xA5);
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        const std::vector<unsigned char> &f = files[(size_t)i];
        const int hr = hvc_jpeg_read_header(f.data(), f.size(), &infos[(size_t)i]);
        if (hr) {
            std::printf("header %d %d\n", i, hr);
            return 0;
        }
        tabs[(size_t)i].reset(new hvc::HdTables);
        std::memset(tabs[(size_t)i].get(), 0, sizeof(hvc::HdTables));
        bool ok = false;
        size_t got = 0;
        const int r = hvc::prepare_gpu_decode_to(f.data(), f.size(), &infos[(size_t)i], *tabs[(size_t)i], ecs.data() + at, (f.size() + SB - 1) / SB * SB, &got, ok);
        if (!r && ok) std::memset(ecs.data() + at + got, 0, hvc::hdm_file_room(got) - got);
        std::printf("segment %d %d %d %zu\n", i, r, ok ? 1 : 0, got);
        in[(size_t)i] = hvc::HdmFileIn{&infos[(size_t)i], at, (!r && ok) ? got : 0, tabs[(size_t)i].get(), !r && ok, coef};
        at += hvc::hdm_file_room(f.size());
        coef += (infos[(size_t)i].coef_count + 63) / 64 * 64;
    }
    std::vector<int> list;
    if (!std::strcmp(list_arg, "all")) {
        for (int i = 0; i < n; i++) list.push_back(i);
    } else if (std::strcmp(list_arg, "none")) {
        for (const char *p = list_arg; *p;) {
            char *end;
            list.push_back((int)std::strtol(p, &end, 10));
            p = *end ? end + 1 : end;
        }
    }
    hvc::HdmPlan plan;
    // ("all": the null list, which means the same)
    const int r = hvc::hdm_plan_build(in.data(), n, !std::strcmp(list_arg, "all") ? nullptr : list.data(), (int)list.size(), plan);
    std::printf("status %d\n", r);
    if (r) return 0;
    const std::string bad = check_plan(in, list, plan);
    std::printf("check %s\n", bad.empty() ? "ok" : bad.c_str());
    print_plan(plan);
    return 0;
}

// a grey frame of mw x mh MCUs (one block each), its record tight
hvc_jpeg_info grey_info(int mw, int mh) {
    hvc_jpeg_info fi;
    std::memset(&fi, 0, sizeof fi);
    fi.n_comp = 1;
    fi.comp[0].hscale = fi.comp[0].vscale = 1;
    fi.comp[0].decoded_width = mw * 8;
    fi.comp[0].decoded_height = mh * 8;
    fi.layout[0].blocks_w = mw;
    fi.layout[0].blocks_h = mh;
    fi.coef_count = (size_t)mw * (size_t)mh * 64;
    return fi;
}

// "Sizes beyond the 32-bit indices": every limit of hdm_geometry and hdm_plan_build from both sides -- the largest value that
// is taken, the smallest that is HDM_TOO_LARGE -- per file and per chunk (a file pushed over a limit by the files before
// it), each with small files around it, which must stay in a plan that keeps its invariants.  Synthetic inputs: no buffer
// is touched.  Prints one line per case: its refusals and the check's verdict.
int cmd_limits() {
    std::unique_ptr<hvc::HdTables> tab(new hvc::HdTables);
    std::memset(tab.get(), 7, sizeof(hvc::HdTables));
    int bad = 0;
    auto run = [&](const char *name, std::vector<hvc_jpeg_info> &infos, std::vector<hvc::HdmFileIn> &in) {
        for (size_t f = 0; f < in.size(); f++) {
            in[f].info = &infos[f];
            in[f].tables = tab.get();
            in[f].tables_ok = true;
        }
        std::vector<int> list;
        for (size_t f = 0; f < in.size(); f++) list.push_back((int)f);
        hvc::HdmPlan plan;
        const int r = hvc::hdm_plan_build(in.data(), (int)in.size(), nullptr, (int)in.size(), plan);
        const std::string chk = r ? std::string("status") : check_plan(in, list, plan);
        std::printf("case %s", name);
        if (in.size() <= 8)
            for (int w : plan.refusal) std::printf(" %d", w);
        else // (many files: the first refusal's place, how many are refused, the last file's answer)
            for (size_t l = 0; l < plan.refusal.size(); l++)
                if (plan.refusal[l]) {
                    size_t n = 0;
                    for (int w : plan.refusal) n += w != 0;
                    std::printf(" first %zu why %d refused %zu last %d", l, plan.refusal[l], n, plan.refusal.back());
                    break;
                }
        std::printf(" check %s\n", chk.empty() ? "ok" : chk.c_str());
        if (r || !chk.empty()) bad++;
    };
    const hvc::HdmFileIn none{nullptr, 0, 0, nullptr, true, 0};
    auto small_around = [&](const hvc_jpeg_info &mid, const hvc::HdmFileIn &mid_in, std::vector<hvc_jpeg_info> &infos, std::vector<hvc::HdmFileIn> &in) {
        infos = {grey_info(3, 2), mid, grey_info(5, 1)};
        in = {none, mid_in, none};
        in[0].seg_bytes = 300;
        in[0].ecs_off = 0;
        in[2].seg_bytes = 77;
        in[2].ecs_off = 1024;
        in[2].coef_base = 512;
    };
    std::vector<hvc_jpeg_info> infos;
    std::vector<hvc::HdmFileIn> in;
    hvc::HdmFileIn mid = none;
    mid.ecs_off = 2048;
    mid.seg_bytes = 500;
    mid.coef_base = 1024;
    // per file, hdm_geometry: coef_count, a component's coef_offset, the blocks of the frame
    for (int over = 0; over < 2; over++) {
        hvc_jpeg_info fi = grey_info(4, 4);
        fi.coef_count = over ? (size_t)1 << 32 : ((size_t)1 << 32) - 64;
        small_around(fi, mid, infos, in);
        run(over ? "coef_count_2^32" : "coef_count_below", infos, in);
        fi = grey_info(4, 4);
        fi.n_comp = 2;
        fi.comp[1].hscale = fi.comp[1].vscale = 1;
        fi.layout[1] = fi.layout[0];
        fi.layout[1].coef_offset = over ? (size_t)1 << 32 : ((size_t)1 << 32) - 2048; // (below: the plane's 1024 elements end inside the record)
        fi.coef_count = ((size_t)1 << 32) - 1024; // (below its own limit, which is asked above)
        small_around(fi, mid, infos, in);
        run(over ? "coef_offset_2^32" : "coef_offset_below", infos, in);
        // 46340^2 = 2147395600 < 2^31 <= 46341 * 46341; 32768 * 65536 = 2^31 exactly
        fi = over ? grey_info(32768, 65536) : grey_info(46340, 46340);
        fi.coef_count = 4096; // (a record that size cannot be described: the block count's own limit is what is asked here)
        small_around(fi, mid, infos, in);
        if (!over) { // (taken: the harness's own check wants the record to hold the frame, which 32 bits cannot say -- the refusal alone is looked at)
            hvc::HdmFileK k;
            std::printf("case blocks_below %d check ok\n", hvc::hdm_geometry(fi, k));
        } else {
            run("blocks_2^31", infos, in);
        }
    }
    // per file, hdm_plan_build: the segment's bytes (bit positions inside a file are 32 bits), the end of its room
    for (int over = 0; over < 2; over++) {
        hvc::HdmFileIn m = mid;
        m.seg_bytes = over ? (size_t)1 << 28 : ((size_t)1 << 28) - 1;
        small_around(grey_info(4, 4), m, infos, in);
        run(over ? "seg_bytes_2^28" : "seg_bytes_below", infos, in);
        m = mid;
        m.seg_bytes = 100; // room: 3 subsequences = 384 bytes
        m.ecs_off = over ? ((size_t)1 << 32) - 384 : ((size_t)1 << 32) - 512;
        small_around(grey_info(4, 4), m, infos, in);
        run(over ? "room_end_2^32" : "room_end_below", infos, in);
    }
    // per chunk: subsequences (2^31), entries of the DC rows (2^32) -- the file that crosses the limit is refused, the ones
    // behind it that still fit are taken
    {
        const size_t seg = ((size_t)1 << 28) - 1, per = hvc::hdm_file_subs(seg); // 2^21 + 1 subsequences each
        const size_t n = (((size_t)1 << 31) - 1) / per + 2;
        infos.assign(n, grey_info(2, 2));
        in.assign(n, none);
        for (size_t f = 0; f + 1 < n; f++) in[f].seg_bytes = seg; // (segments may overlap for the plan's sake: no byte is read)
        in[n - 1].seg_bytes = 10;
        run("chunk_subsequences", infos, in);
    }
    {
        const hvc_jpeg_info big = grey_info(8191, 8192); // 67100672 blocks, coef_count 4294443008 < 2^32
        infos.assign(66, big);
        infos[65] = grey_info(1, 1);
        in.assign(66, none);
        for (size_t f = 0; f < in.size(); f++) in[f].seg_bytes = 1000;
        run("chunk_dc_rows", infos, in);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad != 0;
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
    std::vector<std::unique_ptr<hvc::HdTables>> kinds;
    for (int t = 0; t < 3; t++) { // a few table contents, so that sets repeat across files
        kinds.emplace_back(new hvc::HdTables);
        std::memset(kinds.back().get(), t + 1, sizeof(hvc::HdTables));
    }
    int taken = 0, refused = 0;
    for (int it = 0; it < count; it++) {
        const int n = (int)rnd(14);
        const bool given = rnd(2) != 0; // the caller names every file's table record itself (HdmFileIn::tabrec)
        std::vector<hvc_jpeg_info> infos((size_t)n);
        std::vector<hvc::HdmFileIn> in((size_t)n);
        std::vector<int> want((size_t)n, hvc::HDM_TAKEN);
        size_t at = 0, coef = 0;
        for (int f = 0; f < n; f++) {
            hvc_jpeg_info &fi = infos[(size_t)f];
            std::memset(&fi, 0, sizeof fi);
            fi.n_comp = 1 + (int)rnd(3);
            const int mw = 1 + (int)rnd(40), mh = 1 + (int)rnd(30);
            int blocks = 0;
            size_t co = 0;
            for (int i = 0; i < fi.n_comp; i++) {
                const int h = 1 + (int)rnd(4), v = 1 + (int)rnd(3);
                fi.comp[i].hscale = h;
                fi.comp[i].vscale = v;
                fi.layout[i].blocks_w = mw * h + (int)rnd(2);
                fi.layout[i].blocks_h = mh * v + (int)rnd(2);
                fi.layout[i].coef_offset = co;
                co += (size_t)fi.layout[i].blocks_w * fi.layout[i].blocks_h * 64;
                blocks += h * v;
            }
            fi.comp[0].decoded_width = mw * 8 * fi.comp[0].hscale;
            fi.comp[0].decoded_height = mh * 8 * fi.comp[0].vscale;
            fi.coef_count = co;
            int why = blocks > HVC_HD_MAX_MCU_BLOCKS ? hvc::HDM_MCU_BLOCKS : hvc::HDM_TAKEN;
            const unsigned twist = rnd(12);
            if (twist == 0) { // four components
                fi.n_comp = 4;
                why = hvc::HDM_NO_COMPONENTS;
            } else if (twist == 1 && why == hvc::HDM_TAKEN) { // the grid leaves the last component's plane
                fi.layout[fi.n_comp - 1].blocks_h = mh * fi.comp[fi.n_comp - 1].vscale - 1;
                why = hvc::HDM_MCU_GRID;
            } else if (twist == 2 && why == hvc::HDM_TAKEN) {
                fi.comp[0].decoded_width = 0; // no MCU at all
                why = hvc::HDM_NO_BLOCKS;
            }
            const bool tables_ok = rnd(10) != 0;
            if (why == hvc::HDM_TAKEN && !tables_ok) why = hvc::HDM_TABLES;
            const size_t seg = rnd(5) == 0 ? rnd(3) * 128 : rnd(40000);
            const unsigned kind = rnd(3);
            in[(size_t)f] = hvc::HdmFileIn{&fi, at, seg, kinds[kind].get(), tables_ok, coef, given ? (int)kind : -1};
            if (why == hvc::HDM_TAKEN && rnd(15) == 0) { // a record off its 16 bytes
                in[(size_t)f].coef_base += 4;
                why = hvc::HDM_PLACE;
            }
            want[(size_t)f] = why;
            at += hvc::hdm_file_room(seg);
            coef += co;
        }
        std::vector<int> list;
        for (int f = 0; f < n; f++)
            if (rnd(5)) list.push_back(f);
        if (list.size() > 1 && rnd(2)) std::swap(list.front(), list.back()); // (any order)
        hvc::HdmPlan plan;
        const int r = hvc::hdm_plan_build(in.data(), n, list.data(), (int)list.size(), plan);
        if (r) {
            std::printf("set %d: status %d\n", it, r);
            return 1;
        }
        for (size_t l = 0; l < list.size(); l++) {
            if (plan.refusal[l] != want[(size_t)list[l]]) {
                std::printf("set %d: file %d refusal %d, expected %d\n", it, list[l], plan.refusal[l], want[(size_t)list[l]]);
                return 1;
            }
            (plan.refusal[l] ? refused : taken)++;
        }
        const std::string bad = check_plan(in, list, plan);
        if (!bad.empty()) {
            std::printf("set %d: %s\n", it, bad.c_str());
            return 1;
        }
    }
    std::printf("ok %d taken %d refused %d\n", count, taken, refused);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "files")) return cmd_files(argv[2], argc - 3, argv + 3);
    if (argc >= 2 && !std::strcmp(argv[1], "limits")) return cmd_limits();
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    std::fprintf(stderr, "usage: hdec_mixed_plan_harness files all|none|I,J,... FILE... | random SEED COUNT | limits\n");
    return 2;
}
