// Stand-alone driver of csrc/hvc_hdec_plan.h for tests/test_hdec_plan.py, built by Makefile.hdec_plan with
// -fsanitize=address,undefined (CPU only, no device code):
//   hdec_plan_harness sweep     chunk layouts and index fills over C x cnt x ipf x max_file x segment lengths x table patterns:
//                               every array is allocated at the size the layout states and written the way the pipeline's
//                               workers, its orchestrating thread and the reader's launches write it, so that a wrong offset is
//                               a sanitizer report; every value is compared with a restatement of the arithmetic the batch
//                               pipeline carried before the plan existed
//   hdec_plan_harness limits    the 2^31 refusals from both sides (size_t arithmetic, nothing allocated)
//   hdec_plan_harness restart   the restart-interval decision at its edges and at both callers' ceilings
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "hvc_hdec_plan.h"

namespace {

constexpr size_t SB = 128;
static_assert(hvc::HD_SB == SB, "the sweep's sizes are stated for subsequences of 128 bytes");

int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (failures++ < 20) {                         \
                std::printf("FAILED %s: ", #cond);         \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

// subsequences by counting them: one per started stretch of SB bytes
size_t count_stretches(size_t bytes) {
    size_t n = 0;
    for (size_t b = 0; b < bytes; b += SB) n++;
    return n;
}
size_t file_subs_restated(size_t bytes) { return count_stretches(bytes) + 1; }             // ... and one of zeros
size_t unit_subs_restated(size_t bytes) { return bytes ? count_stretches(bytes) : 1; }     // an interval: none, but at least one

// the layout as the batch pipeline wrote it out where it was used
struct Restated {
    size_t CU, nsub_max, R, ecs_bytes, meta_words, sub_off, tabset_of, frame_of, frame_blocks, changed, status, upload_words, state_subs, cap;
};
Restated restate(size_t C, size_t ipf, size_t max_file) {
    Restated r;
    r.CU = C * ipf;
    r.nsub_max = ipf > 1 ? (max_file + SB - 1) / SB + 2 * ipf : (max_file + SB - 1) / SB + 1;
    r.R = ipf > 1 ? (max_file + SB - 1) / SB * SB + ipf * (2 * SB + 16) : r.nsub_max * SB + 16;
    r.ecs_bytes = C * r.R;
    r.meta_words = r.CU + (r.CU + 1) + r.CU + C * r.nsub_max + r.CU + 2;
    r.sub_off = r.CU;
    r.tabset_of = r.CU + r.CU + 1;
    r.frame_of = r.CU + r.CU + 1 + r.CU;
    r.frame_blocks = r.meta_words - 2 - r.CU;
    r.changed = r.meta_words - 2;
    r.status = r.meta_words - 1;
    r.upload_words = 3 * r.CU + 1;
    r.state_subs = C * r.nsub_max;
    r.cap = ipf > 1 ? r.R : (r.nsub_max - 1) * SB;
    return r;
}

unsigned long long cases = 0, fills = 0;

// one chunk: cnt files, file f's reader frames of lens[f * ipf + q] bytes, tables of their own where pf[f]
void one_fill(const hvc::HdChunkLayout &L, int cnt, const std::vector<unsigned> &lens, const std::vector<char> &pf) {
    const size_t ipf = L.ipf, nu = (size_t)cnt * ipf;
    // the pinned segment slot, written the way a worker writes it
    std::unique_ptr<unsigned char[]> ecs(new unsigned char[L.ecs_bytes]);
    std::memset(ecs.get(), 0xa5, L.ecs_bytes);
    std::vector<unsigned> ecs_size((size_t)cnt), unit_off(ipf > 1 ? nu : 0), unit_len(ipf > 1 ? nu : 0);
    for (int f = 0; f < cnt; f++) {
        unsigned char *dst = ecs.get() + L.file_at((size_t)f);
        CHECK(L.file_at((size_t)f) == (size_t)f * L.R, "file %d", f);
        if (ipf > 1) {
            size_t at = 0, total = 0;
            for (size_t q = 0; q < ipf; q++) { // (extract_ecs_units_to: slot after slot)
                const size_t len = lens[(size_t)f * ipf + q], slot = hvc::hd_unit_slot(len);
                CHECK(slot <= L.file_cap() - at, "interval %zu of file %d leaves the room the worker is given", q, f);
                std::memset(dst + at, 0x11, len);
                std::memset(dst + at + len, 0, slot - len);
                unit_off[(size_t)f * ipf + q] = (unsigned)at;
                unit_len[(size_t)f * ipf + q] = (unsigned)len;
                at += slot;
                total += len;
            }
            ecs_size[(size_t)f] = (unsigned)total;
        } else {
            const size_t got = lens[(size_t)f];
            CHECK(got <= L.file_cap(), "file %d", f);
            std::memset(dst, 0x11, got);
            std::memset(dst + got, 0, hvc::hd_file_subs(got) * SB + 16 - got); // its zero subsequence and the overshoot
            ecs_size[(size_t)f] = (unsigned)got;
        }
    }
    // the pinned words that travel: exactly upload_words of them
    std::vector<unsigned> hm(L.upload_words, 0xdeadbeefu);
    const hvc::HdChunkFill fill = hvc::hd_chunk_fill(L, hm.data(), cnt, ecs_size.data(), ipf > 1 ? unit_off.data() : nullptr,
                                                     ipf > 1 ? unit_len.data() : nullptr, pf.data());
    fills++;
    // ... against the loop the pipeline carried
    std::vector<unsigned> want(L.upload_words, 0xdeadbeefu);
    unsigned subs = 0;
    bool own = false;
    for (int f = 0; f < cnt; f++) {
        own |= pf[(size_t)f] != 0;
        for (size_t q = 0; q < ipf; q++) {
            const size_t u = (size_t)f * ipf + q;
            const unsigned bytes = ipf > 1 ? unit_len[u] : ecs_size[(size_t)f];
            want[L.CU + L.CU + 1 + u] = pf[(size_t)f] ? 1u + (unsigned)f : 0u;
            want[u] = (unsigned)((size_t)f * L.R + (ipf > 1 ? unit_off[u] : 0u));
            want[L.CU + u] = subs;
            subs += (unsigned)(ipf > 1 ? unit_subs_restated(bytes) : file_subs_restated(bytes));
        }
    }
    want[L.CU + nu] = subs;
    CHECK(hm == want, "the words that travel (C %zu cnt %d ipf %zu)", L.C, cnt, ipf);
    CHECK(fill.subs == subs && fill.own_tables == own, "the fill's answer: %u %d, want %u %d", fill.subs, (int)fill.own_tables, subs, (int)own);
    const unsigned *ecs_off = hm.data() + L.ecs_off, *sub_off = hm.data() + L.sub_off, *tabset_of = hm.data() + L.tabset_of;
    CHECK(sub_off[0] == 0 && sub_off[nu] == fill.subs && fill.subs <= L.state_subs, "subsequences %u of %zu", fill.subs, L.state_subs);
    // the device's index arrays, written the way the launches write them
    std::vector<unsigned> dm(L.meta_words, 0);
    std::memcpy(dm.data(), hm.data(), L.upload_words * sizeof(unsigned));
    unsigned long long sum = 0;
    for (size_t u = 0; u < nu; u++) {
        const size_t f = u / ipf;
        CHECK(sub_off[u] < sub_off[u + 1], "sub_off does not increase at %zu", u);
        CHECK(tabset_of[u] == 0 || tabset_of[u] == 1 + f, "tabset_of[%zu] = %u", u, tabset_of[u]);
        // the reader's frame: its subsequences (a file's: the zero one among them) and 16 bytes of overshoot
        const size_t begin = ecs_off[u], end = begin + (size_t)(sub_off[u + 1] - sub_off[u]) * SB + 16;
        CHECK(begin >= f * L.R && end <= (f + 1) * L.R && end <= L.ecs_bytes, "frame %zu: [%zu, %zu) outside its file's [%zu, %zu)", u, begin, end, f * L.R, (f + 1) * L.R);
        CHECK(begin % 16 == 0, "frame %zu starts at %zu", u, begin);
        const size_t bytes = ipf > 1 ? unit_len[u] : ecs_size[f];
        for (size_t b = begin; b < end && b < L.ecs_bytes; b++) { // (the worker wrote all of it: the frame's bytes, zeros behind them)
            sum += ecs[b];
            if (ecs[b] != (b - begin < bytes ? 0x11 : 0)) {
                CHECK(false, "frame %zu: byte %zu is %u", u, b - begin, (unsigned)ecs[b]);
                break;
            }
        }
        for (unsigned s = sub_off[u]; s < sub_off[u + 1]; s++) dm[L.frame_of + s] = (unsigned)u; // k_hd_frame_of
        dm[L.frame_blocks + u] = 1;
    }
    dm[L.changed] = 3;
    dm[L.status] = 0;
    unsigned flags[2];
    std::memcpy(flags, dm.data() + L.changed, sizeof flags); // the read-back: two words
    CHECK(flags[0] == 3 && flags[1] == 0 && &dm[L.status] == &dm[L.meta_words - 1], "flags");
    if (sum == 0xffffffffffffffffull) std::printf("(unreachable)\n");
}

void sweep() {
    const size_t Cs[] = {1, 2, 5}, ipfs[] = {1, 2, 7}, files[] = {1, SB - 1, SB, SB + 1, 3 * SB + 5};
    unsigned long long lcg = 20261019;
    for (size_t C : Cs)
        for (size_t ipf : ipfs)
            for (size_t max_file : files) {
                const hvc::HdChunkLayout L = hvc::hd_chunk_layout(C, ipf, max_file);
                const Restated r = restate(C, ipf, max_file);
                cases++;
                CHECK(L.C == C && L.ipf == ipf && L.CU == r.CU && L.nsub_max == r.nsub_max && L.R == r.R && L.ecs_bytes == r.ecs_bytes, "sizes");
                CHECK(L.R % 16 == 0, "R = %zu", L.R);
                CHECK(L.ecs_off == 0 && L.sub_off == r.sub_off && L.tabset_of == r.tabset_of && L.frame_of == r.frame_of &&
                          L.frame_blocks == r.frame_blocks && L.changed == r.changed && L.status == r.status && L.meta_words == r.meta_words,
                      "offsets");
                CHECK(L.upload_words == r.upload_words && L.state_subs == r.state_subs && L.file_cap() == r.cap, "upload / state / cap");
                // in order, disjoint, nothing between them, ending at meta_words; the prefix that travels ends where frame_of begins
                CHECK(L.ecs_off + L.CU == L.sub_off && L.sub_off + L.CU + 1 == L.tabset_of && L.tabset_of + L.CU == L.frame_of &&
                          L.frame_of == L.upload_words && L.frame_of + L.state_subs == L.frame_blocks && L.frame_blocks + L.CU == L.changed &&
                          L.changed + 1 == L.status && L.status + 1 == L.meta_words,
                      "regions");
                CHECK(L.fits(), "a small chunk is refused");
                for (int cnt = 1; cnt <= (int)C; cnt++)
                    for (int pattern = 0; pattern < 3; pattern++) { // tables of their own: no file, every file, every other file
                        std::vector<char> pf((size_t)cnt);
                        for (int f = 0; f < cnt; f++) pf[(size_t)f] = pattern == 1 || (pattern == 2 && (f & 1)) ? 1 : 0;
                        const size_t n = (size_t)cnt * ipf;
                        size_t combos = 1;
                        for (size_t i = 0; i < n && combos <= 1296; i++) combos *= 6;
                        const bool all = combos <= 1296; // every combination of the six lengths, or 1296 drawn ones
                        if (!all) combos = 1296;
                        std::vector<unsigned> lens(n);
                        for (size_t k = 0; k < combos; k++) {
                            size_t code = k;
                            for (int f = 0; f < cnt; f++) {
                                // a file's segment is shorter than the file: its intervals share max_file bytes; without
                                // intervals the worker's cap is the bound
                                size_t left = ipf > 1 ? max_file : L.file_cap();
                                for (size_t q = 0; q < ipf; q++) {
                                    size_t pick;
                                    if (all) {
                                        pick = code % 6;
                                        code /= 6;
                                    } else {
                                        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                                        pick = (size_t)(lcg >> 33) % 6;
                                    }
                                    const size_t cand[6] = {0, 1, SB - 1, SB, SB + 1, left}; // (the last: all the room there is)
                                    const size_t len = cand[pick] < left ? cand[pick] : left;
                                    lens[(size_t)f * ipf + q] = (unsigned)len;
                                    if (ipf > 1) left -= len;
                                }
                            }
                            one_fill(L, cnt, lens, pf);
                        }
                    }
            }
    std::printf("sweep layouts %llu fills %llu\n", cases, fills);
}

void limits() {
    const size_t lim = (size_t)1 << 31;
    auto fits = [](size_t C, size_t nsub_max, size_t R) {
        hvc::HdChunkLayout L{};
        L.C = C, L.nsub_max = nsub_max, L.R = R;
        return L.fits();
    };
    // C * nsub_max
    CHECK(fits(1, lim - 1, 16), "one below");
    CHECK(!fits(1, lim, 16) && !fits(1, lim + 1, 16) && !fits(2, lim / 2, 16) && !fits(65535, 32769, 16), "at and above");
    CHECK(fits(65535, 32768, 16), "65535 x 32768 is below");
    // C * R
    CHECK(fits(1, 1, lim - 16) && fits(3, 1, (lim - 16) / 3), "one below");
    CHECK(!fits(1, 1, lim) && !fits(1, 1, lim + 16) && !fits(4, 1, lim / 4) && !fits(5, 1, (size_t)1 << 40), "at and above");
    // through the layout: one file whose region ends 112 bytes below 2^31, and the next size up
    const size_t nsub = (lim - 16) / SB; // 16777215: R = nsub * SB + 16 = 2^31 - 112
    const hvc::HdChunkLayout below = hvc::hd_chunk_layout(1, 1, (nsub - 1) * SB), above = hvc::hd_chunk_layout(1, 1, (nsub - 1) * SB + 1);
    CHECK(below.R == lim - 112 && below.fits(), "R = %zu", below.R);
    CHECK(above.R == lim + 16 && !above.fits(), "R = %zu", above.R);
    const hvc::HdChunkLayout two = hvc::hd_chunk_layout(2, 7, (nsub / 2 - 20) * SB);
    CHECK(two.fits() == (2 * two.R < lim && 2 * two.nsub_max < lim), "two files with intervals");
    CHECK(!hvc::hd_chunk_layout(2, 7, (nsub / 2) * SB).fits(), "two files with intervals, above");
    std::printf("limits checked\n");
}

void restart() {
    using hvc::hd_restart_units;
    auto is = [](const hvc::HdRestart &r, bool host, unsigned interval, unsigned ipf) { return r.host == host && r.interval == interval && r.ipf == ipf; };
    // one interval covers the scan, or none is declared, or they are not honoured: frame = file
    CHECK(is(hd_restart_units(10, true, 10, 4096), false, 0, 1) && is(hd_restart_units(9, true, 10, 4096), false, 0, 1), "mcus <= interval");
    CHECK(is(hd_restart_units(100, true, 0, 4096), false, 0, 1) && is(hd_restart_units(100, false, 7, 4096), false, 0, 1), "no DRI / not honoured");
    CHECK(is(hd_restart_units(11, true, 10, 4096), false, 10, 2), "mcus = interval + 1");
    CHECK(is(hd_restart_units(8160, true, 5, 4096), false, 5, 1632), "1080p in intervals of 5");
    CHECK(hd_restart_units(11, true, 10, 4096).blocks_per_frame(6) == 60, "blocks per reader frame");
    // the batch pipeline's ceiling: q > 4096
    CHECK(is(hd_restart_units(4095, true, 1, 4096), false, 1, 4095) && is(hd_restart_units(4096, true, 1, 4096), false, 1, 4096) &&
              is(hd_restart_units(4097, true, 1, 4096), true, 0, 1),
          "4096 intervals a file");
    CHECK(is(hd_restart_units(2 * 4096 + 1, true, 2, 4096), true, 0, 1) && is(hd_restart_units(2 * 4096, true, 2, 4096), false, 2, 4096), "... rounded up");
    // the single call's: q * n_frames > 65535, stated as a ceiling of 65535 / n_frames
    for (unsigned long long n = 1; n <= 70000; n = n < 300 ? n + 1 : n + 997)
        for (unsigned long long q = 2; q <= 70000; q = q < 300 ? q + 1 : q + 991)
            for (unsigned long long d = 0; d < 3; d++) {
                const unsigned long long qq = d == 0 ? q : 65535 / n + d - 1; // ... and around the ceiling itself
                if (qq < 2) continue;
                const hvc::HdRestart r = hd_restart_units(qq * 3, true, 3, 65535ull / n);
                CHECK(r.host == (qq * n > 65535ull) && (r.host || (r.ipf == qq && r.interval == 3)), "q %llu n %llu", qq, n);
            }
    CHECK(is(hd_restart_units(3 * 21845, true, 3, 65535 / 3), false, 3, 21845) && is(hd_restart_units(3 * 21846, true, 3, 65535 / 3), true, 0, 1), "three files");
    std::printf("restart checked\n");
}

} // namespace

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "";
    if (!std::strcmp(what, "sweep")) sweep();
    else if (!std::strcmp(what, "limits")) limits();
    else if (!std::strcmp(what, "restart")) restart();
    else {
        std::fprintf(stderr, "usage: hdec_plan_harness sweep | limits | restart\n");
        return 2;
    }
    if (failures) {
        std::printf("failures %d\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
