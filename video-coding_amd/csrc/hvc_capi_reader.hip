// hvc_capi_reader.hip -- the GPU Huffman reader (hvc_hdec.hip) behind the C ABI: hvc_jpeg_entropy_decode_gpu and the batch
// pipeline built on it (hvc_jpeg_decode_batch_gpu: host threads unstuff, the copy engine uploads, the reader and the block
// stage run per chunk).  What both decide and lay out on the host -- restart units, subsequence counts, a ring slot's index
// arrays -- is plain C++ in hvc_hdec_plan.h; the batch pipeline's per-chunk steps are UniformGpuReader's and its host-output
// thread ChunkDownloader (hvc_uniform_reader.h), decode_batch_gpu is the loop over them.
#include "hvc_batch.h"
#include "hvc_uniform_reader.h"

#ifndef HVC_NRD
#define HVC_NRD 2
#endif
constexpr int NRD = HVC_NRD; // reader streams in use by the batch pipeline (round 1: 1: 71 Gpixel/s on config 3, 2: 77, 3: 79 with half as much scratch again)

// Two files of one batch: the same frame geometry (sizes, sampling, planes)?  The Huffman table selectors of the scan
// may differ -- the GPU reader takes every file's tables from the file itself.
static bool same_geometry(const hvc_jpeg_info &a, const hvc_jpeg_info &b) {
    if (a.n_comp != b.n_comp || a.coef_count != b.coef_count || a.width != b.width || a.height != b.height ||
        std::memcmp(a.layout, b.layout, sizeof a.layout))
        return false;
    for (int i = 0; i < a.n_comp; i++) {
        const hvc_jpeg_component &x = a.comp[i], &y = b.comp[i];
        if (x.identifier != y.identifier || x.hscale != y.hscale || x.vscale != y.vscale || x.decoded_width != y.decoded_width ||
            x.decoded_height != y.decoded_height || x.actual_width != y.actual_width || x.actual_height != y.actual_height)
            return false;
    }
    return true;
}

// Geometry part of the GPU Huffman decoder's parameter block; false = this frame layout needs the host decoder.
static bool gd_geometry(const hvc_jpeg_info &info0, hvc::HdParams &P) {
    std::memset(&P, 0, sizeof P);
    if (info0.n_comp < 1 || info0.n_comp > 3) return false;
    P.n_comp = info0.n_comp;
    const hvc_jpeg_component &c0 = info0.comp[0];
    if (c0.hscale < 1 || c0.vscale < 1) return false;
    P.mbs_wide = c0.decoded_width / (8 * c0.hscale);
    P.mbs_high = c0.decoded_height / (8 * c0.vscale);
    int base = 0;
    for (int i = 0; i < info0.n_comp; i++) {
        P.comp[i].h = info0.comp[i].hscale;
        P.comp[i].v = info0.comp[i].vscale;
        P.comp[i].bw = info0.layout[i].blocks_w;
        P.comp[i].mcu_base = base;
        P.comp[i].coef_off = info0.layout[i].coef_offset;
        if (P.comp[i].h < 1 || P.comp[i].v < 1) return false;
        // the decoder raises when the MCU grid leaves a plane ("Plane.set out of bounds"): host path decides
        if (P.mbs_wide * P.comp[i].h > info0.layout[i].blocks_w || P.mbs_high * P.comp[i].v > info0.layout[i].blocks_h)
            return false;
        if (base + P.comp[i].h * P.comp[i].v > HVC_HD_MAX_MCU_BLOCKS) return false;
        for (int k = 0; k < P.comp[i].h * P.comp[i].v; k++) P.b2comp[base + k] = (unsigned char)i;
        base += P.comp[i].h * P.comp[i].v;
    }
    P.blocks_per_mcu = base;
    const unsigned long long bpf = (unsigned long long)P.mbs_wide * P.mbs_high * base;
    if (bpf == 0 || bpf >= (1ull << 31) || info0.coef_count >= (1ull << 32)) return false;
    P.blocks_per_frame = (unsigned)bpf;
    return true;
}

// The per-subsequence arrays of the GPU Huffman decoder inside one allocation of HVC_HD_STATE_BYTES(n).
static void gd_carve_state(hvc::HdParams &P, void *mem, size_t n) {
    unsigned long long *sp = (unsigned long long *)mem;
    P.start_used = sp;
    P.exit_a = sp + n;
    P.exit_b = sp + 2 * n;
    P.exit_c = sp + 3 * n;
    unsigned *up = (unsigned *)(sp + 4 * n);
    P.nblk = up;
    P.list0 = up + n;
    P.list1 = up + 2 * n;
    P.list_n = up + 3 * n;
}

// Huffman tables of a batch -> device: the value tables and, when the components use at most two table
// sets, the synchronisation tables (HdSpec) behind them.  Fills P.tables / P.spec / P.slotmask.
static int gd_upload_tables(hvc_ctx *c, const hvc::HdTables &t, hvc::HdParams &P, hipStream_t st) {
    int r;
    if ((r = grow(c, c->gd_tables, sizeof(hvc::HdTables) + sizeof(hvc::HdSpec) + sizeof(hvc::HdSpecOvf)))) return r;
    hvc::HdSpec spec;
    hvc::HdSpecOvf spec_ovf; // (the overflow records of tables with more than HVC_HD_SUBTABLES long prefixes: hvc_hdec.h)
    unsigned char slot[4];
    static const bool classic = std::getenv("HVC_HD_CLASSIC") != nullptr; // tests: force k_hd_round / k_hd_write
    const bool have_spec = hvc::make_spec(t, P.n_comp, spec, slot, P.slot_rep, &spec_ovf) && !classic;
    // file after file with the same tables (the usual case: an encoder's fixed set) finds them on the device already
    if (!c->gd_tables_host) c->gd_tables_host.reset(new (std::nothrow) hvc::HdTables);
    if (!c->gd_tables_host) return HVC_E_OUT_OF_MEMORY;
    if (!(c->gd_tables_valid && c->gd_tables_ncomp == P.n_comp && !std::memcmp(c->gd_tables_host.get(), &t, sizeof t))) {
        c->gd_tables_valid = false;
        HIPCHK(c, hipMemcpyAsync(c->gd_tables.p, &t, sizeof t, hipMemcpyHostToDevice, st));
        if (have_spec) {
            HIPCHK(c, hipMemcpyAsync(c->gd_tables.as<char>() + sizeof t, &spec, sizeof spec, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(c->gd_tables.as<char>() + sizeof t + sizeof spec, &spec_ovf, sizeof spec_ovf, hipMemcpyHostToDevice, st));
        }
        HIPCHK(c, hipStreamSynchronize(st)); // the sources live on a stack frame
        std::memcpy(c->gd_tables_host.get(), &t, sizeof t);
        c->gd_tables_ncomp = P.n_comp;
        c->gd_tables_valid = true;
    }
    P.tables = c->gd_tables.as<const hvc::HdTables>();
    P.spec = have_spec ? (const hvc::HdSpec *)(c->gd_tables.as<char>() + sizeof t) : nullptr;
    P.spec_ovf = have_spec ? (const hvc::HdSpecOvf *)(c->gd_tables.as<char>() + sizeof t + sizeof(hvc::HdSpec)) : nullptr;
    P.ftabs = nullptr;
    P.tabset_of = nullptr;
    P.slotmask = P.selmask = 0;
    for (int b = 0; b < P.blocks_per_mcu; b++) {
        P.slotmask |= (unsigned)slot[P.b2comp[b]] << b;
        P.selmask |= (unsigned)slot[P.b2comp[b]] << (2 * b);
    }
    return HVC_OK;
}

// PF mode: one work list per frame (hvc::HdParams::list_fn) pays where a frame fills workgroups of 512 subsequences by
// itself -- 1080p files have 7 000 -- and the frames fit the launch grid's second dimension; batches of small files
// keep the batch-wide lists, which pack the subsequences of many frames into one workgroup.
static bool gd_lists_per_frame(size_t total_sub, int n_frames) {
    return n_frames >= 1 && n_frames <= 65535 && total_sub / (size_t)n_frames >= 1024;
}

// PF mode (per-frame Huffman tables, hvc_hdec.h): which tables block b of an MCU reads = its component
static unsigned gd_component_selmask(const hvc::HdParams &P) {
    unsigned m = 0;
    for (int b = 0; b < P.blocks_per_mcu; b++) m |= (unsigned)P.b2comp[b] << (2 * b);
    return m;
}
// PF mode's part of the parameter block: the records at ftabs, tabset_of naming every reader frame's; list_fn: work lists
// per file (k_hd_sync_pf) for files of at most max_frame_sub subsequences -- where gd_lists_per_frame says so -- or null
static void gd_params_pf(hvc::HdParams &P, const hvc::HdFrameTabs *ftabs, const unsigned *tabset_of, unsigned *list_fn, unsigned max_frame_sub) {
    P.tables = nullptr;
    P.spec = nullptr;
    P.ftabs = ftabs;
    P.tabset_of = tabset_of;
    P.selmask = gd_component_selmask(P);
    if (list_fn) {
        P.list_fn = list_fn;
        P.max_frame_sub = max_frame_sub;
    }
}

// Restart intervals honoured (hvc_set_restart_markers) and the first file's scan has more than one: every interval of
// every file is a reader frame of its own (hvc_hdec.h HdParams::rst_*).  P: gd_geometry's; max_ipf: the caller's ceiling
// on intervals per file (beyond it: host = the host reader's).
static hvc::HdRestart gd_restart_units(const uint8_t *jpeg0, size_t size0, hvc::HdParams &P, unsigned long long max_ipf) {
    const bool honour = hvc::tl_honour_restart;
    const hvc::HdRestart ru = hvc::hd_restart_units((unsigned long long)P.mbs_wide * (unsigned long long)P.mbs_high, honour,
                                                    honour ? hvc::restart_interval_of(jpeg0, size0) : 0, max_ipf);
    if (ru.ipf > 1) {
        P.rst_mcus = ru.interval;
        P.rst_ipf = ru.ipf;
        P.blocks_per_frame = ru.blocks_per_frame((unsigned)P.blocks_per_mcu);
    }
    return ru;
}

// Enqueue the whole decode on `st`: the clearing launch (frame_of, flags, list lengths), `rounds` synchronisation
// launches, the finish passes -- kernels only, no memset node in between.  Afterwards *P.changed holds the number of the
// last launch that still changed something (gd_unsettled), *P.status the error bits.
static hipError_t gd_enqueue(const hvc::HdParams &P, int rounds, hipStream_t st) {
    hipError_t e = hvc::launch_hd_frame_of(P, st);
    for (int r = 0; r < rounds && e == hipSuccess; r++) e = hvc::launch_hd_round(P, r, st);
    if (e == hipSuccess) e = hvc::launch_hd_finish(P, rounds, st);
    return e;
}
// the `changed` word after gd_enqueue(P, rounds): the last of the launches 0 .. rounds - 1 still moved a hand-over
static bool gd_unsettled(unsigned changed_word, int rounds) { return rounds > 1 && changed_word == (unsigned)(rounds - 1); }

// ---------------------------------------------------------------------------
// Huffman decoding on the GPU (hvc_hdec.hip).  Returns HVC_OK with *used_gpu = 1 when the coefficient
// records at d_coefs are complete; HVC_OK with *used_gpu = 0 when the stream needs the host decoder
// (nothing usable was written); or the error the host decoder would report while parsing headers.
// HVC_CALL_TIMING=1 (experiments): where a single-file call spends its host time, to stderr
static bool call_timing() {
    static const bool on = std::getenv("HVC_CALL_TIMING") != nullptr;
    return on;
}
struct StageClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    char line[512];
    int n = 0;
    void mark(const char *what) {
        if (!call_timing()) return;
        const auto now = std::chrono::steady_clock::now();
        n += std::snprintf(line + n, sizeof line - (size_t)n, " %s %.1f", what, std::chrono::duration<double, std::micro>(now - last).count());
        if (n > (int)sizeof line - 64) n = (int)sizeof line - 64;
        last = now;
    }
    void done() {
        if (!call_timing()) return;
        std::fprintf(stderr, "hvc call timing (us):%s | total %.1f\n", line, std::chrono::duration<double, std::micro>(last - t0).count());
    }
};

// What the three steps of gpu_entropy_decode share.  Copies out of h_meta and tabset_of are in flight until the call's stream
// has drained: the caller declares this BEFORE the guard that waits for it.
struct GdCall {
    hvc::HdParams P;
    hvc::HdRestart ru{false, 0, 1};
    // Huffman tables per file (decoder.ml:238-259 picks them from the file's own DHT segments): the distinct sets of
    // the batch and which one every frame uses.  One set that fits two slots = the fast LDS-table kernels; anything
    // else = per-frame tables in device memory (PF mode, hvc_hdec.h).
    std::vector<hvc::HdTables> sets;
    std::vector<unsigned> tabset_of;
    std::vector<unsigned> ecs_off, sub_off; // per reader frame: a file, or one of its restart intervals (sub_off: one more)
    std::vector<unsigned> h_meta;           // the index arrays that travel
    size_t units = 0, bytes = 0, subs = 0;  // reader frames, bytes of the pinned segment buffer in use, subsequences
};
constexpr int GD_HOST = 1; // a step's answer beside the hvc_status codes (none is positive): the stream needs the host decoder

// Step 1: the files' places in the pinned buffer, then headers, tables and segments (unstuffed on the way there).
static int gd_lay_out_and_unstuff(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, const hvc_jpeg_info &info0, GdCall &g) {
    const unsigned rst = g.ru.interval, ipf = g.ru.ipf;
    g.units = (size_t)n_frames * ipf;
    // The segments go straight from the files into ONE pinned buffer (unstuffed on the way) and from there to the
    // device: laid out by an upper bound of every segment's length -- its file's -- so that the places are known before
    // the files are read.  (Through per-file vectors, a pageable batch buffer and the runtime's own staging the bytes of
    // a 1 MB file were copied three times before the copy engine saw them: 0.15 of the call's 1.0 ms.)
    const size_t SB = hvc::HD_SB;
    std::vector<unsigned> file_off, uoff, ulen; // (per file; per interval of the file in hand)
    size_t bytes = 0, subs = 0;
    try {
        g.tabset_of.assign(g.units, 0u);
        g.ecs_off.resize(g.units);
        g.sub_off.resize(g.units + 1);
        file_off.resize((size_t)n_frames);
        uoff.resize(ipf);
        ulen.resize(ipf);
        for (int f = 0; f < n_frames; f++) {
            const size_t nsub_most = hvc::hd_file_subs(sizes[f]); // an entropy-coded segment is shorter than its file
            file_off[(size_t)f] = (unsigned)bytes;
            // SB = 128: every frame starts on a 16-byte boundary, 16 zero bytes of overshoot; every interval has a slot of
            // its own (hvc::hd_unit_slot: at most 2 SB + 16 bytes more than its bytes)
            bytes += ipf > 1 ? nsub_most * SB + (size_t)ipf * (2 * SB + 16) : nsub_most * SB + 16;
            if (bytes >= (1ull << 31)) return GD_HOST;
        }
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    if (int r = grow(c, c->gd_h_ecs, bytes, GROW_READER_STAGE)) return r;
    uint8_t *const h_ecs = c->gd_h_ecs.as<uint8_t>();
    try {
        hvc::HdTables t;
        for (int f = 0; f < n_frames; f++) {
            hvc_jpeg_info fi;
            int r = hvc_jpeg_read_header(jpegs[f], sizes[f], &fi);
            if (r) return r;
            if (!same_geometry(fi, info0)) return HVC_E_INVALID_ARG; // a batch shares one geometry
            bool ok = false;
            const size_t room = (hvc::hd_file_subs(sizes[f]) - 1) * SB; // (the frame's slot without its extra subsequence and overshoot)
            size_t got = 0;
            uint8_t *const fdst = h_ecs + file_off[(size_t)f];
            if (ipf > 1) { // its intervals, each in a slot of its own (zeros behind the bytes: written with them)
                hvc::RstUnits ru{rst, ipf, uoff.data(), ulen.data()};
                r = hvc::prepare_gpu_decode_to(jpegs[f], sizes[f], &fi, t, fdst, room + (size_t)ipf * (2 * SB + 16), &got, ok, &ru);
                if (r) return r;
                if (!ok) return GD_HOST;
                for (unsigned q = 0; q < ipf; q++) {
                    const size_t u = (size_t)f * ipf + q;
                    g.ecs_off[u] = file_off[(size_t)f] + uoff[q];
                    g.sub_off[u] = (unsigned)subs;
                    subs += hvc::hd_unit_subs(ulen[q]);
                }
            } else {
                r = hvc::prepare_gpu_decode_to(jpegs[f], sizes[f], &fi, t, fdst, room, &got, ok);
                if (r) return r;
                if (!ok) return GD_HOST;
                const size_t nsub = hvc::hd_file_subs(got); // one extra: the reader sees zeros past the end
                std::memset(fdst + got, 0, nsub * SB + 16 - got); // (the buffer is reused from call to call)
                g.ecs_off[(size_t)f] = file_off[(size_t)f];
                g.sub_off[(size_t)f] = (unsigned)subs;
                subs += nsub;
            }
            if (subs >= (1ull << 31)) return GD_HOST;
            size_t k = g.sets.size(); // newest first: files of one source tend to come in runs
            while (k > 0 && std::memcmp(&g.sets[k - 1], &t, sizeof t)) k--;
            if (k == 0) {
                g.sets.push_back(t);
                k = g.sets.size();
            }
            for (unsigned q = 0; q < ipf; q++) g.tabset_of[(size_t)f * ipf + q] = (unsigned)(k - 1);
        }
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    g.sub_off[g.units] = (unsigned)subs;
    g.bytes = bytes;
    g.subs = subs;
    return HVC_OK;
}

// Step 2: device scratch, the uploads on c->stream, the parameter block.  From its first copy on, copies out of g's vectors,
// ftabs and the reused pinned buffer are in flight (the caller's guard waits for them on every way out).
static int gd_upload_and_params(hvc_ctx *c, int n_frames, int16_t *d_coefs, size_t coef_fs, const AfterReader *after, GdCall &g,
                                std::vector<hvc::HdFrameTabs> &ftabs) {
    hvc::HdParams &P = g.P;
    const size_t nU = g.units, subs = g.subs; // the reader's frames: files, or their restart intervals
    const unsigned ipf = g.ru.ipf;
    P.n_frames = (int)nU;
    P.total_sub = (unsigned)subs;
    // the index arrays: [ecs_off n][sub_off n + 1] travel; [frame_of subs] is filled on the device from sub_off,
    // [frame_blocks n][changed, status] are written there
    const size_t meta_words = nU + (nU + 1) + subs + nU + 2;
    try {
        g.h_meta.resize(2 * nU + 1);
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    for (size_t f = 0; f < nU; f++) {
        g.h_meta[f] = g.ecs_off[f];
        g.h_meta[nU + f] = g.sub_off[f];
    }
    g.h_meta[2 * nU] = g.sub_off[nU];
    int r;
    if ((r = grow(c, c->gd_ecs, g.bytes + HVC_HD_ECS_SLACK))) return r;
    if ((r = grow(c, c->gd_meta, meta_words * sizeof(unsigned) + 64))) return r;
    if ((r = grow(c, c->gd_state, HVC_HD_STATE_BYTES(subs)))) return r;
    if ((r = grow(c, c->gd_dcd, nU * P.blocks_per_frame * sizeof(int16_t)))) return r;
    P.dcd = c->gd_dcd.as<int16_t>();
    unsigned *m = c->gd_meta.as<unsigned>();
    unsigned *d_ecs_off = m, *d_sub_off = m + nU, *d_frame_of = d_sub_off + nU + 1;
    unsigned *d_frame_blocks = d_frame_of + subs, *d_flags = d_frame_blocks + nU;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->gd_ecs.p, c->gd_h_ecs.p, g.bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(m, g.h_meta.data(), g.h_meta.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    bool pf = g.sets.size() > 1;
    bool any_ovf = false; // a table with prefixes beyond its sub-tables: only the fast kernels know the overflow search
    for (const hvc::HdTables &ts : g.sets) any_ovf |= hvc::tables_use_overflow(ts, P.n_comp);
    if (!pf) {
        if ((r = gd_upload_tables(c, g.sets[0], P, st))) return r;
        static const bool classic = std::getenv("HVC_HD_CLASSIC") != nullptr;
        pf = !P.spec && !classic; // one set, but three different table pairs in it: no slots for that, per-component tables
        if (any_ovf && !P.spec && !pf) return GD_HOST; // (HVC_HD_CLASSIC: the general kernels -> the host reader has it)
    }
    P.coef_fs = coef_fs;
    if (any_ovf && !hvc::hd_write2_fits(P)) return GD_HOST; // (k_hd_write, the general write pass, would be chosen)
    if (pf) {
        if (!hvc::hd_write2_fits(P)) return GD_HOST; // (PF mode has the fast write pass only)
        try {
            ftabs.resize(g.sets.size());
        } catch (const std::bad_alloc &) {
            return HVC_E_OUT_OF_MEMORY;
        }
        for (size_t k = 0; k < g.sets.size(); k++) hvc::make_frame_tabs(g.sets[k], P.n_comp, ftabs[k]);
        const size_t tb = g.sets.size() * sizeof(hvc::HdFrameTabs);
        if ((r = grow(c, c->gd_ftabs, tb + nU * sizeof(unsigned)))) return r;
        HIPCHK(c, hipMemcpyAsync(c->gd_ftabs.p, ftabs.data(), tb, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->gd_ftabs.as<char>() + tb, g.tabset_of.data(), nU * sizeof(unsigned), hipMemcpyHostToDevice, st));
        unsigned *list_fn = nullptr, max_frame_sub = 0;
        if (gd_lists_per_frame(P.total_sub, n_frames)) {
            if ((r = grow(c, c->gd_fcnt, (size_t)HVC_HD_LIST_N * nU * sizeof(unsigned)))) return r;
            list_fn = c->gd_fcnt.as<unsigned>(); // work lists per file (k_hd_sync_pf)
            for (size_t f = 0; f < (size_t)n_frames; f++) max_frame_sub = std::max(max_frame_sub, g.sub_off[(f + 1) * ipf] - g.sub_off[f * ipf]);
        }
        gd_params_pf(P, c->gd_ftabs.as<const hvc::HdFrameTabs>(), (const unsigned *)(c->gd_ftabs.as<char>() + tb), list_fn, max_frame_sub);
    }
    P.ecs = c->gd_ecs.as<const uint8_t>();
    P.ecs_off = d_ecs_off;
    P.sub_off = d_sub_off;
    P.frame_of = d_frame_of;
    P.coefs = d_coefs;
    P.coef_fs = coef_fs;
    gd_carve_state(P, c->gd_state.p, subs);
    P.frame_blocks = d_frame_blocks;
    P.changed = d_flags;
    P.status = d_flags + 1;
    if (after && after->dc_plane) {
        P.dc_plane = after->dc_plane;
        P.dc_fs = after->dc_fs;
    }
    return HVC_OK;
}

// Step 3: the reader's launches, the caller's consumer behind them, the two flags; a stream that has not settled is done
// again round by round.  flags: [changed, status] of the run that counts; *consumer_enqueued: the consumer ran behind it.
static int gd_run_and_settle(hvc_ctx *c, const hvc::HdParams &P, AfterReader *after, StageClock &clk, unsigned flags[2], bool *consumer_enqueued) {
    hipStream_t st = c->stream;
    int r;
    // (no clearing of the records: the write pass stores every index of every coded block exactly once)
    // Everything in one go, as the batch pipeline does: four synchronisation launches (all of k_hd_sync's rounds count
    // as the first), the finish passes, one look at the two flags.  Only a stream that has not settled by then -- smooth
    // content can take hundreds of rounds -- is done again round by round.
    const int first_rounds = 4;
    HIPCHK(c, gd_enqueue(P, first_rounds, st)); // (its first launch clears the flags and the list lengths)
    clk.mark("reader-enqueued");
    // The consumer of the records goes in behind the reader before anybody has looked at the reader's flags: a call
    // that waited for them first and launched the block stage afterwards stood still for 75 us in between (one file:
    // profiles/r03e_single_call_timeline_before.txt).  Records of a run that turns out unusable are garbage of the
    // right size: the consumer's output is thrown away then.
    *consumer_enqueued = false;
    if (after && after->enqueue) {
        if ((r = after->enqueue())) return r;
        *consumer_enqueued = true;
    }
    clk.mark("consumer-enqueued");
    flags[0] = flags[1] = 0;
    HIPCHK(c, hipMemcpyAsync(flags, P.changed, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    clk.mark("synchronised");
    clk.done();
#ifdef HVC_HD_STATS // experiments: entries of k_hd_sync's work lists per round; walks / inner rounds of k_hd_round's launches
    {
        unsigned ln[HVC_HD_LIST_N];
        HIPCHK(c, hipMemcpy(ln, P.list_n, sizeof ln, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "hd stats: %u subsequences; lists", P.total_sub);
        for (int q = 2; q < HVC_HD_LIST_N - 2; q++) std::fprintf(stderr, " %u", ln[q]);
        std::fprintf(stderr, "; k_hd_round walks %u, inner rounds %u; changed %u status %u\n", ln[HVC_HD_LIST_N - 2], ln[HVC_HD_LIST_N - 1], flags[0], flags[1]);
        unsigned long long hs[4];
        hvc::hd_stats_read(hs);
        std::fprintf(stderr, "hd stats: round 0 walked %llu symbols (%.1f a subsequence); 64 x the longest walk of every wavefront: %llu (lanes busy %.1f %%)\n",
                     hs[0], (double)hs[0] / P.total_sub, hs[1], 100.0 * (double)hs[0] / (double)(hs[1] ? hs[1] : 1));
        const unsigned long long own = hs[2] & 0xffffffffull, over = hs[2] >> 32;
        std::fprintf(stderr, "hd stats: write pass %llu symbols inside the lanes' own subsequences + %llu beyond them (%.1f %%); 64 x trips of every wavefront: %llu (lanes busy %.1f %%)\n",
                     own, over, 100.0 * (double)over / (double)(own ? own : 1), hs[3], 100.0 * (double)(own + over) / (double)(hs[3] ? hs[3] : 1));
    }
#endif
    if (gd_unsettled(flags[0], first_rounds)) { // (the finish passes have turned the block counts into block indices: the rounds start over)
        *consumer_enqueued = false; // (it ran on records the write pass never stored)
        const int max_rounds = 48;
        int round = 0;
        HIPCHK(c, hvc::launch_hd_frame_of(P, st)); // flags and list lengths cleared again
        for (;; round++) {
            HIPCHK(c, hvc::launch_hd_round(P, round, st));
            if (round >= 4) {
                unsigned changed = 0;
                HIPCHK(c, hipMemcpyAsync(&changed, P.changed, sizeof changed, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
                if (!gd_unsettled(changed, round + 1)) break;
                if (round >= max_rounds) return GD_HOST; // does not settle: let the host decoder handle it
            }
        }
        HIPCHK(c, hvc::launch_hd_finish(P, round + 1, st)); // launches 0..round have run
        HIPCHK(c, hipMemcpyAsync(flags + 1, P.status, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return HVC_OK;
}

int gpu_entropy_decode(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, const hvc_jpeg_info &info0,
                       int16_t *d_coefs, size_t coef_fs, int *used_gpu, AfterReader *after) {
    *used_gpu = 0;
    if (after) after->speculated = false;
    StageClock clk;
    GdCall g;
    if (!gd_geometry(info0, g.P)) return HVC_OK;
    g.ru = gd_restart_units(jpegs[0], sizes[0], g.P, 65535ull / (unsigned long long)std::max(n_frames, 1)); // (the launches' grids: frames per launch)
    if (g.ru.host) return HVC_OK;
    int r;
    if ((r = gd_lay_out_and_unstuff(c, jpegs, sizes, n_frames, info0, g))) return r == GD_HOST ? HVC_OK : r;
    clk.mark("headers+unstuff");
    // From here on copies out of this call's own vectors (g.h_meta, ftabs, g.tabset_of) and out of the reused pinned
    // buffer are in flight: EVERY way out of the function waits for the stream first (the early returns included).
    std::vector<hvc::HdFrameTabs> ftabs; // (declared BEFORE the guard: destroyed after the guard has waited)
    struct SyncOnExit {
        hipStream_t s;
        ~SyncOnExit() { (void)hipStreamSynchronize(s); }
    } sync_on_exit{c->stream};
    if ((r = gd_upload_and_params(c, n_frames, d_coefs, coef_fs, after, g, ftabs))) return r == GD_HOST ? HVC_OK : r;
    clk.mark("uploads-enqueued");
    unsigned flags[2] = {0, 0};
    bool consumer_enqueued = false;
    if ((r = gd_run_and_settle(c, g.P, after, clk, flags, &consumer_enqueued))) return r == GD_HOST ? HVC_OK : r;
    const unsigned status = flags[1];
    static const bool hd_debug = std::getenv("HVC_HD_DEBUG") != nullptr; // (diagnostics: why a call went to the host reader)
    if (hd_debug) std::fprintf(stderr, "hd debug: frames %d subs %u changed %u status %u\n", g.P.n_frames, g.P.total_sub, flags[0], status);
    if (status) return HVC_OK; // the model raises / range / truncated stream: the host decoder reproduces it exactly
    *used_gpu = 1;
    if (after) after->speculated = consumer_enqueued;
    return HVC_OK;
}

int hvc_jpeg_entropy_decode_gpu(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int16_t *coefs,
                                size_t coef_fs, int where, hvc_jpeg_info *info, int *used_gpu) try {
    if (!c || !jpegs || !sizes || !coefs || !info || n_frames < 1) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    hvc::RestartScope honour(c->honour_restart);
    int r = hvc_jpeg_read_header(jpegs[0], sizes[0], info);
    if (r) return r;
    if ((n_frames > 1 && coef_fs < info->coef_count) || (coef_fs & 7)) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    int16_t *d = coefs;
    const size_t total = ((size_t)(n_frames - 1) * coef_fs + info->coef_count) * sizeof(int16_t);
    if (where == HVC_MEM_HOST) {
        if ((r = grow(c, c->gd_coefs, total))) return r;
        d = c->gd_coefs.as<int16_t>();
    } else if ((uintptr_t)coefs & 15) {
        return HVC_E_ALIGNMENT;
    }
    int gpu = 0;
    r = gpu_entropy_decode(c, jpegs, sizes, n_frames, *info, d, coef_fs, &gpu);
    if (r) return r;
    if (used_gpu) *used_gpu = gpu;
    if (gpu) {
        if (where == HVC_MEM_HOST) {
            for (int f = 0; f < n_frames; f++)
                HIPCHK(c, hipMemcpyAsync(coefs + (size_t)f * coef_fs, d + (size_t)f * coef_fs, info->coef_count * sizeof(int16_t),
                                         hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        return HVC_OK;
    }
    // host decoder (exact model behaviour for everything unusual)
    std::vector<int16_t> tmp;
    for (int f = 0; f < n_frames; f++) {
        hvc_jpeg_info fi;
        if ((r = hvc_jpeg_read_header(jpegs[f], sizes[f], &fi))) return r;
        if (fi.coef_count != info->coef_count || std::memcmp(fi.layout, info->layout, sizeof fi.layout)) return HVC_E_INVALID_ARG;
        if (where == HVC_MEM_HOST) {
            if ((r = hvc_jpeg_entropy_decode(jpegs[f], sizes[f], &fi, coefs + (size_t)f * coef_fs))) return r;
        } else {
            tmp.resize(info->coef_count);
            if ((r = hvc_jpeg_entropy_decode(jpegs[f], sizes[f], &fi, tmp.data()))) return r;
            HIPCHK(c, hipMemcpyAsync(coefs + (size_t)f * coef_fs, tmp.data(), info->coef_count * sizeof(int16_t),
                                     hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    return HVC_OK;
} HVC_ABI_CATCH

// ---------------------------------------------------------------------------
// UniformGpuReader and ChunkDownloader (hvc_uniform_reader.h): the per-chunk steps of the batch pipeline below

int UniformGpuReader::begin(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int *frames_per_chunk, int where,
                            size_t pixel_fs, OutputForm &form, bool *host_pipeline) {
    constexpr int NB = hvc_ctx::RING;
    c_ = c, jpegs_ = jpegs, sizes_ = sizes, n_frames_ = n_frames;
    *host_pipeline = true; // (every HVC_OK below but the last)
    int r = hvc_jpeg_read_header(jpegs[0], sizes[0], &info0_);
    if (r) return r;
    form.of(info0_);
    if ((r = form.batch_check(pixel_fs))) return r;
    const bool geo = gd_geometry(info0_, G_);
    if (geo) units_ = gd_restart_units(jpegs[0], sizes[0], G_, 4096); // (intervals of a few MCUs: half of every frame's subsequences would be padding)
    if (units_.host) return HVC_OK;
    const unsigned ipf = units_.ipf;
    { // the first file's probe: its tables are the batch's, and what the reader cannot take of it no chunk could
        bool ok = false;
        try {
            if (ipf > 1) {
                std::vector<uint8_t> tmp(sizes[0] + (size_t)ipf * (2 * hvc::HD_SB + 16) + hvc::HD_SB);
                std::vector<unsigned> uo(ipf), ul(ipf);
                hvc::RstUnits ru{units_.interval, ipf, uo.data(), ul.data()};
                size_t got = 0;
                r = hvc::prepare_gpu_decode_to(jpegs[0], sizes[0], &info0_, tables0_, tmp.data(), tmp.size(), &got, ok, &ru);
            } else {
                std::vector<uint8_t> tmp;
                r = hvc::prepare_gpu_decode(jpegs[0], sizes[0], &info0_, tables0_, tmp, ok);
            }
        } catch (const std::bad_alloc &) {
            return HVC_E_OUT_OF_MEMORY;
        }
        if (r) return r;
        if (!ok || !geo) return HVC_OK;
    }
    // the reader's launches want many subsequences at once, the pipeline at least four chunks
    // (measured: 256 files best in chunks of 64, 1024 and more in chunks of 256)
    int &fpc = *frames_per_chunk;
    if (fpc < 1) fpc = n_frames / 4 < 64 ? 64 : n_frames / 4 > 256 ? 256 : n_frames / 4;
    if (fpc > n_frames) fpc = n_frames;
    if ((unsigned long long)fpc * ipf > 65535ull) fpc = (int)(65535u / ipf); // (the reader's grids: frames per launch)
    const int C = fpc;
    n_chunks_ = (n_frames + C - 1) / C;
    size_t max_file = 0;
    for (int f = 0; f < n_frames; f++) {
        if (!jpegs[f]) return HVC_E_INVALID_ARG;
        max_file = sizes[f] > max_file ? sizes[f] : max_file;
    }
    L_ = hvc::hd_chunk_layout((size_t)C, ipf, max_file);
    if (!L_.fits()) return HVC_OK;
    const size_t CU = L_.CU, meta_bytes = L_.meta_words * sizeof(unsigned);
    const size_t ftabs_bytes = ((size_t)C + 1) * sizeof(hvc::HdFrameTabs); // record 0: the first file's tables, 1 + f: frame f's own
    const size_t coef_chunk = info0_.coef_count * sizeof(int16_t) * (size_t)C;
    const size_t oring_bytes = where == HVC_MEM_HOST ? form.out_bytes * (size_t)C : 0;

    guard_.emplace(c->device);
    if (!guard_->ok) return fail_hip(c, hipErrorInvalidDevice);
    if ((r = pipeline_events(c))) return r;
    for (int i = 0; i < NB; i++)
        for (int k = 0; k < 3; k++)
            HIPCHK(c, c->ev_et[i][k].ensure()); // per-slot stage timers
    if ((r = ring_ensure(c, reader_rings(c), {L_.ecs_bytes, L_.ecs_bytes, meta_bytes, meta_bytes, ftabs_bytes, ftabs_bytes}))) return r;
    if ((r = ring_ensure(c, coef_rings(c), {coef_chunk, coef_chunk}))) return r; // the coefficient ring of the host-decoder pipeline is reused
    if ((r = ring_ensure(c, out_rings(c), {oring_bytes}))) return r;
    // The reader of chunk k runs on rd_stream[k % NRD] with its own per-subsequence state, the block stage of all
    // chunks on c->stream: the last synchronisation rounds of a chunk (a handful of wavefronts chasing the few
    // stretches that are slow to synchronise, each round a full kernel's latency) overlap with the next chunk's
    // first ones, which fill the GPU.
    static_assert(hvc_ctx::RING <= 3, "ev_rd");
    if (where == HVC_MEM_HOST) HIPCHK(c, c->down_stream.ensure());
    if (!c->rd_stream[0]) {
        // two streams of the same priority can end up on one hardware queue (they did: no overlap at all);
        // streams of different priorities never share one
        int least = 0, greatest = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(c, c->rd_stream[0].ensure(least));
        HIPCHK(c, c->rd_stream[1].ensure(greatest));
        HIPCHK(c, c->rd_stream[2].ensure((least + greatest) / 2));
    }
    for (int i = 0; i < NB; i++)
        HIPCHK(c, c->ev_rd[i].ensure());
    state_bytes_ = (HVC_HD_STATE_BYTES(L_.state_subs) + 255) & ~(size_t)255;
    if ((r = grow(c, c->gd_state, NRD * state_bytes_))) return r;
    if ((r = grow(c, c->gd_fcnt, (size_t)NRD * HVC_HD_LIST_N * CU * sizeof(unsigned)))) return r;
    dcd_elems_ = (CU * G_.blocks_per_frame + 127) & ~(size_t)127;
    if ((r = grow(c, c->gd_dcd, NRD * dcd_elems_ * sizeof(int16_t)))) return r;
    // The DC values go from the reader's DC pass to the block stage through a compact array, one per ring slot (a
    // chunk's block stage may still read it while the next chunk's DC pass runs), instead of 2 bytes into each
    // 128-byte record -- unless a diagnostic kernel selection asks for the A/B alternates, which read the records.
    dc_compact_ = c->decode_kernel == 0 || c->decode_kernel == 2;
    dcv_fs_ = info0_.coef_count / 64; // (a tight record: whole blocks)
    dcv_elems_ = ((size_t)C * dcv_fs_ + 127) & ~(size_t)127;
    if (dc_compact_ && (r = grow(c, c->gd_dcv, (size_t)NB * dcv_elems_ * sizeof(int16_t)))) return r;
    if ((r = gd_upload_tables(c, tables0_, G_, c->stream))) return r;
    // A chunk whose files all carry the first file's tables (and those fit two slots) runs on the LDS-table kernels;
    // any other chunk in PF mode (hvc_hdec.h): per-frame tables in device memory, record 0 of every ring slot = the
    // first file's, record 1 + f = frame f's own (written by the worker that unstuffs the file).
    uniform_ok_ = G_.spec != nullptr;
    pf_fits_ = (unsigned long long)C * info0_.coef_count < (1ull << 35); // hvc::hd_write2_fits for a full chunk
    if (!uniform_ok_ && !pf_fits_) return HVC_OK;
    // tables with overflow prefixes (hvc_hdec.h HVC_HD_OVF) need the fast write pass, which a chunk this size may not fit
    if (!pf_fits_ && hvc::tables_use_overflow(tables0_, G_.n_comp)) return HVC_OK;
    for (int i = 0; i < NB; i++) hvc::make_frame_tabs(tables0_, G_.n_comp, *c->gp_h_ftabs[i].as<hvc::HdFrameTabs>());
    frame_pf_.assign((size_t)n_frames, 0);
    chunk_host_.assign((size_t)n_chunks_, 0);
    ecs_size_.assign((size_t)n_frames, 0);
    if (ipf > 1) {
        try {
            unit_off_.resize((size_t)n_frames * ipf);
            unit_len_.resize((size_t)n_frames * ipf);
        } catch (const std::bad_alloc &) {
            return HVC_E_OUT_OF_MEMORY;
        }
    }
    *host_pipeline = false;
    return HVC_OK;
}

int UniformGpuReader::prepare(int f, std::mutex &mu) {
    const int C = (int)L_.C, k = f / C, slot = k % hvc_ctx::RING;
    const unsigned ipf = units_.ipf;
    hvc::HdTables t;
    hvc_jpeg_info fi;
    int e = hvc_jpeg_read_header(jpegs_[f], sizes_[f], &fi);
    if (!e && (!same_geometry(fi, info0_) || fi.n_qtabs != info0_.n_qtabs || std::memcmp(fi.qtabs, info0_.qtabs, sizeof fi.qtabs)))
        e = HVC_E_INVALID_ARG; // a batch shares one geometry and one set of quantiser tables
    bool ok = false;
    uint8_t *dst = c_->gp_h_ecs[slot].as<uint8_t>() + L_.file_at((size_t)(f - k * C)); // unstuffed straight into the pinned slot
    size_t got = 0;
    if (!e && ipf > 1) { // (every interval's slot is zero-filled behind its bytes as it is written)
        hvc::RstUnits ru{units_.interval, ipf, unit_off_.data() + (size_t)f * ipf, unit_len_.data() + (size_t)f * ipf};
        e = hvc::prepare_gpu_decode_to(jpegs_[f], sizes_[f], &fi, t, dst, L_.file_cap(), &got, ok, &ru);
    } else if (!e) {
        e = hvc::prepare_gpu_decode_to(jpegs_[f], sizes_[f], &fi, t, dst, L_.file_cap(), &got, ok);
    }
    const bool own_tables = !e && ok && std::memcmp(&t, &tables0_, sizeof t) != 0;
    const bool unfit = !e && (!ok || (own_tables && !pf_fits_) || (!pf_fits_ && ok && hvc::tables_use_overflow(t, info0_.n_comp)));
    if (own_tables && !unfit) { // its own Huffman tables: a record of its own
        hvc::make_frame_tabs(t, info0_.n_comp, (c_->gp_h_ftabs[slot].as<hvc::HdFrameTabs>())[1 + (f - k * C)]);
        frame_pf_[(size_t)f] = 1;
    }
    if (!e && !unfit) {
        if (ipf == 1) {
            const size_t used = hvc::hd_file_subs(got) * hvc::HD_SB + 16; // this frame's subsequences + overshoot
            std::memset(dst + got, 0, used - got);
        }
        ecs_size_[(size_t)f] = (unsigned)got;
    }
    if (unfit) {
        std::lock_guard<std::mutex> lk(mu);
        chunk_host_[(size_t)k] = 1;
    }
    return e;
}

hipError_t UniformGpuReader::enqueue(int k, Chunk &out) {
    hvc_ctx *c = c_;
    const hvc::HdChunkLayout &L = L_;
    const int slot = k % hvc_ctx::RING, first = first_of(k), cnt = count_of(k);
    const unsigned ipf = units_.ipf;
    // the chunk's index arrays (frame_of: filled on the GPU)
    unsigned *hm = c->gp_h_meta[slot].as<unsigned>(), *dm = c->gp_d_meta[slot].as<unsigned>();
    const hvc::HdChunkFill fill = hvc::hd_chunk_fill(L, hm, cnt, ecs_size_.data() + first, ipf > 1 ? unit_off_.data() + (size_t)first * ipf : nullptr,
                                                     ipf > 1 ? unit_len_.data() + (size_t)first * ipf : nullptr, frame_pf_.data() + first);
    for (int f = 0; f < cnt; f++) ecs_total_ += ecs_size_[(size_t)(first + f)];
    const bool pf = !uniform_ok_ || fill.own_tables;
    hvc::HdParams P = G_;
    P.n_frames = cnt * (int)ipf;
    P.total_sub = fill.subs;
    P.ecs = c->gp_d_ecs[slot].as<const uint8_t>();
    P.ecs_off = dm + L.ecs_off;
    P.sub_off = dm + L.sub_off;
    P.frame_of = dm + L.frame_of;
    if (pf) // work lists per frame (k_hd_sync_pf) where that pays
        gd_params_pf(P, c->gp_d_ftabs[slot].as<const hvc::HdFrameTabs>(), dm + L.tabset_of,
                     gd_lists_per_frame(fill.subs, cnt) ? c->gd_fcnt.as<unsigned>() + (size_t)(k % NRD) * HVC_HD_LIST_N * L.CU : nullptr, (unsigned)L.nsub_max);
    P.frame_blocks = dm + L.frame_blocks;
    P.changed = dm + L.changed;
    P.status = dm + L.status;
    P.coefs = c->d_ring[slot].as<int16_t>();
    P.coef_fs = info0_.coef_count;
    gd_carve_state(P, c->gd_state.as<char>() + (size_t)(k % NRD) * state_bytes_, L.state_subs);
    P.dcd = c->gd_dcd.as<int16_t>() + (size_t)(k % NRD) * dcd_elems_;
    P.dc_plane = dc_compact_ ? c->gd_dcv.as<int16_t>() + (size_t)slot * dcv_elems_ : nullptr;
    P.dc_fs = dcv_fs_;
    hipStream_t rs = c->rd_stream[k % NRD];
    hipError_t he = hipEventRecord(c->ev_et[slot][0], c->copy_stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(c->gp_d_ecs[slot].p, c->gp_h_ecs[slot].p, L.file_at((size_t)cnt), hipMemcpyHostToDevice, c->copy_stream); // (the chunk's cnt files)
    if (he == hipSuccess)
        he = hipMemcpyAsync(dm, hm, L.upload_words * sizeof(unsigned), hipMemcpyHostToDevice, c->copy_stream);
    if (he == hipSuccess && pf) // the tables of the chunk's frames (36 KB a frame against ~1 MB of segment)
        he = hipMemcpyAsync(c->gp_d_ftabs[slot].p, c->gp_h_ftabs[slot].p, ((size_t)cnt + 1) * sizeof(hvc::HdFrameTabs),
                            hipMemcpyHostToDevice, c->copy_stream);
    if (he == hipSuccess) he = hipEventRecord(c->ev_h2d[slot], c->copy_stream);
    // (the slot's records and index arrays are free: the caller's verdict waited for chunk k - RING's block stage)
    if (he == hipSuccess) he = hipStreamWaitEvent(rs, c->ev_h2d[slot], 0);
    if (he == hipSuccess) he = hipEventRecord(c->ev_et[slot][1], rs);
    if (he == hipSuccess) he = gd_enqueue(P, 4, rs);
    if (he == hipSuccess) // changed + status -> the pinned copy of the index arrays
        he = hipMemcpyAsync(hm + L.changed, P.changed, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, rs);
    if (he == hipSuccess) he = hipEventRecord(c->ev_rd[slot], rs);
    if (he == hipSuccess) he = hipStreamWaitEvent(c->stream, c->ev_rd[slot], 0);
    out = {P.coefs, P.dc_plane, P.dc_fs};
    return he;
}

void UniformGpuReader::verdict(int k) {
    const int slot = k % hvc_ctx::RING;
    const unsigned *hm = c_->gp_h_meta[slot].as<const unsigned>();
    if (gd_unsettled(hm[L_.changed], 4) || hm[L_.status]) chunk_host_[(size_t)k] = 1; // not settled / the model raises / truncated: what was decoded is redone
    float ms = 0; // stage times of the chunk that just finished (read late so that nothing waits for them)
    if (hipEventElapsedTime(&ms, c_->ev_et[slot][0], c_->ev_h2d[slot]) == hipSuccess) h2d_ms_ += ms;
    if (hipEventElapsedTime(&ms, c_->ev_et[slot][1], c_->ev_et[slot][2]) == hipSuccess) k_ms_ += ms;
}

int ChunkDownloader::start(hvc_ctx *c, const UniformGpuReader &rd, uint8_t *pixels, size_t pixel_fs, size_t out_bytes) {
    return c->pool.submit([this, c, &rd, pixels, pixel_fs, out_bytes] {
        std::mutex &mu = feed_->mutex();
        std::condition_variable &cv = feed_->cv();
        (void)pin_to_ctx_cpus(c);
        if (hipSetDevice(c->device) != hipSuccess) { err_.store((int)hipErrorInvalidDevice); return; }
        for (int k = 0; k < rd.n_chunks(); k++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stage_done_.load() > k || abort_.load(); });
            }
            if (abort_.load()) return;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (skipped_[(size_t)k]) { // nothing was decoded here: the host-reader pipeline fills it in later
                    downloaded_[(size_t)k] = 1;
                    cv.notify_all();
                    continue;
                }
            }
            const int slot = k % hvc_ctx::RING;
            hipError_t e = hipStreamWaitEvent(c->down_stream, c->ev_et[slot][2], 0);
            if (e == hipSuccess)
                e = hipMemcpy2DAsync(pixels + (size_t)rd.first_of(k) * pixel_fs, pixel_fs, c->d_oring[slot].p, out_bytes, out_bytes,
                                     (size_t)rd.count_of(k), hipMemcpyDeviceToHost, c->down_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->down_stream);
            if (e != hipSuccess) err_.store((int)e);
            std::lock_guard<std::mutex> lk(mu);
            downloaded_[(size_t)k] = 1;
            cv.notify_all();
            if (e != hipSuccess) return;
        }
    }, 1);
}

void ChunkDownloader::hand_over(int k, bool skipped) {
    std::lock_guard<std::mutex> lk(feed_->mutex());
    if (skipped) {
        skipped_[(size_t)k] = 1;
        feed_->release_locked(k);
    }
    stage_done_.store(k + 1);
    feed_->cv().notify_all();
}

hipError_t ChunkDownloader::wait_downloaded(int k) {
    std::unique_lock<std::mutex> lk(feed_->mutex());
    feed_->cv().wait(lk, [&] { return downloaded_[(size_t)k] != 0 || err_.load(); });
    return (hipError_t)err_.load();
}

// ---------------------------------------------------------------------------
// BASELINE config 3 with the Huffman reader on the GPU as well: host threads only parse headers and
// unstuff the entropy-coded segments into a pinned ring; hipMemcpyAsync (copy stream) brings ~1 MB per
// frame to the device, where the self-synchronising decoder (hvc_hdec.hip) writes the coefficient
// records that the block stage reads.  Anything the GPU decoder hands back (unusual tables, streams the
// model treats specially, a chunk that does not settle in four launches) restarts the call on the
// host-decoder pipeline, so results and error codes are always the host decoder's.
// form: what every frame's records become (OutputForm, hvc_ctx.h); a scaled chunk's block stage reads the chunk's compact DC array.
int decode_batch_gpu(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads, int frames_per_chunk,
                     uint8_t *pixels, size_t pixel_fs, int where, hvc_batch_stats *stats, OutputForm form) {
    if (!c || !jpegs || !sizes || !pixels || n_frames < 0) return HVC_E_INVALID_ARG;
    if (!form.known()) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_frames == 0) return HVC_OK;
    hvc::RestartScope honour(c->honour_restart);
    constexpr int NB = hvc_ctx::RING;
    // (everything a pool task touches is declared BEFORE the feed, whose scope waits for the tasks: destroyed after it has waited)
    UniformGpuReader rd;
    bool host_pipeline = false;
    int r = rd.begin(c, jpegs, sizes, n_frames, &frames_per_chunk, where, pixel_fs, form, &host_pipeline);
    if (r) return r;
    if (host_pipeline) return decode_batch_impl(c, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels, pixel_fs, where, stats, form);
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    const int C = frames_per_chunk, n_chunks = rd.n_chunks();
    std::atomic<long long> prep_ns{0};
    ChunkDownloader down(n_chunks);
    const auto wall0 = std::chrono::steady_clock::now();
    if ((r = pool_ready(c, threads, where == HVC_MEM_HOST ? 1 : 0))) return r;
    hvc::ChunkFeed feed(c->pool, n_chunks, NB, [&] { down.abort(); });
    down.attach(feed);
    std::mutex &mu = feed.mutex(); // ... which also guards the reader's marks of chunks for the host reader and the downloader's state
    // workers: header parse, table check, unstuffing into the pinned segment ring
    auto worker = [&]() {
        if (!pin_to_ctx_cpus(c)) feed.raise(HVC_E_INVALID_ARG); // hvc_set_host_cpus
        hvc::RestartScope honour(c->honour_restart);
        for (;;) {
            const int f = feed.claim();
            if (f >= n_frames || feed.error()) return;
            const int k = f / C;
            if (!feed.wait_slot(k)) return;
            const auto t0 = std::chrono::steady_clock::now();
            const int e = rd.prepare(f, mu);
            prep_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            feed.report(k, 1, e);
        }
    };
    if (where == HVC_MEM_HOST && (r = down.start(c, rd, pixels, pixel_fs, form.out_bytes))) return feed.finish(r); // (wakes and waits for whatever was queued)
    if ((r = feed.start(threads, worker))) return r;

    int rc = HVC_OK;
    hipStream_t compute = c->stream;
    DecodeOpts block_stage(c); // (the chunks' launches take no entry of the profiling ring -- but a scaled chunk's: hvc_jpeg_decode_batch_scaled)
    block_stage.profile = form.chunk_profile(c);
    int pending_release = -1; // the chunk whose pinned segment slot is handed on once its upload has finished
    auto release_after_upload = [&](int k) -> hipError_t {
        const hipError_t he = wait_event(c->ev_h2d[k % NB]);
        if (he != hipSuccess) return he;
        feed.release(k);
        return hipSuccess;
    };
    try {
    for (int it = 0; it < n_chunks + NB && rc == HVC_OK; it++) {
        // verdict on chunk it - NB's slot before it is overwritten (and on the last chunks at the end)
        const int v = it - NB;
        if (v >= 0 && !down.skipped(v)) { // the slot's frames have left the device / its block stage is through
            const hipError_t he = where == HVC_MEM_HOST ? down.wait_downloaded(v) : wait_event(c->ev_kern[v % NB]);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            rd.verdict(v);
        }
        if (it >= n_chunks) continue;
        const int k = it, slot = k % NB, first = rd.first_of(k), cnt = rd.count_of(k);
        if ((rc = feed.wait_chunk(k, cnt))) break;
        bool skip;
        {
            std::lock_guard<std::mutex> lk(mu);
            skip = rd.host_chunk(k);
        }
        if (skip) { // no GPU work for this chunk; its pinned slot goes to chunk k + NB, the downloader moves on
            if (pending_release >= 0) { // (slots are released in order: the previous chunk's upload first)
                const hipError_t he = release_after_upload(pending_release);
                pending_release = -1;
                if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            }
            down.hand_over(k, true);
            continue;
        }
        UniformGpuReader::Chunk ch;
        hipError_t he = rd.enqueue(k, ch);
        if (he != hipSuccess) { rc = fail_hip(c, he); break; }
        uint8_t *dst = where == HVC_MEM_DEVICE ? pixels + (size_t)first * pixel_fs : c->d_oring[slot].as<uint8_t>();
        const size_t dst_fs = where == HVC_MEM_DEVICE ? pixel_fs : form.out_bytes;
        block_stage.dc_plane = ch.dc_plane;
        block_stage.dc_fs = ch.dc_fs;
        rc = form.run(c, ch.coefs, cnt, dst, dst_fs, HVC_MEM_DEVICE, block_stage);
        if (rc) break;
        he = hipEventRecord(c->ev_et[slot][2], compute);
        if (he == hipSuccess && where == HVC_MEM_HOST) down.hand_over(k, false); // the downloader takes over
        if (he == hipSuccess && where != HVC_MEM_HOST) he = hipEventRecord(c->ev_kern[slot], compute);
        // Hand the PREVIOUS chunk's pinned segment slot to chunk k - 1 + NB now that its upload is through -- this
        // chunk's upload is queued behind it, so the copy engine goes from one to the next while this thread waits
        // here, prepares the next chunk's index arrays and enqueues its launches (waiting for a chunk's own upload
        // at this point left the engine idle for as long as that took: 0.5 - 2 ms in every 4.8).
        if (he == hipSuccess && pending_release >= 0) he = release_after_upload(pending_release);
        if (he != hipSuccess) { rc = fail_hip(c, he); break; }
        pending_release = k;
    }
    if (rc == HVC_OK && pending_release >= 0) {
        const hipError_t he = release_after_upload(pending_release);
        if (he != hipSuccess) rc = fail_hip(c, he);
    }
    } catch (...) {
        rc = hvc::exception_code();
    }
    rc = feed.finish(rc); // (after a complete run the downloader has finished: the last verdicts waited for its last chunks)
    for (int i = 0; i < 3; i++) (void)hipStreamSynchronize(c->rd_stream[i]);
    (void)hipStreamSynchronize(compute);
    (void)hipStreamSynchronize(c->copy_stream);
    // everything has drained: the chunks left to the host reader (skipped above, or found out at the verdict) are redone by
    // the host-reader pipeline -- chunk by chunk, not the whole call
    double host_entropy_ms = 0;
    for (int k = 0; k < n_chunks && rc == HVC_OK; k++)
        if (rd.host_chunk(k)) {
            const int first = rd.first_of(k);
            hvc_batch_stats hs;
            rc = decode_batch_impl(c, jpegs + first, sizes + first, rd.count_of(k), threads, 0, pixels + (size_t)first * pixel_fs, pixel_fs,
                                   where, &hs, form);
            host_entropy_ms += hs.entropy_ms_sum;
        }
    if (stats) {
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        stats->entropy_ms_sum = host_entropy_ms; // host entropy decoding: only for the chunks that fell to the host reader
        stats->host_prep_ms_sum = (double)prep_ns.load() * 1e-6;
        stats->h2d_ms_sum = rd.h2d_ms();
        stats->kernel_ms_sum = rd.kernel_ms();
        stats->chunks = n_chunks;
        stats->threads = threads;
        stats->frames_per_chunk = C;
        stats->coef_bytes = rd.ecs_total(); // bytes uploaded: the unstuffed segments
    }
    return rc;
}

int hvc_jpeg_decode_batch_gpu(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads,
                              int frames_per_chunk, uint8_t *pixels, size_t pixel_fs, int where, int yuv444,
                              hvc_batch_stats *stats) try {
    if (c && yuv444 && c->arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (no RTL form of the fused path)
    return decode_batch_gpu(c, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels, pixel_fs, where, stats,
                            OutputForm(yuv444 ? OutputForm::YUV444 : OutputForm::PLANES));
} HVC_ABI_CATCH
