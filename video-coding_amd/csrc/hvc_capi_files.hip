// hvc_capi_files.hip -- the encoder's back end behind the C ABI: the GPU Huffman coder (hvc_huffman_encode_frames) and
// BASELINE's configuration 5 end to end, raw frames in, JPEG files out (hvc_jpeg_encode_batch, hvc_jpeg_encode_batch_gpu).
#include "hvc_ctx.h"
#include "hvc_mixed_rgb_plan.h"

// ---------------------------------------------------------------------------
// Encoder back end on the GPU: RLE + Huffman + byte stuffing of coefficient records (hvc_huff.hip)

// the default code tables on the device, once per context (hvc_huff.hip reads them through HuffParams::tables).  The
// context holds them only once the copy has succeeded: a failed upload is tried again by the next call.
int upload_enc_tables(hvc_ctx *c) {
    if (c->hd_tables) return HVC_OK;
    uint32_t t[2][16 + 256];
    hvc::default_enc_tables(t);
    Buf d;
    if (grow(c, d, sizeof t, GROW_EXACT)) return HVC_E_HIP; // (last_hip says why)
    HIPCHK(c, hipMemcpy(d.p, t, sizeof t, hipMemcpyHostToDevice));
    c->hd_tables.adopt(d);
    return HVC_OK;
}

int hvc_huffman_code_tables(hvc_ctx *c, int table_set, int where, uint32_t *codes) try {
    if (!codes || table_set < 0 || table_set > 1) return HVC_E_INVALID_ARG;
    if (where == HVC_MEM_HOST) {
        uint32_t t[2][16 + 256];
        hvc::default_enc_tables(t);
        std::memcpy(codes, t[table_set], sizeof t[0]);
        return HVC_OK;
    }
    if (where != HVC_MEM_DEVICE || !c) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    int r = upload_enc_tables(c);
    if (r) return r;
    HIPCHK(c, hipMemcpy(codes, c->hd_tables.as<unsigned>() + (size_t)table_set * (16 + 256), (16 + 256) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HVC_OK;
} HVC_ABI_CATCH

// Geometry + scratch of one call.  `out` / `offsets` are device pointers (the caller's, or NULL = scratch
// inside ctx, see huffman_scratch_out).
int huffman_prepare(hvc_ctx *c, const hvc_jpeg_info *info, const int16_t *d_coefs, size_t coef_fs, int n_frames, uint8_t *d_out,
                    size_t out_cap, unsigned long long *d_offsets, hvc::HuffParams &P, bool optimised, int restart) {
    int r = hvc_jpeg_encoder_check(info);
    if (r) return r;
    std::memset(&P, 0, sizeof P);
    const hvc_jpeg_component &c0 = info->comp[0];
    P.mbs_wide = c0.decoded_width / (8 * c0.hscale);
    P.mbs_high = c0.decoded_height / (8 * c0.vscale);
    int tile = 0, base = 0;
    for (int i = 0; i < 3; i++) {
        hvc::HuffComp &K = P.comp[i];
        K.bw = info->layout[i].blocks_w;
        K.bh = info->layout[i].blocks_h;
        K.nblk = K.bw * K.bh;
        K.tile0 = tile;
        K.h = info->comp[i].hscale;
        K.v = info->comp[i].vscale;
        K.mcu_base = base;
        K.table = info->comp[i].dc_table ? 1 : 0;
        K.coef_off = info->layout[i].coef_offset;
        tile += (K.nblk + 255) / 256;
        base += K.h * K.v;
    }
    P.tiles_per_frame = tile;
    P.blocks_per_mcu = base;
    // a table set that no component selects has no symbol to fit a table to: refused as hvc_huffman_optimal_tables refuses
    // it (k_huff_build would look for the reserved symbol's code length in a table without one)
    if (optimised && P.comp[0].table == P.comp[1].table && P.comp[1].table == P.comp[2].table) return HVC_E_INVALID_ARG;
    const unsigned long long bpf = (unsigned long long)P.mbs_wide * P.mbs_high * base;
    // restart intervals: a scan of a single interval (Ri >= MCUs) holds no marker and is the plain segment
    const unsigned long long mcus = (unsigned long long)P.mbs_wide * P.mbs_high;
    const unsigned long long n_ivl = restart > 0 && (unsigned long long)restart < mcus ? (mcus + restart - 1) / restart : 0;
    // 32-bit bit offsets per frame (up to 7 pad bits per interval on top of the fields)
    if (bpf == 0 || bpf * 64ull * 27ull + 7ull * n_ivl >= (1ull << 32)) return HVC_E_TOO_LARGE;
    P.restart = n_ivl ? restart : 0;
    P.n_intervals = (unsigned)n_ivl;
    P.blocks_per_frame = (unsigned)bpf;
    P.n_frames = n_frames;
    P.coefs = d_coefs;
    P.coef_fs = coef_fs;
    // worst case per block: 64 fields of 27 bits (216 bytes); the segment buffer is sized for it
    // (+ one pad byte per interval)
    const size_t words = ((size_t)bpf * 216 + (size_t)n_ivl + 3) / 4 + 2;
    P.bitbuf_words = (words + 15) / 16 * 16;
    P.ff_stride = P.bitbuf_words / 16;
    const size_t nf = (size_t)n_frames;
    if (optimised) { // per frame: counts, code tables (both HUFF_TABLE_WORDS words), four specs
        const size_t words = nf * hvc::HUFF_TABLE_WORDS;
        if ((r = grow(c, c->hd_opt, 2 * words * sizeof(unsigned) + nf * 4 * sizeof(hvc_huff_spec)))) return r;
        P.hist = c->hd_opt.as<unsigned>();
        P.opt_tables = P.hist + words;
        P.specs = (hvc_huff_spec *)(P.opt_tables + words);
        P.tables = P.opt_tables;
        P.table_stride = hvc::HUFF_TABLE_WORDS;
    } else {
        if ((r = upload_enc_tables(c))) return r;
        P.tables = c->hd_tables.as<unsigned>();
    }
    if ((r = grow(c, c->hd_lens, nf * bpf * sizeof(unsigned)))) return r;
    if ((r = grow(c, c->hd_meta, (4 * nf + 2 * (nf + 1) + 4) * sizeof(unsigned) + 64))) return r;
    if ((r = grow(c, c->hd_bitbuf, nf * P.bitbuf_words * sizeof(unsigned)))) return r;
    if ((r = grow(c, c->hd_ff, nf * P.ff_stride * sizeof(unsigned)))) return r;
    P.lens = c->hd_lens.as<unsigned>();
    unsigned *m = c->hd_meta.as<unsigned>();
    P.status = m;
    P.frame_bits = m + 4;
    P.frame_bytes = P.frame_bits + nf;
    P.frame_pieces = P.frame_bytes + nf;
    P.frame_ff = P.frame_pieces + nf;
    unsigned long long *scratch_off = (unsigned long long *)(((uintptr_t)(P.frame_ff + nf) + 7) & ~(uintptr_t)7);
    P.bitbuf = c->hd_bitbuf.as<unsigned>();
    P.ff = c->hd_ff.as<unsigned>();
    if (n_ivl) {
        if ((r = grow(c, c->hd_ivl, nf * (size_t)n_ivl * sizeof(unsigned)))) return r;
        P.ivl = c->hd_ivl.as<unsigned>();
    }
    P.out_offsets = d_offsets ? d_offsets : scratch_off;
    P.out = d_out;
    P.out_cap = out_cap;
    return HVC_OK;
}

int hvc_jpeg_header(const hvc_jpeg_info *info, uint8_t *out, size_t cap, size_t *len) try {
    if (!info || !len || info->n_comp != 3) return HVC_E_INVALID_ARG;
    std::vector<uint8_t> o;
    hvc::jpeg_header_bytes(info, o);
    *len = o.size();
    if (!out || cap < o.size()) return HVC_E_INVALID_ARG;
    std::memcpy(out, o.data(), o.size());
    return HVC_OK;
} HVC_ABI_CATCH

// specs != nullptr: each frame's own optimal tables, its four specs into specs[4 f .. 4 f + 3] (host memory)
static int huffman_encode_frames_impl(hvc_ctx *c, const hvc_jpeg_info *info, const int16_t *coefs, size_t coef_fs, int n_frames,
                                      uint8_t *out, size_t out_cap, uint64_t *offsets, hvc_huff_spec *specs, int where,
                                      int restart = 0) {
    if (!c || !info || !coefs || !out || !offsets || n_frames < 0 || info->n_comp != 3) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    if (n_frames == 0) {
        if (where == HVC_MEM_HOST) offsets[0] = 0;
        return HVC_OK;
    }
    if (n_frames > 65535) return HVC_E_TOO_LARGE;
    if (n_frames > 1 && coef_fs < info->coef_count) return HVC_E_INVALID_ARG;
    if (coef_fs & 7) return HVC_E_ALIGNMENT;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    hvc::HuffParams P;
    int r;
    unsigned status = 0;
    if (where == HVC_MEM_DEVICE) {
        if (((uintptr_t)coefs & 15) || ((uintptr_t)offsets & 7)) return HVC_E_ALIGNMENT;
        if ((r = huffman_prepare(c, info, coefs, coef_fs, n_frames, out, out_cap, (unsigned long long *)offsets, P, specs != nullptr, restart))) return r;
        HIPCHK(c, hvc::launch_huffman_encode(P, c->stream));
        HIPCHK(c, hipMemcpyAsync(&status, P.status, sizeof status, hipMemcpyDeviceToHost, c->stream));
        if (specs)
            HIPCHK(c, hipMemcpyAsync(specs, P.specs, (size_t)n_frames * 4 * sizeof(hvc_huff_spec), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        const size_t cbytes = ((size_t)(n_frames - 1) * coef_fs + info->coef_count) * sizeof(int16_t);
        if ((r = grow(c, c->d_in, cbytes))) return r;
        if ((r = grow(c, c->hd_out, out_cap))) return r;
        if ((r = huffman_prepare(c, info, c->d_in.as<const int16_t>(), coef_fs, n_frames, c->hd_out.as<uint8_t>(), out_cap, nullptr, P,
                                   specs != nullptr, restart)))
            return r;
        HIPCHK(c, hipMemcpyAsync(c->d_in.p, coefs, cbytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hvc::launch_huffman_encode(P, c->stream));
        HIPCHK(c, hipMemcpyAsync(&status, P.status, sizeof status, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(offsets, P.out_offsets, (size_t)(n_frames + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                 c->stream));
        if (specs)
            HIPCHK(c, hipMemcpyAsync(specs, P.specs, (size_t)n_frames * 4 * sizeof(hvc_huff_spec), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!(status & 7u) && offsets[n_frames] <= out_cap)
            HIPCHK(c, hipMemcpy(out, c->hd_out.p, (size_t)offsets[n_frames], hipMemcpyDeviceToHost));
    }
    if (status & 1u) return HVC_E_RANGE;       // a value the tables have no code for (DC category > 11, AC size > 10)
    if (status & 6u) return HVC_E_INVALID_ARG; // out_cap too small
    return HVC_OK;
}

int hvc_huffman_encode_frames(hvc_ctx *c, const hvc_jpeg_info *info, const int16_t *coefs, size_t coef_fs, int n_frames,
                              uint8_t *out, size_t out_cap, uint64_t *offsets, int where) try {
    return huffman_encode_frames_impl(c, info, coefs, coef_fs, n_frames, out, out_cap, offsets, nullptr, where);
} HVC_ABI_CATCH

int hvc_huffman_encode_frames_optimised(hvc_ctx *c, const hvc_jpeg_info *info, const int16_t *coefs, size_t coef_fs,
                                        int n_frames, uint8_t *out, size_t out_cap, uint64_t *offsets, hvc_huff_spec *specs,
                                        int where) try {
    if (!specs) return HVC_E_INVALID_ARG;
    return huffman_encode_frames_impl(c, info, coefs, coef_fs, n_frames, out, out_cap, offsets, specs, where);
} HVC_ABI_CATCH

int hvc_huffman_encode_frames_restart(hvc_ctx *c, const hvc_jpeg_info *info, const int16_t *coefs, size_t coef_fs, int n_frames,
                                      int restart_interval, int tables, uint8_t *out, size_t out_cap, uint64_t *offsets,
                                      hvc_huff_spec *specs, int where) try {
    if (restart_interval < 0 || restart_interval > 65535) return HVC_E_INVALID_ARG;
    if (tables != HVC_HUFF_DEFAULT && tables != HVC_HUFF_OPTIMISED) return HVC_E_INVALID_ARG;
    if (tables == HVC_HUFF_OPTIMISED && !specs) return HVC_E_INVALID_ARG;
    return huffman_encode_frames_impl(c, info, coefs, coef_fs, n_frames, out, out_cap, offsets,
                                      tables == HVC_HUFF_OPTIMISED ? specs : nullptr, where, restart_interval);
} HVC_ABI_CATCH

// ---------------------------------------------------------------------------
// BASELINE config 5 end to end: raw frames in, JPEG files out.
//   host threads: Plane.blit_available into zero-padded planes (pinned ring)     encoder.ml:514-516
//   copy stream:  hipMemcpyAsync H2D                  compute stream: k_encode, then D2H of the coefficient records
//   host threads: write_headers + rle + write_bits + EOI per frame                encoder.ml:127-193, 371-418
// The orchestrating thread runs a three-stage software pipeline over chunks (pad k | GPU k-1 | entropy k-2).
// gpu_entropy = false: coefficient records come back to the host and host threads entropy-code them;
// gpu_entropy = true: the Huffman coder runs on the GPU too (hvc_huff.hip), only the packed segments come back
// and host threads just assemble header + segment + EOI.
static int encode_batch_impl(hvc_ctx *c, const uint8_t *const *frames, int n_frames, int width, int height, int chroma,
                             int quality, int threads, int frames_per_chunk, uint8_t *const *jpegs, const size_t *caps,
                             size_t *sizes, hvc_batch_stats *stats, bool gpu_entropy) {
    if (!c || !frames || !jpegs || !caps || !sizes || n_frames < 0) return HVC_E_INVALID_ARG;
    if (stats) std::memset(stats, 0, sizeof *stats);
    hvc_jpeg_info info;
    int r = hvc_jpeg_encoder_layout(width, height, chroma, quality, &info);
    if (r) return r;
    if ((r = hvc_jpeg_encoder_check(&info))) return r; // the model raises for this geometry
    if (n_frames == 0) return HVC_OK;
    for (int f = 0; f < n_frames; f++)
        if (!frames[f] || !jpegs[f]) return HVC_E_INVALID_ARG;
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    if (frames_per_chunk < 1) frames_per_chunk = 16;
    if (frames_per_chunk > n_frames) frames_per_chunk = n_frames;
    const int C = frames_per_chunk, NB = hvc_ctx::RING;
    const int n_chunks = (n_frames + C - 1) / C;
    const size_t pix_bytes = info.pixel_bytes, coef_bytes = info.coef_count * sizeof(int16_t);
    const size_t in_bytes = pix_bytes * (size_t)C, out_bytes = coef_bytes * (size_t)C;

    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    HIPCHK(c, c->copy_stream.ensure());
    HIPCHK(c, c->down_stream.ensure());
    for (int i = 0; i < NB; i++) {
        HIPCHK(c, c->ev_up[i].ensure());
        HIPCHK(c, c->ev_down[i].ensure());
        for (int k = 0; k < 3; k++)
            HIPCHK(c, c->ev_et[i][k].ensure());
        HIPCHK(c, c->ev_gpu[i].ensure());
    }
    std::vector<uint8_t> header_default;
    const bool opt = c->huff_tables == HVC_HUFF_OPTIMISED; // each file its own tables (hvc_set_huffman_tables)
    const int ri = c->restart_interval;                    // DRI + RSTn every ri MCUs (hvc_set_restart_interval)
    if (gpu_entropy && opt) { // per slot: the chunk's specs, pinned
        if ((r = ring_ensure(c, enc_spec_rings(c), {(size_t)C * 4 * sizeof(hvc_huff_spec)}))) return r;
    }
    if (gpu_entropy) {
        hvc::jpeg_header_bytes(&info, header_default, nullptr, ri);
        // per slot: packed segments on the device (capacity = the coefficient chunk: 2 bytes per sample, twice the raw
        // frames), and (C + 1) offsets + one status word, on the device and pinned
        const size_t off_bytes = ((size_t)C + 2) * sizeof(unsigned long long);
        if ((r = ring_ensure(c, enc_seg_rings(c), {out_bytes, off_bytes, off_bytes}))) return r;
    }
    if ((r = ring_ensure(c, enc_rings(c), {in_bytes, out_bytes, in_bytes, out_bytes}))) return r;

    struct Task {
        int kind, frame; // 0 = pad into the pinned pixel ring, 1 = entropy-code from the pinned coefficient ring
    };
    std::mutex mu;
    std::condition_variable cv_task, cv_done;
    std::deque<Task> queue;
    bool stop = false;
    std::atomic<int> error{0};
    std::vector<int> pads_done((size_t)n_chunks, 0), ent_done((size_t)n_chunks, 0);
    std::atomic<long long> pad_ns{0}, ent_ns{0};
    auto worker = [&]() {
        if (!pin_to_ctx_cpus(c)) error.store(HVC_E_INVALID_ARG); // hvc_set_host_cpus
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_task.wait(lk, [&] { return stop || !queue.empty(); });
                if (queue.empty()) return;
                t = queue.front();
                queue.pop_front();
            }
            const int f = t.frame, k = f / C, slot = k % NB;
            const auto t0 = std::chrono::steady_clock::now();
            int e = HVC_OK;
            if (error.load() == 0) try {
                if (t.kind == 0) {
                    // (the info's actual plane sizes are width x height and the chroma's by `chroma`: tests/test_mixed_encode_chunks.py)
                    // (hvc_set_encode_libjpeg: the replicating sibling, hvc_libjpeg_encode_plan.h)
                    (c->enc_libjpeg ? hvc::pad_frame_replicate : pad_frame)(info, frames[f], c->eh_in[slot].as<uint8_t>() + (size_t)(f - k * C) * pix_bytes);
                } else if (!gpu_entropy) {
                    const int16_t *cf = c->eh_out[slot].as<const int16_t>() + (size_t)(f - k * C) * info.coef_count;
                    e = opt ? hvc::entropy_encode_optimised(&info, cf, jpegs[f], caps[f], &sizes[f], ri)
                            : hvc::entropy_encode_file(&info, nullptr, cf, jpegs[f], caps[f], &sizes[f], ri);
                } else { // header + the frame's segment + EOI (complete_and_write_eoi, encoder.ml:507-510)
                    const unsigned long long *off = c->eh_off[slot].as<const unsigned long long>();
                    const int fi = f - k * C;
                    const size_t seg = (size_t)(off[fi + 1] - off[fi]);
                    std::vector<uint8_t> own; // optimised: the frame's own DHT bodies
                    if (opt) hvc::jpeg_header_bytes(&info, own, c->eh_specs[slot].as<const hvc_huff_spec>() + 4 * fi, ri);
                    const std::vector<uint8_t> &header = opt ? own : header_default;
                    sizes[f] = header.size() + seg + 2;
                    if (sizes[f] > caps[f]) {
                        e = HVC_E_INVALID_ARG;
                    } else {
                        std::memcpy(jpegs[f], header.data(), header.size());
                        std::memcpy(jpegs[f] + header.size(), c->eh_out[slot].as<const uint8_t>() + off[fi], seg);
                        jpegs[f][header.size() + seg] = 0xff;
                        jpegs[f][header.size() + seg + 1] = 0xd9;
                    }
                }
            } catch (...) { // (the counters below must move whatever happened: the orchestrator waits for them)
                e = hvc::exception_code();
            }
            const long long ns =
                std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            (t.kind == 0 ? pad_ns : ent_ns) += ns;
            std::lock_guard<std::mutex> lk(mu);
            if (e) error.store(e);
            (t.kind == 0 ? pads_done : ent_done)[(size_t)k]++;
            cv_done.notify_all();
        }
    };
    const auto wall0 = std::chrono::steady_clock::now();
    if ((r = pool_ready(c, threads))) return r;
    hvc::PoolScope scope(c->pool, [&] { // however this function is left: the workers drain the queue and return
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
        cv_task.notify_all();
    });
    if ((r = c->pool.submit(worker, threads))) return r;
    auto chunk_count = [&](int k) { return (k * C + C <= n_frames) ? C : n_frames - k * C; };
    auto submit = [&](int kind, int k) {
        std::lock_guard<std::mutex> lk(mu);
        for (int f = k * C; f < k * C + chunk_count(k); f++) queue.push_back(Task{kind, f});
        cv_task.notify_all();
    };
    auto wait_for = [&](std::vector<int> &done, int k) {
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return done[(size_t)k] == chunk_count(k); });
    };

    int rc = HVC_OK;
    double h2d_ms = 0, k_ms = 0, d2h_ms = 0;
    unsigned long long seg_bytes = 0;
    hipStream_t compute = c->stream;
    EncodeOpts block_stage(c); // (the chunks' launches take no entry of the profiling ring)
    block_stage.profile = false;
    block_stage.edges = &info; // (hvc_set_encode_libjpeg: the files' dummy blocks)
    try {
    for (int it = 0; it < n_chunks + 3 && rc == HVC_OK; it++) {
        // stage 1: pad chunk `it` (its pinned slot was uploaded and synchronised two iterations ago)
        if (it < n_chunks) submit(0, it);
        // stage 2: GPU work of chunk it - 1
        const int j = it - 1;
        if (j >= 0 && j < n_chunks) {
            const int slot = j % NB, cnt = chunk_count(j);
            wait_for(pads_done, j);
            // the slot's pinned buffers (coefficients, or offsets + segments) are free again once chunk j - NB
            // has been entropy-coded / assembled
            if (j >= NB) wait_for(ent_done, j - NB);
            hipError_t he = hipEventRecord(c->ev_et[slot][0], c->copy_stream);
            if (he == hipSuccess)
                he = hipMemcpyAsync(c->ed_in[slot].p, c->eh_in[slot].p, pix_bytes * (size_t)cnt, hipMemcpyHostToDevice,
                                    c->copy_stream);
            if (he == hipSuccess) he = hipEventRecord(c->ev_up[slot], c->copy_stream);
            if (he == hipSuccess) he = hipStreamWaitEvent(compute, c->ev_up[slot], 0);
            if (he == hipSuccess) he = hipEventRecord(c->ev_et[slot][1], compute);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            rc = encode_frames_impl(c, c->ed_in[slot].as<const uint8_t>(), pix_bytes, &info.qtabs[0][0], info.n_qtabs,
                                    info.layout, 3, cnt, c->ed_out[slot].as<int16_t>(), info.coef_count, HVC_MEM_DEVICE, block_stage);
            if (rc) break;
            if (!gpu_entropy) {
                he = hipEventRecord(c->ev_et[slot][2], compute);
                if (he == hipSuccess)
                    he = hipMemcpyAsync(c->eh_out[slot].p, c->ed_out[slot].p, coef_bytes * (size_t)cnt, hipMemcpyDeviceToHost,
                                        compute);
                if (he == hipSuccess) he = hipEventRecord(c->ev_down[slot], compute);
            } else {
                hvc::HuffParams HP;
                rc = huffman_prepare(c, &info, c->ed_out[slot].as<const int16_t>(), info.coef_count, cnt,
                                     c->ed_seg[slot].as<uint8_t>(), out_bytes, c->ed_off[slot].as<unsigned long long>(), HP, opt, ri);
                if (rc) break;
                he = hvc::launch_huffman_encode(HP, compute);
                if (he == hipSuccess) he = hipEventRecord(c->ev_et[slot][2], compute);
                // offsets, then the status word behind them (slot C + 1 of the pinned array)
                if (he == hipSuccess)
                    he = hipMemcpyAsync(c->eh_off[slot].p, c->ed_off[slot].p, ((size_t)cnt + 1) * sizeof(unsigned long long),
                                        hipMemcpyDeviceToHost, compute);
                if (he == hipSuccess)
                    he = hipMemcpyAsync(c->eh_off[slot].as<unsigned long long>() + C + 1, HP.status, sizeof(unsigned),
                                        hipMemcpyDeviceToHost, compute);
                if (he == hipSuccess && opt) // (the context's scratch: copied before the next chunk's coder reuses it)
                    he = hipMemcpyAsync(c->eh_specs[slot].p, HP.specs, (size_t)cnt * 4 * sizeof(hvc_huff_spec),
                                        hipMemcpyDeviceToHost, compute);
                if (he == hipSuccess) he = hipEventRecord(c->ev_gpu[slot], compute);
            }
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
        }
        // stage 3:
        //   host coder: wait for chunk it - 2's coefficients, hand them to the entropy threads
        //   GPU coder:  wait for chunk it - 2's offsets, then download exactly its packed segments -- on a
        //               stream of its own, so that the copy is not queued behind the next chunk's kernels
        const int e = it - 2;
        if (e >= 0 && e < n_chunks) {
            const int slot = e % NB;
            float ms = 0;
            if (!gpu_entropy) {
                hipError_t he = wait_event(c->ev_down[slot]);
                if (he != hipSuccess) { rc = fail_hip(c, he); break; }
                submit(1, e);
                if (hipEventElapsedTime(&ms, c->ev_et[slot][0], c->ev_up[slot]) == hipSuccess) h2d_ms += ms;
                if (hipEventElapsedTime(&ms, c->ev_et[slot][2], c->ev_down[slot]) == hipSuccess) d2h_ms += ms;
            } else {
                hipError_t he = wait_event(c->ev_gpu[slot]);
                if (he != hipSuccess) { rc = fail_hip(c, he); break; }
                if (hipEventElapsedTime(&ms, c->ev_et[slot][0], c->ev_up[slot]) == hipSuccess) h2d_ms += ms;
                const unsigned long long *off = c->eh_off[slot].as<const unsigned long long>();
                const int cnt = chunk_count(e);
                const unsigned status = (unsigned)off[C + 1];
                if (status & 1u) { rc = HVC_E_RANGE; break; }              // a value without a code
                if ((status & 6u) || off[cnt] > out_bytes) { rc = HVC_E_TOO_LARGE; break; } // > 2x the raw frames
                if (e >= NB) wait_for(ent_done, e - NB); // the pinned segment slot has been assembled
                he = hipEventRecord(c->ev_et[slot][0], c->down_stream);
                if (he == hipSuccess && off[cnt])
                    he = hipMemcpyAsync(c->eh_out[slot].p, c->ed_seg[slot].p, (size_t)off[cnt], hipMemcpyDeviceToHost,
                                        c->down_stream);
                if (he == hipSuccess) he = hipEventRecord(c->ev_down[slot], c->down_stream);
                if (he != hipSuccess) { rc = fail_hip(c, he); break; }
                seg_bytes += off[cnt];
            }
            if (hipEventElapsedTime(&ms, c->ev_et[slot][1], c->ev_et[slot][2]) == hipSuccess) k_ms += ms;
        }
        // stage 4 (GPU coder): assemble the files of chunk it - 3 once its segments have landed
        const int a = it - 3;
        if (gpu_entropy && a >= 0 && a < n_chunks) {
            const int slot = a % NB;
            hipError_t he = wait_event(c->ev_down[slot]);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            float ms = 0;
            if (hipEventElapsedTime(&ms, c->ev_et[slot][0], c->ev_down[slot]) == hipSuccess) d2h_ms += ms;
            submit(1, a);
        }
        if (error.load()) rc = error.load();
    }
    if (rc == HVC_OK)
        for (int k = 0; k < n_chunks; k++) wait_for(ent_done, k);
    } catch (...) {
        rc = hvc::exception_code();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        if (rc != HVC_OK) {
            error.store(rc);
            queue.clear();
        }
        stop = true;
        cv_task.notify_all();
    }
    {
        const int te = scope.finish();
        if (rc == HVC_OK && te) rc = te;
    }
    (void)hipStreamSynchronize(compute);
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->down_stream);
    if (rc == HVC_OK && error.load()) rc = error.load();
    if (stats) {
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        stats->entropy_ms_sum = (double)ent_ns.load() * 1e-6;
        stats->host_prep_ms_sum = (double)pad_ns.load() * 1e-6;
        stats->h2d_ms_sum = h2d_ms;
        stats->kernel_ms_sum = k_ms;
        stats->d2h_ms_sum = d2h_ms;
        stats->chunks = n_chunks;
        stats->threads = threads;
        stats->frames_per_chunk = C;
        stats->coef_bytes = gpu_entropy ? (uint64_t)seg_bytes : (uint64_t)coef_bytes * (uint64_t)n_frames; // bytes downloaded
    }
    return rc;
}

int hvc_jpeg_encode_batch(hvc_ctx *c, const uint8_t *const *frames, int n_frames, int width, int height, int chroma,
                          int quality, int threads, int frames_per_chunk, uint8_t *const *jpegs, const size_t *caps,
                          size_t *sizes, hvc_batch_stats *stats) try {
    return encode_batch_impl(c, frames, n_frames, width, height, chroma, quality, threads, frames_per_chunk, jpegs, caps,
                             sizes, stats, false);
} HVC_ABI_CATCH

int hvc_jpeg_encode_batch_gpu(hvc_ctx *c, const uint8_t *const *frames, int n_frames, int width, int height, int chroma,
                              int quality, int threads, int frames_per_chunk, uint8_t *const *jpegs, const size_t *caps,
                              size_t *sizes, hvc_batch_stats *stats) try {
    return encode_batch_impl(c, frames, n_frames, width, height, chroma, quality, threads, frames_per_chunk, jpegs, caps,
                             sizes, stats, true);
} HVC_ABI_CATCH

// ---------------------------------------------------------------------------
// Mixed batches, encoding (hvc_capi_mixed_encode.hip, hvc_mixed_encode_plan.cpp)

int hvc_jpeg_encoder_mixed_layout(const int *widths, const int *heights, const int *chromas, const int *qualities, int n_frames,
                                  size_t align, hvc_jpeg_info *infos, int *status, size_t *pixel_offsets, size_t *coef_offsets,
                                  size_t *pixel_total, size_t *coef_total) try {
    return hvc::encoder_mixed_layout(widths, heights, chromas, qualities, n_frames, align, infos, status, pixel_offsets, coef_offsets,
                                     pixel_total, coef_total);
} HVC_ABI_CATCH

int hvc_encode_frames_mixed(hvc_ctx *c, const uint8_t *pixels, const size_t *pixel_offsets, const hvc_jpeg_info *infos, int n_frames,
                            int16_t *coefs, const size_t *coef_offsets, int where) try {
    return encode_frames_mixed_impl(c, pixels, pixel_offsets, infos, n_frames, coefs, coef_offsets, where);
} HVC_ABI_CATCH

int hvc_jpeg_encode_batch_mixed(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames,
                                int threads, size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes,
                                hvc_batch_stats *stats) try {
    return encode_batch_mixed_impl(c, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, caps, sizes, stats);
} HVC_ABI_CATCH

// the same with the mixed GPU Huffman coder (hvc_capi_mixed_coder.hip, hvc_huff_mixed.hip)
int hvc_huffman_encode_frames_mixed(hvc_ctx *c, const hvc_jpeg_info *infos, const int16_t *coefs, const size_t *coef_offsets, int n_frames,
                                    int tables, uint8_t *out, size_t out_cap, uint64_t *offsets, int *status, hvc_huff_spec *specs,
                                    int where) try {
    return huffman_encode_frames_mixed_impl(c, infos, coefs, coef_offsets, n_frames, tables, out, out_cap, offsets, status, specs, where);
} HVC_ABI_CATCH

int hvc_jpeg_encode_batch_mixed_gpu(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames,
                                    int threads, size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes,
                                    hvc_batch_stats *stats) try {
    return encode_batch_mixed_gpu_impl(c, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, caps, sizes, stats);
} HVC_ABI_CATCH

// ... from RGB images (k_rgb_to_ycc_mixed in front of the block stage: hvc_mixed_rgb.hip, hvc_mixed_rgb_plan.cpp)
int hvc_jpeg_encoder_mixed_rgb_layout(const int *widths, const int *heights, const int *chromas, const int *qualities, int n_frames,
                                      int layout, size_t align, size_t row_align, hvc_jpeg_info *infos, int *status, size_t *rgb_offsets,
                                      size_t *rgb_row_strides, size_t *rgb_total, size_t *pixel_offsets, size_t *coef_offsets,
                                      size_t *pixel_total, size_t *coef_total) try {
    return hvc::encoder_mixed_rgb_layout(widths, heights, chromas, qualities, n_frames, layout, align, row_align, infos, status, rgb_offsets,
                                         rgb_row_strides, rgb_total, pixel_offsets, coef_offsets, pixel_total, coef_total);
} HVC_ABI_CATCH

int hvc_encode_frames_mixed_rgb(hvc_ctx *c, const uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout,
                                const hvc_jpeg_info *infos, int n_frames, int16_t *coefs, const size_t *coef_offsets, int where) try {
    return encode_frames_mixed_rgb_impl(c, rgb, rgb_offsets, rgb_row_strides, layout, infos, n_frames, coefs, coef_offsets, where);
} HVC_ABI_CATCH

int hvc_jpeg_encode_batch_mixed_rgb(hvc_ctx *c, const uint8_t *const *frames, const size_t *rgb_row_strides, int layout,
                                    const hvc_jpeg_info *infos, int *status, int n_frames, int threads, size_t chunk_bytes,
                                    uint8_t *const *jpegs, const size_t *caps, size_t *sizes, hvc_batch_stats *stats) try {
    MixedEncodeInput in;
    in.rgb = true, in.layout = layout, in.rgb_row_strides = rgb_row_strides;
    return encode_batch_mixed_impl(c, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, caps, sizes, stats, in);
} HVC_ABI_CATCH

int hvc_jpeg_encode_batch_mixed_rgb_gpu(hvc_ctx *c, const uint8_t *const *frames, const size_t *rgb_row_strides, int layout,
                                        const hvc_jpeg_info *infos, int *status, int n_frames, int threads, size_t chunk_bytes,
                                        uint8_t *const *jpegs, const size_t *caps, size_t *sizes, hvc_batch_stats *stats) try {
    MixedEncodeInput in;
    in.rgb = true, in.layout = layout, in.rgb_row_strides = rgb_row_strides;
    return encode_batch_mixed_gpu_impl(c, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, caps, sizes, stats, in);
} HVC_ABI_CATCH

int hvc_last_mixed_coder_files(const hvc_ctx *c, uint64_t *gpu_files, uint64_t *host_files) try {
    if (!c) return HVC_E_INVALID_ARG;
    if (gpu_files) *gpu_files = c->mixed_coder_gpu_files;
    if (host_files) *host_files = c->mixed_coder_host_files;
    return HVC_OK;
} HVC_ABI_CATCH
