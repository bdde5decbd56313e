// hvc_capi_mixed_coder.hip -- the MIXED GPU Huffman coder behind the C ABI (hvc_huff_mixed.hip, hvc_huff_mixed_plan.cpp):
// the coder alone over a set of coefficient records (behind hvc_huffman_encode_frames_mixed) and the file pipeline built on it
// (behind hvc_jpeg_encode_batch_mixed_gpu); the entry points themselves stand in hvc_capi_files.hip.
// The pipeline is encode_batch_mixed_impl's up to the coefficient slot -- both run encode_mixed_chunks (MixedEncodeFront,
// hvc_batch.h; hvc_capi_mixed_encode.hip) -- with the coder stage of hvc_jpeg_encode_batch_gpu behind it:
//   host threads: Plane.blit_available into zero-padded planes (pinned ring)  [RGB input, MixedEncodeInput: the image's rows, tight]
//   copy stream:  hipMemcpyAsync H2D           compute stream: [RGB input: the plane slot cleared, k_rgb_to_ycc_mixed into it,]
//                                               k_encode_mixed into the device slot, the mixed coder over it,
//                                               D2H of the chunk's offsets, status words and (optimised) specs
//   down stream:  exactly the packed segments of the files the GPU finished, into the pinned slot
//   host threads: header (jpeg_header_bytes with the file's info and its own specs) + segment + EOI per file
// The files the GPU path does not finish -- flagged by the length pass, past the segment slot (huff_mixed_hand_back),
// refused by the coder's plan, or all of them under a restart interval -- are coded by the host coder in ONE pass behind the
// GPU chunks, through encode_batch_mixed_impl itself with every other file masked out by its status.
#include "hvc_batch.h"
#include "hvc_huff_mixed.h"

namespace {

// Plan image (files | planes | map, each part on 16 bytes, c->mixed_huff_plan) + scratch + tables of one run of the coder over
// `plan`.  d_offsets: device, plan.files.size() + 1 entries (nullptr: inside the context's scratch).
int mixed_coder_prepare(hvc_ctx *c, const hvc::HuffMixedPlan &plan, const int16_t *d_coefs, uint8_t *d_out, size_t out_cap,
                        unsigned long long *d_offsets, bool optimised, bool partial, hvc::HuffMixedParams &P) {
    std::memset(&P, 0, sizeof P);
    const size_t nf = plan.files.size();
    size_t at[3];
    int r = upload_parts(c, c->mixed_huff_plan, {{plan.files.data(), nf * sizeof(hvc::HuffMixedFileK)},
                                                 {plan.planes.data(), plan.planes.size() * sizeof(hvc::HuffMixedPlaneK)},
                                                 {plan.map.data(), plan.map.size() * sizeof(unsigned)}}, at);
    if (r) return r;
    const unsigned char *d = c->mixed_huff_plan.d.as<const unsigned char>();
    P.files = reinterpret_cast<const hvc::HuffMixedFileK *>(d);
    P.planes = reinterpret_cast<const hvc::HuffMixedPlaneK *>(d + at[1]);
    P.map = reinterpret_cast<const unsigned *>(d + at[2]);
    P.n_files = (unsigned)nf;
    P.n_units = (unsigned)plan.map.size();
    P.coefs = d_coefs;
    if (optimised) { // per file: counts, code tables (both HUFF_TABLE_WORDS words), four specs
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
    if ((r = grow(c, c->hd_lens, (size_t)plan.lens_total * sizeof(unsigned)))) return r;
    if ((r = grow(c, c->hd_meta, (4 + 6 * nf + 1 + 2 * (nf + 1)) * sizeof(unsigned) + 64))) return r;
    if ((r = grow(c, c->hd_bitbuf, (size_t)plan.bitbuf_words * sizeof(unsigned)))) return r;
    if ((r = grow(c, c->hd_ff, (size_t)plan.pieces_cap * sizeof(unsigned)))) return r;
    P.lens = c->hd_lens.as<unsigned>();
    unsigned *m = c->hd_meta.as<unsigned>();
    P.status = m;
    P.file_bits = m + 4;
    P.file_bytes = P.file_bits + nf;
    P.file_pieces = P.file_bytes + nf;
    P.file_ff = P.file_pieces + nf;
    P.file_status = P.file_ff + nf;
    P.piece_base = P.file_status + nf; // nf + 1 entries
    unsigned long long *scratch_off = (unsigned long long *)(((uintptr_t)(P.piece_base + nf + 1) + 7) & ~(uintptr_t)7);
    P.bitbuf = c->hd_bitbuf.as<unsigned>();
    P.bitbuf_words = plan.bitbuf_words;
    P.ff = c->hd_ff.as<unsigned>();
    P.pieces_cap = (unsigned)plan.pieces_cap;
    P.out_offsets = d_offsets ? d_offsets : scratch_off;
    P.out = d_out;
    P.out_cap = out_cap;
    P.partial = partial ? 1 : 0;
    return HVC_OK;
}

int file_code(unsigned file_status) { // a file's status word as an hvc_status
    return (file_status & 1u) ? HVC_E_RANGE : file_status ? HVC_E_INTERNAL : HVC_OK;
}

} // namespace

// behind hvc_huffman_encode_frames_mixed (hvc_capi_files.hip)
int huffman_encode_frames_mixed_impl(hvc_ctx *c, const hvc_jpeg_info *infos, const int16_t *coefs, const size_t *coef_offsets, int n_frames,
                                     int tables, uint8_t *out, size_t out_cap, uint64_t *offsets, int *status, hvc_huff_spec *specs,
                                     int where) {
    if (!c || n_frames < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    if (tables != HVC_HUFF_DEFAULT && tables != HVC_HUFF_OPTIMISED) return HVC_E_INVALID_ARG;
    if (n_frames == 0) return HVC_OK; // (an empty set needs no memory)
    const bool opt = tables == HVC_HUFF_OPTIMISED;
    if (!infos || !coef_offsets || !offsets || !status || (opt && !specs)) return HVC_E_INVALID_ARG;
    for (int f = 0; f < n_frames; f++)
        if (coef_offsets[f] & 7) return HVC_E_ALIGNMENT;
    if (where == HVC_MEM_DEVICE && (((uintptr_t)coefs & 15) || ((uintptr_t)offsets & 7))) return HVC_E_ALIGNMENT;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    hvc::HuffMixedPlan plan;
    int r = hvc::huff_mixed_plan_build(infos, coef_offsets, nullptr, n_frames, opt, plan);
    if (r) return r;
    const size_t nf = plan.files.size();
    const std::vector<int> frame_status = plan.status; // (the host-memory path plans the taken frames again, at their staging offsets)
    std::vector<uint64_t> all((size_t)n_frames + 1, 0); // the offsets with the refused frames' empty segments in place
    if (nf == 0) {
        for (int f = 0; f < n_frames; f++) status[f] = plan.status[(size_t)f];
        if (where == HVC_MEM_HOST)
            std::memcpy(offsets, all.data(), all.size() * sizeof(uint64_t));
        else
            HIPCHK(c, hipMemcpy(offsets, all.data(), all.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        return HVC_OK;
    }
    if (!coefs || !out) return HVC_E_INVALID_ARG;
    hvc::HuffMixedParams P;
    const size_t worst = (size_t)plan.bitbuf_words * 8; // every byte stuffed: what the device can ever write
    if (where == HVC_MEM_DEVICE) {
        if ((r = mixed_coder_prepare(c, plan, coefs, out, out_cap, nullptr, opt, false, P))) return r;
    } else {
        // host memory: the taken frames' records one after another in c->d_in, each on 16 bytes; the segments in c->hd_out
        std::vector<size_t> d_coef((size_t)n_frames, 0);
        size_t ctot = 0;
        for (size_t k = 0; k < nf; k++) {
            const int f = plan.file_of[k];
            d_coef[(size_t)f] = ctot;
            ctot += (infos[f].coef_count + 7) & ~(size_t)7;
        }
        if ((r = grow(c, c->d_in, ctot * sizeof(int16_t)))) return r;
        if ((r = grow(c, c->hd_out, std::min(out_cap, worst) + 64))) return r;
        const std::vector<int> taken = plan.file_of;
        if ((r = hvc::huff_mixed_plan_build(infos, d_coef.data(), taken.data(), (int)nf, opt, plan))) return r;
        if (plan.files.size() != nf) return HVC_E_INTERNAL;
        for (size_t k = 0; k < nf; k++) {
            const int f = plan.file_of[k];
            HIPCHK(c, hipMemcpyAsync(c->d_in.as<int16_t>() + d_coef[(size_t)f], coefs + coef_offsets[f], infos[f].coef_count * sizeof(int16_t),
                                     hipMemcpyHostToDevice, c->stream));
        }
        if ((r = mixed_coder_prepare(c, plan, c->d_in.as<const int16_t>(), c->hd_out.as<uint8_t>(), out_cap, nullptr, opt, false, P))) return r;
    }
    unsigned call_status = 0;
    std::vector<unsigned> fstat(nf, 0);
    std::vector<unsigned long long> off(nf + 1, 0);
    std::vector<hvc_huff_spec> sp(opt ? 4 * nf : 0);
    HIPCHK(c, hvc::launch_huffman_encode_mixed(P, c->stream));
    HIPCHK(c, hipMemcpyAsync(&call_status, P.status, sizeof call_status, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fstat.data(), P.file_status, nf * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(off.data(), P.out_offsets, (nf + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (opt) HIPCHK(c, hipMemcpyAsync(sp.data(), P.specs, sp.size() * sizeof(hvc_huff_spec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((call_status & 4u) || off[nf] > out_cap) return HVC_E_INVALID_ARG; // out_cap too small: nothing was written
    // frame by frame: the refused ones keep the plan's code and an empty segment
    {
        size_t k = 0;
        for (int f = 0; f < n_frames; f++) {
            all[(size_t)f] = off[k];
            status[f] = frame_status[(size_t)f];
            if (status[f] != HVC_OK) continue;
            status[f] = file_code(fstat[k]);
            if (opt && status[f] == HVC_OK) std::memcpy(specs + 4 * (size_t)f, sp.data() + 4 * k, 4 * sizeof(hvc_huff_spec));
            k++;
        }
        all[(size_t)n_frames] = off[nf];
    }
    if (where == HVC_MEM_HOST) {
        if (off[nf]) HIPCHK(c, hipMemcpy(out, c->hd_out.p, (size_t)off[nf], hipMemcpyDeviceToHost));
        std::memcpy(offsets, all.data(), all.size() * sizeof(uint64_t));
    } else {
        HIPCHK(c, hipMemcpy(offsets, all.data(), all.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    return HVC_OK;
}

// behind hvc_jpeg_encode_batch_mixed_gpu (hvc_capi_files.hip)
int encode_batch_mixed_gpu_impl(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                                size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes, hvc_batch_stats *stats,
                                const MixedEncodeInput &in) {
    if (!c || !frames || !infos || !status || !jpegs || !caps || !sizes || n_frames < 0) return HVC_E_INVALID_ARG;
    if (c->enc_arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG;
    if (in.rgb && in.layout != HVC_RGB_INTERLEAVED && in.layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (stats) std::memset(stats, 0, sizeof *stats);
    c->mixed_coder_gpu_files = c->mixed_coder_host_files = 0;
    if (n_frames == 0) return HVC_OK;
    // The host coder's pass: the files named by `mine` (1 = handed back), every other file masked out by its status
    auto host_pass = [&](const std::vector<char> &mine, hvc_batch_stats *st) {
        std::vector<int> st2((size_t)n_frames, HVC_E_INTERNAL);
        unsigned long long n = 0;
        for (int f = 0; f < n_frames; f++)
            if (mine[(size_t)f]) st2[(size_t)f] = HVC_OK, n++;
        const int r = encode_batch_mixed_impl(c, frames, infos, st2.data(), n_frames, threads, chunk_bytes, jpegs, caps, sizes, st, in);
        for (int f = 0; f < n_frames; f++)
            if (mine[(size_t)f]) status[f] = st2[(size_t)f];
        c->mixed_coder_host_files += n;
        return r;
    };
    if (c->restart_interval) { // restart intervals are not in the mixed GPU coder: every file goes to the host coder
        std::vector<char> mine((size_t)n_frames, 0);
        for (int f = 0; f < n_frames; f++) mine[(size_t)f] = status[f] == HVC_OK;
        return host_pass(mine, stats);
    }
    constexpr int NB = hvc_ctx::RING;
    const bool opt = c->huff_tables == HVC_HUFF_OPTIMISED; // each file its own tables (hvc_set_huffman_tables)
    MixedEncodeFront fr; // the chunks are encode_batch_mixed_impl's but for the coder's cap on a chunk's files
    fr.max_files_per_chunk = HVC_HUFF_MIXED_MAX_FILES;
    fr.down_stream = true;
    const hvc::MixedEncodeChunks &plan = fr.plan;
    const std::vector<int> &take = plan.take;

    // what the orchestrating thread leaves for the assembling workers, per position in `take` (written before the chunk's
    // release, which the feed's mutex orders)
    std::vector<char> by_gpu, handed((size_t)n_frames, 0);
    std::vector<unsigned long long> seg_at, seg_len;
    std::vector<hvc_huff_spec> own_specs;
    std::vector<std::vector<int>> chunk_files; // per chunk: the position in `take` of each file of its coder plan
    std::vector<size_t> chunk_cap;
    unsigned long long seg_total = 0, gpu_done = 0, n_handed = 0;
    size_t words_at = 0;
    std::atomic<long long> ent_ns{0};
    fr.setup = [&]() {
        int r;
        if (opt && (r = ring_ensure(c, enc_spec_rings(c), {(size_t)plan.largest * 4 * sizeof(hvc_huff_spec)}))) return r;
        // per slot: the packed segments on the device (capacity = the chunk's coefficient records, the uniform pipeline's rule),
        // and (count + 1) offsets, the launch's status word and `count` file status words, on the device and pinned
        words_at = ((size_t)plan.largest + 2) * sizeof(unsigned long long);
        const size_t off_bytes = words_at + (size_t)plan.largest * sizeof(unsigned);
        if ((r = ring_ensure(c, enc_seg_rings(c), {plan.out_bytes, off_bytes, off_bytes}))) return r;
        by_gpu.assign(take.size(), 0);
        seg_at.assign(take.size(), 0);
        seg_len.assign(take.size(), 0);
        own_specs.resize(opt ? 4 * take.size() : 0);
        chunk_files.resize(plan.chunks.size());
        chunk_cap.assign(plan.chunks.size(), 0);
        return (int)HVC_OK;
    };
    fr.worker = [&]() { // header + the file's segment + EOI (complete_and_write_eoi, encoder.ml:507-510)
        hvc::ChunkFeed &codf = *fr.codf;
        if (!pin_to_ctx_cpus(c)) codf.raise(HVC_E_INVALID_ARG);
        std::vector<uint8_t> header;
        for (;;) {
            const int t = codf.claim();
            if (t >= (int)take.size() || codf.error()) return;
            const int f = take[(size_t)t], k = plan.chunk_of[(size_t)f];
            if (!codf.wait_slot(k)) return;
            if (by_gpu[(size_t)t]) {
                const auto t0 = std::chrono::steady_clock::now();
                header.clear();
                hvc::jpeg_header_bytes(&infos[f], header, opt ? own_specs.data() + 4 * (size_t)t : nullptr, 0);
                const size_t seg = (size_t)seg_len[(size_t)t];
                sizes[f] = header.size() + seg + 2;
                if (sizes[f] > caps[f]) {
                    status[f] = HVC_E_INVALID_ARG; // the file's own result: it stops nobody else
                } else {
                    std::memcpy(jpegs[f], header.data(), header.size());
                    std::memcpy(jpegs[f] + header.size(), c->eh_out[k % NB].as<const uint8_t>() + seg_at[(size_t)t], seg);
                    jpegs[f][header.size() + seg] = 0xff;
                    jpegs[f][header.size() + seg + 1] = 0xd9;
                    status[f] = HVC_OK;
                }
                ent_ns += MixedEncodeFront::ns_since(t0);
            }
            codf.report(k, 1, HVC_OK);
        }
    };
    // behind the block stage: the coder over the chunk's records; a file its plan refuses is the host coder's
    fr.stage = [&](int k, int slot) {
        const hvc::MixedEncodeChunk &ch = plan.chunks[(size_t)k];
        const int *list = take.data() + ch.first;
        hipStream_t compute = c->stream;
        int rc;
        hvc::HuffMixedPlan hp;
        if ((rc = hvc::huff_mixed_plan_build(infos, plan.coef_rel.data(), list, ch.count, opt, hp))) return rc;
        std::vector<int> &files = chunk_files[(size_t)k];
        for (int i = 0; i < ch.count; i++) {
            if (hp.status[(size_t)i] == HVC_OK)
                files.push_back(ch.first + i);
            else
                handed[(size_t)list[i]] = 1, n_handed++;
        }
        chunk_cap[(size_t)k] = ch.coef_elems * sizeof(int16_t);
        const size_t nf = files.size();
        unsigned long long *d_off = c->ed_off[slot].as<unsigned long long>();
        hipError_t he;
        if (nf) {
            hvc::HuffMixedParams P;
            if ((rc = mixed_coder_prepare(c, hp, c->ed_out[slot].as<const int16_t>(), c->ed_seg[slot].as<uint8_t>(), chunk_cap[(size_t)k], d_off,
                                          opt, true, P)))
                return rc;
            he = hvc::launch_huffman_encode_mixed(P, compute);
            if (he == hipSuccess) he = hipEventRecord(c->ev_et[slot][2], compute);
            if (he == hipSuccess)
                he = hipMemcpyAsync(c->eh_off[slot].p, d_off, (nf + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, compute);
            if (he == hipSuccess) // (the context's scratch: copied before the next chunk's coder reuses it)
                he = hipMemcpyAsync(c->eh_off[slot].as<unsigned char>() + words_at, P.file_status, nf * sizeof(unsigned),
                                    hipMemcpyDeviceToHost, compute);
            if (he == hipSuccess && opt)
                he = hipMemcpyAsync(c->eh_specs[slot].p, P.specs, nf * 4 * sizeof(hvc_huff_spec), hipMemcpyDeviceToHost, compute);
        } else {
            he = hipEventRecord(c->ev_et[slot][2], compute);
        }
        if (he == hipSuccess) he = hipEventRecord(c->ev_gpu[slot], compute);
        return he == hipSuccess ? (int)HVC_OK : fail_hip(c, he);
    };
    std::vector<int> complete, back;
    // chunk j's offsets and status words have landed: the hand-back decision, then exactly its segments on down_stream
    auto coded = [&](int j) {
        const int slot = j % NB;
        hipError_t he = wait_event(c->ev_gpu[slot]);
        if (he != hipSuccess) return fail_hip(c, he);
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_et[slot][0], c->ev_up[slot]) == hipSuccess) fr.h2d_ms += ms;
        if (hipEventElapsedTime(&ms, c->ev_et[slot][1], c->ev_et[slot][2]) == hipSuccess) fr.k_ms += ms;
        const std::vector<int> &files = chunk_files[(size_t)j];
        const int nf = (int)files.size();
        const unsigned long long *off = c->eh_off[slot].as<const unsigned long long>();
        const unsigned *fstat = reinterpret_cast<const unsigned *>(c->eh_off[slot].as<const unsigned char>() + words_at);
        hvc::huff_mixed_hand_back(off, fstat, nf, chunk_cap[(size_t)j], complete, back);
        unsigned long long end = 0;
        for (int k : complete) {
            const int t = files[(size_t)k];
            by_gpu[(size_t)t] = 1;
            seg_at[(size_t)t] = off[k];
            seg_len[(size_t)t] = off[k + 1] - off[k];
            end = off[k + 1];
            if (opt) std::memcpy(own_specs.data() + 4 * (size_t)t, c->eh_specs[slot].as<const hvc_huff_spec>() + 4 * (size_t)k, 4 * sizeof(hvc_huff_spec));
        }
        for (int k : back) handed[(size_t)take[(size_t)files[(size_t)k]]] = 1, n_handed++;
        gpu_done += complete.size();
        he = hipEventRecord(c->ev_et[slot][0], c->down_stream);
        if (he == hipSuccess && end) he = hipMemcpyAsync(c->eh_out[slot].p, c->ed_seg[slot].p, (size_t)end, hipMemcpyDeviceToHost, c->down_stream);
        if (he == hipSuccess) he = hipEventRecord(c->ev_down[slot], c->down_stream);
        if (he != hipSuccess) return fail_hip(c, he);
        seg_total += end;
        return (int)HVC_OK;
    };
    // chunk j's segments have landed: its pinned slot goes to the assembling workers
    auto landed = [&](int j) {
        const int slot = j % NB;
        const hipError_t he = wait_event(c->ev_down[slot]);
        if (he != hipSuccess) return fail_hip(c, he);
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_et[slot][0], c->ev_down[slot]) == hipSuccess) fr.d2h_ms += ms;
        fr.codf->release(j);
        return (int)HVC_OK;
    };
    fr.retire = [&](int k) {
        int rc = HVC_OK;
        if (k > 1) rc = landed(k - 2);
        if (rc == HVC_OK && k > 0) rc = coded(k - 1); // (while this chunk's kernels run)
        return rc;
    };
    fr.drain = [&]() {
        const int n_chunks = (int)plan.chunks.size();
        int rc = HVC_OK;
        if (n_chunks > 1) rc = landed(n_chunks - 2);
        if (rc == HVC_OK) rc = coded(n_chunks - 1);
        if (rc == HVC_OK) rc = landed(n_chunks - 1);
        return rc;
    };
    int rc = encode_mixed_chunks(c, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, in, fr, stats);
    if (!fr.ran) return rc;
    c->mixed_coder_gpu_files = gpu_done;
    hvc_batch_stats host_stats;
    std::memset(&host_stats, 0, sizeof host_stats);
    if (rc == HVC_OK && n_handed) rc = host_pass(handed, &host_stats); // ONE pass behind the GPU chunks
    if (stats) { // (with the host pass's)
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - fr.wall0).count();
        stats->entropy_ms_sum = (double)ent_ns.load() * 1e-6 + host_stats.entropy_ms_sum;
        stats->host_prep_ms_sum += host_stats.host_prep_ms_sum;
        stats->h2d_ms_sum += host_stats.h2d_ms_sum;
        stats->kernel_ms_sum += host_stats.kernel_ms_sum;
        stats->d2h_ms_sum += host_stats.d2h_ms_sum;
        stats->chunks += host_stats.chunks;
        stats->coef_bytes = (uint64_t)seg_total + host_stats.coef_bytes; // bytes downloaded: the segments (+ the host pass's records)
    }
    return rc;
}
