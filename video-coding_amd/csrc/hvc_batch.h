// hvc_batch.h -- what the batch decode pipelines share (internal): the streams and events of a pipeline call, and the
// orchestrating loop of the two pipelines with the host reader (decode_batch_impl, decode_batch_mixed_impl):
//   host Huffman threads (hvc_feed.h) || hipMemcpyAsync (copy stream) || block stage (compute stream)
// and, at the end, the part the two mixed ENCODE file pipelines run in common (MixedEncodeFront, encode_mixed_chunks)
#ifndef HVC_BATCH_H
#define HVC_BATCH_H

#include "hvc_ctx.h"
#include "hvc_feed.h"

// the copy stream and the events of the decode pipelines, created by the first call that needs them
inline int pipeline_events(hvc_ctx *c) {
    HIPCHK(c, c->copy_stream.ensure());
    for (int i = 0; i < hvc_ctx::RING; i++) {
        HIPCHK(c, c->ev_h2d[i].ensure());
        HIPCHK(c, c->ev_kern[i].ensure());
    }
    for (int i = 0; i < 4; i++)
        HIPCHK(c, c->ev_t[i].ensure());
    return HVC_OK;
}

// Chunk after chunk, once the feed's workers (started by the caller) have filled it: h_ring[slot] -> d_ring[slot] on the copy
// stream, the caller's block stage and downloads behind it on the compute stream, the pinned slot back to the workers as soon
// as the upload is through.  Ends the feed, drains both streams and fills what it knows of `stats` (the caller adds
// entropy_ms_sum, frames_per_chunk and coef_bytes).
//   count_of(k)       items of chunk k
//   upload_bytes(k)   bytes of h_ring[slot] to upload once chunk k is complete; 0: no copy
//                     (called with the copy stream waiting for the slot's last kernel: a pipeline whose chunk is not
//                     coefficients -- the mixed GPU reader's segments and descriptors -- enqueues its own copies there and returns 0)
//   stage(k, slot)    enqueues the block stage on c->stream: an hvc_status
//   download(k, slot) enqueues what brings the chunk home on c->stream: a hipError_t
template <class Count, class Bytes, class Stage, class Download>
inline int host_reader_chunks(hvc_ctx *c, hvc::ChunkFeed &feed, int n_chunks, int threads, std::chrono::steady_clock::time_point wall0,
                              Count count_of, Bytes upload_bytes, Stage stage, Download download, hvc_batch_stats *stats) {
    constexpr int NB = hvc_ctx::RING;
    int rc = HVC_OK;
    double h2d_ms = 0, k_ms = 0, d2h_ms = 0;
    hipStream_t compute = c->stream;
    try {
        for (int k = 0; k < n_chunks && rc == HVC_OK; k++) {
            const int slot = k % NB;
            if ((rc = feed.wait_chunk(k, count_of(k)))) break;
            hipError_t he = hipSuccess;
            // the device chunk (and output ring slot) is reused every NB chunks: its previous kernel must be done
            if (k >= NB) he = hipStreamWaitEvent(c->copy_stream, c->ev_kern[slot], 0);
            if (he == hipSuccess) he = hipEventRecord(c->ev_t[0], c->copy_stream);
            if (he == hipSuccess)
                if (const size_t bytes = upload_bytes(k))
                    he = hipMemcpyAsync(c->d_ring[slot].p, c->h_ring[slot].p, bytes, hipMemcpyHostToDevice, c->copy_stream);
            if (he == hipSuccess) he = hipEventRecord(c->ev_h2d[slot], c->copy_stream);
            if (he == hipSuccess) he = hipStreamWaitEvent(compute, c->ev_h2d[slot], 0);
            if (he == hipSuccess) he = hipEventRecord(c->ev_t[1], compute);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            if ((rc = stage(k, slot))) break;
            he = hipEventRecord(c->ev_t[2], compute);
            if (he == hipSuccess) he = download(k, slot);
            if (he == hipSuccess) he = hipEventRecord(c->ev_kern[slot], compute);
            if (he == hipSuccess) he = hipEventRecord(c->ev_t[3], compute);
            // wait for this chunk's upload, then hand the pinned slot to chunk k + NB
            if (he == hipSuccess) he = wait_event(c->ev_h2d[slot]);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            feed.release(k);
            float ms = 0;
            if (hipEventElapsedTime(&ms, c->ev_t[0], c->ev_h2d[slot]) == hipSuccess) h2d_ms += ms;
            // kernel / d2h times of this chunk: the events are shared by all chunks, so they are read (and the
            // chunk waited for) before the next one records them; the worker threads -- the bound of this
            // pipeline -- keep decoding into the other ring slots meanwhile
            if (wait_event(c->ev_t[3]) == hipSuccess) {
                if (hipEventElapsedTime(&ms, c->ev_t[1], c->ev_t[2]) == hipSuccess) k_ms += ms;
                if (hipEventElapsedTime(&ms, c->ev_t[2], c->ev_t[3]) == hipSuccess) d2h_ms += ms;
            }
        }
    } catch (...) {
        rc = hvc::exception_code();
    }
    rc = feed.finish(rc);
    {
        const hipError_t h1 = hipStreamSynchronize(compute), h2 = hipStreamSynchronize(c->copy_stream);
        if (rc == HVC_OK && (h1 != hipSuccess || h2 != hipSuccess)) rc = fail_hip(c, h1 != hipSuccess ? h1 : h2);
    }
    if (stats) {
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        stats->h2d_ms_sum = h2d_ms;
        stats->kernel_ms_sum = k_ms;
        stats->d2h_ms_sum = d2h_ms;
        stats->chunks = n_chunks;
        stats->threads = threads;
    }
    return rc;
}

// The two mixed ENCODE file pipelines (host coder: hvc_capi_mixed_encode.hip; GPU coder: hvc_capi_mixed_coder.hip) are one
// pipeline up to the coefficient slot.  encode_mixed_chunks (hvc_capi_mixed_encode.hip) runs that part: the chunk cut
// (hvc_mixed_encode_chunks.h), streams, events and the rings of the pixel side, two feeds -- the padding workers fill pinned
// pixel slots for the orchestrating thread, the orchestrating thread hands the slots behind the block stage to the pipeline's
// own workers --, per chunk the upload and the block stage (RGB input: the colour stage in front of it) into ed_out[slot],
// and the way out: both feeds ended, the streams drained, what it knows of `stats` filled (the pipeline adds entropy_ms_sum
// and coef_bytes).  The pipeline fills in what stands behind the block stage before the call and reads the rest after it.
struct MixedEncodeFront {
    int max_files_per_chunk = 0; // a chunk closes at that many files (0: no cap)
    bool down_stream = false;    // the pipeline also uses c->down_stream and ev_gpu[]
    std::function<int()> setup;  // (optional) rings and tables of its own, sized by `plan`, before anything starts
    std::function<void()> worker;             // body of a thread of the feed `codf`: items are positions in plan.take
    std::function<int(int k, int slot)> stage; // enqueues what follows chunk k's block stage: an hvc_status
    std::function<int(int k)> retire;         // chunk k is enqueued and its upload through: what it retires of the chunks before
    std::function<int()> drain;               // behind the last chunk: what retire has left
    // the call under way
    hvc::MixedEncodeChunks plan;
    hvc::ChunkFeed *codf = nullptr; // ring 0: chunk k may be read by the workers once release(k) says it has landed
    int threads = 0;                // as clamped
    bool ran = false;               // the pipeline started: `stats` are filled
    std::chrono::steady_clock::time_point wall0;
    double h2d_ms = 0, k_ms = 0, d2h_ms = 0; // retire / drain add the chunks' event times
    static long long ns_since(std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    }
};
int encode_mixed_chunks(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                        size_t chunk_bytes, uint8_t *const *jpegs, const MixedEncodeInput &in, MixedEncodeFront &fr, hvc_batch_stats *stats);

#endif
