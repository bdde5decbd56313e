// hvc_capi_mixed_reader.hip -- the mixed GPU Huffman reader (hvc_hdec_mixed.hip) behind the C ABI: the per-chunk driver the
// mixed batch pipeline of hvc_capi_mixed.hip runs under hvc_set_mixed_reader(HVC_READER_GPU) (hvc_mixed_reader.h), and
// the function behind hvc_jpeg_entropy_decode_gpu_mixed, the same driver over one chunk on the calling thread.
#include "hvc_mixed_reader.h"

#include "hvc_batch.h"
#include "hvc_hdec_mixed.h"

namespace {

constexpr size_t SB = HVC_HD_SUBSEQ_BITS / 8;
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
// what a file of `size` bytes can need in the segment buffer: its segment is shorter than the file
size_t room_most(size_t size) { return hvc::hdm_file_room(size); }

} // namespace

int MixedGpuReader::begin(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, const hvc_jpeg_info *infos, const size_t *coef_base,
                          const std::vector<int> &take, const std::vector<int> &chunk_first, const std::vector<int> &chunk_count) {
    c_ = c;
    jpegs_ = jpegs;
    sizes_ = sizes;
    infos_ = infos;
    coef_base_ = coef_base;
    take_ = &take;
    first_ = &chunk_first;
    count_ = &chunk_count;
    ecs_off_.assign(take.size(), 0);
    geo_.assign(take.size(), hvc::HDM_TAKEN);
    size_t ecs_bytes = 0, meta_bytes = 0, subs_most = 0, dcd_most = 0, sets_most = 0, files_most = 0;
    for (size_t k = 0; k < chunk_first.size(); k++) {
        size_t at = 0, subs = 0, units = 0, dcd = 0;
        for (int t = chunk_first[k]; t < chunk_first[k] + chunk_count[k]; t++) {
            const int f = take[(size_t)t];
            hvc::HdmFileK geo;
            geo_[(size_t)t] = hvc::hdm_geometry(infos[f], geo);
            ecs_off_[(size_t)t] = at;
            if (geo_[(size_t)t] != hvc::HDM_TAKEN) continue; // (takes no room)
            const size_t n_sub = hvc::hdm_file_subs(sizes[f]);
            at += room_most(sizes[f]);
            subs += n_sub;
            units += (n_sub + HVC_HDM_UNIT - 1) / HVC_HDM_UNIT;
            dcd += geo.need;
        }
        ecs_bytes = std::max(ecs_bytes, at);
        subs_most = std::max(subs_most, subs);
        dcd_most = std::max(dcd_most, dcd);
        files_most = std::max(files_most, (size_t)chunk_count[k]);
        meta_bytes = std::max(meta_bytes, up16((size_t)chunk_count[k] * sizeof(hvc::HdmFileK)) + up16(units * sizeof(unsigned)) +
                                              up16((size_t)chunk_count[k] * sizeof(unsigned)));
    }
    // (a chunk whose files could need more than the 32-bit offsets reach: the plan refuses the files past that point)
    ecs_cap_ = std::min(ecs_bytes, (size_t)0xfff00000u);
    sets_most = std::min(files_most, (size_t)HVC_HDM_MAX_TABLE_SETS);
    sets_cap_ = sets_most;
    int r = pipeline_events(c);
    if (r) return r;
    if ((r = ring_ensure(c, reader_rings(c), {ecs_cap_ + 16, ecs_cap_ + 16, meta_bytes + 16, meta_bytes + 16, sets_most * sizeof(hvc::HdFrameTabs) + 16,
                                              sets_most * sizeof(hvc::HdFrameTabs) + 16})))
        return r;
    if ((r = grow(c, c->gd_state, HVC_HDM_STATE_BYTES(subs_most)))) return r;
    if ((r = grow(c, c->gd_dcd, dcd_most * sizeof(int16_t) + 16))) return r;
    slots_.reset(new Slot[hvc_ctx::RING]);
    return HVC_OK;
}

void MixedGpuReader::prepare(int k, int t) {
    Slot &S = slots_[k % hvc_ctx::RING];
    const int slot = k % hvc_ctx::RING, pos = t - (*first_)[(size_t)k], f = (*take_)[(size_t)t];
    {
        std::lock_guard<std::mutex> lk(S.mu);
        if (S.chunk != k) { // the chunk's first file: the slot starts over
            S.chunk = k;
            S.sets.clear();
            S.sets.reserve(sets_cap_);
            S.files.assign((size_t)(*count_)[(size_t)k], SlotFile());
        }
    }
    SlotFile sf;
    const size_t off = ecs_off_[(size_t)t], size = sizes_[f];
    const bool dri = c_->honour_restart && hvc::restart_interval_of(jpegs_[f], size) != 0; // (restart intervals: the host reader honours them)
    if (geo_[(size_t)t] == hvc::HDM_TAKEN && !dri && off + room_most(size) <= ecs_cap_) {
        std::unique_ptr<hvc::HdTables> tabs(new hvc::HdTables);
        std::memset(tabs.get(), 0, sizeof(hvc::HdTables)); // (compared byte by byte below)
        uint8_t *dst = c_->gp_h_ecs[slot].as<uint8_t>() + off;
        size_t got = 0;
        bool ok = false;
        const int r = hvc::prepare_gpu_decode_to(jpegs_[f], size, &infos_[f], *tabs, dst, (size + SB - 1) / SB * SB, &got, ok);
        if (!r && ok && got <= size) {
            std::memset(dst + got, 0, hvc::hdm_file_room(got) - got); // the zero subsequence and the overshoot (the slot is reused)
            int set = -1;
            bool fresh = false;
            {
                std::lock_guard<std::mutex> lk(S.mu);
                size_t q = S.sets.size(); // newest first: files of one source tend to come in runs
                while (q > 0 && std::memcmp(&S.sets[q - 1], tabs.get(), sizeof(hvc::HdTables))) q--;
                if (q > 0) {
                    set = (int)q - 1;
                } else if (S.sets.size() < sets_cap_) {
                    S.sets.push_back(*tabs);
                    set = (int)S.sets.size() - 1;
                    fresh = true;
                }
            }
            if (fresh) hvc::make_frame_tabs(*tabs, infos_[f].n_comp, (c_->gp_h_ftabs[slot].as<hvc::HdFrameTabs>())[set]);
            if (set >= 0) {
                sf.ok = true;
                sf.set = set;
                sf.seg_bytes = got;
            }
        }
    }
    S.files[(size_t)pos] = sf;
}

hipError_t MixedGpuReader::upload(int k, hipStream_t s) {
    const int slot = k % hvc_ctx::RING, first = (*first_)[(size_t)k], count = (*count_)[(size_t)k];
    Slot &S = slots_[slot];
    static const hvc::HdTables no_tables = {};
    std::vector<hvc::HdmFileIn> in((size_t)count);
    for (int p = 0; p < count; p++) {
        const int f = (*take_)[(size_t)(first + p)];
        const SlotFile &sf = S.files[(size_t)p];
        in[(size_t)p] = hvc::HdmFileIn{&infos_[f], ecs_off_[(size_t)(first + p)], sf.seg_bytes, sf.ok ? &S.sets[(size_t)sf.set] : &no_tables, sf.ok, coef_base_[f],
                                       sf.set}; // (the slot's sets are deduplicated already: prepare())
    }
    if (hvc::hdm_plan_build(in.data(), count, nullptr, count, S.plan)) return hipErrorInvalidValue;
    const hvc::HdmPlan &plan = S.plan;
    if (plan.files.empty()) return hipSuccess;
    // descriptors | map | verdicts (device only), each part on 16 bytes
    const size_t map_at = up16(plan.files.size() * sizeof(hvc::HdmFileK));
    S.status_at = map_at + up16(plan.map.size() * sizeof(unsigned));
    uint8_t *hm = c_->gp_h_meta[slot].as<uint8_t>();
    std::memcpy(hm, plan.files.data(), plan.files.size() * sizeof(hvc::HdmFileK)); // (tabrec: the slot's set index, as the records lie)
    std::memcpy(hm + map_at, plan.map.data(), plan.map.size() * sizeof(unsigned));
    hipError_t e = hipMemcpyAsync(c_->gp_d_ecs[slot].p, c_->gp_h_ecs[slot].p, plan.seg_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(c_->gp_d_meta[slot].p, hm, S.status_at, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c_->gp_d_ftabs[slot].p, c_->gp_h_ftabs[slot].p, S.sets.size() * sizeof(hvc::HdFrameTabs), hipMemcpyHostToDevice, s);
    return e;
}

int MixedGpuReader::read(int k, int16_t *d_coefs, hipStream_t s, std::vector<char> &back, int *gpu_files) {
    const int slot = k % hvc_ctx::RING, first = (*first_)[(size_t)k], count = (*count_)[(size_t)k];
    Slot &S = slots_[slot];
    const hvc::HdmPlan &plan = S.plan;
    for (int p = 0; p < count; p++) back[(size_t)(*take_)[(size_t)(first + p)]] = 1; // ... until the verdict says otherwise
    *gpu_files = 0;
    if (plan.files.empty()) return HVC_OK;
    if ((uintptr_t)d_coefs & 15) return HVC_E_ALIGNMENT;
    hvc::HdmParams P;
    std::memset(&P, 0, sizeof P);
    const uint8_t *dm = c_->gp_d_meta[slot].as<const uint8_t>();
    P.ecs = c_->gp_d_ecs[slot].as<const uint8_t>();
    P.files = (const hvc::HdmFileK *)dm;
    P.map = (const unsigned *)(dm + up16(plan.files.size() * sizeof(hvc::HdmFileK)));
    P.status = (unsigned *)(dm + S.status_at);
    P.ftabs = c_->gp_d_ftabs[slot].as<const hvc::HdFrameTabs>();
    P.n_files = (unsigned)plan.files.size();
    P.n_units = (unsigned)plan.map.size();
    P.coefs = d_coefs;
    P.dcd = c_->gd_dcd.as<int16_t>();
    hvc::hdm_carve_state(P, c_->gd_state.p, plan.total_sub);
    HIPCHK(c_, hvc::launch_hd_mixed(P, s));
    verdict_.assign(plan.files.size(), 0xffu);
    HIPCHK(c_, hipMemcpyAsync(verdict_.data(), P.status, plan.files.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(c_, hipStreamSynchronize(s));
    for (size_t i = 0; i < plan.files.size(); i++)
        if (verdict_[i] == 0u) {
            back[(size_t)(*take_)[(size_t)(first + plan.file_of[i])]] = 0;
            ++*gpu_files;
        }
    return HVC_OK;
}

// ---------------------------------------------------------------------------
// behind hvc_jpeg_entropy_decode_gpu_mixed (hvc_capi_jpeg.hip)
int entropy_decode_gpu_mixed_impl(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, const hvc_jpeg_info *infos,
                                  int *status, int16_t *coefs, const size_t *coef_offsets, size_t coef_cap, int where, int *used_gpu) {
    if (!c || !jpegs || !sizes || !infos || !status || !coef_offsets || n_files < 0) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    std::vector<int> take;
    size_t span = 0;
    for (int f = 0; f < n_files; f++) {
        if (used_gpu) used_gpu[f] = 0;
        if (status[f] != HVC_OK) continue;
        if (!jpegs[f] || infos[f].n_comp < 0 || infos[f].n_comp > 4) return HVC_E_INVALID_ARG;
        if (infos[f].coef_count) {
            if (coef_offsets[f] & 7) return HVC_E_ALIGNMENT;
            if (coef_offsets[f] > coef_cap || infos[f].coef_count > coef_cap - coef_offsets[f]) return HVC_E_INVALID_ARG;
            span = std::max(span, coef_offsets[f] + (size_t)infos[f].coef_count);
        }
        take.push_back(f);
    }
    if (take.empty()) return HVC_OK;
    if (span && (!coefs || (where == HVC_MEM_DEVICE && ((uintptr_t)coefs & 15)))) return coefs ? HVC_E_ALIGNMENT : HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    hvc::RestartScope honour(c->honour_restart);
    int r;
    int16_t *d = coefs;
    if (where == HVC_MEM_HOST) {
        if ((r = grow(c, c->gd_coefs, span * sizeof(int16_t) + 16))) return r;
        d = c->gd_coefs.as<int16_t>();
    }
    const std::vector<int> first{0}, count{(int)take.size()};
    std::vector<char> back((size_t)n_files, 0);
    MixedGpuReader rd;
    if ((r = rd.begin(c, jpegs, sizes, infos, coef_offsets, take, first, count))) return r;
    for (int t = 0; t < (int)take.size(); t++) rd.prepare(0, t);
    hipError_t he = rd.upload(0, c->stream);
    if (he != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return fail_hip(c, he);
    }
    int n_gpu = 0;
    if ((r = rd.read(0, d, c->stream, back, &n_gpu))) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    // the handed-back files: the host reader on this thread, its result the file's own
    std::vector<hvc::WideDc> wide;
    std::vector<int16_t> tmp;
    for (int f : take) {
        const size_t n = infos[f].coef_count;
        if (!back[(size_t)f]) {
            if (used_gpu) used_gpu[f] = 1;
            if (where == HVC_MEM_HOST && n)
                HIPCHK(c, hipMemcpyAsync(coefs + coef_offsets[f], d + coef_offsets[f], n * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
            continue;
        }
        if (n == 0) {
            status[f] = hvc_jpeg_entropy_decode(jpegs[f], sizes[f], &infos[f], nullptr);
            continue;
        }
        wide.clear();
        int16_t *dst = coefs + coef_offsets[f];
        if (where == HVC_MEM_DEVICE) {
            tmp.assign(n, 0);
            dst = tmp.data();
        }
        int e = hvc::entropy_decode_wide(jpegs[f], sizes[f], &infos[f], dst, wide);
        if (!e && !wide.empty()) e = HVC_E_RANGE; // (a DC beyond int16: no side list here)
        status[f] = e;
        if (!e && where == HVC_MEM_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(coefs + coef_offsets[f], dst, n * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream)); // (tmp is reused)
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}
