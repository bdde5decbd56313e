// hvc_hdec_mixed.hip -- the GPU Huffman reader of hvc_hdec.hip for files of DIFFERENT geometry (gfx950).
//
// hvc_hdec.hip's launches serve one geometry: blocks per MCU, the MCU grid, the components' planes and the record stride
// are kernel arguments, and one status word speaks for the whole chunk.  Here all of that is per FILE and lives in device
// memory (HdmFileK, hvc_hdec_mixed_plan.h), found the way k_decode_mixed finds its plane: a work unit is 64 consecutive
// subsequences of one file = one wavefront, a map names the unit's file, and what the wavefront reads of the descriptor is
// wave-uniform.  The Huffman tables are the chunk's distinct HdFrameTabs records (PF mode's), read in device memory.
//   k_hdm_sync   one synchronisation round over every unit (HVC_HDM_ROUNDS launches back to back): subsequence j of a file
//                starts from the exit its predecessor j - 1 OF THE SAME FILE recorded in the round before -- exits are double
//                buffered by round, so a round never sees a half-updated neighbour and the run is deterministic -- and walks
//                only if that differs from what it started from last time (spec_walk of hvc_hdec_dev.h, rows staged in LDS)
//   k_hdm_scan   per file: exclusive scan of the blocks per subsequence; fewer blocks than the file needs -> status bit 2
//   k_hdm_write  every lane decodes the blocks that START in its subsequence and stores them whole; it checks that its start
//                is its predecessor's recorded exit and that its own walk crosses the subsequence's end in the recorded
//                state.  By induction from subsequence 0, whose start is the truth, a file whose lanes all pass has been
//                parsed as the sequential reader parses it; any lane that does not pass raises the FILE's status bit 3, and
//                the file goes to the host reader.  No host round trip, no "changed" flag: the verdict sorts it out.
//   k_hdm_dc     per (file, component): DC differences -> values by a prefix sum in scan order, into the records
// Bounds: a walk takes its block-in-MCU index only from a state of its own file (< its blocks per MCU); stores happen for block
// indices below the file's need at addresses computed from that index inside the file's record; reads end inside the segment
// buffer + HVC_HD_ECS_SLACK (a lane gives up four subsequences past the start of its own).
#include "hvc_hdec_mixed.h"

#include "hvc_hdec_dev.h"

namespace hvc {

using namespace hd_dev;

namespace {

constexpr int HDM_WG = HVC_HDM_GROUP * HVC_HDM_UNIT; // 256 lanes: four units
constexpr int HDM_EXTRA = 3;                         // subsequences past its own a lane of the write pass may walk into

// the file of this wavefront's unit (wave-uniform: a scalar register)
__device__ __forceinline__ unsigned unit_file(const HdmParams &P, unsigned unit) {
    return (unsigned)__builtin_amdgcn_readfirstlane((int)P.map[unit]);
}

} // namespace

__global__ __launch_bounds__(HDM_WG) void k_hdm_sync(HdmParams P, int round) {
    __shared__ unsigned rows[HVC_HDM_GROUP][64 * SROW + 2]; // (+ 2: see spec_walk)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned unit = blockIdx.x * (unsigned)HVC_HDM_GROUP + (unsigned)wave;
    if (unit >= P.n_units) return; // (per wavefront; the kernel has no barrier)
    const unsigned f = unit_file(P, unit);
    const HdmFileK &F = P.files[f];
    const unsigned j = (unit - F.unit0) * 64u + (unsigned)lane;
    if (round == 0 && j == 0u) P.status[f] = 0u; // the run's first launch clears the verdicts
    if (j >= F.n_sub) return;
    const unsigned i = F.sub0 + j;
    const unsigned long long *pe = (round & 1) ? P.exit_a : P.exit_b; // exits of round - 1
    unsigned long long *ce = (round & 1) ? P.exit_b : P.exit_a;       // exits of this round
    const unsigned base = j * (unsigned)S;
    unsigned long long st = pack_state(base, 0, 0); // the guess; the truth for j == 0
    if (round > 0) {
        if (j > 0) st = pe[i - 1]; // (same file: its block-in-MCU index is below this file's blocks per MCU)
        if (st == P.start_used[i]) { // nothing new: the exit stands
            ce[i] = pe[i];
            return;
        }
    }
    unsigned *row = rows[wave] + lane * SROW;
    stage_row(row, P.ecs + F.ecs_off + (size_t)j * (S / 8));
    unsigned p = (unsigned)st, nb = 0;
    int k = (int)((st >> 32) & 0xffu), b = (int)((st >> 40) & 0xffu);
    auto rd = [row](unsigned q) { return row[q]; };
    const HdFrameTabs &ft = P.ftabs[F.tabrec];
    spec_walk<true, false>(rd, row, &ft.spec[0][0][0], &ft.ovf[0][0], F.selmask, (int)F.blocks_per_mcu, base, p, k, b, nb);
    ce[i] = pack_state(p, k, b);
    P.start_used[i] = st;
    P.nblk[i] = nb;
}

// Exclusive scan of nblk inside every file (one workgroup per file).
__global__ __launch_bounds__(256) void k_hdm_scan(HdmParams P) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned carry_s;
    const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
    const HdmFileK &F = P.files[blockIdx.x];
    unsigned *d = P.nblk + F.sub0;
    const unsigned n = F.n_sub;
    if (lane == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < n; base += 256u) {
        const unsigned idx = base + (unsigned)lane;
        const unsigned v = idx < n ? d[idx] : 0u;
        unsigned incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(incl, o);
            if (wl >= o) incl += t;
        }
        if (wl == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned wbase = 0;
        for (int q = 0; q < wave; q++) wbase += wsum[q];
        const unsigned excl = carry_s + wbase + incl - v;
        if (idx < n) d[idx] = excl;
        __syncthreads();
        if (lane == 255) carry_s = excl + v;
        __syncthreads();
    }
    if (lane == 0 && carry_s < F.need) atomicOr(&P.status[blockIdx.x], 4u); // the stream ends before the file does
}

// The write pass.  A block belongs to the lane it STARTS in: that lane decodes on past the end of its subsequence (up to
// HDM_EXTRA more: 64 symbols of at most 32 bits) until the block ends, and a lane that starts in the middle of a block walks
// to its end without storing.  Coefficients are assembled in a 128-byte LDS buffer per lane and leave as whole blocks; the
// bits come straight from global memory, a dword per refill.  The per-symbol step is val_symbol of hvc_hdec_dev.h, the one
// k_hd_write2 takes; what differs is what surrounds it: no batching of block ends, a lane stores its own blocks.
__global__ __launch_bounds__(HDM_WG) void k_hdm_write(HdmParams P, int rounds) {
    __shared__ uint4 lbuf[HDM_WG * 8]; // 64 int16 per lane
    __shared__ HdmFileK Fs[HVC_HDM_GROUP]; // the units' files: what a lane indexes by component or block-in-MCU
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned unit = blockIdx.x * (unsigned)HVC_HDM_GROUP + (unsigned)wave;
    if (unit >= P.n_units) return; // (per wavefront; the kernel has no barrier: a wavefront reads its own LDS only)
    const unsigned f = unit_file(P, unit);
    if ((unsigned)lane < sizeof(HdmFileK) / 4u) reinterpret_cast<unsigned *>(&Fs[wave])[lane] = reinterpret_cast<const unsigned *>(&P.files[f])[lane];
#pragma unroll
    for (int q = 0; q < 8; q++) lbuf[tid * 8 + q] = make_uint4(0, 0, 0, 0);
    const HdmFileK &F = P.files[f]; // the wave-uniform fields: scalar loads
    const HdmFileK &G = Fs[wave];
    const unsigned j = (unit - F.unit0) * 64u + (unsigned)lane;
    if (j >= F.n_sub) return;
    const unsigned i = F.sub0 + j;
    const unsigned need = F.need, B = F.blocks_per_mcu, mbs_wide = F.mbs_wide, selmask = F.selmask;
    unsigned bi = P.nblk[i]; // the block this subsequence starts in
    if (bi >= need) return;  // past the last coded block: the model never reads this far
    const unsigned long long *fin = (rounds & 1) ? P.exit_a : P.exit_b; // round rounds - 1 wrote it
    const unsigned long long st = P.start_used[i], fin_i = fin[i];
    const unsigned base = j * (unsigned)S;
    int k = (int)((st >> 32) & 0xffu);
    unsigned b = (unsigned)((st >> 40) & 0xffu);
    // the hand-over: this lane started where its predecessor says it stopped (subsequence 0: at the file's first bit)
    if (st != (j ? fin[i - 1] : pack_state(0u, 0, 0)) || b != bi % B || (unsigned)st - base >= 32u || k > 63) {
        atomicOr(&P.status[f], 8u); // (MCU coordinates count from bi, the block-in-MCU index comes from the state: a lane
        return;                     // where they disagree must not store anything)
    }
    __builtin_amdgcn_wave_barrier(); // (the descriptor copy above and the reads below are this wavefront's own LDS traffic, in order)
    const unsigned *gbits = reinterpret_cast<const unsigned *>(P.ecs + F.ecs_off + (size_t)j * (S / 8));
    auto rd = [&](unsigned q) -> unsigned { return __builtin_bswap32(gbits[q]); };
    int16_t *const lb = reinterpret_cast<int16_t *>(lbuf + tid * 8);
    bool live = k == 0; // the block in progress is this lane's (it started here): its coefficients are stored, its errors count
    const unsigned mcu = bi / B;
    unsigned my = mcu / mbs_wide, mx = mcu - my * mbs_wide; // advance by counting
    uint4 *const recs = reinterpret_cast<uint4 *>(P.coefs + F.coef_base);
    auto block_at = [&](unsigned bb) -> uint4 * { // (bi < need: my is inside the MCU grid, which the plan keeps inside every plane)
        const unsigned comp = G.b2comp[bb];
        return recs + (G.coef_off[comp] >> 3) +
               ((size_t)(my * G.v[comp] + G.b2sy[bb]) * G.bw[comp] + (size_t)(mx * G.h[comp] + G.b2sx[bb])) * 8u;
    };
    const HdFrameTabs &ft = P.ftabs[F.tabrec];
    const uint16_t *const tvb = &ft.val[0][0][0];
    const HdOvf *const ovf = &ft.ovf[0][0];
    // the bit position as mm = ~(P + 31), P = bits consumed since the start of the lane's subsequence (see k_hd_write2)
    const unsigned p0 = (unsigned)st;
    unsigned mm = ~(p0 - base + 31u);
    const unsigned l0 = (p0 - base + 31u) >> 5;
    unsigned hi = l0 ? rd(l0 - 1u) : 0u, lo = rd(l0), nx = rd(l0 + 1u);
    const unsigned mm_limit = ~((unsigned)S + 31u), mm_hard = ~((unsigned)((HDM_EXTRA + 1) * S) + 31u);
    unsigned err = 0;
    bool crossed = false;
    const uint16_t *bt = tvb + ((selmask >> (2 * b)) & 3u) * (2 * SPEC_T);
    for (;;) {
        const unsigned w = __builtin_amdgcn_alignbit(hi, lo, mm); // the next 32 bits: a whole symbol
        const uint16_t *t = k ? bt + SPEC_T : bt;
        const HdSymbol sy = val_symbol(w, t, ovf, selmask, (int)b, k); // k_hd_write2's step (hvc_hdec_dev.h)
        const unsigned used = sy.used;
        const int mag = sy.mag, kn = sy.kn;
        const bool wrong = sy.wrong, end_block = sy.end_block;
        if (live) {
            if (wrong) err |= 1u;
            else lb[kn - 1] = (int16_t)mag; // (1 <= kn <= 64)
        }
        const unsigned mn = mm - used;
        if (((mn ^ mm) >> 5) != 0u) { // the window's first dword is used up
            hi = lo;
            lo = nx;
            nx = rd((31u - mn) >> 5);
        }
        mm = mn;
        const unsigned b1 = b + 1u == B ? 0u : b + 1u;
        bool stop = false;
        if (!crossed && mm <= mm_limit) { // the one symbol that takes the position across the subsequence's end: where the
            crossed = true;               // synchronisation walk of this subsequence stopped
            if (pack_state(base + ~mm - 31u, end_block ? 0 : kn, (int)(end_block ? b1 : b)) != fin_i) err |= 8u;
            if (!end_block && !live) stop = true; // a block in progress that is not this lane's (or nobody's: past the file)
        } else if (mm <= mm_hard) { // cannot happen: 64 symbols of <= 32 bits end a block
            err |= 1u;
            stop = true;
        }
        if (end_block) {
            if (live) { // the block is complete: it leaves whole, its DC difference once more where k_hdm_dc finds it
                uint4 *dst = block_at(b);
                P.dcd[(size_t)F.dcd0 + bi] = lb[0];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    dst[q] = lbuf[tid * 8 + q];
                    lbuf[tid * 8 + q] = make_uint4(0, 0, 0, 0);
                }
            }
            k = 0;
            b = b1;
            bi++;
            live = bi < need;
            bt = tvb + ((selmask >> (2 * b)) & 3u) * (2 * SPEC_T);
            if (b == 0u) { // next MCU
                mx++;
                if (mx == mbs_wide) {
                    mx = 0;
                    my++;
                }
            }
            if (crossed) stop = true; // the next block starts in another lane's subsequence
        } else {
            k = kn;
        }
        if (stop) break;
    }
    if (err) atomicOr(&P.status[f], err);
}

// DC differences -> DC values (decoder.ml:143): inclusive prefix sum over the component's blocks in scan order, one
// workgroup per (file, component), into the records.  A file whose verdict is already bad is skipped.
__global__ __launch_bounds__(256) void k_hdm_dc(HdmParams P) {
    __shared__ int wsum[4];
    __shared__ int carry_s;
    const unsigned f = blockIdx.x / 3u, comp = blockIdx.x - f * 3u;
    const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
    const HdmFileK &F = P.files[f];
    // (uniform, before any barrier: bits 0, 2 and 3 are final before this launch; bit 1 is what the workgroups of this launch
    // raise themselves, possibly while another component's reads the word)
    if (comp >= F.n_comp || (P.status[f] & 13u) != 0u) return;
    const unsigned h = F.h[comp], v = F.v[comp], bw = F.bw[comp], hv = h * v, B = F.blocks_per_mcu, mbs_wide = F.mbs_wide;
    const unsigned n = F.need / B * hv; // the component's blocks in this file
    int16_t *rec = P.coefs + F.coef_base + F.coef_off[comp];
    const int16_t *dcd = P.dcd + F.dcd0 + F.mcu_base[comp];
    if (lane == 0) carry_s = 0;
    __syncthreads();
    bool bad = false;
    constexpr int DC_E = 4;
    for (unsigned base = 0; base < n; base += 256u * DC_E) {
        int16_t *dcp[DC_E];
        int val[DC_E];
        int run = 0;
#pragma unroll
        for (int e = 0; e < DC_E; e++) {
            const unsigned o = base + (unsigned)lane * DC_E + (unsigned)e;
            dcp[e] = nullptr;
            val[e] = 0;
            if (o < n) {
                const unsigned m = o / hv, r = o - m * hv;
                const unsigned sy = r / h, sx = r - sy * h;
                const unsigned my = m / mbs_wide, mx = m - my * mbs_wide;
                dcp[e] = rec + ((size_t)(my * v + sy) * bw + (size_t)(mx * h + sx)) * 64;
                val[e] = dcd[(size_t)m * B + r];
            }
            run += val[e];
            val[e] = run; // inclusive prefix inside the lane's run
        }
        int incl = run;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int t = __shfl_up(incl, s);
            if (wl >= s) incl += t;
        }
        if (wl == 63) wsum[wave] = incl;
        __syncthreads();
        int wbase = 0;
        for (int q = 0; q < wave; q++) wbase += wsum[q];
        const int before = carry_s + wbase + incl - run; // everything in front of this lane's run
#pragma unroll
        for (int e = 0; e < DC_E; e++) {
            if (!dcp[e]) continue;
            const int dc = before + val[e];
            if (dc < -32768 || dc > 32767) bad = true;
            *dcp[e] = (int16_t)dc;
        }
        __syncthreads();
        if (lane == 255) carry_s = before + run;
        __syncthreads();
    }
    if (bad) atomicOr(&P.status[f], 2u);
}

hipError_t launch_hd_mixed(const HdmParams &P, hipStream_t s) {
    if (P.n_units == 0 || P.n_files == 0) return hipSuccess;
    const unsigned groups = (P.n_units + (unsigned)HVC_HDM_GROUP - 1u) / (unsigned)HVC_HDM_GROUP;
    for (int r = 0; r < HVC_HDM_ROUNDS; r++) hipLaunchKernelGGL(k_hdm_sync, dim3(groups), dim3(HDM_WG), 0, s, P, r);
    hipLaunchKernelGGL(k_hdm_scan, dim3(P.n_files), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_hdm_write, dim3(groups), dim3(HDM_WG), 0, s, P, HVC_HDM_ROUNDS);
    hipLaunchKernelGGL(k_hdm_dc, dim3(P.n_files * 3u), dim3(256), 0, s, P);
    return hipGetLastError();
}

} // namespace hvc
