// hvc_dct_fixed.hip -- gfx950 kernels of the model's parametric fixed-point DCT (Dct.Fixed_point, dct.ml:443-482), its
// float64 reference (Dct.Floating_point.Eight_point, fmul) and the precision search of jpeg/bin/dct.ml: bit exact for every
// accepted (rom_prec, transpose_prec) and input (hvc_dct_spec.h; tests/test_dct_fixed_point.py proves the widths).
//
// Arithmetic per lane, one 8x8 block: the 64 inputs stay in VGPRs as int32 and the output is made row by row -- row r
// of T needs all of X but only row r of C, and row r of Y only row r of T -- so no more than 8 values of T are live.
// Every product is v_mad_i64_i32 of an int32 value with a ROM entry: the ROM of a pass is one precision for the whole
// wave, so its entries are scalar loads.  Rounding (ties away from zero) is sign, magnitude, add half, shift, sign.
// The float64 reference is the same row order with __dmul_rn / __dadd_rn, summed from 0.0 in the order of fmul; the
// Makefile builds this file with -ffp-contract=off (hipcc's default fuses them into FMAs, pragma or not).  Why not MFMA: K is 8, the sums need 43 bits exactly, and a matrix op would have to split every
// operand; the VALU form is exact with no fix-up.
//
// k_dct_search: lanes = generated blocks, grid y = chunks of DCT_SEARCH_CFGS configurations.  A lane generates its
// block once and runs it through every configuration of its chunk; the round trip keeps the forward result while the
// forward parameters repeat (the search's order changes them every 54 configurations).  Per configuration the wave
// reduces (error, block) to its best -- larger error, then smaller block index -- and lane 0 folds that into its
// wave's LDS slot; at the end the workgroup folds its four waves and writes one slot per configuration, and
// k_dct_search_reduce folds the workgroup columns.  The fold is exact and order free, so the result is the same for
// any grid and any split of the block range.  Nothing is read from memory but the tables; the slots are the only
// writes besides the result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvc_dct_fixed.h"

#pragma clang fp contract(off)

namespace hvc {

namespace {

struct Shift {
    int l, r;
    long long h;
};
// round_matrix by p (dct.ml:459-467): p > 0 rounds ties away from zero, p < 0 shifts left, 0 is the identity
__device__ inline Shift shift_of(int p) { return p > 0 ? Shift{0, p, 1ll << (p - 1)} : Shift{-p, 0, 0ll}; }
__device__ inline long long rnd(long long x, Shift s) {
    const long long g = x >> 63;
    long long m = (x ^ g) - g;
    m = ((m << s.l) + s.h) >> s.r;
    return (m ^ g) - g;
}

// C[r][k] of the forward ROM, or of the inverse ROM (its transpose)
template <bool INV> __device__ inline int coef(const int32_t *__restrict__ rom, int r, int k) {
    return INV ? rom[k * 8 + r] : rom[r * 8 + k];
}

// Fixed_point.transform: out(r, c, Y[r][c]) for every output, row by row
template <bool INV, class Out>
__device__ inline void fixed_rows(const int32_t *x, const int32_t *__restrict__ rom, int rom_prec, int tp, Out out) {
    const Shift s1 = shift_of(rom_prec - tp), s2 = shift_of(rom_prec + tp);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int32_t t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            long long a = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) a += (long long)coef<INV>(rom, r, j) * x[j * 8 + k];
            t[k] = (int32_t)rnd(a, s1);
        }
#pragma unroll
        for (int c = 0; c < 8; c++) {
            long long a = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) a += (long long)t[k] * coef<INV>(rom, c, k);
            out(r, c, (int32_t)rnd(a, s2));
        }
    }
}

// fmul (fmul F X) F^T in float64, F = M (forward) or M^T (inverse): out(r, c, R[r][c]), row by row
template <bool INV, class Out> __device__ inline void reference_rows(const int32_t *x, const double *__restrict__ m, Out out) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
        double b[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 8; j++) s = __dadd_rn(s, __dmul_rn(INV ? m[j * 8 + r] : m[r * 8 + j], (double)x[j * 8 + k]));
            b[k] = s;
        }
#pragma unroll
        for (int c = 0; c < 8; c++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) s = __dadd_rn(s, __dmul_rn(b[k], INV ? m[k * 8 + c] : m[c * 8 + k]));
            out(r, c, s);
        }
    }
}

__device__ inline bool better(unsigned long long ka, unsigned long long ia, unsigned long long kb, unsigned long long ib) {
    return ka > kb || (ka == kb && ia < ib);
}

__global__ __launch_bounds__(256) void k_dct_fixed(const DctTables *__restrict__ tab, int inverse, int rom_prec, int tp,
                                                   const int32_t *__restrict__ in, int32_t *__restrict__ out,
                                                   size_t n_blocks, unsigned *bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks) return;
    const int32_t *src = in + i * 64;
    int32_t x[64];
    const int lim = inverse ? HVC_DCT_INV_IN_MAX : HVC_DCT_FWD_IN_MAX;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        x[j] = src[j];
        ok &= x[j] >= -lim && x[j] <= lim;
    }
    if (!ok) {
        atomicOr(bad, 1u);
        return;
    }
    int32_t *dst = out + i * 64;
    auto store = [&](int r, int c, int32_t v) { dst[r * 8 + c] = v; };
    if (inverse) fixed_rows<true>(x, tab->rom[rom_prec], rom_prec, tp, store);
    else fixed_rows<false>(x, tab->rom[rom_prec], rom_prec, tp, store);
}

__global__ __launch_bounds__(256) void k_dct_reference(const DctTables *__restrict__ tab, int inverse,
                                                       const int32_t *__restrict__ in, double *__restrict__ out,
                                                       size_t n_blocks) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks) return;
    const int32_t *src = in + i * 64;
    int32_t x[64];
#pragma unroll
    for (int j = 0; j < 64; j++) x[j] = src[j];
    double *dst = out + i * 64;
    auto store = [&](int r, int c, double v) { dst[r * 8 + c] = v; };
    if (inverse) reference_rows<true>(x, tab->m, store);
    else reference_rows<false>(x, tab->m, store);
}

template <int MODE>
__global__ __launch_bounds__(DCT_SEARCH_WG) void k_dct_search(const DctTables *__restrict__ tab,
                                                              const DctCfg *__restrict__ cfg, int n_cfg, uint64_t seed,
                                                              int range, uint64_t first, uint64_t n_blocks,
                                                              DctWorst *__restrict__ slab) {
    constexpr int WAVES = DCT_SEARCH_WG / 64;
    __shared__ DctWorst best[WAVES][DCT_SEARCH_CFGS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * DCT_SEARCH_CFGS, cn = min(DCT_SEARCH_CFGS, n_cfg - c0);
    for (int i = threadIdx.x; i < WAVES * DCT_SEARCH_CFGS; i += DCT_SEARCH_WG) best[i / DCT_SEARCH_CFGS][i % DCT_SEARCH_CFGS] = {0ull, ~0ull};
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * DCT_SEARCH_WG;
    for (uint64_t base = (uint64_t)blockIdx.x * DCT_SEARCH_WG; base < n_blocks; base += stride) {
        const uint64_t b = base + threadIdx.x;
        const bool valid = b < n_blocks;
        const uint64_t idx = first + b;
        int32_t x[64], y[64];
        dct_block(seed, range, idx, x);
        int y_rom = -1, y_tp = -1; // the forward parameters y holds (round trip)
        for (int ci = 0; ci < cn; ci++) {
            const DctCfg c = cfg[c0 + ci];
            double err;
            if constexpr (MODE == 2) {
                if (c.fwd_rom != y_rom || c.fwd_tp != y_tp) {
                    fixed_rows<false>(x, tab->rom[c.fwd_rom], c.fwd_rom, c.fwd_tp,
                                      [&](int r, int k, int32_t v) { y[r * 8 + k] = v; });
                    y_rom = c.fwd_rom;
                    y_tp = c.fwd_tp;
                }
                int e = 0;
                fixed_rows<true>(y, tab->rom[c.inv_rom], c.inv_rom, c.inv_tp,
                                 [&](int r, int k, int32_t v) { e = max(e, abs(x[r * 8 + k] - v)); });
                err = (double)e;
            } else {
                double e = 0.0;
                auto cmp = [&](int r, int k, double v) { e = fmax(e, fabs(__dsub_rn((double)y[r * 8 + k], v))); };
                if constexpr (MODE == 0) {
                    fixed_rows<false>(x, tab->rom[c.fwd_rom], c.fwd_rom, c.fwd_tp,
                                      [&](int r, int k, int32_t v) { y[r * 8 + k] = v; });
                    reference_rows<false>(x, tab->m, cmp);
                } else {
                    fixed_rows<true>(x, tab->rom[c.inv_rom], c.inv_rom, c.inv_tp,
                                     [&](int r, int k, int32_t v) { y[r * 8 + k] = v; });
                    reference_rows<true>(x, tab->m, cmp);
                }
                y_rom = y_tp = -1;
                err = e;
            }
            unsigned long long key = valid ? (unsigned long long)__double_as_longlong(err) : 0ull;
            unsigned long long id = valid ? idx : ~0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long k2 = __shfl_xor(key, o), i2 = __shfl_xor(id, o);
                if (better(k2, i2, key, id)) {
                    key = k2;
                    id = i2;
                }
            }
            if (lane == 0 && better(key, id, best[wave][ci].key, best[wave][ci].idx)) best[wave][ci] = {key, id};
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < cn; t += DCT_SEARCH_WG) {
        DctWorst w = best[0][t];
#pragma unroll
        for (int v = 1; v < WAVES; v++)
            if (better(best[v][t].key, best[v][t].idx, w.key, w.idx)) w = best[v][t];
        slab[(size_t)(c0 + t) * gridDim.x + blockIdx.x] = w;
    }
}

__global__ __launch_bounds__(256) void k_dct_search_reduce(const DctWorst *__restrict__ slab, int n_cfg, int cols,
                                                           DctWorst *__restrict__ worst) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cfg) return;
    DctWorst w = {0ull, ~0ull};
    for (int x = 0; x < cols; x++) {
        const DctWorst s = slab[(size_t)c * cols + x];
        if (better(s.key, s.idx, w.key, w.idx)) w = s;
    }
    worst[c] = w;
}

} // namespace

hipError_t launch_dct_fixed(const DctTables *tab, int inverse, int rom, int tp, const int32_t *in, int32_t *out,
                            size_t n_blocks, unsigned *bad, hipStream_t s) {
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dct_fixed, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, s, tab, inverse, rom, tp, in,
                       out, n_blocks, bad);
    return hipGetLastError();
}

hipError_t launch_dct_reference(const DctTables *tab, int inverse, const int32_t *in, double *out, size_t n_blocks,
                                hipStream_t s) {
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dct_reference, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, s, tab, inverse, in, out,
                       n_blocks);
    return hipGetLastError();
}

// Workgroup columns: about 4096 workgroups in all (eight rounds of the 512 that fit at two waves per SIMD), never more
// columns than the blocks fill.
size_t dct_search_grid_x(uint64_t n_blocks, int n_cfg) {
    const uint64_t rows = (uint64_t)(n_cfg + DCT_SEARCH_CFGS - 1) / DCT_SEARCH_CFGS;
    const uint64_t need = (n_blocks + DCT_SEARCH_WG - 1) / DCT_SEARCH_WG;
    uint64_t cols = (4096 + rows - 1) / rows;
    if (cols > need) cols = need;
    return (size_t)(cols ? cols : 1);
}

hipError_t launch_dct_search(const DctTables *tab, int mode, const DctCfg *cfg, int n_cfg, uint64_t seed, int range,
                             uint64_t first, uint64_t n_blocks, DctWorst *slab, DctWorst *worst, hipStream_t s,
                             hipEvent_t k0, hipEvent_t k1) {
    if (n_cfg <= 0 || n_blocks == 0) return hipSuccess;
    const unsigned cols = (unsigned)dct_search_grid_x(n_blocks, n_cfg);
    const unsigned rows = (unsigned)((n_cfg + DCT_SEARCH_CFGS - 1) / DCT_SEARCH_CFGS);
    hipError_t e;
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    const dim3 grid(cols, rows);
    if (mode == 0) hipLaunchKernelGGL(k_dct_search<0>, grid, dim3(DCT_SEARCH_WG), 0, s, tab, cfg, n_cfg, seed, range, first, n_blocks, slab);
    else if (mode == 1) hipLaunchKernelGGL(k_dct_search<1>, grid, dim3(DCT_SEARCH_WG), 0, s, tab, cfg, n_cfg, seed, range, first, n_blocks, slab);
    else hipLaunchKernelGGL(k_dct_search<2>, grid, dim3(DCT_SEARCH_WG), 0, s, tab, cfg, n_cfg, seed, range, first, n_blocks, slab);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dct_search_reduce, dim3((unsigned)((n_cfg + 255) / 256)), dim3(256), 0, s, slab, n_cfg,
                       (int)cols, worst);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc
