// hvc_scaled_spec.h -- the reduced-size inverse DCT (decode at 1/2, 1/4, 1/8: N = 4, 2, 1 samples per block side): its
// constants, the guard of k_decode_scaled's int32 path, and the launcher's prototype.  The definition itself is stated
// in include/hvc_jpeg.h and restated in numpy in tools/scaled_reference.py; tests/test_scaled_guard.py reads the
// numbers below and proves the guard by interval arithmetic over both passes.
//
// Notation: d[k] = coefficient * table entry at natural position k = 8 * row + col (always an int32: 32768 * 65535 <
// 2^31); D(x, n) = (x + 2^(n-1)) >> n.  A one-dimensional step takes a vector v[0..7].
#ifndef HVC_SCALED_SPEC_H
#define HVC_SCALED_SPEC_H

/* N = 4: t0 = v0 << 14; t2 = C4_V2 v2 - C4_V6 v6; t10 = t0 + t2; t12 = t0 - t2;
 * o0 = -C4_O0_V7 v7 + C4_O0_V5 v5 - C4_O0_V3 v3 + C4_O0_V1 v1;  o2 = -C4_O2_V7 v7 - C4_O2_V5 v5 + C4_O2_V3 v3 + C4_O2_V1 v1;
 * results D(t10 + o2, sh) D(t12 + o0, sh) D(t12 - o0, sh) D(t10 - o2, sh); columns 0 1 2 3 5 6 7 with sh = 12, then the four
 * rows of the workspace with sh = 19. */
#define HVC_S4_V0_SHIFT 14
#define HVC_S4_V2 15137
#define HVC_S4_V6 6270
#define HVC_S4_O0_V7 1730
#define HVC_S4_O0_V5 11893
#define HVC_S4_O0_V3 17799
#define HVC_S4_O0_V1 8697
#define HVC_S4_O2_V7 4176
#define HVC_S4_O2_V5 4926
#define HVC_S4_O2_V3 7373
#define HVC_S4_O2_V1 20995
#define HVC_S4_PASS1_SHIFT 12
#define HVC_S4_PASS2_SHIFT 19

/* N = 2: t10 = v0 << 15; t0 = -C2_V7 v7 + C2_V5 v5 - C2_V3 v3 + C2_V1 v1; results D(t10 + t0, sh) D(t10 - t0, sh);
 * columns 0 1 3 5 7 with sh = 13, then the two rows of the workspace with sh = 20. */
#define HVC_S2_V0_SHIFT 15
#define HVC_S2_V7 5906
#define HVC_S2_V5 6967
#define HVC_S2_V3 10426
#define HVC_S2_V1 29692
#define HVC_S2_PASS1_SHIFT 13
#define HVC_S2_PASS2_SHIFT 20

/* N = 1: D(d[0], 3): no pass, no guard. */
#define HVC_S1_SHIFT 3

/* The guard of the int32 path.  With  DC = |d[0]|  and  AC = max |d[k]| over the other positions the definition uses
 * (N = 4: rows and columns 0 1 2 3 5 6 7; N = 2: rows and columns 0 1 3 5 7), a block takes the int32 path when
 *         WD * DC + WA * AC <= LIMIT        (evaluated without overflow: 64-bit, or after DC, AC <= 2^31)
 * and the int64 path (same lane, same formulas) otherwise.  Where the numbers come from, N = 4: column 0 of pass 1 is at
 * most 16384 DC + 61526 AC + 2^11 in magnitude, every other column 77910 AC + 2^11 (the sums of the absolute constants);
 * after >> 12 the workspace holds at most 4 DC + 15.03 AC + 0.5 in column 0 and 19.03 AC + 0.5 elsewhere, and a row of
 * pass 2 at most 16384 * column 0 + 61526 * the others + 2^18 -- a linear form in DC and AC whose coefficients, rounded up,
 * are WD and WA, and whose constant part is what LIMIT leaves below 2^31 - 1.  N = 2 alike.  The guard admits every block
 * with max |d[k]| <= 1448 (N = 4) / 2391 (N = 2), the crude bound of equal DC and AC, and a DC of ordinary files (up to
 * 8 * 2^10) beside AC terms up to about 1100 / 1400.  Under the guard every multiplicand of both passes also fits 24
 * signed bits, which is what lets the int32 path multiply with v_mul_i32_i24. */
#define HVC_S4_GUARD_WD 65536u
#define HVC_S4_GUARD_WA 1416390u
#define HVC_S4_GUARD_LIMIT 2147182548u /* 2^31 - 1 - 301099 */
#define HVC_S2_GUARD_WD 131072u
#define HVC_S2_GUARD_WA 766708u
#define HVC_S2_GUARD_LIMIT 2146916479u /* 2^31 - 1 - 567168 */

#ifdef __cplusplus
#include "hvc_kernels.h"
namespace hvc {
// k_decode_scaled over the geometry of a DecodeParams whose comp[].plane_off / .stride describe the SCALED planes (bw * N
// bytes per row, bh * N rows).  n = 4, 2 or 1.  dwords: every row of every plane of every frame starts on a 4-byte
// boundary (base, frame stride, plane offsets, strides): neighbouring lanes' samples leave as one dword; otherwise byte
// stores.  P.dc_plane selects the instantiation that takes the DC from the compact array.  P.wide_total (cleared by the
// caller) receives the number of blocks that took the int64 path.  k0 / k1 (optional): events around the kernel.
hipError_t launch_decode_scaled(const DecodeParams &P, int n, bool dwords, hipStream_t s, hipEvent_t k0 = nullptr,
                                hipEvent_t k1 = nullptr);
} // namespace hvc
#endif

#endif
