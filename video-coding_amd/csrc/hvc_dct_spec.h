/* hvc_dct_spec.h -- the storage widths of the parametric fixed-point DCT (k_dct_fixed, k_dct_search) AS DATA.
 *
 * The arithmetic is the model's Dct.Fixed_point.transform (jpeg/model/src/dct.ml:443-482) for any accepted
 * (rom_prec, transpose_prec):
 *   C = round_nearest(M * 2^rom_prec), M the static x86 forward matrix (its transpose for the inverse direction);
 *   T = round_matrix(C X, rom_prec - transpose_prec);   Y = round_matrix(T C^T, rom_prec + transpose_prec);
 *   round_matrix by p > 0 rounds ties away from zero, by p < 0 shifts left, by 0 is the identity.
 * Every product and every sum of a pass is an int64 (v_mad_i64_i32 of two int32 operands); what the kernels keep
 * between passes is narrower: the input X, the rounded T and the output Y are int32.  tests/test_dct_fixed_point.py
 * parses these #defines and proves, from the row absolute sums of each ROM, that every accumulator fits int64 and that
 * X, T and Y fit int32 for every accepted parameter and input.  Keep every value a plain integer expression.
 */
#ifndef HVC_DCT_SPEC_H
#define HVC_DCT_SPEC_H

#define HVC_DCT_ROM_PREC_MAX 16      /* 0 <= rom_prec <= 16 */
#define HVC_DCT_TP_MAX 8             /* 0 <= transpose_prec <= 8 */
#define HVC_DCT_FWD_IN_MAX 2048      /* |x| <= 2048 into the forward transform */
#define HVC_DCT_INV_IN_MAX 32768     /* |x| <= 32768 into the inverse: the largest |Y| of any accepted forward call */
#define HVC_DCT_ACC_BITS 64          /* both passes accumulate in int64 */
#define HVC_DCT_STORE_BITS 32        /* X, T and Y are kept as int32 */

#endif
