/* hvc_hardcaml_spec.h -- the arithmetic of the Hardcaml RTL decoder's block datapath (k_hardcaml) AS DATA.
 *
 * The RTL (jpeg/hardcaml/src) does not compute the model's Chen-Wang IDCT.  Per 8x8 block it
 *   - takes the low 12 bits of each coefficient (codeblock_decoder.ml:14, 30, 224: a 12-bit bus and DC predictor);
 *   - dequantises d = sext12((q & 0xff) * c mod 4096) (dequant.ml:25-49: an 8-bit table entry, a 12-bit product),
 *     q indexed by zig-zag position, d placed at natural position Zigzag.inverse (dequant.ml:42-48);
 *   - runs Dct.Make(Idct_config) (dct.ml:24-33): T = C X rounded from 12 to 4 fractional bits (ties away from zero,
 *     wrapped to 19 bits), R = T C^T rounded by 16 bits (ties away from zero) and saturated to [-128, 127];
 *   - adds 128 (decoder_datapath.ml:187-188).
 * Two readers of this file: hvc_hardcaml.hip compiles the kernel from it, and tests/test_hardcaml_twin.py parses the
 * #defines and replays both passes on intervals (the proof that no int32 operation wraps and the 19-bit wrap of pass 1
 * is unreachable for every input).  Keep every value a plain integer expression of other names in this file.
 */
#ifndef HVC_HARDCAML_SPEC_H
#define HVC_HARDCAML_SPEC_H

/* Idct_config (dct.ml:24-33) */
#define HVC_HC_IN_BITS 12
#define HVC_HC_OUT_BITS 8
#define HVC_HC_ROM_PREC 12
#define HVC_HC_TRANSPOSE_PREC 4
#define HVC_HC_T_BITS (HVC_HC_IN_BITS + HVC_HC_TRANSPOSE_PREC + 3) /* transpose_bits: the width pass 1 wraps to */
#define HVC_HC_Q_BITS 8                                             /* the table RAM keeps element.:[7, 0] */

/* Dequantisation on packed halves: v_pk_mul_lo_u16 of the record's int16 pair with (q & 0xff) << QSHIFT gives
 * 16 * sext12(q * c mod 4096) as an int16 exactly (the product's low 12 bits land in the top 12 of the half), so no
 * masking or sign extension is needed; pass 1's rounding shift absorbs the factor 16. */
#define HVC_HC_QSHIFT 4
#define HVC_HC_P1_SHIFT (HVC_HC_ROM_PREC - HVC_HC_TRANSPOSE_PREC + HVC_HC_QSHIFT)
#define HVC_HC_P2_SHIFT (HVC_HC_ROM_PREC + HVC_HC_TRANSPOSE_PREC)
#define HVC_HC_LEVEL 128

/* C = round_nearest(4096 * M), M = the inverse matrix = the transpose of the x86 static forward matrix
 * (jpeg/model/src/dct.ml:255-346, dct.ml:75-83), row r = HVC_HC_ROM_R<r>.  Rows 7 - r are rows r with the odd
 * columns negated (C[7-r][k] = (-1)^k C[r][k]); the kernel reads rows 0-3 only and forms the others by the
 * butterfly: out[r] = E + O, out[7-r] = E - O, E = the even-column products, O = the odd-column ones. */
#define HVC_HC_ROM_R0 1448, 2009, 1892, 1703, 1448, 1138, 784, 400
#define HVC_HC_ROM_R1 1448, 1703, 784, -400, -1448, -2009, -1892, -1138
#define HVC_HC_ROM_R2 1448, 1138, -784, -2009, -1448, 400, 1892, 1703
#define HVC_HC_ROM_R3 1448, 400, -1892, -1138, 1448, 1703, -784, -2009
#define HVC_HC_ROM_R4 1448, -400, -1892, 1138, 1448, -1703, -784, 2009
#define HVC_HC_ROM_R5 1448, -1138, -784, 2009, -1448, -400, 1892, -1703
#define HVC_HC_ROM_R6 1448, -1703, 784, 400, -1448, 2009, -1892, 1138
#define HVC_HC_ROM_R7 1448, -2009, 1892, -1703, 1448, -1138, 784, -400

/* The schedule.  Pass 1, per column y, per r in 0..3 (v_dot2_i32_i16 on operand pairs of the column's entries):
 *     E = dot2((x0, x2), (C[r][0], C[r][2])) + dot2((x4, x6), (C[r][4], C[r][6]))
 *     O = dot2((x1, x3), (C[r][1], C[r][3])) + dot2((x5, x7), (C[r][5], C[r][7]))
 *     T[r][y] = RND(E + O, P1_SHIFT), T[7-r][y] = RND(E - O, P1_SHIFT)
 * Pass 2, per row x, per r in 0..3 (v_mul_i32_i24 / v_mad_i32_i24: |T| < 2^23, |C| < 2^11):
 *     E = T[x][0] C[r][0] + T[x][2] C[r][2] + T[x][4] C[r][4] + T[x][6] C[r][6],  O likewise over the odd k
 *     pixel[x][r] = SAT_U8(RND(E + O, P2_SHIFT) + LEVEL), pixel[x][7-r] = SAT_U8(RND(E - O, P2_SHIFT) + LEVEL)
 * RND(v, p) = (v + 2^(p-1) + (v >> 31)) >> p: round half away from zero (Hardcaml_fixed_point tie_away_from_zero);
 * for pass 2 the level shift rides in the addend (LEVEL << P2_SHIFT) and v_ashr_pk_u8_i32 shifts and saturates to
 * [0, 255] = [-128, 127] + 128 in one instruction. */

#endif /* HVC_HARDCAML_SPEC_H */
