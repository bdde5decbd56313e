/* hvc_hardcaml_fwd_spec.h -- the arithmetic of the Hardcaml RTL encoder's block datapath (k_hardcaml_encode) AS DATA.
 *
 * The finished half of jpeg/hardcaml's encoder datapath (encoder_datapath.ml) per 8x8 block of a component plane:
 *   - X = p - 128 (encoder_datapath.ml:67);
 *   - Dct.Make(Dct_config) (dct.ml:13-22): T = C X rounded from 12 to 4 fractional bits (ties away from zero, wrapped to
 *     15 bits), R = T C^T rounded by 16 bits (ties away from zero, a 30-bit accumulator) and saturated to [-2048, 2047];
 *   - quant.ml: q = wrap12(RND(R * (4096 / t), 12)), the quantiser RAM holding one_over_quant_coef t = 4096 / t.
 * Coefficient k (natural order) goes to record position Zigzag.forward[k] and is divided by t = table[Zigzag.forward[k]]:
 * the zig-zag table convention of DQT and of the model's Encoder.quant (encoder.ml:103-108).
 * Two readers of this file: hvc_hardcaml.hip compiles the kernel from it, and tests/test_hardcaml_encoder_twin.py parses
 * the #defines and replays the schedule on intervals (the proof that no int32 / i24 operand overflows and that the 15-bit
 * wrap, the 30-bit accumulator, the 12-bit saturation and the 12-bit quantiser wrap are unreachable for 8-bit pixels).
 * Keep every value a plain integer expression of other names in this file.
 */
#ifndef HVC_HARDCAML_FWD_SPEC_H
#define HVC_HARDCAML_FWD_SPEC_H

/* Dct_config (dct.ml:13-22) and quant.ml */
#define HVC_HCE_IN_BITS 8
#define HVC_HCE_OUT_BITS 12
#define HVC_HCE_ROM_PREC 12
#define HVC_HCE_TRANSPOSE_PREC 4
#define HVC_HCE_T_BITS (HVC_HCE_IN_BITS + HVC_HCE_TRANSPOSE_PREC + 3)  /* transpose_bits: the width pass 1 wraps to */
#define HVC_HCE_MAC_BITS (HVC_HCE_T_BITS + HVC_HCE_ROM_PREC + 3)       /* mac_bits: pass 2's accumulator */
#define HVC_HCE_QUANT_COEF_BITS 13                                    /* quant.ml: the RAM's 13-bit reciprocals */
#define HVC_HCE_QR_NUM (1 << (HVC_HCE_QUANT_COEF_BITS - 1))           /* one_over_quant_coef t = QR_NUM / t */
#define HVC_HCE_LEVEL 128

#define HVC_HCE_P1_SHIFT (HVC_HCE_ROM_PREC - HVC_HCE_TRANSPOSE_PREC)
#define HVC_HCE_P2_SHIFT (HVC_HCE_ROM_PREC + HVC_HCE_TRANSPOSE_PREC)
#define HVC_HCE_Q_SHIFT (HVC_HCE_QUANT_COEF_BITS - 1)
/* the kernel multiplies by the reciprocal << QR_SCALE and rounds by Q_SHIFT + QR_SCALE = 16 bits: the quotient is then
 * the high half of the rounded product (one v_perm_b32 packs two), and the result is the same for every R (the product
 * is a multiple of 2^QR_SCALE, so the negative addend 2^15 - 1 rounds as 2^11 - 1 does) */
#define HVC_HCE_QR_SCALE 4
#define HVC_HCE_QZ_SHIFT (HVC_HCE_Q_SHIFT + HVC_HCE_QR_SCALE)

/* C = round_nearest(4096 * F), F = the x86 static forward matrix (jpeg/model/src/dct.ml:255-346), row u = HVC_HCE_ROM_R<u>:
 * the transpose of hvc_hardcaml_spec.h's inverse ROM.  C[u][7 - x] = (-1)^u C[u][x]: the kernel uses columns 0-3 only,
 * even rows against x + (7 - x) sums, odd rows against x - (7 - x) differences. */
#define HVC_HCE_ROM_R0 1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448
#define HVC_HCE_ROM_R1 2009, 1703, 1138, 400, -400, -1138, -1703, -2009
#define HVC_HCE_ROM_R2 1892, 784, -784, -1892, -1892, -784, 784, 1892
#define HVC_HCE_ROM_R3 1703, -400, -2009, -1138, 1138, 2009, 400, -1703
#define HVC_HCE_ROM_R4 1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448
#define HVC_HCE_ROM_R5 1138, -2009, 400, 1703, -1703, -400, 2009, -1138
#define HVC_HCE_ROM_R6 784, -1892, 1892, -784, -784, 1892, -1892, 784
#define HVC_HCE_ROM_R7 400, -1138, 1703, -2009, 2009, -1703, 1138, -400

/* The schedule.  Pass 1, per column y, on the raw pixels p (v_perm_b32 gathers two rows' bytes as an unsigned int16 pair,
 * v_pk_add_u16 / v_pk_sub_u16 form the butterfly):
 *     S0 = (p[0][y] + p[7][y], p[1][y] + p[6][y])   S1 = (p[2][y] + p[5][y], p[3][y] + p[4][y])   in [0, 510]
 *     D0 = (p[0][y] - p[7][y], p[1][y] - p[6][y])   D1 = (p[2][y] - p[5][y], p[3][y] - p[4][y])   in [-255, 255]
 *     even u: v = dot2(S1, (C[u][2], C[u][3]), dot2(S0, (C[u][0], C[u][1]), -LEVEL * 2 * (C[u][0] + .. + C[u][3])))
 *     odd u:  v = dot2(D1, (C[u][2], C[u][3]), dot2(D0, (C[u][0], C[u][1]), 0))
 * (the level shift cancels in the differences and rides in the accumulator for the sums), then
 *     w = v + 2^(P1_SHIFT - 1) + (v >> 31)   and T[u][y] = w >> P1_SHIFT = bytes 1-2 of w, which v_perm_b32 packs.
 * Pass 2, per row u, on int16 pairs of T (v_pk_add_u16 / v_pk_sub_u16):
 *     E0 = (T[u][0] + T[u][7], T[u][1] + T[u][6])   E1 = (T[u][2] + T[u][5], T[u][3] + T[u][4])   O0, O1 the differences
 *     even v: v2 = dot2(E1, (C[v][2], C[v][3]), dot2(E0, (C[v][0], C[v][1]), 0));  odd v: the same on O0, O1
 *     R[u][v] = RND(v2, P2_SHIFT)
 * Quantiser (v_mul_i32_i24, |R| < 2^23, QR16 = (QR_NUM / t) << QR_SCALE < 2^23):
 *     z = R * QR16 + 2^(QZ_SHIFT - 1) + (R >> 31),  q = z >> QZ_SHIFT = the high half of z, packed in zig-zag pairs
 * RND(v, p) = (v + 2^(p-1) + (v >> 31)) >> p: round half away from zero (Hardcaml_fixed_point tie_away_from_zero, and
 * quant.ml's round). */

#endif /* HVC_HARDCAML_FWD_SPEC_H */
