/* hvc_islow_spec.h -- the arithmetic of k_islow (hvc_libjpeg.hip; hvc_set_arithmetic HVC_ARITH_LIBJPEG) AS DATA: the
 * 8 x 8 inverse DCT of libjpeg's jidctint.c ("islow"), stated in include/hvc_jpeg.h ("Bit-exact to libjpeg") and restated
 * in numpy in tools/libjpeg_reference.py.
 *
 * One list of operations describes the one-dimensional step.  Two readers:
 *   - hvc_libjpeg.hip expands HVC_ISLOW_STEP into the statements of the int path's step and, at compile time, into the
 *     8 x 8 integer matrix its int64 path multiplies by (every other block): the kernel's arithmetic IS this list;
 *   - tests/test_islow_guard.py parses THIS FILE (the #defines and the list) and replays the operations on linear forms:
 *     the proof that the int path cannot overflow under the guard below is a proof about the code that ships.
 * Keep every value a plain integer: the parser evaluates nothing else.
 *
 * Notation: d[k] = coefficient * table entry at natural position k = 8 * row + col; D(x, n) = (x + 2^(n-1)) >> n. */
#ifndef HVC_ISLOW_SPEC_H
#define HVC_ISLOW_SPEC_H

/* jidctint.c: FIX(x) = round(x * 2^13) */
#define HVC_IS_CONST_BITS 13
#define HVC_IS_FIX_0_298631336 2446
#define HVC_IS_FIX_0_390180644 3196
#define HVC_IS_FIX_0_541196100 4433
#define HVC_IS_FIX_0_765366865 6270
#define HVC_IS_FIX_0_899976223 7373
#define HVC_IS_FIX_1_175875602 9633
#define HVC_IS_FIX_1_501321110 12299
#define HVC_IS_FIX_1_847759065 15137
#define HVC_IS_FIX_1_961570560 16069
#define HVC_IS_FIX_2_053119869 16819
#define HVC_IS_FIX_2_562915447 20995
#define HVC_IS_FIX_3_072711026 25172

/* Pass 1 runs down the eight columns of d and descales by PASS1_SHIFT into the workspace; pass 2 runs along the eight rows
 * of the workspace and descales by PASS2_SHIFT; the sample is clamp(x + LEVEL, 0, 255).  The int path folds pass 2's
 * rounding and the level shift into one addend, (1 << (PASS2_SHIFT - 1)) + (LEVEL << PASS2_SHIFT), and lets the saturating
 * pack shift (v_add3_u32 + v_ashr_pk_u8_i32). */
#define HVC_IS_PASS1_SHIFT 11
#define HVC_IS_PASS2_SHIFT 18
#define HVC_IS_LEVEL 128

/* The guard of the int path:  S = SUM over all 64 positions of |d[k]|  <=  HVC_IS_GUARD_SUM  (S is evaluated exactly as
 * SUM |coefficient| * table entry, saturating at 2^32 - 1).  Every value of a step is a linear combination of the step's
 * eight inputs, so under  SUM |v[i]| <= s  its magnitude is at most (largest |weight|) * s.  Pass 1: column c has s = S_c
 * with SUM S_c = S, so every value is within W1 * S and the workspace within (A * S_c + 2^10) / 2^11, A the largest output
 * weight.  Pass 2: a row's inputs are one workspace entry per column, so a value with weights k[c] is within
 * max |k| * A * S / 2^11 + SUM |k| / 2.  tests/test_islow_guard.py evaluates these bounds for every operation of the list:
 * under the guard no int32 value wraps, every multiplicand fits the 24 signed bits of v_mul_i32_i24, and every d[k] fits
 * int16 (|d[k]| <= S), which is what makes the v_pk_mul_lo_u16 dequantisation exact.  The first bound to give way is the
 * sum q2 = w2 + w3 of pass 2, whose weight on v3 is -20995 - 16069 + 9633 = -27431 (14109 would still pass).  Ordinary files stay far inside: S of a photograph's block is a few
 * thousand, a DC of 8 * 1023 included. */
#define HVC_IS_GUARD_SUM 14000

/* The step on v0 .. v7.  MUL(d, a, k): d = a * k (k a constant of this file, sign given);  ADD / SUB(d, a, b): d = a +- b;
 * SHL(d, a, n): d = a * 2^n;  OUTADD / OUTSUB(i, a, b): result i = a +- b, descaled by the pass. */
#define HVC_ISLOW_STEP(MUL, ADD, SUB, SHL, OUTADD, OUTSUB)                                                              \
    ADD(e26, v2, v6)  MUL(z1, e26, HVC_IS_FIX_0_541196100)                                                              \
    MUL(m6, v6, HVC_IS_FIX_1_847759065)  SUB(tmp2, z1, m6)  MUL(m2, v2, HVC_IS_FIX_0_765366865)  ADD(tmp3, z1, m2)      \
    ADD(e04, v0, v4)  SUB(f04, v0, v4)  SHL(tmp0, e04, HVC_IS_CONST_BITS)  SHL(tmp1, f04, HVC_IS_CONST_BITS)            \
    ADD(t10, tmp0, tmp3)  SUB(t13, tmp0, tmp3)  ADD(t11, tmp1, tmp2)  SUB(t12, tmp1, tmp2)                              \
    ADD(y1, v7, v1)  ADD(y2, v5, v3)  ADD(y3, v7, v3)  ADD(y4, v5, v1)  ADD(y34, y3, y4)                                \
    MUL(z5, y34, HVC_IS_FIX_1_175875602)                                                                                \
    MUL(a0, v7, HVC_IS_FIX_0_298631336)  MUL(a1, v5, HVC_IS_FIX_2_053119869)                                            \
    MUL(a2, v3, HVC_IS_FIX_3_072711026)  MUL(a3, v1, HVC_IS_FIX_1_501321110)                                            \
    MUL(w1, y1, -HVC_IS_FIX_0_899976223)  MUL(w2, y2, -HVC_IS_FIX_2_562915447)                                          \
    MUL(p3, y3, -HVC_IS_FIX_1_961570560)  MUL(p4, y4, -HVC_IS_FIX_0_390180644)                                          \
    ADD(w3, p3, z5)  ADD(w4, p4, z5)                                                                                    \
    ADD(q0, w1, w3)  ADD(q1, w2, w4)  ADD(q2, w2, w3)  ADD(q3, w1, w4)                                                  \
    ADD(b0, a0, q0)  ADD(b1, a1, q1)  ADD(b2, a2, q2)  ADD(b3, a3, q3)                                                  \
    OUTADD(0, t10, b3)  OUTADD(1, t11, b2)  OUTADD(2, t12, b1)  OUTADD(3, t13, b0)                                      \
    OUTSUB(4, t13, b0)  OUTSUB(5, t12, b1)  OUTSUB(6, t11, b2)  OUTSUB(7, t10, b3)

#endif /* HVC_ISLOW_SPEC_H */
