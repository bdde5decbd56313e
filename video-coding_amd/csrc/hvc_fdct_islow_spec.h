/* hvc_fdct_islow_spec.h -- the arithmetic of k_fdct_islow (hvc_libjpeg_encode.hip; hvc_set_encode_libjpeg) AS DATA: the
 * 8 x 8 forward DCT of libjpeg's jfdctint.c ("islow"), stated in include/hvc_jpeg.h ("Encoding bit-exact to libjpeg").
 *
 * One list of operations describes the one-dimensional step.  Three readers:
 *   - hvc_fdct_islow_dev.h expands HVC_FDCT_ISLOW_STEP into the statements of the kernel's step: the kernel's arithmetic IS
 *     this list;
 *   - tools/libjpeg_encode_reference.py parses THIS FILE (the #defines and the list) and replays the operations on numpy
 *     int64 arrays: the definition tests/test_libjpeg_encode_reference.py holds against libjpeg-turbo;
 *   - tests/test_fdct_islow_bounds.py replays them on intervals: the proof that no int32 value wraps, that every
 *     multiplicand fits the 24 signed bits of v_mul_i32_i24, and of the largest |t| the quantiser sees.
 * Keep every value a plain integer: the parsers evaluate nothing else.
 *
 * Notation: D(x, n) = (x + 2^(n-1)) >> n (arithmetic shift). */
#ifndef HVC_FDCT_ISLOW_SPEC_H
#define HVC_FDCT_ISLOW_SPEC_H

/* jfdctint.c: FIX(x) = round(x * 2^13) */
#define HVC_FI_CONST_BITS 13
#define HVC_FI_PASS1_BITS 2
#define HVC_FI_FIX_0_298631336 2446
#define HVC_FI_FIX_0_390180644 3196
#define HVC_FI_FIX_0_541196100 4433
#define HVC_FI_FIX_0_765366865 6270
#define HVC_FI_FIX_0_899976223 7373
#define HVC_FI_FIX_1_175875602 9633
#define HVC_FI_FIX_1_501321110 12299
#define HVC_FI_FIX_1_847759065 15137
#define HVC_FI_FIX_1_961570560 16069
#define HVC_FI_FIX_2_053119869 16819
#define HVC_FI_FIX_2_562915447 20995
#define HVC_FI_FIX_3_072711026 25172

/* The samples go in as p - LEVEL.  Pass 1 runs along the eight rows of the block, pass 2 down the eight columns of pass 1's
 * results.  The results 0 and 4 of a step carry no constant (OUTLO): pass 1 scales them up by PASS1_BITS, x << 2, pass 2
 * takes it off again, D(x, 2).  The other six (OUTHI) are D(x, CONST_BITS - PASS1_BITS) = D(x, 11) in pass 1 and
 * D(x, CONST_BITS + PASS1_BITS) = D(x, 15) in pass 2.  The output is the DCT scaled by 8. */
#define HVC_FI_LEVEL 128
#define HVC_FI_PASS1_LO_SHL 2
#define HVC_FI_PASS1_HI_SHIFT 11
#define HVC_FI_PASS2_LO_SHIFT 2
#define HVC_FI_PASS2_HI_SHIFT 15

/* What tests/test_fdct_islow_bounds.py proves for samples in 0..255 and asserts to be these very numbers: the largest |t|
 * a step hands on after pass 2, and with the largest divisor 8 * 255 the largest numerator |t| + 4 q of the quantiser.
 * hvc_libjpeg_encode_plan.cpp's division magics are exhausted up to HVC_FI_T_MAX (tests/host_harness). */
#define HVC_FI_T_MAX 8192
#define HVC_FI_Q_MAX 255

/* The step on v0 .. v7.  MUL(d, a, k): d = a * k (k a constant of this file, sign given);  ADD / SUB(d, a, b): d = a +- b;
 * OUTLO(i, a) / OUTHI(i, a): result i = a, scaled as the pass says above. */
#define HVC_FDCT_ISLOW_STEP(MUL, ADD, SUB, OUTLO, OUTHI)                                                                \
    ADD(tmp0, v0, v7)  SUB(tmp7, v0, v7)  ADD(tmp1, v1, v6)  SUB(tmp6, v1, v6)                                          \
    ADD(tmp2, v2, v5)  SUB(tmp5, v2, v5)  ADD(tmp3, v3, v4)  SUB(tmp4, v3, v4)                                          \
    ADD(tmp10, tmp0, tmp3)  SUB(tmp13, tmp0, tmp3)  ADD(tmp11, tmp1, tmp2)  SUB(tmp12, tmp1, tmp2)                      \
    ADD(s0, tmp10, tmp11)  OUTLO(0, s0)  SUB(s4, tmp10, tmp11)  OUTLO(4, s4)                                            \
    ADD(e23, tmp12, tmp13)  MUL(z1, e23, HVC_FI_FIX_0_541196100)                                                        \
    MUL(m13, tmp13, HVC_FI_FIX_0_765366865)  ADD(s2, z1, m13)  OUTHI(2, s2)                                             \
    MUL(m12, tmp12, -HVC_FI_FIX_1_847759065)  ADD(s6, z1, m12)  OUTHI(6, s6)                                            \
    ADD(y1, tmp4, tmp7)  ADD(y2, tmp5, tmp6)  ADD(y3, tmp4, tmp6)  ADD(y4, tmp5, tmp7)  ADD(y34, y3, y4)                \
    MUL(z5, y34, HVC_FI_FIX_1_175875602)                                                                                \
    MUL(a4, tmp4, HVC_FI_FIX_0_298631336)  MUL(a5, tmp5, HVC_FI_FIX_2_053119869)                                        \
    MUL(a6, tmp6, HVC_FI_FIX_3_072711026)  MUL(a7, tmp7, HVC_FI_FIX_1_501321110)                                        \
    MUL(w1, y1, -HVC_FI_FIX_0_899976223)  MUL(w2, y2, -HVC_FI_FIX_2_562915447)                                          \
    MUL(p3, y3, -HVC_FI_FIX_1_961570560)  MUL(p4, y4, -HVC_FI_FIX_0_390180644)                                          \
    ADD(w3, p3, z5)  ADD(w4, p4, z5)                                                                                    \
    ADD(b7, a4, w1)  ADD(s7, b7, w3)  OUTHI(7, s7)                                                                      \
    ADD(b5, a5, w2)  ADD(s5, b5, w4)  OUTHI(5, s5)                                                                      \
    ADD(b3, a6, w2)  ADD(s3, b3, w3)  OUTHI(3, s3)                                                                      \
    ADD(b1, a7, w1)  ADD(s1, b1, w4)  OUTHI(1, s1)

#endif /* HVC_FDCT_ISLOW_SPEC_H */
