// hvc_normalize_lut.cpp -- behind hvc_normalize_lut (include/hvc_jpeg.h, Typed output; the entry point is in hvc_yuv.hip): the
// table that turns an 8-bit sample into the element a model reads, ((float)v / 255.0f - mean[c]) / std[c] in IEEE single with one rounding per operation -- torchvision's
// ToTensor() followed by Normalize(mean, std) on the CPU -- and for the 16-bit types one round-to-nearest-even conversion of
// that.  Host only, plain C++ (no HIP), compiled with -ffp-contract=off: a fused multiply-add or a reciprocal in place of a
// division changes the last bit.  The conversions are written out on the bits, so that no compiler flag or library decides them.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/hvc_jpeg.h"

namespace {

uint32_t bits_of(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// IEEE single -> half, round to nearest even; overflow to infinity, subnormals kept, NaN stays a (quiet) NaN
uint16_t to_f16(float v) {
    const uint32_t u = bits_of(v);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t mag = u & 0x7FFFFFFFu;
    if (mag >= 0x7F800000u) return (uint16_t)(sign | (mag > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (mag >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);           // >= 2^16: beyond the rounding of the largest half
    if (mag < 0x33000000u) return sign;                                  // < 2^-25: rounds to zero (2^-25 itself: the tie, to even = 0)
    uint32_t man = (mag & 0x007FFFFFu) | 0x00800000u;                    // 24 bits with the hidden one
    const int e = (int)(mag >> 23) - 127;                                // value = man * 2^(e - 23)
    // half: normal for e >= -14 (10 fraction bits: drop 13), subnormal below (units of 2^-24: drop -e - 1 bits, 14 .. 24)
    const int drop = e >= -14 ? 13 : -e - 1;
    const uint32_t kept = man >> drop, rest = man & ((1u << drop) - 1), half = 1u << (drop - 1);
    uint32_t r = kept + ((rest > half || (rest == half && (kept & 1u))) ? 1u : 0u);
    // normal: r holds the hidden bit at 2^10, so adding (e + 14) << 10 gives exponent field e + 15 and a carry moves it up by
    // itself; subnormal: r is the fraction, and a carry into 2^10 is the smallest normal
    if (e >= -14) r += (uint32_t)(e + 14) << 10;
    return (uint16_t)(sign | r);                                         // (r <= 0x7C00: 65520 and above went out before)
}

// IEEE single -> bfloat16, round to nearest even; NaN stays a (quiet) NaN
uint16_t to_bf16(float v) {
    const uint32_t u = bits_of(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

} // namespace

namespace hvc {

int normalize_lut(const float *mean, const float *std, int elem, void *lut) {
    if (!mean || !std || !lut) return HVC_E_INVALID_ARG;
    if (elem != HVC_ELEM_F32 && elem != HVC_ELEM_F16 && elem != HVC_ELEM_BF16) return HVC_E_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f) return HVC_E_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        for (int v = 0; v < 256; v++) {
            const float x = (float)v / 255.0f;
            const float y = x - mean[c];
            const float z = y / std[c];
            const size_t at = (size_t)c * 256 + (size_t)v;
            if (elem == HVC_ELEM_F32)
                static_cast<float *>(lut)[at] = z;
            else
                static_cast<uint16_t *>(lut)[at] = elem == HVC_ELEM_F16 ? to_f16(z) : to_bf16(z);
        }
    return HVC_OK;
}

} // namespace hvc
