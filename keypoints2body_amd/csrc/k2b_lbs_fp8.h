// k2b_lbs_fp8.h — the e4m3 correction operands of the SMPL stream kernel's pose phase (k2b_lbs_stream.hip, description SmplF8;
// DESIGN.md 4.2).  v_posed * kPdScale = X . Pd is X_hi . Pd_hi + X_hi . Pd_lo + X_lo . Pd_hi over f16 hi / lo terms; the two
// correction products are 2^-11 of the first and need three or four correct bits, so for the k-steps 0..5 they run as ONE
// block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 per pair of k-steps, into the same accumulator.  Pure functions, no HIP call:
// the encoder is shared by the pose set-up kernel (X side), the image builder (k2b_model_tables.h, Pd side) and the host tests.
//
// The instruction's K = 128 is four blocks of 32 with one power-of-two scale (E8M0 byte) per block and operand.  Lane (row,
// g = lane / 16) holds 32 bytes; bytes 0..15 of the lane groups 0, 1 are block 0, of the groups 2, 3 block 1, bytes 16..31 of the
// groups 0, 1 block 2, of the groups 2, 3 block 3, and the scale of block b is the one lane group b supplies.  A k-step's e4m3
// strip takes the place of its f16 lo strip, 16 bytes per lane like it, so the first 16 bytes of a lane come from the even k-step
// of a pair and the last 16 from the odd one:
//   X  strip of a k-step, lane group g:  0: X_hi8[k 0..15]   1: X_hi8[k 16..31]   2: X_lo8[k 0..15]   3: X_lo8[k 16..31]
//   Pd strip of a k-step, lane group g:  0: Pd_lo8[k 0..15]  1: Pd_lo8[k 16..31]  2: Pd_hi8[k 0..15]  3: Pd_hi8[k 16..31]
// so the blocks 0 and 2 are X_hi8 . Pd_lo8 and the blocks 1 and 3 X_lo8 . Pd_hi8 of the two k-steps, and a lane of group g
// supplies the scales of (g & 1 ? X_lo8, Pd_hi8 : X_hi8, Pd_lo8).  The last k-step (6: the last pose features, the shape
// coefficients and the template, whose lo terms are not small against 5e-6 m) keeps its three f16 products: it has no partner,
// and a half-empty K = 128 instruction costs what its two f16 corrections cost.
#pragma once
#include <stdint.h>

#include "k2b_layout.h"

namespace k2b {

constexpr int kF8PoseSteps = 6;      // 32-deep k-steps whose strips are e4m3 (three pairs); the features from 32 x 6 on keep f16
constexpr int kF8XHiExp = -4;        // X_hi8 = e4m3(X_hi * 2^4): |X_hi| <= 28 before it saturates (rotation entries: <= 2)
constexpr int kF8XLoExp = -15;       // X_lo8 = e4m3(X_lo * 2^15): |X_lo| <= 2^-11 |X_hi|

// exact 2^e, -126 <= e <= 127
constexpr float f8_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }

// fp32 -> OCP e4m3fn (bias 7, no infinities, 0x7f / 0xff NaN, largest finite 448 = 0x7e), round to nearest even, saturating:
// everything beyond 448, the infinities included, becomes +-448; NaN stays NaN.
constexpr uint8_t e4m3_encode(float x) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, x);
    const uint8_t sign = (uint8_t)((bits >> 24) & 0x80);
    const uint32_t mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) return (uint8_t)(sign | 0x7f);
    if (mag >= 0x43e00000u) return (uint8_t)(sign | 0x7e);                    // |x| >= 448
    if (mag < 0x3c800000u) {                                                  // |x| < 2^-6: subnormal codes, units of 2^-9
        const float t = __builtin_bit_cast(float, mag) * 512.0f;              // exact, in [0, 8)
        uint32_t q = (uint32_t)t;
        const float frac = t - (float)q;
        if (frac > 0.5f || (frac == 0.5f && (q & 1))) ++q;                    // q == 8 is the code of 2^-6 itself
        return (uint8_t)(sign | q);
    }
    uint32_t r = mag >> 20;                                                   // exponent | three mantissa bits
    const uint32_t rem = mag & 0xfffffu;
    if (rem > 0x80000u || (rem == 0x80000u && (r & 1))) ++r;                  // a carry runs into the exponent by itself
    const uint32_t code = r - ((127 - 7) << 3);
    return (uint8_t)(sign | (code > 0x7e ? 0x7e : code));
}
constexpr float e4m3_decode(uint8_t c) {
    const int e = (c >> 3) & 15, m = c & 7;
    const float s = (c & 0x80) ? -1.f : 1.f;
    if (e == 15 && m == 7) return __builtin_bit_cast(float, 0x7fc00000u);
    if (e == 0) return s * (float)m * f8_pow2(-9);
    return s * (1.f + (float)m * 0.125f) * f8_pow2(e - 7);
}
// x / 2^exp as e4m3 (the division is exact)
constexpr uint8_t e4m3_encode_scaled(float x, int exp) { return e4m3_encode(x * f8_pow2(-exp)); }
constexpr float e4m3_decode_scaled(uint8_t c, int exp) { return e4m3_decode(c) * f8_pow2(exp); }

// The power-of-two scale of an operand whose largest magnitude is max_abs: the smallest exponent e with max_abs / 2^e <= 448,
// so that nothing saturates and the largest values keep their three mantissa bits; kept inside +-60 (0 for an all-zero operand).
constexpr int e4m3_scale_exp(float max_abs) {
    if (!(max_abs > 0.f)) return 0;
    int e = -60;
    while (e < 60 && max_abs * f8_pow2(-e) > 448.f) ++e;
    return e;
}
// the E8M0 byte of the instruction's scale operand
constexpr int e8m0(int exp) { return exp + 127; }

// X side: the two codes of one feature value (what the pose set-up stores; the f16 split is the one of the three-product form)
struct XCodes { uint8_t hi8, lo8; };
constexpr XCodes x_fp8_codes(k2b_half hi, k2b_half lo) {
    return XCodes{e4m3_encode_scaled((float)hi, kF8XHiExp), e4m3_encode_scaled((float)lo, kF8XLoExp)};
}
}  // namespace k2b
