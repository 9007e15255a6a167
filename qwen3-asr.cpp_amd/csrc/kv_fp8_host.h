// kv_fp8_host.h -- the conversion rule of the FP8 shadow KV cache (option kv_fp8), stated once: the
// rule in full and a plain reference of it, pure C++ with no device code.  kv_fp8.hip's kernels are held to it bit
// for bit (tests/test_gpu_kv_fp8_kernel.py, against torch's float8_e4m3fn conversion on the CPU).
//
// The rule.  x is an fp16 element of the K or V cache, s the context's exponent (option kv_fp8_exp, -8 .. 8):
//     q = RNE_E4M3FN(clamp(x * 2^s, -448, 448))
//   * x * 2^s is exact in fp32 (an fp16 value times a power of two; the smallest, 2^-24 * 2^-8, is a normal fp32).
//   * E4M3FN is OCP FP8 E4M3: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; 0x7f / 0xff are the NaNs;
//     the largest value is 448 (0x7e), the smallest normal 2^-6, subnormals k * 2^-9 (k = 1 .. 7).
//   * RNE: round to the nearest code, a value half way between two codes to the one with an even mantissa.  Below
//     2^-10 the result is (signed) zero; 2^-10 itself is the tie between 0 and 2^-9 and goes to 0.
//   * NaN stays NaN (the clamp does not apply to it): code 0x7f | sign.
// The value the attention uses is float(q) * 2^-s.  It is an fp16 value for every code and |s| <= 8 (a normal code has
// four significant bits; the smallest subnormal, 2^-9 * 2^-8 = 2^-17, is a multiple of fp16's 2^-24) with one
// exception: at s = -8 an |x| >= 63488 rounds to the code of 256, and 256 * 2^8 = 65536 is past fp16's 65504.  The
// packed hardware conversion then yields infinity; keys of that size with s = -8 are outside what the option serves.
#pragma once
#include <cmath>
#include <cstdint>

namespace qasr {

constexpr int kKvFp8ExpMin = -8, kKvFp8ExpMax = 8;
constexpr float kE4m3Max = 448.0f;

// RNE_E4M3FN(clamp(v, -448, 448)) of an fp32 value (reference; the kernels use v_cvt_pk_fp8_f32)
inline uint8_t e4m3fn_from_float(float v) {
    const uint8_t sign = std::signbit(v) ? 0x80 : 0;
    if (std::isnan(v)) return sign | 0x7f;
    const float a = std::fmin(std::fabs(v), kE4m3Max);
    if (a < 0x1p-6f) return sign | (uint8_t)std::nearbyint(a * 0x1p9f);   // subnormals and zero: multiples of 2^-9 (8 -> 2^-6)
    int e;
    const float m = std::frexp(a, &e);                                     // a = m * 2^e, m in [0.5, 1)
    const int k = (int)std::nearbyint(m * 16.0f);                          // 8 .. 16 (16: carries into the next binade)
    const int E = k == 16 ? e + 7 : e + 6, M = k == 16 ? 0 : k - 8;        // biased exponent of 2^(e - 1) is e + 6
    return sign | (uint8_t)(E << 3 | M);
}

inline float e4m3fn_to_float(uint8_t q) {
    const int E = q >> 3 & 15, M = q & 7;
    if (E == 15 && M == 7) return NAN;
    const float a = E ? std::ldexp(1.0f + M / 8.0f, E - 7) : std::ldexp((float)M, -9);
    return q & 0x80 ? -a : a;
}

// the rule on one cache element given as its fp32 value (exact: every fp16 is an fp32)
inline uint8_t kv_fp8_quant(float x, int s) { return e4m3fn_from_float(std::ldexp(x, s)); }
// the value the attention uses
inline float kv_fp8_dequant(uint8_t q, int s) { return std::ldexp(e4m3fn_to_float(q), -s); }

}  // namespace qasr
