// det_accum.h -- order-independent accumulation of float32 partial sums (EGS_CALL_DETERMINISTIC, include/egs_raster.h).
// Plain C++: the backward blend (render_bwd.hip) and a host program (tests/test_det_accum_cpu.py) compile the same functions.
//
// A (Gaussian, value) pair receives up to 4 partials per tile from the quadrant-waves of the backward blend, in an order that differs from
// run to run.  Float addition does not associate, integer addition does: every partial is rounded ONCE to a multiple of a quantum the whole
// pair shares, the multiples are added as int64, and the sum is turned into a float32 once.
//   max_bits  the largest float_bits(|partial|) of the pair (a first pass gathers it with an integer atomic max: the bit patterns of
//             non-negative floats order like the floats, NaN above Inf above every finite value).
//   e         the exponent of that maximum, 2^e <= max < 2^(e+1); -126 for a denormal maximum.
//   quantum   q = 2^(e - 38) <= 2^-38 max.  Every |partial| <= max < 2^(e+1), so |partial / q| < 2^39.
//   overflow  an image has at most EGS_MAX_TILES = 36 864 tiles and a Gaussian at most 4 quadrant-waves in each: at most 147 456 < 2^18
//             partials per pair, |sum| < 2^57 -- int64 cannot overflow.
//   error     each partial is off by at most q / 2 and the conversion of the sum rounds once: |decoded - exact| <= N q / 2 + ulp / 2.
//             Partials below 2^(e - 14) lose bits to q; the float32 chain this replaces rounds its running sum to ulp(sum) at every step.
//   zero      max_bits == 0: every partial was +-0 -> 0.
//   non-finite max_bits >= 0x7f800000 (an Inf or NaN partial): nothing is converted to an integer, the pair decodes to NaN.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGS_DET_HD __host__ __device__ inline
#else
#define EGS_DET_HD inline
#endif

#define EGS_DET_QUANTUM_SHIFT 38          // q = 2^(e - 38)
#define EGS_DET_NONFINITE 0x7f800000u     // max_bits at or above this: the pair saw an Inf or a NaN

EGS_DET_HD uint32_t egs_det_abs_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u & 0x7fffffffu; }
// the biased exponent the pair scales by (1 for a denormal maximum: its quantum is the smallest normal binade's)
EGS_DET_HD int egs_det_biased_exp(uint32_t max_bits) { const int be = (int)(max_bits >> 23); return be < 1 ? 1 : be; }
// 2^k as a float64, for -1022 <= k <= 1023
EGS_DET_HD double egs_det_pow2(int k) { const uint64_t b = (uint64_t)(1023 + k) << 52; double d; memcpy(&d, &b, 8); return d; }

// partial / q, rounded to the nearest integer (ties to even).  0 for a pair that cannot be summed (zero or non-finite maximum) and for a
// partial that does not belong to it (non-finite, or so far above the maximum that the bound on the sum would not hold).
EGS_DET_HD int64_t egs_det_encode(float partial, uint32_t max_bits) {
    if (max_bits == 0u || max_bits >= EGS_DET_NONFINITE) return 0;
    const int e = egs_det_biased_exp(max_bits) - 127;
    const double scaled = (double)partial * egs_det_pow2(EGS_DET_QUANTUM_SHIFT - e);      // exact: a power of two, well inside float64's range
    if (!(scaled < 1099511627776.0 && scaled > -1099511627776.0)) return 0;              // 2^40; also catches NaN
    // round to nearest even without a library call: adding 1.5 * 2^52 leaves the integer in the low mantissa bits (|scaled| < 2^51)
    const double magic = 6755399441055744.0;
    const double r = scaled + magic;
    int64_t bits; memcpy(&bits, &r, 8);
    int64_t magic_bits; memcpy(&magic_bits, &magic, 8);
    return bits - magic_bits;
}

// sum * q as a float32, rounded once
EGS_DET_HD float egs_det_decode(int64_t sum, uint32_t max_bits) {
    if (max_bits >= EGS_DET_NONFINITE) { const uint32_t n = 0x7fc00000u; float f; memcpy(&f, &n, 4); return f; }
    if (max_bits == 0u || sum == 0) return 0.f;
    const int e = egs_det_biased_exp(max_bits) - 127;
    const bool neg = sum < 0;
    uint64_t m = neg ? (uint64_t)0 - (uint64_t)sum : (uint64_t)sum;
    int shift = 0;
    if (m >> 53) { m = (m >> 8) | ((m & 0xffu) ? 1u : 0u); shift = 8; }                 // keep the float64 exact: the dropped bits only matter as "not zero" (sticky)
    const double mag = (double)(int64_t)m * egs_det_pow2(e - EGS_DET_QUANTUM_SHIFT + shift);   // exact (<= 53 significant bits, exponent in range)
    return (float)(neg ? -mag : mag);                                                     // the one rounding (to nearest even; Inf if the sum exceeds float32)
}
