// divmagic.h — division by a per-launch constant as one multiply-high and one shift.
//
// The conv kernels turn an output row m into (image, row in image, y, x) by dividing by P*Q, Q and a pyramid level's width:
// constants of the launch. A 32-bit integer division is ~37 instructions on the device (there is no divide instruction); with
// the multiplier and the shift worked out once on the host it is three.
//
//   l   = ceil(log2 d)                      (0 for d = 1)
//   mul = ceil(2^(31 + l) / d)              in [2^31, 2^32): fits 32 bits, since d > 2^(l - 1) (or d = 2^l: mul = 2^31)
//   n / d = ((2 n * mul) >> 32) >> l        = floor(n * mul / 2^(31 + l))
//
// PROVEN RANGE: exact for every dividend 0 <= n < 2^31 and every divisor 1 <= d < 2^31.
//   Let e = mul * d - 2^(31 + l), 0 <= e < d <= 2^l. Then n * mul / 2^(31 + l) = n / d + n * e / (d * 2^(31 + l)), and the second
//   term is below 1 / d because n * e < 2^31 * 2^l: adding it to n / d = q + r / d (r <= d - 1) cannot reach q + 1.
//   2 n < 2^32 does not overflow the 32-bit operand of the multiply-high.
// Launches whose dividends could leave that range are refused on the host (divmagic_make returns false; launch_conv and
// launch_bneck return hipErrorInvalidValue): there is no slower fall-back.
//
// No HIP dependency: tests/test_conv_divmagic.py compiles this header into a stand-alone host program.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YH_DIVMAGIC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define YH_DIVMAGIC_FN inline
#endif

namespace yh {

struct DivMagic { uint32_t mul, shift; };

constexpr int64_t kDivMagicLimit = (int64_t)1 << 31;   // dividends and divisors stay below this

// false: d is outside [1, 2^31) - the caller refuses the launch
inline bool divmagic_make(int64_t d, DivMagic* out) {
    if (d < 1 || d >= kDivMagicLimit) return false;
    uint32_t l = 0;
    while (((int64_t)1 << l) < d) ++l;
    const uint64_t two = (uint64_t)1 << (31 + l);
    out->mul = (uint32_t)((two + (uint64_t)d - 1) / (uint64_t)d);
    out->shift = l;
    return true;
}

// n / d for 0 <= n < 2^31
YH_DIVMAGIC_FN uint32_t divmagic_div(uint32_t n, const DivMagic dm) {
    return (uint32_t)(((uint64_t)(n << 1) * dm.mul) >> 32) >> dm.shift;
}

}  // namespace yh
