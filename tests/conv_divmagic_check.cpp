// Stand-alone check of csrc/divmagic.h (tests/test_conv_divmagic.py compiles and runs it; it may also be built by hand with
// -fsanitize=address,undefined). Reads "divisor rows" pairs from the command line; for each, compares divmagic_div with / and %
// for EVERY dividend 0 <= n < rows, and at the top of the proven range.
#include <cstdio>
#include <cstdlib>

#include "divmagic.h"

int main(int argc, char** argv) {
    using namespace yh;
    long long checked = 0;
    DivMagic dm;
    // refused divisors: 0, negative, 2^31 and beyond
    const long long bad[] = { 0, -1, -324, kDivMagicLimit, kDivMagicLimit + 1, (long long)1 << 40 };
    for (long long d : bad)
        if (divmagic_make(d, &dm)) { std::printf("FAIL: divisor %lld was not refused\n", d); return 1; }
    for (int a = 1; a + 1 < argc; a += 2) {
        const long long d = std::atoll(argv[a]), rows = std::atoll(argv[a + 1]);
        if (rows < 1 || rows > kDivMagicLimit) { std::printf("FAIL: rows %lld outside the proven range\n", rows); return 1; }
        if (!divmagic_make(d, &dm)) { std::printf("FAIL: divisor %lld refused\n", d); return 1; }
        if (dm.mul < 0x80000000u || dm.shift > 31) { std::printf("FAIL: divisor %lld: mul %u shift %u\n", d, dm.mul, dm.shift); return 1; }
        const uint32_t ud = (uint32_t)d;
        for (uint32_t n = 0; n < (uint32_t)rows; ++n) {
            const uint32_t q = divmagic_div(n, dm);
            if (q != n / ud || n - q * ud != n % ud) { std::printf("FAIL: %u / %u = %u, got %u\n", n, ud, n / ud, q); return 1; }
        }
        // the last dividends of the proven range, and those around the multiples of d just below it
        for (uint32_t k = 0; k < 4096; ++k) {
            const uint32_t top = 0x7FFFFFFFu - k, edge = (0x7FFFFFFFu / ud) * ud;
            const uint32_t probe[] = { top, edge >= k ? edge - k : 0u, edge + k <= 0x7FFFFFFFu ? edge + k : 0x7FFFFFFFu };
            for (uint32_t n : probe)
                if (divmagic_div(n, dm) != n / ud) { std::printf("FAIL: %u / %u = %u, got %u\n", n, ud, n / ud, divmagic_div(n, dm)); return 1; }
        }
        checked += rows;
    }
    std::printf("ok: %d divisors, %lld dividends\n", (argc - 1) / 2, checked);
    return 0;
}
