// Host driver of egogaussian_amd/csrc/det_accum.h for tests/test_det_accum_cpu.py: the functions the backward blend runs on the device,
// compiled by the host compiler.
//   det_accum_host abi                 prints EGS_ABI_VERSION and EGS_CALL_DETERMINISTIC as the header defines them
//   det_accum_host sum FILE N K        FILE holds K arrays of N float32 each (K orderings of one set of partials); per array one line
//                                      "max_bits sum decoded_bits": the maximum of the |partial| bit patterns, the int64 sum of the encoded
//                                      partials added in the array's order, the bit pattern of the decoded float32
//   det_accum_host repeat BITS COUNT   COUNT partials, all the float32 with bit pattern BITS: the same line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/egs_raster.h"
#include "../egogaussian_amd/csrc/det_accum.h"

static void report(uint32_t max_bits, int64_t sum) {
    const float f = egs_det_decode(sum, max_bits);
    uint32_t fb; memcpy(&fb, &f, 4);
    printf("%u %lld %u\n", max_bits, (long long)sum, fb);
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "abi")) { printf("%d %d\n", EGS_ABI_VERSION, EGS_CALL_DETERMINISTIC); return 0; }
    if (argc == 4 && !strcmp(argv[1], "repeat")) {
        const uint32_t bits = (uint32_t)strtoul(argv[2], nullptr, 10); const long count = atol(argv[3]);
        float v; memcpy(&v, &bits, 4);
        const uint32_t mb = egs_det_abs_bits(v);
        int64_t sum = 0;
        for (long i = 0; i < count; i++) sum += egs_det_encode(v, mb);
        report(mb, sum);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "sum")) {
        const size_t n = (size_t)atol(argv[3]), k = (size_t)atol(argv[4]);
        std::vector<float> x(n * k);
        FILE* f = fopen(argv[2], "rb");
        if (!f || fread(x.data(), sizeof(float), n * k, f) != n * k) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        fclose(f);
        for (size_t a = 0; a < k; a++) {
            const float* p = x.data() + a * n;
            uint32_t mb = 0;                                         // pass 1: the integer maximum of the bit patterns
            for (size_t i = 0; i < n; i++) { const uint32_t b = egs_det_abs_bits(p[i]); mb = b > mb ? b : mb; }
            int64_t sum = 0;                                         // pass 2: the integer sum, in the array's order
            for (size_t i = 0; i < n; i++) sum += egs_det_encode(p[i], mb);
            report(mb, sum);
        }
        return 0;
    }
    fprintf(stderr, "usage: det_accum_host abi | sum FILE N K | repeat BITS COUNT\n");
    return 2;
}
