// png_common.h -- what the PNG encoder (png.hip) and the PNG decoder (png_decode.hip) share: the Paeth predictor and the arithmetic that
// combines the CRC-32 of slices (a lane's CRC times x^(8 n) mod P, n the bytes behind its slice).
#pragma once
#include <stdint.h>

#define PNG_POLY 0xedb88320u

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// a * b mod P over GF(2), reflected (bit 31 is x^0), as zlib's multmodp; 32 steps whatever the operands
__device__ __forceinline__ uint32_t png_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return p;
}
