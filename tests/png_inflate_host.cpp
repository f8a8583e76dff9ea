// Host program around egogaussian_amd/csrc/png_inflate.h -- the very header the device inflater includes -- for tests/test_png_decode_cpu.py,
// which builds it with -fsanitize=address,undefined.
//   png_inflate_host IN OUT
// IN:  records of  u32 n, u32 expect, n bytes of a zlib stream.
// OUT: per record  u32 status, u32 produced, u64 loop iterations, then -- for status 0 -- the `expect` inflated bytes.
// Stream and output live in heap blocks of exactly n and expect bytes: a read or a write one byte outside is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../egogaussian_amd/csrc/png_inflate.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: png_inflate_host IN OUT\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    PngiMem* mem = new PngiMem;
    uint32_t hdr[2];
    size_t records = 0;
    while (fread(hdr, 4, 2, fi) == 2) {
        const uint32_t n = hdr[0], expect = hdr[1];
        uint8_t* in = (uint8_t*)malloc(n ? n : 1);
        uint8_t* out = (uint8_t*)malloc(expect ? expect : 1);
        if (n && fread(in, 1, n, fi) != n) { fprintf(stderr, "short record\n"); return 2; }
        if (!n) { free(in); in = (uint8_t*)malloc(0); }                  // (a zero-byte block: any read is out of bounds)
        memset(mem, 0xA5, sizeof(PngiMem));                             // nothing may depend on what the tables held before
        PngiState s;
        s.in = in; s.n = n; s.out = out; s.expect = expect; s.m = mem;
        pngi_inflate(s);
        const uint32_t res[2] = {s.status, s.outpos};
        const uint64_t it = s.iters;
        fwrite(res, 4, 2, fo);
        fwrite(&it, 8, 1, fo);
        if (!s.status) fwrite(out, 1, expect, fo);
        free(in);
        free(out);
        records++;
    }
    delete mem;
    fclose(fi);
    if (fclose(fo)) return 2;
    printf("%zu records\n", records);
    return 0;
}
