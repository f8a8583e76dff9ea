// Host program around egogaussian_amd/csrc/png_segments.h -- the very header the device kernels include -- for tests/test_png_segments_cpu.py,
// which builds it with -fsanitize=address,undefined.  It emulates the three passes of the segmented route chunk by chunk, runs the serial
// inflater over the same stream, and holds the route to its one promise: a file it accepts is one pngi_inflate accepts, with the same
// bytes and the same Adler-32.
//   png_segments_host IN OUT
// IN:  records of  u32 expect, u32 chunks, per chunk (u32 length, u32 CRC flag), then the stream (the chunks' bytes in order).
// OUT: per record  u32 route word, u32 serial status, then -- for route 1 -- the `expect` bytes the placement pass wrote.
// A chunk's wave gets the stream up to the chunk's end in a heap block of exactly that size (streams up to 64 KiB), and the placement pass
// an output block of exactly `expect` bytes: a read or a write one byte outside is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../egogaussian_amd/csrc/png_segments.h"

static int fail(size_t record, const char* what) {
    fprintf(stderr, "record %zu: %s\n", record, what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: png_segments_host IN OUT\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    PngsMem* mem = new PngsMem;
    PngiMem* big = new PngiMem;
    uint32_t hdr[2];
    size_t records = 0, accepted = 0;
    while (fread(hdr, 4, 2, fi) == 2) {
        const uint32_t expect = hdr[0], chunks = hdr[1];
        std::vector<uint32_t> table(2 * (size_t)chunks);
        if (chunks < 1 || fread(table.data(), 4, table.size(), fi) != table.size()) { fprintf(stderr, "short record\n"); return 2; }
        uint32_t n = 0;
        for (uint32_t k = 0; k < chunks; k++) n += table[2 * k];
        uint8_t* in = (uint8_t*)malloc(n);                                // (n = 0: a zero-byte block, any read is out of bounds)
        if (n && fread(in, 1, n, fi) != n) { fprintf(stderr, "short record\n"); return 2; }

        // pass 1: a record per chunk
        std::vector<PngsRecord> rec(chunks);
        std::vector<uint32_t> begin(chunks);
        uint32_t at = 0;
        for (uint32_t k = 0; k < chunks; k++) {
            begin[k] = at;
            const uint32_t end = at + table[2 * k];
            uint8_t* part = end <= 65536u ? (uint8_t*)malloc(end) : in;
            if (part != in && end) memcpy(part, in, end);
            memset(mem, 0xA5, sizeof(PngsMem));
            PngsState s;
            s.in = part; s.n = end; s.out = nullptr; s.m = mem;
            rec[k] = pngs_measure(s, at, k == 0, table[2 * k] == 0, table[2 * k + 1] != 0);
            if (rec[k].length > PNGS_MAX) return fail(records, "a record longer than the cap");
            if (part != in) free(part);
            at = end;
        }
        // pass 2
        const uint32_t route = pngs_scan(rec.data(), chunks, expect);
        // pass 3
        uint8_t* out = (uint8_t*)malloc(expect ? expect : 1);
        memset(out, 0x5A, expect);
        if (route == PNGS_ROUTE_SEGMENTS) {
            for (uint32_t k = 0; k < chunks; k++) {
                if (!rec[k].length) continue;
                if ((uint64_t)rec[k].aux + rec[k].length > expect) return fail(records, "a segment placed outside the inflated data");
                memset(mem, 0xA5, sizeof(PngsMem));
                PngsState s;
                s.in = in; s.n = begin[k] + table[2 * k]; s.out = nullptr; s.m = mem;
                pngs_place(s, begin[k], k == 0, rec[k].length, out + rec[k].aux);
            }
        }
        // the serial inflater, which decides every verdict
        uint8_t* ref = (uint8_t*)malloc(expect ? expect : 1);
        memset(big, 0xA5, sizeof(PngiMem));
        PngiState t;
        t.in = in; t.n = n; t.out = ref; t.expect = expect; t.m = big;
        pngi_inflate(t);
        uint32_t crc = 0;
        for (uint32_t k = 0; k < chunks; k++) crc |= table[2 * k + 1];
        if (route == PNGS_ROUTE_SEGMENTS) {
            accepted++;
            if (crc) return fail(records, "accepted with a CRC flag set");
            if (t.status) return fail(records, "accepted, but the serial inflater refuses the stream");
            if (memcmp(out, ref, expect)) return fail(records, "accepted, but the bytes differ from the serial inflater's");
            PngsRun all = {0u, 1u, 0u};
            for (uint32_t k = 0; k < chunks; k++) {
                const PngsRun x = {rec[k].length, rec[k].adler & 0xffffu, rec[k].adler >> 16};
                all = pngs_join(all, x);
            }
            if (all.a != t.adler_a || all.b != t.adler_b || all.len != expect) return fail(records, "accepted, but the combined Adler-32 is not the serial one");
        } else if ((route & 255u) || (route >> 8) < 1u || (route >> 8) >= PNGS_REASONS) return fail(records, "a route word that is neither 1 nor 0 | reason << 8");
        const uint32_t res[2] = {route, t.status};
        fwrite(res, 4, 2, fo);
        if (route == PNGS_ROUTE_SEGMENTS) fwrite(out, 1, expect, fo);
        free(in); free(out); free(ref);
        records++;
    }
    delete mem;
    delete big;
    fclose(fi);
    if (fclose(fo)) return 2;
    printf("%zu records, %zu accepted\n", records, accepted);
    return 0;
}
