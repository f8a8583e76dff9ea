// png_segments.h -- one PNG file inflated by many waves, where the file allows it.  The project's encoder (csrc/png.hip) ends every row
// segment on a byte boundary with the empty stored block of a full flush and puts it into an IDAT chunk of its own: such chunks are
// independent deflate streams, and the chunk table the host builds is the segment table.  Three passes (csrc/png_decode.hip launches
// them; tests/png_segments_host.cpp runs the same text chunk by chunk under the sanitizers):
//   pngs_measure  per chunk.  A SPECULATIVE decode of the chunk as whole blocks from its first bit, into a buffer of PNGS_MAX bytes that holds
//                 the segment whole -> a 16-byte record: bytes produced, their Adler-32, a state word (a reason, or 0; BFINAL seen; the chunk
//                 is empty; its CRC flag), and the four bytes behind a final block.
//   pngs_scan     per file.  Applies the rules below to the records -> the route word: 1, or 0 | reason << 8.  For an accepted file it
//                 leaves every segment's place (the exclusive prefix of the lengths) in its record.
//   pngs_place    per chunk of an accepted file.  The same decode again, then the buffer goes to inflated[prefix, prefix + length).
// The route only ever ACCEPTS.  A file it does not accept is inflated by pngi_inflate as if this header did not exist, and that status
// stands; for an accepted file the status is 0.
//
// Acceptance ("segment" = IDAT chunk; an empty chunk is a segment with no blocks).  All of:
//   (a) no chunk's CRC flag is set;
//   (b) chunk 0 holds at least the two zlib header bytes, which pass pngi_inflate's header test; segment 0 starts at stream byte 2;
//   (c) every segment, read from its first bit, is a sequence of whole blocks, the last of which ends exactly at bit 8 * length of the
//       chunk; every block is non-final except the last block of the last non-empty chunk, which is final, and behind which -- after
//       byte alignment -- exactly four bytes follow to the end of the chunk;
//   (d) no match reaches before the first byte its own segment produced (dist <= produced), no segment produces more than PNGS_MAX bytes;
//   (e) the lengths sum to `expect` = H (1 + W C);
//   (f) the segments' Adler pairs, combined in order, equal the four bytes of (c) read big-endian.
//
// Why an accepted file is one pngi_inflate accepts, with the same bytes (induction over the chunks, for a file that satisfies (a) .. (f)).
// Claim for k = 0, 1, ...: when the serial inflater reaches the first bit of chunk k it stands at a block boundary (for k = 0: behind the
// header it accepted, by (b)), has seen no BFINAL and no error, and has produced exactly the concatenation of segments 0 .. k-1.
// Step: from that bit the serial inflater and the measure wave read the SAME bits with the same code (pngi_block); a block's decoding
// depends on earlier output only through match sources.  By (d) every source lies inside the segment's own output, which by the claim is
// byte for byte what the serial window holds at the same distance; so both produce the same bytes, block after block, and neither can
// fail where the other does not: the wave's checks are the serial ones with tighter limits (the distance against the segment instead of
// the stream; PNGD_TOO_MANY against PNGS_MAX, while the serial limit `expect` is not reached before the last byte, by (e)); the wave treats
// bytes at and past the chunk's end as absent where the serial inflater sees the next chunk, but by (c) no bit past the chunk's end is
// consumed.  By (c) the last block of the chunk ends at its last bit, non-final unless k is the last non-empty chunk: the claim holds for
// k + 1 (empty chunks change nothing).  In the last non-empty chunk the serial inflater meets the final block, aligns, reads the four
// bytes: by (f) and the associativity of the Adler combination they equal its running Adler-32; the stream ends there (later chunks are
// empty: not PNGD_BEHIND) and `expect` bytes were produced, by (e): status 0, and the bytes are the concatenation of the segments, which is
// what pngs_place wrote.  Conversely nothing is accepted that zlib refuses, since pngi_inflate's verdicts are zlib's.
//
// Bounds.  The stream is read as png_inflate.h states, with n = the chunk's end inside the file's stream: a wave reads no byte of a later
// chunk.  The buffer is written by the emit functions under outpos + count <= expect <= PNGS_MAX = WIN: no index wraps.  pngs_place writes
// out[0, length) only, bytes at an unaligned head and tail and 32-bit words in between: no two segments store to the same word, whatever
// their offsets.  Every loop consumes a bit or sets the status, as there.
#pragma once
#include "png_inflate.h"

#define PNGS_MAX 8192u                // bytes one segment may produce (EGS_PNG_SEGMENT_MAX): the buffer in LDS, a power of two >= the encoder's 4096

// route words: PNGS_ROUTE_SEGMENTS, or 0 | reason << 8
enum {
    PNGS_ROUTE_SEGMENTS = 1,
    PNGS_HEADER_SPLIT = 1,    // chunk 0 is shorter than the zlib header
    PNGS_BLOCK_END = 2,       // a chunk does not end on a block end (the decode ran into the chunk's end)
    PNGS_DISTANCE = 3,        // a distance before the first byte of its segment
    PNGS_CAP = 4,             // a segment of more than PNGS_MAX bytes
    PNGS_TRAILER = 5,         // no final block, one that is not the last block of the last non-empty chunk, or not exactly 4 bytes behind it
    PNGS_SUM = 6,             // the lengths do not sum to H (1 + W C)
    PNGS_ADLER = 7,           // the combined Adler-32 is not the trailer
    PNGS_INFLATE = 8,         // any other inflate error inside a segment (the zlib header's among them)
    PNGS_CRC = 9,             // an IDAT chunk's CRC-32 (the serial wave reports which)
    PNGS_REASONS = 10
};
#define PNGS_ST_REASON 255u
#define PNGS_ST_FINAL 256u
#define PNGS_ST_EMPTY 512u
#define PNGS_ST_CRC 1024u

struct PngsRecord {
    uint32_t length;                  // bytes the segment produces
    uint32_t adler;                   // their Adler-32 (B << 16 | A, from 1)
    uint32_t state;                   // reason (0: whole blocks to the chunk's last bit) | PNGS_ST_*
    uint32_t aux;                     // measure: the four bytes behind a final block; scan, accepted files: the segment's offset in the inflated data
};
typedef PngiMemT<PNGS_MAX> PngsMem;
typedef PngiStateT<PNGS_MAX> PngsState;

#if defined(__HIP_DEVICE_COMPILE__)
#define PNGS_UP(v, o) ((uint32_t)__shfl_up((int)(v), (unsigned)(o)))
#define PNGS_XOR(v, o) ((uint32_t)__shfl_xor((int)(v), (int)(o)))
#define PNGS_LAST(v) ((uint32_t)__shfl((int)(v), 63))
#else
#define PNGS_UP(v, o) (v)             // (never evaluated: one lane)
#define PNGS_XOR(v, o) (v)
#define PNGS_LAST(v) (v)
#endif

// ---- the decode of one chunk ---------------------------------------------------------------------------------------------------------------
// s.in: the file's stream, s.n: the chunk's end in it, s.m, s.expect <= PNGS_MAX set by the caller; `start`: the chunk's first byte; `first`:
// chunk 0.  -> the record's state word without the chunk flags; s.outpos bytes stand in the buffer; aux: the bytes behind a final block.
PNGI_FN uint32_t pngs_decode(PngsState& s, uint32_t start, bool first, uint32_t& aux) {
    s.bitbuf = 0; s.bitcnt = 0; s.pos = start; s.in_base = 0x80000000u;
    s.outpos = 0; s.flushed = 0; s.adler_a = 1; s.adler_b = 0; s.status = 0; s.iters = 0;
    aux = 0;
    if (first) {
        if (s.n - start < 2u) return PNGS_HEADER_SPLIT;
        const uint32_t cmf = pngi_bits(s, 8), flg = pngi_bits(s, 8);
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 32u)) pngi_fail(s, PNGD_ZLIB_HEADER);
    }
    bool last = false;
    // every turn consumes a block's 3 header bits or sets the status
    while (!last && !s.status) {
        if (8ull * s.pos - s.bitcnt == 8ull * s.n) break;             // the chunk ends on a block end
        last = pngi_block(s);
    }
    if (s.status)
        return s.status == PNGD_TRUNCATED ? PNGS_BLOCK_END : s.status == PNGD_DISTANCE ? PNGS_DISTANCE : s.status == PNGD_TOO_MANY ? PNGS_CAP : PNGS_INFLATE;
    if (!last) return 0;
    pngi_drop(s, s.bitcnt & 7u);
    if (s.n - (s.pos - s.bitcnt / 8u) != 4u) return PNGS_TRAILER | PNGS_ST_FINAL;     // (consumed bits <= 8 n: the difference does not wrap)
    for (int k = 0; k < 4; k++) aux = (aux << 8) | pngi_bits(s, 8);
    return PNGS_ST_FINAL;
}

// the Adler-32 of buffer[0, outpos), from 1, in pieces whose sums hold in 32 bits (pngi_flush's arithmetic)
PNGI_FN uint32_t pngs_adler(PngsState& s) {
    PNGI_SYNC();
    const uint8_t* win = pngi_win(s);
    uint32_t a = 1, b = 0;
    for (uint32_t f0 = 0; f0 < s.outpos; f0 += PNGI_FLUSH) {
        const uint32_t f1 = s.outpos - f0 > PNGI_FLUSH ? f0 + PNGI_FLUSH : s.outpos;
        uint32_t A = 0, B = 0;
        for (uint32_t j = f0 + PNGI_LANE; j < f1; j += PNGI_LANES) {
            const uint32_t v = win[j];                                // j < outpos <= PNGS_MAX
            A += v;
            B += (f1 - j) * v;
        }
        A = pngi_sum(A);
        B = pngi_sum(B);
        b = (b + (f1 - f0) * a + B % PNGI_ADLER) % PNGI_ADLER;
        a = (a + A) % PNGI_ADLER;
    }
    return (b << 16) | a;
}

PNGI_FN PngsRecord pngs_measure(PngsState& s, uint32_t start, bool first, bool empty, bool crc_flag) {
    PngsRecord r;
    s.expect = PNGS_MAX;
    r.state = pngs_decode(s, start, first, r.aux) | (empty ? PNGS_ST_EMPTY : 0u) | (crc_flag ? PNGS_ST_CRC : 0u);
    r.length = s.outpos;
    r.adler = pngs_adler(s);
    return r;
}

// The chunk of an accepted file again, to out[0, length): `out` is the segment's first byte in the inflated data, at ANY alignment.
// Bytes up to the first 4-aligned address, whole words the segment owns, bytes behind them.
PNGI_FN void pngs_place(PngsState& s, uint32_t start, bool first, uint32_t length, uint8_t* out) {
    uint32_t aux;
    s.expect = length <= PNGS_MAX ? length : PNGS_MAX;                // (it is: the scan accepted)
    pngs_decode(s, start, first, aux);
    if (s.outpos != length) return;                                   // (it is: the same bits, the same code)
    PNGI_SYNC();
    const uint8_t* win = pngi_win(s);
    uint32_t head = (4u - (uint32_t)((uintptr_t)out & 3u)) & 3u;
    if (head > length) head = length;
    const uint32_t nw = (length - head) >> 2;
    for (uint32_t j = PNGI_LANE; j < head; j += PNGI_LANES) out[j] = win[j];
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out + head);
    for (uint32_t w = PNGI_LANE; w < nw; w += PNGI_LANES) {
        const uint32_t j = head + 4u * w;                             // j + 3 < head + 4 nw <= length
        out32[w] = (uint32_t)win[j] | ((uint32_t)win[j + 1] << 8) | ((uint32_t)win[j + 2] << 16) | ((uint32_t)win[j + 3] << 24);
    }
    for (uint32_t j = head + 4u * nw + PNGI_LANE; j < length; j += PNGI_LANES) out[j] = win[j];
}

// ---- the scan ---------------------------------------------------------------------------------------------------------------------------------
// (length, Adler pair) of a run of bytes; pngs_join(x, y) is the pair of x's bytes followed by y's: A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1)
// mod 65521.  (len2 mod 65521) (A1 - 1) <= 65520^2 < 2^32.  The length saturates (a sum that large is not `expect`).
struct PngsRun { uint32_t len, a, b; };

PNGI_FN PngsRun pngs_join(PngsRun x, PngsRun y) {
    PngsRun r;
    const uint64_t l = (uint64_t)x.len + y.len;
    r.len = l > 0xffffffffull ? 0xffffffffu : (uint32_t)l;
    const uint32_t a1 = (x.a % PNGI_ADLER + PNGI_ADLER - 1u) % PNGI_ADLER;
    r.a = (a1 + y.a % PNGI_ADLER) % PNGI_ADLER;
    r.b = (x.b % PNGI_ADLER + y.b % PNGI_ADLER) % PNGI_ADLER;
    r.b = (r.b + ((y.len % PNGI_ADLER) * a1) % PNGI_ADLER) % PNGI_ADLER;
    return r;
}

// the run of all n records; with `write`, record k receives the length of the run before it
PNGI_FN PngsRun pngs_runs(PngsRecord* rec, uint32_t n, bool write) {
    PngsRun carry = {0u, 1u, 0u};
    for (uint32_t base = 0; base < n; base += PNGI_LANES) {           // (uniform)
        const uint32_t k = base + PNGI_LANE;
        PngsRun x = {0u, 1u, 0u};
        if (k < n) { x.len = rec[k].length; x.a = rec[k].adler & 0xffffu; x.b = rec[k].adler >> 16; }
        for (uint32_t o = 1; o < PNGI_LANES; o <<= 1) {               // inclusive scan over the lanes
            PngsRun y = {PNGS_UP(x.len, o), PNGS_UP(x.a, o), PNGS_UP(x.b, o)};
            if (PNGI_LANE >= o) x = pngs_join(y, x);
        }
        if (write && k < n) {
            const PngsRun before = pngs_join(carry, x);               // the run up to and with k
            rec[k].aux = before.len - rec[k].length;                  // (an accepted file: nothing saturated)
        }
        const PngsRun tile = {PNGS_LAST(x.len), PNGS_LAST(x.a), PNGS_LAST(x.b)};
        carry = pngs_join(carry, tile);
    }
    return carry;
}

PNGI_FN uint32_t pngs_min(uint32_t v) {
    for (uint32_t o = PNGI_LANES / 2u; o > 0; o >>= 1) { const uint32_t w = PNGS_XOR(v, o); v = w < v ? w : v; }
    return v;
}

PNGI_FN uint32_t pngs_max(uint32_t v) {
    for (uint32_t o = PNGI_LANES / 2u; o > 0; o >>= 1) { const uint32_t w = PNGS_XOR(v, o); v = w > v ? w : v; }
    return v;
}

// rec[0, n): the records of a file's chunks, n >= 1 -> the route word (the same in every lane)
PNGI_FN uint32_t pngs_scan(PngsRecord* rec, uint32_t n, uint32_t expect) {
    const uint32_t none = 0xffffffffu;
    uint32_t crc = 0, first_final = none, finals = 0, behind_last = 0;       // behind_last: 1 + the last chunk that holds stream bytes
    for (uint32_t k = PNGI_LANE; k < n; k += PNGI_LANES) {
        const uint32_t st = rec[k].state;
        if (st & PNGS_ST_CRC) crc = 1;
        if (st & PNGS_ST_FINAL) { finals++; first_final = k < first_final ? k : first_final; }
        if (!(st & PNGS_ST_EMPTY)) behind_last = k + 1u;
    }
    crc = pngs_max(crc);
    first_final = pngs_min(first_final);
    finals = pngi_sum(finals);
    behind_last = pngs_max(behind_last);
    if (crc) return PNGS_CRC << 8;
    uint32_t bad = none;                                              // the first chunk with a reason, up to the one with the final block
    for (uint32_t k = PNGI_LANE; k < n; k += PNGI_LANES)
        if ((rec[k].state & PNGS_ST_REASON) && k <= first_final) bad = k < bad ? k : bad;
    bad = pngs_min(bad);
    if (bad != none) return (rec[bad].state & PNGS_ST_REASON) << 8;
    if (finals != 1u || behind_last != first_final + 1u) return PNGS_TRAILER << 8;
    const PngsRun all = pngs_runs(rec, n, false);
    if (all.len != expect) return PNGS_SUM << 8;
    if (((all.b << 16) | all.a) != rec[first_final].aux) return PNGS_ADLER << 8;
    pngs_runs(rec, n, true);
    return PNGS_ROUTE_SEGMENTS;
}
