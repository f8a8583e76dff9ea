// png_inflate.h -- the zlib stream of a PNG file inflated into the filtered data (RFC 1950, RFC 1951), with every check a reader owes the
// stream, written once for the device (csrc/png_decode.hip k_pngd_inflate: one wave per file) and for the host compiler
// (tests/png_inflate_host.cpp: the same text under the sanitizers).  The code is SPMD over PNGI_LANES lanes that run the symbol loop
// uniformly -- the bit reader and every decision are the same in all lanes -- and share the work around it: building the code tables,
// copying a match, flushing the window and summing the Adler-32.  On the host there is one lane and the barriers are empty.
//
// Memory.  PngiMem is the working set (LDS on the device, 39 KiB): the 32 KiB window as a ring, a 1 KiB buffer of the stream, the two
// code tables (a 10-bit direct table + count per length + the symbols in canonical order: every length up to 15 is reachable), the code
// lengths (PngiMemT<WIN>: png_segments.h decodes one segment with an 8 KiB buffer, 15 KiB in all).  A match reads the ring, never global memory.  Output leaves through pngi_flush: whole 32-bit words, lane after lane.
//
// Bounds and termination (the contract, not an afterthought):
//   * the stream is read at two places.  Every BIT comes through pngi_word: bytes at or past `n` read as zero; pngi_drop counts the bits
//     consumed, and the first bit consumed past 8 n raises PNGD_TRUNCATED -- after which every loop ends, because every loop tests the
//     status.  The payload of a stored block is copied by pngi_stored straight from in[bp, bp + LEN), only after it has tested
//     LEN <= n - bp (else PNGD_TRUNCATED and nothing is read).
//   * output is written to the ring ONLY by pngi_emit_literal / pngi_emit_match / pngi_stored, each of which first checks
//     outpos + count <= expect (else PNGD_TOO_MANY and nothing is written), and to `out` only by pngi_flush, which copies
//     [flushed, outpos) with outpos <= expect.
//   * every loop iteration consumes at least one bit of the stream or sets the status, and a set status ends every loop: the iterations of
//     all loops together are at most 8 n + PNGI_ITER_SLACK.  `iters` counts them; the host test holds the count to that bound.
// Verdicts equal zlib's inflate() (1.2.11 and later, not INFLATE_STRICT): a stream is accepted exactly when zlib accepts it, ends in it
// and yields `expect` bytes.  In particular a distance may exceed the window the header declares (up to 32768 and the bytes produced),
// and a literal/length or distance code may be incomplete only as a single code of length 1 (distance: or no code at all).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNGI_FN __host__ __device__ __forceinline__
#else
#define PNGI_FN static inline
#endif
// Every function that takes the state is a template over WIN, the bytes of output the working set keeps (a power of two).  The file
// inflater is WIN = PNGI_WINDOW, the deflate window as a ring; png_segments.h decodes one independent segment with a smaller WIN that holds
// the segment whole.
#define PNGI_T template <uint32_t WIN> PNGI_FN

#if defined(__HIP_DEVICE_COMPILE__)
#define PNGI_LANE ((uint32_t)threadIdx.x)
#define PNGI_LANES 64u
#define PNGI_SYNC() __syncthreads()                                  // (the workgroup is one wave)
#define PNGI_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define PNGI_LANE 0u
#define PNGI_LANES 1u
#define PNGI_SYNC() ((void)0)
#define PNGI_UNI(x) ((uint32_t)(x))
#endif

// status words: 0 for a good file, else the first failure (PNGD_IDAT_CRC carries the chunk index in bits 8 ..)
enum {
    PNGD_OK = 0,
    PNGD_IDAT_CRC = 1,        // an IDAT chunk's CRC-32 (status = 1 | chunk index << 8)
    PNGD_ZLIB_HEADER = 2,     // CM != 8, CINFO > 7, FCHECK, FDICT
    PNGD_BLOCK_TYPE = 3,      // BTYPE 3
    PNGD_STORED_LEN = 4,      // LEN != ~NLEN
    PNGD_CODE_SET = 5,        // a code-length code or a set of code lengths over-subscribed or incomplete
    PNGD_REPEAT = 6,          // repeat with no previous length, or past HLIT + HDIST
    PNGD_NO_END = 7,          // no end-of-block code
    PNGD_SYMBOL = 8,          // literal/length symbol 286 / 287 or distance symbol 30 / 31 (declared by HLIT / HDIST or decoded), or a
                              // bit pattern no code of an incomplete set owns
    PNGD_DISTANCE = 9,        // a distance reaching before the start of the output
    PNGD_TRUNCATED = 10,      // the stream ends inside a block (or inside the header or the Adler-32)
    PNGD_TOO_MANY = 11,       // more inflated bytes than H (1 + W C)
    PNGD_TOO_FEW = 12,        // fewer
    PNGD_ADLER = 13,          // Adler-32
    PNGD_BEHIND = 14,         // bytes behind the stream
    PNGD_FILTER = 15,         // a filter type above 4 (raised by the unfilter pass)
    PNGD_CODES = 16
};

#define PNGI_WINDOW 32768u
#define PNGI_FAST_BITS 10
#define PNGI_FAST (1u << PNGI_FAST_BITS)
#define PNGI_INBUF 1024u              // bytes of the stream kept in PngiMem
#define PNGI_FLUSH 4096u              // pending output is flushed at this many bytes (the Adler sums of a piece stay below 2^32)
#define PNGI_ADLER 65521u
#define PNGI_ITER_SLACK 8u

struct PngiCode {
    uint16_t fast[PNGI_FAST];         // next PNGI_FAST_BITS bits of the stream -> symbol << 4 | length; 0: a longer code, or none
    uint16_t sym[288];                // the symbols in canonical order (by length, then by value)
    uint16_t count[16];               // codes per length
    uint16_t first[16];               // canonical code of the first symbol of a length
    uint16_t index[16];               // its place in sym[]
    uint16_t offs[16];                // (the fill positions while sym[] is built)
};

template <uint32_t WIN> struct PngiMemT {
    uint32_t win32[WIN / 4];          // the window, a ring: byte j of the output lives at j & (WIN - 1)
    uint32_t inbuf[PNGI_INBUF / 4];
    PngiCode lit, dist;               // (dist holds the code-length code while a dynamic block's header is read)
    uint8_t lens[320];
    uint8_t cl[20];
};
typedef PngiMemT<PNGI_WINDOW> PngiMem;

template <uint32_t WIN> struct PngiStateT {
    const uint8_t* in;                // the zlib stream, 4-byte aligned; readable up to n rounded up to 4
    uint32_t n;
    uint8_t* out;                     // 4-byte aligned, `expect` bytes
    uint32_t expect;
    PngiMemT<WIN>* m;
    uint64_t bitbuf;
    uint32_t bitcnt, pos;             // bits in bitbuf; the stream byte the next word comes from (consumed bits: 8 pos - bitcnt)
    uint32_t in_base;                 // first stream byte inbuf holds (device)
    uint32_t outpos, flushed;
    uint32_t adler_a, adler_b;
    uint32_t status;
    uint64_t iters;
};
typedef PngiStateT<PNGI_WINDOW> PngiState;

PNGI_T void pngi_fail(PngiStateT<WIN>& s, uint32_t code) {
    if (!s.status) s.status = code;
}

PNGI_T uint8_t* pngi_win(PngiStateT<WIN>& s) { return reinterpret_cast<uint8_t*>(s.m->win32); }

// ---- the one fetch: four stream bytes at `pos`, little-endian, zero at and past n ---------------------------------------------------------
PNGI_T uint32_t pngi_word(PngiStateT<WIN>& s, uint32_t pos) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t a = pos & ~3u;
    if (a < s.in_base || a + 8u > s.in_base + PNGI_INBUF) {           // (uniform: every lane holds the same pos)
        PNGI_SYNC();
        s.in_base = a;
        const uint32_t* in32 = reinterpret_cast<const uint32_t*>(s.in);
        for (uint32_t w = PNGI_LANE; w < PNGI_INBUF / 4u; w += PNGI_LANES) {
            const uint32_t o = a + 4u * w;                            // (n < 2^31: no wrap)
            uint32_t v = 0;
            if (o < s.n) {
                v = in32[o >> 2];                                     // inside n rounded up to 4
                if (o + 4u > s.n) v &= (1u << (8u * (s.n - o))) - 1u;
            }
            s.m->inbuf[w] = v;
        }
        PNGI_SYNC();
    }
    const uint32_t i = (a - s.in_base) >> 2, sh = (pos & 3u) * 8u;
    const uint32_t lo = s.m->inbuf[i], hi = s.m->inbuf[i + 1];        // i + 1 <= INBUF / 4 - 1 by the test above
    return PNGI_UNI(sh ? (lo >> sh) | (hi << (32u - sh)) : lo);
#else
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; k++)
        if (pos + k < s.n) v |= (uint32_t)s.in[pos + k] << (8u * k);
    return v;
#endif
}

PNGI_T void pngi_need(PngiStateT<WIN>& s, uint32_t k) {                    // k <= 32
    if (s.bitcnt < k) {
        s.bitbuf |= (uint64_t)pngi_word(s, s.pos) << s.bitcnt;        // bitcnt < 32: the word fits
        s.pos += 4u;
        s.bitcnt += 32u;
    }
}

PNGI_T void pngi_drop(PngiStateT<WIN>& s, uint32_t k) {                    // k <= bitcnt
    s.bitbuf >>= k;
    s.bitcnt -= k;
    if (8ull * s.pos - s.bitcnt > 8ull * s.n) pngi_fail(s, PNGD_TRUNCATED);
}

PNGI_T uint32_t pngi_bits(PngiStateT<WIN>& s, uint32_t k) {                // k <= 16
    if (!k) return 0;
    pngi_need(s, k);
    const uint32_t v = (uint32_t)s.bitbuf & ((1u << k) - 1u);
    pngi_drop(s, k);
    return v;
}

// ---- output -------------------------------------------------------------------------------------------------------------------------------
PNGI_FN uint32_t pngi_sum(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
#endif
    return v;
}

// [flushed, outpos) leaves the ring for `out` in pieces of at most PNGI_FLUSH bytes, whole words unless `all`; the Adler pair follows.
// A piece of m <= 4096 bytes: A = sum b_j, B = sum (m - j) b_j <= 255 * 4096 * 4097 / 2 < 2^32 -- 32-bit sums hold.
PNGI_T void pngi_flush(PngiStateT<WIN>& s, bool all) {
    PNGI_SYNC();
    const uint32_t upto = all ? s.outpos : s.outpos & ~3u;
    const uint8_t* win = pngi_win(s);
    while (s.flushed < upto) {                                        // (no stream bits: at most expect / 4096 + 1 turns per call, and a call
        const uint32_t f0 = s.flushed;                                //  follows 4096 emitted bytes or the end)
        const uint32_t f1 = upto - f0 > PNGI_FLUSH ? f0 + PNGI_FLUSH : upto;
        uint32_t A = 0, B = 0;
        for (uint32_t j = f0 + PNGI_LANE; j < f1; j += PNGI_LANES) {
            const uint32_t b = win[j & (WIN - 1u)];
            A += b;
            B += (f1 - j) * b;
        }
        A = pngi_sum(A);
        B = pngi_sum(B);
        s.adler_b = (s.adler_b + (f1 - f0) * s.adler_a + B % PNGI_ADLER) % PNGI_ADLER;      // 4096 * 65520 + 2 * 65520 < 2^32
        s.adler_a = (s.adler_a + A) % PNGI_ADLER;
        const uint32_t nw = (f1 - f0) >> 2;                           // f0 is a multiple of 4: flushed only ends elsewhere after `all`
        uint32_t* out32 = reinterpret_cast<uint32_t*>(s.out);
        for (uint32_t w = PNGI_LANE; w < nw; w += PNGI_LANES)
            out32[(f0 >> 2) + w] = s.m->win32[((f0 >> 2) + w) & (WIN / 4u - 1u)];   // f0 + 4 w + 3 < f1 <= outpos <= expect
        for (uint32_t j = f0 + 4u * nw + PNGI_LANE; j < f1; j += PNGI_LANES) s.out[j] = win[j & (WIN - 1u)];
        s.flushed = f1;
    }
    PNGI_SYNC();
}

// pending output leaves at PNGI_FLUSH bytes -- of the ring.  A smaller WIN holds its whole output (expect <= WIN) until its caller takes it.
PNGI_T void pngi_pending(PngiStateT<WIN>& s) {
    if (WIN >= PNGI_WINDOW && s.outpos - s.flushed >= PNGI_FLUSH) pngi_flush(s, false);
}

PNGI_T void pngi_emit_literal(PngiStateT<WIN>& s, uint32_t b) {
    if (s.outpos >= s.expect) { pngi_fail(s, PNGD_TOO_MANY); return; }
    pngi_win(s)[s.outpos & (WIN - 1u)] = (uint8_t)b;                  // (every lane the same byte)
    s.outpos++;
    pngi_pending(s);
}

// len 3 .. 258, dist 1 .. 32768.  Byte k of the match is byte k % dist of the dist bytes before it: sources lie before outpos, targets at
// or behind it (at dist = 32768 a lane's source and target share a ring slot: it reads, then writes).
PNGI_T void pngi_emit_match(PngiStateT<WIN>& s, uint32_t len, uint32_t dist) {
    if (dist > s.outpos) { pngi_fail(s, PNGD_DISTANCE); return; }
    if (len > s.expect - s.outpos) { pngi_fail(s, PNGD_TOO_MANY); return; }
    PNGI_SYNC();                                                      // the bytes other lanes copied are in the ring
    uint8_t* win = pngi_win(s);
    const uint32_t from = s.outpos - dist;
    for (uint32_t k = PNGI_LANE; k < len; k += PNGI_LANES) {
        const uint32_t v = win[(from + k % dist) & (WIN - 1u)];
        win[(s.outpos + k) & (WIN - 1u)] = (uint8_t)v;
    }
    s.outpos += len;
    pngi_pending(s);
}

// ---- code tables ----------------------------------------------------------------------------------------------------------------------------
// lens[0 .. n) -> code.  false (and the status) for an over-subscribed set, and for an incomplete one unless `lone` allows what zlib
// allows: a single code of length 1, or (lone == 2, the distance set) no code at all.
PNGI_T bool pngi_build(PngiStateT<WIN>& s, PngiCode& c, const uint8_t* lens, uint32_t n, int lone) {
    PNGI_SYNC();
    if (PNGI_LANE == 0) {
        for (int l = 0; l < 16; l++) c.count[l] = 0;
        for (uint32_t i = 0; i < n; i++) c.count[lens[i]]++;
        uint32_t code = 0, at = 0;
        c.first[0] = 0; c.index[0] = 0;
        for (int l = 1; l < 16; l++) {
            code = (code + (l > 1 ? c.count[l - 1] : 0u)) << 1;
            c.first[l] = (uint16_t)code;                              // (an over-subscribed set overflows this; it is refused below)
            c.index[l] = (uint16_t)at;
            at += c.count[l];
        }
        for (int l = 0; l < 16; l++) c.offs[l] = c.index[l];
        for (uint32_t i = 0; i < n; i++)
            if (lens[i]) c.sym[c.offs[lens[i]]++] = (uint16_t)i;      // at most n <= 288 entries
    }
    for (uint32_t k = PNGI_LANE; k < PNGI_FAST; k += PNGI_LANES) c.fast[k] = 0;
    PNGI_SYNC();
    int left = 1, maxlen = 0, total = 0;
    for (int l = 1; l < 16; l++) {
        const int cnt = c.count[l];
        left = (left << 1) - cnt;
        if (left < 0) { pngi_fail(s, PNGD_CODE_SET); return false; }
        if (cnt) maxlen = l;
        total += cnt;
    }
    if (left > 0 && !((lone >= 1 && maxlen == 1) || (lone == 2 && total == 0))) { pngi_fail(s, PNGD_CODE_SET); return false; }
    for (uint32_t i = PNGI_LANE; i < (uint32_t)total; i += PNGI_LANES) {
        const uint32_t sy = c.sym[i], l = lens[sy];
        if (l > PNGI_FAST_BITS) continue;
        const uint32_t code = (uint32_t)c.first[l] + (i - c.index[l]);
        uint32_t rev = 0;
        for (uint32_t b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1u - b);
        for (uint32_t k = rev; k < PNGI_FAST; k += 1u << l) c.fast[k] = (uint16_t)(sy << 4 | l);      // a prefix code: no two symbols share a slot
    }
    PNGI_SYNC();
    return true;
}

// the next symbol of `c`, or -1 (PNGD_SYMBOL) when no code owns the bits
PNGI_T int pngi_decode(PngiStateT<WIN>& s, const PngiCode& c) {
    pngi_need(s, 15);
    const uint32_t v = (uint32_t)s.bitbuf;
    const uint32_t e = PNGI_UNI(c.fast[v & (PNGI_FAST - 1u)]);
    if (e) { pngi_drop(s, e & 15u); return (int)(e >> 4); }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {                               // canonical walk, one bit per turn (15 turns at most)
        code |= (v >> (l - 1u)) & 1u;
        const uint32_t cnt = PNGI_UNI(c.count[l]);
        if (code - first < cnt) {
            pngi_drop(s, l);
            return (int)PNGI_UNI(c.sym[index + (code - first)]);
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    pngi_fail(s, PNGD_SYMBOL);
    return -1;
}

// ---- blocks -------------------------------------------------------------------------------------------------------------------------------
PNGI_T void pngi_stored(PngiStateT<WIN>& s) {
    pngi_drop(s, s.bitcnt & 7u);
    const uint32_t len = pngi_bits(s, 16), nlen = pngi_bits(s, 16);
    if (s.status) return;
    if ((len ^ nlen) != 0xffffu) { pngi_fail(s, PNGD_STORED_LEN); return; }
    uint32_t bp = s.pos - s.bitcnt / 8u;                              // bitcnt is a multiple of 8 here; bp <= n (nothing was consumed past n)
    if (len > s.n - bp) { pngi_fail(s, PNGD_TRUNCATED); return; }
    if (len > s.expect - s.outpos) { pngi_fail(s, PNGD_TOO_MANY); return; }
    uint8_t* win = pngi_win(s);
    uint32_t rest = len;
    while (rest) {                                                    // each turn consumes >= 1 stream byte
        s.iters++;
        const uint32_t m = rest < 2048u ? rest : 2048u;
        for (uint32_t k = PNGI_LANE; k < m; k += PNGI_LANES) win[(s.outpos + k) & (WIN - 1u)] = s.in[bp + k];      // bp + k < bp + rest <= n
        s.outpos += m; bp += m; rest -= m;
        pngi_pending(s);
    }
    s.pos = bp; s.bitbuf = 0; s.bitcnt = 0;
}

PNGI_T void pngi_codes(PngiStateT<WIN>& s) {
    // every turn consumes at least one bit (every code has a length >= 1) or sets the status, and the status ends the loop
    while (!s.status) {
        s.iters++;
        const int sym = pngi_decode(s, s.m->lit);
        if (sym < 0) break;
        if (sym < 256) { pngi_emit_literal(s, (uint32_t)sym); continue; }
        if (sym == 256) break;
        if (sym >= 286) { pngi_fail(s, PNGD_SYMBOL); break; }
        const uint32_t ls = (uint32_t)sym - 257u;
        uint32_t len;
        if (ls < 8u) len = 3u + ls;
        else if (ls == 28u) len = 258u;
        else { const uint32_t eb = (ls >> 2) - 1u; len = 3u + ((4u + (ls & 3u)) << eb) + pngi_bits(s, eb); }
        const int ds = pngi_decode(s, s.m->dist);
        if (ds < 0) break;
        if (ds >= 30) { pngi_fail(s, PNGD_SYMBOL); break; }
        uint32_t dist;
        if (ds < 4) dist = 1u + (uint32_t)ds;
        else { const uint32_t eb = ((uint32_t)ds >> 1) - 1u; dist = 1u + ((2u + ((uint32_t)ds & 1u)) << eb) + pngi_bits(s, eb); }
        if (s.status) break;                                          // (the extra bits ran past the end)
        pngi_emit_match(s, len, dist);
    }
}

PNGI_T bool pngi_fixed_tables(PngiStateT<WIN>& s) {
    PNGI_SYNC();
    for (uint32_t i = PNGI_LANE; i < 320u; i += PNGI_LANES)
        s.m->lens[i] = (uint8_t)(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : i < 288u ? 8 : 5);      // 288 literal/length, 32 distance codes of 5 bits
    PNGI_SYNC();
    return pngi_build(s, s.m->lit, s.m->lens, 288, 0) && pngi_build(s, s.m->dist, s.m->lens + 288, 32, 0);
}

PNGI_T bool pngi_dynamic_tables(PngiStateT<WIN>& s) {
    const uint32_t nlen = pngi_bits(s, 5) + 257u, ndist = pngi_bits(s, 5) + 1u, ncode = pngi_bits(s, 4) + 4u;
    if (s.status) return false;
    if (nlen > 286u || ndist > 30u) { pngi_fail(s, PNGD_SYMBOL); return false; }
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    PNGI_SYNC();
    for (uint32_t i = PNGI_LANE; i < 20u; i += PNGI_LANES) s.m->cl[i] = 0;
    PNGI_SYNC();
    for (uint32_t i = 0; i < ncode; i++) {                            // <= 19 turns of 3 bits
        s.m->cl[order[i]] = (uint8_t)pngi_bits(s, 3);
    }
    if (s.status) return false;
    if (!pngi_build(s, s.m->dist, s.m->cl, 19, 0)) return false;
    const uint32_t total = nlen + ndist;
    uint32_t idx = 0, prev = 0;
    // every turn consumes at least one bit or sets the status; idx also grows by >= 1 per turn: at most 316 turns
    while (idx < total && !s.status) {
        s.iters++;
        const int sym = pngi_decode(s, s.m->dist);
        if (sym < 0) break;
        uint32_t rep = 1, v = (uint32_t)sym;
        if (sym == 16) {
            if (idx == 0) { pngi_fail(s, PNGD_REPEAT); break; }
            v = prev; rep = 3u + pngi_bits(s, 2);
        } else if (sym == 17) { v = 0; rep = 3u + pngi_bits(s, 3); }
        else if (sym == 18) { v = 0; rep = 11u + pngi_bits(s, 7); }
        if (rep > total - idx) { pngi_fail(s, PNGD_REPEAT); break; }
        for (uint32_t k = 0; k < rep; k++) s.m->lens[idx + k] = (uint8_t)v;      // idx + k < total <= 316
        idx += rep; prev = v;
    }
    if (s.status) return false;
    PNGI_SYNC();
    if (s.m->lens[256] == 0) { pngi_fail(s, PNGD_NO_END); return false; }
    return pngi_build(s, s.m->lit, s.m->lens, nlen, 1) && pngi_build(s, s.m->dist, s.m->lens + nlen, ndist, 2);
}

// One block, from its header bits -> BFINAL.  It consumes its 3 header bits or sets the status; see the loops inside for theirs.
PNGI_T bool pngi_block(PngiStateT<WIN>& s) {
    s.iters++;
    const bool last = pngi_bits(s, 1) != 0;
    const uint32_t type = pngi_bits(s, 2);
    if (s.status) return last;
    if (type == 0) pngi_stored(s);
    else if (type == 3) pngi_fail(s, PNGD_BLOCK_TYPE);
    else if (type == 1 ? pngi_fixed_tables(s) : pngi_dynamic_tables(s)) pngi_codes(s);
    return last;
}

// The whole stream.  s.in / n / out / expect / m are set by the caller; -> s.status (0: `expect` bytes are in `out`).
PNGI_T void pngi_inflate(PngiStateT<WIN>& s) {
    s.bitbuf = 0; s.bitcnt = 0; s.pos = 0; s.in_base = 0x80000000u;
    s.outpos = 0; s.flushed = 0; s.adler_a = 1; s.adler_b = 0; s.status = 0; s.iters = 0;
    const uint32_t cmf = pngi_bits(s, 8), flg = pngi_bits(s, 8);
    if (!s.status && ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 32u))) pngi_fail(s, PNGD_ZLIB_HEADER);
    bool last = false;
    while (!last && !s.status) last = pngi_block(s);
    if (s.status) return;
    pngi_flush(s, true);
    pngi_drop(s, s.bitcnt & 7u);
    uint32_t adler = 0;
    for (int k = 0; k < 4; k++) adler = (adler << 8) | pngi_bits(s, 8);
    if (s.status) return;
    if (adler != ((s.adler_b << 16) | s.adler_a)) { pngi_fail(s, PNGD_ADLER); return; }
    if (s.pos - s.bitcnt / 8u < s.n) { pngi_fail(s, PNGD_BEHIND); return; }
    if (s.outpos < s.expect) pngi_fail(s, PNGD_TOO_FEW);
}
