// png.hip -- 8-bit PNG files written on the device (include/egs_raster.h egs_png_encode): planar uint8 images (CHW, as the evaluation sweep's
// `images`, the mask pass's `masks` and a frame store's `img` hold them) become complete files -- signature, IHDR, IDAT chunks, IEND -- in
// the caller's buffer, with no host work and no read-back.  PNG is lossless: a file is right when it decodes to the input bytes and every
// checksum holds; egogaussian_amd/png.py filter_rows / encode_statement / decode are the torch and zlib statements of it.
//
// Stream.  The filtered data are H rows of 1 + W C bytes: the filter type, then the filtered bytes of the interleaved row.  The type of a
// row is libpng's minimum-sum heuristic made exact: filters 0 .. 4 on the RAW neighbours (left pixel and row above are 0 where they do not
// exist), score = sum of min(v, 256 - v) over the W C filtered bytes, lowest score, ties to the lowest type.  The stream is cut into
// SEGMENTS: one per row, a row longer than PNG_SEG bytes into pieces of PNG_SEG.  One workgroup compresses one segment on its own and ends
// it on a byte boundary, so segments concatenate without bit shifts, and each is an IDAT chunk of its own with its own CRC-32:
//     stored   one stored block (segment bytes + 5), when nothing else is smaller
//     fixed / dynamic Huffman   one block of literals and matches, then the empty stored block a zlib full flush emits.  Matches are LZ77
//              inside the segment: per position the longest repeat at a distance of up to 1024 among the first 128 candidates (zlib's
//              level-6 limits), parsed greedily.  The block kind is chosen by the exact bit cost.
// A dynamic block's literal/length and distance codes are Huffman codes (two-queue merge of the rank-sorted counts) -- complete by
// construction (an alphabet with fewer than two used symbols gets two one-bit codes) --, kept within 15 bits by halving the counts of a
// segment with more than 2583 tokens (png_huffman); the code-length code is a fixed complete one.
//
// Launches (three, whatever the content: the call can be captured).
//   k_png_segment   grid (segments, images), 256 lanes.  Scores the row (integer sums: any order gives the same), filters its piece into
//                   LDS, finds the matches, marks the token starts of the greedy parse by pointer doubling, builds the codes, prices the
//                   three kinds, ORs the tokens (lane t owns bytes 16 t .. 16 t + 15) into zeroed LDS words at the positions an exclusive
//                   scan of their bit lengths gives, and writes the finished chunk (length, "IDAT", data, CRC) to the segment's slot of
//                   `scratch` with its size and Adler-32 pair.  The CRC: every lane the CRC of its slice, combined by multiplication with
//                   x^(8 n) mod P.
//   k_png_layout    one workgroup per image: exclusive scan of the chunk sizes, the Adler pairs combined modulo 65521, then signature,
//                   IHDR, the zlib header, the final block with the Adler-32, IEND and sizes[i].
//   k_png_gather    grid (segments, images): the chunk goes to its offset in the file.
// Every byte is a pure function of the image: integer LDS atomics (add, or, xor) and scans only, nothing depends on arrival order.
#include "egs_common.h"
#include "png_common.h"

#define PNG_WG 256
#define PNG_PER 16
#define PNG_SEG (PNG_WG * PNG_PER)       // filtered bytes per segment at most
#define PNG_MAXD 1024                    // matches reach this far back at most
#define PNG_CHAIN 128                    // candidates tried per position
#define PNG_NICE 128                     // a match this long ends the search
#define PNG_STEP 16                      // distances examined per step of the search (loads in flight)
#define PNG_NSYM 288
#define PNG_HUFF_SUM 2583u                  // a Huffman tree over counts of this sum is at most 15 deep (Fibonacci(18) = 2584)
#define PNG_FIXED_BYTES 77               // signature 8, IHDR 25, zlib header chunk 14, final block + Adler chunk 18, IEND 12
#define PNG_CHUNK_EXTRA 17               // per segment: chunk framing 12 + stored-block header 5
#define PNG_MAX_SIDE 32767
#define PNG_ADLER 65521u

namespace {

struct PngArgs {
    int W, H, RB;                        // RB = W * C bytes of a raw row
    int segs_per_row, nseg;
    long long image_stride, plane_stride;
    unsigned slot_stride;                // bytes of a segment's slot in scratch
    unsigned long long slots_begin;      // where the slots start in an image's scratch
    unsigned long long image_scratch;    // bytes of scratch per image: uint4 info[nseg] (256-aligned), then the slots
    long long out_stride;
};

__host__ __device__ inline int png_seg_len(const PngArgs& a, int seg) {       // filtered bytes of segment `seg` of an image
    const int piece = seg % a.segs_per_row;
    const int g0 = piece * PNG_SEG;
    const int rest = a.RB + 1 - g0;
    return rest < PNG_SEG ? rest : PNG_SEG;
}

__device__ __forceinline__ int png_filter(int f, int x, int a, int b, int c) {
    int v;
    switch (f) {
        case 0: v = x; break;
        case 1: v = x - a; break;
        case 2: v = x - b; break;
        case 3: v = x - ((a + b) >> 1); break;
        default: v = x - png_paeth(a, b, c); break;
    }
    return v & 255;
}

__device__ __forceinline__ uint32_t png_crc_bitwise(uint32_t c, uint32_t byte) {
    c ^= byte;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
    return c;
}

// inclusive block scans over PNG_WG lanes in LDS (Hillis-Steele); `buf` holds PNG_WG ints
template <class Op>
__device__ __forceinline__ int png_scan(int v, int* buf, Op op) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int o = 1; o < PNG_WG; o <<= 1) {
        int x = buf[t];
        if (t >= o) x = op(buf[t - o], x);
        __syncthreads();
        buf[t] = x;
        __syncthreads();
    }
    return buf[t];
}

__device__ __forceinline__ void png_put(uint32_t* w, unsigned pos, unsigned long long v) {      // v's bits start at bit `pos` (LSB first)
    const unsigned wi = pos >> 5, sh = pos & 31u;
    const unsigned long long x = v << sh;
    if ((uint32_t)x) atomicOr(&w[wi], (uint32_t)x);
    if ((uint32_t)(x >> 32)) atomicOr(&w[wi + 1], (uint32_t)(x >> 32));
}

__device__ __forceinline__ uint32_t png_rev(uint32_t code, int len) { return len ? __brev(code) >> (32 - len) : 0u; }

__device__ __forceinline__ void png_fixed_code(int sym, int& len, uint32_t& code) {
    if (sym < 144) { len = 8; code = 0x30u + sym; }
    else if (sym < 256) { len = 9; code = 0x190u + (sym - 144); }
    else if (sym < 280) { len = 7; code = (uint32_t)(sym - 256); }
    else { len = 8; code = 0xC0u + (sym - 280); }
}

// length 3 .. 258 -> symbol 257 .. 285, count and value of its extra bits
__device__ __forceinline__ void png_len_symbol(int len, int& sym, int& nb, int& val) {
    if (len == 258) { sym = 285; nb = 0; val = 0; return; }
    const int l = len - 3;
    if (l < 8) { sym = 257 + l; nb = 0; val = 0; return; }
    nb = (31 - __clz(l)) - 2;
    sym = 257 + 4 * nb + 4 + ((l >> nb) & 3);
    val = l & ((1 << nb) - 1);
}

// the code-length code: fixed and complete (2/8 + 8/16 + 8/32 = 1); symbol 16 is not used
__device__ __forceinline__ int png_cl_len(int s) {
    return (s == 0 || s == 18) ? 3 : (s == 17 || (s >= 2 && s <= 8)) ? 4 : (s == 16 ? 0 : 5);
}
__device__ __forceinline__ uint32_t png_cl_code(int s) {      // canonical codes of the lengths above
    if (s == 0) return 0;
    if (s == 18) return 1;
    if (s >= 2 && s <= 8) return 4u + (s - 2);
    if (s == 17) return 11;
    if (s == 1) return 24;
    return 25u + (s - 9);                                     // 9 .. 15
}

// One walk over the lane's 16 positions: f(j, is_match, length, distance) for every token that starts there
template <class F>
__device__ __forceinline__ void png_tokens(const uint8_t* s, const uint8_t* tok, const uint8_t* mlen, const unsigned short* mdist, int n, int j0, F f) {
#pragma unroll 4
    for (int k = 0; k < PNG_PER; k++) {
        const int j = j0 + k;
        if (j >= n) break;
        if (!tok[j]) continue;
        const int d = mdist[j];
        f(j, d != 0, d ? (int)mlen[j] + 3 : (int)s[j], d);
    }
}

__device__ __forceinline__ void png_dist_symbol(int D, int& sym, int& nb, int& val) {
    const int d = D - 1;
    if (d < 4) { sym = d; nb = 0; val = 0; return; }
    nb = (31 - __clz(d)) - 1;
    sym = 2 * nb + 2 + ((d >> nb) & 1);
    val = d & ((1 << nb) - 1);
}

// canonical code of symbol `sym` (length len > 0) from the per-length counts bl[1 .. 15] and the lengths of the symbols before it
__device__ __forceinline__ uint32_t png_canon(const int* lens, const uint32_t* bl, int sym, int len) {
    uint32_t code = 0;
    for (int b = 1; b <= len; b++) code = (code + (b > 1 ? bl[b - 1] : 0u)) << 1;
    int before = 0;
#pragma unroll 1
    for (int q = 0; q < sym; q++) before += lens[q] == len ? 1 : 0;
    return code + (uint32_t)before;
}

// Huffman lengths (Kraft sum exactly 1) of an alphabet of nsym <= 288 symbols, by the whole workgroup.  lens[] and bl[0 .. 15], *used are ZERO on
// entry; bl[l] comes back as the number of codes of length l.  Fewer than two used symbols: the used one (or symbol 0) and a partner get one bit each.
// No code is longer than 15 bits: a Huffman tree of depth k weighs at least Fibonacci(k + 2), 2584 for k = 16, and the caller asks for the
// counts to be halved (rounded up) when they sum to more than PNG_HUFF_SUM -- at most (4097 + 286) / 2 = 2191 then.  Halving keeps the order of the
// counts, so the code stays a prefix code sorted by frequency; it is what "limiting" costs here, a fraction of a per cent on the segments it touches.
__device__ __forceinline__ void png_huffman(const int* hist, int nsym, bool halve, int* lens, unsigned short* sorted, int* wgt, unsigned short* par,
                                            uint32_t* bl, uint32_t* used) {
    const int t = threadIdx.x;
    for (int sym = t; sym < nsym; sym += PNG_WG) {               // rank of every used symbol by (count, symbol): the leaves in ascending order
        const int c = hist[sym];
        if (c) {
            int r = 0;
#pragma unroll 1
            for (int q = 0; q < nsym; q++) {
                const int cq = hist[q];
                r += (cq && (cq < c || (cq == c && q < sym))) ? 1 : 0;
            }
            sorted[r] = (unsigned short)sym;
            wgt[r] = halve ? (c + 1) >> 1 : c;
            atomicAdd(used, 1u);
        }
    }
    __syncthreads();
    const int m = (int)*used;
    if (m < 2) {
        if (t == 0) {
            const int sym = m ? (int)sorted[0] : 0;
            lens[sym] = 1;
            lens[sym == 0 ? 1 : 0] = 1;
            bl[1] = 2;
        }
        __syncthreads();
        return;
    }
    if (t == 0) {                                                // two-queue merge: leaves li .., internal nodes ii .. nx
        int li = 0, ii = m, nx = m;
#pragma unroll 1
        for (int k = 0; k < m - 1; k++) {
            int x, z;
            if (li < m && (ii >= nx || wgt[li] <= wgt[ii])) x = li++; else x = ii++;
            if (li < m && (ii >= nx || wgt[li] <= wgt[ii])) z = li++; else z = ii++;
            wgt[nx] = wgt[x] + wgt[z];
            par[x] = par[z] = (unsigned short)nx;
            nx++;
        }
    }
    __syncthreads();
    for (int r = t; r < m; r += PNG_WG) {                        // depth of leaf r (root: node 2 m - 2); <= 15 by the weight bound above
        int d = 0, p = r;
#pragma unroll 1
        while (p != 2 * m - 2 && d < 15) { p = par[p]; d++; }
        atomicAdd(&bl[d], 1u);
    }
    __syncthreads();
    for (int r = t; r < m; r += PNG_WG) {                        // the most frequent symbols get the shortest lengths
        const int k = m - 1 - r;
        int cum = 0, len = 15;
#pragma unroll 1
        for (int l = 1; l <= 15; l++) {
            cum += (int)bl[l];
            if (k < cum) { len = l; break; }
        }
        lens[sorted[r]] = len;
    }
    __syncthreads();
}

// misc words in LDS
enum { M_SCORE = 0, M_BL = 16, M_DBL = 32, M_ADLER_A = 48, M_ADLER_B, M_EXTRA, M_NMATCH, M_NTOK, M_TOK_FIXED, M_TOK_DYN, M_RLE_BITS, M_USED, M_DUSED, M_CRC,
       M_ND, M_X2N = 64, M_WORDS = 96 };

template <int C>
__global__ __launch_bounds__(PNG_WG) void k_png_segment(PngArgs a, const uint8_t* __restrict__ src, uint8_t* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[PNG_SEG + 32];
    __shared__ __attribute__((aligned(16))) uint32_t outw[(PNG_SEG + 64) / 4];      // the chunk: length, "IDAT", data (<= n + 5), CRC
    __shared__ __attribute__((aligned(16))) uint32_t region[PNG_SEG + PNG_STEP];           // the 3-byte keys during the search, then the two jump tables
    __shared__ unsigned short mdist[PNG_SEG];                    // 0: no match starts here
    __shared__ uint8_t mlen[PNG_SEG];                            // its length - 3
    __shared__ uint8_t tok[PNG_SEG + 8];                         // a token of the greedy parse starts here
    __shared__ int hist[PNG_NSYM], llen[PNG_NSYM];
    __shared__ uint32_t lcode[PNG_NSYM];
    __shared__ int dhist[32], dlen[32];
    __shared__ uint32_t dcode[32];
    __shared__ unsigned short sorted[PNG_NSYM];
    __shared__ int wgt[2 * PNG_NSYM];
    __shared__ unsigned short par[2 * PNG_NSYM];
    __shared__ int scan_a[PNG_WG];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t misc[M_WORDS];

    const int t = threadIdx.x;
    const int seg = blockIdx.x, img = blockIdx.y;
    const int y = seg / a.segs_per_row;
    const int g0 = (seg - y * a.segs_per_row) * PNG_SEG;         // first byte of the row's stream this segment holds
    const int n = min(PNG_SEG, a.RB + 1 - g0);
    uint8_t* s = sbuf;

    // ---- clear, tables -------------------------------------------------------------------------------------------------------------
    for (int i = t; i < (PNG_SEG + 64) / 4; i += PNG_WG) outw[i] = 0;
    for (int i = t; i < PNG_NSYM; i += PNG_WG) { hist[i] = 0; llen[i] = 0; }
    if (t < 32) { dhist[t] = 0; dlen[t] = 0; }
    if (t < M_WORDS) misc[t] = 0;
    {
        uint32_t c = (uint32_t)t;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
        crc_tab[t] = c;
    }
    __syncthreads();
    if (t == PNG_WG - 1) {                                       // x^(2^k) mod P, k = 0 .. 16 (a chunk is < 2^13 bytes = 2^16 bits)
        uint32_t p = 0x40000000u;
        misc[M_X2N] = p;
        for (int k = 1; k <= 16; k++) { p = png_mulmod(p, p); misc[M_X2N + k] = p; }
    }

    // ---- the row's filter type: five scores over the WHOLE row -----------------------------------------------------------------------
    const uint8_t* cur = src + (long long)img * a.image_stride + (long long)y * a.W;
    const uint8_t* up = cur - a.W;                               // read only when y > 0
    {
        unsigned sc[5] = {0, 0, 0, 0, 0};
        for (int x = t; x < a.W; x += PNG_WG) {
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                const long long po = (long long)ch * a.plane_stride;
                const int v = cur[po + x];
                const int l = x ? (int)cur[po + x - 1] : 0;
                const int b = y ? (int)up[po + x] : 0;
                const int c = (x && y) ? (int)up[po + x - 1] : 0;
#pragma unroll
                for (int f = 0; f < 5; f++) {
                    const int r = png_filter(f, v, l, b, c);
                    sc[f] += (unsigned)min(r, 256 - r);
                }
            }
        }
#pragma unroll
        for (int f = 0; f < 5; f++) {
            unsigned v = sc[f];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((t & 63) == 0) atomicAdd(&misc[M_SCORE + f], v);
        }
    }
    __syncthreads();
    int ftype = 0;
    {
        unsigned best = misc[M_SCORE];
#pragma unroll
        for (int f = 1; f < 5; f++)
            if (misc[M_SCORE + f] < best) { best = misc[M_SCORE + f]; ftype = f; }
    }

    // ---- this segment's filtered bytes --------------------------------------------------------------------------------------------
    for (int i = t; i < n; i += PNG_WG) {
        const int g = g0 + i;
        int v = ftype;
        if (g > 0) {
            const int jj = g - 1, x = jj / C, ch = jj - x * C;
            const long long po = (long long)ch * a.plane_stride;
            const int l = x ? (int)cur[po + x - 1] : 0;
            const int b = y ? (int)up[po + x] : 0;
            const int c = (x && y) ? (int)up[po + x - 1] : 0;
            v = png_filter(ftype, (int)cur[po + x], l, b, c);
        }
        s[i] = (uint8_t)v;
    }
    for (int i = n + t; i < PNG_SEG + 32; i += PNG_WG) s[i] = 0;
    __syncthreads();

    // ---- Adler pair of the segment: A = sum s[j], B = sum (n - j) s[j]; B <= 255 * 4096 * 4097 / 2 = 2 139 617 280 < 2^32 ----------------
    const int j0 = t * PNG_PER;
    if (j0 < n) {
        unsigned A = 0, B = 0;
#pragma unroll
        for (int k = 0; k < PNG_PER; k++) {
            const int j = j0 + k;
            if (j < n) { A += s[j]; B += (unsigned)(n - j) * s[j]; }
        }
        atomicAdd(&misc[M_ADLER_A], A);
        atomicAdd(&misc[M_ADLER_B], B);
    }

    // ---- matches: for every position the longest repeat of >= 3 bytes at a distance of 1 .. PNG_MAXD inside the segment, the nearest of the
    //      longest.  Candidates are the distances whose 3-byte key equals the position's; as zlib does, the search ends after PNG_CHAIN
    //      candidates or at a match of PNG_NICE bytes.  Lane -> consecutive positions: a wave reads consecutive keys.
    uint32_t* key = region + PNG_STEP;                           // (PNG_STEP words in front that equal no key: the search reads that many distances at a time)
    if (t < PNG_STEP) region[t] = 0xfe000000u | (uint32_t)t;
    for (int i = t; i < PNG_SEG; i += PNG_WG)
        key[i] = i + 2 < n ? ((uint32_t)s[i] | ((uint32_t)s[i + 1] << 8) | ((uint32_t)s[i + 2] << 16)) : (0xff000000u | (uint32_t)i);
    __syncthreads();
    for (int j = t; j < n; j += PNG_WG) {
        int best = 0, bd = 0;
        if (j + 2 < n) {
            const uint32_t k = key[j];
            const int ml = min(258, n - j), dmax = min(j, PNG_MAXD);
            int tried = 0;
            bool done = false;
#pragma unroll 1
            for (int d = 1; d <= dmax && !done; d += PNG_STEP) {
                unsigned hits = 0;                               // bit q: distance d + q is a candidate (j - d - q >= -(PNG_STEP - 1): the words in front)
#pragma unroll
                for (int q = 0; q < PNG_STEP; q++) hits |= (key[j - d - q] == k ? 1u : 0u) << q;
#pragma unroll 1
                while (hits && !done) {
                    const int dd = d + __ffs(hits) - 1;
                    hits &= hits - 1;
                    if (dd > dmax) break;
                    int l = 3;                                   // three bytes at a time by their keys (valid up to n - 3), then the tail
                    while (l + 6 <= ml) {
                        const uint32_t a0 = key[j + l], b0 = key[j - dd + l], a1 = key[j + l + 3], b1 = key[j - dd + l + 3];
                        if (a0 != b0) break;
                        if (a1 != b1) { l += 3; break; }
                        l += 6;
                    }
                    while (l + 3 <= ml && key[j + l] == key[j - dd + l]) l += 3;
                    while (l < ml && s[j + l] == s[j - dd + l]) l++;
                    if (l > best) { best = l; bd = dd; }
                    done = best >= PNG_NICE || best >= ml || ++tried >= PNG_CHAIN;
                }
            }
        }
        mlen[j] = (uint8_t)(best >= 3 ? best - 3 : 0);
        mdist[j] = (unsigned short)(best >= 3 ? bd : 0);
    }
    __syncthreads();

    // ---- the greedy parse: a token at j is followed by one at jump[j]; the positions reached from 0 are marked by pointer doubling -- after
    //      round r the first 2^(r + 1) tokens carry their mark (a mark set early is a token all the same) ----------------------------------------
    {
        unsigned short* ja = reinterpret_cast<unsigned short*>(region);
        unsigned short* jb = ja + PNG_SEG + 8;
        for (int i = t; i <= n; i += PNG_WG) {
            ja[i] = (unsigned short)(i < n ? i + (mdist[i] ? (int)mlen[i] + 3 : 1) : n);
            tok[i] = i == 0 ? 1 : 0;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < 12; r++) {
            for (int i = t; i <= n; i += PNG_WG) {
                const int to = min((int)ja[i], n);
                jb[i] = ja[to];
                if (i < n && to < n && tok[i]) tok[to] = 1;
            }
            __syncthreads();
            unsigned short* x = ja; ja = jb; jb = x;
            if ((int)ja[0] >= n) break;                          // (the same word for every lane: 2^(r + 1) tokens reach the end)
        }
        __syncthreads();
    }

    // ---- histograms -------------------------------------------------------------------------------------------------------------------
    {
        unsigned extra = 0, nmatch = 0, ntok = 0;
        if (j0 < n)
            png_tokens(s, tok, mlen, mdist, n, j0, [&](int, bool is_match, int v, int d) {
                ntok++;
                if (!is_match) { atomicAdd(&hist[v], 1); return; }
                int sym, nb, val;
                png_len_symbol(v, sym, nb, val);
                atomicAdd(&hist[sym], 1);
                extra += (unsigned)nb;
                png_dist_symbol(d, sym, nb, val);
                atomicAdd(&dhist[sym], 1);
                extra += (unsigned)nb;
                nmatch++;
            });
        if (extra) atomicAdd(&misc[M_EXTRA], extra);
        if (nmatch) atomicAdd(&misc[M_NMATCH], nmatch);
        if (ntok) atomicAdd(&misc[M_NTOK], ntok);
        if (t == 0) atomicAdd(&hist[256], 1);
    }
    __syncthreads();

    // ---- Huffman lengths of both alphabets ----------------------------------------------------------------------------------------------
    png_huffman(hist, 286, misc[M_NTOK] + 1u > PNG_HUFF_SUM, llen, sorted, wgt, par, &misc[M_BL], &misc[M_USED]);
    png_huffman(dhist, 30, false, dlen, sorted, wgt, par, &misc[M_DBL], &misc[M_DUSED]);      // (at most 4096 / 3 matches)

    // ---- price the kinds ------------------------------------------------------------------------------------------------------------
    {
        unsigned tf = 0, td = 0;
        for (int sym = t; sym < 286; sym += PNG_WG) {
            int fl; uint32_t fc;
            png_fixed_code(sym, fl, fc);
            tf += (unsigned)(hist[sym] * fl);
            td += (unsigned)(hist[sym] * llen[sym]);
        }
        if (t < 30) td += (unsigned)(dhist[t] * dlen[t]);
        if (tf) atomicAdd(&misc[M_TOK_FIXED], tf);
        if (td) atomicAdd(&misc[M_TOK_DYN], td);
    }
    const int nmatch = (int)misc[M_NMATCH];
    const int nl = nmatch ? 286 : 257;                           // HLIT + 257
    auto seq_len = [&](int i) -> int { return i < nl ? llen[i] : dlen[i - nl]; };
    // the run-length coded lengths: f(symbol, extra bit count, extra value)
    auto walk_lengths = [&](int nd, auto f) {
        const int tot = nl + nd;
        int i = 0;
#pragma unroll 1
        while (i < tot) {
            const int v = seq_len(i);
            if (v) { f(v, 0, 0); i++; continue; }
            int z = 1;
            while (i + z < tot && seq_len(i + z) == 0) z++;
            i += z;
#pragma unroll 1
            while (z > 0) {
                if (z >= 11) { const int k = min(z, 138); f(18, 7, k - 11); z -= k; }
                else if (z >= 3) { f(17, 3, z - 3); z = 0; }
                else { f(0, 0, 0); z--; }
            }
        }
    };
    if (t == 0) {
        int nd = 2;                                              // HDIST + 1: up to the last distance symbol with a code
        for (int q = 2; q < 30; q++)
            if (dlen[q]) nd = q + 1;
        unsigned bits = 0;
        walk_lengths(nd, [&](int sym, int nb, int) { bits += (unsigned)(png_cl_len(sym) + nb); });
        misc[M_RLE_BITS] = bits;
        misc[M_ND] = (uint32_t)nd;
    }
    __syncthreads();
    const int nd = (int)misc[M_ND];
    const unsigned fixed_bits = 3u + misc[M_TOK_FIXED] + misc[M_EXTRA] + (unsigned)(nmatch * 5);
    const unsigned dyn_hdr = 3u + 14u + 57u + misc[M_RLE_BITS];
    const unsigned dyn_bits = dyn_hdr + misc[M_TOK_DYN] + misc[M_EXTRA];
    const bool dyn = dyn_bits < fixed_bits;
    const unsigned end_bits = dyn ? dyn_bits : fixed_bits;       // the block, its end code included
    const unsigned comp_bytes = (end_bits + 3u + 7u) / 8u + 4u;  // + the empty stored block: 3 bits, alignment, 00 00 FF FF
    const bool stored = comp_bytes >= (unsigned)n + 5u;
    const unsigned mbytes = stored ? (unsigned)n + 5u : comp_bytes;
    uint8_t* outb = reinterpret_cast<uint8_t*>(outw);
    uint32_t* dataw = outw + 2;

    if (stored) {
        if (t == 0) {
            outb[8] = 0;
            outb[9] = (uint8_t)(n & 255); outb[10] = (uint8_t)(n >> 8);
            outb[11] = (uint8_t)(~n & 255); outb[12] = (uint8_t)((~n >> 8) & 255);
        }
        for (int i = t; i < n; i += PNG_WG) outb[13 + i] = s[i];
    } else {
        // ---- the codes the tokens are written with: bit-reversed code | length << 16 --------------------------------------------------------
        for (int sym = t; sym < PNG_NSYM; sym += PNG_WG) {
            int len = 0; uint32_t code = 0;
            if (!dyn) png_fixed_code(sym, len, code);
            else if (sym < 286 && llen[sym]) { len = llen[sym]; code = png_canon(llen, &misc[M_BL], sym, len); }
            lcode[sym] = png_rev(code, len) | ((uint32_t)len << 16);
        }
        if (t < 30) {
            int len = 5; uint32_t code = (uint32_t)t;
            if (dyn) { len = dlen[t]; code = len ? png_canon(dlen, &misc[M_DBL], t, len) : 0u; }
            dcode[t] = png_rev(code, len) | ((uint32_t)len << 16);
        }
        __syncthreads();
        const unsigned hdr_bits = dyn ? dyn_hdr : 3u;
        if (t == 0) {
            png_put(dataw, 0, dyn ? 4u : 2u);                    // BFINAL 0, BTYPE 10 / 01
            if (dyn) {
                unsigned pos = 3;
                png_put(dataw, pos, (unsigned long long)(nl - 257)); pos += 5;
                png_put(dataw, pos, (unsigned long long)(nd - 1)); pos += 5;
                png_put(dataw, pos, 15ull); pos += 4;           // all 19 lengths of the code-length code follow
                const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                for (int k = 0; k < 19; k++) { png_put(dataw, pos, (unsigned long long)png_cl_len(order[k])); pos += 3; }
                walk_lengths(nd, [&](int sym, int nb, int val) {
                    const int cl = png_cl_len(sym);
                    png_put(dataw, pos, (unsigned long long)png_rev(png_cl_code(sym), cl) | ((unsigned long long)val << cl));
                    pos += (unsigned)(cl + nb);
                });
            }
        }
        // bit lengths of the lane's tokens, their exclusive scan, then the tokens
        int mybits = 0;
        if (j0 < n)
            png_tokens(s, tok, mlen, mdist, n, j0, [&](int, bool is_match, int v, int d) {
                if (!is_match) { mybits += (int)(lcode[v] >> 16); return; }
                int sym, nb, val;
                png_len_symbol(v, sym, nb, val);
                mybits += (int)(lcode[sym] >> 16) + nb;
                png_dist_symbol(d, sym, nb, val);
                mybits += (int)(dcode[sym] >> 16) + nb;
            });
        const int incl = png_scan(mybits, scan_a, [](int x, int z) { return x + z; });
        unsigned pos = hdr_bits + (unsigned)(incl - mybits);
        if (j0 < n)
            png_tokens(s, tok, mlen, mdist, n, j0, [&](int, bool is_match, int v, int d) {
                int sym = v, nb = 0, val = 0;
                if (is_match) png_len_symbol(v, sym, nb, val);
                const uint32_t lc = lcode[sym];
                const int ll = (int)(lc >> 16);
                png_put(dataw, pos, (unsigned long long)(lc & 0xffffu) | ((unsigned long long)val << ll));
                pos += (unsigned)(ll + nb);
                if (is_match) {
                    png_dist_symbol(d, sym, nb, val);
                    const uint32_t dcd = dcode[sym];
                    const int dl = (int)(dcd >> 16);
                    png_put(dataw, pos, (unsigned long long)(dcd & 0xffffu) | ((unsigned long long)val << dl));
                    pos += (unsigned)(dl + nb);
                }
            });
        if (t == PNG_WG - 1) {                                   // the end code (the last lane's `pos` is behind every token), then the flush
            png_put(dataw, pos, (unsigned long long)(lcode[256] & 0xffffu));
            png_put(dataw, (comp_bytes - 2u) * 8u, 0xffffull);   // 00 00 FF FF: the zero bytes are the cleared words (an OR like every other write of them)
        }
    }
    if (t == 0) {
        outb[0] = (uint8_t)(mbytes >> 24); outb[1] = (uint8_t)(mbytes >> 16); outb[2] = (uint8_t)(mbytes >> 8); outb[3] = (uint8_t)mbytes;
        outb[4] = 'I'; outb[5] = 'D'; outb[6] = 'A'; outb[7] = 'T';
    }
    __syncthreads();

    // ---- CRC-32 of type + data: slices, each shifted by the bytes behind it ----------------------------------------------------------------
    {
        const unsigned clen = mbytes + 4u;
        const unsigned cs = (clen + PNG_WG - 1) / PNG_WG;
        const unsigned b0 = (unsigned)t * cs, b1 = min(clen, b0 + cs);
        if (b0 < b1) {
            uint32_t c = 0xffffffffu;
            for (unsigned i = b0; i < b1; i++) c = crc_tab[(c ^ outb[4 + i]) & 255u] ^ (c >> 8);
            c ^= 0xffffffffu;
            unsigned k = clen - b1;                              // x^(8 k) mod P
            uint32_t p = 0x80000000u;
            int e = 3;
#pragma unroll 1
            while (k) {
                if (k & 1u) p = png_mulmod(misc[M_X2N + e], p);
                k >>= 1; e++;
            }
            atomicXor(&misc[M_CRC], png_mulmod(p, c));
        }
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t c = misc[M_CRC];
        const unsigned at = 8u + mbytes;
        outb[at] = (uint8_t)(c >> 24); outb[at + 1] = (uint8_t)(c >> 16); outb[at + 2] = (uint8_t)(c >> 8); outb[at + 3] = (uint8_t)c;
    }
    __syncthreads();

    // ---- the chunk and its record ------------------------------------------------------------------------------------------------------
    uint8_t* base = scratch + (unsigned long long)img * a.image_scratch;
    uint32_t* slot = reinterpret_cast<uint32_t*>(base + a.slots_begin + (size_t)seg * a.slot_stride);
    const unsigned words = (mbytes + 12u + 3u) / 4u;             // <= slot_stride / 4: the slot holds n + 17 bytes rounded up to 16
    for (unsigned i = t; i < words; i += PNG_WG) slot[i] = outw[i];
    if (t == 0)
        reinterpret_cast<uint4*>(base)[seg] = make_uint4(mbytes + 12u, misc[M_ADLER_A] % PNG_ADLER, misc[M_ADLER_B] % PNG_ADLER, 0u);
}

// one workgroup per image
__global__ __launch_bounds__(PNG_WG) void k_png_layout(PngArgs a, int channels, uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
                                                       uint32_t* __restrict__ sizes) {
    __shared__ uint32_t l_bytes[PNG_WG], l_n[PNG_WG], l_a[PNG_WG], l_b[PNG_WG];
    __shared__ uint32_t l_tot[4];
    __shared__ uint8_t hdr[96];
    const int t = threadIdx.x, img = blockIdx.x;
    uint4* info = reinterpret_cast<uint4*>(scratch + (unsigned long long)img * a.image_scratch);
    const int per = (a.nseg + PNG_WG - 1) / PNG_WG;
    const int s0 = min(a.nseg, t * per), s1 = min(a.nseg, s0 + per);
    // Adler of a concatenation X Y:  A = A_X + A_Y,  B = B_X + |Y| A_X + B_Y  (mod 65521).  With every term reduced first, |Y| <= 4096 for
    // a segment and < 65521 for a lane's range after reduction: |Y| A_X + B_X + B_Y < 65521^2 + 2 * 65521 < 2^32 -- 32-bit sums hold.
    uint32_t bytes = 0, nn = 0, A = 0, B = 0;
    for (int sg = s0; sg < s1; sg++) {
        const uint4 e = info[sg];
        const uint32_t ns = (uint32_t)png_seg_len(a, sg);
        B = (B + ns * A + e.z % PNG_ADLER) % PNG_ADLER;
        A = (A + e.y % PNG_ADLER) % PNG_ADLER;
        nn = (nn + ns) % PNG_ADLER;
        bytes += min(e.x, ns + PNG_CHUNK_EXTRA);                 // (a chunk is never longer: the file stays inside egs_png_bound whatever a slot holds)
    }
    l_bytes[t] = bytes; l_n[t] = nn; l_a[t] = A; l_b[t] = B;
    __syncthreads();
    if (t == 0) {
        uint32_t off = 47, ta = 0, tb = 0, tn = 0;               // 47: signature, IHDR, the zlib header's chunk
        for (int k = 0; k < PNG_WG; k++) {
            const uint32_t by = l_bytes[k];
            l_bytes[k] = off;
            off += by;
            tb = (tb + l_n[k] * ta + l_b[k]) % PNG_ADLER;
            ta = (ta + l_a[k]) % PNG_ADLER;
            tn = (tn + l_n[k]) % PNG_ADLER;
        }
        l_tot[0] = off;
        l_tot[1] = (1u + ta) % PNG_ADLER;                        // the stream starts at a = 1, b = 0: a = 1 + A, b = N + B
        l_tot[2] = (tn + tb) % PNG_ADLER;
    }
    __syncthreads();
    {
        uint32_t off = l_bytes[t];
        for (int sg = s0; sg < s1; sg++) {
            uint4 e = info[sg];
            e.x = min(e.x, (uint32_t)png_seg_len(a, sg) + PNG_CHUNK_EXTRA);
            e.w = off;
            off += e.x;
            info[sg] = e;
        }
    }
    if (t == 0) {
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        for (int k = 0; k < 8; k++) hdr[k] = sig[k];
        auto be32 = [&](int at, uint32_t v) { hdr[at] = (uint8_t)(v >> 24); hdr[at + 1] = (uint8_t)(v >> 16); hdr[at + 2] = (uint8_t)(v >> 8); hdr[at + 3] = (uint8_t)v; };
        auto crc = [&](int from, int to) { uint32_t c = 0xffffffffu; for (int k = from; k < to; k++) c = png_crc_bitwise(c, hdr[k]); return c ^ 0xffffffffu; };
        be32(8, 13); hdr[12] = 'I'; hdr[13] = 'H'; hdr[14] = 'D'; hdr[15] = 'R';
        be32(16, (uint32_t)a.W); be32(20, (uint32_t)a.H);
        hdr[24] = 8; hdr[25] = channels == 3 ? 2 : 0; hdr[26] = 0; hdr[27] = 0; hdr[28] = 0;
        be32(29, crc(12, 29));
        be32(33, 2); hdr[37] = 'I'; hdr[38] = 'D'; hdr[39] = 'A'; hdr[40] = 'T'; hdr[41] = 0x78; hdr[42] = 0x01;      // 32 KB window, no dictionary
        be32(43, crc(37, 43));
        // 47 .. 76: the final (empty, fixed Huffman) block and the Adler-32, then IEND
        be32(47, 6); hdr[51] = 'I'; hdr[52] = 'D'; hdr[53] = 'A'; hdr[54] = 'T'; hdr[55] = 0x03; hdr[56] = 0x00;
        be32(57, (l_tot[2] << 16) | l_tot[1]);
        be32(61, crc(51, 61));
        be32(65, 0); hdr[69] = 'I'; hdr[70] = 'E'; hdr[71] = 'N'; hdr[72] = 'D';
        be32(73, crc(69, 73));
        sizes[img] = l_tot[0] + 30u;
    }
    __syncthreads();
    uint8_t* o = out + (long long)img * a.out_stride;
    if (t < 47) o[t] = hdr[t];
    else if (t < PNG_FIXED_BYTES) o[(size_t)l_tot[0] + (size_t)(t - 47)] = hdr[t];
}

__global__ __launch_bounds__(PNG_WG) void k_png_gather(PngArgs a, const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out) {
    const int seg = blockIdx.x, img = blockIdx.y;
    const uint8_t* base = scratch + (unsigned long long)img * a.image_scratch;
    const uint4 e = reinterpret_cast<const uint4*>(base)[seg];
    const uint8_t* slot = base + a.slots_begin + (size_t)seg * a.slot_stride;
    uint8_t* o = out + (long long)img * a.out_stride + (size_t)e.w;
    const unsigned nb = min(e.x, a.slot_stride);                 // (a chunk is never longer than its slot)
    for (unsigned i = threadIdx.x; i < nb; i += PNG_WG) o[i] = slot[i];
}

bool png_geometry(int width, int height, int channels, PngArgs& a) {
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE || (channels != 1 && channels != 3)) return false;
    a = PngArgs();
    a.W = width; a.H = height; a.RB = width * channels;
    a.segs_per_row = (a.RB + 1 + PNG_SEG - 1) / PNG_SEG;
    a.nseg = height * a.segs_per_row;
    const int seg_len = a.RB + 1 < PNG_SEG ? a.RB + 1 : PNG_SEG;
    a.slot_stride = (unsigned)((seg_len + PNG_CHUNK_EXTRA + 15) & ~15);
    a.slots_begin = (unsigned long long)egs_align((size_t)a.nseg * 16);
    a.image_scratch = a.slots_begin + (unsigned long long)a.nseg * a.slot_stride;
    a.image_scratch = (unsigned long long)egs_align((size_t)a.image_scratch);
    return true;
}

}  // namespace

extern "C" {

size_t egs_png_bound(int width, int height, int channels) {
    PngArgs a;
    if (!png_geometry(width, height, channels, a)) return 0;
    return (size_t)PNG_FIXED_BYTES + (size_t)height * (size_t)(a.RB + 1) + (size_t)PNG_CHUNK_EXTRA * (size_t)a.nseg;
}

size_t egs_png_scratch_bytes(int n_images, int width, int height, int channels) {
    PngArgs a;
    if (n_images < 1 || !png_geometry(width, height, channels, a)) return 0;
    return (size_t)n_images * (size_t)a.image_scratch;
}

int egs_png_encode(int n_images, int width, int height, int channels, const uint8_t* src, int64_t image_stride, int64_t plane_stride,
                   uint8_t* out, int64_t out_stride, uint32_t* sizes, void* scratch, void* stream) {
    if (n_images < 1) return EGS_ERR_ARG;
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE || (channels != 1 && channels != 3) || n_images > 65535) return EGS_ERR_RANGE;
    if (!src || !out || !sizes || !scratch) return EGS_ERR_ARG;
    if (((uintptr_t)scratch & 15) || ((uintptr_t)sizes & 3)) return EGS_ERR_ARG;
    PngArgs a;
    png_geometry(width, height, channels, a);
    const int64_t pixels = (int64_t)width * height;
    if (channels == 3 && plane_stride < pixels) return EGS_ERR_ARG;
    if (channels == 1) plane_stride = 0;
    if (n_images > 1 && image_stride < (int64_t)(channels - 1) * plane_stride + pixels) return EGS_ERR_ARG;
    if (out_stride < (int64_t)egs_png_bound(width, height, channels)) return EGS_ERR_ARG;
    if (egs_png_bound(width, height, channels) >= ((size_t)1 << 32)) return EGS_ERR_RANGE;      // sizes and offsets are 32-bit
    a.image_stride = image_stride; a.plane_stride = plane_stride; a.out_stride = out_stride;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a.nseg, (unsigned)n_images);
    if (channels == 3) hipLaunchKernelGGL(k_png_segment<3>, grid, dim3(PNG_WG), 0, st, a, src, (uint8_t*)scratch);
    else hipLaunchKernelGGL(k_png_segment<1>, grid, dim3(PNG_WG), 0, st, a, src, (uint8_t*)scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_png_layout, dim3((unsigned)n_images), dim3(PNG_WG), 0, st, a, channels, (uint8_t*)scratch, out, sizes);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_png_gather, grid, dim3(PNG_WG), 0, st, a, (const uint8_t*)scratch, out);
    return (int)hipGetLastError();
}

}  // extern "C"
