// jpeg_decode.hip -- baseline JPEG files read on the device (include/egs_raster.h egs_jpeg_decode): the bytes of a batch of files, uploaded
// as they are, become interleaved uint8 [h][w][C] arrays for the ingest kernel (csrc/ingest.hip).  The host has walked the marker segments
// up to the SOS header (egogaussian_amd/jpeg.py parse) and built a record and a set of tables per file; it has not touched an
// entropy-coded byte.  Everything about those bytes is decided here and reported in one status word per file.  The arithmetic of every
// step is stated in egogaussian_amd/jpeg.py (decode and the functions it calls), which tests/test_jpeg_cpu.py holds against Pillow.
//
// Launches (four per batch, whatever the files hold: no allocation, no synchronisation, no global state; can be captured; ordered by
// launch boundaries only).
//   k_jpgd_intervals  grid (files), 256 lanes.  Steps of 4096 bytes in order: every lane looks at its 16 bytes (and the one behind them);
//                     the first terminating event of the step (EOI, another marker, the file's end) is a minimum over the lanes, the
//                     restart markers in front of it are numbered by a scan over the lanes' counts, carried from step to step.
//   k_jpgd_entropy    grid (files, slices), one lane per restart interval.  The workgroup first builds the file's decode tables in LDS.
//                     Bounds: a lane's reader loads p[pos] only with start <= pos < end; it writes the blocks of MCUs
//                     [k ri, min((k + 1) ri, MCUs)) and nothing else, whatever the bytes hold.
//   k_jpgd_idct       grid (files, slices), eight lanes per block, 32 blocks per workgroup step; the workspace goes through LDS between
//                     the column pass and the row pass.
//   k_jpgd_colour     grid (files, slices), one lane per output pixel; lane 0 of slice 0 writes the file's status word.
// Between the launches a file's verdict lives in four stage words in scratch (JpgdWords), so that no launch reads a word another workgroup
// of the same launch writes.
#include "egs_common.h"
#include "decode_args.h"

#define JPGD_WG 256
#define JPGD_MAX_SIDE 32767
#define JPGD_NONE 0xffffffffu

namespace {

struct JpgdWords { uint32_t scan, key, range, pad; };      // intervals' status; min (interval << 8 | code) of the entropy lanes; idct's flag

struct JpgdArgs {
    const uint8_t* files;
    const egs_jpeg_file* desc;
    const egs_jpeg_tables* tables;
    uint8_t* out;
    uint32_t* status;
    JpgdWords* words;                        // scratch: [n_files]
    uint2* intervals;                        // scratch: [n_intervals] (start, end) offsets inside the file
    uint8_t* coef;                           // scratch: int16 [blocks][64]
    uint8_t* planes;                         // scratch: uint8 component planes
};

__constant__ uint8_t c_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ uint32_t jpgd_blocks_per_mcu(const egs_jpeg_file& f) { return f.channels == 3 ? (uint32_t)(f.hs * f.vs + 2) : 1u; }

// ---- (a) the restart intervals -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPGD_WG) void k_jpgd_intervals(JpgdArgs a) {
    __shared__ unsigned long long sh_stop;                 // min over the lanes of (position << 2 | kind): 0 EOI, 1 another marker, 3 the file's end
    __shared__ uint32_t sh_bad;                            // min position of a restart marker with the wrong number
    __shared__ uint32_t sh_scan[JPGD_WG];
    const uint32_t t = threadIdx.x, file = blockIdx.x;
    const egs_jpeg_file f = a.desc[file];
    const uint8_t* d = a.files + f.file_offset;           // the host entry has checked: [file_offset, file_offset + file_bytes) inside `files`
    const uint32_t n = (uint32_t)f.file_bytes;            // < 2^31
    uint2* iv = a.intervals + f.interval_begin;           // [n_intervals] (host-checked against the table's length)
    const uint32_t n_iv = f.n_intervals;
    if (t == 0) {
        sh_stop = ~0ull;
        sh_bad = JPGD_NONE;
        iv[0].x = f.entropy_begin;
    }
    __syncthreads();
    uint32_t count = 0, status = EGS_JPEG_OK;
    for (uint32_t base = f.entropy_begin;; base += JPGD_WG * 16u) {
        if (base >= n) {                                  // (uniform)
            status = EGS_JPEG_NO_EOI;
            break;
        }
        const uint32_t lo = min(n, base + t * 16u), hi = min(n, lo + 16u);
        uint32_t rst_pos[8], n_rst = 0, nums = 0;         // at most 8 markers of 2 bytes start in 16 bytes; their numbers in 4 bits each
        unsigned long long stop = ~0ull;
        for (uint32_t i = lo; i < hi; i++) {
            if (d[i] != 0xffu) continue;
            if (i + 1u >= n) { stop = ((unsigned long long)i << 2) | 3ull; break; }
            const uint32_t m = d[i + 1u];                 // i + 1 < n: inside the file
            if (m == 0u) continue;
            if (m >= 0xd0u && m <= 0xd7u) {
                nums |= (m - 0xd0u) << (4u * n_rst);
                rst_pos[n_rst++] = i++;                   // (the marker's second byte is no FF: the next candidate is two bytes on)
                continue;
            }
            stop = ((unsigned long long)i << 2) | (m == 0xd9u ? 0ull : 1ull);
            break;
        }
        if (stop != ~0ull) atomicMin(&sh_stop, stop);
        __syncthreads();
        const unsigned long long first = sh_stop;
        const uint32_t stop_pos = first == ~0ull ? JPGD_NONE : (uint32_t)(first >> 2);
        uint32_t mine = 0;
        for (uint32_t j = 0; j < n_rst; j++) mine += rst_pos[j] < stop_pos ? 1u : 0u;
        sh_scan[t] = mine;
        __syncthreads();
        for (uint32_t o = 1; o < JPGD_WG; o <<= 1) {      // inclusive scan of the lanes' counts
            const uint32_t v = t >= o ? sh_scan[t - o] : 0u;
            __syncthreads();
            sh_scan[t] += v;
            __syncthreads();
        }
        const uint32_t before = count + sh_scan[t] - mine, total = sh_scan[JPGD_WG - 1];
        for (uint32_t j = 0; j < mine; j++) {
            const uint32_t ord = before + j, num = (nums >> (4u * j)) & 15u;
            if (num != (ord & 7u)) atomicMin(&sh_bad, rst_pos[j]);
            if (ord + 1u < n_iv) {                        // interval ord ends here, interval ord + 1 starts behind the marker: both < n_iv
                iv[ord].y = rst_pos[j];
                iv[ord + 1u].x = rst_pos[j] + 2u;
            }
        }
        count += total;
        __syncthreads();
        const uint32_t bad = sh_bad;
        if (bad < stop_pos) {                             // (sh_bad only ever holds positions in front of the stop: both sides uniform)
            status = EGS_JPEG_RESTART;
            break;
        }
        if (first != ~0ull) {
            const uint32_t kind = (uint32_t)(first & 3ull);
            if (kind == 0u) {
                if (count + 1u != n_iv) status = EGS_JPEG_RESTART;
                else if (t == 0) iv[count].y = stop_pos;
            } else {
                status = kind == 1u ? EGS_JPEG_MARKER : EGS_JPEG_NO_EOI;
            }
            break;
        }
        __syncthreads();                                  // (every lane has read sh_stop and sh_bad; they still hold "none")
    }
    if (t == 0) {
        JpgdWords w;
        w.scan = status; w.key = JPGD_NONE; w.range = 0u; w.pad = 0u;
        a.words[file] = w;
    }
}

// ---- (b) entropy decode ----------------------------------------------------------------------------------------------------------------------
struct JpgdBook {                                         // tables 0 .. 3: DC, 4 .. 7: AC
    uint16_t lut[8][256];                                 // the next 8 bits -> length << 8 | symbol; 0: no code of at most 8 bits
    int32_t maxcode[8][18];                               // per length 1 .. 16 the largest code, -1 when the length has none
    int32_t valoff[8][18];                                // index of the length's first symbol minus its smallest code
    uint8_t values[8][256];
    uint8_t quant[4][64];
    uint8_t zigzag[64];
};

struct JpgdBits {
    const uint8_t* p;                                     // the file
    uint32_t pos, end;                                    // the next byte to load; loads only with pos < end
    uint64_t buf;                                         // the low `n` bits are valid
    uint32_t n;
};

__device__ __forceinline__ void jpgd_fill(JpgdBits& b) {
    while (b.n <= 56u && b.pos < b.end) {
        const uint32_t v = b.p[b.pos++];
        if (v == 0xffu) b.pos++;                          // the stuffed 00 behind it (k_jpgd_intervals has looked at every FF of the interval)
        b.buf = (b.buf << 8) | v;
        b.n += 8u;
    }
}

// the next 16 bits, zeros behind the last one
__device__ __forceinline__ uint32_t jpgd_peek16(const JpgdBits& b) {
    return (uint32_t)(b.n >= 16u ? b.buf >> (b.n - 16u) : b.buf << (16u - b.n)) & 0xffffu;
}

// -> the symbol, or -EGS_JPEG_SHORT / -EGS_JPEG_CODE.  jpeg.py _symbol is the statement: the canonical walk, a bit at a time.
__device__ __forceinline__ int jpgd_symbol(JpgdBits& b, const JpgdBook& bk, uint32_t t) {
    jpgd_fill(b);
    const uint32_t peek = jpgd_peek16(b);
    const uint32_t e = bk.lut[t][peek >> 8];
    if (e) {
        const uint32_t len = e >> 8;
        if (len > b.n) return -(int)EGS_JPEG_SHORT;
        b.n -= len;
        return (int)(e & 255u);
    }
    for (uint32_t len = 9; len <= 16u; len++) {
        if (len > b.n) return -(int)EGS_JPEG_SHORT;
        const int32_t code = (int32_t)(peek >> (16u - len));
        if (code <= bk.maxcode[t][len]) {
            b.n -= len;
            return (int)bk.values[t][(uint32_t)(bk.valoff[t][len] + code) & 255u];
        }
    }
    return -(int)EGS_JPEG_CODE;
}

// s bits (1 .. 15) extended to a signed value; false when the interval's bits run out
__device__ __forceinline__ bool jpgd_receive(JpgdBits& b, uint32_t s, int32_t& v) {
    jpgd_fill(b);
    if (s > b.n) return false;
    b.n -= s;
    const int32_t raw = (int32_t)((b.buf >> b.n) & ((1ull << s) - 1ull));
    v = raw >= (1 << (s - 1u)) ? raw : raw - (1 << s) + 1;
    return true;
}

__global__ __launch_bounds__(JPGD_WG) void k_jpgd_entropy(JpgdArgs a) {
    __shared__ JpgdBook bk;
    const uint32_t t = threadIdx.x, file = blockIdx.x;
    const egs_jpeg_file f = a.desc[file];
    if (blockIdx.y * blockDim.x >= f.n_intervals) return;             // (uniform) a slice this file has no interval for
    if (a.words[file].scan != EGS_JPEG_OK) return;                    // (uniform; written by the launch before)
    const egs_jpeg_tables* tb = a.tables + file;
    for (uint32_t i = t; i < 8u * 256u; i += blockDim.x) {
        const uint32_t k = i >> 8;
        bk.values[k][i & 255u] = (k < 4u ? tb->dc[k] : tb->ac[k - 4u]).values[i & 255u];
    }
    for (uint32_t i = t; i < 256u; i += blockDim.x) bk.quant[i >> 6][i & 63u] = tb->quant[i >> 6][i & 63u];
    if (t < 64u) bk.zigzag[t] = c_zigzag[t];
    if (t < 8u) {
        const egs_jpeg_huffman& h = t < 4u ? tb->dc[t] : tb->ac[t - 4u];
        int32_t code = 0, k = 0;
        bk.maxcode[t][0] = -1;
        bk.valoff[t][0] = 0;
        for (int len = 1; len <= 16; len++) {
            const int32_t c = (int32_t)h.counts[len - 1];
            bk.valoff[t][len] = k - code;
            k += c;
            code += c;
            bk.maxcode[t][len] = c ? code - 1 : -1;
            code <<= 1;
        }
        bk.maxcode[t][17] = -1;
        bk.valoff[t][17] = 0;
    }
    __syncthreads();
    for (uint32_t i = t; i < 8u * 256u; i += blockDim.x) {
        const uint32_t k = i >> 8, bits = i & 255u;
        uint32_t e = 0;
        for (uint32_t len = 1; len <= 8u; len++) {
            const int32_t code = (int32_t)(bits >> (8u - len));
            if (code <= bk.maxcode[k][len]) {
                e = (len << 8) | bk.values[k][(uint32_t)(bk.valoff[k][len] + code) & 255u];
                break;
            }
        }
        bk.lut[k][bits] = (uint16_t)e;
    }
    __syncthreads();
    const uint32_t mcus = (uint32_t)f.mcus_x * (uint32_t)f.mcus_y, bpm = jpgd_blocks_per_mcu(f), luma = bpm == 1u ? 1u : bpm - 2u;
    const uint32_t per = f.restart_interval ? (uint32_t)f.restart_interval : mcus;
    const uint2* iv = a.intervals + f.interval_begin;
    for (uint32_t k = blockIdx.y * blockDim.x + t; k < f.n_intervals; k += gridDim.y * blockDim.x) {
        const uint2 range = iv[k];
        JpgdBits b;
        b.p = a.files + f.file_offset;
        b.pos = range.x;
        b.end = range.y;                                              // start <= end <= the EOI's position < file_bytes (k_jpgd_intervals)
        b.buf = 0;
        b.n = 0;
        int32_t pred[3] = {0, 0, 0};
        uint32_t fail = 0;
        // the interval's MCUs: n_intervals = ceil(mcus / per), so m0 < mcus and every block index below is < mcus * bpm
        const uint32_t m0 = k * per, m1 = min(mcus, m0 + per);
        for (uint32_t m = m0; m < m1 && !fail; m++) {
            for (uint32_t j = 0; j < bpm && !fail; j++) {
                const uint32_t c = j < luma ? 0u : j - luma + 1u;
                const uint8_t* q = bk.quant[f.tq[c] & 3u];
                int16_t* block = reinterpret_cast<int16_t*>(a.coef + f.coef_offset) + ((size_t)m * bpm + j) * 64u;
                uint4* block4 = reinterpret_cast<uint4*>(block);      // 128 bytes, 16-aligned (coef_offset is; the area is 256-aligned)
#pragma unroll
                for (int i = 0; i < 8; i++) block4[i] = make_uint4(0u, 0u, 0u, 0u);
                int s = jpgd_symbol(b, bk, f.td[c] & 3u);
                if (s < 0) { fail = (uint32_t)-s; break; }
                if (s & 15) {                                         // (a DC symbol is at most 15: host-checked)
                    int32_t v;
                    if (!jpgd_receive(b, (uint32_t)s & 15u, v)) { fail = EGS_JPEG_SHORT; break; }
                    pred[c] += v;
                }
                const int32_t dcv = pred[c] * (int32_t)q[0];          // |pred| <= 32768 is checked before it grows further: no overflow
                if (pred[c] < -32768 || pred[c] > 32767 || dcv < -32768 || dcv > 32767) { fail = EGS_JPEG_COEF_RANGE; break; }
                block[0] = (int16_t)dcv;
                uint32_t at = 1;
                while (at < 64u) {
                    const int rs = jpgd_symbol(b, bk, 4u + (f.ta[c] & 3u));
                    if (rs < 0) { fail = (uint32_t)-rs; break; }
                    const uint32_t r = (uint32_t)rs >> 4, sz = (uint32_t)rs & 15u;
                    if (sz == 0u) {
                        if (r != 15u) break;
                        at += 16u;
                        if (at > 63u) { fail = EGS_JPEG_INDEX; break; }
                        continue;
                    }
                    at += r;
                    if (at > 63u) { fail = EGS_JPEG_INDEX; break; }
                    int32_t v;
                    if (!jpgd_receive(b, sz, v)) { fail = EGS_JPEG_SHORT; break; }
                    const uint32_t nat = bk.zigzag[at];               // < 64
                    v *= (int32_t)q[nat];                              // |v| < 2^15, q < 2^8
                    if (v < -32768 || v > 32767) { fail = EGS_JPEG_COEF_RANGE; break; }
                    block[nat] = (int16_t)v;
                    at++;
                }
            }
        }
        if (!fail) {
            jpgd_fill(b);
            if (b.n >= 8u || b.pos < b.end) fail = EGS_JPEG_LEFT_OVER;
        }
        if (fail) atomicMin(&a.words[file].key, (k << 8) | fail);
    }
}

// ---- (c) the inverse DCT -----------------------------------------------------------------------------------------------------------------
// One 1-D pass of the `islow` inverse DCT (jpeg.py idct_pass, expression for expression).  With |v[i]| <= 2^15 every intermediate is below
// 2^15 * 61 214 + 2^17 < 2^31 (jpeg.py idct_forms).
__device__ __forceinline__ void jpgd_pass(int32_t v[8], int shift) {
    int32_t z2 = v[2], z3 = v[6];
    int32_t z1 = (z2 + z3) * 4433;
    int32_t tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
    int32_t tmp0 = (v[0] + v[4]) * 8192, tmp1 = (v[0] - v[4]) * 8192;
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int32_t t0 = v[7], t1 = v[5], t2 = v[3], t3 = v[1];
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
    int32_t z4 = t1 + t3;
    const int32_t z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    const int32_t half = 1 << (shift - 1);
    v[0] = (tmp10 + t3 + half) >> shift; v[7] = (tmp10 - t3 + half) >> shift;
    v[1] = (tmp11 + t2 + half) >> shift; v[6] = (tmp11 - t2 + half) >> shift;
    v[2] = (tmp12 + t1 + half) >> shift; v[5] = (tmp12 - t1 + half) >> shift;
    v[3] = (tmp13 + t0 + half) >> shift; v[4] = (tmp13 - t0 + half) >> shift;
}

__global__ __launch_bounds__(JPGD_WG) void k_jpgd_idct(JpgdArgs a) {
    __shared__ int32_t ws[32][8][9];                                  // [block][row][column], rows padded against bank conflicts
    const uint32_t t = threadIdx.x, file = blockIdx.x, lane8 = t & 7u, slot = t >> 3;
    const JpgdWords w = a.words[file];
    if (w.scan != EGS_JPEG_OK || w.key != JPGD_NONE) return;          // (uniform; written by the launches before)
    const egs_jpeg_file f = a.desc[file];
    const uint32_t mcus = (uint32_t)f.mcus_x * (uint32_t)f.mcus_y, bpm = jpgd_blocks_per_mcu(f), luma = bpm == 1u ? 1u : bpm - 2u;
    const uint32_t n_blocks = mcus * bpm;                             // < 2^24 * 6
    const uint32_t luma_pitch = (uint32_t)f.mcus_x * (uint32_t)f.hs * 8u, chroma_pitch = (uint32_t)f.mcus_x * 8u;
    const size_t luma_bytes = (size_t)mcus * luma * 64u, chroma_bytes = (size_t)mcus * 64u;
    const int16_t* coef = reinterpret_cast<const int16_t*>(a.coef + f.coef_offset);
    uint8_t* planes = a.planes + f.plane_offset;
    bool out_of_range = false;
    for (uint32_t b0 = blockIdx.y * 32u; b0 < n_blocks; b0 += gridDim.y * 32u) {      // (uniform bounds: the barriers below are reached by all)
        const uint32_t blk = b0 + slot;
        const bool live = blk < n_blocks;
        int32_t v[8];
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) v[r] = (int32_t)coef[(size_t)blk * 64u + (uint32_t)r * 8u + lane8];      // column lane8
            jpgd_pass(v, 11);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                out_of_range = out_of_range || v[r] < -32768 || v[r] > 32767;
                ws[slot][r][lane8] = v[r];
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = ws[slot][lane8][c];                   // row lane8
            // a workspace value outside int16 makes the file fail (below); the row pass of such a block may wrap, its bytes are never used
            jpgd_pass(v, 18);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                lo |= (uint32_t)min(255, max(0, v[c] + 128)) << (8 * c);
                hi |= (uint32_t)min(255, max(0, v[c + 4] + 128)) << (8 * c);
            }
            const uint32_t m = blk / bpm, j = blk - m * bpm, mx = m % (uint32_t)f.mcus_x, my = m / (uint32_t)f.mcus_x;
            size_t at;                                                // row lane8 of the block inside its plane: 8 bytes, 8-aligned
            if (j < luma) {
                const uint32_t bx = mx * (uint32_t)f.hs + j % (uint32_t)f.hs, by = my * (uint32_t)f.vs + j / (uint32_t)f.hs;
                at = ((size_t)by * 8u + lane8) * luma_pitch + (size_t)bx * 8u;            // < luma_bytes: by < mcus_y vs, bx < mcus_x hs
            } else {
                at = luma_bytes + (size_t)(j - luma) * chroma_bytes + ((size_t)my * 8u + lane8) * chroma_pitch + (size_t)mx * 8u;
            }
            *reinterpret_cast<uint2*>(planes + at) = make_uint2(lo, hi);
        }
        __syncthreads();
    }
    if (out_of_range) atomicOr(&a.words[file].range, 1u);
}

// ---- (d) chroma upsampling and colour ---------------------------------------------------------------------------------------------------------
// The chroma sample at output pixel (x, y) (jpeg.py upsample): p is the plane, pitch its row length, cw x ch its cropped size.
__device__ __forceinline__ int32_t jpgd_chroma(const uint8_t* p, uint32_t pitch, int32_t cw, int32_t ch, int32_t x, int32_t y, int32_t hs, int32_t vs) {
    if (hs == 1) return (int32_t)p[(size_t)y * pitch + x];
    const int32_t i = x >> 1, j = vs == 2 ? y >> 1 : y;                // i < cw, j < ch: x < W <= 2 cw, y < H <= vs ch
    if (cw <= 2) return (int32_t)p[(size_t)j * pitch + i];
    const uint8_t* near = p + (size_t)j * pitch;
    if (vs == 1) {
        const int32_t v = near[i];
        if (x == 0 || x == 2 * cw - 1) return v;
        return (x & 1) ? (3 * v + (int32_t)near[i + 1] + 2) >> 2 : (3 * v + (int32_t)near[i - 1] + 1) >> 2;      // 0 < x < 2 cw - 1: i - 1 >= 0, i + 1 < cw
    }
    const int32_t jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const uint8_t* far = p + (size_t)jf * pitch;
    const int32_t s = 3 * (int32_t)near[i] + (int32_t)far[i];
    if (x & 1) {
        const int32_t k = min(i + 1, cw - 1);
        return (3 * s + 3 * (int32_t)near[k] + (int32_t)far[k] + 7) >> 4;
    }
    const int32_t k = max(i - 1, 0);
    return (3 * s + 3 * (int32_t)near[k] + (int32_t)far[k] + 8) >> 4;
}

__global__ __launch_bounds__(JPGD_WG) void k_jpgd_colour(JpgdArgs a) {
    const uint32_t file = blockIdx.x;
    const JpgdWords w = a.words[file];
    uint32_t status = w.scan;
    if (status == EGS_JPEG_OK && w.key != JPGD_NONE) status = (w.key & 255u) == EGS_JPEG_COEF_RANGE ? (uint32_t)EGS_JPEG_COEF_RANGE : w.key;
    if (status == EGS_JPEG_OK && w.range) status = EGS_JPEG_WORKSPACE_RANGE;
    if (blockIdx.y == 0 && threadIdx.x == 0) a.status[file] = status;
    if (status != EGS_JPEG_OK) return;                                // (uniform)
    const egs_jpeg_file f = a.desc[file];
    const int32_t W = f.width, H = f.height, hs = f.hs, vs = f.vs;
    const uint32_t mcus = (uint32_t)f.mcus_x * (uint32_t)f.mcus_y;
    const uint32_t luma_pitch = (uint32_t)f.mcus_x * (uint32_t)hs * 8u, chroma_pitch = (uint32_t)f.mcus_x * 8u;
    const uint8_t* py = a.planes + f.plane_offset;
    uint8_t* out = a.out + f.out_offset;
    const uint32_t pixels = (uint32_t)W * (uint32_t)H;                // < 2^31 / channels (host-checked)
    if (f.channels == 1) {
        for (uint32_t i = blockIdx.y * JPGD_WG + threadIdx.x; i < pixels; i += gridDim.y * JPGD_WG) {
            const uint32_t y = i / (uint32_t)W, x = i - y * (uint32_t)W;
            out[i] = py[(size_t)y * luma_pitch + x];
        }
        return;
    }
    const uint8_t* pcb = py + (size_t)mcus * (uint32_t)(hs * vs) * 64u;
    const uint8_t* pcr = pcb + (size_t)mcus * 64u;
    const int32_t cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    for (uint32_t i = blockIdx.y * JPGD_WG + threadIdx.x; i < pixels; i += gridDim.y * JPGD_WG) {
        const int32_t y = (int32_t)(i / (uint32_t)W), x = (int32_t)(i - (uint32_t)y * (uint32_t)W);
        const int32_t yy = py[(size_t)y * luma_pitch + x];
        const int32_t cb = jpgd_chroma(pcb, chroma_pitch, cw, ch, x, y, hs, vs) - 128, cr = jpgd_chroma(pcr, chroma_pitch, cw, ch, x, y, hs, vs) - 128;
        const int32_t r = yy + ((91881 * cr + 32768) >> 16);
        const int32_t g = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        const int32_t b = yy + ((116130 * cb + 32768) >> 16);
        uint8_t* o = out + (size_t)i * 3u;                            // 3 i + 2 < 3 W H
        o[0] = (uint8_t)min(255, max(0, r));
        o[1] = (uint8_t)min(255, max(0, g));
        o[2] = (uint8_t)min(255, max(0, b));
    }
}

// counts that fit the code space, at most 256 symbols, and for a DC table no symbol above 15
bool table_ok(const egs_jpeg_huffman& h, bool dc) {
    uint32_t code = 0, total = 0;
    for (int len = 1; len <= 16; len++) {
        code += h.counts[len - 1];
        total += h.counts[len - 1];
        if (code > (1u << len)) return false;
        code <<= 1;
    }
    if (total > 256) return false;
    for (uint32_t k = 0; dc && k < total; k++)
        if (h.values[k] > 15) return false;
    return true;
}

}  // namespace

extern "C" {

size_t egs_jpeg_decode_scratch_bytes(int n_files, int n_intervals, size_t coef_bytes, size_t plane_bytes) {
    if (n_files < 1 || n_intervals < 1) return 0;
    return egs_align((size_t)n_files * sizeof(JpgdWords)) + egs_align((size_t)n_intervals * sizeof(uint2)) + egs_align(coef_bytes) + egs_align(plane_bytes);
}

int egs_jpeg_decode_phases(int n_files, const uint8_t* files, size_t files_bytes, const egs_jpeg_file* desc_host, const egs_jpeg_file* desc_device,
                           const egs_jpeg_tables* tables_host, const egs_jpeg_tables* tables_device, int n_intervals, uint8_t* out,
                           size_t out_bytes, uint32_t* status, void* scratch, size_t scratch_bytes, void* stream, int phases) {
    if (phases < 1 || phases > 15) return EGS_ERR_ARG;
    if (const int e = decode_open(n_files, n_intervals, files, desc_host, desc_device, tables_host, tables_device, 8, out, status, scratch)) return e;
    size_t coef_total = 0, plane_total = 0, file_end = 0, out_end = 0;
    uint64_t interval_next = 0, max_intervals = 0, max_blocks = 0, max_pixels = 0;
    for (int i = 0; i < n_files; i++) {
        const egs_jpeg_file& f = desc_host[i];
        if (f.width < 1 || f.height < 1 || f.width > JPGD_MAX_SIDE || f.height > JPGD_MAX_SIDE || (f.channels != 1 && f.channels != 3)) return EGS_ERR_RANGE;
        const bool sampling = f.channels == 1 ? (f.hs == 1 && f.vs == 1) : ((f.hs == 1 && f.vs == 1) || (f.hs == 2 && (f.vs == 1 || f.vs == 2)));
        if (!sampling || f.restart_interval < 0 || f.restart_interval > 65535) return EGS_ERR_RANGE;
        const uint64_t pixels = (uint64_t)f.height * (uint64_t)f.width * (uint64_t)f.channels;
        if (pixels >= ((uint64_t)1 << 31) || f.file_bytes >= ((uint64_t)1 << 31)) return EGS_ERR_RANGE;
        // the counts follow from the geometry
        if (f.mcus_x != (f.width + 8 * f.hs - 1) / (8 * f.hs) || f.mcus_y != (f.height + 8 * f.vs - 1) / (8 * f.vs)) return EGS_ERR_ARG;
        const uint64_t mcus = (uint64_t)f.mcus_x * (uint64_t)f.mcus_y, bpm = f.channels == 3 ? (uint64_t)(f.hs * f.vs + 2) : 1;
        const uint64_t want = f.restart_interval ? (mcus + (uint64_t)f.restart_interval - 1) / (uint64_t)f.restart_interval : 1;
        if (f.n_intervals != want || f.interval_begin != interval_next || interval_next + want > (uint64_t)n_intervals) return EGS_ERR_ARG;
        interval_next += want;
        // files, coefficients, planes and outputs each in ascending order without overlap, and inside their buffers (decode_args.h)
        if (!decode_region(f.file_offset, f.file_bytes, 1, files_bytes, &file_end)) return EGS_ERR_ARG;
        if (f.entropy_begin >= f.file_bytes || (uint64_t)f.entropy_begin + f.entropy_bytes != f.file_bytes) return EGS_ERR_ARG;
        if (!decode_region(f.coef_offset, up16((size_t)(mcus * bpm * 128)), 16, scratch_bytes, &coef_total) ||
            !decode_region(f.plane_offset, up16((size_t)(mcus * bpm * 64)), 16, scratch_bytes, &plane_total) ||
            !decode_region(f.out_offset, pixels, 1, out_bytes, &out_end)) return EGS_ERR_ARG;
        const egs_jpeg_tables& tb = tables_host[i];
        for (int c = 0; c < f.channels; c++) {
            if (f.tq[c] > 3 || f.td[c] > 3 || f.ta[c] > 3) return EGS_ERR_ARG;
            for (int k = 0; k < 64; k++)
                if (tb.quant[f.tq[c]][k] == 0) return EGS_ERR_ARG;
            if (!table_ok(tb.dc[f.td[c]], true) || !table_ok(tb.ac[f.ta[c]], false)) return EGS_ERR_ARG;
        }
        max_intervals = want > max_intervals ? want : max_intervals;
        max_blocks = mcus * bpm > max_blocks ? mcus * bpm : max_blocks;
        max_pixels = pixels > max_pixels ? pixels : max_pixels;
    }
    if (interval_next != (uint64_t)n_intervals) return EGS_ERR_ARG;
    const size_t need = egs_jpeg_decode_scratch_bytes(n_files, n_intervals, coef_total, plane_total);
    if (need > scratch_bytes) return EGS_ERR_ARG;
    JpgdArgs a;
    a.files = files; a.desc = desc_device; a.tables = tables_device; a.out = out; a.status = status;
    uint8_t* s = (uint8_t*)scratch;
    a.words = reinterpret_cast<JpgdWords*>(s);
    s += egs_align((size_t)n_files * sizeof(JpgdWords));
    a.intervals = reinterpret_cast<uint2*>(s);
    s += egs_align((size_t)n_intervals * sizeof(uint2));
    a.coef = s;
    a.planes = s + egs_align(coef_total);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    const auto slices = [](uint64_t work, uint64_t per, uint64_t cap) { return (unsigned)(work <= per ? 1 : (work + per - 1) / per > cap ? cap : (work + per - 1) / per); };
    if (phases & 1) hipLaunchKernelGGL(k_jpgd_intervals, dim3((unsigned)n_files), dim3(JPGD_WG), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (phases & 2) {
        const unsigned wg = max_intervals <= 64 ? 64u : (unsigned)JPGD_WG;          // a file of few intervals: one wave holds them
        hipLaunchKernelGGL(k_jpgd_entropy, dim3((unsigned)n_files, slices(max_intervals, wg, 1024)), dim3(wg), 0, st, a);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (phases & 4) hipLaunchKernelGGL(k_jpgd_idct, dim3((unsigned)n_files, slices(max_blocks, 128, 4096)), dim3(JPGD_WG), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (phases & 8) hipLaunchKernelGGL(k_jpgd_colour, dim3((unsigned)n_files, slices(max_pixels, 1024, 4096)), dim3(JPGD_WG), 0, st, a);
    return (int)hipGetLastError();
}

int egs_jpeg_decode(int n_files, const uint8_t* files, size_t files_bytes, const egs_jpeg_file* desc_host, const egs_jpeg_file* desc_device,
                    const egs_jpeg_tables* tables_host, const egs_jpeg_tables* tables_device, int n_intervals, uint8_t* out, size_t out_bytes,
                    uint32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    return egs_jpeg_decode_phases(n_files, files, files_bytes, desc_host, desc_device, tables_host, tables_device, n_intervals, out, out_bytes, status,
                                  scratch, scratch_bytes, stream, 15);
}

}  // extern "C"
