// png_decode.hip -- 8-bit PNG files read on the device (include/egs_raster.h egs_png_decode): the bytes of a batch of files, uploaded as they
// are, become interleaved uint8 [h][w][C] arrays for the ingest kernel (csrc/ingest.hip) and the metric kernels.  The host has walked the
// chunks (egogaussian_amd/png.py parse: signature, order, lengths, IHDR, the CRC of the small critical chunks) and built two tables -- a
// record per file and one per IDAT chunk; it has not touched an IDAT byte.  Everything about those bytes is decided here, and reported in
// one status word per file: 0, or the first failure (the codes are csrc/png_inflate.h's).
//
// Launches (three per batch, whatever the files hold: no allocation, no synchronisation, no global state; can be captured).
//   k_pngd_gather    grid (IDAT chunks of the batch), 256 lanes.  Copies the payload to its place in the file's contiguous stream in scratch
//                    and computes the chunk's CRC-32 -- every lane the CRC of its slice, combined by multiplication with x^(8 n) mod P as
//                    png.hip does -- and leaves a flag word per chunk: stored CRC equal or not.
//   k_pngd_inflate   one wave per file, 39 KiB of LDS (the 32 KiB window as a ring, the code tables, a buffer of the stream): four files
//                    per CU.  The first flagged chunk of the file, else png_inflate.h's pngi_inflate: the symbol loop runs uniformly in the
//                    wave, the lanes share table construction, match copies, the flushes of the window to scratch and the Adler-32.
//   k_pngd_unfilter  one wave per file.  Refuses a filter type above 4, then undoes the filters in blocks of 64 rows: lane l works on row
//                    y0 + l one pixel behind lane l - 1, takes b and c (the pixels above and above-left) from that lane by a shift of the
//                    wave and keeps a (the pixel to the left) itself; a block takes W + 63 steps.  The predictor is selected per lane
//                    without a branch.  Lane 0 reads the row above the block from the output, which the block before it wrote.
// egs_png_decode_ex adds, behind flags (include/egs_raster.h), the segmented route -- k_pngd_measure, k_pngd_scan, k_pngd_place in front of
// k_pngd_inflate, which then skips the files they decoded (png_segments.h).
// A file whose status is not 0 leaves its output unspecified inside its own slot; nothing outside a file's slots is written (the bounds
// argument is in png_inflate.h for the inflater, and at each index below for the rest).
#include "egs_common.h"
#include "png_inflate.h"
#include "png_segments.h"
#include "png_common.h"
#include "decode_args.h"

#define PNGD_WG 256
#define PNGD_CRC_IDAT 0x35af061eu            // CRC-32 of the four bytes "IDAT"
#define PNGD_MAX_SIDE 32767

namespace {

struct PngdArgs {
    const uint8_t* files;
    const egs_png_file* desc;
    const egs_png_idat* idat;
    uint8_t* out;
    uint32_t* status;
    uint8_t* scratch;                        // flag words [n_idat], then the streams, then the inflated data
    unsigned long long stream_base, inflate_base;
    // egs_png_decode_ex with EGS_PNG_SEGMENTS (else NULL: the launches below that do not name them run as they always did)
    PngsRecord* records;                     // scratch: a record per IDAT chunk
    uint32_t* routes;                        // scratch: the route word per file, which k_pngd_inflate reads as its skip array
    uint32_t* route_out;                     // the caller's copy, or NULL
};

static_assert(PNGS_MAX == EGS_PNG_SEGMENT_MAX && sizeof(PngsRecord) == 16, "png_segments.h and egs_raster.h disagree");

__device__ __forceinline__ uint32_t pngd_x8n(uint32_t k) {       // x^(8 k) mod P: at most 32 squarings
    uint32_t p = 0x80000000u, sq = 0x00800000u;
#pragma unroll 1
    while (k) {
        if (k & 1u) p = png_mulmod(sq, p);
        sq = png_mulmod(sq, sq);
        k >>= 1;
    }
    return p;
}

__global__ __launch_bounds__(PNGD_WG) void k_pngd_gather(PngdArgs a) {
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t acc;
    const uint32_t t = threadIdx.x;
    {
        uint32_t c = t;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
        crc_tab[t] = c;
    }
    if (t == 0) acc = 0;
    __syncthreads();
    const egs_png_idat e = a.idat[blockIdx.x];
    const egs_png_file f = a.desc[e.file];
    // the host entry has checked: src + length + 4 <= file_bytes, dst + length <= stream_bytes, the file and its stream inside their buffers
    const uint8_t* src = a.files + f.file_offset + e.src;
    uint8_t* dst = a.scratch + a.stream_base + f.stream_offset + e.dst;
    const uint32_t len = e.length;
    for (uint32_t i = t; i < len; i += PNGD_WG) dst[i] = src[i];
    const uint32_t cs = (len + PNGD_WG - 1) / PNGD_WG;
    const uint32_t b0 = min(len, t * cs), b1 = min(len, b0 + cs);
    uint32_t mine = 0;
    if (b0 < b1) {
        uint32_t c = 0xffffffffu;
        for (uint32_t i = b0; i < b1; i++) c = crc_tab[(c ^ src[i]) & 255u] ^ (c >> 8);
        mine = png_mulmod(pngd_x8n(len - b1), c ^ 0xffffffffu);
    }
    if (t == 0) mine ^= png_mulmod(pngd_x8n(len), PNGD_CRC_IDAT);       // the chunk type in front of the payload
    if (mine) atomicXor(&acc, mine);
    __syncthreads();
    if (t == 0) {
        const uint32_t stored = ((uint32_t)src[len] << 24) | ((uint32_t)src[len + 1] << 16) | ((uint32_t)src[len + 2] << 8) | (uint32_t)src[len + 3];
        reinterpret_cast<uint32_t*>(a.scratch)[blockIdx.x] = stored == acc ? 0u : 1u;
    }
}

// ---- the segmented route (png_segments.h): measure per chunk, scan per file, place per chunk -------------------------------------------------
// 15 KiB of LDS (the 8 KiB segment buffer, the code tables, the buffer of the stream): ten workgroups per CU.
__device__ __forceinline__ void pngd_chunk(const PngdArgs& a, uint32_t k, PngsState& s, uint32_t& start, bool& first, egs_png_file& f, egs_png_idat& e) {
    e = a.idat[k];
    f = a.desc[e.file];
    s.in = a.scratch + a.stream_base + f.stream_offset;               // the file's stream; the wave reads below n = this chunk's end
    s.n = e.dst + e.length;                                           // <= stream_bytes (host-checked: the chunks tile the stream)
    s.out = nullptr;
    start = e.dst;
    first = k == f.idat_begin;
}

__global__ __launch_bounds__(64) void k_pngd_measure(PngdArgs a) {
    __shared__ PngsMem mem;
    PngsState s;
    s.m = &mem;
    uint32_t start;
    bool first;
    egs_png_file f;
    egs_png_idat e;
    pngd_chunk(a, blockIdx.x, s, start, first, f, e);
    const bool flag = reinterpret_cast<const uint32_t*>(a.scratch)[blockIdx.x] != 0u;
    const PngsRecord r = pngs_measure(s, start, first, e.length == 0u, flag);
    if (threadIdx.x == 0) a.records[blockIdx.x] = r;
}

__global__ __launch_bounds__(64) void k_pngd_scan(PngdArgs a) {
    const uint32_t file = blockIdx.x;
    const egs_png_file f = a.desc[file];
    const uint32_t expect = (uint32_t)f.height * (1u + (uint32_t)f.width * (uint32_t)f.channels);
    const uint32_t route = pngs_scan(a.records + f.idat_begin, (uint32_t)f.n_idat, expect);      // idat_begin + n_idat <= the table's length
    if (threadIdx.x == 0) {
        a.routes[file] = route;
        if (a.route_out) a.route_out[file] = route;
        if (route == PNGS_ROUTE_SEGMENTS) a.status[file] = PNGD_OK;  // (the serial wave, which writes every other status, skips this file)
    }
}

__global__ __launch_bounds__(64) void k_pngd_place(PngdArgs a) {
    __shared__ PngsMem mem;
    if (a.routes[a.idat[blockIdx.x].file] != PNGS_ROUTE_SEGMENTS) return;      // (uniform)
    const PngsRecord r = a.records[blockIdx.x];
    if (r.length == 0u) return;
    PngsState s;
    s.m = &mem;
    uint32_t start;
    bool first;
    egs_png_file f;
    egs_png_idat e;
    pngd_chunk(a, blockIdx.x, s, start, first, f, e);
    // aux + length <= the sum of the file's lengths = H (1 + W C): inside the file's inflated data
    pngs_place(s, start, first, r.length, a.scratch + a.inflate_base + f.inflate_offset + r.aux);
}

__global__ __launch_bounds__(64) void k_pngd_inflate(PngdArgs a) {
    __shared__ PngiMem mem;
    const uint32_t lane = threadIdx.x, file = blockIdx.x;
    if (a.routes && a.routes[file] == PNGS_ROUTE_SEGMENTS) return;    // (uniform) the segments of this file are in place
    const egs_png_file f = a.desc[file];
    const uint32_t* flags = reinterpret_cast<const uint32_t*>(a.scratch) + f.idat_begin;
    uint32_t bad = 0xffffffffu;
    for (uint32_t k = lane; k < (uint32_t)f.n_idat; k += 64u)          // idat_begin + n_idat <= the table's length (host-checked)
        if (flags[k]) bad = min(bad, k);
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o));
    if (bad != 0xffffffffu) {
        if (lane == 0) a.status[file] = PNGD_IDAT_CRC | (bad << 8);
        return;
    }
    PngiState s;
    s.in = a.scratch + a.stream_base + f.stream_offset;
    s.n = f.stream_bytes;
    s.out = a.scratch + a.inflate_base + f.inflate_offset;
    s.expect = (uint32_t)f.height * (1u + (uint32_t)f.width * (uint32_t)f.channels);      // < 2^31 + 2^15 (host-checked)
    s.m = &mem;
    pngi_inflate(s);
    if (lane == 0) a.status[file] = s.status;
}

// rows of 1 + W C filtered bytes -> rows of W C bytes.  Reads infl[0, H (1 + W C)), writes out[0, H W C): y < H and 0 <= x < W at every index.
template <int C>
__device__ __forceinline__ void pngd_unfilter(const uint8_t* __restrict__ infl, uint8_t* out, int W, int H) {
    const int lane = threadIdx.x;
    const size_t rb = (size_t)W * C, sb = rb + 1;
    for (int y0 = 0; y0 < H; y0 += 64) {
        const int y = y0 + lane;
        const bool row = y < H;
        const int f = row ? (int)infl[(size_t)y * sb] : 0;
        const uint8_t* in_row = infl + (size_t)(row ? y : 0) * sb + 1;
        uint8_t* out_row = out + (size_t)(row ? y : 0) * rb;
        const uint8_t* above = out + (size_t)(y0 > 0 ? y0 - 1 : 0) * rb;         // lane 0's row above: the last row of the block before
        const int steps = W + min(64, H - y0) - 1;
        uint32_t r1 = 0, r2 = 0, cprev = 0;                       // the lane's pixels of the two steps before, channels packed in bytes
        for (int s = 0; s < steps; s++) {
            const int x = s - lane;
            uint32_t b = (uint32_t)__shfl_up((int)r1, 1), c = (uint32_t)__shfl_up((int)r2, 1);
            if (lane == 0) {
                b = 0;
                if (y0 > 0 && x < W) {
#pragma unroll
                    for (int ch = 0; ch < C; ch++) b |= (uint32_t)above[(size_t)x * C + ch] << (8 * ch);
                }
                c = cprev;
                cprev = b;
            }
            uint32_t v = 0;
            if (row && x >= 0 && x < W) {
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    const int pa = (int)((r1 >> (8 * ch)) & 255u), pb = (int)((b >> (8 * ch)) & 255u), pc = (int)((c >> (8 * ch)) & 255u);
                    int pred = f == 1 ? pa : 0;
                    pred = f == 2 ? pb : pred;
                    pred = f == 3 ? (pa + pb) >> 1 : pred;
                    pred = f == 4 ? png_paeth(pa, pb, pc) : pred;
                    const uint32_t px = ((uint32_t)in_row[(size_t)x * C + ch] + (uint32_t)pred) & 255u;
                    out_row[(size_t)x * C + ch] = (uint8_t)px;
                    v |= px << (8 * ch);
                }
            }
            r2 = r1;
            r1 = v;
        }
        __threadfence_block();
        __syncthreads();                                          // the block's last row is in memory before lane 0 of the next block reads it
    }
}

__global__ __launch_bounds__(64) void k_pngd_unfilter(PngdArgs a) {
    const uint32_t lane = threadIdx.x, file = blockIdx.x;
    if (a.status[file]) return;                                   // (uniform)
    const egs_png_file f = a.desc[file];
    const uint8_t* infl = a.scratch + a.inflate_base + f.inflate_offset;
    const int W = f.width, H = f.height, C = f.channels;
    const size_t sb = (size_t)W * C + 1;
    uint32_t worst = 0;
    for (int y = (int)lane; y < H; y += 64) worst = max(worst, (uint32_t)infl[(size_t)y * sb]);
    for (int o = 32; o > 0; o >>= 1) worst = max(worst, (uint32_t)__shfl_xor((int)worst, o));
    if (worst > 4u) {
        if (lane == 0) a.status[file] = PNGD_FILTER;
        return;
    }
    uint8_t* out = a.out + f.out_offset;
    if (C == 3) pngd_unfilter<3>(infl, out, W, H);
    else pngd_unfilter<1>(infl, out, W, H);
}

}  // namespace

extern "C" {

size_t egs_png_decode_scratch_bytes(int n_idat, size_t total_stream_bytes, size_t total_inflate_bytes) {
    if (n_idat < 1) return 0;
    return egs_align((size_t)n_idat * 4) + egs_align(total_stream_bytes) + egs_align(total_inflate_bytes);
}

size_t egs_png_decode_scratch_bytes_ex(int n_idat, size_t total_stream_bytes, size_t total_inflate_bytes, int flags) {
    if (n_idat < 1 || (flags & ~EGS_PNG_SEGMENTS)) return 0;
    size_t need = egs_png_decode_scratch_bytes(n_idat, total_stream_bytes, total_inflate_bytes);
    if (flags & EGS_PNG_SEGMENTS) need += egs_align((size_t)n_idat * sizeof(PngsRecord)) + egs_align((size_t)n_idat * 4);
    return need;
}

int egs_png_decode_ex(int n_files, const uint8_t* files, size_t files_bytes, const egs_png_file* desc_host, const egs_png_file* desc_device,
                      const egs_png_idat* idat_host, const egs_png_idat* idat_device, int n_idat, uint8_t* out, size_t out_bytes,
                      uint32_t* status, void* scratch, size_t scratch_bytes, void* stream, int phases, int flags, uint32_t* route) {
    if (phases < 1 || phases > 7 || (flags & ~EGS_PNG_SEGMENTS) || ((uintptr_t)route & 3)) return EGS_ERR_ARG;
    if (const int e = decode_open(n_files, n_idat, files, desc_host, desc_device, idat_host, idat_device, 4, out, status, scratch)) return e;
    size_t stream_total = 0, inflate_total = 0, file_end = 0, out_end = 0;
    uint32_t idat_next = 0;
    for (int i = 0; i < n_files; i++) {
        const egs_png_file& f = desc_host[i];
        if (f.width < 1 || f.height < 1 || f.width > PNGD_MAX_SIDE || f.height > PNGD_MAX_SIDE || (f.channels != 1 && f.channels != 3)) return EGS_ERR_RANGE;
        const uint64_t pixels = (uint64_t)f.height * (uint64_t)f.width * (uint64_t)f.channels;
        if (pixels >= ((uint64_t)1 << 31) || f.stream_bytes >= (1u << 31)) return EGS_ERR_RANGE;
        const uint64_t inflated = pixels + (uint64_t)f.height;
        // files, streams, inflated data and outputs each in ascending order without overlap, and inside their buffers (decode_args.h; both
        // rooms are below 2^32)
        if (!decode_region(f.file_offset, f.file_bytes, 1, files_bytes, &file_end) ||
            !decode_region(f.stream_offset, up16(f.stream_bytes), 16, scratch_bytes, &stream_total) ||
            !decode_region(f.inflate_offset, up16((size_t)inflated), 16, scratch_bytes, &inflate_total) ||
            !decode_region(f.out_offset, pixels, 1, out_bytes, &out_end)) return EGS_ERR_ARG;
        // the file's chunks: consecutive in the table, inside the file, tiling its stream
        if (f.n_idat < 1 || f.idat_begin != idat_next || (uint64_t)f.idat_begin + (uint64_t)f.n_idat > (uint64_t)n_idat) return EGS_ERR_ARG;
        uint64_t at = 0;
        for (uint32_t k = f.idat_begin; k < f.idat_begin + (uint32_t)f.n_idat; k++) {
            const egs_png_idat& e = idat_host[k];
            if (e.file != (uint32_t)i || e.dst != at || (uint64_t)e.src + e.length + 4 > f.file_bytes) return EGS_ERR_ARG;
            at += e.length;
        }
        if (at != f.stream_bytes) return EGS_ERR_ARG;
        idat_next = f.idat_begin + (uint32_t)f.n_idat;
    }
    if (idat_next != (uint32_t)n_idat) return EGS_ERR_ARG;
    const size_t need = egs_png_decode_scratch_bytes_ex(n_idat, stream_total, inflate_total, flags);
    if (need > scratch_bytes) return EGS_ERR_ARG;
    PngdArgs a;
    a.files = files; a.desc = desc_device; a.idat = idat_device; a.out = out; a.status = status; a.scratch = (uint8_t*)scratch;
    a.stream_base = (unsigned long long)egs_align((size_t)n_idat * 4);
    a.inflate_base = a.stream_base + (unsigned long long)egs_align(stream_total);
    a.records = nullptr; a.routes = nullptr; a.route_out = nullptr;
    if (flags & EGS_PNG_SEGMENTS) {
        const unsigned long long records_base = a.inflate_base + (unsigned long long)egs_align(inflate_total);
        a.records = reinterpret_cast<PngsRecord*>((uint8_t*)scratch + records_base);
        a.routes = reinterpret_cast<uint32_t*>((uint8_t*)scratch + records_base + egs_align((size_t)n_idat * sizeof(PngsRecord)));
        a.route_out = route;
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (phases & 1) hipLaunchKernelGGL(k_pngd_gather, dim3((unsigned)n_idat), dim3(PNGD_WG), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if ((phases & 2) && (flags & EGS_PNG_SEGMENTS)) {
        hipLaunchKernelGGL(k_pngd_measure, dim3((unsigned)n_idat), dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_pngd_scan, dim3((unsigned)n_files), dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_pngd_place, dim3((unsigned)n_idat), dim3(64), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (phases & 2) hipLaunchKernelGGL(k_pngd_inflate, dim3((unsigned)n_files), dim3(64), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (phases & 4) hipLaunchKernelGGL(k_pngd_unfilter, dim3((unsigned)n_files), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

int egs_png_decode_phases(int n_files, const uint8_t* files, size_t files_bytes, const egs_png_file* desc_host, const egs_png_file* desc_device,
                          const egs_png_idat* idat_host, const egs_png_idat* idat_device, int n_idat, uint8_t* out, size_t out_bytes,
                          uint32_t* status, void* scratch, size_t scratch_bytes, void* stream, int phases) {
    return egs_png_decode_ex(n_files, files, files_bytes, desc_host, desc_device, idat_host, idat_device, n_idat, out, out_bytes, status, scratch,
                             scratch_bytes, stream, phases, 0, nullptr);
}

int egs_png_decode(int n_files, const uint8_t* files, size_t files_bytes, const egs_png_file* desc_host, const egs_png_file* desc_device,
                   const egs_png_idat* idat_host, const egs_png_idat* idat_device, int n_idat, uint8_t* out, size_t out_bytes,
                   uint32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    return egs_png_decode_phases(n_files, files, files_bytes, desc_host, desc_device, idat_host, idat_device, n_idat, out, out_bytes, status, scratch,
                                 scratch_bytes, stream, 7);
}

}  // extern "C"
