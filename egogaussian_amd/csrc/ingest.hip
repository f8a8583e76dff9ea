// ingest.hip -- the producer of the 8-bit frame store (include/egs_raster.h egs_frame_ingest, egs_resample_tables): one source-resolution
// 8-bit array (image, hand mask or object mask, interleaved [h][w][C] as np.array(pil_image) gives it) resized the way PIL.Image.resize
// does on modes L and RGB -- bicubic, antialiased, two separable passes of 22-bit fixed-point coefficients with an 8-bit intermediate -- and
// written straight into one frame's rows of a store: CHW image bytes, or one bit plane.  Every value has one right answer;
// egogaussian_amd/ingest.py resize_u8 / binarize are the torch statement of it.
//
// Coefficients.  kk[out][ksize] and bounds[out] = {xmin, xmax} of an axis are HOST arithmetic in double (egs_resample_tables below, the order
// of evaluation of Pillow's precompute_coeffs) and reach the kernel as device arrays: the kernel does integer arithmetic only, so its
// result does not depend on how a device evaluates a double expression.
//
// Mapping.  A workgroup of 256 lanes owns a tile of ING_TW x ING_TH = 64 x 16 output pixels.
//   phase 1  the source rows the tile's vertical taps reach, [row0, row1) -- at most 15 scale + 2 support + 2 <= 154 of them for scale <= 8 --
//            go through the horizontal pass for the tile's 64 columns: lane -> column, the waves stride the rows; each value is rounded
//            and clamped to a byte and stored in LDS as inter[row][channel][column].  A horizontal pass that is skipped copies the bytes.
//   phase 2  lane -> column, wave -> output row (4 rows per wave): the vertical taps from LDS (or the byte itself when that pass is
//            skipped), then
//              image  one byte per channel to img[c H W + Y W + X], times the pixel's bit of the object plane for the object-loss layout
//              mask   the wave's 64 bits by __ballot; pixel p = Y W + X0 .. + 63 of the plane covers up to three words, whose non-zero
//                     parts lanes 0 .. 2 OR in.  The frame's words of that plane were cleared by a memset node in front of the launch:
//                     W may be anything, and an OR gives the same word in any order.
//   LDS: int32 kk_h[64][ks_h], kk_v[16][ks_v], bounds 2 x (64 + 16), then rows_cap x C x 64 bytes: <= 11.2 KB + 29.6 KB.
//
// Safety.  Whatever the tables hold, {xmin, xmax} are clamped into the source and the tap count into ksize before anything is addressed with
// them, and [row0, row1) into rows_cap rows; stores go to pixels of the tile inside W x H only.
#include <math.h>

#include <vector>

#include "egs_common.h"

#define ING_TW 64
#define ING_TH 16
#define ING_WG 256
#define ING_PRECISION 22
#define ING_MAX_SCALE 8
#define ING_MAX_SIDE 32767

namespace {

struct IngestArgs {
    int H, W, h, w;                  // target and source size
    int ks_h, ks_v;                  // ksize of the axis, 0: the pass is skipped
    int rows_cap;                    // rows of the intermediate the LDS holds
    int plane;                       // EGS_INGEST_*
    int premul;                      // image: times the object plane's bit
};

__device__ __forceinline__ int clip8(int s) { return min(max(s >> ING_PRECISION, 0), 255); }

// grid: (ceil(W / 64), ceil(H / 16)); dynamic LDS: see above
template <int C>
__global__ __launch_bounds__(ING_WG) void k_frame_ingest(IngestArgs a, const uint8_t* __restrict__ src, const int32_t* __restrict__ kk_h,
                                                         const int32_t* __restrict__ bounds_h, const int32_t* __restrict__ kk_v,
                                                         const int32_t* __restrict__ bounds_v, uint8_t* __restrict__ img,
                                                         uint32_t* __restrict__ plane_out, const uint32_t* __restrict__ obj_plane) {
    extern __shared__ __attribute__((aligned(16))) int32_t ing_lds[];
    int32_t* kh = ing_lds;                                   // [64][ks_h]
    int32_t* kv = kh + ING_TW * a.ks_h;                      // [16][ks_v]
    int32_t* xb = kv + ING_TH * a.ks_v;                      // [64][2]
    int32_t* yb = xb + 2 * ING_TW;                           // [16][2]
    uint8_t* inter = reinterpret_cast<uint8_t*>(yb + 2 * ING_TH);      // [rows_cap][C][64]
    const int t = threadIdx.x;
    const int X0 = blockIdx.x * ING_TW, Y0 = blockIdx.y * ING_TH;

    // ---- the tile's slices of the tables ---------------------------------------------------------------------------------------------
    if (t < ING_TW) {
        const int X = X0 + t;
        int lo = 0, n = 0;
        if (X < a.W) {
            if (a.ks_h) {
                lo = min(max(bounds_h[2 * X], 0), a.w - 1);
                n = min(max(bounds_h[2 * X + 1], 0), min(a.ks_h, a.w - lo));
            } else { lo = X; n = 1; }                         // (w == W)
        }
        xb[2 * t] = lo; xb[2 * t + 1] = n;
    } else if (t < ING_TW + ING_TH) {
        const int y = t - ING_TW, Y = Y0 + y;
        int lo = 0, n = 0;
        if (Y < a.H) {
            if (a.ks_v) {
                lo = min(max(bounds_v[2 * Y], 0), a.h - 1);
                n = min(max(bounds_v[2 * Y + 1], 0), min(a.ks_v, a.h - lo));
            } else { lo = Y; n = 1; }                         // (h == H)
        }
        yb[2 * y] = lo; yb[2 * y + 1] = n;
    }
    for (int j = t; j < ING_TW * a.ks_h; j += ING_WG) {
        const long long g = (long long)X0 * a.ks_h + j;
        kh[j] = g < (long long)a.W * a.ks_h ? kk_h[g] : 0;
    }
    for (int j = t; j < ING_TH * a.ks_v; j += ING_WG) {
        const long long g = (long long)Y0 * a.ks_v + j;
        kv[j] = g < (long long)a.H * a.ks_v ? kk_v[g] : 0;
    }
    __syncthreads();

    // ---- phase 1: the horizontal pass of the rows this tile reads -----------------------------------------------------------------------
    const int y_last = min(ING_TH, a.H - Y0) - 1;            // >= 0: the grid covers H
    int row0 = yb[0], row1 = yb[2 * y_last] + yb[2 * y_last + 1];
#pragma unroll 1
    for (int y = 0; y <= y_last; y++) {                      // (monotone for honest tables; a tile of any table stays inside its rows)
        row0 = min(row0, yb[2 * y]);
        row1 = max(row1, yb[2 * y] + yb[2 * y + 1]);
    }
    const int nrows = min(row1 - row0, a.rows_cap);
    const int x = t & (ING_TW - 1);
    {
        const int xlo = xb[2 * x], xn = xb[2 * x + 1];
        const int32_t* k = kh + x * a.ks_h;
        for (int r = t >> 6; r < nrows; r += ING_WG / ING_TW) {
            const uint8_t* p = src + ((size_t)(row0 + r) * (size_t)a.w + (size_t)xlo) * C;
            int s[C];
            if (a.ks_h) {
#pragma unroll
                for (int c = 0; c < C; c++) s[c] = 1 << (ING_PRECISION - 1);
                for (int i = 0; i < xn; i++) {
                    const int kk = k[i];
#pragma unroll
                    for (int c = 0; c < C; c++) s[c] += (int)p[i * C + c] * kk;
                }
#pragma unroll
                for (int c = 0; c < C; c++) s[c] = clip8(s[c]);
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) s[c] = xn ? (int)p[c] : 0;
            }
#pragma unroll
            for (int c = 0; c < C; c++) inter[(r * C + c) * ING_TW + x] = (uint8_t)s[c];
        }
    }
    __syncthreads();

    // ---- phase 2: the vertical pass, then the store's bytes or bits ---------------------------------------------------------------------
    const int X = X0 + x;
    const size_t n_pix = (size_t)a.H * (size_t)a.W;
#pragma unroll 1
    for (int y = t >> 6; y <= y_last; y += ING_WG / ING_TW) {      // (y is the same in every lane of a wave)
        const int Y = Y0 + y;
        const bool valid = X < a.W;
        int off = min(max(yb[2 * y] - row0, 0), max(nrows - 1, 0));
        const int yn = min(yb[2 * y + 1], nrows - off);
        int v[C];
        if (a.ks_v) {
            const int32_t* k = kv + y * a.ks_v;
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = 1 << (ING_PRECISION - 1);
            for (int i = 0; i < yn; i++) {
                const int kk = k[i];
#pragma unroll
                for (int c = 0; c < C; c++) v[c] += (int)inter[((off + i) * C + c) * ING_TW + x] * kk;
            }
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = clip8(v[c]);
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = yn > 0 ? (int)inter[(off * C + c) * ING_TW + x] : 0;
        }
        const size_t p = (size_t)Y * (size_t)a.W + (size_t)X;
        if (a.plane == EGS_INGEST_IMAGE) {
            if (valid) {
                int keep = 1;
                if (a.premul) keep = (int)((obj_plane[p >> 5] >> (unsigned)(p & 31)) & 1u);
#pragma unroll
                for (int c = 0; c < C; c++) img[(size_t)c * n_pix + p] = (uint8_t)(v[c] * keep);
            }
        } else {
            bool any = false;
#pragma unroll
            for (int c = 0; c < C; c++) any = any || v[c] > 0;
            const bool bit = valid && (a.plane == EGS_INGEST_HAND_MASK ? !any : any);
            const unsigned long long m = __ballot(bit);      // bit j: pixel p0 + j
            const size_t p0 = (size_t)Y * (size_t)a.W + (size_t)X0;
            const unsigned sh = (unsigned)(p0 & 31);
            const int lane = t & 63;
            if (lane < 3) {
                uint32_t part;
                if (lane == 0) part = (uint32_t)(m << sh);
                else if (lane == 1) part = (uint32_t)(sh ? (m >> (32u - sh)) : (m >> 32));
                else part = sh ? (uint32_t)(m >> (64u - sh)) : 0u;
                if (part) atomicOr(plane_out + (p0 >> 5) + lane, part);      // a set bit is a pixel of the image: the word is inside the plane
            }
        }
    }
}

double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct AxisGeometry { double scale, filterscale, support; int ksize; };

AxisGeometry axis_geometry(int in, int out) {
    AxisGeometry g;
    g.filterscale = g.scale = (double)in / out;
    if (g.filterscale < 1.0) g.filterscale = 1.0;
    g.support = 2.0 * g.filterscale;
    g.ksize = (int)ceil(g.support) * 2 + 1;
    return g;
}

}  // namespace

extern "C" {

int egs_resample_ksize(int in, int out) {
    if (in < 1 || out < 1) return 0;
    return axis_geometry(in, out).ksize;
}

int egs_resample_tables(int in, int out, int32_t* kk, int32_t* bounds) {
    if (in < 1 || out < 1 || !kk || !bounds) return EGS_ERR_ARG;
    const AxisGeometry g = axis_geometry(in, out);
    const int ksize = g.ksize;
    std::vector<double> row((size_t)ksize);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * g.scale;
        double ww = 0.0;
        const double ss = 1.0 / g.filterscale;
        int xmin = (int)(center - g.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + g.support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        int x;
        for (x = 0; x < xmax; x++) {
            const double v = bicubic((x + xmin - center + 0.5) * ss);
            row[x] = v;
            ww += v;
        }
        for (x = 0; x < xmax; x++)
            if (ww != 0.0) row[x] /= ww;
        for (; x < ksize; x++) row[x] = 0;
        int32_t* k = kk + (size_t)xx * ksize;
        for (x = 0; x < ksize; x++)
            k[x] = row[x] < 0 ? (int)(-0.5 + row[x] * (1 << ING_PRECISION)) : (int)(0.5 + row[x] * (1 << ING_PRECISION));
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return 0;
}

int egs_frame_ingest(int height, int width, int flags, int n_frames, int frame, int plane, uint8_t* img, uint32_t* bits,
                     const uint8_t* src, int src_h, int src_w, int src_c, const int32_t* kk_h, const int32_t* bounds_h,
                     const int32_t* kk_v, const int32_t* bounds_v, void* stream) {
    if (height < 1 || width < 1 || n_frames < 1 || src_h < 1 || src_w < 1 || frame < 0 || frame >= n_frames) return EGS_ERR_ARG;
    if (plane != EGS_INGEST_IMAGE && plane != EGS_INGEST_HAND_MASK && plane != EGS_INGEST_OBJ_MASK) return EGS_ERR_ARG;
    egs_frame_layout L;
    const int rc = egs_frame_store_layout(height, width, flags, &L);
    if (rc) return rc;
    if (plane == EGS_INGEST_IMAGE ? src_c != 3 : (src_c != 1 && src_c != 3)) return EGS_ERR_ARG;
    const bool has_obj = L.obj_mask_begin >= 0, has_gate = L.gate_begin >= 0;
    if ((plane == EGS_INGEST_IMAGE && !L.image_floats) || (plane == EGS_INGEST_HAND_MASK && !has_gate) || (plane == EGS_INGEST_OBJ_MASK && !has_obj))
        return EGS_ERR_MODE;
    if (height > ING_MAX_SIDE || width > ING_MAX_SIDE || src_h > ING_MAX_SIDE || src_w > ING_MAX_SIDE) return EGS_ERR_RANGE;
    if ((long long)src_w > (long long)ING_MAX_SCALE * width || (long long)src_h > (long long)ING_MAX_SCALE * height) return EGS_ERR_RANGE;
    const bool pass_h = src_w != width, pass_v = src_h != height;
    const bool premul = plane == EGS_INGEST_IMAGE && (flags & EGS_FRAME_OBJECT_LOSS);
    if (!src || (plane == EGS_INGEST_IMAGE ? !img : !bits) || (premul && !bits)) return EGS_ERR_ARG;
    if ((pass_h && (!kk_h || !bounds_h)) || (pass_v && (!kk_v || !bounds_v))) return EGS_ERR_ARG;

    IngestArgs a = {};
    a.H = height; a.W = width; a.h = src_h; a.w = src_w; a.plane = plane; a.premul = premul ? 1 : 0;
    a.ks_h = pass_h ? axis_geometry(src_w, width).ksize : 0;
    a.rows_cap = ING_TH;
    if (pass_v) {
        // rows between the first tap of a tile's first output row and the last tap of its last: <= (TH - 1) scale + 2 support + 1
        const AxisGeometry g = axis_geometry(src_h, height);
        a.ks_v = g.ksize;
        a.rows_cap = (int)floor((ING_TH - 1) * g.scale + 2.0 * g.support) + 2;
        if (a.rows_cap > src_h) a.rows_cap = src_h;
    }
    const size_t lds = (size_t)(ING_TW * a.ks_h + ING_TH * a.ks_v + 2 * (ING_TW + ING_TH)) * 4 + (size_t)a.rows_cap * (size_t)src_c * ING_TW;
    if (lds > 65536) return EGS_ERR_RANGE;                                     // (41 KB at scale 8: not reached inside the range above)
    const int obj_index = has_gate ? 1 : 0;                                   // planes: gate first, then obj_mask
    const size_t frame_words = (size_t)frame * (size_t)L.n_planes * (size_t)L.plane_words;
    uint8_t* img_row = img ? img + (size_t)frame * (size_t)L.image_stride : nullptr;
    uint32_t* plane_out = nullptr;
    const uint32_t* obj_plane = premul ? bits + frame_words + (size_t)obj_index * (size_t)L.plane_words : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (plane != EGS_INGEST_IMAGE) {
        plane_out = bits + frame_words + (size_t)(plane == EGS_INGEST_OBJ_MASK ? obj_index : 0) * (size_t)L.plane_words;
        const hipError_t e = hipMemsetAsync(plane_out, 0, (size_t)L.plane_words * 4, st);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)((width + ING_TW - 1) / ING_TW), (unsigned)((height + ING_TH - 1) / ING_TH));
    if (src_c == 3)
        hipLaunchKernelGGL(k_frame_ingest<3>, grid, dim3(ING_WG), lds, st, a, src, kk_h, bounds_h, kk_v, bounds_v, img_row, plane_out, obj_plane);
    else
        hipLaunchKernelGGL(k_frame_ingest<1>, grid, dim3(ING_WG), lds, st, a, src, kk_h, bounds_h, kk_v, bounds_v, img_row, plane_out, obj_plane);
    return (int)hipGetLastError();
}

}  // extern "C"
