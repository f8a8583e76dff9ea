// eval_metrics.hip -- the evaluation pass's figures of one frame (include/egs_raster.h egs_eval_metrics): the squared 8-bit error and the SSIM
// sum of the QUANTISED, hand-masked render against the quantised, hand-masked ground truth -- what the reference's eval_and_metric measures
// after its round trip through 8-bit PNG files (trainers/eval_metric.py:41-175):
//     q(v) = uint8(clamp(v * 255 + 0.5, 0, 255))          float32, one multiply, one add, truncation; NaN -> 0
//     kept = keep >= 0.5                                   keep = 1 - hand mask, [H,W]; NULL: every pixel kept
//     u = kept ? q(x) / 255 : 0     v = kept ? q(y) / 255 : 0
//     sse      = sum over kept pixels and channels of (q(x) - q(y))^2            an exact integer
//     ssim_sum = sum over all C H W entries of SSIM_map(u, v)                    11x11 window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2
// No gradients: nothing is stored per pixel but (optionally) the two quantised images as planar bytes, which is what a caller writes to PNG.
//
// Mapping: loss.hip's strips (k_l1_ssim_forward).  A wave owns SW = 54 output columns x SR = 15 output rows of ONE channel plane; lane L is
// image column strip_x0 - 5 + L and walks down the rows; the vertical 11-tap blur runs in a register window rotated by full unrolling, the
// horizontal one through a wave-private LDS row; no workgroup barriers; workgroups are dealt to the XCDs in contiguous runs
// (eval_logical_block = loss.hip's loss_logical_block).  Values are quantised and masked when they enter the window.  A strip row of `keep` is
// loaded once per wave and row: a wave holds one channel (three channels' windows are 3 x 44 registers), so the three waves of a strip
// position each read it -- from the same XCD's L2 when the planes' runs meet, else from HBM: HW * 4 of 3HW * 8 + HW * 4 bytes per frame.
// Per lane: the SSIM map values in float32 (at most 15), the squared byte differences in uint32 (15 x 255^2 < 2^20); per strip one
// {float ssim_sum; uint32 sse} partial; a one-wave launch of its own (k_eval_finish) adds the partials in a fixed order -- int64 and float64 --
// and writes the frame's row.  Bytes at 3x540x960: 12.4 MB + 2.1 MB read, 3.1 MB written with both byte images; k_l1_ssim_forward writes 37 MB.
#include "egs_common.h"
#include "loss_window.h"

#define HALO 5
#define SW 54                 // useful columns per wave (64 lanes - 2 * HALO)
#define SR 15                 // output rows per wave
#define WPB 2                 // waves per workgroup (independent)

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f pk_fma(float w, v2f a, v2f c) { return __builtin_elementwise_fma((v2f)(w), a, c); }

// (loss.hip hblur_issue / hblur_collect / vblur: the same operations in the same order)
__device__ __forceinline__ void hblur_issue(v2f v, v2f* row /* [80], lane L at [8 + L] */, unsigned lane) { row[8 + lane] = v; }
__device__ __forceinline__ v2f hblur_collect(const v2f* row, unsigned lane) {
    v2f r[11];
#pragma unroll
    for (int k = 0; k < 11; k++) r[k] = row[3 + lane + k];                     // r[k] = v[lane - 5 + k]
    v2f acc = (v2f)(kwin(0)) * (r[0] + r[10]);
    acc = pk_fma(kwin(1), r[1] + r[9], acc); acc = pk_fma(kwin(2), r[2] + r[8], acc);
    acc = pk_fma(kwin(3), r[3] + r[7], acc); acc = pk_fma(kwin(4), r[4] + r[6], acc);
    return pk_fma(kwin(5), r[5], acc);
}
template <int NEWEST>
__device__ __forceinline__ v2f vblur(const v2f (&w)[11]) {
    v2f acc = (v2f)(0.f);
#pragma unroll
    for (int k = 0; k < 11; k++) acc = pk_fma(kwin(k), w[(NEWEST + 1 + k) % 11], acc);
    return acc;
}

// q(v) of both images as a float pair: the float32 statement of torchvision's save_image conversion -- one multiply, one add (never fused:
// -ffp-contract=off), clamp, truncation.  fmaxf(NaN, 0) = 0: NaN quantises to 0.  The pair holds the integers 0..255 exactly.
__device__ __forceinline__ v2f quant8_pair(float x, float y) {
    const v2f t = v2f{x, y} * (v2f)(255.f) + (v2f)(0.5f);
    return v2f{truncf(fminf(fmaxf(t.x, 0.f), 255.f)), truncf(fminf(fmaxf(t.y, 0.f), 255.f))};
}
// q / 255 correctly rounded for q = 0..255 without the division sequence: one refinement of q * RN(1/255) by the exact residual
__device__ __forceinline__ v2f unit8_pair(v2f q) {
    const float c = 1.f / 255.f;
    const v2f r = q * (v2f)(c);
    return pk_fma(c, pk_fma(-255.f, r, q), r);
}

struct EvalCtx {
    int H, W, gx, y_first, y_end; bool col_ok, col_out; unsigned lane;
    uint8_t* q_img; uint8_t* q_gt;          // this wave's plane, or NULL
    v2f* rows;                              // [2][80] pairs
    float sm; unsigned sse;
};

// One input row enters (slot NEWEST); if 11 rows are in, the output row 5 above it leaves.
template <int NEWEST, bool MASKED, bool OUT8>
__device__ __forceinline__ void eval_step(EvalCtx& c, v2f (&w01)[11], v2f (&w23)[11], int y_in, float x, float y, float keep) {
    const bool inside = c.col_ok && y_in >= 0 && y_in < c.H;             // outside the image: the window's zero padding (the loads were clamped)
    const bool kept = inside && (!MASKED || keep >= 0.5f);
    const v2f q = quant8_pair(x, y), r = unit8_pair(q);
    // (selects, not a multiply by a 0 / 1 pair: a packed operand names a register PAIR, and the partner of `keep` is a load still in flight)
    const float u = kept ? r.x : 0.f, v = kept ? r.y : 0.f;
    if (y_in >= c.y_first && y_in < c.y_end) {                           // (wave-uniform) one of the strip's own rows: its lanes own these pixels
        if (c.col_out) {                                                 // halo lanes never store, never count
            const float d = q.x - q.y;                                   // exact: integers below 2^8, their square below 2^16
            c.sse += kept ? (unsigned)(d * d) : 0u;
            if (OUT8) {
                const unsigned p = (unsigned)y_in * (unsigned)c.W + (unsigned)c.gx;
                if (c.q_img) c.q_img[p] = (uint8_t)(unsigned)q.x;        // (the quantised images are NOT masked: the reference writes them whole)
                if (c.q_gt) c.q_gt[p] = (uint8_t)(unsigned)q.y;
            }
        }
    }
    w01[NEWEST] = v2f{u, v}; w23[NEWEST] = v2f{fmaf(u, u, v * v), u * v};
    const int y_out = y_in - HALO;
    if (y_out < c.y_first || y_out >= c.y_end) return;                   // wave-uniform
    const v2f vb01 = vblur<NEWEST>(w01), vb23 = vblur<NEWEST>(w23);
    hblur_issue(vb01, c.rows, c.lane); hblur_issue(vb23, c.rows + 80, c.lane);
    __builtin_amdgcn_wave_barrier();
    const v2f hb01 = hblur_collect(c.rows, c.lane), hb23 = hblur_collect(c.rows + 80, c.lane);
    __builtin_amdgcn_wave_barrier();
    if (c.col_out) {
        const float mu1 = hb01.x, mu2 = hb01.y, exx_eyy = hb23.x, exy = hb23.y;
        const float C1 = 0.0001f, C2 = 0.0009f;
        const float s12 = exy - mu1 * mu2;
        const float A = 2.f * mu1 * mu2 + C1, B = 2.f * s12 + C2, D = mu1 * mu1 + mu2 * mu2 + C1, E = (exx_eyy - (D - C1)) + C2;
        // 1 / (D E) as v_rcp_f32 + one Newton step, as k_l1_ssim_forward
        const float de_ = D * E; float invDE = __builtin_amdgcn_rcpf(de_); invDE = fmaf(fmaf(-de_, invDE, 1.f), invDE, invDE);
        c.sm += A * B * invDE;
    }
}

// loss.hip loss_logical_block: workgroup b runs on XCD b % 8; logical index (b % 8) * per + b / 8 gives each XCD one contiguous run of strips
__device__ __forceinline__ unsigned eval_logical_block(unsigned b, unsigned main) {
    const unsigned per = (main + 7u) / 8u;
    return (b & 7u) * per + (b >> 3);
}

struct EvalPartial { float ssim_sum; unsigned sse; };

// grid: 8 * ceil(C * ceil(strips_x * strips_y / WPB) / 8) (1-D); a wave = one strip of one plane
// MASKED: `keep` is given; OUT8: at least one byte image is.  Compile-time, so that the row loads sit in straight-line code: with a branch
// around the `keep` load or the byte stores the compiler counts outstanding loads conservatively and waits for rows it does not need yet
// (with those branches and the mask applied as a packed 0 / 1 multiply the call took 25.0 us at 3x540x960, in this form 23.2 us -- both before
// the finishing launch was repaired, see k_eval_finish).
template <bool MASKED, bool OUT8>
__global__ __launch_bounds__(64 * WPB) void k_eval_metrics(int H, int W, int strips_x, int strips_y, const float* __restrict__ img,
                                                            const float* __restrict__ gt, const float* __restrict__ keep,
                                                            EvalPartial* __restrict__ partial, uint8_t* __restrict__ q_img,
                                                            uint8_t* __restrict__ q_gt, unsigned per_plane, unsigned main_wgs) {
    __shared__ v2f lds[WPB][2 * 80];
    const unsigned lane = threadIdx.x & 63, wv = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rel = eval_logical_block(blockIdx.x, main_wgs);
    if (rel >= main_wgs) return;
    const unsigned plane_z = rel / per_plane;
    const int strip = (int)(rel - plane_z * per_plane) * WPB + (int)wv;
    if (strip >= strips_x * strips_y) return;
    for (int k = lane; k < 2 * 80; k += 64) lds[wv][k] = (v2f)(0.f);   // the padding words stay zero
    __builtin_amdgcn_wave_barrier();
    const size_t plane = (size_t)plane_z * H * W;
    EvalCtx c;
    c.H = H; c.W = W; c.lane = lane; c.rows = lds[wv]; c.sm = 0.f; c.sse = 0u;
    c.q_img = (OUT8 && q_img) ? q_img + plane : nullptr; c.q_gt = (OUT8 && q_gt) ? q_gt + plane : nullptr;
    const int sx = strip % strips_x, sy = strip / strips_x;
    c.gx = sx * SW - HALO + (int)lane;
    c.col_ok = c.gx >= 0 && c.gx < W;
    c.col_out = c.col_ok && lane >= HALO && lane < HALO + SW;
    c.y_first = sy * SR; c.y_end = min(c.y_first + SR, H);
    v2f w01[11], w23[11];
#pragma unroll
    for (int k = 0; k < 11; k++) { w01[k] = (v2f)(0.f); w23[k] = (v2f)(0.f); }
    // as k_l1_ssim_forward: eleven rows per trip, one buffer refilled in place, every load eleven row-steps ahead of its use; a row's address
    // is a wave-uniform base plus the lane's column, both clamped into the image (what lies outside is zeroed when it enters the window)
    const unsigned col = (unsigned)min(max(c.gx, 0), W - 1);
    const float* __restrict__ img_p = img + plane; const float* __restrict__ gt_p = gt + plane;
    auto load_row = [&](int y, float& a, float& b, float& k) {
        const unsigned ro = (unsigned)min(max(y, 0), H - 1) * (unsigned)W;   // (one plane has fewer than 2^31 elements: egs_eval_metrics checks)
        a = img_p[ro + col]; b = gt_p[ro + col];
        k = MASKED ? keep[ro + col] : 1.f;
    };
    float cx[11], cy[11], ck[11];
#pragma unroll
    for (int k = 0; k < 11; k++) load_row(c.y_first - HALO + k, cx[k], cy[k], ck[k]);
    for (int y0 = c.y_first - HALO; y0 < c.y_end + HALO; y0 += 11) {
#define ESTEP(K) eval_step<K, MASKED, OUT8>(c, w01, w23, y0 + K, cx[K], cy[K], ck[K]); load_row(y0 + 11 + K, cx[K], cy[K], ck[K])
        ESTEP(0); ESTEP(1); ESTEP(2); ESTEP(3); ESTEP(4); ESTEP(5); ESTEP(6); ESTEP(7); ESTEP(8); ESTEP(9); ESTEP(10);
#undef ESTEP
    }
    float sm = c.sm; unsigned sse = c.sse;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sm += __shfl_xor(sm, d, 64); sse += (unsigned)__shfl_xor((int)sse, d, 64); }
    if (lane == 0) {
        EvalPartial p; p.ssim_sum = sm; p.sse = sse;
        partial[(size_t)plane_z * strips_x * strips_y + strip] = p;
    }
}

// One wave, fixed order: lane l adds partials l, l + 64, ... (int64 / float64; n >= 1), the lanes are folded by a butterfly; lane 0 writes the row the
// device-side cursor names and advances the cursor -- a captured launch cannot carry a frame index in its arguments.
__global__ __launch_bounds__(64) void k_eval_finish(unsigned n, const EvalPartial* __restrict__ partial, const uint32_t* __restrict__ overflow,
                                                    egs_eval_row* __restrict__ rows, int capacity, int32_t* __restrict__ cursor) {
    const unsigned lane = threadIdx.x;
    long long sse = 0; double sm = 0.0;
    const uint2* __restrict__ words = reinterpret_cast<const uint2*>(partial);      // {float bits, uint32}
    // sixteen loads in flight per lane.  The index is clamped and the value selected AFTER the load: with `i < n ? words[i] : 0` the compiler
    // branches around every load and waits for each before the next (dependent round trips: 6.6 us of a 23.2 us call at 3x540x960,
    // 1 944 partials; profiles/eval_pass.md).
    for (unsigned i0 = 0; i0 < n; i0 += 64 * 16) {
        uint2 v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = words[min(i0 + (unsigned)k * 64 + lane, n - 1u)];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const bool in = i0 + (unsigned)k * 64 + lane < n;
            sm += in ? (double)__uint_as_float(v[k].x) : 0.0; sse += in ? (long long)v[k].y : 0ll;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sse += __shfl_xor(sse, d, 64); sm += __shfl_xor(sm, d, 64); }
    if (lane == 0) {
        const int32_t at = cursor[0];
        if (at >= 0 && at < capacity) {
            egs_eval_row r;
            r.sse = sse; r.ssim_sum = sm;
            r.clipped = overflow ? (int64_t)overflow[0] : 0; r.instances = overflow ? (int64_t)overflow[1] : 0;
            rows[at] = r;
        }
        cursor[0] = at + 1;                 // also past a full array: the host sees the overrun
    }
}

}  // namespace

extern "C" {

size_t egs_eval_metrics_partial_bytes(int channels, int height, int width) {
    if (channels <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)channels * (size_t)((height + SR - 1) / SR) * (size_t)((width + SW - 1) / SW) * sizeof(EvalPartial);
}

int egs_eval_metrics(int channels, int height, int width, const float* img, const float* gt, const float* keep, const uint32_t* overflow,
                     void* partial, uint8_t* q_img, uint8_t* q_gt, void* rows, int capacity, int32_t* cursor, void* stream) {
    if ((channels != 1 && channels != 3) || height < 1 || width < 1 || capacity < 0) return EGS_ERR_ARG;
    if (!img || !gt || !partial || !rows || !cursor) return EGS_ERR_ARG;
    if ((size_t)height * (size_t)width >= ((size_t)1 << 31)) return EGS_ERR_RANGE;            // 32-bit indices within a plane
    const int strips_x = (width + SW - 1) / SW, strips_y = (height + SR - 1) / SR;
    if ((size_t)strips_x * (size_t)strips_y * (size_t)channels >= ((size_t)1 << 31)) return EGS_ERR_RANGE;
    const unsigned per_plane = (unsigned)((strips_x * strips_y + WPB - 1) / WPB), main_wgs = per_plane * (unsigned)channels;
    const unsigned main_pad = ((main_wgs + 7u) / 8u) * 8u;
#define EV_LAUNCH(M, O) hipLaunchKernelGGL((k_eval_metrics<M, O>), dim3(main_pad), dim3(64 * WPB), 0, (hipStream_t)stream, height, width, strips_x, strips_y, \
                                           img, gt, keep, (EvalPartial*)partial, q_img, q_gt, per_plane, main_wgs)
    const bool out8 = q_img || q_gt;
    if (keep && out8) EV_LAUNCH(true, true); else if (keep) EV_LAUNCH(true, false); else if (out8) EV_LAUNCH(false, true); else EV_LAUNCH(false, false);
#undef EV_LAUNCH
    hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned)(strips_x * strips_y * channels), (const EvalPartial*)partial,
                       overflow, (egs_eval_row*)rows, capacity, cursor);
    return (int)hipGetLastError();
}

}  // extern "C"
