// masks.hip -- the mask hand-off between the static stage and the background stage (include/egs_raster.h egs_label_mask,
// egs_interaction_gate).  Both are integer-exact: a mask byte, a count and a gate value have one right answer.
//
// k_label_mask: the predicted object mask of one label render and its counts against the dataset's mask
//     x = egs_label_logit(c0, c1, c2)      set = x > threshold (strict: NaN is not set)      mask8 = set ? 255 : 0   (every pixel, gated or not)
//     kept = keep >= 0.5 (NULL: all)       tgt = target >= 0.5 (NULL: none)
//     predicted = #(kept & set)   target = #(kept & tgt)   intersection = #(kept & set & tgt)   kept = #kept
//   Mapping: a workgroup of 256 lanes owns 1024 consecutive pixels.  When every address allows it (VEC: all pointers 16-byte aligned -- the
//   byte mask 4 -- and H*W a multiple of 4, which also puts planes 1 and 2 on 16-byte boundaries) a lane takes four consecutive pixels: five
//   16-byte loads, one 4-byte store.  Otherwise lane t takes pixels t, t + 256, t + 512, t + 768 of the workgroup's run with 4-byte loads and
//   byte stores (consecutive lanes, consecutive addresses).  The same workgroup owns the same pixels either way, so the partials are the
//   same.  One uint32[4] partial per workgroup; k_mask_finish (one wave) adds them in a fixed order as int64 and writes the row at the
//   device-side cursor, as k_eval_finish.  Bytes at 540x960 with target and keep: 10.4 MB read, 0.5 MB written.
//
// k_interaction_gate: gate = 1 - dilate_k(a != 0 | b != 0), the window clipped to the image.
//   Mapping: a wave owns 64 columns x `rows` output rows and walks down the rows; lane L is column x0 + L.  A row's set bits are ONE 64-bit
//   ballot; a second, half-empty load brings the 16 columns on either side (lanes 0-15 left, 16-31 right; k <= 31 needs 15), whose ballot
//   completes a 96-bit word that lives in scalar registers.  The horizontal dilation by r = k / 2 is a few shift-and-OR steps on that word
//   (steps 1, 2, 4, ... : an interval of radius p grows to p + s under {-s, 0, +s} while s <= 2p + 1), wave-uniform, no per-pixel window.
//   The vertical one needs no window either: a lane keeps the LAST input row at which its bit of the dilated word was set; output row
//   y - r is gated when that row lies within the k rows ending at y.  So: no LDS, no barrier, O(1) work per row whatever k is, and the
//   waves are independent (keeping k row words and ORing them would do the same; the last-set row replaces them by one register).
//   Loads go out eight rows at a time before the first is used.  A wave reads rows + 2r rows for `rows` outputs; egs_interaction_gate
//   picks rows (4 .. 22, by k) so that rows + 2r is a whole number of batches.  Output: one 4-byte store per lane and row (the gate may be a 4-byte-aligned view into a packed frame).
#include "egs_common.h"
#include "label_bce.h"

#define MASK_WG 256
#define MASK_PPW 1024               // pixels per workgroup
#define GATE_WPB 4                  // waves per workgroup (independent)
#define GATE_HALO 16                // columns fetched on either side of a wave's 64
#define GATE_BATCH 8                // input rows whose loads are in flight together

namespace {

struct MaskCount { unsigned pred, tgt, inter, kept; };

__device__ __forceinline__ unsigned mask_pixel(float c0, float c1, float c2, float threshold, bool tgt, bool kept, MaskCount& c) {
    const bool set = egs_label_logit(c0, c1, c2) > threshold;
    c.pred += (kept && set) ? 1u : 0u; c.tgt += (kept && tgt) ? 1u : 0u; c.inter += (kept && set && tgt) ? 1u : 0u; c.kept += kept ? 1u : 0u;
    return set ? 255u : 0u;
}

// grid: ceil(H W / 1024)
template <bool VEC>
__global__ __launch_bounds__(MASK_WG) void k_label_mask(unsigned n_pix, const float* __restrict__ img, float threshold, const float* __restrict__ target,
                                                        const float* __restrict__ keep, uint4* __restrict__ partial, uint8_t* __restrict__ mask8) {
    __shared__ MaskCount wave_sum[MASK_WG / 64];
    const unsigned t = threadIdx.x, base = blockIdx.x * MASK_PPW;
    const float* __restrict__ p0 = img; const float* __restrict__ p1 = img + n_pix; const float* __restrict__ p2 = img + 2 * (size_t)n_pix;
    MaskCount c = {0u, 0u, 0u, 0u};
    if (VEC) {
        const unsigned i = base + 4 * t;                                  // n_pix % 4 == 0: a quad is inside or outside as a whole
        if (i < n_pix) {
            const float4 a0 = *reinterpret_cast<const float4*>(p0 + i), a1 = *reinterpret_cast<const float4*>(p1 + i),
                         a2 = *reinterpret_cast<const float4*>(p2 + i);
            const float4 tg = target ? *reinterpret_cast<const float4*>(target + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 kp = keep ? *reinterpret_cast<const float4*>(keep + i) : make_float4(1.f, 1.f, 1.f, 1.f);
            unsigned m = mask_pixel(a0.x, a1.x, a2.x, threshold, tg.x >= 0.5f, kp.x >= 0.5f, c);
            m |= mask_pixel(a0.y, a1.y, a2.y, threshold, tg.y >= 0.5f, kp.y >= 0.5f, c) << 8;
            m |= mask_pixel(a0.z, a1.z, a2.z, threshold, tg.z >= 0.5f, kp.z >= 0.5f, c) << 16;
            m |= mask_pixel(a0.w, a1.w, a2.w, threshold, tg.w >= 0.5f, kp.w >= 0.5f, c) << 24;
            if (mask8) *reinterpret_cast<uint32_t*>(mask8 + i) = m;
        }
    } else {
        float a0[4], a1[4], a2[4], tg[4], kp[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {                                     // the index is clamped and the pixel counted only when inside
            const unsigned i = min(base + (unsigned)j * MASK_WG + t, n_pix - 1u);
            a0[j] = p0[i]; a1[j] = p1[i]; a2[j] = p2[i];
            tg[j] = target ? target[i] : 0.f; kp[j] = keep ? keep[i] : 1.f;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned i = base + (unsigned)j * MASK_WG + t;
            if (i < n_pix) {
                const unsigned m = mask_pixel(a0[j], a1[j], a2[j], threshold, tg[j] >= 0.5f, kp[j] >= 0.5f, c);
                if (mask8) mask8[i] = (uint8_t)m;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c.pred += (unsigned)__shfl_xor((int)c.pred, d, 64); c.tgt += (unsigned)__shfl_xor((int)c.tgt, d, 64);
        c.inter += (unsigned)__shfl_xor((int)c.inter, d, 64); c.kept += (unsigned)__shfl_xor((int)c.kept, d, 64);
    }
    if ((t & 63u) == 0u) wave_sum[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        uint4 s = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int w = 0; w < MASK_WG / 64; w++) { s.x += wave_sum[w].pred; s.y += wave_sum[w].tgt; s.z += wave_sum[w].inter; s.w += wave_sum[w].kept; }
        partial[blockIdx.x] = s;
    }
}

// One wave, fixed order (k_eval_finish's form): lane l adds partials l, l + 64, ... as int64, a butterfly folds the lanes, lane 0 writes the row
// the device-side cursor names and advances the cursor.
__global__ __launch_bounds__(64) void k_mask_finish(unsigned n, const uint4* __restrict__ partial, const uint32_t* __restrict__ overflow,
                                                    egs_mask_row* __restrict__ rows, int capacity, int32_t* __restrict__ cursor) {
    const unsigned lane = threadIdx.x;
    long long s[4] = {0, 0, 0, 0};
    for (unsigned i0 = 0; i0 < n; i0 += 64 * 8) {                           // eight loads in flight per lane; clamped index, selected after the load
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = partial[min(i0 + (unsigned)k * 64 + lane, n - 1u)];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool in = i0 + (unsigned)k * 64 + lane < n;
            s[0] += in ? (long long)v[k].x : 0ll; s[1] += in ? (long long)v[k].y : 0ll;
            s[2] += in ? (long long)v[k].z : 0ll; s[3] += in ? (long long)v[k].w : 0ll;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] += __shfl_xor(s[k], d, 64);
    }
    if (lane == 0) {
        const int32_t at = cursor[0];
        if (at >= 0 && at < capacity) {
            egs_mask_row r;
            r.predicted = s[0]; r.target = s[1]; r.intersection = s[2]; r.kept = s[3];
            r.clipped = overflow ? (int64_t)overflow[0] : 0; r.instances = overflow ? (int64_t)overflow[1] : 0;
            rows[at] = r;
        }
        cursor[0] = at + 1;                 // also past a full array: the host sees the overrun
    }
}

// grid: ceil(blocks_x * strips / GATE_WPB); a wave = 64 columns x `rows` output rows.  r = k / 2 <= 15.
template <bool TWO>
__global__ __launch_bounds__(64 * GATE_WPB) void k_interaction_gate(int H, int W, int blocks_x, int strips, int rows, int r,
                                                                     const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ gate) {
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * GATE_WPB + (threadIdx.x >> 6)));
    if (wave >= blocks_x * strips) return;                               // wave-uniform
    const int x0 = (wave % blocks_x) * 64, y0 = (wave / blocks_x) * rows, y_end = min(y0 + rows, H);
    const int cx = x0 + (int)lane;                                        // this lane's own column
    const bool cx_ok = cx < W;
    // the side columns: lanes 0-15 are x0 - 16 .. x0 - 1, lanes 16-31 are x0 + 64 .. x0 + 79, lanes 32-63 none
    const int hx = lane < GATE_HALO ? x0 - GATE_HALO + (int)lane : x0 + 48 + (int)lane;
    const bool hx_ok = lane < 2 * GATE_HALO && hx >= 0 && hx < W;
    const unsigned cxc = (unsigned)min(cx, W - 1), hxc = (unsigned)min(max(hx, 0), W - 1);
    const int k = 2 * r + 1;
    int last = -(1 << 20);                                                // the last input row whose dilated word had this lane's bit
    // input rows y0 - r .. y_end - 1 + r; those outside the image hold nothing (the reference's zero padding) and rows above it are skipped
    const int y_first = max(y0 - r, 0), y_stop = y_end + r;
    // Two batches of rows are in flight: the loads of the next batch go out BEFORE the current one is worked on, so that they never queue
    // behind this batch's stores (loads and stores share one in-order counter here: a batch issued after its predecessor's stores waits
    // for them as well).  Addresses are clamped into the wave's own rows and the image; what lies outside is dropped at the ballot.
    const int y_last = min(y_stop, H) - 1;
    float ca[GATE_BATCH], cb[GATE_BATCH], ha[GATE_BATCH], hb[GATE_BATCH], na[GATE_BATCH], nb[GATE_BATCH], nha[GATE_BATCH], nhb[GATE_BATCH];
#define GATE_LOAD(A, B, HA, HB, Y0)                                                                          \
    _Pragma("unroll") for (int j = 0; j < GATE_BATCH; j++) {                                                 \
        const unsigned ro = (unsigned)min((Y0) + j, y_last) * (unsigned)W;                                   \
        A[j] = a[ro + cxc]; B[j] = TWO ? b[ro + cxc] : 0.f;                                                  \
        HA[j] = r ? a[ro + hxc] : 0.f; HB[j] = (TWO && r) ? b[ro + hxc] : 0.f;                               \
    }
    GATE_LOAD(ca, cb, ha, hb, y_first)
    for (int yb = y_first; yb < y_stop; yb += GATE_BATCH) {
        if (yb + GATE_BATCH < y_stop) { GATE_LOAD(na, nb, nha, nhb, yb + GATE_BATCH) }                  // (wave-uniform: a whole batch or none)
#pragma unroll
        for (int j = 0; j < GATE_BATCH; j++) {
            const int y = yb + j;
            if (y >= y_stop) break;                                       // wave-uniform
            const bool in = y < H;
            const unsigned long long own = __ballot(in && cx_ok && (ca[j] != 0.f || cb[j] != 0.f));       // NaN != 0: set, as logical_or
            const unsigned long long side = __ballot(in && hx_ok && (ha[j] != 0.f || hb[j] != 0.f));
            // bit j of (hi:lo) is column x0 - 16 + j, j = 0 .. 95
            unsigned long long lo = (own << GATE_HALO) | (side & 0xffffull), hi = (own >> (64 - GATE_HALO)) | (((side >> GATE_HALO) & 0xffffull) << GATE_HALO);
            for (int p = 0; p < r;) {                                     // p: the radius reached
                const int s = min(p + 1, r - p);                          // 1 <= s <= 8
                const unsigned long long l_lo = lo << s, l_hi = (hi << s) | (lo >> (64 - s)), r_lo = (lo >> s) | (hi << (64 - s)), r_hi = hi >> s;
                lo |= l_lo | r_lo; hi |= l_hi | r_hi;
                p += s;
            }
            const unsigned long long word = (lo >> GATE_HALO) | (hi << (64 - GATE_HALO));
            if ((word >> lane) & 1ull) last = y;
            const int yo = y - r;
            if (yo >= y0 && cx_ok) gate[(unsigned)yo * (unsigned)W + (unsigned)cx] = last > y - k ? 0.f : 1.f;     // (yo < y_end: y < y_stop)
        }
#pragma unroll
        for (int j = 0; j < GATE_BATCH; j++) { ca[j] = na[j]; cb[j] = nb[j]; ha[j] = nha[j]; hb[j] = nhb[j]; }
    }
#undef GATE_LOAD
}

inline bool aligned_to(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" {

size_t egs_label_mask_partial_bytes(int height, int width) {
    if (height <= 0 || width <= 0) return 0;
    return (((size_t)height * (size_t)width + MASK_PPW - 1) / MASK_PPW) * sizeof(uint4);
}

int egs_label_mask(int height, int width, const float* img, float threshold, const float* target, const float* keep, const uint32_t* overflow,
                   void* partial, uint8_t* mask8, void* rows, int capacity, int32_t* cursor, void* stream) {
    if (height < 1 || width < 1 || capacity < 0) return EGS_ERR_ARG;
    if (!img || !partial || !rows || !cursor) return EGS_ERR_ARG;
    if ((size_t)height * (size_t)width >= ((size_t)1 << 31)) return EGS_ERR_RANGE;            // 32-bit indices within a plane
    const unsigned n_pix = (unsigned)height * (unsigned)width, wgs = (n_pix + MASK_PPW - 1) / MASK_PPW;
    const bool vec = n_pix % 4 == 0 && aligned_to(img, 16) && aligned_to(target, 16) && aligned_to(keep, 16) && aligned_to(mask8, 4);
    if (vec) hipLaunchKernelGGL((k_label_mask<true>), dim3(wgs), dim3(MASK_WG), 0, (hipStream_t)stream, n_pix, img, threshold, target, keep, (uint4*)partial, mask8);
    else hipLaunchKernelGGL((k_label_mask<false>), dim3(wgs), dim3(MASK_WG), 0, (hipStream_t)stream, n_pix, img, threshold, target, keep, (uint4*)partial, mask8);
    hipLaunchKernelGGL(k_mask_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, wgs, (const uint4*)partial, overflow, (egs_mask_row*)rows, capacity, cursor);
    return (int)hipGetLastError();
}

int egs_interaction_gate(int height, int width, const float* a, const float* b, int k, float* gate, void* stream) {
    if (height < 1 || width < 1 || !gate || (!a && !b)) return EGS_ERR_ARG;
    if (k < 1 || k > 31 || (k & 1) == 0) return EGS_ERR_ARG;
    if ((size_t)height * (size_t)width >= ((size_t)1 << 31)) return EGS_ERR_RANGE;
    // rows per wave: what makes rows + 2r, the rows a wave walks, a whole number of batches (1, 2, 3 or 5 of them): the walk is a chain of
    // dependent batches, and the rows beyond a wave's own are served by the L2 (at most four times the image at k = 31)
    const int r = k / 2, blocks_x = (width + 63) / 64;
    const int rows = (r <= 2 ? 1 : r <= 4 ? 2 : r <= 8 ? 3 : 5) * GATE_BATCH - 2 * r;
    const int strips = (height + rows - 1) / rows;
    if ((size_t)blocks_x * (size_t)strips >= ((size_t)1 << 31)) return EGS_ERR_RANGE;
    const unsigned wgs = (unsigned)((blocks_x * strips + GATE_WPB - 1) / GATE_WPB);
    const float* first = a ? a : b;
    if (a && b) hipLaunchKernelGGL((k_interaction_gate<true>), dim3(wgs), dim3(64 * GATE_WPB), 0, (hipStream_t)stream, height, width, blocks_x, strips, rows, r, a, b, gate);
    else hipLaunchKernelGGL((k_interaction_gate<false>), dim3(wgs), dim3(64 * GATE_WPB), 0, (hipStream_t)stream, height, width, blocks_x, strips, rows, r, first, first, gate);
    return (int)hipGetLastError();
}

}  // extern "C"
