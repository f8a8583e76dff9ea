// sh.hip -- the spherical-harmonics launches of a scene with egs_sh_apart() (egs_common.h), for gfx950: colour after k_preprocess,
// dL/dSH and the view-direction term of dL/dmean3D after k_preprocess_backward (preprocess.hip).  The basis is sh_basis.h's.
// Compiled with -ffp-contract=off like preprocess.hip, whose inline M = 1 path evaluates the same expressions.
#include "egs_common.h"
#include "object_motion.h"          // the rigid object motion of the positions (EGS_ACT_OBJECT_MOTION)
#include "sh_basis.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Spherical harmonics with more than one coefficient (or given as separate DC / rest arrays).  A Gaussian's row is 12 M
// bytes; one lane walking its own row touches a different cache line per load, and the M * 3 gradient stores of the backward
// are 4-byte writes 12 M bytes apart.  Here a wave owns 64 consecutive Gaussians and moves their rows as ONE contiguous block:
// float4 loads / stores in lane order (full lines), transposed through an LDS tile of 64 x (3 M + 1) words whose odd row
// stride makes the per-lane row accesses conflict-free.  Rows of invisible Gaussians and coefficients above the active degree
// are not loaded; their gradient is written as zeros by the same coalesced stores.
//   k_sh_forward   after k_preprocess: colour + clamp flags into the record it left open
//   k_sh_backward  after k_preprocess_backward: reads dL/dcolour, writes dL/dSH, adds the view-direction term to dL/dmean3D
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void sh_row_col(int e, int rw, float inv_rw, int& r, int& c) {
    r = (int)(((float)e + 0.5f) * inv_rw);                             // e < 64 * 48: exact
    c = e - r * rw;
}

// Rows [i0, i0 + nvalid) of a [P, rw] float array -> tile[row * ld + col0 + col]; elements of invisible rows or with col >= need are
// left alone (never read).
__device__ __forceinline__ void sh_load_rows(float* tile, int ld, int col0, const float* __restrict__ src, int rw, int i0, int nvalid,
                                             uint64_t vmask, int need, unsigned lane) {
    if (need <= 0) return;
    const float inv_rw = 1.f / (float)rw;
    const float* base = src + (size_t)i0 * rw;
    const int n = nvalid * rw;
    if ((((uintptr_t)base) & 15) == 0 && (n & 3) == 0 && rw <= 48) {
        // all (up to 12) loads of the lane are issued before the first one is used: one HBM round trip per wave, not twelve
        const float4* b4 = reinterpret_cast<const float4*>(base);
        float4 v[12]; bool want[12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int q = (int)lane + 64 * k;
            int r0, c0, r3, c3;
            sh_row_col(4 * q, rw, inv_rw, r0, c0); sh_row_col(4 * q + 3, rw, inv_rw, r3, c3);
            want[k] = 4 * q < n && ((((vmask >> r0) & 1) && c0 < need) || (r3 != r0 && ((vmask >> r3) & 1)) ||
                                    (r3 - r0 > 1 && ((vmask >> (r0 + 1)) & 1)));
            if (want[k]) v[k] = b4[q];
        }
#pragma unroll
        for (int k = 0; k < 12; k++) {
            if (!want[k]) continue;
            const int q = (int)lane + 64 * k;
            const float vv[4] = { v[k].x, v[k].y, v[k].z, v[k].w };
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int r, c; sh_row_col(4 * q + j, rw, inv_rw, r, c);
                tile[r * ld + col0 + c] = vv[j];
            }
        }
    } else {
        for (int e = lane; e < n; e += 64) {
            int r, c; sh_row_col(e, rw, inv_rw, r, c);
            if (((vmask >> r) & 1) && c < need) tile[r * ld + col0 + c] = base[e];
        }
    }
}

// tile[row * ld + col0 + col] -> rows [i0, i0 + nvalid) of a [P, rw] float array, every element.
__device__ __forceinline__ void sh_store_rows(const float* tile, int ld, int col0, float* __restrict__ dst, int rw, int i0, int nvalid,
                                              unsigned lane) {
    const float inv_rw = 1.f / (float)rw;
    float* base = dst + (size_t)i0 * rw;
    const int n = nvalid * rw;
    if ((((uintptr_t)base) & 15) == 0 && (n & 3) == 0) {
        float4* b4 = reinterpret_cast<float4*>(base);
        for (int q = lane; 4 * q < n; q += 64) {
            float vv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int r, c; sh_row_col(4 * q + j, rw, inv_rw, r, c);
                vv[j] = tile[r * ld + col0 + c];
            }
            b4[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
    } else {
        for (int e = lane; e < n; e += 64) {
            int r, c; sh_row_col(e, rw, inv_rw, r, c);
            base[e] = tile[r * ld + col0 + c];
        }
    }
}

extern __shared__ __attribute__((aligned(16))) float sh_tile[];

// sh_rest == nullptr: sh_a is [P, M, 3]; otherwise sh_a is the DC block [P, 1, 3] and sh_rest [P, M - 1, 3].
template <bool MOTION>
__global__ __launch_bounds__(64) void k_sh_forward(int P, int D, int M, const float* __restrict__ means3D, const float* __restrict__ campos,
                                                   const float* __restrict__ sh_a, const float* __restrict__ sh_rest,
                                                   const uint8_t* __restrict__ visible, float4* __restrict__ rec, uint8_t* __restrict__ clamped, EgsMotion mot) {
    const unsigned lane = threadIdx.x;
    const int i0 = blockIdx.x * 64, i = i0 + (int)lane;
    const bool vis = i < P && visible[i] != 0;
    const uint64_t vmask = __ballot(vis);
    if (!vmask) return;
    const int rw = 3 * M, ld = rw + 1, nvalid = min(64, P - i0), need = 3 * (D + 1) * (D + 1);
    if (sh_rest) {
        sh_load_rows(sh_tile, ld, 0, sh_a, 3, i0, nvalid, vmask, 3, lane);
        sh_load_rows(sh_tile, ld, 3, sh_rest, rw - 3, i0, nvalid, vmask, need - 3, lane);
    } else {
        sh_load_rows(sh_tile, ld, 0, sh_a, rw, i0, nvalid, vmask, need, lane);
    }
    __syncthreads();                                                   // one wave: orders the LDS writes before the row reads
    if (!vis) return;
    float p[3] = { means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2] };
    if constexpr (MOTION) {
        if (!mot.moved || mot.moved[i]) { const float p0[3] = { p[0], p[1], p[2] }; egs_motion_point(mot.A, p0, p); }   // (visible: a live row)
    }
    float x, y, z, inv; sh_view_dir(p, campos, x, y, z, inv);
    float rgb[3];
    const uint32_t cl = sh_colour(D, sh_tile + lane * ld, x, y, z, rgb);
    clamped[i] = (uint8_t)((clamped[i] & ~EGS_CLAMP_MASK) | cl);      // (bits 3-5: the HOT code k_preprocess left)
    float* r = reinterpret_cast<float*>(rec + (size_t)i * EGS_SPLAT_REC_F4);
    r[6] = rgb[0]; r[7] = rgb[1]; r[8] = rgb[2];
}

// MOTION (object_motion.h): the row is placed; the positions' gradient is complete here, so this launch chains it through the placement
// (dL/dp = A^T dL/dp') and writes the wave's line of the pose sums (one wave per workgroup: the six shuffle levels, no LDS).
template <bool MOTION>
__global__ __launch_bounds__(64) void k_sh_backward(int P, int D, int M, const float* __restrict__ means3D, const float* __restrict__ campos,
                                                    const float* __restrict__ sh_a, const float* __restrict__ sh_rest,
                                                    const int32_t* __restrict__ radii, const uint8_t* __restrict__ clamped,
                                                    const float* __restrict__ dcolors, float* __restrict__ dsh_a, float* __restrict__ dsh_rest,
                                                    float* __restrict__ dmeans3D, EgsMotion mot) {
    const unsigned lane = threadIdx.x;
    const int i0 = blockIdx.x * 64, i = i0 + (int)lane;
    const bool vis = i < P && radii[i] > 0;
    const uint64_t vmask = __ballot(vis);
    const int rw = 3 * M, ld = rw + 1, nvalid = min(64, P - i0), need = 3 * (D + 1) * (D + 1);
    float* row = sh_tile + lane * ld;
    if (vmask && D > 0) {                                              // the coefficients only enter through the view-direction term
        if (sh_rest) sh_load_rows(sh_tile, ld, 3, sh_rest, rw - 3, i0, nvalid, vmask, need - 3, lane);
        else sh_load_rows(sh_tile, ld, 0, sh_a, rw, i0, nvalid, vmask, need, lane);
        __syncthreads();
    }
    float red[MOTION ? EGS_MOTION_POSE_SUMS : 1];
    if constexpr (MOTION) {
#pragma unroll
        for (int k = 0; k < EGS_MOTION_POSE_SUMS; k++) red[k] = 0.f;
    }
    if (vis) {
        float p[3] = { means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2] };
        [[maybe_unused]] const float p0[3] = { p[0], p[1], p[2] };
        [[maybe_unused]] bool row_moved = false;
        if constexpr (MOTION) {
            row_moved = !mot.moved || mot.moved[i];
            if (row_moved) egs_motion_point(mot.A, p0, p);
        }
        float x, y, z, inv; sh_view_dir(p, campos, x, y, z, inv);
        const uint32_t cl = clamped[i] & EGS_CLAMP_MASK;
        float gdir[3] = { 0.f, 0.f, 0.f };
        for (int ch = 0; ch < 3; ch++) {
            const float g = ((cl >> ch) & 1u) ? 0.f : dcolors[3 * i + ch];
            sh_channel_backward(D, M, row, row, ch, x, y, z, g, gdir);     // the gradient in place, over the coefficients it has read
        }
        if (MOTION || D > 0) {                                         // what k_preprocess_backward wrote, finished
            float gm[3] = { dmeans3D[3 * i], dmeans3D[3 * i + 1], dmeans3D[3 * i + 2] };
            if (D > 0) sh_dir_to_pos(x, y, z, inv, gdir, gm);
            if constexpr (MOTION) {
                if (row_moved) {
                    if (mot.pose_partial) egs_motion_pose_terms(gm, p0, red);
                    const float gp[3] = { gm[0], gm[1], gm[2] };
                    egs_motion_point_backward(mot.A, gp, gm);
                }
            }
            dmeans3D[3 * i] = gm[0]; dmeans3D[3 * i + 1] = gm[1]; dmeans3D[3 * i + 2] = gm[2];
        }
    } else {
        for (int k = 0; k < rw; k++) row[k] = 0.f;
    }
    if constexpr (MOTION) {
        if (mot.pose_partial) egs_motion_wave_line<EGS_MOTION_POSE_SUMS>(red, mot.pose_partial + (size_t)blockIdx.x * EGS_MOTION_POSE_SUMS);
    }
    __syncthreads();
    if (dsh_rest) {
        sh_store_rows(sh_tile, ld, 0, dsh_a, 3, i0, nvalid, lane);
        sh_store_rows(sh_tile, ld, 3, dsh_rest, rw - 3, i0, nvalid, lane);
    } else {
        sh_store_rows(sh_tile, ld, 0, dsh_a, rw, i0, nvalid, lane);
    }
}

// ---- M = 16 (the reference's max_sh_degree = 3), 16-byte aligned arrays: the same two kernels with the index arithmetic of the
// transposition removed.
//   CAT   [P,16,3]: float4 q of the block goes to LDS slot q + q / 12, i.e. rows of 13 float4 -- an odd stride, so the twelve
//         ds_read_b128 / ds_write_b128 a lane does on its own row are conflict-free.
//   SPLIT [P,1,3] + [P,15,3]: both blocks are copied linearly; rows of 3 and 45 words are odd strides already (scalar row accesses).
// A lane keeps its row (48 coefficients, then 48 gradients) in registers.
#define SH16_CAT 1
#define SH16_SPLIT 2
#define SH16_REST_WORDS (64 * 45)

// gather this block's rows into LDS; `need` = words of a row's head that will be read (3 (D+1)^2)
template <int MODE>
__device__ __forceinline__ void sh16_stage_in(float* tile, const float* __restrict__ sh_a, const float* __restrict__ sh_rest, int i0, int nvalid,
                                              uint64_t vmask, int need, unsigned lane) {
    if (MODE == SH16_CAT) {
        const float4* b4 = reinterpret_cast<const float4*>(sh_a + (size_t)i0 * 48);
        float4* t4 = reinterpret_cast<float4*>(tile);
        // (twelve named registers, not an array: the compiler parks an array of conditionally loaded float4 in scratch, which
        // serialises the loads)
#define SH16_LD(k) float4 v##k = make_float4(0.f, 0.f, 0.f, 0.f); bool w##k;                                   \
        { const unsigned q = lane + 64u * k, row = q / 12u, j = q - row * 12u;                                 \
          w##k = (int)row < nvalid && ((vmask >> row) & 1) && (int)(4u * j) < need; if (w##k) v##k = b4[q]; }
#define SH16_PUT(k) { const unsigned q = lane + 64u * k; if (w##k) t4[q + q / 12u] = v##k; }
        SH16_LD(0) SH16_LD(1) SH16_LD(2) SH16_LD(3) SH16_LD(4) SH16_LD(5) SH16_LD(6) SH16_LD(7) SH16_LD(8) SH16_LD(9) SH16_LD(10) SH16_LD(11)
        SH16_PUT(0) SH16_PUT(1) SH16_PUT(2) SH16_PUT(3) SH16_PUT(4) SH16_PUT(5) SH16_PUT(6) SH16_PUT(7) SH16_PUT(8) SH16_PUT(9) SH16_PUT(10) SH16_PUT(11)
#undef SH16_LD
#undef SH16_PUT
    } else {
        float* tdc = tile + SH16_REST_WORDS;
        const int n_dc = nvalid * 3, n_rest = nvalid * 45, need_rest = need - 3;
        const float* bdc = sh_a + (size_t)i0 * 3;
        const float* brest = sh_rest + (size_t)i0 * 45;
        float4 vd = make_float4(0.f, 0.f, 0.f, 0.f); bool wd = false;
        {
            const int e = 4 * (int)lane;
            wd = e + 3 < n_dc && ((vmask >> (e / 3)) | (vmask >> ((e + 3) / 3))) & 1;
            if (wd) vd = reinterpret_cast<const float4*>(bdc)[lane];
        }
#define SH16_LD(k) float4 v##k = make_float4(0.f, 0.f, 0.f, 0.f); bool w##k;                                   \
        { const int e = 4 * ((int)lane + 64 * k), r0 = e / 45, r1 = (e + 3) / 45;                              \
          w##k = need_rest > 0 && e + 3 < n_rest &&                                                            \
                 ((((vmask >> r0) & 1) && e - 45 * r0 < need_rest) || (r1 != r0 && ((vmask >> r1) & 1)));      \
          if (w##k) v##k = reinterpret_cast<const float4*>(brest)[lane + 64 * k]; }
#define SH16_PUT(k) if (w##k) reinterpret_cast<float4*>(tile)[lane + 64 * k] = v##k;
        SH16_LD(0) SH16_LD(1) SH16_LD(2) SH16_LD(3) SH16_LD(4) SH16_LD(5) SH16_LD(6) SH16_LD(7) SH16_LD(8) SH16_LD(9) SH16_LD(10) SH16_LD(11)
        if (wd) reinterpret_cast<float4*>(tdc)[lane] = vd;
        SH16_PUT(0) SH16_PUT(1) SH16_PUT(2) SH16_PUT(3) SH16_PUT(4) SH16_PUT(5) SH16_PUT(6) SH16_PUT(7) SH16_PUT(8) SH16_PUT(9) SH16_PUT(10) SH16_PUT(11)
#undef SH16_LD
#undef SH16_PUT
        if (lane < 3) {                                                // ragged last block: the words after the last whole float4
            const int ed = (n_dc & ~3) + (int)lane, er = (n_rest & ~3) + (int)lane;
            if (ed < n_dc) tdc[ed] = bdc[ed];
            if (er < n_rest && need_rest > 0) tile[er] = brest[er];
        }
    }
}

template <int MODE>
__device__ __forceinline__ void sh16_row_to_regs(const float* tile, unsigned lane, int need, float (&c)[48]) {
    if (MODE == SH16_CAT) {
        const float4* t4 = reinterpret_cast<const float4*>(tile) + lane * 13u;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * j < need) t = t4[j];
            c[4 * j] = t.x; c[4 * j + 1] = t.y; c[4 * j + 2] = t.z; c[4 * j + 3] = t.w;
        }
    } else {
        const float* tdc = tile + SH16_REST_WORDS + lane * 3u;
        const float* tr = tile + lane * 45u;
        c[0] = tdc[0]; c[1] = tdc[1]; c[2] = tdc[2];
#pragma unroll
        for (int t = 0; t < 45; t++) c[3 + t] = t < need - 3 ? tr[t] : 0.f;
    }
}

template <int MODE>
__device__ __forceinline__ void sh16_regs_to_row(float* tile, unsigned lane, const float (&g)[48]) {
    if (MODE == SH16_CAT) {
        float4* t4 = reinterpret_cast<float4*>(tile) + lane * 13u;
#pragma unroll
        for (int j = 0; j < 12; j++) t4[j] = make_float4(g[4 * j], g[4 * j + 1], g[4 * j + 2], g[4 * j + 3]);
    } else {
        float* tdc = tile + SH16_REST_WORDS + lane * 3u;
        float* tr = tile + lane * 45u;
        tdc[0] = g[0]; tdc[1] = g[1]; tdc[2] = g[2];
#pragma unroll
        for (int t = 0; t < 45; t++) tr[t] = g[3 + t];
    }
}

// LDS rows -> this block's rows of the gradient arrays, every word, in lane order
template <int MODE>
__device__ __forceinline__ void sh16_stage_out(const float* tile, float* __restrict__ dsh_a, float* __restrict__ dsh_rest, int i0, int nvalid,
                                               unsigned lane) {
    if (MODE == SH16_CAT) {
        float4* b4 = reinterpret_cast<float4*>(dsh_a + (size_t)i0 * 48);
        const float4* t4 = reinterpret_cast<const float4*>(tile);
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const unsigned q = lane + 64u * k, row = q / 12u;
            if ((int)row < nvalid) b4[q] = t4[q + row];
        }
    } else {
        const float* tdc = tile + SH16_REST_WORDS;
        const int n_dc = nvalid * 3, n_rest = nvalid * 45;
        float* bdc = dsh_a + (size_t)i0 * 3;
        float* brest = dsh_rest + (size_t)i0 * 45;
        if (4 * (int)lane + 3 < n_dc) reinterpret_cast<float4*>(bdc)[lane] = reinterpret_cast<const float4*>(tdc)[lane];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int q = (int)lane + 64 * k;
            if (4 * q + 3 < n_rest) reinterpret_cast<float4*>(brest)[q] = reinterpret_cast<const float4*>(tile)[q];
        }
        if (lane < 3) {
            const int ed = (n_dc & ~3) + (int)lane, er = (n_rest & ~3) + (int)lane;
            if (ed < n_dc) bdc[ed] = tdc[ed];
            if (er < n_rest) brest[er] = tile[er];
        }
    }
}

template <int MODE, bool MOTION>
__global__ __launch_bounds__(64) void k_sh16_forward(int P, int D, const float* __restrict__ means3D, const float* __restrict__ campos,
                                                     const float* __restrict__ sh_a, const float* __restrict__ sh_rest,
                                                     const uint8_t* __restrict__ visible, float4* __restrict__ rec, uint8_t* __restrict__ clamped, EgsMotion mot) {
    const unsigned lane = threadIdx.x;
    const int i0 = blockIdx.x * 64, i = i0 + (int)lane;
    const bool inb = i < P;
    const bool vis = inb && visible[i] != 0;
    float p[3] = { 0.f, 0.f, 1.f };
    if (inb) { p[0] = means3D[3 * i]; p[1] = means3D[3 * i + 1]; p[2] = means3D[3 * i + 2]; }   // (in flight together with the rows)
    if constexpr (MOTION) {
        if (vis && (!mot.moved || mot.moved[i])) { const float p0[3] = { p[0], p[1], p[2] }; egs_motion_point(mot.A, p0, p); }
    }
    const uint64_t vmask = __ballot(vis);
    if (!vmask) return;
    const int need = 3 * (D + 1) * (D + 1);
    sh16_stage_in<MODE>(sh_tile, sh_a, sh_rest, i0, min(64, P - i0), vmask, need, lane);
    __syncthreads();
    if (!vis) return;
    float c[48];
    sh16_row_to_regs<MODE>(sh_tile, lane, need, c);
    float x, y, z, inv; sh_view_dir(p, campos, x, y, z, inv);
    float rgb[3];
    const uint32_t cl = sh_colour(D, c, x, y, z, rgb);
    clamped[i] = (uint8_t)((clamped[i] & ~EGS_CLAMP_MASK) | cl);      // (bits 3-5: the HOT code k_preprocess left)
    float* r = reinterpret_cast<float*>(rec + (size_t)i * EGS_SPLAT_REC_F4);
    r[6] = rgb[0]; r[7] = rgb[1]; r[8] = rgb[2];
}

// One span of `n` floats (n4 = n / 4 float4 + a tail) of a leaf stepped with the gradients in `t` (LDS, same order): the stand-alone
// optimizer kernel's arithmetic on the store pattern of sh16_stage_out.
__device__ __forceinline__ void sh16_adam_span(const float* t, const EgsSinkLeaf& f, size_t first, int n, float ss, float ib, float b1, float b2,
                                               float eps, unsigned lane) {
    float* __restrict__ p = f.p + first; float* __restrict__ m = f.m + first; float* __restrict__ v = f.v + first;
    const bool vec = ((((size_t)p) | ((size_t)m) | ((size_t)v)) & 15) == 0;
    for (int q0 = 0; 4 * q0 < n; q0 += 4 * 64) {                      // four float4 per lane and round: twelve loads in flight
        float4 P4[4], M4[4], V4[4]; bool on[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = q0 + (int)lane + 64 * k;
            on[k] = vec && 4 * q + 3 < n;
            if (on[k]) { P4[k] = reinterpret_cast<const float4*>(p)[q]; M4[k] = reinterpret_cast<const float4*>(m)[q]; V4[k] = reinterpret_cast<const float4*>(v)[q]; }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!on[k]) continue;
            const int q = q0 + (int)lane + 64 * k;
            const float4 G = reinterpret_cast<const float4*>(t)[q];
            egs_adam1(P4[k].x, G.x, M4[k].x, V4[k].x, b1, b2, eps, ss, ib); egs_adam1(P4[k].y, G.y, M4[k].y, V4[k].y, b1, b2, eps, ss, ib);
            egs_adam1(P4[k].z, G.z, M4[k].z, V4[k].z, b1, b2, eps, ss, ib); egs_adam1(P4[k].w, G.w, M4[k].w, V4[k].w, b1, b2, eps, ss, ib);
            reinterpret_cast<float4*>(p)[q] = P4[k]; reinterpret_cast<float4*>(m)[q] = M4[k]; reinterpret_cast<float4*>(v)[q] = V4[k];
        }
    }
    const int done = vec ? (n & ~3) : 0;                              // the tail (and everything, if a base is not 16-byte aligned) element by element
    for (int e = done + (int)lane; e < n; e += 64) {
        float P1 = p[e], M1 = m[e], V1 = v[e];
        egs_adam1(P1, t[e], M1, V1, b1, b2, eps, ss, ib);
        p[e] = P1; m[e] = M1; v[e] = V1;
    }
}

// SINK (split arrays only; include/egs_raster.h egs_backward_adam): the launch also takes the Adam step of the leaves whose gradient it
// finishes -- features_dc, features_rest and, because the view-direction term lands here, the positions -- for its 64 rows.
// MOTION: as in k_sh_backward -- and the Adam step of the positions, when this launch takes it, steps with dL/dp = A^T dL/dp'.
template <int MODE, bool SINK, bool MOTION>
__global__ __launch_bounds__(64) void k_sh16_backward(int P, int D, const float* __restrict__ means3D, const float* __restrict__ campos,
                                                      const float* __restrict__ sh_a, const float* __restrict__ sh_rest,
                                                      const int32_t* __restrict__ radii, const uint8_t* __restrict__ clamped,
                                                      const float* __restrict__ dcolors, float* __restrict__ dsh_a, float* __restrict__ dsh_rest,
                                                      float* __restrict__ dmeans3D, EgsSink sink, EgsMotion mot) {
    const unsigned lane = threadIdx.x;
    const int i0 = blockIdx.x * 64, i = i0 + (int)lane;
    const bool inb = i < P;
    const bool vis = inb && radii[i] > 0;
    float p[3] = { 0.f, 0.f, 1.f }, dc[3] = { 0.f, 0.f, 0.f }, gm[3] = { 0.f, 0.f, 0.f };
    uint32_t cl = 0;
    if (inb) {                                                         // everything the row math needs besides the rows, issued up front
        p[0] = means3D[3 * i]; p[1] = means3D[3 * i + 1]; p[2] = means3D[3 * i + 2];
        dc[0] = dcolors[3 * i]; dc[1] = dcolors[3 * i + 1]; dc[2] = dcolors[3 * i + 2];
        cl = clamped[i] & EGS_CLAMP_MASK;
        if (MOTION || D > 0 || (SINK && sink.leaf[EGS_SINK_MEANS3D].p)) { gm[0] = dmeans3D[3 * i]; gm[1] = dmeans3D[3 * i + 1]; gm[2] = dmeans3D[3 * i + 2]; }
    }
    [[maybe_unused]] const float p0[3] = { p[0], p[1], p[2] };
    [[maybe_unused]] bool row_moved = false;
    float red[MOTION ? EGS_MOTION_POSE_SUMS : 1];
    if constexpr (MOTION) {
#pragma unroll
        for (int k = 0; k < EGS_MOTION_POSE_SUMS; k++) red[k] = 0.f;
        row_moved = vis && (!mot.moved || mot.moved[i]);
        if (row_moved) egs_motion_point(mot.A, p0, p);
    }
    const uint64_t vmask = __ballot(vis);
    const int nvalid = min(64, P - i0), need = 3 * (D + 1) * (D + 1);
    float c[48], g[48];
#pragma unroll
    for (int k = 0; k < 48; k++) { c[k] = 0.f; g[k] = 0.f; }
    if (vmask && D > 0) {                                              // the coefficients only enter through the view-direction term
        sh16_stage_in<MODE>(sh_tile, sh_a, sh_rest, i0, nvalid, vmask, need, lane);
        __syncthreads();
        if (vis) sh16_row_to_regs<MODE>(sh_tile, lane, need, c);
    }
    if (vis) {
        float x, y, z, inv; sh_view_dir(p, campos, x, y, z, inv);
        float gdir[3] = { 0.f, 0.f, 0.f };
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float gg = ((cl >> ch) & 1u) ? 0.f : dc[ch];
            sh_channel_backward(D, 0, c, g, ch, x, y, z, gg, gdir);        // (M = 0: nothing to zero above the active degree, g starts as zeros)
        }
        if (D > 0) {
            sh_dir_to_pos(x, y, z, inv, gdir, gm);
            if constexpr (!MOTION) { dmeans3D[3 * i] = gm[0]; dmeans3D[3 * i + 1] = gm[1]; dmeans3D[3 * i + 2] = gm[2]; }
        }
        if constexpr (MOTION) {
            if (row_moved) {
                if (mot.pose_partial) egs_motion_pose_terms(gm, p0, red);
                const float gp[3] = { gm[0], gm[1], gm[2] };
                egs_motion_point_backward(mot.A, gp, gm);
            }
            if (row_moved || D > 0) { dmeans3D[3 * i] = gm[0]; dmeans3D[3 * i + 1] = gm[1]; dmeans3D[3 * i + 2] = gm[2]; }
        }
    }
    if constexpr (MOTION) {
        if (mot.pose_partial) egs_motion_wave_line<EGS_MOTION_POSE_SUMS>(red, mot.pose_partial + (size_t)blockIdx.x * EGS_MOTION_POSE_SUMS);
    }
    sh16_regs_to_row<MODE>(sh_tile, lane, g);                          // (a lane touches only its own row: no barrier since the reads above)
    __syncthreads();
    if (!SINK || dsh_a) sh16_stage_out<MODE>(sh_tile, dsh_a, dsh_rest, i0, nvalid, lane);
    if (SINK && MODE == SH16_SPLIT) {
        if (sink.skip && *sink.skip) return;                          // overflowed frame: no step
        const int rows = sink.active_rows ? min(P, max(*sink.active_rows, 0)) : P;
        const int live = min(64, rows - i0);
        if (live <= 0) return;
        if (sink.leaf[EGS_SINK_SH_REST].p)
            sh16_adam_span(sh_tile, sink.leaf[EGS_SINK_SH_REST], (size_t)i0 * 45, live * 45, sink.coef[2 * EGS_SINK_SH_REST],
                           sink.coef[2 * EGS_SINK_SH_REST + 1], sink.b1, sink.b2, sink.eps, lane);
        if (sink.leaf[EGS_SINK_SH].p)
            sh16_adam_span(sh_tile + SH16_REST_WORDS, sink.leaf[EGS_SINK_SH], (size_t)i0 * 3, live * 3, sink.coef[2 * EGS_SINK_SH],
                           sink.coef[2 * EGS_SINK_SH + 1], sink.b1, sink.b2, sink.eps, lane);
        if (sink.leaf[EGS_SINK_MEANS3D].p && (int)lane < live) {       // three floats per lane (gm is zero for a culled row, as its gradient is)
            const EgsSinkLeaf& f = sink.leaf[EGS_SINK_MEANS3D];
            const float ss = sink.coef[2 * EGS_SINK_MEANS3D], ib = sink.coef[2 * EGS_SINK_MEANS3D + 1];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float P1 = f.p[3 * i + k], M1 = f.m[3 * i + k], V1 = f.v[3 * i + k];
                egs_adam1(P1, gm[k], M1, V1, sink.b1, sink.b2, sink.eps, ss, ib);
                f.p[3 * i + k] = P1; f.m[3 * i + k] = M1; f.v[3 * i + k] = V1;
            }
        }
    }
}

}  // namespace

bool egs_sh_backward_can_sink(int M, const float* sh_a, const float* sh_rest) {
    return M == 16 && sh_rest && ((((uintptr_t)sh_a) | ((uintptr_t)sh_rest)) & 15) == 0;
}
static bool sh16_fast(int M, const void* a, const void* b, const void* c, const void* d) {
    return M == 16 && ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

hipError_t egs_launch_sh_forward(const EgsScene& sc, EgsCamera cam, EgsGeomPtrs g, EgsMotion mot, hipStream_t s) {
    const int P = sc.P, D = sc.D, M = sc.M;
    const float* sh_a = sc.shs; const float* sh_rest = sc.shs_rest;
    if (P == 0) return hipSuccess;
    const dim3 grid((P + 63) / 64), block(64);
#define SHF_ARGS sc.means3D, cam.campos, sh_a, sh_rest, g.visible, g.rec, g.clamped, mot
    if (sh16_fast(M, sh_a, sh_rest, nullptr, nullptr)) {
        const size_t lds16 = sh_rest ? (SH16_REST_WORDS + 192) * sizeof(float) : 64 * 13 * sizeof(float4);
        if (sh_rest) {
            if (mot.A) hipLaunchKernelGGL((k_sh16_forward<SH16_SPLIT, true>), grid, block, lds16, s, P, D, SHF_ARGS);
            else hipLaunchKernelGGL((k_sh16_forward<SH16_SPLIT, false>), grid, block, lds16, s, P, D, SHF_ARGS);
        } else {
            if (mot.A) hipLaunchKernelGGL((k_sh16_forward<SH16_CAT, true>), grid, block, lds16, s, P, D, SHF_ARGS);
            else hipLaunchKernelGGL((k_sh16_forward<SH16_CAT, false>), grid, block, lds16, s, P, D, SHF_ARGS);
        }
        return hipGetLastError();
    }
    const size_t lds = (size_t)64 * (3 * M + 1) * sizeof(float);
    if (mot.A) hipLaunchKernelGGL(k_sh_forward<true>, grid, block, lds, s, P, D, M, SHF_ARGS);
    else hipLaunchKernelGGL(k_sh_forward<false>, grid, block, lds, s, P, D, M, SHF_ARGS);
#undef SHF_ARGS
    return hipGetLastError();
}

hipError_t egs_launch_sh_backward(const EgsScene& sc, EgsCamera cam, const int32_t* radii, EgsGeomPtrs g, const EgsGrads& d, const EgsSink* sink,
                                  EgsMotion mot, hipStream_t s) {
    const int P = sc.P, D = sc.D, M = sc.M;
    const float* sh_a = sc.shs; const float* sh_rest = sc.shs_rest;
    if (P == 0) return hipSuccess;
    const dim3 grid((P + 63) / 64), block(64);
    EgsSink none = {};
#define SHB_ARGS sc.means3D, cam.campos, sh_a, sh_rest, radii, g.clamped, d.colors, d.sh, d.sh_rest, d.means3D
    const size_t lds_split = (SH16_REST_WORDS + 192) * sizeof(float), lds_cat = 64 * 13 * sizeof(float4);
    if (sink) {                                                       // (the caller checked egs_sh_backward_can_sink)
        if (mot.A) hipLaunchKernelGGL((k_sh16_backward<SH16_SPLIT, true, true>), grid, block, lds_split, s, P, D, SHB_ARGS, *sink, mot);
        else hipLaunchKernelGGL((k_sh16_backward<SH16_SPLIT, true, false>), grid, block, lds_split, s, P, D, SHB_ARGS, *sink, mot);
        return hipGetLastError();
    }
    if (sh16_fast(M, sh_a, sh_rest, d.sh, d.sh_rest)) {
        if (sh_rest) {
            if (mot.A) hipLaunchKernelGGL((k_sh16_backward<SH16_SPLIT, false, true>), grid, block, lds_split, s, P, D, SHB_ARGS, none, mot);
            else hipLaunchKernelGGL((k_sh16_backward<SH16_SPLIT, false, false>), grid, block, lds_split, s, P, D, SHB_ARGS, none, mot);
        } else {
            if (mot.A) hipLaunchKernelGGL((k_sh16_backward<SH16_CAT, false, true>), grid, block, lds_cat, s, P, D, SHB_ARGS, none, mot);
            else hipLaunchKernelGGL((k_sh16_backward<SH16_CAT, false, false>), grid, block, lds_cat, s, P, D, SHB_ARGS, none, mot);
        }
        return hipGetLastError();
    }
    const size_t lds = (size_t)64 * (3 * M + 1) * sizeof(float);
    if (mot.A) hipLaunchKernelGGL(k_sh_backward<true>, grid, block, lds, s, P, D, M, SHB_ARGS, mot);
    else hipLaunchKernelGGL(k_sh_backward<false>, grid, block, lds, s, P, D, M, SHB_ARGS, mot);
#undef SHB_ARGS
    return hipGetLastError();
}
