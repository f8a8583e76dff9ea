// object_motion.h -- arithmetic of the rigid object motion (include/egs_raster.h egs_object_move_points): one place for every
// kernel that places a row, chains a gradient through the placement, or sums the pose gradient.
//   p' = A p + b          A12 = [A | b], row-major 3x4 in device memory
//   dL/dp = A^T g         g = dL/dp'
//   dL/dA = sum g p^T     dL/db = sum g        (12 sums, in A12's layout)
// The translation units are compiled with -ffp-contract=off, so the fused multiply-adds below are exactly the ones written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define EGS_MOTION_POSE_SUMS 12        // dL/dA12
#define EGS_MOTION_ROT_SUMS 9          // dL/dM9
#define EGS_MOTION_SUMS (EGS_MOTION_POSE_SUMS + EGS_MOTION_ROT_SUMS)

// Scratch of the pose reduction (egs_object_motion_scratch_bytes): lines of 12 pose sums, one per workgroup of the launch that finishes
// the positions' gradient -- 256 rows each, or 64 when that launch is the spherical-harmonics backward -- then one line of 9 rotation
// sums per 256 rows.
__host__ __device__ inline size_t egs_motion_pose_lines_max(int P) { return ((size_t)P + 63) / 64; }
__host__ __device__ inline size_t egs_motion_rot_lines(int P) { return ((size_t)P + 255) / 256; }
__host__ __device__ inline size_t egs_motion_rot_offset(int P) { return egs_motion_pose_lines_max(P) * EGS_MOTION_POSE_SUMS; }      // floats
__host__ __device__ inline size_t egs_motion_scratch_floats(int P) {
    return P > 0 ? egs_motion_rot_offset(P) + egs_motion_rot_lines(P) * EGS_MOTION_ROT_SUMS : 0;
}

// Whether row i is placed: inside the live rows (capacity-sized models) and selected by the EXACT mask (NULL = every row).
__device__ __forceinline__ bool egs_motion_row_moved(int i, int live, const uint8_t* __restrict__ moved) {
    return i < live && (!moved || moved[i] != 0);
}

// p' = A p + b: per component one chain of three fused multiply-adds, x then y then z onto the translation.
__device__ __forceinline__ void egs_motion_point(const float* __restrict__ A12, const float* p, float* o) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = fmaf(A12[4 * r + 2], p[2], fmaf(A12[4 * r + 1], p[1], fmaf(A12[4 * r], p[0], A12[4 * r + 3])));
}

// dL/dp = A^T g, the same shape of chain over the rows of A.
__device__ __forceinline__ void egs_motion_point_backward(const float* __restrict__ A12, const float* g, float* o) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = fmaf(A12[8 + c], g[2], fmaf(A12[4 + c], g[1], A12[c] * g[0]));
}

// One row's share of dL/dA12: t[4 r + c] = g_r p_c, t[4 r + 3] = g_r (one product rounding per term, none for the translation).
__device__ __forceinline__ void egs_motion_pose_terms(const float* g, const float* p, float* t) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        t[4 * r] = g[r] * p[0]; t[4 * r + 1] = g[r] * p[1]; t[4 * r + 2] = g[r] * p[2]; t[4 * r + 3] = g[r];
    }
}

// Sum of NV per-lane values over a 256-thread workgroup, written as one plain line line[0 .. NV): six __shfl_xor levels inside the
// wave, then the four waves through LDS as (w0 + w1) + (w2 + w3) -- an eight-deep float32 tree whose shape never depends on the
// data, so the line is a pure function of the lanes' values.  No atomics; the lines are added by k_motion_finish.  Every thread
// of the workgroup must call it (it holds a barrier).
template <int NV>
__device__ __forceinline__ void egs_motion_block_sum(const float* v, float (*wsum)[NV], float* __restrict__ line) {
#pragma unroll
    for (int k = 0; k < NV; k++) {
        float s = v[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) line[threadIdx.x] = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
}

// The same for a workgroup of ONE wave (the spherical-harmonics kernels): the six shuffle levels, lane 0 writes the line.
template <int NV>
__device__ __forceinline__ void egs_motion_wave_line(const float* v, float* __restrict__ line) {
#pragma unroll
    for (int k = 0; k < NV; k++) {
        float s = v[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if ((threadIdx.x & 63) == 0) line[k] = s;
    }
}

// The finish of one component: the workgroup lines in index order, in float64.
__device__ __forceinline__ double egs_motion_finish_span(const float* __restrict__ partial, int b0, int b1, int stride, int k) {
    double t = 0.0;
    for (int b = b0; b < b1; b++) t += (double)partial[(size_t)b * stride + k];
    return t;
}
