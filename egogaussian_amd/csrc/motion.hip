// motion.hip -- rigid object motion of the positions as stand-alone launches (include/egs_raster.h):
//   egs_object_move_points            p'_i = A p_i + b for the moved rows, a copy for the others
//   egs_object_move_points_backward   dL/dp_i = A^T g_i, and dL/dA12 = sum over the moved rows of [g p^T | g]
// Replaces what the reference runs around EVERY render of a dynamic frame to pose the object -- apply_T_xyz's
// cat / matmul / slice and the torch.where around it (/root/reference/utils/geometry_utils.py:188-193,
// /root/reference/scene/gaussian_model.py:939-986), ObjectMove.forward for the trainable part (geometry_utils.py:19-21) -- and, since
// nothing is mutated, the matrix inverse that undoes it afterwards (reverse_trans_rot_new, gaussian_model.py:1037-1060).
// One lane per row, 12 B in / 12 B out; the pose gradient is a deterministic reduction (object_motion.h): workgroup lines, then one
// finish workgroup.  No float atomics (cov3d.hip records what they cost on a handful of words).
#include "egs_common.h"
#include "object_motion.h"

namespace {

__global__ __launch_bounds__(256) void k_move_points(int P, const float* __restrict__ means3D, const float* __restrict__ A12,
                                                     const uint8_t* __restrict__ moved, const int32_t* __restrict__ active_count,
                                                     float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int live = active_count ? min(P, max(*active_count, 0)) : P;
    const float p[3] = { means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2] };
    float o[3] = { p[0], p[1], p[2] };
    if (egs_motion_row_moved(i, live, moved)) egs_motion_point(A12, p, o);
    out[3 * (size_t)i] = o[0]; out[3 * (size_t)i + 1] = o[1]; out[3 * (size_t)i + 2] = o[2];
}

// POSE: the workgroup also writes its line of the 12 pose sums (compiled out otherwise: no shuffles, no barrier).
template <bool POSE>
__global__ __launch_bounds__(256) void k_move_points_backward(int P, const float* __restrict__ means3D, const float* __restrict__ A12,
                                                              const uint8_t* __restrict__ moved, const int32_t* __restrict__ active_count,
                                                              const float* __restrict__ g_in, float* __restrict__ dmeans3D,
                                                              float* __restrict__ partial) {
    __shared__ float wsum[4][POSE ? EGS_MOTION_POSE_SUMS : 1];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float t[EGS_MOTION_POSE_SUMS];
#pragma unroll
    for (int k = 0; k < EGS_MOTION_POSE_SUMS; k++) t[k] = 0.f;
    if (i < P) {
        const int live = active_count ? min(P, max(*active_count, 0)) : P;
        const float g[3] = { g_in[3 * (size_t)i], g_in[3 * (size_t)i + 1], g_in[3 * (size_t)i + 2] };
        float o[3] = { g[0], g[1], g[2] };
        if (egs_motion_row_moved(i, live, moved)) {
            egs_motion_point_backward(A12, g, o);
            if (POSE) {
                const float p[3] = { means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2] };
                egs_motion_pose_terms(g, p, t);
            }
        }
        if (dmeans3D) { dmeans3D[3 * (size_t)i] = o[0]; dmeans3D[3 * (size_t)i + 1] = o[1]; dmeans3D[3 * (size_t)i + 2] = o[2]; }
    }
    if constexpr (POSE) egs_motion_block_sum<EGS_MOTION_POSE_SUMS>(t, wsum, partial + (size_t)blockIdx.x * EGS_MOTION_POSE_SUMS);
}

// One workgroup.  Component k of the lines is added in index order, in float64: sixteen threads take one contiguous span of the lines
// each, then the first of them adds the sixteen span sums in order -- the grouping is fixed by the line count alone.
// out[0..12) from the pose lines, out[12..21) (when out_has_rot) from the rotation lines; no lines: zeros.
#define EGS_FIN_SPANS 16
__global__ __launch_bounds__(EGS_MOTION_SUMS * EGS_FIN_SPANS) void k_motion_finish(const float* __restrict__ pose_partial, int pose_lines,
                                                                                   const float* __restrict__ dM_partial, int dM_lines,
                                                                                   int out_has_rot, float* __restrict__ out) {
    __shared__ double span[EGS_MOTION_SUMS][EGS_FIN_SPANS];
    const int k = (int)threadIdx.x / EGS_FIN_SPANS, c = (int)threadIdx.x % EGS_FIN_SPANS;
    const bool pose = k < EGS_MOTION_POSE_SUMS;
    const float* part = pose ? pose_partial : dM_partial;
    const int lines = part ? (pose ? pose_lines : dM_lines) : 0, per = (lines + EGS_FIN_SPANS - 1) / EGS_FIN_SPANS;
    const int b0 = min(lines, c * per), b1 = min(lines, b0 + per);
    span[k][c] = egs_motion_finish_span(part, b0, b1, pose ? EGS_MOTION_POSE_SUMS : EGS_MOTION_ROT_SUMS, pose ? k : k - EGS_MOTION_POSE_SUMS);
    __syncthreads();
    if (c == 0 && (pose || out_has_rot)) {
        double t = 0.0;
        for (int j = 0; j < EGS_FIN_SPANS; j++) t += span[k][j];
        out[k] = (float)t;
    }
}

}  // namespace

hipError_t egs_launch_motion_finish(const float* pose_partial, int pose_lines, const float* dM_partial, int dM_lines, float* grad21, hipStream_t s) {
    hipLaunchKernelGGL(k_motion_finish, dim3(1), dim3(EGS_MOTION_SUMS * EGS_FIN_SPANS), 0, s, pose_partial, pose_lines, dM_partial, dM_lines, 1, grad21);
    return hipGetLastError();
}

extern "C" {

size_t egs_object_motion_scratch_bytes(int P) { return egs_motion_scratch_floats(P) * sizeof(float); }

int egs_object_move_points(int P, const float* means3D, const float* A12, const uint8_t* moved, const int32_t* active_count, float* out,
                           void* stream) {
    if (P < 0) return EGS_ERR_ARG;
    if (P == 0) return 0;
    if (!means3D || !A12 || !out) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_move_points, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, means3D, A12, moved, active_count, out);
    return (int)hipGetLastError();
}

int egs_object_move_points_backward(int P, const float* means3D, const float* A12, const uint8_t* moved, const int32_t* active_count,
                                    const float* g, float* dmeans3D, float* grad12, void* scratch, void* stream) {
    if (P < 0) return EGS_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        if (grad12) { hipError_t e = egs_launch_zero_u32((uint32_t*)grad12, EGS_MOTION_POSE_SUMS, s); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    if (!A12 || !g || (!dmeans3D && !grad12)) return EGS_ERR_ARG;
    if (grad12 && (!means3D || !scratch)) return EGS_ERR_ARG;
    const int nblocks = (P + 255) / 256;
    if (grad12) {
        hipLaunchKernelGGL(k_move_points_backward<true>, dim3(nblocks), dim3(256), 0, s, P, means3D, A12, moved, active_count, g, dmeans3D,
                           (float*)scratch);
        hipLaunchKernelGGL(k_motion_finish, dim3(1), dim3(EGS_MOTION_SUMS * EGS_FIN_SPANS), 0, s, (const float*)scratch, nblocks, (const float*)nullptr, 0, 0, grad12);
    } else {
        hipLaunchKernelGGL(k_move_points_backward<false>, dim3(nblocks), dim3(256), 0, s, P, means3D, A12, moved, active_count, g, dmeans3D,
                           (float*)nullptr);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
