// cov3d.hip -- fused 3D covariance producer, forward and backward.
// Replaces the chain of PyTorch ops the reference runs before EVERY rasterizer call because it forces
// pipe.compute_cov3D_python = True (/root/reference/train.py:49):
//   build_rotation / build_scaling_rotation / strip_symmetric     /root/reference/utils/general_utils.py:110-156
//   covariance activation and its object-rotated variant          /root/reference/scene/gaussian_model.py:29-33,46-63
// i.e.  q <- q/|q| ;  L = R(q) diag(mod * s) ;  [L <- M L for selected rows] ;  Sigma = L L^T ;  out = 6 unique entries.
// In PyTorch that is ~15 kernels forward and ~40 backward over [N,3,3] temporaries (and, with the reference's own
// `L @ L.transpose`, a 500k-batch 3x3 GEMM that rocBLAS runs for milliseconds).  Here: one streaming kernel each way,
// 28 B in / 24 B out per Gaussian forward, 52 B in / 28 B out backward; HBM-bound.
#include "egs_common.h"
#include "splat_geom.h"          // the chain itself: the one text preprocess.hip's in-rasterizer rotation runs too

namespace {

// `log_scaling`: the scaling tensor holds the RAW parameters (log of the scales, /root/reference/scene/gaussian_model.py:36
// scaling_activation = torch.exp); the exponential and its derivative are then applied here instead of by two more
// elementwise kernels over [N,3] per step.
__global__ __launch_bounds__(256) void k_cov3d_forward(int N, const float* __restrict__ scaling, int log_scaling, float mod,
                                                        const float* __restrict__ rotation, const float* __restrict__ M,
                                                        const uint8_t* __restrict__ sel, float* __restrict__ cov,
                                                        const float* __restrict__ opacity_raw, float* __restrict__ opacity) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (opacity_raw) opacity[i] = 1.f / (1.f + expf(-opacity_raw[i]));           // opacity_activation = torch.sigmoid (gaussian_model.py:40)
    float q[4] = { rotation[4 * i], rotation[4 * i + 1], rotation[4 * i + 2], rotation[4 * i + 3] };
    float s3[3] = { scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2] };
    float inv; activate_scale_rot(log_scaling != 0, true, s3, q, inv);
    CovFactor f; cov_factor(s3, mod, q, M && (!sel || sel[i]), M, f);
    cov_from_factor(f.L, cov + 6 * (size_t)i);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_cov3d_backward(int N, const float* __restrict__ scaling, int log_scaling, float mod,
                                                         const float* __restrict__ rotation, const float* __restrict__ M,
                                                         const uint8_t* __restrict__ sel, float row0_mult,
                                                         const float* __restrict__ row0_mult_dev,
                                                         const float* __restrict__ dcov, float* __restrict__ dscaling,
                                                         float* __restrict__ drotation, float* __restrict__ dM_partial,
                                                         const float* __restrict__ opacity, const float* __restrict__ dopacity,
                                                         float* __restrict__ dopacity_raw) {
    __shared__ float wsum[4][9];
    if (opacity && blockIdx.x * blockDim.x + threadIdx.x < (unsigned)N) {
        const int j = blockIdx.x * blockDim.x + threadIdx.x;
        const float o = opacity[j];
        dopacity_raw[j] = dopacity[j] * ((1.f - o) * o);                        // sigmoid backward: grad * (1 - y) * y
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float gM[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (i < N) {
        float q[4] = { rotation[4 * i], rotation[4 * i + 1], rotation[4 * i + 2], rotation[4 * i + 3] };
        float s3[3] = { scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2] };
        float inv; activate_scale_rot(log_scaling != 0, true, s3, q, inv);
        const bool moved = M && (!sel || sel[i]);
        CovFactor f; cov_factor(s3, mod, q, moved, M, f);
        const float* g6 = dcov + 6 * (size_t)i;
        const float mult = (moved && i == 0) ? (row0_mult_dev ? row0_mult_dev[0] : row0_mult) : 1.f;   // the reference's duplicated-index gradient (covariance.py)
        CovGrad g; cov_factor_backward(f, s3, mod, q, inv, moved, M, g6, mult, true, log_scaling != 0, true, g);
#pragma unroll
        for (int k = 0; k < 9; k++) gM[k] = g.dM[k];
#pragma unroll
        for (int k = 0; k < 3; k++) dscaling[3 * i + k] = g.dscale[k];   // d/d raw = d/d scale * exp(raw) under log_scaling
#pragma unroll
        for (int k = 0; k < 4; k++) drotation[4 * i + k] = g.gq[k];
    }
    // d/dM is a sum over every Gaussian.  One float atomic per wave and component (70k device-scope atomics on nine words
    // of one cache line at 500k Gaussians) serialises at the memory side: 896 us for this kernel instead of 9.  Workgroup
    // partial sums are written out plainly and added up by k_cov3d_dm_finish.
    if (dM_partial) {                                                      // workgroup-uniform branch
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const float s = wave_sum(gM[k]);
            if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = s;
        }
        __syncthreads();
        if (threadIdx.x < 9) dM_partial[(size_t)blockIdx.x * 9 + threadIdx.x] = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
    }
}

__global__ __launch_bounds__(1024) void k_cov3d_dm_finish(int nblocks, const float* __restrict__ partial, float* __restrict__ dM) {
    __shared__ float red[16];
    for (int k = 0; k < 9; k++) {
        float v = 0.f;
        for (int b = threadIdx.x; b < nblocks; b += 1024) v += partial[(size_t)b * 9 + k];
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) { float t = 0.f; for (int w = 0; w < 16; w++) t += red[w]; dM[k] = t; }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int egs_cov3d_forward(int N, const float* scaling, int scaling_is_log, float scale_modifier, const float* rotation, const float* M9,
                      const uint8_t* selected, float* cov6, const float* opacity_raw, float* opacity, void* stream) {
    if (N < 0) return EGS_ERR_ARG;
    if (N == 0) return 0;
    if (!scaling || !rotation || !cov6 || (opacity_raw && !opacity)) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_cov3d_forward, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, scaling, scaling_is_log, scale_modifier,
                       rotation, M9, selected, cov6, opacity_raw, opacity);
    return (int)hipGetLastError();
}

size_t egs_cov3d_dm_scratch_floats(int N) { return N > 0 ? (size_t)((N + 255) / 256) * 9 : 0; }

int egs_cov3d_backward(int N, const float* scaling, int scaling_is_log, float scale_modifier, const float* rotation, const float* M9,
                       const uint8_t* selected, float row0_grad_mult, const float* row0_grad_mult_dev, const float* dL_dcov6, float* dL_dscaling,
                       float* dL_drotation, float* dL_dM9, float* dM_scratch, const float* opacity, const float* dL_dopacity,
                       float* dL_dopacity_raw, void* stream) {
    if (N < 0) return EGS_ERR_ARG;
    if (dL_dM9 && N == 0) { hipError_t e = egs_launch_zero_u32((uint32_t*)dL_dM9, 9, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
    if (N == 0) return 0;
    if (!scaling || !rotation || !dL_dcov6 || !dL_dscaling || !dL_drotation) return EGS_ERR_ARG;
    if (M9 && dL_dM9 && !dM_scratch) return EGS_ERR_ARG;
    if (opacity && (!dL_dopacity || !dL_dopacity_raw)) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_cov3d_backward, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, scaling, scaling_is_log, scale_modifier,
                       rotation, M9, selected, row0_grad_mult, row0_grad_mult_dev, dL_dcov6, dL_dscaling, dL_drotation, (M9 && dL_dM9) ? dM_scratch : nullptr,
                       opacity, dL_dopacity, dL_dopacity_raw);
    if (dL_dM9) {
        if (M9) hipLaunchKernelGGL(k_cov3d_dm_finish, dim3(1), dim3(1024), 0, (hipStream_t)stream, (N + 255) / 256, dM_scratch, dL_dM9);
        else { hipError_t e = egs_launch_zero_u32((uint32_t*)dL_dM9, 9, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
    }
    return (int)hipGetLastError();
}

}  // extern "C"
