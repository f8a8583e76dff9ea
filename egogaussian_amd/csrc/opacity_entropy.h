// opacity_entropy.h -- arithmetic of the opacity-entropy regulariser (include/egs_raster.h egs_opacity_entropy): one place for the
// stand-alone kernels (entropy.hip) and for the rasterizer's preprocess backward (preprocess.hip pp_bwd_one<.., ENT = true>).
// Between std_train_iter and std_train_iter + entropy_reg_iter both static trainers add
//     0.1 * mean over the visible Gaussians of  -o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10)
// to the image loss (/root/reference/trainers/train_static.py:97-102, trainers/train_static_bg.py:105-110).  Per visible row, with o the
// float32 activated opacity the forward blended with:
//     a = o + 1e-10f      b = (1.0f - o) + 1e-10f                      (float32, as the reference forms them)
//     h     = -o logf(a) - (1 - o) logf(b)
//     dh/do = -logf(a) - o / a + logf(b) + (1 - o) / b
//     value = (sum of h over the visible rows) / n_vis
//     dL/do += weight * upstream / n_vis * dh/do                       (then the sigmoid chain when the opacity arrives as a logit)
// o == 0 and o == 1 are finite: the 1e-10 keeps both logarithms finite (a or b is 1e-10, the other exactly 1).
// The translation units are compiled with -ffp-contract=off: the operations below are exactly the ones written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define EGS_ENTROPY_EPS 1e-10f

// Kernel argument of the entropy instantiation of k_preprocess_backward: three device words.
struct EgsEntropy {
    const uint32_t* n_vis;         // visible rows of this frame (k_entropy_finish)
    const float* weight;           // device float[1]
    const float* upstream;         // device float[1] or nullptr (= 1)
};
struct EgsNoEntropy {};            // what the other instantiations take in its place: nothing

// Scratch of the reduction (egs_opacity_entropy_scratch_bytes): one float32 sum of h and one uint32 count per 256 rows.
__host__ __device__ inline size_t egs_entropy_lines(int P) { return P > 0 ? ((size_t)P + 255) / 256 : 0; }

// The activated opacity of a logit, as k_preprocess forms it (preprocess.hip).
__device__ __forceinline__ float egs_entropy_activate(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float egs_entropy_h(float o) {
    const float a = o + EGS_ENTROPY_EPS, om = 1.f - o, b = om + EGS_ENTROPY_EPS;
    return -o * logf(a) - om * logf(b);
}

__device__ __forceinline__ float egs_entropy_dh(float o) {
    const float a = o + EGS_ENTROPY_EPS, om = 1.f - o, b = om + EGS_ENTROPY_EPS;
    return -logf(a) - o / a + logf(b) + om / b;
}

// weight * upstream / n_vis, read from the device words; no visible row: 0 (no gradient anywhere).
__device__ __forceinline__ float egs_entropy_coef(const uint32_t* __restrict__ n_vis, const float* __restrict__ weight, const float* __restrict__ upstream) {
    const uint32_t n = *n_vis;
    if (n == 0u) return 0.f;
    return weight[0] * (upstream ? upstream[0] : 1.f) / (float)n;
}

// One visible row's addend to dL/do.
__device__ __forceinline__ float egs_entropy_grad(float coef, float o) { return coef * egs_entropy_dh(o); }
