// label_bce.h -- the label phase's loss, BCE-with-logits of the channel mean of the label render against the object mask
// (/root/reference/trainers/train_static.py:104-109), as the kernels see it.  ONE definition for the stand-alone loss launches
// (label_loss.hip), for the backward blend that forms the gradient itself (render_bwd.hip k_render_backward<3, true>) and for the launch
// that finishes the step (k_label_finish): every operation is spelled out, so the three are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

// x = (C0 + C1 + C2) / 3: the logit of one pixel (torch: render_label.mean(0))
__device__ __forceinline__ float egs_label_logit(float c0, float c1, float c2) {
    return __fdiv_rn(__fadd_rn(__fadd_rn(c0, c1), c2), 3.f);
}
// l = max(x, 0) - x m + log1p(exp(-|x|))   (torch's binary_cross_entropy_with_logits, overflow-safe for any x)
__device__ __forceinline__ float egs_label_bce_value(float x, float m) {
    return __fadd_rn(__fsub_rn(fmaxf(x, 0.f), __fmul_rn(x, m)), log1pf(expf(-fabsf(x))));
}
// dL/dx = up * gate * (sigmoid(x) - m) / (H W); the sigmoid in the two-branch form that never exponentiates a positive number
__device__ __forceinline__ float egs_label_bce_grad(float x, float m, float inv_hw, float up, bool gated, float gate) {
    float sig;
    if (x >= 0.f) sig = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x)));
    else { const float e = expf(x); sig = __fdiv_rn(e, __fadd_rn(1.f, e)); }
    float g = __fmul_rn(__fmul_rn(__fsub_rn(sig, m), inv_hw), up);
    if (gated) g = __fmul_rn(g, gate);
    return g;
}

// What the loss needs of its caller, device side.  The value's partial sums are one float per (tile, 8x8 quadrant) -- partial[tile * 4 + q],
// the sum of l over the quadrant's pixels inside the image, 0 for a quadrant outside it -- whoever writes them (k_label_bce_forward or the
// backward blend): the same 64 values go through the same butterfly, so the two are bit-identical.
struct EgsLabelLossK {
    const float* img; const float* mask; const float* gate; const float* up;      // [3,H,W], [H,W], [H,W] or NULL, device float[1]
    float* partial; float inv_hw;
};

// the wave's sum of l (lanes outside the image hold 0), every lane ends up with it
__device__ __forceinline__ float egs_label_wave_sum(float l) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) l += __shfl_xor(l, d, 64);
    return l;
}

// The loss value from the quadrant partials, by ONE wave: lane k adds partials k, k + 64, ... in index order in float64, then a fixed
// butterfly (float64 as well) -- deterministic, the same bits from whichever launch carries it.
__device__ __forceinline__ void egs_label_wave_finish(size_t n, const float* __restrict__ partial, float inv_hw, float* __restrict__ loss,
                                                      float* __restrict__ running_sum, unsigned lane) {
    double a = 0.0;
    for (size_t i0 = 0; i0 < n; i0 += 64 * 8) {                        // eight loads in flight per lane, added in index order
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { const size_t i = i0 + (size_t)k * 64 + lane; v[k] = i < n ? partial[i] : 0.f; }
#pragma unroll
        for (int k = 0; k < 8; k++) a += (double)v[k];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
    if (lane == 0) {
        const float v = (float)(a * (double)inv_hw);
        if (loss) loss[0] = v;
        if (running_sum) running_sum[0] += v;
    }
}
