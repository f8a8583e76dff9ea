// loss_window.h -- the SSIM window of the image loss (loss.hip; also the loss gradient computed inside the backward blend, render_bwd.hip).
#pragma once
// gaussian(11, 1.5) normalised, as float32 (/root/reference/utils/loss_utils.py:66-68)
#define KW0 1.028380124e-03f
#define KW1 7.598758209e-03f
#define KW2 3.600077331e-02f
#define KW3 1.093606874e-01f
#define KW4 2.130055279e-01f
#define KW5 2.660117149e-01f
__device__ __forceinline__ constexpr float kwin(int k) {
    return k == 0 || k == 10 ? KW0 : k == 1 || k == 9 ? KW1 : k == 2 || k == 8 ? KW2 : k == 3 || k == 7 ? KW3 : k == 4 || k == 6 ? KW4 : KW5;
}

// The scalar loss from the per-strip partial sums, by ONE wave (fixed order, so the value is deterministic): used by the backward kernel when the caller deferred
// the loss value to it (egs_l1_ssim_forward with loss == NULL) -- a training step replayed from a graph reads the value only after
// the backward anyway, and every launch it does not make is ~4.5 us of GPU time.
__device__ __forceinline__ void wave_finish_loss(size_t nblocks, const float* __restrict__ partial, float w_l1, float w_ssim, float lambda,
                                                 float* __restrict__ loss, float* __restrict__ running_sum, unsigned lane) {
    float a = 0.f, b = 0.f;
    for (size_t i0 = 0; i0 < nblocks; i0 += 64 * 8) {                  // eight loads in flight per lane
        float2 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { const size_t i = i0 + (size_t)k * 64 + lane; v[k] = i < nblocks ? reinterpret_cast<const float2*>(partial)[i] : make_float2(0.f, 0.f); }
#pragma unroll
        for (int k = 0; k < 8; k++) { a += v[k].x; b += v[k].y; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    if (lane == 0) {
        const float v = w_l1 * a + lambda - w_ssim * b;
        if (loss) loss[0] = v;
        if (running_sum) running_sum[0] += v;
    }
}

// ---- the object stages' loss (include/egs_raster.h egs_object_loss):
//     lambda_image * [(1 - lambda) L1 + lambda (1 - SSIM)](image, gt) + lambda_l1a * mean|m - alpha| + lambda_l2a * mean (m - alpha)^2
// What the kernels need of it, device side.  The image term's partial sums and weights are those of the plain loss; the alpha sums have
// a partial array of their own (one float2 per strip of ONE plane).
struct EgsObjLossK {
    const float* alpha; const float* mask;          // [H,W] each
    float* apartial;                                // [strips of one plane] x (sum |m - alpha|, sum (m - alpha)^2)
    float* terms;                                   // device float[3] or NULL: image loss, mean |m - alpha|, mean (m - alpha)^2
    float w_l1a, w_l2a2;                            // lambda_l1a / (H W), 2 lambda_l2a / (H W): the weights of the alpha gradient
    float l_img, l_l1a, l_l2a, inv_hw;              // the value: l_img * image loss + l_l1a * (inv_hw * sum|.|) + l_l2a * (inv_hw * sum(.)^2)
    float fin_w_l1, fin_w_ssim;                     // (1 - lambda) / n, lambda / n: the image loss's own weights (NOT scaled by lambda_image)
    unsigned n_astrips;
};

// dL/dalpha at one pixel: gate * up * (lambda_l1a sign(alpha - m) + 2 lambda_l2a (alpha - m)) / (H W), sign(0) = 0 -- a pixel no splat reached
// has alpha = 0 exactly on a mask of 0 and gets 0, as torch's abs() backward gives.  ONE definition for the loss-backward launch (loss.hip) and for the
// backward blend that computes it itself (render_bwd.hip): every operation is spelled out, so the two are bit-identical.
__device__ __forceinline__ float egs_alpha_grad(float alpha, float m, float w1, float w2, float up, bool gated, float gate) {
    const float d = alpha - m;
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    float g = __fmaf_rn(w2, d, __fmul_rn(w1, sgn));
    g = __fmul_rn(g, up);
    if (gated) g = __fmul_rn(g, gate);
    return g;
}

// wave_finish_loss with the alpha terms: the image sums are added in the same order (with every alpha weight 0 and lambda_image 1 the value is the plain loss's, bit for bit)
__device__ __forceinline__ void wave_finish_obj_loss(size_t nblocks, const float* __restrict__ partial, float lambda, const EgsObjLossK& o,
                                                     float* __restrict__ loss, float* __restrict__ running_sum, unsigned lane) {
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
    for (size_t i0 = 0; i0 < nblocks; i0 += 64 * 8) {
        float2 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { const size_t i = i0 + (size_t)k * 64 + lane; v[k] = i < nblocks ? reinterpret_cast<const float2*>(partial)[i] : make_float2(0.f, 0.f); }
#pragma unroll
        for (int k = 0; k < 8; k++) { a += v[k].x; b += v[k].y; }
    }
    for (unsigned i = lane; i < o.n_astrips; i += 64) { const float2 v = reinterpret_cast<const float2*>(o.apartial)[i]; c += v.x; d += v.y; }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { a += __shfl_xor(a, s, 64); b += __shfl_xor(b, s, 64); c += __shfl_xor(c, s, 64); d += __shfl_xor(d, s, 64); }
    if (lane == 0) {
        const float img = o.fin_w_l1 * a + lambda - o.fin_w_ssim * b;
        const float t1 = o.inv_hw * c, t2 = o.inv_hw * d;
        const float v = __fmaf_rn(o.l_l2a, t2, __fmaf_rn(o.l_l1a, t1, o.l_img * img));
        if (o.terms) { o.terms[0] = img; o.terms[1] = t1; o.terms[2] = t2; }
        if (loss) loss[0] = v;
        if (running_sum) running_sum[0] += v;
    }
}

