// label_loss.hip -- the label phase of the static stage (/root/reference/trainers/train_static.py:104-109):
//   loss = BCEWithLogits(mean_c(render_label), obj_mask), the gradient gated by 1 - hand_mask, Adam on the label alone.
// The arithmetic of one pixel is label_bce.h's.  Here: the loss as launches of its own (the eager route, and the yardstick of the
// backward blend that forms the gradient itself, render_bwd.hip k_render_backward<3, true>) and the launch that ends a label step,
// k_label_finish: the per-Gaussian gradient out of the accumulator lines, the label's Adam step and the loss value.
// One workgroup per 16x16 tile, wave q = its 8x8 quadrant q (the blend's mapping), so that the value's partial sums -- one per quadrant,
// 64 values through one butterfly -- are the same bits whichever launch wrote them.
#include "egs_common.h"
#include "label_bce.h"

namespace {

__global__ __launch_bounds__(256) void k_label_bce_forward(int W, int H, int gx, const float* __restrict__ img, const float* __restrict__ mask,
                                                           float* __restrict__ partial) {
    const int tile = (int)blockIdx.x;
    const unsigned lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int px = (tile % gx) * EGS_TILE + (int)(q & 1) * 8 + (int)(lane & 7), py = (tile / gx) * EGS_TILE + (int)(q >> 1) * 8 + (int)(lane >> 3);
    float l = 0.f;
    if (px < W && py < H) {
        const size_t pix = (size_t)py * W + px, HW = (size_t)H * W;
        l = egs_label_bce_value(egs_label_logit(img[pix], img[HW + pix], img[2 * HW + pix]), mask[pix]);
    }
    l = egs_label_wave_sum(l);
    if (lane == 0) partial[(size_t)tile * 4 + q] = l;
}

__global__ __launch_bounds__(64) void k_label_bce_finish(size_t n, const float* __restrict__ partial, float inv_hw, float* loss, float* running) {
    egs_label_wave_finish(n, partial, inv_hw, loss, running, threadIdx.x);
}

// dL/dC[3,H,W]: dL/dx / 3 in each plane.  fin_partial != NULL: one wave also assembles the value the forward deferred.
__global__ __launch_bounds__(256) void k_label_bce_backward(int W, int H, int gx, int n_tiles, EgsLabelLossK k, float* __restrict__ dimg,
                                                            const float* __restrict__ fin_partial, float* fin_loss, float* fin_running) {
    const int tile = (int)blockIdx.x;
    const unsigned lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    if (fin_partial && tile == 0 && q == 0) egs_label_wave_finish((size_t)n_tiles * 4, fin_partial, k.inv_hw, fin_loss, fin_running, lane);
    const int px = (tile % gx) * EGS_TILE + (int)(q & 1) * 8 + (int)(lane & 7), py = (tile / gx) * EGS_TILE + (int)(q >> 1) * 8 + (int)(lane >> 3);
    if (px >= W || py >= H) return;
    const size_t pix = (size_t)py * W + px, HW = (size_t)H * W;
    const float x = egs_label_logit(k.img[pix], k.img[HW + pix], k.img[2 * HW + pix]);
    const float g = egs_label_bce_grad(x, k.mask[pix], k.inv_hw, k.up[0], k.gate != nullptr, k.gate ? k.gate[pix] : 1.f);
    const float g3 = __fdiv_rn(g, 3.f);
    dimg[pix] = g3; dimg[HW + pix] = g3; dimg[2 * HW + pix] = g3;
}

// The last launch of a label step.  Thread i: g_i = slot 6 of Gaussian i's accumulator line plus its replica lines when it is hot (exactly 0
// when radii[i] <= 0: its line was never added to and its hot code never written), written to dlabel if wanted; with an Adam leaf the
// label's step for EVERY live row, zero-gradient rows included -- torch's Adam is dense: the moments decay and the parameter moves on
// momentum -- with egs_adam1 and the two coefficients the prologue's egs_adam_tick left: bit-identical to k_adam fed the same g.
// An overflowed frame (skip set) writes no gradient and takes no step.  One wave also assembles the loss value from the quadrant partials.
__global__ __launch_bounds__(256) void k_label_finish(int P, const float* __restrict__ grad_acc, const float* __restrict__ hot_acc, size_t hot_slots,
                                                      const uint8_t* __restrict__ clamped, const int32_t* __restrict__ radii, float* __restrict__ dlabel,
                                                      EgsLabelAdam ad, const uint32_t* __restrict__ skip, const float* __restrict__ partial, size_t n_partial,
                                                      float inv_hw, float* loss, float* running) {
    if (partial && blockIdx.x == 0 && threadIdx.x < 64) egs_label_wave_finish(n_partial, partial, inv_hw, loss, running, threadIdx.x);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (skip && *skip) return;
    float g = 0.f;
    if (radii[i] > 0) {
        g = grad_acc[(size_t)i * EGS_GRAD_STRIDE + 6];
        const uint32_t code = (uint32_t)clamped[i] >> 3;
        if (code) {
            const float* hl = hot_acc + ((size_t)(i >> 8) * EGS_HOT_PER_BLOCK + (code - 1u)) * EGS_HOT_LINE;
            for (unsigned rp = 0; rp < EGS_HOT_REPLICAS; rp++) g += hl[(size_t)rp * hot_slots * EGS_HOT_LINE + 6];
        }
    }
    if (dlabel) dlabel[i] = g;
    if (!ad.p) return;
    if (ad.active_rows && i >= *ad.active_rows) return;
    float p = ad.p[i], m = ad.m[i], v = ad.v[i];
    egs_adam1(p, g, m, v, ad.b1, ad.b2, ad.eps, ad.coef[0], ad.coef[1]);
    ad.p[i] = p; ad.m[i] = m; ad.v[i] = v;
}

}  // namespace

hipError_t egs_launch_label_bce_forward(int H, int W, const float* img, const float* mask, float* partial, float* loss, float* running, int finish, hipStream_t s) {
    const int gx = (W + EGS_TILE - 1) / EGS_TILE, n_tiles = gx * ((H + EGS_TILE - 1) / EGS_TILE);
    hipLaunchKernelGGL(k_label_bce_forward, dim3(n_tiles), dim3(256), 0, s, W, H, gx, img, mask, partial);
    if (finish) hipLaunchKernelGGL(k_label_bce_finish, dim3(1), dim3(64), 0, s, (size_t)n_tiles * 4, partial, 1.f / ((float)H * (float)W), loss, running);
    return hipGetLastError();
}
hipError_t egs_launch_label_bce_backward(int H, int W, const float* img, const float* mask, const float* gate, const float* up, float* dL_dimg,
                                         const float* fin_partial, float* fin_loss, float* fin_running, hipStream_t s) {
    const int gx = (W + EGS_TILE - 1) / EGS_TILE, n_tiles = gx * ((H + EGS_TILE - 1) / EGS_TILE);
    const EgsLabelLossK k = { img, mask, gate, up, nullptr, 1.f / ((float)H * (float)W) };
    hipLaunchKernelGGL(k_label_bce_backward, dim3(n_tiles), dim3(256), 0, s, W, H, gx, n_tiles, k, dL_dimg, fin_partial, fin_loss, fin_running);
    return hipGetLastError();
}
hipError_t egs_launch_label_finish(int P, const float* grad_acc, const uint8_t* clamped, const int32_t* radii, float* dlabel, const EgsLabelAdam* leaf,
                                   const uint32_t* skip, const float* partial, size_t n_partial, float inv_hw, float* loss, float* running, hipStream_t s) {
    if (P <= 0 && !partial) return hipSuccess;
    const EgsLabelAdam ad = leaf ? *leaf : EgsLabelAdam{};
    hipLaunchKernelGGL(k_label_finish, dim3(P > 0 ? (P + 255) / 256 : 1), dim3(256), 0, s, P, grad_acc, grad_acc + (size_t)(P > 0 ? P : 0) * EGS_GRAD_STRIDE,
                       egs_hot_slots((size_t)(P > 0 ? P : 0)), clamped, radii, dlabel, ad, skip, partial, n_partial, inv_hw, loss, running);
    return hipGetLastError();
}
