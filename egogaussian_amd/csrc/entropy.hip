// entropy.hip -- the opacity-entropy regulariser (include/egs_raster.h egs_opacity_entropy; arithmetic: opacity_entropy.h):
//   k_entropy_partial   per 256 rows: the float32 sum of h over the visible rows and their count, one line each in the scratch
//   k_entropy_finish    one workgroup: the lines in index order, in float64 -> n_vis (uint32) and value = sum / n_vis
//   k_entropy_backward  dL/dopacity [P] of weight * upstream * value, w.r.t. what the forward received (logit or activated)
// Replaces, for a trainer that does not fuse, the dozen elementwise torch launches of the reference's expression
// (/root/reference/trainers/train_static.py:97-102: index by the visibility filter, two logs, mean) and their backward; the
// rasterizer's own backward runs the first two in front of its preprocess backward, which then adds the gradient itself
// (egs_backward_entropy_lossgrad).  The reduction is deterministic, the pattern of the pose gradient (object_motion.h): six
// __shfl_xor levels inside the wave, four waves through LDS, lines added in index order in float64.  No float atomics.
#include "egs_common.h"
#include "opacity_entropy.h"

namespace {

// FROM_REC: the opacity is the activated value the forward parked in the splat record (slot [1].y) -- the very bits the blend used;
// radii <= 0 covers the rows at or beyond *active_count there (the forward culls them).  Otherwise `opac` is what the caller's forward
// received, activated here when `logit`, and rows at or beyond *active_count are skipped whatever they hold.
template <bool FROM_REC>
__global__ __launch_bounds__(256) void k_entropy_partial(int P, const float* __restrict__ opac, const float4* __restrict__ rec, int logit,
                                                         const int32_t* __restrict__ radii, const int32_t* __restrict__ active_count,
                                                         float* __restrict__ activated, float* __restrict__ line_h, uint32_t* __restrict__ line_n) {
    __shared__ float wh[4];
    __shared__ uint32_t wn[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float h = 0.f; uint32_t n = 0u;
    if (i < P) {
        const int live = (!FROM_REC && active_count) ? min(P, max(*active_count, 0)) : P;
        const bool alive = i < live;
        const bool vis = alive && radii[i] > 0;
        float o = 0.f;
        if (FROM_REC) { if (vis) o = rec[(size_t)i * EGS_SPLAT_REC_F4 + 1].y; }
        else if (alive) { const float x = opac[i]; o = logit ? egs_entropy_activate(x) : x; }
        if (!FROM_REC && activated) activated[i] = o;
        if (vis) { h = egs_entropy_h(o); n = 1u; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { h += __shfl_xor(h, d, 64); n += __shfl_xor(n, d, 64); }
    if ((threadIdx.x & 63) == 0) { wh[threadIdx.x >> 6] = h; wn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        line_h[blockIdx.x] = (wh[0] + wh[1]) + (wh[2] + wh[3]);
        line_n[blockIdx.x] = (wn[0] + wn[1]) + (wn[2] + wn[3]);
    }
}

// One workgroup of one wave.  Lane c adds one contiguous span of the lines in index order, in float64; lane 0 then adds the 64 span
// sums in order: the grouping is fixed by the line count alone.  No visible row: n_vis = 0, value = NaN (torch's mean() of an empty tensor).
#define EGS_ENT_SPANS 64
__global__ __launch_bounds__(EGS_ENT_SPANS) void k_entropy_finish(const float* __restrict__ line_h, const uint32_t* __restrict__ line_n, int lines,
                                                                  uint32_t* __restrict__ n_vis, float* __restrict__ value) {
    __shared__ double sh[EGS_ENT_SPANS];
    __shared__ uint32_t sn[EGS_ENT_SPANS];
    const int c = (int)threadIdx.x, per = (lines + EGS_ENT_SPANS - 1) / EGS_ENT_SPANS;
    const int b0 = min(lines, c * per), b1 = min(lines, b0 + per);
    double t = 0.0; uint32_t n = 0u;
    for (int b = b0; b < b1; b++) { t += (double)line_h[b]; n += line_n[b]; }
    sh[c] = t; sn[c] = n;
    __syncthreads();
    if (c == 0) {
        double T = 0.0; uint32_t N = 0u;
        for (int j = 0; j < EGS_ENT_SPANS; j++) { T += sh[j]; N += sn[j]; }
        *n_vis = N;
        if (value) *value = (float)(T / (double)N);
    }
}

__global__ __launch_bounds__(256) void k_entropy_backward(int P, const float* __restrict__ opac, int logit, const int32_t* __restrict__ radii,
                                                          const int32_t* __restrict__ active_count, EgsEntropy ent, float* __restrict__ dopac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int live = active_count ? min(P, max(*active_count, 0)) : P;
    float g = 0.f;
    if (i < live && radii[i] > 0) {
        const float x = opac[i];
        const float o = logit ? egs_entropy_activate(x) : x;
        g = egs_entropy_grad(egs_entropy_coef(ent.n_vis, ent.weight, ent.upstream), o);
        if (logit) g = g * (o * (1.f - o));                          // the sigmoid chain of k_preprocess_backward
    }
    dopac[i] = g;
}

}  // namespace

// The reduction of the frame a rasterizer forward left in `rec` / `radii` (rec != nullptr), or of a caller's opacities.
hipError_t egs_launch_entropy_reduce(int P, const float* opac, const float4* rec, int logit, const int32_t* radii, const int32_t* active_count,
                                     float* activated, void* scratch, uint32_t* n_vis, float* value, hipStream_t s) {
    const int lines = (int)egs_entropy_lines(P);
    float* line_h = (float*)scratch; uint32_t* line_n = (uint32_t*)scratch + lines;
    if (lines > 0) {
        if (rec) hipLaunchKernelGGL(k_entropy_partial<true>, dim3(lines), dim3(256), 0, s, P, opac, rec, logit, radii, active_count, activated, line_h, line_n);
        else hipLaunchKernelGGL(k_entropy_partial<false>, dim3(lines), dim3(256), 0, s, P, opac, rec, logit, radii, active_count, activated, line_h, line_n);
    }
    hipLaunchKernelGGL(k_entropy_finish, dim3(1), dim3(EGS_ENT_SPANS), 0, s, line_h, line_n, lines, n_vis, value);
    return hipGetLastError();
}

extern "C" {

size_t egs_opacity_entropy_scratch_bytes(int P) { return egs_align(egs_entropy_lines(P) * (sizeof(float) + sizeof(uint32_t))); }

int egs_opacity_entropy_forward(int P, const float* opacity, int activation_flags, const int32_t* radii, const int32_t* active_count,
                                float* activated, const egs_opacity_entropy* ent, void* stream) {
    if (P < 0 || !ent || !ent->n_vis || (activation_flags & ~EGS_ACT_LOGIT_OPACITY)) return EGS_ERR_ARG;
    if (P > 0 && (!opacity || !radii || !ent->scratch)) return EGS_ERR_ARG;
    return (int)egs_launch_entropy_reduce(P, opacity, nullptr, (activation_flags & EGS_ACT_LOGIT_OPACITY) ? 1 : 0, radii, active_count, activated,
                                          ent->scratch, ent->n_vis, ent->value, (hipStream_t)stream);
}

int egs_opacity_entropy_backward(int P, const float* opacity, int activation_flags, const int32_t* radii, const int32_t* active_count,
                                 const egs_opacity_entropy* ent, float* dL_dopacity, void* stream) {
    if (P < 0 || !ent || !ent->n_vis || !ent->weight || (activation_flags & ~EGS_ACT_LOGIT_OPACITY)) return EGS_ERR_ARG;
    if (P == 0) return 0;
    if (!opacity || !radii || !dL_dopacity) return EGS_ERR_ARG;
    const EgsEntropy k = { ent->n_vis, ent->weight, ent->upstream };
    hipLaunchKernelGGL(k_entropy_backward, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, opacity,
                       (activation_flags & EGS_ACT_LOGIT_OPACITY) ? 1 : 0, radii, active_count, k, dL_dopacity);
    return (int)hipGetLastError();
}

}  // extern "C"
