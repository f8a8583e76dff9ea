// preprocess.hip -- per-Gaussian stages of the rasterizer for gfx950:
//   k_preprocess           3D->2D projection, EWA covariance, conic, radius, tile rect, SH->RGB
//   k_preprocess_backward  conic/mean2D/colour/depth gradients -> mean3D, cov3D, SH, scale, quaternion
//   k_mark_visible         near-plane test
// The colour of a single SH coefficient (M = 1) is evaluated inline here through sh_basis.h; harmonics with more coefficients, or given as
// DC / rest arrays, run as launches of their own (sh.hip, egs_sh_apart).
// Replaces the per-Gaussian stages of the upstream op called from
// /root/reference/gaussian_renderer/__init__.py:90-98.
//
// One lane per Gaussian; a wave reads 64 consecutive xyz / cov6 / SH rows, i.e. contiguous 768 B /
// 1.5 KB / 768 B spans, so the array-of-rows inputs coalesce without staging.  The forward result is
// packed into one 48-byte record per Gaussian (egs_common.h) so the blend kernels gather three
// dwordx4 per splat instead of touching five arrays.
//
// This translation unit is compiled with -ffp-contract=off and every expression follows the order of
// oracle/raster_oracle.c, so radii, tile rectangles and depth bits are bit-identical to the oracle.
#include "egs_common.h"
#include <stdlib.h>
#include "bin_walk.h"              // the count pass of the tile bucketing, carried by k_preprocess_count
#include "backward_prologue.h"
#include "object_motion.h"          // the rigid object motion of the positions (EGS_ACT_OBJECT_MOTION)
#include "opacity_entropy.h"        // the opacity-entropy term joins dL/dopacity in k_preprocess_backward<.., ENT = true>
#include "sh_basis.h"               // colour of the inline M = 1 harmonics, forward and backward
#include "splat_geom.h"             // transforms, covariance chain (shared with cov3d.hip) and EWA projection
#include <type_traits>

namespace {

// What both forward kernels are given: the scene, the camera, and the arrays the projection writes.
struct EgsPreArgs {
    int P, D, M; const float* means3D; const float* shs; const float* colors; const float* opac; const float* scales; float mod;
    const float* rots; const float* cov3D_in; int act; const float* V; const float* PM; const float* campos; int W, H; float tanfovx, tanfovy;
    int32_t* radii; float4* rec; uint2* rect_out; uint32_t* tiles_touched; uint8_t* clamped_out; uint8_t* visible;
    uint32_t* block_sums; uint32_t* block_hot; const int32_t* active_count;
};
struct PreOut { uint2 rect; float4 r0, r1, r2; };
// Returns the number of tiles the Gaussian touches (0 = culled).
// MOTION: a moved row is placed first, p <- A p + b (object_motion.h), and everything below sees the placed position.
template <bool MOTION>
__device__ __forceinline__ uint32_t preprocess_one(
    int i, int D, int M, const float* __restrict__ means3D, const float* __restrict__ shs,
    const float* __restrict__ colors, const float* __restrict__ opac, const float* __restrict__ scales, float mod,
    const float* __restrict__ rots, const float* __restrict__ cov3D_in, int act, const float* __restrict__ V,
    const float* __restrict__ PM, const float* __restrict__ campos, int W, int H, float tanfovx, float tanfovy,
    int32_t* __restrict__ radii, float4* __restrict__ rec, uint2* __restrict__ rect_out,
    uint32_t* __restrict__ tiles_touched, uint8_t* __restrict__ clamped_out, uint8_t* __restrict__ visible, const EgsObjRot rot,
    const EgsMotion mot, bool& hot, PreOut* out = nullptr /*the rectangle and the record as written (left alone when culled, i.e. on a zero return): k_preprocess_count walks them*/) {
    const int gx = (W + EGS_TILE - 1) / EGS_TILE, gy = (H + EGS_TILE - 1) / EGS_TILE;
    radii[i] = 0; tiles_touched[i] = 0; visible[i] = 0;

    float p[3] = { means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2] };
    if constexpr (MOTION) {
        if (!mot.moved || mot.moved[i]) { const float p0[3] = { p[0], p[1], p[2] }; egs_motion_point(mot.A, p0, p); }   // (i < live: the caller's test)
    }
    float c6[6];
    if (cov3D_in) {
#pragma unroll
        for (int k = 0; k < 6; k++) c6[k] = cov3D_in[6 * (size_t)i + k];
    } else {
        float s[3] = { scales[3 * i], scales[3 * i + 1], scales[3 * i + 2] };
        float q[4] = { rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3] };
        float qinv; activate_scale_rot(act & EGS_ACT_LOG_SCALES, act & EGS_ACT_RAW_QUATS, s, q, qinv);
        // the object rotation of the `fine_all` call shape: L <- M L, the text k_cov3d_forward runs (splat_geom.h)
        CovFactor f; cov_factor(s, mod, q, rot.M && (!rot.sel || rot.sel[i]), rot.M, f);
        cov_from_factor(f.L, c6);
    }
    Ewa e; ewa_project(p, c6, V, W, H, tanfovx, tanfovy, e);
    if (e.t[2] <= 0.2f) return 0u;                              // near-plane cull
    float hom[4]; xform44(p, PM, hom);
    const float pw = 1.f / (hom[3] + 0.0000001f);
    const float ndc_x = hom[0] * pw, ndc_y = hom[1] * pw;

    const float det = e.a * e.c - e.b * e.b;
    if (det == 0.f) return 0u;
    const float det_inv = 1.f / det;
    const float conA = e.c * det_inv, conB = -e.b * det_inv, conC = e.a * det_inv;
    const float mid = 0.5f * (e.a + e.c);
    const float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
    const float lam1 = mid + disc, lam2 = mid - disc;
    const int rad = (int)ceilf(3.f * sqrtf(fmaxf(lam1, lam2)));
    const float px = ((ndc_x + 1.f) * (float)W - 1.f) * 0.5f;
    const float py = ((ndc_y + 1.f) * (float)H - 1.f) * 0.5f;
    const int rx0 = min(gx, max(0, (int)((px - (float)rad) / (float)EGS_TILE)));
    const int ry0 = min(gy, max(0, (int)((py - (float)rad) / (float)EGS_TILE)));
    const int rx1 = min(gx, max(0, (int)((px + (float)rad + (float)(EGS_TILE - 1)) / (float)EGS_TILE)));
    const int ry1 = min(gy, max(0, (int)((py + (float)rad + (float)(EGS_TILE - 1)) / (float)EGS_TILE)));
    if ((rx1 - rx0) * (ry1 - ry0) == 0) return 0u;

    float rgb[3]; uint32_t cl = 0;
    if (colors) {
        // EGS_ACT_SCALAR_COLOR: one value per Gaussian fills the three slots -- no [P,3] copy of the label exists.  A branch on the uniform flag: the
        // strided form (colors[cs * i + k * ck]) moved the register allocation of every instantiation (profiles/label_phase_resources.txt)
        if (act & EGS_ACT_SCALAR_COLOR) rgb[0] = rgb[1] = rgb[2] = colors[i];
        else { rgb[0] = colors[3 * i]; rgb[1] = colors[3 * i + 1]; rgb[2] = colors[3 * i + 2]; }
    } else if (!shs) {
        rgb[0] = rgb[1] = rgb[2] = 0.f;                            // k_sh_forward fills the colour (and the clamp flags) in afterwards
    } else {
        float x, y, z, inv; sh_view_dir(p, campos, x, y, z, inv);
        cl = sh_colour(D, shs + (size_t)i * M * 3, x, y, z, rgb);
    }
    const float o = (act & EGS_ACT_LOGIT_OPACITY) ? 1.f / (1.f + expf(-opac[i])) : opac[i];

    // Conservative pixel bounding box of {alpha >= 1/255}: the ellipse 0.5 d^T Q d <= tau with
    // tau = ln(255 o).  Not part of the published algorithm -- it only lets the blend kernels skip
    // (8x8 pixel block, splat) pairs that provably contribute nothing, so results are unchanged.
    uint32_t bbx = 1u, bby = 1u;                                   // x0 = 1 > x1 = 0: empty
    {
        const float lo = 255.f * o;
        if (!(lo < 0.999f)) {
            const float tau2 = 2.f * (logf(fmaxf(lo, 1.f)) + 0.01f);
            const float detq = conA * conC - conB * conB;
            float ex = 1e9f, ey = 1e9f;
            if (detq > 0.f && conA * conC < 1e4f * detq) {
                ex = fmaxf(sqrtf(tau2 * conC / detq), sqrtf(tau2 * e.a)) * 1.002f + 0.01f;
                ey = fmaxf(sqrtf(tau2 * conA / detq), sqrtf(tau2 * e.c)) * 1.002f + 0.01f;
            }
            const float fx0 = fmaxf(floorf(px - ex), 0.f), fx1 = fminf(ceilf(px + ex), (float)(W - 1));
            const float fy0 = fmaxf(floorf(py - ey), 0.f), fy1 = fminf(ceilf(py + ey), (float)(H - 1));
            if (fx0 <= fx1 && fy0 <= fy1) {
                bbx = (uint32_t)fx0 | ((uint32_t)fx1 << 16);
                bby = (uint32_t)fy0 | ((uint32_t)fy1 << 16);
                // a box over this many tiles: its accumulator line would be hit by every quadrant-wave of all of them (egs_common.h)
                hot = (((uint32_t)fx1 >> 4) - ((uint32_t)fx0 >> 4) + 1u) * (((uint32_t)fy1 >> 4) - ((uint32_t)fy0 >> 4) + 1u) >= EGS_HOT_MIN_TILES;
            } else if (!(ex == ex) || !(ey == ey) || !(px == px) || !(py == py)) {   // NaN: never cull
                bbx = 0u | ((uint32_t)(W - 1) << 16); bby = 0u | ((uint32_t)(H - 1) << 16);
            }
        }
    }

    radii[i] = rad; visible[i] = 1;                                  // radii > 0 as one byte (a torch.bool view for the caller)
    tiles_touched[i] = (uint32_t)((rx1 - rx0) * (ry1 - ry0));
    rect_out[i] = make_uint2((uint32_t)rx0 | ((uint32_t)rx1 << 16), (uint32_t)ry0 | ((uint32_t)ry1 << 16));
    clamped_out[i] = (uint8_t)cl;
    float4* r = rec + (size_t)i * EGS_SPLAT_REC_F4;
    const float4 q0 = make_float4(px, py, (-0.5f * EGS_LOG2E) * conA, -EGS_LOG2E * conB);
    const float4 q1 = make_float4((-0.5f * EGS_LOG2E) * conC, o, rgb[0], rgb[1]);
    const float4 q2 = make_float4(rgb[2], e.t[2], __uint_as_float(bbx), __uint_as_float(bby));
    r[0] = q0; r[1] = q1; r[2] = q2;
    if (out) { out->rect = make_uint2((uint32_t)rx0 | ((uint32_t)rx1 << 16), (uint32_t)ry0 | ((uint32_t)ry1 << 16)); out->r0 = q0; out->r1 = q1; out->r2 = q2; }
    return (uint32_t)((rx1 - rx0) * (ry1 - ry0));
}

// The tail of a 256-Gaussian block in both forward kernels, in two halves around the caller's barrier.  Before it: a wave's instance count and
// hot count go to wsum / whot.  After it: the block's first wave w0 (0 in k_preprocess, w & ~3 in k_preprocess_count) writes the per-block
// instance count -- the host adds the block sums to get R (no contended atomic, deterministic) -- and the hot count; a hot Gaussian takes its
// rank among the block's hot ones -> the code that names its replica lines (egs_common.h; few per frame).
__device__ __forceinline__ void pp_tail_publish(uint32_t my_tiles, uint64_t hot_wave, unsigned w, unsigned lane, uint32_t* wsum, uint32_t* whot) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) my_tiles += (uint32_t)__shfl_xor((int)my_tiles, d, 64);
    if (lane == 0) { wsum[w] = my_tiles; whot[w] = (uint32_t)__popcll(hot_wave); }
}
__device__ __forceinline__ void pp_tail_finish(const uint32_t* wsum, const uint32_t* whot, unsigned w0, unsigned w, unsigned lane, bool first, unsigned blk, int i, bool hot,
                                               uint64_t hot_wave, float4* __restrict__ rec, uint8_t* __restrict__ clamped_out,
                                               uint32_t* __restrict__ block_sums, uint32_t* __restrict__ block_hot) {
    if (first) {
        block_sums[blk] = wsum[w0] + wsum[w0 + 1] + wsum[w0 + 2] + wsum[w0 + 3];
        block_hot[blk] = min(whot[w0] + whot[w0 + 1] + whot[w0 + 2] + whot[w0 + 3], EGS_HOT_PER_BLOCK);
    }
    if (hot) {
        uint32_t rank = (uint32_t)__popcll(hot_wave & (lane ? (~0ull >> (64 - lane)) : 0ull));
        for (unsigned k = w0; k < w; k++) rank += whot[k];
        if (rank < EGS_HOT_PER_BLOCK) {
            float4* r2 = rec + (size_t)i * EGS_SPLAT_REC_F4 + 2;
            uint32_t bbx = __float_as_uint(r2->z), bby = __float_as_uint(r2->w);
            egs_hot_code_set(bbx, bby, rank + 1u);
            r2->z = __uint_as_float(bbx); r2->w = __uint_as_float(bby);
            clamped_out[i] = (uint8_t)((clamped_out[i] & EGS_CLAMP_MASK) | ((rank + 1u) << 3));   // where the backward looks for it
        }
    }
}

// PLACE: the first eight workgroups do not preprocess anything -- each orders one XCD band of the forward blend's tiles by the
// costs the image buffer holds (backward_prologue.h), a job that needs doing before that blend and fits under this launch.
template <bool PLACE, bool MOTION>
__global__ __launch_bounds__(256) void k_preprocess(EgsPreArgs a, uint32_t* __restrict__ zero_words, size_t zero_n, EgsPrologueArgs place, EgsObjRot rot, EgsMotion mot) {
    __shared__ uint32_t wsum[4], whot[4];
    if (PLACE) {
        __shared__ EgsOrderLds order_lds;
        if (blockIdx.x < EGS_XCDS) { egs_order_band<256>(place, (int)blockIdx.x, order_lds); return; }
    }
    const unsigned bid = blockIdx.x - (PLACE ? EGS_XCDS : 0u), nblk = gridDim.x - (PLACE ? EGS_XCDS : 0u);
    const int i = (int)(bid * blockDim.x + threadIdx.x);
    for (size_t z = (size_t)i; z < zero_n; z += (size_t)nblk * blockDim.x) zero_words[z] = 0u;   // on the side (egs_common.h)
    uint32_t my_tiles = 0;
    // capacity-sized models (include/egs_raster.h): rows at and beyond the device-side live count are culled whatever they hold
    const int P = a.P, live = a.active_count ? min(P, max(*a.active_count, 0)) : P;
    if (i >= live && i < P) { a.radii[i] = 0; a.tiles_touched[i] = 0; a.visible[i] = 0; }
    bool hot = false;
    if (i < live) my_tiles = preprocess_one<MOTION>(i, a.D, a.M, a.means3D, a.shs, a.colors, a.opac, a.scales, a.mod, a.rots, a.cov3D_in, a.act, a.V, a.PM, a.campos,
                                                     a.W, a.H, a.tanfovx, a.tanfovy, a.radii, a.rec, a.rect_out, a.tiles_touched, a.clamped_out, a.visible, rot, mot, hot);
    hot = hot && my_tiles != 0;
    const uint64_t hot_wave = __ballot(hot);
    pp_tail_publish(my_tiles, hot_wave, threadIdx.x >> 6, threadIdx.x & 63, wsum, whot);
    __syncthreads();
    pp_tail_finish(wsum, whot, 0u, threadIdx.x >> 6, threadIdx.x & 63, threadIdx.x == 0, bid, i, hot, hot_wave, a.rec, a.clamped_out, a.block_sums, a.block_hot);
}

// k_preprocess and the COUNT pass of the tile bucketing (binning.hip k_bin_count) in one launch.  The count pass's workgroup is a chain
// of latencies -- launch, set-up loads (~4 us with every workgroup asking at once), walk, flush -- of which the first two only fetch
// what k_preprocess had in registers a launch earlier (profiles/r5_bucketing_experiments.md); here wave w of a 16-wave workgroup
// projects one 64-Gaussian group of the round and parks rectangle, box and conic in the walk's LDS block directly.  The walk, the
// [tile][workgroup] table and the chunk sums are bin_walk.h's, so the lists stay what k_bin_scatter + k_tile_sort made of them before.
// Blocks of 256 Gaussians are dealt to workgroups (bin_walk.h): the per-block instance and hot counts are those of k_preprocess
// (block B = Gaussians 256 B .. 256 B + 255; waves 4 m .. 4 m + 3 of a round hold one block).  Needs gpr % 4 == 0 (egs_can_fuse_count).
// PLACE: the first eight workgroups order the forward blend's tiles instead (as in k_preprocess), in the dynamic LDS block.
struct EgsCountArgs { int gpr, gx, n_tiles; uint32_t nblocks; int cull, use_map; uint32_t* table; uint32_t stride; uint32_t* chunk_sum; };
extern __shared__ __attribute__((aligned(16))) uint32_t pc_dyn_lds[];
// ONE_ROUND: every workgroup's groups fit one round (no loop: what the projection loads is dead before the walk starts -- inside a loop the
// camera matrices and the argument pointers stayed live through it and the kernel needed 105 VGPRs; 64 keep the 16-wave workgroups two per CU).
template <bool PLACE, bool ONE_ROUND, bool MOTION>
__global__ __launch_bounds__(EGS_BIN_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_preprocess_count(EgsPreArgs a, EgsCountArgs c, EgsPrologueArgs place, EgsObjRot rot, EgsMotion mot) {
    __shared__ uint32_t wsum[EGS_BIN_WAVES], whot[EGS_BIN_WAVES];
    if (PLACE) {
        if (blockIdx.x < EGS_XCDS) { egs_order_band<EGS_BIN_THREADS>(place, (int)blockIdx.x, *reinterpret_cast<EgsOrderLds*>(pc_dyn_lds)); return; }
    }
    const unsigned bid = bin_logical_block(c.nblocks, PLACE ? EGS_XCDS : 0u);
    if (bid >= c.nblocks) return;
    uint32_t* hist = pc_dyn_lds;
    const BinRound L = bin_round_carve(pc_dyn_lds + ((c.n_tiles + 3) & ~3), c.gpr, c.cull != 0);
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < c.n_tiles; t += EGS_BIN_THREADS) hist[t] = 0;            // (the first round's barrier orders this)
    const int P = a.P;
    const int live = a.active_count ? min(P, max(*a.active_count, 0)) : P;                  // capacity-sized models: rows beyond the live count are culled
    const unsigned groups = ((unsigned)P + 63u) / 64u, per_block = bin_groups_per_block((unsigned)P, c.nblocks);
    unsigned g0 = 0;
    do {
        if (!ONE_ROUND && g0) __syncthreads();                         // the previous round's readers (walk, block sums, hot ranks) are done
        bool hot = false; uint64_t hot_wave = 0ull; int i = -1;
        if ((int)w < c.gpr) {
            const unsigned j = bin_group_of(bid, c.nblocks, g0 + w);
            const bool have = g0 + w < per_block && j < groups;
            i = have ? (int)(j * 64u + lane) : -1;
            uint32_t my_tiles = 0; PreOut o;
            if (i >= live && i < P) { a.radii[i] = 0; a.tiles_touched[i] = 0; a.visible[i] = 0; }
            const float* V = a.V; const float* PM = a.PM; const float* campos = a.campos;
            if (!ONE_ROUND) asm volatile("" : "+s"(V), "+s"(PM), "+s"(campos));     // (re-read every round instead of held in 35 scalar registers through the walk)
            if (i >= 0 && i < live)
                my_tiles = preprocess_one<MOTION>(i, a.D, a.M, a.means3D, a.shs, a.colors, a.opac, a.scales, a.mod, a.rots, a.cov3D_in, a.act, V, PM, campos,
                                          a.W, a.H, a.tanfovx, a.tanfovy, a.radii, a.rec, a.rect_out, a.tiles_touched, a.clamped_out, a.visible, rot, mot, hot, &o);
            hot = hot && my_tiles != 0;
            hot_wave = __ballot(hot);
            if (my_tiles == 0) { o.rect = make_uint2(0u, 0u); o.r0 = o.r1 = o.r2 = make_float4(0.f, 0.f, 0.f, 0.f); }      // (culled: preprocess_one left `o` alone)
            bin_park_group(L, w, lane, i >= 0 && i < P, my_tiles, o.rect, o.r0, o.r1, o.r2, false, c.cull != 0, c.use_map != 0);
            pp_tail_publish(my_tiles, hot_wave, w, lane, wsum, whot);
        }
        __syncthreads();
        // the 256-Gaussian block of this wave: waves (w & ~3) .. (w & ~3) + 3 of the round (all present: gpr is a multiple of four)
        if ((int)w < c.gpr && i >= 0) pp_tail_finish(wsum, whot, w & ~3u, w, lane, (w & 3u) == 0 && lane == 0, (unsigned)i >> 8, i, hot, hot_wave, a.rec, a.clamped_out, a.block_sums, a.block_hot);
        bin_walk_round(L, bid, c.nblocks, g0, c.gpr, c.gx, false, c.cull != 0, c.use_map != 0, a.W, a.H,
                       [&](uint32_t tile, uint32_t, uint32_t) { atomicAdd(&hist[tile], 1u); });
        g0 += (unsigned)c.gpr;
    } while (!ONE_ROUND && g0 < per_block);
    __syncthreads();
    bin_flush_counts(hist, c.n_tiles, bid, c.stride, c.table, c.chunk_sum, blockIdx.x);
}

// stage offsets (floats) of the leaves a fused optimizer owns: rows of the workgroup's 256 Gaussians, leaf after leaf
#define ST_MEANS 0
#define ST_OPAC 768
#define ST_SCALES 1024
#define ST_ROTS 1792
#define ST_SH 2816
// MOT (object motion, object_motion.h): 0 none; 1 the row is placed, its gradient stays dL/dp' (the spherical-harmonics launch finishes it);
// 2 the gradient is finished here: dL/dp = A^T dL/dp', the row's pose terms go to red[0..12).  MOT != 0: a rotated row's dL/dM terms go to red[12..21).
// ENT (opacity_entropy.h): a visible row's share of the opacity-entropy term, ent_coef * dh/do, joins dL/dopacity before the sigmoid chain, the
// dopac store and the stage of the sink -- the Adam step inside the kernel sees the whole gradient of the logit.
template <bool SINK, int MOT, bool ENT = false>
__device__ __forceinline__ void pp_bwd_one(
    const int i, int D, int M, const float* __restrict__ means3D, const float* __restrict__ shs,
    const float* __restrict__ scales, float mod, const float* __restrict__ rots, const float* __restrict__ cov3D_in, int act,
    const float* __restrict__ V, const float* __restrict__ PM, const float* __restrict__ campos, int W, int H,
    float tanfovx, float tanfovy, const int32_t* __restrict__ radii, const uint8_t* __restrict__ clamped,
    const float4* __restrict__ rec, const float* __restrict__ grad_acc, const float* __restrict__ hot_acc, const size_t hot_slots, float* __restrict__ dmeans2D, float* __restrict__ dcolors,
    float* __restrict__ dopac, float* __restrict__ dmeans3D, float* __restrict__ dcov3D, float* __restrict__ dsh,
    float* __restrict__ dscales, float* __restrict__ drots,
    float* __restrict__ stat_grad_accum, float* __restrict__ stat_denom, float* __restrict__ stat_max_radii,
    const uint32_t* __restrict__ skip_flag, float* __restrict__ stage, const unsigned fused, const EgsObjRot rot, const EgsMotion mot, float* red,
    [[maybe_unused]] const float ent_coef = 0.f) {
    // SINK: the gradients of the leaves in `fused` (bit = EGS_SINK_*) also go to `stage` (LDS), from where the workgroup applies
    // Adam to its 256 rows; their dX arrays may then be NULL (nothing written)
    const unsigned tid = threadIdx.x;
    const bool vis = radii[i] > 0;
    float acc[12];                                                    // slots 0..9 (+ two spare) of the 64-byte line: three of its four float4
    {
        const float4* ga = reinterpret_cast<const float4*>(grad_acc + (size_t)i * EGS_GRAD_STRIDE);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float4 v = vis ? ga[k] : make_float4(0.f, 0.f, 0.f, 0.f);
            acc[4 * k] = v.x; acc[4 * k + 1] = v.y; acc[4 * k + 2] = v.z; acc[4 * k + 3] = v.w;
        }
    }
    // acc[0..4] are moments of gd = dL/dalpha * G (egs_common.h); with the opacity o and the conic (A, B, C) of this Gaussian
    //   dL/dmean2D = -o (A Sx + B Sy, C Sy + B Sx)   and   dL/dconic = -0.5 o (Sxx, Sxy, Syy)  (xy slot: half the derivative)
    // The published op reports dL/dmean2D in NDC units (x 0.5 W, 0.5 H).
    float gmx = 0.f, gmy = 0.f;
    if (vis) {
        const float4* r = rec + (size_t)i * EGS_SPLAT_REC_F4;
        const float4 r0 = r[0], r1 = r[1];
        const uint32_t code = (uint32_t)clamped[i] >> 3;
        if (code) {   // a hot Gaussian: the blend spread its sums over EGS_HOT_REPLICAS lines behind the regular ones (egs_common.h)
            const float* hl = hot_acc + ((size_t)(i >> 8) * EGS_HOT_PER_BLOCK + (code - 1u)) * EGS_HOT_LINE;
            for (unsigned rp = 0; rp < EGS_HOT_REPLICAS; rp++) {
                const float4* ga = reinterpret_cast<const float4*>(hl + (size_t)rp * hot_slots * EGS_HOT_LINE);
#pragma unroll
                for (int k = 0; k < 3; k++) { const float4 v = ga[k]; acc[4 * k] += v.x; acc[4 * k + 1] += v.y; acc[4 * k + 2] += v.z; acc[4 * k + 3] += v.w; }
            }
        }
        const float cA = r0.z * (-2.f * EGS_LN2), cB = r0.w * (-EGS_LN2), cC = r1.x * (-2.f * EGS_LN2);
        const float o = r1.y;
        gmx = -o * (cA * acc[0] + cB * acc[1]); gmy = -o * (cC * acc[1] + cB * acc[0]);
        acc[2] *= -0.5f * o; acc[3] *= -0.5f * o; acc[4] *= -0.5f * o;
    }
    acc[0] = gmx * (0.5f * (float)W); acc[1] = gmy * (0.5f * (float)H);
    dmeans2D[3 * i] = acc[0]; dmeans2D[3 * i + 1] = acc[1]; dmeans2D[3 * i + 2] = 0.f;
    if (stat_grad_accum && vis && !(skip_flag && *skip_flag)) {       // (skip_flag: this frame overflowed its instance capacity)
        // the trainer's per-iteration densification statistics, where their inputs are produced
        // (/root/reference/scene/gaussian_model.py:735-737 add_densification_stats, trainers/train_static.py:125 max_radii2D)
        stat_grad_accum[i] += sqrtf(acc[0] * acc[0] + acc[1] * acc[1]);
        stat_denom[i] += 1.f;
        if (stat_max_radii) stat_max_radii[i] = fmaxf(stat_max_radii[i], (float)radii[i]);
    }
    if (dcolors) { dcolors[3 * i] = acc[6]; dcolors[3 * i + 1] = acc[7]; dcolors[3 * i + 2] = acc[8]; }
    {   // logit opacities: chain through the sigmoid with the activated value the forward parked in the record
        const float o = rec[(size_t)i * EGS_SPLAT_REC_F4 + 1].y;
        if constexpr (ENT) { if (vis) acc[5] += egs_entropy_grad(ent_coef, o); }
        const float go = (vis && (act & EGS_ACT_LOGIT_OPACITY)) ? acc[5] * (o * (1.f - o)) : acc[5];
        if (dopac) dopac[i] = go;
        if (SINK && (fused & (1u << EGS_SINK_OPACITY))) stage[ST_OPAC + tid] = go;
    }
    float gmean[3] = { 0.f, 0.f, 0.f }, g6[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (!vis) {
#pragma unroll
        for (int k = 0; k < 3; k++) if (dmeans3D) dmeans3D[3 * i + k] = 0.f;
#pragma unroll
        for (int k = 0; k < 6; k++) if (dcov3D) dcov3D[6 * (size_t)i + k] = 0.f;
        if (dsh) for (int k = 0; k < M * 3; k++) dsh[(size_t)i * M * 3 + k] = 0.f;
        if (dscales) { dscales[3 * i] = 0.f; dscales[3 * i + 1] = 0.f; dscales[3 * i + 2] = 0.f; }
        if (drots) { drots[4 * i] = 0.f; drots[4 * i + 1] = 0.f; drots[4 * i + 2] = 0.f; drots[4 * i + 3] = 0.f; }
        if (SINK) {                                                   // a culled Gaussian still takes its Adam step, with a zero gradient
#pragma unroll
            for (int k = 0; k < 3; k++) { stage[ST_MEANS + 3 * tid + k] = 0.f; stage[ST_SCALES + 3 * tid + k] = 0.f; stage[ST_SH + 3 * tid + k] = 0.f; }
            *reinterpret_cast<float4*>(stage + ST_ROTS + 4 * tid) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    float p[3] = { means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2] };
    [[maybe_unused]] const float p0[3] = { p[0], p[1], p[2] };       // the canonical position (pose terms)
    if constexpr (MOT != 0) {
        if (!mot.moved || mot.moved[i]) egs_motion_point(mot.A, p0, p);       // (visible: a live row)
    }
    float c6[6], s[3] = { 0.f, 0.f, 0.f }, q[4] = { 1.f, 0.f, 0.f, 0.f }, qinv = 1.f;
    if (cov3D_in) {
#pragma unroll
        for (int k = 0; k < 6; k++) c6[k] = cov3D_in[6 * (size_t)i + k];
    } else {
        s[0] = scales[3 * i]; s[1] = scales[3 * i + 1]; s[2] = scales[3 * i + 2];
        q[0] = rots[4 * i]; q[1] = rots[4 * i + 1]; q[2] = rots[4 * i + 2]; q[3] = rots[4 * i + 3];
        activate_scale_rot(act & EGS_ACT_LOG_SCALES, act & EGS_ACT_RAW_QUATS, s, q, qinv);
        CovFactor f; cov_factor(s, mod, q, rot.M && (!rot.sel || rot.sel[i]), rot.M, f);
        cov_from_factor(f.L, c6);
    }
    Ewa e; ewa_project(p, c6, V, W, H, tanfovx, tanfovy, e);

    // conic (xx, xy/2, yy) -> cov2D (a,b,c); the published backward regularises 1/det^2 by 1e-7.
    // These three lines are dL/dcov2D = -cov2D^-1 (dL/dconic) cov2D^-1 written out, and the lines after them multiply the result by the
    // covariance again (gm0 = 2 S0 dL_da + S1 dL_db ...): the product only cancels back to "cov2D^-1 x gradient" if the three numbers keep
    // that structure.  In float32 they do not for an elongated splat (a c within 2 % of b^2: every term below is ~60 x the sum, the rounding
    // of each lands in the next lines' cancellation once more) -- dL/dmeans3D of the one recorded parity miss was 7e-4 of the array's
    // maximum off with EXACT blend sums, float32 oracle included (tools/dev/chain_precision.py).  Evaluated in float64 from the same float32
    // (a, b, c) they are the exact formula of a covariance 1e-7 away, and the row lands 2e-6 from the float64 oracle.  ~25 double
    // operations per Gaussian in a kernel that streams 300 B per Gaussian.
    const double gA = (double)acc[2], gB = (double)acc[3], gC = (double)acc[4];
    const double ea = (double)e.a, eb = (double)e.b, ec = (double)e.c;
    const double denom = ea * ec - eb * eb;
    const double d2inv = 1.0 / (denom * denom + 0.0000001);
    float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
    if (d2inv != 0.0) {
        dL_da = (float)(d2inv * (-ec * ec * gA + 2.0 * eb * ec * gB + (denom - ea * ec) * gC));
        dL_dc = (float)(d2inv * (-ea * ea * gC + 2.0 * ea * eb * gB + (denom - ea * ec) * gA));
        dL_db = (float)(d2inv * 2.0 * (eb * ec * gA - (denom + 2.0 * eb * eb) * gB + ea * eb * gC));
        const float* m0 = e.m0; const float* m1 = e.m1;
        g6[0] = m0[0] * m0[0] * dL_da + m0[0] * m1[0] * dL_db + m1[0] * m1[0] * dL_dc;
        g6[3] = m0[1] * m0[1] * dL_da + m0[1] * m1[1] * dL_db + m1[1] * m1[1] * dL_dc;
        g6[5] = m0[2] * m0[2] * dL_da + m0[2] * m1[2] * dL_db + m1[2] * m1[2] * dL_dc;
        g6[1] = 2.f * m0[0] * m0[1] * dL_da + (m0[0] * m1[1] + m0[1] * m1[0]) * dL_db + 2.f * m1[0] * m1[1] * dL_dc;
        g6[2] = 2.f * m0[0] * m0[2] * dL_da + (m0[0] * m1[2] + m0[2] * m1[0]) * dL_db + 2.f * m1[0] * m1[2] * dL_dc;
        g6[4] = 2.f * m0[2] * m0[1] * dL_da + (m0[1] * m1[2] + m0[2] * m1[1]) * dL_db + 2.f * m1[1] * m1[2] * dL_dc;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) if (dcov3D) dcov3D[6 * (size_t)i + k] = g6[k];     // NULL: only the scale / rotation gradients are wanted

    // cov2D -> rows of (J R) -> J -> camera-space point -> mean
    float gJ00 = 0.f, gJ02 = 0.f, gJ11 = 0.f, gJ12 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float gm0 = 2.f * e.S0[k] * dL_da + e.S1[k] * dL_db;
        const float gm1 = 2.f * e.S1[k] * dL_dc + e.S0[k] * dL_db;
        gJ00 += V[4 * k + 0] * gm0; gJ02 += V[4 * k + 2] * gm0;
        gJ11 += V[4 * k + 1] * gm1; gJ12 += V[4 * k + 2] * gm1;
    }
    const float xmask = (e.txtz < -e.limx || e.txtz > e.limx) ? 0.f : 1.f;
    const float ymask = (e.tytz < -e.limy || e.tytz > e.limy) ? 0.f : 1.f;
    const float tz = 1.f / e.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
    const float gtx = xmask * -e.fx * tz2 * gJ02;
    const float gty = ymask * -e.fy * tz2 * gJ12;
    const float gtz = -e.fx * tz2 * gJ00 - e.fy * tz2 * gJ11 + (2.f * e.fx * e.tx) * tz3 * gJ02 +
                      (2.f * e.fy * e.ty) * tz3 * gJ12;
#pragma unroll
    for (int k = 0; k < 3; k++) gmean[k] += V[4 * k + 0] * gtx + V[4 * k + 1] * gty + V[4 * k + 2] * gtz;

    // screen-space mean (NDC-scaled) through the projective divide
    float hom[4]; xform44(p, PM, hom);
    const float mw = 1.f / (hom[3] + 0.0000001f);
    const float mul1 = hom[0] * mw * mw, mul2 = hom[1] * mw * mw;
#pragma unroll
    for (int k = 0; k < 3; k++)
        gmean[k] += (PM[4 * k + 0] * mw - PM[4 * k + 3] * mul1) * acc[0] + (PM[4 * k + 1] * mw - PM[4 * k + 3] * mul2) * acc[1];

    // depth = view.z
    const float mul3 = V[2] * p[0] + V[6] * p[1] + V[10] * p[2] + V[14];
#pragma unroll
    for (int k = 0; k < 3; k++) gmean[k] += (V[4 * k + 2] - V[4 * k + 3] * mul3) * acc[9];

    // colour -> SH coefficients and view direction
    if (shs) {
        float x, y, z, inv; sh_view_dir(p, campos, x, y, z, inv);
        const float* sh = shs + (size_t)i * M * 3;
        // (fused SH leaf: M == 1, checked by the caller; without a dsh array the three values go straight to the stage)
        float* gsh = dsh ? dsh + (size_t)i * M * 3 : stage + ST_SH + 3 * tid;
        const uint32_t cl = clamped[i] & EGS_CLAMP_MASK;
        float gdir[3] = { 0.f, 0.f, 0.f };
        for (int ch = 0; ch < 3; ch++) {
            const float g = ((cl >> ch) & 1u) ? 0.f : acc[6 + ch];
            sh_channel_backward(D, M, sh, gsh, ch, x, y, z, g, gdir);
        }
        if (SINK && dsh && (fused & (1u << EGS_SINK_SH))) { stage[ST_SH + 3 * tid] = gsh[0]; stage[ST_SH + 3 * tid + 1] = gsh[1]; stage[ST_SH + 3 * tid + 2] = gsh[2]; }
        sh_dir_to_pos(x, y, z, inv, gdir, gmean);
    }
    if constexpr (MOT == 2) {                                          // gmean is dL/dp', complete: chain it through the placement
        if (!mot.moved || mot.moved[i]) {
            if (mot.pose_partial) egs_motion_pose_terms(gmean, p0, red);
            const float gp[3] = { gmean[0], gmean[1], gmean[2] };
            egs_motion_point_backward(mot.A, gp, gmean);
        }
    }
    if (dmeans3D) { dmeans3D[3 * i] = gmean[0]; dmeans3D[3 * i + 1] = gmean[1]; dmeans3D[3 * i + 2] = gmean[2]; }
    if (SINK && (fused & (1u << EGS_SINK_MEANS3D))) { stage[ST_MEANS + 3 * tid] = gmean[0]; stage[ST_MEANS + 3 * tid + 1] = gmean[1]; stage[ST_MEANS + 3 * tid + 2] = gmean[2]; }

    // cov3D -> scale, quaternion (only when the forward built cov3D itself)
    if (!cov3D_in) {
        // splat_geom.h, the text k_cov3d_backward runs: under the object rotation (egs_object_rotation) L = M L0, dL/dL0 = M^T dL/dL, with the
        // reference's duplicated-index multiplier on row 0 (covariance.py)
        const bool moved = rot.M && (!rot.sel || rot.sel[i]);
        const float mult = (moved && i == 0) ? (rot.mult_dev ? rot.mult_dev[0] : rot.mult) : 1.f;
        bool want_dM = false;
        if constexpr (MOT != 0) want_dM = moved && mot.dM_partial;
        CovFactor f; cov_factor(s, mod, q, moved, rot.M, f);
        CovGrad g; cov_factor_backward(f, s, mod, q, qinv, moved, rot.M, g6, mult, want_dM, act & EGS_ACT_LOG_SCALES, act & EGS_ACT_RAW_QUATS, g);
        if constexpr (MOT != 0) {
            if (want_dM) {                                            // dL/dM = gL L0^T (the row-0 multiplier is in gL)
#pragma unroll
                for (int k = 0; k < 9; k++) red[EGS_MOTION_POSE_SUMS + k] = g.dM[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (dscales) dscales[3 * i + k] = g.dscale[k];
            if (SINK && (fused & (1u << EGS_SINK_SCALES))) stage[ST_SCALES + 3 * tid + k] = g.dscale[k];
        }
        const float* gq = g.gq;
        if (drots) { drots[4 * i + 0] = gq[0]; drots[4 * i + 1] = gq[1]; drots[4 * i + 2] = gq[2]; drots[4 * i + 3] = gq[3]; }
        if (SINK && (fused & (1u << EGS_SINK_ROTATIONS))) *reinterpret_cast<float4*>(stage + ST_ROTS + 4 * tid) = make_float4(gq[0], gq[1], gq[2], gq[3]);
    }
}

// One lane per Gaussian.  SINK (the optimizer fused into the backward, include/egs_raster.h egs_backward_adam): instead of (or besides)
// writing the gradients of the leaves it owns, the workgroup parks them in LDS in array order and then takes the Adam step of ITS 256
// rows of every such leaf with the stand-alone kernel's arithmetic (egs_adam1) and access pattern (float4, fully coalesced:
// rows 256 b .. 256 b + 255 of a [P, k] array are one contiguous span).  The gradients never reach HBM and the parameters are not
// read a second time by another launch: 16 B in + 12 B out per element become 12 + 12, and the step has one launch less.
// 896 float4 tasks per workgroup (64 x (3 + 1 + 3 + 4 + 3)), task -> leaf boundaries fall on wave boundaries.
// MOT: see pp_bwd_one.  The pose sums are a workgroup-uniform branch on the scratch pointers: a constant pose (no gradient asked for) pays no shuffle.
template <bool SINK, int MOT, bool ENT = false>
__global__ __launch_bounds__(256) void k_preprocess_backward(
    int P, int D, int M, const float* __restrict__ means3D, const float* __restrict__ shs,
    const float* __restrict__ scales, float mod, const float* __restrict__ rots, const float* __restrict__ cov3D_in, int act,
    const float* __restrict__ V, const float* __restrict__ PM, const float* __restrict__ campos, int W, int H,
    float tanfovx, float tanfovy, const int32_t* __restrict__ radii, const uint8_t* __restrict__ clamped,
    const float4* __restrict__ rec, const float* __restrict__ grad_acc, float* __restrict__ dmeans2D, float* __restrict__ dcolors,
    float* __restrict__ dopac, float* __restrict__ dmeans3D, float* __restrict__ dcov3D, float* __restrict__ dsh,
    float* __restrict__ dscales, float* __restrict__ drots,
    float* __restrict__ stat_grad_accum, float* __restrict__ stat_denom, float* __restrict__ stat_max_radii,
    const uint32_t* __restrict__ skip_flag, EgsSink sink, EgsObjRot rot, EgsMotion mot, std::conditional_t<ENT, EgsEntropy, EgsNoEntropy> ent) {
    __shared__ __attribute__((aligned(16))) float stage[SINK ? 4 * EGS_SINK_TASKS : 4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned fused = 0;
    if (SINK) {
#pragma unroll
        for (int l = 0; l < EGS_SINK_PP_LEAVES; l++) fused |= sink.leaf[l].p ? (1u << l) : 0u;
    }
    float red[MOT != 0 ? EGS_MOTION_SUMS : 1];
    if constexpr (MOT != 0) {
#pragma unroll
        for (int k = 0; k < EGS_MOTION_SUMS; k++) red[k] = 0.f;
    }
    float ent_coef = 0.f;
    if constexpr (ENT) ent_coef = egs_entropy_coef(ent.n_vis, ent.weight, ent.upstream);
    if (i < P)
        pp_bwd_one<SINK, MOT, ENT>(i, D, M, means3D, shs, scales, mod, rots, cov3D_in, act, V, PM, campos, W, H, tanfovx, tanfovy, radii, clamped, rec,
                         grad_acc, grad_acc + (size_t)P * EGS_GRAD_STRIDE, egs_hot_slots((size_t)P), dmeans2D, dcolors, dopac, dmeans3D, dcov3D, dsh, dscales, drots, stat_grad_accum, stat_denom,
                         stat_max_radii, skip_flag, stage, fused, rot, mot, red, ent_coef);
    if constexpr (MOT != 0) {
        __shared__ float wsum_p[4][EGS_MOTION_POSE_SUMS], wsum_m[4][EGS_MOTION_ROT_SUMS];
        if (MOT == 2 && mot.pose_partial) egs_motion_block_sum<EGS_MOTION_POSE_SUMS>(red, wsum_p, mot.pose_partial + (size_t)blockIdx.x * EGS_MOTION_POSE_SUMS);
        if (mot.dM_partial) egs_motion_block_sum<EGS_MOTION_ROT_SUMS>(red + EGS_MOTION_POSE_SUMS, wsum_m, mot.dM_partial + (size_t)blockIdx.x * EGS_MOTION_ROT_SUMS);
    }
    if (!SINK) return;
    __syncthreads();
    if (sink.skip && *sink.skip) return;                            // the frame overflowed its instance capacity: no step (and none was counted)
    const int rows = sink.active_rows ? min(P, max(*sink.active_rows, 0)) : P;      // capacity-sized model: live rows only
    const int row0 = blockIdx.x * 256;
    const int live = min(256, rows - row0);                          // rows of this workgroup that take the step
    if (live <= 0) return;
    constexpr int RF[EGS_SINK_PP_LEAVES] = { 3, 1, 3, 4, 3 };
    constexpr int T0[EGS_SINK_PP_LEAVES + 1] = { 0, 192, 256, 448, 704, 896 };
    // all loads of the thread's (up to four) tasks first, then the arithmetic, then the stores
    float4 Pq[4], Mq[4], Vq[4]; int cnt[4]; float* pp[4]; float* pm[4]; float* pv[4]; float ss[4], ib[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int task = (int)threadIdx.x + 256 * k;
        cnt[k] = 0;
#pragma unroll
        for (int l = 0; l < EGS_SINK_PP_LEAVES; l++) {
            if (task < T0[l] || task >= T0[l + 1] || !sink.leaf[l].p) continue;
            const int e = 4 * (task - T0[l]);                         // first element of the task inside the workgroup's span of leaf l
            const size_t off = (size_t)row0 * RF[l] + e;
            pp[k] = sink.leaf[l].p + off; pm[k] = sink.leaf[l].m + off; pv[k] = sink.leaf[l].v + off;
            cnt[k] = max(0, min(4, live * RF[l] - e));
            ss[k] = sink.coef[2 * l]; ib[k] = sink.coef[2 * l + 1];
        }
        if (cnt[k] == 4 && ((((size_t)pp[k]) | ((size_t)pm[k]) | ((size_t)pv[k])) & 15) == 0) {
            Pq[k] = *reinterpret_cast<const float4*>(pp[k]); Mq[k] = *reinterpret_cast<const float4*>(pm[k]); Vq[k] = *reinterpret_cast<const float4*>(pv[k]);
        } else if (cnt[k] > 0) {
            float t[12];
#pragma unroll
            for (int j = 0; j < 4; j++) { const bool ok = j < cnt[k]; t[j] = ok ? pp[k][j] : 0.f; t[4 + j] = ok ? pm[k][j] : 0.f; t[8 + j] = ok ? pv[k][j] : 0.f; }
            Pq[k] = make_float4(t[0], t[1], t[2], t[3]); Mq[k] = make_float4(t[4], t[5], t[6], t[7]); Vq[k] = make_float4(t[8], t[9], t[10], t[11]);
            cnt[k] = -cnt[k];                                          // negative: element-wise stores
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (cnt[k] == 0) continue;
        const float4 G = *reinterpret_cast<const float4*>(stage + 4 * ((int)threadIdx.x + 256 * k));
        float4 Pn = Pq[k], Mn = Mq[k], Vn = Vq[k];
        egs_adam1(Pn.x, G.x, Mn.x, Vn.x, sink.b1, sink.b2, sink.eps, ss[k], ib[k]); egs_adam1(Pn.y, G.y, Mn.y, Vn.y, sink.b1, sink.b2, sink.eps, ss[k], ib[k]);
        egs_adam1(Pn.z, G.z, Mn.z, Vn.z, sink.b1, sink.b2, sink.eps, ss[k], ib[k]); egs_adam1(Pn.w, G.w, Mn.w, Vn.w, sink.b1, sink.b2, sink.eps, ss[k], ib[k]);
        if (cnt[k] == 4) {
            *reinterpret_cast<float4*>(pp[k]) = Pn; *reinterpret_cast<float4*>(pm[k]) = Mn; *reinterpret_cast<float4*>(pv[k]) = Vn;
        } else {
            const float a[4] = { Pn.x, Pn.y, Pn.z, Pn.w }, b_[4] = { Mn.x, Mn.y, Mn.z, Mn.w }, c_[4] = { Vn.x, Vn.y, Vn.z, Vn.w };
#pragma unroll
            for (int j = 0; j < 4; j++) if (j < -cnt[k]) { pp[k][j] = a[j]; pm[k][j] = b_[j]; pv[k][j] = c_[j]; }
        }
    }
}

__global__ __launch_bounds__(256) void k_mark_visible(int P, const float* __restrict__ means3D,
                                                       const float* __restrict__ V, uint8_t* __restrict__ present) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float p[3] = { means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2] };
    float t[3]; xform43(p, V, t);
    present[i] = t[2] > 0.2f ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_zero_f4(float4* __restrict__ p, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

namespace {
__global__ void k_zero_u32(uint32_t* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}
}  // namespace
hipError_t egs_launch_zero_u32(uint32_t* p, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_zero_u32, dim3(blocks), dim3(256), 0, s, p, n);
    return hipGetLastError();
}

hipError_t egs_launch_zero_f4(float4* p, size_t n4, hipStream_t s) {
    if (n4 == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_zero_f4, dim3(blocks), dim3(256), 0, s, p, n4);
    return hipGetLastError();
}

// The leading arguments of the preprocess kernels, forward and backward, in the order all of them declare: written once.  `shs` is what the
// kernel is given (NULL when the spherical harmonics run as launches of their own, and for the backward of precomputed colours).
#define PP_SCENE sc.P, sc.D, sc.M, sc.means3D, shs
#define PP_SHAPE_CAM sc.scales, sc.mod, sc.rots, sc.cov3D, sc.act, cam.view, cam.proj, cam.campos, cam.W, cam.H, cam.tanfovx, cam.tanfovy, radii
// the record of the forward kernels, member for member
#define PP_ARGS(active_count) { PP_SCENE, sc.colors, sc.opac, PP_SHAPE_CAM, g.rec, g.rect, g.offsets, g.clamped, g.visible, g.scan_scratch, g.block_hot, active_count }

hipError_t egs_launch_preprocess(const EgsScene& sc, EgsCamera cam, int32_t* radii, EgsGeomPtrs g, uint32_t* zero_words, size_t zero_n,
                                 const int32_t* active_count, const EgsImgPtrs* place, EgsObjRot rot, EgsMotion mot, hipStream_t s) {
    const int P = sc.P;
    if (P == 0) return hipSuccess;
    if (!zero_words) zero_n = 0;
    const float* shs = egs_sh_apart(sc) ? nullptr : sc.shs;
    const EgsPreArgs a = PP_ARGS(active_count);
    EgsPrologueArgs pa = {};
    if (place) {
        pa.n_tiles = (int)egs_tiles(cam.W, cam.H);
        pa.quad_work = place->fwd_cost; pa.tile_order = place->fwd_order;
        if (mot.A) hipLaunchKernelGGL((k_preprocess<true, true>), dim3((P + 255) / 256 + EGS_XCDS), dim3(256), 0, s, a, zero_words, zero_n, pa, rot, mot);
        else hipLaunchKernelGGL((k_preprocess<true, false>), dim3((P + 255) / 256 + EGS_XCDS), dim3(256), 0, s, a, zero_words, zero_n, pa, rot, mot);
    } else {
        if (mot.A) hipLaunchKernelGGL((k_preprocess<false, true>), dim3((P + 255) / 256), dim3(256), 0, s, a, zero_words, zero_n, pa, rot, mot);
        else hipLaunchKernelGGL((k_preprocess<false, false>), dim3((P + 255) / 256), dim3(256), 0, s, a, zero_words, zero_n, pa, rot, mot);
    }
    return hipGetLastError();
}

bool egs_can_fuse_count(int P, int W, int H, int cull) {
    if (P <= 0) return false;
    const EgsBinGeometry q = egs_bin_geometry(P, W, H, cull);
    // one round only: the looped instantiation holds the projection's inputs through the walk and spills (1M @ 1080p, four rounds of eight
    // groups: 116 + 151 us against 34 + 214 with the separate count pass) -- EGS_FUSE_MULTI_ROUND=1 lets it run all the same (measurements)
    static const bool multi = getenv("EGS_FUSE_MULTI_ROUND") != nullptr;
    if (!multi && bin_groups_per_block((unsigned)P, q.nblocks) > (unsigned)q.gpr) return false;
    return q.gpr >= 4 && q.gpr % 4 == 0 && q.lds >= sizeof(EgsOrderLds);
}
hipError_t egs_launch_preprocess_count(const EgsScene& sc, EgsCamera cam, int32_t* radii, EgsGeomPtrs g, EgsBinPtrs b,
                                       const int32_t* active_count, const EgsImgPtrs* place, EgsObjRot rot, EgsMotion mot, int cull, hipStream_t s) {
    const int P = sc.P;
    const EgsBinGeometry q = egs_bin_geometry(P, cam.W, cam.H, cull);
    const float* shs = egs_sh_apart(sc) ? nullptr : sc.shs;
    const EgsPreArgs a = PP_ARGS(active_count);
    EgsCountArgs c = { q.gpr, q.gx, q.n_tiles, q.nblocks, q.cull, q.use_map, b.table, q.stride, b.chunk_sum };
    EgsPrologueArgs pa = {};
    const unsigned grid = ((q.nblocks + 7) / 8) * 8;
    const bool one = bin_groups_per_block((unsigned)P, q.nblocks) <= (unsigned)q.gpr;
    if (place) { pa.n_tiles = q.n_tiles; pa.quad_work = place->fwd_cost; pa.tile_order = place->fwd_order; }
#define PC_LAUNCH(PL, ONE, MO) do {                                                                                                       \
        if (q.lds > 64 * 1024) {                                                                                                      \
            hipError_t e = hipFuncSetAttribute((const void*)k_preprocess_count<PL, ONE, MO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.lds); \
            if (e != hipSuccess) return e;                                                                                            \
        }                                                                                                                             \
        hipLaunchKernelGGL((k_preprocess_count<PL, ONE, MO>), dim3(grid + (PL ? EGS_XCDS : 0)), dim3(EGS_BIN_THREADS), q.lds, s, a, c, pa, rot, mot); } while (0)
    if (mot.A) {
        if (place) { if (one) PC_LAUNCH(true, true, true); else PC_LAUNCH(true, false, true); }
        else { if (one) PC_LAUNCH(false, true, true); else PC_LAUNCH(false, false, true); }
    } else {
        if (place) { if (one) PC_LAUNCH(true, true, false); else PC_LAUNCH(true, false, false); }
        else { if (one) PC_LAUNCH(false, true, false); else PC_LAUNCH(false, false, false); }
    }
#undef PC_LAUNCH
    return hipGetLastError();
}

// With split or M > 1 harmonics egs_launch_sh_backward follows and finishes the positions' gradient (the <.., 1> instantiations under motion).
hipError_t egs_launch_preprocess_backward(const EgsScene& sc, EgsCamera cam, const int32_t* radii, EgsGeomPtrs g, const float* grad_acc,
                                          const EgsGrads& d, const EgsStats& st, const EgsSink* sink, EgsObjRot rot, EgsMotion mot, hipStream_t s,
                                          const EgsEntropy* ent) {
    const int P = sc.P;
    if (P == 0) return hipSuccess;
    if (ent && mot.A) return hipErrorInvalidValue;                   // (the entropy instantiations exist without object motion: the static stages)
    EgsSink none = {};
    const EgsNoEntropy no_ent = {};
    const bool motion_finished_later = egs_sh_apart(sc), own_sh = !sc.colors && !motion_finished_later;
    const float* shs = own_sh ? sc.shs : nullptr;
#define PPB_ARGS PP_SCENE, PP_SHAPE_CAM, g.clamped, g.rec, grad_acc, d.means2D, d.colors, d.opacity, d.means3D, d.cov3D, own_sh ? d.sh : nullptr, \
                 sc.cov3D ? nullptr : d.scales, sc.cov3D ? nullptr : d.rotations, st.grad_accum, st.denom, st.max_radii, st.skip_flag
    const dim3 grid((P + 255) / 256), block(256);
    if (ent) {
        if (sink) hipLaunchKernelGGL((k_preprocess_backward<true, 0, true>), grid, block, 0, s, PPB_ARGS, *sink, rot, mot, *ent);
        else hipLaunchKernelGGL((k_preprocess_backward<false, 0, true>), grid, block, 0, s, PPB_ARGS, none, rot, mot, *ent);
    } else if (!mot.A) {
        if (sink) hipLaunchKernelGGL((k_preprocess_backward<true, 0>), grid, block, 0, s, PPB_ARGS, *sink, rot, mot, no_ent);
        else hipLaunchKernelGGL((k_preprocess_backward<false, 0>), grid, block, 0, s, PPB_ARGS, none, rot, mot, no_ent);
    } else if (motion_finished_later) {
        if (sink) hipLaunchKernelGGL((k_preprocess_backward<true, 1>), grid, block, 0, s, PPB_ARGS, *sink, rot, mot, no_ent);
        else hipLaunchKernelGGL((k_preprocess_backward<false, 1>), grid, block, 0, s, PPB_ARGS, none, rot, mot, no_ent);
    } else {
        if (sink) hipLaunchKernelGGL((k_preprocess_backward<true, 2>), grid, block, 0, s, PPB_ARGS, *sink, rot, mot, no_ent);
        else hipLaunchKernelGGL((k_preprocess_backward<false, 2>), grid, block, 0, s, PPB_ARGS, none, rot, mot, no_ent);
    }
#undef PPB_ARGS
#undef PP_ARGS
#undef PP_SHAPE_CAM
#undef PP_SCENE
    return hipGetLastError();
}


hipError_t egs_launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t s) {
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mark_visible, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, present);
    return hipGetLastError();
}
