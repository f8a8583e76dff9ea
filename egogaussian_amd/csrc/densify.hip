// densify.hip -- densification bookkeeping on the device (densify / prune part).
// What the reference does with boolean-mask indexing, torch.cat and repeated nn.Parameter re-creation
// (/root/reference/scene/gaussian_model.py:506-709, :735-740; trainers/train_static.py:125-127) is restated as:
//   k_densify_stats      the per-iteration statistics (gradient-norm accumulator, visit count, largest screen radius) in one
//                        pass over the Gaussians -- no index tensors, no host round trip for the mask size
//   k_densify_flags      every selection rule of densify_and_clone / densify_and_split / the final prune, evaluated once per
//                        source Gaussian for the up to four results it can produce (itself, a clone, two split children)
//   scans + k_densify_emit   stream compaction: the results' (source, kind) in EXACTLY the order the reference's
//                        cat / mask sequence leaves them: [kept originals | kept clones | kept first children | kept second children]
//   k_gather_rows_f32 / k_gather_i32 / k_split_children      build every array of the new model from the plan
//   k_densify_flags_dev / k_mask_flags_dev + k_apply_gather / k_apply_commit   the same plan over the `capacity` rows of a capacity-sized
//                        model with the live count and the rule values read on the device, applied in place in two launches through a
//                        shadow copy: no count goes to the host, so the chain can be recorded once and replayed
// Semantics follow the reference code path as it actually runs, including: NaN gradient means (0/0) count as 0; the
// statistics (and with them max_radii2D) are zeroed by densification_postfix before the final prune whenever a clone or
// split step ran; clones take `curr_gen` when it is given, split children always inherit (see oracle/densify_torch.py).
#include "egs_common.h"
#include <math.h>
#include <string.h>

namespace {

__global__ __launch_bounds__(256) void k_densify_stats(int P, const float* __restrict__ vs_grad, const uint8_t* __restrict__ visible,
                                                        const int32_t* __restrict__ radii, float* __restrict__ accum,
                                                        float* __restrict__ denom, float* __restrict__ max_radii) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const bool vis = visible ? visible[i] != 0 : radii[i] > 0;
    if (!vis) return;
    const float gx = vs_grad[3 * i], gy = vs_grad[3 * i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.f;
    if (radii && max_radii) max_radii[i] = fmaxf(max_radii[i], (float)radii[i]);
}

struct DensifyRules {
    float max_grad, min_opacity, dense_extent /* percent_dense * extent */, big_extent /* 0.1 * extent */, max_screen_size;
    int use_screen_size, clone, split, has_curr_gen, curr_gen, prune_prev_gen, has_object, which_object, stats_reset;
};

// One source Gaussian's four decisions -> bit 0 keep_orig, 1 keep_clone, 2 keep_child, 3 is_split (shared by the host-sized and the
// device-sized plan: the same expressions, so the same plan).
__device__ __forceinline__ uint32_t densify_flags_row(float accum, float denom, const float* __restrict__ scaling_raw3, float opacity_raw,
                                                       float max_radius, int gen, int is_object, const DensifyRules& r) {
    float g = accum / denom;
    if (g != g) g = 0.f;                                              // grads[grads.isnan()] = 0
    const float smax = fmaxf(fmaxf(expf(scaling_raw3[0]), expf(scaling_raw3[1])), expf(scaling_raw3[2]));
    const bool obj_ok = !r.has_object || is_object == r.which_object;
    const bool C = r.clone && fabsf(g) >= r.max_grad && smax <= r.dense_extent && obj_ok;
    const bool S = r.split && g >= r.max_grad && smax > r.dense_extent && obj_ok;
    const float opacity = 1.f / (1.f + expf(-opacity_raw));
    const bool faint = opacity < r.min_opacity;
    const bool big_vs = r.use_screen_size && !r.stats_reset && max_radius > r.max_screen_size;
    const bool big_ws = r.use_screen_size && smax > r.big_extent;
    const bool big_ws_child = r.use_screen_size && expf(logf(smax / 1.6f)) > r.big_extent;    // children carry log(scale / 1.6)
    const bool gen_orig = r.prune_prev_gen || gen == r.curr_gen;
    const bool gen_clone = r.prune_prev_gen || (r.has_curr_gen ? r.curr_gen : gen) == r.curr_gen;
    const bool prune_orig = (faint || big_vs || big_ws) && gen_orig;
    const bool prune_clone = (faint || big_ws) && gen_clone;
    const bool prune_child = (faint || big_ws_child) && gen_orig;
    return ((!S && !prune_orig) ? 1u : 0u) | ((C && !prune_clone) ? 2u : 0u) | ((S && !prune_child) ? 4u : 0u) | (S ? 8u : 0u);
}

__global__ __launch_bounds__(256) void k_densify_flags(int P, const float* __restrict__ accum, const float* __restrict__ denom,
                                                        const float* __restrict__ scaling_raw, const float* __restrict__ opacity_raw,
                                                        const float* __restrict__ max_radii, const int32_t* __restrict__ generation,
                                                        const int32_t* __restrict__ is_object, DensifyRules r,
                                                        uint32_t* __restrict__ keep_orig, uint32_t* __restrict__ keep_clone,
                                                        uint32_t* __restrict__ keep_child, uint32_t* __restrict__ is_split) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t f = densify_flags_row(accum[i], denom[i], scaling_raw + 3 * (size_t)i, opacity_raw[i], max_radii[i], generation[i], is_object[i], r);
    keep_orig[i] = f & 1u; keep_clone[i] = (f >> 1) & 1u; keep_child[i] = (f >> 2) & 1u; is_split[i] = (f >> 3) & 1u;
}

// Plain mask -> flags (prune_points): keep_orig = !mask, nothing else.
__global__ __launch_bounds__(256) void k_mask_flags(int P, const uint8_t* __restrict__ prune_mask, uint32_t* __restrict__ keep_orig,
                                                     uint32_t* __restrict__ keep_clone, uint32_t* __restrict__ keep_child,
                                                     uint32_t* __restrict__ is_split) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    keep_orig[i] = prune_mask[i] ? 0u : 1u; keep_clone[i] = 0u; keep_child[i] = 0u; is_split[i] = 0u;
}

// flags: values before the scans; off_*: their exclusive scans; totals[0..3] = (originals, clones, children, splits)
__global__ __launch_bounds__(256) void k_densify_emit(int P, const uint32_t* __restrict__ flags /* [4][P] */, const uint32_t* __restrict__ offs /* [4][P] */,
                                                       const uint64_t* __restrict__ totals, int32_t* __restrict__ src, uint8_t* __restrict__ kind,
                                                       int32_t* __restrict__ split_rank /* [P] */) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t nO = (uint32_t)totals[0], nC = (uint32_t)totals[1], nK = (uint32_t)totals[2];
    if (flags[i]) { const uint32_t p = offs[i]; src[p] = i; kind[p] = 0; }
    if (flags[(size_t)P + i]) { const uint32_t p = nO + offs[(size_t)P + i]; src[p] = i; kind[p] = 1; }
    if (flags[2 * (size_t)P + i]) {
        const uint32_t p = nO + nC + offs[2 * (size_t)P + i];
        src[p] = i; kind[p] = 2; src[p + nK] = i; kind[p + nK] = 3;
    }
    split_rank[i] = flags[3 * (size_t)P + i] ? (int32_t)offs[3 * (size_t)P + i] : -1;
}

// out[row][0..D) = in[src[row]][0..D); mode 1 (optimizer moments): zero for every row that is not a kept original.
__global__ __launch_bounds__(256) void k_gather_rows_f32(size_t n_elems, int D, const int32_t* __restrict__ src, const uint8_t* __restrict__ kind,
                                                          int zero_new, const float* __restrict__ in, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const size_t row = e / (size_t)D;
    const int col = (int)(e - row * (size_t)D);
    out[e] = (zero_new && kind[row] != 0) ? 0.f : in[(size_t)src[row] * D + col];
}

__global__ __launch_bounds__(256) void k_gather_i32(int n, const int32_t* __restrict__ src, const uint8_t* __restrict__ kind, int clone_value_on,
                                                     int clone_value, const int32_t* __restrict__ in, int32_t* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    out[e] = (clone_value_on && kind[e] == 1) ? clone_value : in[src[e]];
}

// Rows of kind 2 / 3 (first / second split child): position = parent + R(q) (scale * z), raw scale = log(scale / 1.6).
// z holds the 2 * n_split standard-normal draws in the reference's order: all first children, then all second children.
__global__ __launch_bounds__(256) void k_split_children(int n, const int32_t* __restrict__ src, const uint8_t* __restrict__ kind,
                                                         const int32_t* __restrict__ split_rank, int n_split, const float* __restrict__ z,
                                                         const float* __restrict__ xyz_old, const float* __restrict__ scaling_old,
                                                         const float* __restrict__ rot_old, float* __restrict__ xyz_new,
                                                         float* __restrict__ scaling_new) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n || kind[e] < 2) return;
    const int s = src[e];
    const float* zz = z + 3 * ((size_t)(kind[e] - 2) * n_split + split_rank[s]);
    const float sc[3] = { expf(scaling_old[3 * s]), expf(scaling_old[3 * s + 1]), expf(scaling_old[3 * s + 2]) };
    const float v[3] = { sc[0] * zz[0], sc[1] * zz[1], sc[2] * zz[2] };
    float q[4] = { rot_old[4 * s], rot_old[4 * s + 1], rot_old[4 * s + 2], rot_old[4 * s + 3] };
    const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = q[0] * inv, x = q[1] * inv, y = q[2] * inv, w = q[3] * inv;
    const float R[9] = { 1.f - 2.f * (y * y + w * w), 2.f * (x * y - r * w), 2.f * (x * w + r * y),
                         2.f * (x * y + r * w), 1.f - 2.f * (x * x + w * w), 2.f * (y * w - r * x),
                         2.f * (x * w - r * y), 2.f * (y * w + r * x), 1.f - 2.f * (x * x + y * y) };
#pragma unroll
    for (int a = 0; a < 3; a++) {
        xyz_new[3 * e + a] = (R[3 * a] * v[0] + R[3 * a + 1] * v[1] + R[3 * a + 2] * v[2]) + xyz_old[3 * s + a];
        scaling_new[3 * e + a] = logf(sc[a] / 1.6f);
    }
}

// ---- device-sized plan and in-place apply (capacity-sized models; include/egs_raster.h "f-4, capturable") ----------------------------------
__device__ __forceinline__ int live_rows(const int32_t* active_count, int capacity) {
    const int n = *active_count;
    return n < 0 ? 0 : (n > capacity ? capacity : n);
}

// k_densify_flags over capacity rows: the rules from the device block, no flag for a row at or beyond the live count.
__global__ __launch_bounds__(256) void k_densify_flags_dev(int capacity, const int32_t* __restrict__ active_count, const float* __restrict__ accum,
                                                            const float* __restrict__ denom, const float* __restrict__ scaling_raw,
                                                            const float* __restrict__ opacity_raw, const float* __restrict__ max_radii,
                                                            const int32_t* __restrict__ generation, const void* __restrict__ is_object,
                                                            int is_object_is_float, const egs_densify_rules_dev* __restrict__ rules,
                                                            uint32_t* __restrict__ flags /* [4][capacity] */, uint64_t* __restrict__ totals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= capacity) return;
    const int n = live_rows(active_count, capacity);
    if (i == 0) totals[4] = (uint64_t)n;
    uint32_t f = 0u;
    if (i < n) {
        const egs_densify_rules_dev d = *rules;
        DensifyRules r;
        r.max_grad = d.max_grad; r.min_opacity = d.min_opacity; r.dense_extent = d.dense_extent; r.big_extent = d.big_extent;
        r.max_screen_size = d.max_screen_size; r.use_screen_size = d.max_screen_size > 0.f; r.clone = d.clone != 0; r.split = d.split != 0;
        r.has_curr_gen = d.has_curr_gen != 0; r.curr_gen = d.curr_gen; r.prune_prev_gen = d.prune_prev_gen != 0;
        r.has_object = d.has_which_object != 0; r.which_object = d.which_object; r.stats_reset = (d.clone || d.split) ? 1 : 0;
        const int obj = is_object_is_float ? (int)((const float*)is_object)[i] : ((const int32_t*)is_object)[i];
        f = densify_flags_row(accum[i], denom[i], scaling_raw + 3 * (size_t)i, opacity_raw[i], max_radii[i], generation[i], obj, r);
    }
    const size_t C = (size_t)capacity;
    flags[i] = f & 1u; flags[C + i] = (f >> 1) & 1u; flags[2 * C + i] = (f >> 2) & 1u; flags[3 * C + i] = (f >> 3) & 1u;
}

__global__ __launch_bounds__(256) void k_mask_flags_dev(int capacity, const int32_t* __restrict__ active_count, const uint8_t* __restrict__ prune_mask,
                                                         uint32_t* __restrict__ flags /* [4][capacity] */, uint64_t* __restrict__ totals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= capacity) return;
    const int n = live_rows(active_count, capacity);
    if (i == 0) totals[4] = (uint64_t)n;
    const size_t C = (size_t)capacity;
    flags[i] = (i < n && !prune_mask[i]) ? 1u : 0u; flags[C + i] = 0u; flags[2 * C + i] = 0u; flags[3 * C + i] = 0u;
}

struct ApplyArray { uint32_t* data; uint32_t* shadow; int32_t D, role, flags, pad; };
struct ApplyTable { ApplyArray a[EGS_DENSIFY_MAX_ARRAYS]; int32_t xyz, scaling, rotation, n; };

struct ApplyCounts { uint64_t n_new, n_old, n_split; };
__device__ __forceinline__ ApplyCounts apply_counts(const uint64_t* __restrict__ totals) {
    ApplyCounts c;
    c.n_new = totals[0] + totals[1] + 2 * totals[2]; c.n_split = totals[3]; c.n_old = totals[4];
    return c;
}

// Component `col` of a split child's position (which == 0) or raw scale (which == 1): k_split_children's expressions, one output each.
__device__ __forceinline__ float split_child_value(int which, int col, int s, int child, int rank, uint64_t n_split, const float* __restrict__ z,
                                                   const float* __restrict__ xyz_old, const float* __restrict__ scaling_old,
                                                   const float* __restrict__ rot_old) {
    const float sc[3] = { expf(scaling_old[3 * (size_t)s]), expf(scaling_old[3 * (size_t)s + 1]), expf(scaling_old[3 * (size_t)s + 2]) };
    if (which == 1) return logf(sc[col] / 1.6f);
    const float* zz = z + 3 * ((size_t)child * n_split + (size_t)rank);
    const float v[3] = { sc[0] * zz[0], sc[1] * zz[1], sc[2] * zz[2] };
    const float q[4] = { rot_old[4 * (size_t)s], rot_old[4 * (size_t)s + 1], rot_old[4 * (size_t)s + 2], rot_old[4 * (size_t)s + 3] };
    const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = q[0] * inv, x = q[1] * inv, y = q[2] * inv, w = q[3] * inv;
    const float R[9] = { 1.f - 2.f * (y * y + w * w), 2.f * (x * y - r * w), 2.f * (x * w + r * y),
                         2.f * (x * y + r * w), 1.f - 2.f * (x * x + w * w), 2.f * (y * w - r * x),
                         2.f * (x * w - r * y), 2.f * (y * w + r * x), 1.f - 2.f * (x * x + y * y) };
    return (R[3 * col] * v[0] + R[3 * col + 1] * v[1] + R[3 * col + 2] * v[2]) + xyz_old[3 * (size_t)s + col];
}

// Launch 1 of the apply.  grid = (x, arrays): block row y gathers rows [0, n_new) of array y into its shadow; the arrays themselves are only read.
__global__ __launch_bounds__(256) void k_apply_gather(ApplyTable t, int capacity, const int32_t* __restrict__ src, const uint8_t* __restrict__ kind,
                                                       const int32_t* __restrict__ split_rank, const uint64_t* __restrict__ totals,
                                                       const egs_densify_rules_dev* __restrict__ rules, const float* __restrict__ z) {
    const ApplyCounts c = apply_counts(totals);
    if (c.n_new > (uint64_t)capacity || c.n_old == 0) return;                      // refused / empty model: the commit launch reports it
    const int ai = blockIdx.y;
    const ApplyArray A = t.a[ai];
    const bool stats_reset = rules && (rules->clone || rules->split);
    if (A.role == EGS_DENSIFY_STAT && stats_reset) return;
    const bool clone_gen = A.role == EGS_DENSIFY_TAG && (A.flags & EGS_DENSIFY_TAG_CLONE_GEN) && rules && rules->has_curr_gen;
    const uint32_t gen_bits = clone_gen ? (uint32_t)rules->curr_gen : 0u;
    const bool tag_float = A.role == EGS_DENSIFY_TAG && !(A.flags & EGS_DENSIFY_TAG_I32);
    const int child_of = (A.role == EGS_DENSIFY_PARAM && z) ? (ai == t.xyz ? 0 : (ai == t.scaling ? 1 : -1)) : -1;
    const size_t D = (size_t)A.D, n_el = (size_t)c.n_new * D, step = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_el; e += step) {
        const size_t row = e / D;
        const int col = (int)(e - row * D);
        const int s = src[row];
        const int kd = kind[row];
        uint32_t v;
        if (A.role == EGS_DENSIFY_MOMENT && kd != 0) v = 0u;
        else if (clone_gen && kd == 1) v = gen_bits;
        else if (child_of >= 0 && kd >= 2)
            v = __float_as_uint(split_child_value(child_of, col, s, kd - 2, split_rank[s], c.n_split, z, (const float*)t.a[t.xyz].data,
                                                  (const float*)t.a[t.scaling].data, (const float*)t.a[t.rotation].data));
        else {
            v = A.data[(size_t)s * D + col];
            if (tag_float) v = __float_as_uint((float)(int32_t)__uint_as_float(v));            // the host route's .to(int32) and back
        }
        A.shadow[e] = v;
    }
}

// Launch 2: shadow -> arrays, the zeroing, the count and the status words.  Reads no array row, so the order of the blocks does not matter.
__global__ __launch_bounds__(256) void k_apply_commit(ApplyTable t, int capacity, const uint64_t* __restrict__ totals,
                                                       const egs_densify_rules_dev* __restrict__ rules, int32_t* __restrict__ active_count,
                                                       uint32_t* __restrict__ status) {
    const ApplyCounts c = apply_counts(totals);
    const bool refused = c.n_new > (uint64_t)capacity;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (refused) { status[0] += 1u; status[1] = (uint32_t)(c.n_new > 0xffffffffull ? 0xffffffffull : c.n_new); }
        else {
            status[2] += 1u; status[3] = (uint32_t)c.n_new;
            if (c.n_old != 0) *active_count = (int32_t)c.n_new;
        }
    }
    if (refused || c.n_old == 0) return;
    const ApplyArray A = t.a[blockIdx.y];
    const size_t D = (size_t)A.D, step = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (A.role == EGS_DENSIFY_STAT && rules && (rules->clone || rules->split)) {
        for (size_t e = first; e < (size_t)capacity * D; e += step) A.data[e] = 0u;
        return;
    }
    const size_t n_el = (size_t)c.n_new * D;
    for (size_t e = first; e < n_el; e += step) A.data[e] = A.shadow[e];
    if (A.role == EGS_DENSIFY_TAG)                                                          // vacated rows hold no Gaussian
        for (size_t e = n_el + first; e < (size_t)c.n_old * D; e += step) A.data[e] = 0u;
}

}  // namespace

extern "C" {

int egs_densify_stats(int P, const float* viewspace_grad, const uint8_t* visible, const int32_t* radii, float* grad_accum,
                      float* denom, float* max_radii2D, void* stream) {
    if (P < 0) return EGS_ERR_ARG;
    if (P == 0) return 0;
    if (!viewspace_grad || !grad_accum || !denom || (!visible && !radii)) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_densify_stats, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, viewspace_grad, visible, radii,
                       grad_accum, denom, max_radii2D);
    return (int)hipGetLastError();
}

size_t egs_densify_plan_scratch_bytes(int P) {
    const size_t n = (size_t)(P > 0 ? P : 0);
    return egs_align(8 * n * sizeof(uint32_t)) + egs_align((egs_scan_scratch_elems(n) + 64) * sizeof(uint32_t));
}

// Everything is enqueued; the caller reads totals[4] after synchronising and then sizes the new model.
static int plan_common(int P, uint32_t* flags, void* scratch, int32_t* src_index, uint8_t* kind, int32_t* split_rank, uint64_t* totals,
                       hipStream_t s) {
    uint32_t* offs = flags + 4 * (size_t)P;
    uint32_t* spine = (uint32_t*)((char*)scratch + egs_align(8 * (size_t)P * sizeof(uint32_t)));
    for (int k = 0; k < 4; k++) {
        hipError_t e = egs_launch_scan_u32(flags + (size_t)k * P, offs + (size_t)k * P, (size_t)P, 0, spine, totals + k, s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_densify_emit, dim3((P + 255) / 256), dim3(256), 0, s, P, flags, offs, totals, src_index, kind, split_rank);
    return (int)hipGetLastError();
}

int egs_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling_raw, const float* opacity_raw,
                     const float* max_radii2D, const int32_t* generation, const int32_t* is_object, float max_grad, float min_opacity,
                     float percent_dense, float extent, float max_screen_size /* <= 0: criterion off */, int clone, int split,
                     int has_curr_gen, int curr_gen, int prune_prev_gen, int has_which_object, int which_object, void* scratch,
                     int32_t* src_index /*[3P]*/, uint8_t* kind /*[3P]*/, int32_t* split_rank /*[P]*/, uint64_t* totals /*device [4]*/,
                     void* stream) {
    if (P <= 0 || !grad_accum || !denom || !scaling_raw || !opacity_raw || !max_radii2D || !generation || !is_object || !scratch ||
        !src_index || !kind || !split_rank || !totals)
        return EGS_ERR_ARG;
    if (!prune_prev_gen && !has_curr_gen) return EGS_ERR_MODE;
    DensifyRules r;
    r.max_grad = max_grad; r.min_opacity = min_opacity; r.dense_extent = percent_dense * extent; r.big_extent = 0.1f * extent;
    r.max_screen_size = max_screen_size; r.use_screen_size = max_screen_size > 0.f; r.clone = clone != 0; r.split = split != 0;
    r.has_curr_gen = has_curr_gen != 0; r.curr_gen = curr_gen; r.prune_prev_gen = prune_prev_gen != 0;
    r.has_object = has_which_object != 0; r.which_object = which_object; r.stats_reset = (clone || split) ? 1 : 0;
    uint32_t* flags = (uint32_t*)scratch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_densify_flags, dim3((P + 255) / 256), dim3(256), 0, s, P, grad_accum, denom, scaling_raw, opacity_raw, max_radii2D,
                       generation, is_object, r, flags, flags + (size_t)P, flags + 2 * (size_t)P, flags + 3 * (size_t)P);
    return plan_common(P, flags, scratch, src_index, kind, split_rank, totals, s);
}

int egs_prune_plan(int P, const uint8_t* prune_mask, void* scratch, int32_t* src_index, uint8_t* kind, int32_t* split_rank,
                   uint64_t* totals, void* stream) {
    if (P <= 0 || !prune_mask || !scratch || !src_index || !kind || !split_rank || !totals) return EGS_ERR_ARG;
    uint32_t* flags = (uint32_t*)scratch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mask_flags, dim3((P + 255) / 256), dim3(256), 0, s, P, prune_mask, flags, flags + (size_t)P, flags + 2 * (size_t)P,
                       flags + 3 * (size_t)P);
    return plan_common(P, flags, scratch, src_index, kind, split_rank, totals, s);
}

int egs_densify_plan_dev(int capacity, const int32_t* active_count, const float* grad_accum, const float* denom, const float* scaling_raw,
                         const float* opacity_raw, const float* max_radii2D, const int32_t* generation, const void* is_object,
                         int is_object_is_float, const egs_densify_rules_dev* rules, void* scratch, int32_t* src_index, uint8_t* kind,
                         int32_t* split_rank, uint64_t* totals, void* stream) {
    if (capacity <= 0 || !active_count || !grad_accum || !denom || !scaling_raw || !opacity_raw || !max_radii2D || !generation || !is_object ||
        !rules || !scratch || !src_index || !kind || !split_rank || !totals)
        return EGS_ERR_ARG;
    uint32_t* flags = (uint32_t*)scratch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_densify_flags_dev, dim3((capacity + 255) / 256), dim3(256), 0, s, capacity, active_count, grad_accum, denom, scaling_raw,
                       opacity_raw, max_radii2D, generation, is_object, is_object_is_float, rules, flags, totals);
    return plan_common(capacity, flags, scratch, src_index, kind, split_rank, totals, s);
}

int egs_prune_plan_dev(int capacity, const int32_t* active_count, const uint8_t* prune_mask, void* scratch, int32_t* src_index, uint8_t* kind,
                       int32_t* split_rank, uint64_t* totals, void* stream) {
    if (capacity <= 0 || !active_count || !prune_mask || !scratch || !src_index || !kind || !split_rank || !totals) return EGS_ERR_ARG;
    uint32_t* flags = (uint32_t*)scratch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mask_flags_dev, dim3((capacity + 255) / 256), dim3(256), 0, s, capacity, active_count, prune_mask, flags, totals);
    return plan_common(capacity, flags, scratch, src_index, kind, split_rank, totals, s);
}

size_t egs_densify_apply_scratch_bytes(int capacity, int n_arrays, const int32_t* row_floats) {
    if (capacity <= 0 || n_arrays <= 0 || !row_floats) return 0;
    size_t floats = 0;
    for (int a = 0; a < n_arrays; a++) floats += row_floats[a] > 0 ? (size_t)row_floats[a] : 0;
    return (size_t)capacity * floats * sizeof(float);
}

int egs_densify_apply(int capacity, int32_t* active_count, const int32_t* src_index, const uint8_t* kind, const int32_t* split_rank,
                      const uint64_t* totals, const egs_densify_rules_dev* rules, int n_arrays, const egs_densify_array* arrays, int xyz_index,
                      int scaling_index, int rotation_index, const float* z, void* scratch, uint32_t* status, void* stream) {
    if (capacity <= 0 || !active_count || !src_index || !kind || !split_rank || !totals || !arrays || !scratch || !status) return EGS_ERR_ARG;
    if (n_arrays < 1 || n_arrays > EGS_DENSIFY_MAX_ARRAYS) return EGS_ERR_ARG;
    ApplyTable t;
    memset(&t, 0, sizeof(t));
    size_t off = 0;
    int max_d = 1;
    for (int a = 0; a < n_arrays; a++) {
        const egs_densify_array& in = arrays[a];
        if (!in.data || in.row_floats <= 0 || in.role < EGS_DENSIFY_PARAM || in.role > EGS_DENSIFY_TAG) return EGS_ERR_ARG;
        if (in.flags & ~(in.role == EGS_DENSIFY_TAG ? (EGS_DENSIFY_TAG_I32 | EGS_DENSIFY_TAG_CLONE_GEN) : 0)) return EGS_ERR_ARG;
        if ((in.flags & EGS_DENSIFY_TAG_CLONE_GEN) && !(in.flags & EGS_DENSIFY_TAG_I32)) return EGS_ERR_ARG;
        t.a[a].data = (uint32_t*)in.data; t.a[a].shadow = (uint32_t*)scratch + off; t.a[a].D = in.row_floats; t.a[a].role = in.role;
        t.a[a].flags = in.flags;
        off += (size_t)capacity * (size_t)in.row_floats;
        if (in.row_floats > max_d) max_d = in.row_floats;
    }
    if (rules) {                                                       // a densify plan can hold split children: their three arrays and the draws
        const int idx[3] = { xyz_index, scaling_index, rotation_index }, want[3] = { 3, 3, 4 };
        for (int k = 0; k < 3; k++)
            if (idx[k] < 0 || idx[k] >= n_arrays || arrays[idx[k]].role != EGS_DENSIFY_PARAM || arrays[idx[k]].row_floats != want[k]) return EGS_ERR_ARG;
        if (!z) return EGS_ERR_ARG;
        t.xyz = xyz_index; t.scaling = scaling_index; t.rotation = rotation_index;
    } else {
        z = nullptr; t.xyz = t.scaling = t.rotation = -1;
    }
    t.n = n_arrays;
    const size_t blocks = ((size_t)capacity * (size_t)max_d + 255) / 256;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)n_arrays);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_apply_gather, grid, dim3(256), 0, s, t, capacity, src_index, kind, split_rank, totals, rules, z);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_apply_commit, grid, dim3(256), 0, s, t, capacity, totals, rules, active_count, status);
    return (int)hipGetLastError();
}

int egs_gather_rows_f32(int64_t rows, int row_floats, const int32_t* src_index, const uint8_t* kind, int zero_new_rows, const float* in,
                        float* out, void* stream) {
    if (rows < 0 || row_floats < 0) return EGS_ERR_ARG;
    const size_t n = (size_t)rows * (size_t)row_floats;
    if (n == 0) return 0;
    if (!src_index || !kind || !in || !out) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_gather_rows_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, row_floats, src_index, kind,
                       zero_new_rows, in, out);
    return (int)hipGetLastError();
}

int egs_gather_i32(int64_t rows, const int32_t* src_index, const uint8_t* kind, int clone_value_on, int clone_value, const int32_t* in,
                   int32_t* out, void* stream) {
    if (rows < 0) return EGS_ERR_ARG;
    if (rows == 0) return 0;
    if (!src_index || !kind || !in || !out) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_gather_i32, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)rows, src_index, kind,
                       clone_value_on, clone_value, in, out);
    return (int)hipGetLastError();
}

int egs_split_children(int64_t rows, const int32_t* src_index, const uint8_t* kind, const int32_t* split_rank, int n_split, const float* z,
                       const float* xyz_old, const float* scaling_old, const float* rotation_old, float* xyz_new, float* scaling_new,
                       void* stream) {
    if (rows < 0 || n_split < 0) return EGS_ERR_ARG;
    if (rows == 0 || n_split == 0) return 0;
    if (!src_index || !kind || !split_rank || !z || !xyz_old || !scaling_old || !rotation_old || !xyz_new || !scaling_new) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_split_children, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)rows, src_index, kind,
                       split_rank, n_split, z, xyz_old, scaling_old, rotation_old, xyz_new, scaling_new);
    return (int)hipGetLastError();
}

}  // extern "C"
