/*
 * egs_raster.h -- C ABI of libegs_raster.so, the MI355X (gfx950) differentiable 3D Gaussian
 * tile rasterizer behind EgoGaussian's gaussian_renderer.render() path.
 *
 * What each entry point replaces.  The reference binds the CUDA extension
 * `diff_gaussian_rasterization._C` (an un-vendored submodule: ashawkey/diff-gaussian-rasterization
 * @ 8829d14f, /root/reference/README.md:26, /root/reference/.gitmodules:1-3) through the Python
 * surface imported at
 *     /root/reference/gaussian_renderer/__init__.py:14      (GaussianRasterizationSettings, GaussianRasterizer)
 *     /root/reference/gaussian_renderer/render_helper.py:3
 * and invoked at
 *     /root/reference/gaussian_renderer/__init__.py:90-98   (training call: shs + cov3D_precomp)
 *     /root/reference/gaussian_renderer/render_helper.py:61-63 (label call: colors_precomp + scales/rotations)
 *   egs_forward_geometry + egs_forward_render  <->  _C.rasterize_gaussians          (forward)
 *   egs_backward                                <->  _C.rasterize_gaussians_backward (backward)
 *   egs_mark_visible                            <->  _C.mark_visible
 *   egs_*_bytes / egs_*_layout                  <->  the three resizable byte buffers
 *                                                    (geomBuffer, binningBuffer, imgBuffer) the
 *                                                    upstream op allocates through callbacks
 * The forward is split in two because the number of (Gaussian, tile) instances R is data dependent:
 * egs_forward_geometry returns R on the host, the caller sizes the binning buffer, then calls
 * egs_forward_render.
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless marked HOST.  fp32, contiguous, row-major.
 *   - The library never allocates or frees device memory; every buffer is owned by the caller and must
 *     stay alive until the work enqueued on `stream` has completed.
 *   - The opaque geometry / binning / image buffers must start at 256-byte-aligned addresses (hipMalloc and the PyTorch allocator
 *     give at least that); a misaligned one is refused with EGS_ERR_ARG.  Their layouts place every array at a 256-byte offset.
 *   - Process-wide state, all of it: (1) the optional profiling pool (egs_profile_begin / egs_profile_end), off by
 *     default; (2) the result of the one-time device check behind the tile sort's ranker (an atomic int: a property of
 *     the hardware, the same for every caller); (3) one hipEvent per calling thread inside egs_forward (thread_local).
 *     Nothing else is kept between calls -- no switches, no registry of buffers (ABI 6: what were process-wide debug
 *     switches through ABI 5 are bits of the call's own flags word, EGS_CALL_* below; a placement buffer is initialised
 *     by its owner, egs_placement_init).  Concurrent calls on different streams / threads with different settings are safe.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it.  egs_forward_geometry is
 *     the only call that waits on the stream (one 8-byte device->host read of R).
 *   - Matrices use the reference's row-vector layout (/root/reference/scene/cameras.py:67-69):
 *     viewmatrix = W2V^T, projmatrix = W2V^T * P^T, 16 floats each.
 *   - Optional inputs are NULL when absent: exactly one of {shs, colors_precomp} and exactly one of
 *     {cov3D_precomp, (scales, rotations)} must be non-NULL.
 *   - Return value: 0 on success; EGS_ERR_* (negative) for argument errors; a positive hipError_t if
 *     the HIP runtime reported one.  Nothing throws across this boundary.
 *   - The last argument of every compute entry point (`debug`; `flags` on egs_forward_enqueue) is a set of EGS_CALL_* bits.  Bit 0
 *     (EGS_CALL_SYNC -- what debug != 0 meant through ABI 5) synchronises the stream and checks for errors after every kernel.
 */
#ifndef EGS_RASTER_H
#define EGS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_ABI_VERSION 6          /* 6: per-call flags (EGS_CALL_*) instead of the process-wide egs_debug_set_* switches, egs_forward_enqueue takes a flags word,
                                         egs_placement_init is the ONLY thing that clears a placement buffer's sums region (no registry of addresses);
                                         5: the placement buffer grew a sums region (egs_placement_bytes) that must be ZERO when the buffer is first handed over:
                                         egs_placement_init;  4: grad_mask on the backwards, egs_l1_ssim_pair_*, out_depth / out_alpha may both be NULL on every
                                         forward (colour only) */
#define EGS_TILE 16                 /* tile edge in pixels; part of the parity contract */

/* Per-call flags (ABI 6).  None of them but EGS_CALL_DETERMINISTIC (see there) changes an output value: colour, depth, alpha, radii, final transmittance and every gradient are
 * bit-identical whatever the bits; they select which launches produce them (and, for KEEP_ALL_INSTANCES, what the internal lists hold). */
#define EGS_CALL_SYNC               0x01   /* synchronise the stream and check for errors after every kernel (debugging) */
#define EGS_CALL_KEEP_ALL_INSTANCES 0x02   /* no tile culling.  By default an instance (splat, tile) of the reference's 3-sigma rectangle is dropped
                                              when no pixel of the tile can receive alpha >= 1/255 from the splat (exact, conservative ellipse-vs-tile
                                              test): the reference skips such an instance at every pixel, so only the internal lists (binning buffer,
                                              per-pixel contributor positions) get shorter; `num_rendered` stays the reference's count.  With this bit
                                              every instance is kept and the lists are comparable bit for bit with the reference algorithm's (parity
                                              tests).  Give the SAME bit to the forward and to nothing else: the backward reads the lists as they are. */
#define EGS_CALL_SEPARATE_COUNT     0x04   /* the count pass of the tile bucketing as a launch of its own even when a placement buffer would let it
                                              ride in the preprocess launch (A/B measurements, tests) */
#define EGS_CALL_SEPARATE_SORT      0x08   /* the per-tile sort as launch(es) of its own instead of inside the forward blend's launch */
#define EGS_CALL_BALLOT_RANK        0x10   /* the per-tile sort ranks keys with the ballot-based fallback instead of the LDS atomic whose lane-order
                                              behaviour is verified on the device once per process (test hook: covers the fallback) */
#define EGS_CALL_DETERMINISTIC      0x20   /* backwards only (added within ABI 6; forwards ignore it): order-independent gradient sums.  By default the
                                              quadrant-waves of the backward blend add their per-splat partial sums into the Gaussian's accumulator
                                              line with float atomics, in an order that differs from run to run, so gradients differ in their last
                                              bits.  With this bit -- honoured by egs_backward, egs_backward_adam, egs_backward_lossgrad,
                                              egs_backward_object_lossgrad, egs_backward_entropy_lossgrad and egs_backward_label, in every blend mode --
                                              the blend runs twice: the first pass gathers the largest |partial| of every (Gaussian, value) pair with an
                                              integer atomic max, the second adds the partials as int64 multiples of a quantum <= 2^-38 of that
                                              maximum, and the sum becomes a float32 once (csrc/det_accum.h).  Every output of the call -- dL_d*, the
                                              densification statistics, what a sink steps, dL/dA12, dL/dM9, dL/dlabel -- is then a pure function of
                                              the call's inputs: the same bits run to run, eager or replayed from a hipGraph.  The ONE flag that
                                              changes output values: by at most the rounding of the float chain it replaces (N q / 2 + half an ulp
                                              per pair; the default path's bars hold).  A pair that received an Inf or NaN partial comes back NaN.
                                              PRECONDITION: `scratch` holds egs_backward_scratch_bytes_ex(P, flags) bytes -- more than
                                              egs_backward_scratch_bytes(P); also when a loss launch prepared it (egs_backward_prologue.scratch). */
#define EGS_MAX_SH_DEGREE 3

#define EGS_ERR_ARG        (-1)     /* NULL / inconsistent arguments */
#define EGS_ERR_MODE       (-2)     /* colour or covariance mode not "exactly one of" */
#define EGS_ERR_RANGE      (-3)     /* size outside supported range (image side > 32767 px or > 36864 tiles, R >= 2^31, degree > 3) */
#define EGS_ERR_NO_DEVICE  (-4)     /* no HIP device / wrong architecture */
#define EGS_RETRY_LARGER   (-100)   /* egs_forward only: capacity guess too small, nothing rendered; *num_rendered holds R */

int         egs_abi_version(void);
const char* egs_source_hash(void);      /* hash of the sources this library was built from (csrc/Makefile); "unknown" if built by hand */
const char* egs_error_string(int code);
/* Name of the device the current HIP context runs on and its gcnArchName; returns 0 or an error. */
int         egs_device_info(char* name, int name_len, char* arch, int arch_len, int* compute_units);

/* ---- buffer sizes (bytes) -------------------------------------------------------------------- */
size_t egs_geom_bytes(int P);
size_t egs_binning_bytes(int P, int64_t R, int width, int height);
size_t egs_image_bytes(int width, int height);
size_t egs_backward_scratch_bytes(int P);      /* the scratch itself: 64-byte aligned (one 64-byte accumulator line per Gaussian; EGS_ERR_ARG otherwise) */
/* the same for a backward called with `flags` (EGS_CALL_* bits): == egs_backward_scratch_bytes(P) unless EGS_CALL_DETERMINISTIC is among them,
 * which adds the mode's lines (12 P uint32 maxima + 12 P int64 sums, rounded up to 256 bytes) behind the float accumulator */
size_t egs_backward_scratch_bytes_ex(int P, int flags);
/* words of a tile-order array (image layout `tile_order`; second part of the placement buffer, behind 4 words per tile): one per
 * workgroup of a blend launch -- 8 XCD bands of equal slot counts, 0xffffffff = padding workgroup */
int    egs_order_words(int width, int height);

/* ---- buffer layouts, for tests and tools: byte offsets of the named sub-arrays ----------------- */
typedef struct egs_geom_layout {
    size_t rec;            /* float4[P][3]  packed splat record (csrc/egs_common.h): (x, y, qa, qb | qc, opacity, red, green |
                              blue, depth, bits(bbox_x = x0 | x1<<16), bits(bbox_y = y0 | y1<<16)) with (qa, qb, qc) =
                              (-conA/2, -conB, -conC/2) * log2(e), the conic pre-scaled for v_exp_f32 */
    size_t rect;           /* uint32[P][2]  tile rect: (x0 | x1<<16, y0 | y1<<16) */
    size_t offsets;        /* uint32[P]     tiles touched by each Gaussian (0 = culled) */
    size_t clamped;        /* uint8[P]      bit c set <=> colour channel c was clamped at 0 */
    size_t visible;        /* uint8[P]      1 <=> radii > 0 (the renderer's visibility_filter without a compare kernel) */
    size_t scan_scratch;   /* uint32[ceil(P/256)] per-workgroup instance counts (their sum is R) */
    size_t total;          /* reserved */
} egs_geom_layout;
typedef struct egs_binning_layout {
    size_t point_list;     /* uint32[R]  Gaussian indices ordered by (tile, depth bits, index); ALWAYS at offset 0 */
    size_t pairs;          /* uint64[R]  (float bits of depth << 32 | Gaussian index), bucketed by tile */
    size_t scratch;        /* uint64[R]  ping-pong space for buckets too large for the in-register sort */
    size_t table;          /* uint32[tiles][table_stride] per-(tile, bucketing workgroup) counts, exclusive-scanned in place; columns >= bin_blocks unused */
    size_t spine;          /* uint32[..] sums of the table's 2048-entry scan chunks (8 partial accumulators each), scratch words */
    size_t total;          /* uint64[1]  instance count found by the bucketing scan (== R; may exceed a speculative capacity) */
    int    bin_blocks;     /* workgroups of the bucketing kernels: ceil(P / gpb), gpb = 1024 * ceil(P / 524288) */
    int    key_bits;       /* significant bits of the canonical (tile<<32 | depth) key: 32 + bits(tile count) */
    int    index_passes;   /* 9-bit radix passes on the Gaussian index inside the per-tile sort, run only for tiles with depth ties
                             (+ up to 4 on depth: ceil(bits(zmax - zmin of the tile) / 9)) */
    int    table_stride;   /* row length of `table`: the power of two >= max(bin_blocks, 4) */
} egs_binning_layout;
typedef struct egs_image_layout {
    size_t ranges;         /* uint32[tiles][2] */
    size_t final_T;        /* float[H*W] */
    size_t n_contrib;      /* uint32[H*W] */
    size_t quad_work;      /* uint32[tiles][4] estimated backward cost of every 8x8 quadrant (blended splats and list batches), written by the forward */
    size_t tile_order;     /* uint32[8*ceil(tiles/8)] tile handled by each workgroup of the backward blend */
    size_t quad_pairs;     /* uint32[tiles][4] (pixel, splat) pairs every 8x8 quadrant blended (alpha >= 1/255, before saturation) and,
                              in the upper array uint32[tiles][4] right after it, the (wave, splat) visits it made -- measurement only
                              (bench.py: pair throughput Q/s) */
} egs_image_layout;
int egs_get_geom_layout(int P, egs_geom_layout* out);
int egs_get_binning_layout(int P, int64_t R, int width, int height, egs_binning_layout* out);
int egs_get_image_layout(int width, int height, egs_image_layout* out);

/* ---- forward, part 1: per-Gaussian geometry + instance count  (upstream: preprocess + InclusiveSum) ------ */
/* Raw-parameter mode.  The reference activates its parameters with three PyTorch ops before every render
 * (/root/reference/scene/gaussian_model.py:36-44: scaling exp, rotation normalize, opacity sigmoid).  With these flags the
 * forward applies them inside the preprocess kernel and the backward returns the gradients w.r.t. the RAW tensors:
 *   EGS_ACT_LOG_SCALES     `scales` holds log-scales            (only with scales + rotations, not with cov3D_precomp)
 *   EGS_ACT_RAW_QUATS      `rotations` is not normalised        (likewise)
 *   EGS_ACT_LOGIT_OPACITY  `opacities` holds logits
 * Pass the SAME flags to the forward and to egs_backward. */
/* Split spherical harmonics.  The reference keeps the colour coefficients as two parameters, _features_dc [P,1,3] and
 * _features_rest [P,M-1,3], and concatenates them before every render (/root/reference/scene/gaussian_model.py:157-160
 * get_features); autograd splits the gradient again.  With shs_rest != NULL, `shs` is the DC block [P,1,3] and `shs_rest` the
 * remaining [P,M-1,3] (sh_coeffs is still M >= 2); egs_backward then writes dL_dsh [P,1,3] and dL_dsh_rest [P,M-1,3]. */
#define EGS_ACT_LOG_SCALES 1
#define EGS_ACT_RAW_QUATS 2
#define EGS_ACT_LOGIT_OPACITY 4
/* Object rotation inside the rasterizer (ABI 2 addition).  The `fine_all` trainer renders with the covariance of the object's Gaussians
 * rotated by the accumulated object motion: render(..., rot_cov=True, accum_R, which_object)
 * (/root/reference/trainers/fine_all.py:88-93, /root/reference/scene/gaussian_model.py:46-63: L = R S, L <- M L for the selected rows,
 * Sigma = L L^T), which upstream can only be given as cov3D_precomp.  With `rot` the forward builds that covariance itself from
 * scales + rotations (any activation flags) and the backward chains through M: no [P,6] covariance in HBM either way, no producer
 * launches, and the raw parameters stay eligible for egs_backward_adam.  M is a constant of the loss (no gradient is produced for
 * it; a trainable object rotation goes through cov3D_precomp / egs_cov3d_*).  Same arithmetic, operation for operation, as
 * egs_cov3d_forward / egs_cov3d_backward.  NULL = no rotation.  Pass the same to the forward and to egs_backward_adam. */
typedef struct egs_object_rotation {
    const float* M9;                  /* device float[9], row-major 3x3 */
    const uint8_t* selected;          /* device uint8[P]: rows to rotate; NULL = every row */
    float row0_grad_mult;             /* gradient multiplier of row 0 when it is rotated: the reference's [N,1]-index quirk
                                         (egogaussian_amd/covariance.py), 1 = none */
    const float* row0_grad_mult_dev;  /* device float[1] used instead of row0_grad_mult, or NULL */
} egs_object_rotation;
/* Rigid object motion inside the rasterizer (ABI 6 addition).  Every stage after the static one poses the object's Gaussians per frame
 * (gaussians.apply_trans_rot_new before render(..., rot_cov=True, accum_R, which_object), reverse_trans_rot_new after it:
 * /root/reference/trainers/coarse_obj_pose.py:229-239,313-317, /root/reference/trainers/fine_all.py:88-116).  With EGS_ACT_OBJECT_MOTION among the
 * activation flags the `rot` argument of egs_forward_geometry, egs_forward, egs_forward_enqueue, egs_backward_adam and egs_backward_lossgrad
 * points to an egs_object_motion instead: the preprocess kernels place the moved rows, p' = A p + b (see egs_object_move_points below for the
 * arithmetic and for why `moved` is not `rot.selected`), every later stage sees the placed position, and the backward
 *   - writes dL_dmeans3D -- and steps EGS_SINK_MEANS3D -- with the gradient of the CANONICAL position, A^T dL/dp' for a moved row;
 *   - with `grad`, writes dL/dA12 (12 floats in A12's layout) and dL/dM9 (9 floats; zeros without rot.M9) as a deterministic reduction:
 *     per-workgroup lines in `scratch`, one finish launch, no float atomics.  dL/dM9 is k_cov3d_backward's gM operation for operation,
 *     the row-0 multiplier included.  Without `grad` (a constant pose) the backward makes no shuffle and no extra launch.
 * The motion of the positions works with every covariance input (cov3D_precomp too); rot.M9 under egs_object_rotation's conditions.
 * Bit set with A12 == NULL, or grad without scratch: EGS_ERR_ARG before any device work; bit set with rot == NULL: EGS_ERR_MODE.  egs_backward (no `rot` argument)
 * does not take the bit.  Pass the same flags and struct to the forward and to the backward.  Callers that do not set the bit are untouched. */
#define EGS_ACT_OBJECT_MOTION 8
typedef struct egs_object_motion {
    egs_object_rotation rot;      /* first member; rot.M9 == NULL: covariances are not turned */
    const float*   A12;           /* device float[12], row-major 3x4 [A | b]; required */
    const uint8_t* moved;         /* device uint8[P] or NULL = every row */
    float*         grad;          /* device float[21] out (dL/dA12 [12] in A12's layout, dL/dM9 [9]) or NULL */
    void*          scratch;       /* egs_object_motion_scratch_bytes(P), needed with grad */
} egs_object_motion;
int egs_forward_geometry(
    int P, int sh_degree, int sh_coeffs /* M: coefficients per channel in `shs` */,
    const float* means3D /*[P,3]*/, const float* shs /*[P,M,3] or NULL*/, const float* shs_rest /*see below; normally NULL*/,
    const float* colors_precomp /*[P,3] or NULL*/,
    const float* opacities /*[P]*/, const float* scales /*[P,3] or NULL*/, float scale_modifier,
    const float* rotations /*[P,4] or NULL*/, const float* cov3D_precomp /*[P,6] or NULL*/, int activation_flags /*EGS_ACT_*, 0 = none*/,
    const float* viewmatrix /*[16]*/, const float* projmatrix /*[16]*/, const float* campos /*[3]*/,
    int width, int height, float tan_fovx, float tan_fovy, int prefiltered,
    int32_t* radii /*[P] out*/, void* geom_buffer, int64_t* num_rendered /*HOST out: R*/,
    const int32_t* active_count /*device int32[1] or NULL; see "capacity-sized models" below*/,
    const egs_object_rotation* rot /*HOST or NULL*/, void* stream, int debug);

/* ---- forward, part 2: bucket instances by tile, sort each tile by (depth, index), blend
 *      (upstream: duplicateWithKeys, SortPairs, identifyTileRanges, render) ------------------------ */
/* R here (and in egs_backward) is the instance count the binning buffer was laid out for: the exact count from
 * egs_forward_geometry, or the `capacity` given to egs_forward. */
int egs_forward_render(
    int P, int64_t R, const float* background /*[3]*/, int width, int height,
    const void* geom_buffer, void* binning_buffer, void* image_buffer,
    float* out_color /*[3,H,W]*/, float* out_depth /*[1,H,W]*/, float* out_alpha /*[1,H,W]*/,
    void* stream, int debug);

/* Capacity-sized models (ABI 2).  A trainer that densifies / prunes every 100 iterations
 * (/root/reference/scene/gaussian_model.py:565-586,678-709) can keep its arrays at a fixed CAPACITY of P rows and the number
 * of live Gaussians in a device word: with active_count != NULL rows i >= *active_count are treated as culled (radii 0, no
 * instances, zero gradients), whatever their contents.  P, every launch size and every buffer layout then stay fixed while
 * the model grows and shrinks, so a hipGraph captured around the step survives densification.  NULL: all P rows are live.
 *
 * Overflow word (ABI 2).  egs_forward_enqueue cannot report a too-small `capacity` to the host; with overflow_flag != NULL
 * (device uint32[2]) the chain WRITES [0] = 1 when this frame needed more than `capacity` instances (its image is then
 * clipped and invalid), else 0, and [1] = the number of instances the frame bucketed.  Passed on as `skip_flag` to egs_backward and egs_adam_step_capturable it makes the
 * rest of a captured training step a no-op for that frame: no densification statistics, no parameter, moment or step-count
 * update -- every optimizer step follows a complete render, as in the reference (trainers/train_static.py:110-138). */

/* ---- forward in ONE call, without a GPU bubble.  Same work as egs_forward_geometry + egs_forward_render, but the
 *      binning and blend kernels are enqueued against `capacity` (the caller's guess of R, e.g. 1.25 x the largest R seen
 *      so far; layout = egs_binning_bytes(P, capacity, ...)) before R is known, and the host waits only for the copy of
 *      the per-workgroup instance counts into `pinned_host_counts` (page-locked host memory, >= ceil(P/256) uint32).
 *      Returns 0 with *num_rendered = R when R <= capacity.  Returns EGS_RETRY_LARGER with *num_rendered = R when the guess
 *      was too small (or capacity == 0): nothing valid was rendered; allocate a binning buffer for >= R instances and call
 *      egs_forward_render(P, that_size, ...).  Keeps one hipEvent per calling thread. */
int egs_forward(
    int P, int sh_degree, int sh_coeffs,
    const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, int activation_flags,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* background,
    int width, int height, float tan_fovx, float tan_fovy, int prefiltered,
    int32_t* radii /*[P] out*/, void* geom_buffer, int64_t capacity, void* binning_buffer, void* image_buffer,
    float* out_color, float* out_depth, float* out_alpha, uint32_t* pinned_host_counts /*HOST, page-locked*/,
    int64_t* num_rendered /*HOST out*/, const int32_t* active_count /*device int32[1] or NULL*/,
    void* placement /*egs_placement_bytes(width, height) or NULL; see below*/, const egs_object_rotation* rot /*HOST or NULL*/,
    void* stream, int debug);

/* Placement buffer (ABI 2 addition).  The forward blend runs one workgroup per tile, all resident at once, so the launch lasts as
 * long as its busiest SIMD; which tiles share a CU / SIMD is free.  `placement` is caller-owned device memory that PERSISTS between
 * calls: every forward leaves there what its blend spent on each 8x8 quadrant, and the next forward given the same buffer deals its
 * tiles to CUs and its quadrants to SIMDs by those numbers (an ordering job carried by the preprocess launch).  It pays when
 * consecutive calls render similar frames -- a video or an orbit in order, the static buffers of a replayed hipGraph -- and is neutral
 * otherwise.  One buffer per concurrently running forward (it is read and written by the call).  NULL: the static tile mapping.
 * ABI 5: given a placement buffer, the forward also folds the count pass of its tile bucketing into the preprocess launch (one launch and
 * one round of set-up loads less per frame); that pass accumulates per-chunk instance sums in the tail of the buffer, which the chain
 * itself clears again before it ends.  Those words must therefore be ZERO when a forward starts: the owner calls egs_placement_init()
 * (one small launch on `stream`) ONCE per buffer and image size -- after allocating it, and again before using it for another image size
 * (the region's offset follows the tile count) -- and does not use the memory for anything else between calls.  The library keeps no
 * record of buffers (ABI 6): a forward that finds stale sums counts wrongly.  A forward that fails half way clears the words itself before
 * it returns its error.  The cost and tile-order words in front of the sums may hold anything -- they decide when a quadrant is blended,
 * never what is computed.  Results are identical with and without a placement buffer. */
size_t egs_placement_bytes(int width, int height);
int egs_placement_init(void* placement, int width, int height, void* stream);

/* ---- the same chain with NO host wait, for hipGraph capture of a whole training step: everything is only enqueued
 *      (capacity must be > 0).  A frame that needs more than `capacity` instances is invalid (its kernels were clipped to
 *      the capacity) and must be redone with a larger buffer; the caller finds out after synchronising, from either of
 *        pinned_host_counts   optional (NULL: no copy): the per-workgroup rectangle counts, R = egs_sum_counts(P, ..); when
 *                             `overflow_flag` is given as well the buffer holds ceil(P/256) + 2 words and the two overflow words
 *                             ([0] this frame was clipped, [1] instances bucketed) are copied behind the counts at the end of the
 *                             chain -- what an EAGER loop needs to check the frame at its next call instead of waiting now
 *        running_max          optional device uint64: raised by the chain to the number of instances it bucketed whenever
 *                             that is larger, so one word tells whether ANY replay so far overflowed. */
int egs_forward_enqueue(
    int P, int sh_degree, int sh_coeffs,
    const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, int activation_flags,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* background,
    int width, int height, float tan_fovx, float tan_fovy, int prefiltered,
    int32_t* radii, void* geom_buffer, int64_t capacity, void* binning_buffer, void* image_buffer,
    float* out_color, float* out_depth, float* out_alpha, uint32_t* pinned_host_counts, uint64_t* running_max,
    const int32_t* active_count /*device int32[1] or NULL*/, uint32_t* overflow_flag /*device uint32[2] out or NULL*/,
    void* placement /*or NULL*/, const egs_object_rotation* rot /*HOST or NULL*/, void* stream, int flags /*EGS_CALL_*; EGS_CALL_SYNC is ignored: nothing may wait*/);
int64_t egs_sum_counts(int P, const uint32_t* pinned_host_counts /*HOST*/);

/* ---- backward  (upstream: render backward + computeCov2D backward + preprocess backward) ------- */
/* grad_mask (ABI 4): which inputs' gradients the caller is going to read -- autograd's ctx.needs_input_grad.  EGS_GRAD_ALL (0) = all of
 * them, the behaviour of ABI <= 3.  The library uses it to skip work; the one combination it acts on today is colors_precomp given and
 * grad_mask == EGS_GRAD_COLORS -- the reference's label call, which detaches every geometric input
 * (/root/reference/gaussian_renderer/render_helper.py:38-54; 30 000 times in /root/reference/trainers/train_static.py:105-109): the
 * blend then accumulates w * dL/dC only (no dL/dalpha recurrence, no moments, no background term), the preprocess backward is not
 * launched, ONLY dL_dcolors is written and every other dL_d* output may be NULL.  Any other mask: everything is computed and every
 * output must be given as before. */
#define EGS_GRAD_ALL        0
#define EGS_GRAD_MEANS3D    1
#define EGS_GRAD_MEANS2D    2
#define EGS_GRAD_SH         4
#define EGS_GRAD_COLORS     8
#define EGS_GRAD_OPACITY    16
#define EGS_GRAD_SCALES     32
#define EGS_GRAD_ROTATIONS  64
#define EGS_GRAD_COV3D      128
#define EGS_GRAD_MASK_BITS  255
int egs_backward(
    int P, int sh_degree, int sh_coeffs, int64_t R,
    const float* background, const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, int activation_flags,
    const float* viewmatrix, const float* projmatrix, const float* campos,
    int width, int height, float tan_fovx, float tan_fovy,
    const int32_t* radii, const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
    const float* dL_dout_color /*[3,H,W]*/, const float* dL_dout_depth /*[1,H,W] or NULL*/,
    const float* dL_dout_alpha /*[1,H,W] or NULL*/,
    float* dL_dmeans2D /*[P,3] out, NDC-scaled (x 0.5*W, 0.5*H), z = 0*/,
    float* dL_dcolors /*[P,3] out*/, float* dL_dopacity /*[P] out*/, float* dL_dmeans3D /*[P,3] out*/,
    float* dL_dcov3D /*[P,6] out; may be NULL with scales + rotations*/, float* dL_dsh /*[P,M,3] out or NULL*/,
    float* dL_dsh_rest /*[P,M-1,3] out with shs_rest (dL_dsh is then [P,1,3]), else NULL*/,
    float* dL_dscales /*[P,3] out or NULL*/, float* dL_drotations /*[P,4] out or NULL*/,
    /* Optional (all NULL = off): the trainer's per-iteration densification statistics updated IN PLACE by the same launch that
     * produces dL_dmeans2D -- for Gaussians with radii > 0: grad_accum[i] += |dL_dmeans2D[i, :2]|, denom[i] += 1
     * (/root/reference/scene/gaussian_model.py:735-737) and max_radii[i] = max(max_radii[i], radii[i])
     * (/root/reference/trainers/train_static.py:125).  Same arithmetic as egs_densify_stats, one launch less per iteration. */
    float* stat_grad_accum /*[P] in/out or NULL*/, float* stat_denom /*[P] in/out or NULL*/, float* stat_max_radii /*[P] in/out or NULL*/,
    const uint32_t* skip_flag /*device uint32[1] or NULL: non-zero = leave the three statistics untouched (overflowed frame)*/,
    int grad_mask /*EGS_GRAD_* bits, 0 = all (see above)*/,
    void* scratch /* egs_backward_scratch_bytes(P) */, void* stream, int debug);

/* ---- backward with the optimizer inside (ABI 2 addition; no upstream counterpart: upstream returns the gradients to autograd
 *      and torch.optim.Adam reads them back, /root/reference/trainers/train_static.py:97,137).
 * egs_backward_adam is egs_backward plus, for every LEAF the sink owns, the Adam step of that leaf taken by the kernel that
 * produces its gradient: the gradient never reaches HBM, the parameter is not read again by an optimizer launch, and the training
 * step has one launch less.  Arithmetic and results are those of egs_adam_step_capturable, bit for bit.
 *   - A leaf is one of the five per-Gaussian inputs below; `param` must be the SAME device array the call receives as that input
 *     (for EGS_SINK_OPACITY: the array the forward received as `opacities`; the backward itself reads the activated value from the
 *     geometry buffer).  It is updated IN PLACE after its last read; exp_avg / exp_avg_sq have its shape, lr / step are device float[1]:
 *     torch's state["step"], advanced by one per call.  param == NULL: that leaf is not fused.
 *   - The dL_d* output of a fused leaf may be NULL (nothing written); if given, the gradient is written as well.
 *   - Conditions (else EGS_ERR_MODE): EGS_SINK_SCALES / EGS_SINK_ROTATIONS need scales + rotations (not cov3D_precomp).
 *     Colour: either `shs` with sh_coeffs == 1 and no shs_rest (EGS_SINK_SH, and EGS_SINK_MEANS3D is then stepped by the same
 *     kernel as the others), or split spherical harmonics with sh_coeffs == 16 and 16-byte aligned arrays: EGS_SINK_SH (the DC
 *     block), EGS_SINK_SH_REST and EGS_SINK_MEANS3D are then stepped by the spherical-harmonics launch that finishes their gradients
 *     (dL_dmeans3D must be given: it carries the partial gradient between the two launches); with `colors_precomp` only
 *     EGS_SINK_MEANS3D of the three.  Any other colour layout: those three leaves cannot be fused.
 *   - skip_flag set: no step is taken and none is counted.  active_rows: rows >= *active_rows are left alone (capacity-sized
 *     models), as in egs_adam_step_capturable.
 *   - coef: device float[12] scratch owned by the caller, written and read by this call only.
 *   - CALLER-CHECKED PRECONDITION (the library cannot see the caller's computation graph): the gradient this backward produces for a
 *     fused leaf must be the leaf's WHOLE gradient for this optimizer step -- this rasterizer call is the only consumer of the
 *     parameter in the loss.  A second path (colours computed from the positions outside the library, a second render of the same
 *     model in the same iteration, a regulariser written in torch on a fused leaf) would have its share applied with stale moments
 *     or lost.  ONE second path the library takes itself: the static stages' entropy term on the visible opacities, whose share joins
 *     dL/dopacity inside the preprocess backward, ahead of the sigmoid chain and of the Adam step (egs_backward_entropy_lossgrad
 *     below) -- ask for it there instead of adding it outside.
 *     The Python host side enforces the rest where it can (optim.FusedAdam.make_sink leaves the positions out when colors_precomp
 *     requires a gradient; FusedAdam.step raises when a fused leaf arrives with a .grad from another path); a direct C caller owns the check. */
#define EGS_SINK_MEANS3D   0    /* [P,3] */
#define EGS_SINK_OPACITY   1    /* [P,1] */
#define EGS_SINK_SCALES    2    /* [P,3] */
#define EGS_SINK_ROTATIONS 3    /* [P,4] */
#define EGS_SINK_SH        4    /* [P,1,3]: `shs` when it has one coefficient, or the DC block of split spherical harmonics */
#define EGS_SINK_SH_REST   5    /* [P,15,3]: `shs_rest` of split spherical harmonics with sh_coeffs == 16 */
typedef struct egs_adam_leaf {
    float* param; float* exp_avg; float* exp_avg_sq;
    const float* lr;     /* device float[1] */
    float* step;         /* device float[1], in/out */
} egs_adam_leaf;
typedef struct egs_adam_sink {
    egs_adam_leaf leaf[6];       /* indexed by EGS_SINK_* */
    float beta1, beta2, eps;
    float* coef;                 /* device float[12] scratch */
    const int32_t* active_rows;  /* device int32[1] or NULL */
} egs_adam_sink;
int egs_backward_adam(
    int P, int sh_degree, int sh_coeffs, int64_t R,
    const float* background, const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, int activation_flags,
    const float* viewmatrix, const float* projmatrix, const float* campos,
    int width, int height, float tan_fovx, float tan_fovy,
    const int32_t* radii, const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
    const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha,
    float* dL_dmeans2D, float* dL_dcolors /*may be NULL with shs*/, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
    float* dL_dsh_rest, float* dL_dscales, float* dL_drotations,
    float* stat_grad_accum, float* stat_denom, float* stat_max_radii, const uint32_t* skip_flag,
    const egs_adam_sink* sink /*HOST; NULL = no leaf is fused*/,
    int prologue_done /*non-zero: egs_l1_ssim_backward_ex carried this frame's egs_backward_prologue (same scratch, same sink)*/,
    const egs_object_rotation* rot /*HOST or NULL: as given to the forward*/,
    int grad_mask /*as egs_backward; the colours-only path is taken only with sink == NULL*/,
    void* scratch, void* stream, int debug);

/* ---- frustum test only  (upstream: markVisible) -------------------------------------------------- */
int egs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present /*[P] out, 0/1*/, void* stream);

/* ==== "next" rows of SURVEY.md section 8f: the callers either side of the rasterizer ======================= */

/* ---- f-1: fused 3D covariance producer.  Replaces build_scaling_rotation / strip_symmetric
 *      (/root/reference/utils/general_utils.py:110-156) and the covariance activations
 *      (/root/reference/scene/gaussian_model.py:29-33,46-63):
 *      q <- q/|q|; L = R(q) diag(scale_modifier * scaling); rows with selected[i] != 0 (all rows if selected == NULL)
 *      get L <- M L when M9 != NULL; cov6 = unique entries of L L^T in the order (00,01,02,11,12,22).
 *      scaling_is_log != 0: `scaling` holds the raw parameters and the scaling activation exp() (gaussian_model.py:36) is
 *      applied by the kernel; the backward then returns the gradient w.r.t. the raw parameters.
 *      opacity_raw != NULL: the same launch also applies the opacity activation, opacity[i] = sigmoid(opacity_raw[i])
 *      (gaussian_model.py:40), and the backward turns dL/dopacity into dL/dopacity_raw -- two elementwise launches less per step. */
int egs_cov3d_forward(int N, const float* scaling /*[N,3]*/, int scaling_is_log, float scale_modifier, const float* rotation /*[N,4] raw*/,
                      const float* M9 /*[9] device, row-major, or NULL*/, const uint8_t* selected /*[N] or NULL*/,
                      float* cov6 /*[N,6] out*/, const float* opacity_raw /*[N] or NULL*/, float* opacity /*[N] out or NULL*/,
                      void* stream);
/* row0_grad_mult reproduces the reference's duplicated-index gradient on Gaussian 0 (egogaussian_amd/covariance.py);
 * pass 1.0 otherwise; row0_grad_mult_dev (device float[1], may be NULL) overrides it with a value computed on the device, so
 * that the caller needs no host read of the selection count.  dL_dM9 (device [9], may be NULL) is written by the callee; when it is requested, dM_scratch must
 * provide egs_cov3d_dm_scratch_floats(N) floats (per-workgroup partial sums, no atomics). */
size_t egs_cov3d_dm_scratch_floats(int N);
int egs_cov3d_backward(int N, const float* scaling, int scaling_is_log, float scale_modifier, const float* rotation, const float* M9,
                       const uint8_t* selected, float row0_grad_mult, const float* row0_grad_mult_dev, const float* dL_dcov6 /*[N,6]*/,
                       float* dL_dscaling /*[N,3] out*/, float* dL_drotation /*[N,4] out*/, float* dL_dM9, float* dM_scratch,
                       const float* opacity /*[N] forward output or NULL*/, const float* dL_dopacity /*[N]*/,
                       float* dL_dopacity_raw /*[N] out*/, void* stream);

/* ---- rigid object motion of the positions (ABI 6 addition; additions only).  Every EgoGaussian stage after the static one poses the
 *      object's Gaussians per frame: gaussians.apply_trans_rot_new(...) rebuilds _xyz out of place before the render
 *      (/root/reference/scene/gaussian_model.py:939-986: torch.where(is_object == which, apply_T_xyz(T, xyz), xyz), with the trainable
 *      ObjectMove on top during training, /root/reference/utils/geometry_utils.py:14-33,188-193) and reverse_trans_rot_new(...) undoes
 *      it through a matrix inverse afterwards (gaussian_model.py:1037-1060).  Here the pose is an INPUT: for a moved row
 *          p'_i = A p_i + b          A12 = [A | b], device float[12], row-major 3x4; three fused multiply-adds per component
 *      and nothing is mutated, so there is nothing to reverse.  Backward, with g_i = dL/dp'_i:
 *          dL/dp_i = A^T g_i  (moved rows; g_i for the others)      dL/dA12 = sum over the moved rows of [g_i p_i^T | g_i]
 *      `moved` (device uint8[P], NULL = every row) is the EXACT mask of the reference's torch.where -- it is NOT the `selected` of
 *      egs_object_rotation, which carries the reference's [N,1]-index quirk (row 0).  Rows at or beyond *active_count
 *      (capacity-sized models) are never moved and never summed.  How A12 is composed from the accumulated and the trainable pose
 *      (A = R_t A_f, b = R_t b_f + t, the 6-D -> matrix map) is 3x3 algebra the caller does; autograd carries dL/dA12 on from there.
 *      The pose gradient is a deterministic reduction: per-workgroup lines (six __shfl_xor levels, four waves through LDS: an eight-deep
 *      float32 tree) in `scratch`, then one finish workgroup that adds the lines in index order in float64.  No float atomics: the same
 *      inputs give the same bits.  (egs_object_motion_scratch_bytes also covers the rasterizer's backward, whose lines come one per
 *      64 rows when the spherical-harmonics launch finishes the positions' gradient, plus the rotation lines.)
 *      egs_object_move_points           the placed positions as an array [P,3] (evaluation, export of a posed frame, a comparison path);
 *                                       rows that are not moved are copied bit for bit.  `out` must not alias means3D.
 *      egs_object_move_points_backward  dmeans3D [P,3] (may be NULL) and grad12 (device float[12] in A12's layout, may be NULL; needs
 *                                       means3D and `scratch`) from g [P,3]; dmeans3D must not alias g. */
size_t egs_object_motion_scratch_bytes(int P);
int egs_object_move_points(int P, const float* means3D /*[P,3]*/, const float* A12 /*device [12]*/, const uint8_t* moved /*[P] or NULL*/,
                           const int32_t* active_count /*device int32[1] or NULL*/, float* out /*[P,3] out*/, void* stream);
int egs_object_move_points_backward(int P, const float* means3D /*[P,3]*/, const float* A12, const uint8_t* moved, const int32_t* active_count,
                                    const float* g /*[P,3]: dL/dp'*/, float* dmeans3D /*[P,3] out or NULL*/, float* grad12 /*device [12] out or NULL*/,
                                    void* scratch /*egs_object_motion_scratch_bytes(P), needed with grad12*/, void* stream);

/* ---- f-3: fused image loss (1 - lambda) * L1 + lambda * (1 - SSIM), 11x11 Gaussian window sigma 1.5, zero padding.
 *      Replaces l1_loss + ssim (/root/reference/utils/loss_utils.py:57-107) as combined at
 *      /root/reference/trainers/train_static.py:92-95.  The forward writes the scalar loss (device float[1]), using
 *      egs_l1_ssim_partial_count floats of scratch for per-block partial sums, and three derivative maps [C,H,W] the
 *      backward consumes.  `gate` (optional, [H,W]) multiplies the image gradient
 *      per pixel -- the hand-mask hook of train_static.py:91.
 *      `loss_running_sum` (optional device float[1]): the loss value is also ADDED to it -- a trainer's logging sum without a
 *      launch or a host read per iteration.
 *      Deferred value: with loss == NULL the forward does not launch the kernel that assembles the scalar; pass the same
 *      partial_sums to egs_l1_ssim_backward as `deferred_partial_sums` (+ `deferred_loss`, `loss_running_sum`) and one wave of
 *      the backward kernel assembles it.  For a training step replayed from a hipGraph, which reads the value only after the
 *      backward anyway, that is one launch (~4.5 us of GPU time) less. */
size_t egs_l1_ssim_partial_count(int channels, int height, int width);
int egs_l1_ssim_forward(int channels, int height, int width, const float* img /*[C,H,W]*/, const float* gt /*[C,H,W]*/,
                        float lambda_dssim, float* partial_sums /*scratch*/, float* dm_dmu1, float* dm_dexx, float* dm_dexy,
                        float* loss /*device [1] out, or NULL: deferred*/, float* loss_running_sum /*device [1] in/out or NULL*/,
                        void* stream);
/* ABI 4: the two terms as two values, for a loop that combines them itself -- the reference's trainers call l1_loss(x, gt) and
 * ssim(x, gt) (/root/reference/utils/loss_utils.py:57-58,79-107) and weigh them in Python (trainers/train_static.py:92-95).  ONE forward
 * launch (+ a one-workgroup reduction) yields mean|x - gt| and mean SSIM; ONE backward launch takes an upstream scalar for each, read on
 * the device (autograd hands them over as tensors).  Same kernels and maps as egs_l1_ssim_forward / _backward; the backward is declared
 * behind egs_backward_prologue below (it can carry a rasterizer backward's preparation like egs_l1_ssim_backward_ex). */
int egs_l1_ssim_pair_forward(int channels, int height, int width, const float* img, const float* gt, float* partial_sums, float* dm_dmu1,
                             float* dm_dexx, float* dm_dexy, float* l1_out /*[1]*/, float* ssim_out /*[1]*/, void* stream);
int egs_l1_ssim_backward(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                         const float* upstream_grad /*device [1]*/, const float* gate /*[H,W] or NULL*/,
                         const float* dm_dmu1, const float* dm_dexx, const float* dm_dexy, float* dL_dimg /*[C,H,W] out*/,
                         const float* deferred_partial_sums /*NULL unless the forward deferred the value*/,
                         float* deferred_loss /*device [1] out or NULL*/, float* loss_running_sum /*device [1] in/out or NULL*/,
                         void* stream);

/* ---- evaluation figures of one frame: 8-bit, hand-masked PSNR / SSIM sums (added within ABI 6: new entries only).
 *      What the reference's eval_and_metric measures after writing render, ground truth and 1 - hand mask to 8-bit PNGs and reading them
 *      back (the reference, trainers/eval_metric.py:41-175):
 *          q(v) = uint8(clamp(v * 255 + 0.5, 0, 255))   in float32, truncating; NaN -> 0 (torchvision's save_image conversion)
 *          kept = keep >= 0.5     u = kept ? q(img) / 255 : 0     v = kept ? q(gt) / 255 : 0      (masks are binary by contract)
 *          sse      = sum over kept pixels and channels of (q(img) - q(gt))^2                    -- an exact integer
 *          ssim_sum = sum over all C*H*W entries of the SSIM map of (u, v)                       -- the window of egs_l1_ssim_forward
 *      from which the host forms  psnr = 10 log10(255^2 * C*H*W / sse)  (inf for sse == 0; the divisor counts gated pixels too, as the
 *      reference's mean does)  and  ssim = ssim_sum / (C*H*W).  Two launches on `stream`: the strips (one {float, uint32} partial each into
 *      `partial`, egs_eval_metrics_partial_bytes of scratch) and ONE wave that adds the partials in a fixed order, int64 and float64 -- the
 *      row is bit-identical run to run.  That wave writes rows[cursor[0]] and then stores cursor[0] + 1: the frame index lives on the device
 *      because a captured launch cannot carry one in its arguments.  cursor[0] outside [0, capacity): nothing is written, the cursor still
 *      advances, so the host sees an overrun.  `overflow` (device uint32[2] or NULL): the overflow word of the egs_forward_enqueue that
 *      rendered `img` on the same stream -- [0] clipped flag, [1] instance count -- copied into the row, so that ONE host read after a sweep
 *      tells which frames have to be rendered again.  q_img / q_gt (device uint8[C,H,W] or NULL): the quantised images, unmasked, planar --
 *      what a caller writes to a PNG.  channels: 1 or 3 (else EGS_ERR_ARG); H*W >= 2^31: EGS_ERR_RANGE.  No allocation, no global state. */
typedef struct egs_eval_row {
    int64_t sse;                     /* sum of squared 8-bit differences over kept pixels and channels */
    double  ssim_sum;                /* sum of the SSIM map over all C*H*W entries */
    int64_t clipped;                 /* overflow[0] of the forward that produced the image (0 without `overflow`) */
    int64_t instances;               /* overflow[1]: that forward's instance count (0 without `overflow`) */
} egs_eval_row;                      /* 32 bytes */
size_t egs_eval_metrics_partial_bytes(int channels, int height, int width);
int egs_eval_metrics(int channels, int height, int width, const float* img /*[C,H,W]*/, const float* gt /*[C,H,W]*/,
                     const float* keep /*[H,W] or NULL: all kept*/, const uint32_t* overflow /*device [2] or NULL*/, void* partial /*scratch*/,
                     uint8_t* q_img /*[C,H,W] out or NULL*/, uint8_t* q_gt /*[C,H,W] out or NULL*/, void* rows /*egs_eval_row[capacity]*/,
                     int capacity, int32_t* cursor /*device [1] in/out*/, void* stream);

/* ---- the mask hand-off between the static stage and the background stage (added within ABI 6: new entries only).
 *      The reference thresholds the label render of every static frame at the end of each static phase and stores the result as an 8-bit
 *      image (trainers/train_static.py:167-197); the background stage gates its image gradient by 1 - dilate_k(hand mask | object mask)
 *      (trainers/train_static_bg.py:14-21, 81-99).  Both results are integer-exact.
 *
 *      egs_label_mask: per pixel  x = ((c0 + c1) + c2) / 3  in float32 (the label phase's logit, the same definition),
 *          set = x > threshold   (strict; NaN is not set)          mask8 = set ? 255 : 0   for EVERY pixel: the stored mask ignores `keep`
 *          kept = keep >= 0.5 (NULL: every pixel)                  tgt = target >= 0.5 (NULL: none)
 *          predicted = #(kept & set)   target = #(kept & tgt)   intersection = #(kept & set & tgt)   kept = #kept       -- exact integers
 *      Two launches on `stream`: the pixels (one uint32[4] partial per workgroup into `partial`, egs_label_mask_partial_bytes of scratch) and
 *      ONE wave that adds the partials in a fixed order as int64, writes rows[cursor[0]] and stores cursor[0] + 1 -- the conventions of
 *      egs_eval_metrics: cursor[0] outside [0, capacity) writes nothing and still advances; `overflow` (device uint32[2] or NULL) is the
 *      overflow word of the forward that rendered `img`, copied into the row.  img needs 4-byte alignment only, mask8 none; 16-byte loads
 *      and 4-byte mask stores are used when every address and H*W allow them, with the same result.  H*W >= 2^31: EGS_ERR_RANGE.
 *
 *      egs_interaction_gate: a pixel is SET when a != 0 || b != 0 (torch.logical_or's rule: NaN and negative values are set; at least one
 *      of a, b is given); gate = 0.0f when any pixel of the k x k window around it, clipped to the image, is set, else 1.0f -- the
 *      reference's conv2d(ones(k, k), padding = k / 2) > 0 with its zero padding, subtracted from one.  k odd, 1 <= k <= 31 (else
 *      EGS_ERR_ARG); k = 1 is the plain OR.  gate needs 4-byte alignment only (it may be a view into a packed frame) and must not overlap
 *      a or b.  One launch.  No allocation, no global state. */
typedef struct egs_mask_row {
    int64_t predicted;               /* kept pixels whose label logit exceeds the threshold */
    int64_t target;                  /* kept pixels with target >= 0.5 */
    int64_t intersection;            /* kept pixels with both */
    int64_t kept;                    /* pixels with keep >= 0.5 (H*W without `keep`) */
    int64_t clipped;                 /* overflow[0] of the forward that produced the image (0 without `overflow`) */
    int64_t instances;               /* overflow[1]: that forward's instance count (0 without `overflow`) */
} egs_mask_row;                      /* 48 bytes */
size_t egs_label_mask_partial_bytes(int height, int width);
int egs_label_mask(int height, int width, const float* img /*[3,H,W]*/, float threshold, const float* target /*[H,W] or NULL*/,
                   const float* keep /*[H,W] or NULL: all kept*/, const uint32_t* overflow /*device [2] or NULL*/, void* partial /*scratch*/,
                   uint8_t* mask8 /*[H,W] out or NULL*/, void* rows /*egs_mask_row[capacity]*/, int capacity,
                   int32_t* cursor /*device [1] in/out*/, void* stream);
int egs_interaction_gate(int height, int width, const float* a /*[H,W] or NULL*/, const float* b /*[H,W] or NULL*/, int k,
                         float* gate /*[H,W] out*/, void* stream);

/* ---- LPIPS (VGG-16) of two 8-bit images: the evaluation pass's third figure (added within ABI 6: new entries only).
 *      The definition (the Python package's lpips.lpips_vgg is its torch statement; it is written from the published definition and is NOT
 *      pinned against the lpipsPyTorch package the reference imports):
 *          u = kept ? byte / 255 : 0   (kept = keep >= 0.5; NULL: every pixel)      z = (u - mean) / std, NOT mapped to [-1, 1] first,
 *              mean = (-.030, -.088, -.188), std = (.458, .448, .450)
 *          the 13 3x3 convolutions of VGG-16's `features` (stride 1, zero padding 1 -- zero in z-scored space --, bias, ReLU) in blocks of
 *              2, 2, 3, 3, 3 with a 2x2 / stride 2 / floor maximum pool between the blocks; a tap after each block's last ReLU, before the pool
 *          n = f / (sqrt(sum_c f^2) + 1e-10)  (eps OUTSIDE the root)     tap_k = mean over pixels of sum_c lin_k[c] (n_x - n_y)^2
 *          lpips = tap_1 + ... + tap_5
 *      Activations are float32 NHWC, the two images a batch of 2.  Convolutions run on the matrix pipe with f32 inputs and f32
 *      accumulation (v_mfma_f32_32x32x2_f32: exact f32 products).  Weights come from the caller -- none are shipped --, each convolution's
 *      repacked K-major: packed_w[(tap * Cin + c) * Cout + o] = w[o][c][tap / 3][tap % 3], tap = 3 ky + kx; the first layer's Cin padded
 *      3 -> 4 with zeros.
 *
 *      egs_lpips_forward: q_x, q_y device uint8[3,H,W] planar (what egs_eval_metrics writes as q_img / q_gt), keep device float[H,W] or
 *      NULL.  workspace: egs_lpips_workspace_bytes(H, W) device bytes, 256-byte aligned, owned by the caller (the library allocates nothing);
 *      it keeps all five tap maps (122 H W floats per image) next to the scratch of the other layers: 412 H W floats = 0.85 GB at 960 x 540.
 *      egs_lpips_tap_offsets gives the byte offsets of the five tap maps in it, float[2, H >> k, W >> k, C_k], C = 64, 128, 256, 512, 512.
 *      20 launches on `stream`: the input, 13 convolutions, five tap kernels (channel norms, weighted squared difference, one float64
 *      partial per workgroup, and the pooled map of the next block) and ONE wave that adds each tap's partials in a fixed order in float64,
 *      writes rows[cursor[0]] = (tap_1 .. tap_5, lpips) as double[6] and stores cursor[0] + 1 -- the conventions of egs_eval_metrics:
 *      cursor[0] outside [0, capacity) writes nothing and still advances.  No float atomics: the row is bit-identical run to run, and an
 *      identical pair gives exact zeros.  EGS_ERR_ARG before any device work: H or W < 16 (a pool would have no output), a NULL pointer
 *      other than keep, a misaligned workspace or weight array (16 bytes), capacity < 0.  H or W > 8192: EGS_ERR_RANGE (workspace_bytes: 0).
 *
 *      egs_conv3x3_relu_nhwc: one layer of the chain by itself, out[n,H,W,Cout] = relu(conv3x3(in[n,H,W,Cin]) + bias); H, W >= 1 (maps
 *      smaller than a tile are masked, never read outside).  Cin = 4 or a multiple of 16, Cout a multiple of 64, in != out, 16-byte
 *      aligned arrays (else EGS_ERR_ARG); H, W > 32767, Cin, Cout > 4096, n > 65535: EGS_ERR_RANGE. */
typedef struct egs_lpips_weights {
    const float* conv_w[13];         /* device, packed [9 Cin, Cout] (above) */
    const float* conv_b[13];         /* device [Cout] */
    const float* lin[5];             /* device [C_k]: the linear heads' weights */
} egs_lpips_weights;
size_t egs_lpips_workspace_bytes(int height, int width);
int egs_lpips_tap_offsets(int height, int width, int64_t* offsets /*host [5] out*/);
int egs_lpips_forward(int height, int width, const uint8_t* q_x /*[3,H,W]*/, const uint8_t* q_y /*[3,H,W]*/,
                      const float* keep /*[H,W] or NULL: all kept*/, const egs_lpips_weights* weights, void* workspace,
                      void* rows /*double[capacity][6]*/, int capacity, int32_t* cursor /*device [1] in/out*/, void* stream);
int egs_conv3x3_relu_nhwc(int n, int height, int width, int cin, int cout, const float* in /*[n,H,W,Cin]*/,
                          const float* packed_w /*[9 Cin, Cout]*/, const float* bias /*[Cout]*/, float* out /*[n,H,W,Cout]*/, void* stream);

/* ---- the 8-bit frame store (added within ABI 6: new entries only).
 *      The reference's images come from 8-bit files (utils/general_utils.py: uint8 -> float / 255) and its masks are binarised to {0, 1}; a
 *      packed float32 frame of the captured steps (camera, image, accumulated pose, gate, object mask) therefore says in 16 - 20 bytes per
 *      pixel what 3 bytes and 1 - 2 bits hold.  A store keeps F frames of one image size and one frame layout in that precision on the
 *      device; egs_frame_decode writes n_rows complete packed frames from it, chosen on the device through a ring of frame indices, so a
 *      captured step fetches the frames of its next iterations itself.
 *
 *      flags (EGS_FRAME_*) name the layout, as the Python package's graph.frame_layout: DYNAMIC adds accum_R (9 floats), MOTION accum_T (12),
 *      GATED the gate plane, OBJECT_LOSS the obj_mask plane (the image is then stored pre-multiplied by it); LABEL_PHASE is the label step's
 *      frame -- camera[, gate], obj_mask, no image -- and goes with GATED only (else EGS_ERR_MODE).  Every segment of a packed frame starts on
 *      a 16-byte boundary and is padded with 0.0f to the next:   [image] cam [accum_R] [accum_T] [gate] [obj_mask].
 *      egs_frame_store_layout fills the sizes below.  The store's arrays, all caller-owned:
 *          img    uint8  [F][image_stride]              3 H W bytes in CHW order, then zero bytes; image_stride = 3 H W rounded up to 16
 *          bits   uint32 [F][n_planes][plane_words]     pixel p is bit p % 32 of word p / 32; gate first, then obj_mask; 1 means 1.0f;
 *                                                       plane_words = ceil(H W / 32) rounded up to 4; unused bits are 0
 *          small  float  [F][small_floats]              floats small_begin .. small_begin + small_floats of the packed frame, untouched
 *          table  float  [256]                          byte -> float.  The image value of byte b is b / 255.0f by TRUE division; the host
 *                                                       fills the table with exactly that (b * (1 / 255.f) differs at 126 codes).
 *
 *      egs_frame_decode: two launches on `stream`.  The first writes out[k][0 .. frame_floats) for k < n_rows -- every float, the padding as
 *      0.0f, nothing beyond -- from frame ring[(ctl[0] + k) % ctl[1]]: `ring` is a device int32[ring_capacity], `ctl` two device int32 words,
 *      cursor and length, read on the device because a captured launch cannot carry them in its arguments.  The second, one lane, stores
 *      ctl[0] = (ctl[0] + n_rows) % ctl[1]; it is a launch of its own because no workgroup of the first may change the cursor while another
 *      may still read it.  A frame index outside [0, n_frames) is clamped into it and the sticky device word status[0] is incremented (once
 *      per such row; once more per call whose ctl had to be brought into 0 <= cursor < length, 1 <= length <= ring_capacity): whatever the
 *      ring and ctl hold, nothing outside the store is read.  16-byte loads and stores are used when out, img and small are 16-byte
 *      aligned, 4-byte ones otherwise (out may be any 4-byte aligned view), with the same result.
 *      EGS_ERR_ARG before any device work: height, width, n_frames, n_rows or ring_capacity < 1, unknown flag bits, a NULL small / ring /
 *      ctl / status / out, a NULL img or table for a layout with an image, a NULL bits for a layout with planes.  H*W >= 2^31 or
 *      n_rows > 65535: EGS_ERR_RANGE.  No allocation, no global state. */
#define EGS_FRAME_DYNAMIC      1
#define EGS_FRAME_MOTION       2
#define EGS_FRAME_GATED        4
#define EGS_FRAME_OBJECT_LOSS  8
#define EGS_FRAME_LABEL_PHASE 16
typedef struct egs_frame_layout {
    int64_t frame_floats;            /* floats of one packed frame (a multiple of 4) */
    int64_t image_floats;            /* 3 H W, 0 for the label layout; the image segment starts at float 0 */
    int64_t small_begin;             /* first float of `cam` in the packed frame */
    int64_t small_floats;            /* 36, 48 or 60: cam[, accum_R][, accum_T] with their padding */
    int64_t gate_begin;              /* first float of the gate segment, -1 without one */
    int64_t obj_mask_begin;          /* first float of the obj_mask segment, -1 without one */
    int64_t image_stride;            /* bytes per frame of `img` (0 for the label layout) */
    int64_t plane_words;             /* uint32 words per plane and frame of `bits` */
    int64_t n_planes;                /* 0, 1 or 2 */
} egs_frame_layout;                  /* 72 bytes */
int egs_frame_store_layout(int height, int width, int flags, egs_frame_layout* layout /*HOST out*/);
int egs_frame_decode(int height, int width, int flags, int n_frames, int n_rows, const uint8_t* img, const uint32_t* bits, const float* small,
                     const float* table, const int32_t* ring, int ring_capacity, int32_t* ctl /*device [2] in/out*/,
                     int32_t* status /*device [1] in/out*/, float* out /*[n_rows][frame_floats]*/, void* stream);
/* POSE_ROWS (added within ABI 6): a 4-word segment `pose_rows` follows accum_T in the small block (the frame word of the pose sequence
 * below: int32 carried in the float buffer, copied bit for bit like every float of the block); needs MOTION (else EGS_ERR_MODE);
 * small_floats is then 64. */
#define EGS_FRAME_POSE_ROWS   32

/* ---- frame ingest: the producer of the 8-bit frame store (added within ABI 6: new entries only).
 *      The reference resizes every image, hand mask and object mask with PIL.Image.resize (default filter: bicubic, antialiased, on 8-bit
 *      data), divides by 255 and collapses the masks to {0, 1} (utils/camera_utils.py:21-94, utils/general_utils.py:22-60).  These entries
 *      take the source-resolution 8-bit arrays and leave in a store's rows the bits that path followed by a put() would leave there.
 *
 *      The resize of modes L and RGB (Pillow, Resample.c): a horizontal pass when the width changes, then a vertical pass when the height
 *      changes; the intermediate is 8-bit, rounded and clamped like the output; a pass whose size does not change is skipped.  One axis,
 *      in -> out, in C double, in this order of evaluation:
 *          scale = in / out;  filterscale = max(scale, 1.0);  support = 2.0 * filterscale;  ksize = (int)ceil(support) * 2 + 1
 *          per output xx:  center = (xx + 0.5) * scale;  ss = 1.0 / filterscale
 *                          xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), in) - xmin
 *                          w[x] = bicubic((x + xmin - center + 0.5) * ss), x < xmax;  ww = their sum in index order;  w[x] /= ww when ww != 0
 *                          kk[x] = (int)(w < 0 ? -0.5 + w * 2^22 : 0.5 + w * 2^22), 0 for xmax <= x < ksize
 *          bicubic(x), a = -0.5, x = |x|:  x < 1: ((a + 2) x - (a + 3)) x x + 1;  x < 2: (((x - 5) x + 8) x - 4) a;  else 0
 *      A pixel of a pass: clamp((2^21 + sum in[xmin + x] * kk[x]) >> 22, 0, 255), int32, arithmetic shift.
 *      A mask is "any channel > 0" of the resized bytes; the hand mask enters the store as the gate 1 - hand_mask; with OBJECT_LOSS the
 *      image bytes are stored multiplied by the object plane.
 *
 *      egs_resample_ksize   ksize of in -> out; 0 when in or out < 1.
 *      egs_resample_tables  HOST arithmetic, no device: kk[out][ksize] and bounds[out] = {xmin, xmax} as above.  in or out < 1 or a NULL
 *                           pointer: EGS_ERR_ARG.
 *      egs_frame_ingest     resizes ONE source array, src = device uint8 [src_h][src_w][src_c] (interleaved), to width x height and writes
 *                           frame `frame` of a store of the layout `flags` (img, bits: the store's arrays, egs_frame_store_layout):
 *                             EGS_INGEST_IMAGE     src_c = 3: img[frame] as CHW bytes (the padding up to image_stride is not written);
 *                                                  with OBJECT_LOSS each byte times the bit of the frame's obj_mask plane, which the
 *                                                  launch READS: ingest the object mask of a frame before its image
 *                             EGS_INGEST_HAND_MASK src_c = 1 or 3: the gate plane, bit = no channel > 0
 *                             EGS_INGEST_OBJ_MASK  src_c = 1 or 3: the obj_mask plane, bit = any channel > 0
 *                           Both passes run in one launch: the horizontal result of an output tile lies in LDS as bytes (at most 41 KB per
 *                           workgroup), nothing intermediate in device memory.  A plane's words of the frame are cleared by a memset node
 *                           on `stream` and the tiles OR their bits in: any width, the same words whatever the order.  kk_h, bounds_h: the
 *                           device copies of egs_resample_tables(src_w, width), kk_v, bounds_v: of (src_h, height); those of an axis that
 *                           does not change are not read and may be NULL.  The kernel clamps what it reads from them into the source.
 *                           No allocation, no global state, no synchronisation; can be captured.
 *                           EGS_ERR_ARG before any device work: height, width, n_frames, src_h or src_w < 1, frame outside [0, n_frames),
 *                           unknown flag bits or plane, src_c not 3 (image) / 1 or 3 (masks), a NULL src, a NULL img / bits where the
 *                           plane needs it, a NULL table of an axis that changes.  EGS_ERR_MODE: a layout that has no such plane (or is
 *                           refused by egs_frame_store_layout).  EGS_ERR_RANGE: a side of the source or the target > 32767, or
 *                           src_w > 8 width or src_h > 8 height (ksize <= 33 bounds the tile in LDS). */
#define EGS_INGEST_IMAGE      0
#define EGS_INGEST_HAND_MASK  1
#define EGS_INGEST_OBJ_MASK   2
int egs_resample_ksize(int in, int out);
int egs_resample_tables(int in, int out, int32_t* kk /*HOST out [out][ksize]*/, int32_t* bounds /*HOST out [out][2]*/);
int egs_frame_ingest(int height, int width, int flags, int n_frames, int frame, int plane, uint8_t* img, uint32_t* bits,
                     const uint8_t* src, int src_h, int src_w, int src_c, const int32_t* kk_h, const int32_t* bounds_h,
                     const int32_t* kk_v, const int32_t* bounds_v, void* stream);

/* ---- PNG files written on the device (added within ABI 6: new entries only).
 *      Every stage of the reference that produces images ends in 8-bit PNG files (trainers/eval_metric.py:95-126 render_results,
 *      trainers/train_static.py:183-197 the predicted masks).  This entry turns planar uint8 images on the device -- [C][H][W] with
 *      plane_stride bytes between channels, image_stride between images; the evaluation sweep's `images`, the mask pass's `masks`, a frame
 *      store's `img` -- into complete files in the caller's buffer: out + i * out_stride holds sizes[i] bytes of
 *          signature, IHDR (bit depth 8, colour type 0 for one channel and 2 for three, no interlace), IDAT ..., IEND; no other chunk.
 *      The IDAT payloads together are ONE zlib stream (32 KB window) of the filtered data: H rows of 1 + W C bytes, the filter type then the
 *      filtered interleaved bytes.  Filter type of a row: filters 0 .. 4 (None, Sub, Up, Average with floor((a + b) / 2), Paeth) on the raw
 *      neighbours, the pixel to the left and the row above taken as 0 where they do not exist; score = sum of min(v, 256 - v) over the
 *      W C filtered bytes; the lowest score wins, ties go to the lowest type -- a pure function of the image (egogaussian_amd/png.py
 *      filter_rows is the torch statement).  The stream is compressed in independent segments, one per row (a row of more than 4096
 *      stream bytes in pieces of 4096), each a stored block or a fixed / dynamic Huffman block followed by the empty stored block of a
 *      zlib full flush, each an IDAT chunk of its own; the 2-byte zlib header and the final block with the Adler-32 are two more.
 *      Three launches whatever the content, no allocation, no synchronisation, no global state: can be captured.  Same input, same bytes.
 *        egs_png_bound          capacity of one image's slot: 77 + H (W C + 1) + 17 H ceil((W C + 1) / 4096) -- the fixed chunks, the
 *                               filtered data, and per segment 12 bytes of chunk framing + 5 of a stored block's header.  0 for a size
 *                               egs_png_encode refuses.  Host arithmetic.
 *        egs_png_scratch_bytes  device bytes `scratch` must hold for n_images (16-byte aligned); 0 for a refused size or n_images < 1.
 *        egs_png_encode         EGS_ERR_ARG before any device work: n_images < 1, a NULL pointer, a misaligned scratch (16) or sizes (4),
 *                               plane_stride < W H with three channels, image_stride shorter than an image when n_images > 1,
 *                               out_stride < egs_png_bound.  EGS_ERR_RANGE: a side outside 1 .. 32767, channels not 1 or 3,
 *                               n_images > 65535, a bound of 4 GiB or more. */
size_t egs_png_bound(int width, int height, int channels);
size_t egs_png_scratch_bytes(int n_images, int width, int height, int channels);
int egs_png_encode(int n_images, int width, int height, int channels, const uint8_t* src, int64_t image_stride, int64_t plane_stride,
                   uint8_t* out, int64_t out_stride, uint32_t* sizes /*device [n_images] out*/, void* scratch, void* stream);

/* ---- PNG files read on the device (added within ABI 6: new entries only): the read side of the entry above.
 *      The reference opens 8-bit PNG files at dataset load (scene/dataset_readers.py:137-160: image, hand mask, object mask), at the stage
 *      hand-off (the masks the static stage wrote) and in calculate_metric (trainers/eval_metric.py:129-175).  This entry takes the bytes
 *      of a batch of files as they are on disk and leaves interleaved uint8 [height][width][channels] arrays in `out`, which is what frame
 *      ingest (egs_ingest_*) starts from.  Accepted: bit depth 8, colour type 0 or 2, no interlace; ancillary chunks anywhere; the zlib
 *      stream cut into IDAT chunks anywhere (empty ones too); any CINFO <= 7; stored, fixed and dynamic blocks in any mix.  Everything else
 *      is the caller's to refuse from IHDR (egogaussian_amd/png.py parse does).
 *      Host work is the chunk walk -- O(chunks), no IDAT byte touched -- which fills two tables:
 *        egs_png_file   per file: width, height, channels (1 or 3); its IDAT chunks idat[idat_begin .. idat_begin + n_idat), n_idat >= 1;
 *                       stream_bytes, the sum of their lengths; file_offset / file_bytes, the file inside `files`; stream_offset and
 *                       inflate_offset (multiples of 16), its places in the scratch areas of 16-byte-rounded streams and of the inflated data
 *                       (height (1 + width channels) bytes, rounded to 16); out_offset, where its pixels go in `out`.
 *        egs_png_idat   per chunk: file, src (offset of the payload inside the file; "IDAT" precedes it, the CRC follows), length, dst
 *                       (offset inside the file's stream: the chunks of a file tile its stream in order).
 *      Both tables are passed twice: a host copy, which the entry checks, and a device copy with the same content, which the kernels
 *      read (the caller uploads it with the files; the entry copies nothing, so the call can be captured).
 *      Three launches (gather + CRC per chunk; inflate, one wave per file; unfilter), no allocation, no synchronisation, no global state.
 *      status[i] (device): 0, or the first failure of file i --
 *          1 | chunk << 8  CRC-32 of that IDAT chunk          6  repeat without a previous length / past HLIT + HDIST    11  more inflated bytes than H (1 + W C)
 *          2  zlib header (CM, CINFO, FCHECK, FDICT)        7  no end-of-block code                                    12  fewer
 *          3  block type 3                                   8  symbol 286 / 287, distance symbol 30 / 31, or bits      13  Adler-32
 *          4  stored LEN / NLEN                                 no code of an incomplete set owns                       14  bytes behind the stream
 *          5  a code set over-subscribed or incomplete       9  a distance before the start of the output               15  filter type above 4
 *             (zlib's exception: one code of 1 bit;         10  the stream ends inside a block
 *             for distances also none)
 *      A failed file leaves its pixels unspecified inside its own slot; nothing else is touched and the other files are unaffected.
 *      Verdicts equal zlib's inflate().  EGS_ERR_ARG before any device work: n_files or n_idat < 1, a NULL pointer, a misaligned scratch
 *      (16), status (4) or device table, files / streams / inflated data / outputs that are not ascending, overlap or leave their buffers
 *      (files_bytes, out_bytes, scratch_bytes), chunks that leave their file or do not tile the stream.  EGS_ERR_RANGE: a side outside
 *      1 .. 32767, channels not 1 or 3, n_files > 65535, a per-file output or stream of 2 GiB or more.
 *        egs_png_decode_scratch_bytes   256-aligned areas: 4 n_idat flag bytes, the streams, the inflated data (totals as the offsets above
 *                                       imply: the sums of the 16-byte-rounded sizes); 0 for n_idat < 1. */
typedef struct egs_png_file {
    int32_t width, height, channels, n_idat;
    uint32_t idat_begin, stream_bytes;
    uint64_t file_offset, file_bytes, stream_offset, inflate_offset, out_offset;
} egs_png_file;
typedef struct egs_png_idat { uint32_t file, src, length, dst; } egs_png_idat;
size_t egs_png_decode_scratch_bytes(int n_idat, size_t total_stream_bytes, size_t total_inflate_bytes);
int egs_png_decode(int n_files, const uint8_t* files /*device*/, size_t files_bytes, const egs_png_file* desc_host, const egs_png_file* desc_device,
                   const egs_png_idat* idat_host, const egs_png_idat* idat_device, int n_idat, uint8_t* out /*device*/, size_t out_bytes,
                   uint32_t* status /*device [n_files] out*/, void* scratch, size_t scratch_bytes, void* stream);
/*      The same call restricted to some of its launches, for measurements (tools/time_png_decode.py): phases is a mask of 1 (gather + CRC),
 *      2 (inflate) and 4 (unfilter), 1 .. 7 (else EGS_ERR_ARG).  A later launch alone reads what an earlier call with the same arguments
 *      left in `scratch` and `status`.  egs_png_decode is phases = 7. */
int egs_png_decode_phases(int n_files, const uint8_t* files, size_t files_bytes, const egs_png_file* desc_host, const egs_png_file* desc_device,
                          const egs_png_idat* idat_host, const egs_png_idat* idat_device, int n_idat, uint8_t* out, size_t out_bytes,
                          uint32_t* status, void* scratch, size_t scratch_bytes, void* stream, int phases);
/*      The segmented route (added within ABI 6: new entries only; egs_png_decode and egs_png_decode_phases are unchanged).
 *      The files egs_png_encode writes keep every row segment in an IDAT chunk of its own, ending on a byte boundary with the empty stored
 *      block of a full flush: such chunks inflate independently.  With EGS_PNG_SEGMENTS in `flags` the entry decides PER FILE, on the device,
 *      from the stream itself, whether the file's IDAT chunks are such segments, and inflates an accepted file with one wave per chunk.  The
 *      route only ever accepts: a file it does not accept is inflated by the serial wave of egs_png_decode in the same call and that wave's
 *      status word stands, so statuses, the CRC word and "verdicts equal zlib's" are what they are without the flag.  Accepted when ALL hold
 *      (the argument that such a file is one the serial inflater accepts with the same bytes is in csrc/png_segments.h):
 *        no IDAT CRC fails; chunk 0 holds at least the 2-byte zlib header (a valid one); every chunk, read from its first bit, is a sequence
 *        of whole deflate blocks ending exactly at its last bit (an empty chunk is a segment without blocks); every block is non-final but
 *        the last block of the last non-empty chunk, which is final and is followed, after byte alignment, by exactly the four Adler-32
 *        bytes and the chunk's end; no match reaches before the first byte its own segment produced; no segment produces more than
 *        EGS_PNG_SEGMENT_MAX bytes; the segments' lengths sum to H (1 + W C); their Adler-32 values combined in order equal the trailer.
 *      Launches with the flag, whatever the files hold (no allocation, no synchronisation, ordered by launch boundaries only; can be
 *      captured): gather + CRC; measure, one wave per chunk (a speculative decode -> a 16-byte record: length, Adler-32, reason);
 *      scan, one wave per file (the rules above, the offsets, the route word); place, one wave per chunk (exits at once for files not
 *      accepted, else decodes again straight into the inflated data: bytes at a segment's unaligned head and tail, words in between);
 *      the serial inflate, skipping accepted files; unfilter.  phases bit 2 covers the four inflate launches.
 *      route[i] (device, written only with EGS_PNG_SEGMENTS; may be NULL): 1 when the segmented route decoded file i, else 0 | reason << 8 --
 *          1  chunk 0 shorter than the zlib header             4  a segment of more than EGS_PNG_SEGMENT_MAX bytes     7  the combined Adler-32
 *          2  a chunk does not end on a block end              5  the final block or the trailer is not where the       8  any other inflate error inside a segment
 *          3  a distance before the start of its segment          rule above puts them                                  9  an IDAT CRC (status says which)
 *                                                              6  the lengths do not sum to H (1 + W C)
 *      flags = 0: exactly the launches and bytes of egs_png_decode_phases (route is not touched).  EGS_ERR_ARG before any device work:
 *      everything egs_png_decode_phases refuses, a bit of `flags` that is not defined, a route that is not 4-byte aligned, a scratch
 *      smaller than egs_png_decode_scratch_bytes_ex(..., flags): with EGS_PNG_SEGMENTS the three areas of egs_png_decode_scratch_bytes at
 *      the same offsets, then 16 n_idat record bytes and 4 n_idat route bytes, each 256-aligned.  0 for n_idat < 1 or an undefined flag. */
#define EGS_PNG_SEGMENTS         1
#define EGS_PNG_SEGMENT_MAX      8192      /* bytes one segment may produce: the segment buffer in LDS (ten workgroups per CU) */
size_t egs_png_decode_scratch_bytes_ex(int n_idat, size_t total_stream_bytes, size_t total_inflate_bytes, int flags);
int egs_png_decode_ex(int n_files, const uint8_t* files, size_t files_bytes, const egs_png_file* desc_host, const egs_png_file* desc_device,
                      const egs_png_idat* idat_host, const egs_png_idat* idat_device, int n_idat, uint8_t* out, size_t out_bytes,
                      uint32_t* status, void* scratch, size_t scratch_bytes, void* stream, int phases, int flags,
                      uint32_t* route /*device [n_files] out, or NULL*/);

/* ---- baseline JPEG files read on the device (added within ABI 6: new entries only).
 *      The reference opens its frames with Image.open (scene/dataset_readers.py:83-97, 140, 213), which takes .jpg as readily as .png.  This
 *      entry takes the bytes of a batch of baseline JPEG files as they are on disk and leaves interleaved uint8 [height][width][channels]
 *      arrays in `out`, bit for bit what libjpeg-turbo's default path (islow IDCT, fancy upsampling, fixed-point colour) -- and so Pillow --
 *      gives; egogaussian_amd/jpeg.py decode() is the statement of every step.  Accepted: SOF0, 8-bit samples, Huffman coding, ONE scan of
 *      all components; one component, or three marked as YCbCr with luma sampling 1x1, 2x1 or 2x2 and 1x1 chroma; any restart interval.
 *      Everything else is the caller's to refuse from the marker segments (egogaussian_amd/jpeg.py parse does).
 *      Host work is the segment walk up to the SOS header -- no entropy-coded byte touched -- which fills two tables:
 *        egs_jpeg_file    per file: width, height, channels (1 or 3); hs, vs the luma sampling; restart_interval in MCUs (0: none);
 *                         mcus_x = ceil(width / (8 hs)), mcus_y = ceil(height / (8 vs)); its restart intervals
 *                         [interval_begin, interval_begin + n_intervals) of the batch's, n_intervals = ceil(mcus_x mcus_y / restart_interval)
 *                         or 1; entropy_begin, the offset of the first entropy-coded byte inside the file, entropy_bytes = file_bytes -
 *                         entropy_begin; tq / td / ta, per component the index of its quantisation, DC and AC table; file_offset /
 *                         file_bytes, the file inside `files`; coef_offset and plane_offset (multiples of 16), its places in the scratch
 *                         areas of the coefficients (128 bytes per block: mcus_x mcus_y (hs vs + 2) blocks, or mcus_x mcus_y with one
 *                         component) and of the component planes (64 bytes per block); out_offset, where its pixels go in `out`.
 *        egs_jpeg_tables  per file: four 64-byte quantisation tables in NATURAL order, four DC and four AC Huffman tables as (counts[16],
 *                         values[256]).  Tables a component refers to must be valid: no zero divisor, at most 256 symbols, counts that do
 *                         not over-subscribe the code space.
 *      Both tables are passed twice: a host copy, which the entry checks, and a device copy with the same content, which the kernels read
 *      (the caller uploads it with the files; the entry copies nothing, allocates nothing, synchronises nothing: the call can be captured).
 *      Four launches, ordered by launch boundaries only:
 *        intervals  one workgroup per file walks the entropy-coded bytes in order, 256 lanes x 16 bytes per step, carrying the count:
 *                   FF 00 is a stuffed byte, FF D0 .. D7 starts restart interval k + 1 behind it (its number must be k mod 8), FF D9 ends
 *                   the data.  Leaves a [start, end) byte pair per interval.
 *        entropy    one lane per restart interval, the intervals of a file in workgroups that hold its decode tables in LDS (a first-level
 *                   look-up of 8 bits, the canonical-code walk beyond).  DC predictors start at 0; dequantised int16 coefficients, 64 per
 *                   block in natural order.  A lane reads no byte outside its interval and writes no block but its interval's.  A file
 *                   without restart markers is one interval on one lane: that serial chain is the format's.
 *        idct       eight lanes per block: column pass (descaled by 11) into a workspace, row pass (descaled by 18), + 128, saturating
 *                   clamp, in int32 -> uint8 component planes padded to whole MCUs.
 *        colour     one lane per output pixel: triangle-filter chroma upsampling with the edge rules of jpeg.py upsample(), fixed-point
 *                   YCbCr -> RGB (or a copy of Y); also writes the status word.  A file whose status is not 0 receives no pixel.
 *      The range rule: a dequantised coefficient (or a DC predictor) outside int16 is status 8, a workspace value outside int16 status 9;
 *      inside those bounds no int32 expression of the inverse DCT can overflow (jpeg.py, the module text).
 *      status[i] (device): 0, or the first failure of file i --
 *          1  a marker inside the entropy-coded data           4 | k << 8  bits no Huffman code owns            7 | k << 8  interval k has bytes left over
 *          2  a restart marker out of sequence or miscounted   5 | k << 8  a coefficient index beyond 63        8  coefficient range
 *          3  no EOI                                           6 | k << 8  interval k ends before its MCUs do   9  workspace range
 *      (k: the lowest failing restart interval of the file).  Nothing outside a file's slots is written and the other files are unaffected.
 *      EGS_ERR_ARG before any device work: n_files or n_intervals < 1, a NULL pointer, a misaligned scratch (16), status (4) or device
 *      table (8), files / coefficients / planes / outputs that are not ascending, overlap, are misaligned or leave their buffers,
 *      mcus_x / mcus_y / n_intervals / interval_begin / entropy_bytes that disagree with the geometry, a table index above 3 or an
 *      invalid table in use, a scratch smaller than egs_jpeg_decode_scratch_bytes.  EGS_ERR_RANGE: a side outside 1 .. 32767, channels
 *      not 1 or 3, sampling outside the accepted set, a restart interval outside 0 .. 65535, n_files > 65535, a file or an output of
 *      2 GiB or more.
 *        egs_jpeg_decode_scratch_bytes  256-aligned areas: 16 n_files bytes of stage words, 8 n_intervals bytes of byte pairs, the
 *                                       coefficients, the planes (totals as the offsets above imply: the sums of the 16-byte-rounded
 *                                       sizes); 0 for n_files or n_intervals < 1.  Host arithmetic.
 *        egs_jpeg_decode_phases         the same call restricted to some of its launches, for measurements (tools/time_jpeg_decode.py):
 *                                       phases is a mask of 1 (intervals), 2 (entropy), 4 (idct), 8 (colour), 1 .. 15 (else EGS_ERR_ARG).  A
 *                                       later launch alone reads what an earlier call with the same arguments left in `scratch`.
 *                                       egs_jpeg_decode is phases = 15. */
enum { EGS_JPEG_OK = 0, EGS_JPEG_MARKER = 1, EGS_JPEG_RESTART = 2, EGS_JPEG_NO_EOI = 3, EGS_JPEG_CODE = 4, EGS_JPEG_INDEX = 5,
       EGS_JPEG_SHORT = 6, EGS_JPEG_LEFT_OVER = 7, EGS_JPEG_COEF_RANGE = 8, EGS_JPEG_WORKSPACE_RANGE = 9 };
typedef struct egs_jpeg_file {
    int32_t width, height, channels, hs, vs, restart_interval, mcus_x, mcus_y;
    uint32_t interval_begin, n_intervals, entropy_begin, entropy_bytes;
    uint8_t tq[4], td[4], ta[4];
    uint32_t reserved;
    uint64_t file_offset, file_bytes, coef_offset, plane_offset, out_offset;
} egs_jpeg_file;
typedef struct egs_jpeg_huffman { uint8_t counts[16], values[256]; } egs_jpeg_huffman;
typedef struct egs_jpeg_tables { uint8_t quant[4][64]; egs_jpeg_huffman dc[4], ac[4]; } egs_jpeg_tables;
size_t egs_jpeg_decode_scratch_bytes(int n_files, int n_intervals, size_t coef_bytes, size_t plane_bytes);
int egs_jpeg_decode(int n_files, const uint8_t* files /*device*/, size_t files_bytes, const egs_jpeg_file* desc_host, const egs_jpeg_file* desc_device,
                    const egs_jpeg_tables* tables_host, const egs_jpeg_tables* tables_device, int n_intervals, uint8_t* out /*device*/,
                    size_t out_bytes, uint32_t* status /*device [n_files] out*/, void* scratch, size_t scratch_bytes, void* stream);
int egs_jpeg_decode_phases(int n_files, const uint8_t* files, size_t files_bytes, const egs_jpeg_file* desc_host, const egs_jpeg_file* desc_device,
                           const egs_jpeg_tables* tables_host, const egs_jpeg_tables* tables_device, int n_intervals, uint8_t* out,
                           size_t out_bytes, uint32_t* status, void* scratch, size_t scratch_bytes, void* stream, int phases);

/* ---- the object pose sequence on the device (added within ABI 6: new entries only).
 *      The object stages train ONE pose pair per dynamic frame on top of the pose accumulated over the earlier keys, store it under the
 *      frame's key and rebuild the accumulated sequence (/root/reference/trainers/fine_obj.py:97-126,216-224,
 *      /root/reference/utils/geometry_utils.py:69-89,152-186).  Here the table lives on the device and two one-workgroup launches do that
 *      bookkeeping around a rasterizer step, so a captured step can run over dynamic frames with no host work between them.
 *        rel    float[K][12]  per sorted key the relative pose [R | t], row-major 3x4
 *        valid  uint8[K]      0: the key has no pose yet (the reference's None entry)
 *        accum  float[K][12]  [A | b] of T_k ... T_1 over the valid rows; an invalid row repeats its predecessor, a row before any valid one
 *                             is the identity.  Its rotation block is the accumulated rotation.
 *        pose   float[9]      obj_translation[3], then obj_rotation_6d as the reference's (3,2) row-major
 *        exp_avg, exp_avg_sq float[9]; step float[2], lr float[2]: ONE Adam state for the whole sequence, [0] translation, [1] rotation
 *      frame word: device int32[4] = (fixed_row, train_row, reload, 0), read by the kernels; a row outside [0, K) means "none".
 *      egs_pose_head   train_row none: A12 / M9 = bit copies of accum[fixed_row] and its rotation block (identity without a fixed row).
 *                      Else, with reload != 0, first pose <- (t of rel[train_row], first two columns of its R); then R_t = the 6-D map of
 *                      the pose's rotation (normalise with a 1e-12 floor, Gram-Schmidt, cross product), A = R_t A_f, b = R_t b_f + t,
 *                      M = R_t R_f with (A_f | b_f) = accum[fixed_row] or the identity.  Writes A12[12], M9[9].
 *      egs_pose_tail   train_row none, or *skip_flag != 0: nothing at all.  Else from grad21 (dL/dA12[12], dL/dM9[9]): dL/dt = dL/db,
 *                      dL/dR_t = dL/dA A_f^T + dL/db b_f^T + dL/dM R_f^T, back through the 6-D map -> dpose[9] (written when not NULL);
 *                      the Adam step of the nine scalars (the arithmetic and coefficient expressions of egs_adam_step_capturable, bit
 *                      for bit; step[0], step[1] advance by one); rel[train_row] = [R(new rotation) | new t], valid[train_row] = 1;
 *                      accum[j] recomputed for j >= train_row.
 *      egs_pose_accumulate  accum[0 .. K) from rel and valid (after host edits of them).
 *      The small arithmetic runs in float64 and every stored value is rounded to float32 once; the accumulation is a sequential chain
 *      whose carry is the float32 row just stored, so the tail's suffix and a full accumulation agree bit for bit.  One workgroup of one
 *      wave each, no atomics; same inputs, same bits.  EGS_ERR_ARG before any device work: K < 1, a NULL member or argument (dpose and
 *      skip_flag may be NULL).  No allocation, no global state. */
typedef struct egs_pose_sequence {
    int32_t K;
    float* rel; uint8_t* valid; float* accum;          /* device [K][12], [K], [K][12] */
    float* pose; float* exp_avg; float* exp_avg_sq;    /* device [9] each */
    float* step; const float* lr;                      /* device [2] each */
    float beta1, beta2, eps;
} egs_pose_sequence;
int egs_pose_head(const egs_pose_sequence* seq, const int32_t* frame_word /*device [4]*/, float* A12 /*device [12] out*/, float* M9 /*device [9] out*/,
                  void* stream);
int egs_pose_tail(const egs_pose_sequence* seq, const int32_t* frame_word /*device [4]*/, const float* grad21 /*device [21]*/,
                  float* dpose /*device [9] out or NULL*/, const uint32_t* skip_flag /*device [1] or NULL*/, void* stream);
int egs_pose_accumulate(const egs_pose_sequence* seq, void* stream);
/* Stage 4, the poses of the held-out frames inside the dynamic phases (added within ABI 6: a new entry only;
 * /root/reference/trainers/interpolate_pose.py:28-114).  A gap is n consecutive rows of the table `to` that end at a key whose pose T is
 * row old_row of the table `from`; all n rows receive [R(r6) | t] of the END POINT of the reference's descent: from t = 0, r6 = the
 * first two columns of I, `iters` plain gradient steps of size lr on mean over the 16 entries of (M^n - T)^2, M = [R(r6) | t; 0 0 0 1],
 * leaving after the step at which every entry of the float32-rounded M^n is within 1e-9 + 1e-7 |T| of T.
 *   gaps      device int32[n_gaps][3] = (first_row, n, old_row)
 *   residual  device float[n_gaps] out: max |M^n - T| over the twelve entries, of the float64 end point
 *   status    device int32[1] out: 1 when the launch refused the words, else 0
 * One launch, one wave per gap, the iterations inside the kernel with the parameters in float64 registers; the n rows are the
 * float32 rounding of the end point, their valid bytes are set, nothing else of `to` is written and `accum` is NOT rebuilt
 * (egs_pose_accumulate afterwards).  A gap's rows depend on its own word and T only: same bits alone or among other gaps, run to run.
 * n outside [2, 32], first_row < 0, first_row + n > to->K, old_row outside [0, from->K) in ANY gap: no wave writes a row or a residual
 * and the call returns EGS_ERR_RANGE -- the words are read on the device by every wave, so the call copies `status` back and
 * SYNCHRONISES the stream (it cannot be captured; it runs once per stage).  n_gaps > 65535: EGS_ERR_RANGE before any device work.
 * EGS_ERR_ARG before any device work: a table egs_pose_head would refuse, a NULL argument, n_gaps < 1, iters < 0. */
int egs_pose_interpolate(const egs_pose_sequence* from, const egs_pose_sequence* to, const int32_t* gaps /*device [n_gaps][3]*/, int n_gaps,
                         int iters, float lr, float* residual /*device [n_gaps] out*/, int32_t* status /*device [1] out*/, void* stream);

/* The same launch carrying, in extra workgroups, what a rasterizer backward of the same frame needs done before its blend
 * kernel: ordering the tiles by the cost the forward recorded, clearing the gradient accumulator (`scratch`) and, with a sink, the
 * fused optimizer's per-step bookkeeping.  In a training step this launch sits between the two blends and leaves most of the
 * machine idle, while that preparation as a launch of its own (which egs_backward makes otherwise) costs ~12 us.  The
 * egs_backward_adam call that follows on the same stream is told so with prologue_done = 1 and must receive the same scratch,
 * image buffer, sink and skip_flag.  side == NULL: egs_l1_ssim_backward. */
typedef struct egs_backward_prologue {
    int P, width, height;            /* of the rasterizer call */
    void* image_buffer;              /* of that call's forward */
    void* scratch;                   /* egs_backward_scratch_bytes(P): the backward's scratch */
    const egs_adam_sink* sink;       /* HOST, or NULL */
    const uint32_t* skip_flag;       /* device uint32[1] or NULL */
    const void* geom_buffer;         /* ABI 3: of that call's forward, or NULL.  With it only the accumulator lines in use are cleared
                                      * (the replica lines of the frame's hot Gaussians, csrc/egs_common.h); NULL: all of them */
} egs_backward_prologue;
int egs_l1_ssim_pair_backward(int channels, int height, int width, const float* img, const float* gt, const float* upstream_l1 /*[1]*/,
                              const float* upstream_ssim /*[1]*/, const float* gate /*[H,W] or NULL*/, const float* dm_dmu1, const float* dm_dexx,
                              const float* dm_dexy, float* dL_dimg, const egs_backward_prologue* side /*HOST or NULL*/, void* stream);
int egs_l1_ssim_backward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                            const float* upstream_grad, const float* gate, const float* dm_dmu1, const float* dm_dexx,
                            const float* dm_dexy, float* dL_dimg, const float* deferred_partial_sums, float* deferred_loss,
                            float* loss_running_sum, const egs_backward_prologue* side /*HOST or NULL*/, void* stream);

/* ---- ABI 5: a training step WITHOUT a loss-backward launch.  The rasterizer's backward blend runs one workgroup per 16x16 tile and starts
 * by loading dL/dC of its 256 pixels; that gradient is a function of what the loss FORWARD left (its three derivative maps, the image, the
 * ground truth) in an 11x11 neighbourhood of the pixel, so the workgroup can compute it itself -- with k_l1_ssim_backward's arithmetic
 * operation for operation: the values are bit-identical to the ones that kernel would have written (tests/test_gpu_fused.py) -- and the
 * step loses a launch whose own work was ~15 us (config C: 3 350 -> ~3 450 it/s).  What that launch also carried moves:
 *   egs_l1_ssim_forward_ex     the forward, carrying the backward blend's preparation (egs_backward_prologue) as egs_l1_ssim_backward_ex did
 *   egs_backward_lossgrad      egs_backward_adam with an egs_loss_grad in place of the three dL_dout_* arrays (colour loss only: the depth
 *                              and alpha outputs carry no gradient); sink may be NULL (no optimizer inside); with deferred_partial_sums the
 *                              loss VALUE the forward deferred is assembled by one wave of the blend launch. */
typedef struct egs_loss_grad {       /* HOST struct */
    const float* image;              /* [3,H,W] the rendered image the loss was taken on */
    const float* gt;                 /* [3,H,W] */
    const float* dm_dmu1; const float* dm_dexx; const float* dm_dexy;   /* [3,H,W] each, as written by egs_l1_ssim_forward */
    const float* gate;               /* [H,W] or NULL: per-pixel factor on the image gradient (the trainers' 1 - hand_mask hook) */
    const float* upstream_grad;      /* device float[1]: dL/d(loss) */
    float lambda_dssim;
    const float* deferred_partial_sums;   /* NULL unless the forward deferred the value (loss == NULL there) */
    float* deferred_loss;            /* device float[1] out, or NULL */
    float* loss_running_sum;         /* device float[1] in/out, or NULL */
} egs_loss_grad;
int egs_l1_ssim_forward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                           float* partial_sums, float* dm_dmu1, float* dm_dexx, float* dm_dexy, float* loss /*or NULL: deferred*/,
                           float* loss_running_sum, const egs_backward_prologue* side /*HOST or NULL*/, void* stream);
int egs_backward_lossgrad(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                          const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                          const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const egs_loss_grad* loss_grad /*HOST*/,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                          float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                          const uint32_t* skip_flag, const egs_adam_sink* sink /*HOST or NULL*/, int prologue_done, const egs_object_rotation* rot /*HOST or NULL*/,
                          int grad_mask, void* scratch, void* stream, int debug);

/* ---- The object stages' loss (additions to ABI 6; nothing above changes).  The stages that recover the object's motion train on
 *      lambda_image * [(1 - lambda) L1 + lambda (1 - SSIM)](image, gt * obj_mask)
 *          + lambda_l1_alpha * mean|obj_mask - alpha| + lambda_l2_alpha * mean (obj_mask - alpha)^2
 * with the hand-mask gate on the gradient of the image AND of alpha (/root/reference/trainers/coarse_obj_pose.py:239-260,
 * trainers/fine_obj.py:128-151).  `gt` arrives already multiplied by the mask.  The entry points are the image loss's with an
 * egs_object_loss beside them: the forward launch also adds up the two alpha sums (a fixed order: per strip, then over the strips),
 * the finishing code assembles the weighted value and, with `terms`, the three terms apart; the backward launch also writes
 *      dL/dalpha = gate * upstream * (lambda_l1_alpha * sign(alpha - m) + 2 lambda_l2_alpha * (alpha - m)) / (H W),   sign(0) = 0,
 * and egs_backward_object_lossgrad is egs_backward_lossgrad whose blend forms that value itself as well (bit-identical to the launch's;
 * dL/ddepth is 0): the forward it belongs to composited depth and alpha (out_alpha != NULL), `alpha` is that plane. */
typedef struct egs_object_loss {     /* HOST struct */
    const float* alpha;              /* [H,W] the alpha plane of the render the loss is taken on */
    const float* obj_mask;           /* [H,W] */
    float lambda_image, lambda_l1_alpha, lambda_l2_alpha;
    float* alpha_partial_sums;       /* scratch: egs_l1_ssim_partial_count(1, H, W) floats, beside the image loss's partial_sums */
    float* terms;                    /* device float[3] out or NULL: image loss, mean|m - alpha|, mean (m - alpha)^2 (unweighted), written with the value */
} egs_object_loss;
int egs_object_loss_forward(int channels, int height, int width, const float* img, const float* gt /*already gt * obj_mask*/, float lambda_dssim,
                            float* partial_sums, float* dm_dmu1, float* dm_dexx, float* dm_dexy, float* loss /*or NULL: deferred*/,
                            float* loss_running_sum, const egs_object_loss* obj /*HOST*/, void* stream);
int egs_object_loss_forward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                               float* partial_sums, float* dm_dmu1, float* dm_dexx, float* dm_dexy, float* loss /*or NULL: deferred*/,
                               float* loss_running_sum, const egs_object_loss* obj /*HOST*/, const egs_backward_prologue* side /*HOST or NULL*/,
                               void* stream);
int egs_object_loss_backward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                                const float* upstream_grad, const float* gate, const float* dm_dmu1, const float* dm_dexx,
                                const float* dm_dexy, float* dL_dimg /*[C,H,W] out*/, float* dL_dalpha /*[H,W] out*/,
                                const float* deferred_partial_sums, float* deferred_loss, float* loss_running_sum,
                                const egs_object_loss* obj /*HOST*/, const egs_backward_prologue* side /*HOST or NULL*/, void* stream);
int egs_backward_object_lossgrad(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                          const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                          const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const egs_loss_grad* loss_grad /*HOST*/,
                          const egs_object_loss* obj /*HOST*/,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                          float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                          const uint32_t* skip_flag, const egs_adam_sink* sink /*HOST or NULL*/, int prologue_done, const egs_object_rotation* rot /*HOST or NULL*/,
                          int grad_mask, void* scratch, void* stream, int debug);

/* ---- The label phase of the static stage (additions to ABI 6; nothing above changes).  30 000 iterations of
 *          render_label = mean_c(get_render_label(cam, gaussians, bg));  hook: grad *= 1 - hand_mask
 *          loss = BCEWithLogitsLoss()(render_label, obj_mask);  loss.backward();  optimizer.step()      (only the label has a gradient)
 *      (/root/reference/trainers/train_static.py:104-109; the label render detaches the geometry, gaussian_renderer/render_helper.py:38-54).
 *      Per pixel, with the three planes C0, C1, C2 of the label render, the mask m, the gate k (1 when absent) and the upstream scalar up:
 *          x = (C0 + C1 + C2) / 3     l = max(x, 0) - x m + log1p(exp(-|x|))     dL/dx = up k (sigmoid(x) - m) / (H W)
 *      and the loss is the mean of l over the H W pixels; a pixel no splat reaches counts with x = mean(bg).
 *   egs_label_bce_forward   writes one partial sum per (16x16 tile, 8x8 quadrant) into `partial_sums` (egs_label_bce_partial_count floats:
 *                           a fixed partition and a fixed order inside it) and, unless loss == NULL, a finishing launch adds them up in index
 *                           order in float64: deterministic, the same bits on every run.  loss == NULL defers the value (as egs_l1_ssim_forward
 *                           does): pass the partial sums to egs_label_bce_backward as `deferred_partial_sums`, one wave of which assembles it.
 *   egs_label_bce_backward  dL/dC [3,H,W]: dL/dx / 3 in each plane.
 *   egs_backward_label      the backward of a render whose colour is ONE value per Gaussian, the label (the forward got it as colors_precomp with
 *                           EGS_ACT_SCALAR_COLOR... or as that value repeated three times: the backward does not read the colours).  Only dL/dlabel
 *                           exists: one sum per (wave, splat) in the blend, sum over pixels of w (dL/dC0 + dL/dC1 + dL/dC2), then one launch that
 *                           reads it out of the accumulator (exactly 0 where radii <= 0) into dL_dlabel [P] (may be NULL).
 *                           Exactly one of dL_dout_color and `loss` must be given (else EGS_ERR_MODE): with `loss` the blend forms dL/dx above
 *                           itself from the image the forward left -- no loss-backward launch, dL/dC never reaches memory -- and writes the quadrant
 *                           partial sums of the value (the partition and bits of egs_label_bce_forward), which the last launch adds up into
 *                           loss->loss / loss->running (either may be NULL).  loss->partial_sums: egs_label_bce_partial_count floats, n_partial
 *                           says how many the caller provides (fewer: EGS_ERR_ARG).
 *                           `adam` (may be NULL): the label's Adam step taken by the last launch for EVERY row below *active_rows (all rows if NULL),
 *                           rows with a zero gradient included -- torch's Adam is dense -- with the arithmetic, the step count and the bias
 *                           corrections of egs_backward_adam: bit-identical to egs_adam_step_capturable fed the same gradient.  adam->param is
 *                           the label [P], exp_avg / exp_avg_sq have its shape, lr / step are device float[1]; coef: device float[12] scratch.
 *                           skip_flag set (overflowed frame): no gradient is written, no step is taken and none is counted (the value is still
 *                           assembled, of the clipped image).  scratch: egs_backward_scratch_bytes(P).  The chain is prologue (tile order, cleared
 *                           accumulator, step bookkeeping), blend, finish: three launches on `stream`, capturable.
 *                           CALLER-CHECKED PRECONDITION: with `adam`, this call is the label's ONLY consumer in the optimizer step -- the gradient it
 *                           forms is the label's whole gradient (see egs_backward_adam). */
#define EGS_ACT_SCALAR_COLOR 16     /* colors_precomp is float[P], one value per Gaussian, broadcast into the record's three colour slots */
size_t egs_label_bce_partial_count(int height, int width);
int egs_label_bce_forward(int height, int width, const float* img /*[3,H,W]*/, const float* obj_mask /*[H,W]*/, float* partial_sums /*scratch*/,
                          float* loss /*device [1] out, or NULL: deferred*/, float* loss_running_sum /*device [1] in/out or NULL*/, void* stream);
int egs_label_bce_backward(int height, int width, const float* img, const float* obj_mask, const float* gate /*[H,W] or NULL*/,
                           const float* upstream_grad /*device [1]*/, float* dL_dimg /*[3,H,W] out*/,
                           const float* deferred_partial_sums /*NULL unless the forward deferred the value*/, float* deferred_loss /*device [1] out or NULL*/,
                           float* loss_running_sum /*device [1] in/out or NULL*/, void* stream);
typedef struct egs_label_loss {      /* HOST struct */
    const float* img;                /* [3,H,W] the label render the loss is taken on */
    const float* mask;               /* [H,W] the object mask */
    const float* gate;               /* [H,W] or NULL: per-pixel factor on the gradient (1 - hand_mask) */
    const float* upstream;           /* device float[1]: dL/d(loss) */
    float* partial;                  /* scratch: egs_label_bce_partial_count(H, W) floats */
    size_t n_partial;                /* floats `partial` holds */
    float* loss;                     /* device float[1] out, or NULL */
    float* running;                  /* device float[1] in/out, or NULL */
} egs_label_loss;
int egs_backward_label(int P, int64_t R, int width, int height, const int32_t* radii, const void* geom_buffer, const void* binning_buffer,
                       const void* image_buffer, const float* dL_dout_color /*[3,H,W] or NULL*/, const egs_label_loss* loss /*HOST or NULL*/,
                       float* dL_dlabel /*[P] out or NULL*/, const egs_adam_leaf* adam /*HOST or NULL*/, float beta1, float beta2, float eps,
                       float* coef /*device float[12] scratch; needed with adam*/, const int32_t* active_rows /*device int32[1] or NULL*/,
                       const uint32_t* skip_flag /*device uint32[1] or NULL*/, void* scratch, void* stream, int flags);

/* ---- Opacity-entropy regularisation (additions to ABI 6; nothing above changes).  Between std_train_iter and std_train_iter +
 *      entropy_reg_iter both static trainers add to the image loss
 *          0.1 * mean over the visible Gaussians (radii > 0) of  -o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10),   o = get_opacity
 *      (/root/reference/trainers/train_static.py:97-102, trainers/train_static_bg.py:105-110) and prune get_opacity < 0.5 when the phase ends.
 *      Per visible row, with o the float32 activated opacity (csrc/opacity_entropy.h, the one definition every route calls):
 *          a = o + 1e-10f   b = (1.0f - o) + 1e-10f   h = -o logf(a) - (1 - o) logf(b)   dh/do = -logf(a) - o / a + logf(b) + (1 - o) / b
 *          value = (sum of h over the visible rows) / n_vis          dL/do += weight * upstream / n_vis * dh/do
 *      and, when the opacity arrives as a logit (EGS_ACT_LOGIT_OPACITY), the sigmoid chain o (1 - o) after it.  Rows with radii <= 0 and rows
 *      at or beyond *active_count contribute nothing and receive nothing (exactly 0); o == 0, 0.5 and 1 are finite.  n_vis == 0: no gradient
 *      anywhere, value = NaN (torch's mean() of an empty tensor).  The sum is a deterministic reduction: one float32 line per 256 rows (six
 *      __shfl_xor levels, four waves through LDS), then one finish workgroup that adds the lines in index order in float64.  No float
 *      atomics: the same inputs give the same bits.
 *   egs_opacity_entropy_forward   `opacity` [P] as the caller's forward received it (activation_flags: 0 or EGS_ACT_LOGIT_OPACITY) -> ent->n_vis,
 *                                 ent->value (may be NULL), and with `activated` [P] (may be NULL) the activated opacity of every live row as
 *                                 the kernels form it (0 in the dead rows).  Two launches.  ent->weight / upstream are not read.
 *   egs_opacity_entropy_backward  dL/dopacity [P] of weight * upstream * value w.r.t. what the forward received; reads ent->n_vis as the
 *                                 forward left it.  One launch, no scratch.
 *   egs_backward_entropy_lossgrad egs_backward_lossgrad with the term inside: the reduction (of the activated opacities the forward parked in
 *                                 the geometry buffer -- the very bits the blend used -- and `radii`) is enqueued in front of the preprocess
 *                                 backward, whose entropy instantiation adds the row's share to dL/dopacity before the sigmoid chain, the
 *                                 dL_dopacity store and the Adam step of EGS_SINK_OPACITY: the opacity stays a fused leaf.  loss_grad may be
 *                                 NULL: the three dL_dout_* arrays are then read as by egs_backward_adam (with loss_grad they must be NULL).
 *                                 skip_flag set: no step is taken, as everywhere.  Not with EGS_ACT_OBJECT_MOTION and not on the colours-only
 *                                 path (EGS_ERR_MODE): the term belongs to the static stages. */
typedef struct egs_opacity_entropy {     /* HOST struct */
    const float* weight;             /* device float[1]: the term's weight (0.1 in the reference); read on the device, so a captured step changes it without re-capture */
    const float* upstream;           /* device float[1]: dL/d(loss), or NULL = 1 */
    void*        scratch;            /* egs_opacity_entropy_scratch_bytes(P) */
    uint32_t*    n_vis;              /* device uint32[1]: visible rows of the frame (out of the reduction, in of egs_opacity_entropy_backward) */
    float*       value;              /* device float[1] out or NULL: the UNWEIGHTED mean entropy of the visible opacities */
} egs_opacity_entropy;
size_t egs_opacity_entropy_scratch_bytes(int P);
int egs_opacity_entropy_forward(int P, const float* opacity /*[P]*/, int activation_flags /*0 or EGS_ACT_LOGIT_OPACITY*/, const int32_t* radii /*[P]*/,
                                const int32_t* active_count /*device int32[1] or NULL*/, float* activated /*[P] out or NULL*/,
                                const egs_opacity_entropy* ent /*HOST*/, void* stream);
int egs_opacity_entropy_backward(int P, const float* opacity /*[P]*/, int activation_flags, const int32_t* radii /*[P]*/,
                                 const int32_t* active_count /*device int32[1] or NULL*/, const egs_opacity_entropy* ent /*HOST*/,
                                 float* dL_dopacity /*[P] out*/, void* stream);
int egs_backward_entropy_lossgrad(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                          const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                          const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const egs_loss_grad* loss_grad /*HOST or NULL*/,
                          const egs_opacity_entropy* entropy /*HOST*/,
                          const float* dL_dout_color /*NULL with loss_grad*/, const float* dL_dout_depth /*or NULL*/, const float* dL_dout_alpha /*or NULL*/,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                          float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                          const uint32_t* skip_flag, const egs_adam_sink* sink /*HOST or NULL*/, int prologue_done, const egs_object_rotation* rot /*HOST or NULL*/,
                          int grad_mask, void* scratch, void* stream, int debug);

/* ---- f-4 (optimizer part): multi-tensor Adam step in one launch.  Same update as torch.optim.Adam(weight_decay=0,
 *      amsgrad=False), which the reference builds at /root/reference/scene/gaussian_model.py:198 and steps at
 *      /root/reference/trainers/train_static.py:137.  All array arguments are HOST arrays of length n_tensors holding
 *      device pointers / sizes / per-tensor learning rate and 1-based step count. */
int egs_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const int64_t* numels, const float* lrs, const int64_t* steps,
                  float beta1, float beta2, float eps, void* stream);
/* hipGraph-capturable variant: `lr_dev[t]` (device float[1]) is tensor t's learning rate, read by the kernel; the step number
 * comes from `counters[t]` (device uint32[egs_adam_workgroups(numels[t])], one array per tensor, never shared), every word of
 * which must hold the number of steps tensor t has taken; the launch adds one to each, so a captured iteration needs no
 * other kernel to keep count.  `step_dev[t]` (device float[1]) is WRITTEN with the number of the step
 * just taken (torch's state["step"]). */
int64_t egs_adam_workgroups(int64_t numel);
/* ABI 2: `skip_flag` (device uint32[1] or NULL) non-zero makes the launch a no-op (parameters, moments, counters and step_dev
 * untouched) -- the overflow word of egs_forward_enqueue.  `active_rows` (device int32[1] or NULL) with `row_floats` (HOST
 * int32[n_tensors], 0 = whole tensor) limits tensor t to its first *active_rows * row_floats[t] elements: the live rows of a
 * capacity-sized model. */
int egs_adam_step_capturable(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const int64_t* numels, float* const* step_dev /*HOST array of device ptrs*/,
                             const float* const* lr_dev /*HOST array of device ptrs*/, uint32_t* const* counters /*HOST array of device ptrs*/,
                             float beta1, float beta2, float eps, const uint32_t* skip_flag, const int32_t* active_rows,
                             const int32_t* row_floats /*HOST or NULL*/, void* stream);

/* ---- f-4 (densify / prune part): the bookkeeping of /root/reference/scene/gaussian_model.py:506-709,735-740 on the device.
 *      egs_densify_stats         per-iteration statistics in one pass: for every visible Gaussian (visible[i] != 0, or
 *                                radii[i] > 0 when `visible` is NULL)  grad_accum += |viewspace_grad.xy|, denom += 1 and, when
 *                                radii and max_radii2D are given, max_radii2D = max(max_radii2D, radii)
 *                                (add_densification_stats :735-740 + trainers/train_static.py:125).
 *      egs_densify_plan          evaluates densify_and_clone / densify_and_split / the final prune of densify_and_prune
 *                                (:588-709) for every Gaussian and compacts the results: src_index[k], kind[k] (0 kept original,
 *                                1 clone, 2 / 3 first / second split child) for the k-th Gaussian of the new model, in the
 *                                reference's order; split_rank[i] = rank of source i among the split ones (-1: not split);
 *                                totals (device uint64[4]) = kept originals, kept clones, kept children PER COPY, split sources.
 *                                New size = totals[0] + totals[1] + 2 totals[2].  Everything is enqueued; read totals after
 *                                synchronising.  EGS_ERR_MODE for prune_prev_gen == 0 without a curr_gen (the reference raises).
 *      egs_prune_plan            the same plan for prune_points(mask) (:536-563): kept = !mask.
 *      egs_gather_rows_f32       out[k][:] = in[src_index[k]][:]; zero_new_rows != 0 writes zeros for kind != 0 (Adam moments).
 *      egs_gather_i32            same for the int32 side arrays; clone_value_on: clones take clone_value (curr_gen).
 *      egs_split_children        rows of kind 2 / 3: xyz = parent + R(q) (exp(scaling) * z), scaling = log(exp(scaling) / 1.6);
 *                                z = the 2 * n_split standard-normal draws, first children first (torch.normal at :621). */
int egs_densify_stats(int P, const float* viewspace_grad /*[P,3]*/, const uint8_t* visible /*[P] or NULL*/,
                      const int32_t* radii /*[P] or NULL*/, float* grad_accum /*[P]*/, float* denom /*[P]*/,
                      float* max_radii2D /*[P] or NULL*/, void* stream);
size_t egs_densify_plan_scratch_bytes(int P);
int egs_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling_raw /*[P,3]*/,
                     const float* opacity_raw /*[P]*/, const float* max_radii2D /*[P]*/, const int32_t* generation /*[P]*/,
                     const int32_t* is_object /*[P]*/, float max_grad, float min_opacity, float percent_dense, float extent,
                     float max_screen_size /* <= 0: criterion off */, int clone, int split, int has_curr_gen, int curr_gen,
                     int prune_prev_gen, int has_which_object, int which_object, void* scratch,
                     int32_t* src_index /*[3P] out*/, uint8_t* kind /*[3P] out*/, int32_t* split_rank /*[P] out*/,
                     uint64_t* totals /*device [4] out*/, void* stream);
int egs_prune_plan(int P, const uint8_t* prune_mask /*[P]*/, void* scratch, int32_t* src_index, uint8_t* kind, int32_t* split_rank,
                   uint64_t* totals, void* stream);
int egs_gather_rows_f32(int64_t rows, int row_floats, const int32_t* src_index, const uint8_t* kind, int zero_new_rows,
                        const float* in, float* out, void* stream);
int egs_gather_i32(int64_t rows, const int32_t* src_index, const uint8_t* kind, int clone_value_on, int clone_value,
                   const int32_t* in, int32_t* out, void* stream);
int egs_split_children(int64_t rows, const int32_t* src_index, const uint8_t* kind, const int32_t* split_rank, int n_split,
                       const float* z /*[2 n_split, 3]*/, const float* xyz_old, const float* scaling_old, const float* rotation_old,
                       float* xyz_new, float* scaling_new, void* stream);

/* ---- f-4, capturable: densify / prune of a capacity-sized model with no host read.  The two calls above size their launches
 * by a live count the host knows and hand the host `totals` to size the new model; the four below take every count from device
 * memory, so one recorded chain (plan + apply) serves every later state of the model.
 *      egs_densify_plan_dev      egs_densify_plan over `capacity` rows.  The live count is *active_count (clamped to
 *                                [0, capacity]); rows at or beyond it set no flag, so src_index / kind / split_rank / totals[0..3]
 *                                are what egs_densify_plan gives on the live prefix (split_rank = -1 on dead rows).  The rule
 *                                values come from a device block (egs_densify_rules_dev), not from launch arguments: the size
 *                                threshold switches on once per schedule and curr_gen changes per dynamic frame.
 *                                totals is uint64[5]: totals[4] = the live count the plan was made for.  Plan buffers are sized
 *                                for capacity: scratch egs_densify_plan_scratch_bytes(capacity), src_index / kind [3 capacity].
 *                                is_object is read in the model's own type: is_object_is_float != 0 -> float32 (truncated as
 *                                torch's .to(int32) does), else int32.
 *      egs_prune_plan_dev        egs_prune_plan the same way: kept = !mask on the live rows; prune_mask has capacity bytes.
 *      egs_densify_apply         rewrites every array of the table in place from the plan, in two launches whatever the table
 *                                holds: a gather of rows [0, n_new) of every array into `scratch`, then a commit that copies
 *                                them back, zeroes what the roles below say and writes the count.  n_new = totals[0] + totals[1]
 *                                + 2 totals[2], n_old = totals[4], n_split = totals[3], all read on the device.
 *                                   PARAM   row k = old row src_index[k]; in the arrays named by xyz_index / scaling_index rows of
 *                                           kind 2 / 3 take egs_split_children's arithmetic (rotation_index: the quaternions);
 *                                           child c of split rank r reads row c * n_split + r of z [2 capacity, 3]
 *                                   MOMENT  as PARAM, zero where kind[k] != 0
 *                                   STAT    rules != NULL and (clone || split): zeroed over all capacity rows; else gathered
 *                                   TAG     gathered (EGS_DENSIFY_TAG_I32: int32 rows; else float32 rows holding integers);
 *                                           EGS_DENSIFY_TAG_CLONE_GEN: a clone takes rules->curr_gen when has_curr_gen;
 *                                           rows [n_new, n_old) are zeroed
 *                                rules == NULL: a prune plan (no clone value, statistics gathered; z may be NULL).
 *                                n_new > capacity: NOTHING is written but status.  n_old == 0: nothing is written but status
 *                                (an application of 0 rows).  Else *active_count = n_new, by the commit launch.
 *                                status (device uint32[4], zeroed once by the caller): [0] refusals so far, [1] rows the latest
 *                                refusal needed, [2] applications done, [3] n_new of the latest application.
 *                                No allocation, no read-back, no synchronisation; EGS_ERR_ARG before any device work.
 *      egs_densify_apply_scratch_bytes   capacity * sum(row_floats) * 4: one shadow row per row rewritten, nothing else. */
#define EGS_DENSIFY_MAX_ARRAYS 32
enum { EGS_DENSIFY_PARAM = 0, EGS_DENSIFY_MOMENT = 1, EGS_DENSIFY_STAT = 2, EGS_DENSIFY_TAG = 3 };
enum { EGS_DENSIFY_TAG_I32 = 1, EGS_DENSIFY_TAG_CLONE_GEN = 2 };
typedef struct {
    float max_grad, min_opacity, dense_extent /* percent_dense * extent */, big_extent /* 0.1 * extent */, max_screen_size /* <= 0: off */;
    int32_t clone, split, has_curr_gen, curr_gen, prune_prev_gen, has_which_object, which_object;
} egs_densify_rules_dev;                                   /* 12 words of device memory */
typedef struct {
    void* data;                                            /* [capacity, row_floats] float32 (or int32: EGS_DENSIFY_TAG_I32), contiguous */
    int32_t row_floats, role, flags, reserved;
} egs_densify_array;
int egs_densify_plan_dev(int capacity, const int32_t* active_count, const float* grad_accum, const float* denom,
                         const float* scaling_raw /*[capacity,3]*/, const float* opacity_raw, const float* max_radii2D,
                         const int32_t* generation, const void* is_object, int is_object_is_float,
                         const egs_densify_rules_dev* rules /*device*/, void* scratch, int32_t* src_index /*[3 capacity] out*/,
                         uint8_t* kind /*[3 capacity] out*/, int32_t* split_rank /*[capacity] out*/, uint64_t* totals /*device [5] out*/,
                         void* stream);
int egs_prune_plan_dev(int capacity, const int32_t* active_count, const uint8_t* prune_mask /*[capacity]*/, void* scratch,
                       int32_t* src_index, uint8_t* kind, int32_t* split_rank, uint64_t* totals /*device [5] out*/, void* stream);
size_t egs_densify_apply_scratch_bytes(int capacity, int n_arrays, const int32_t* row_floats /*HOST [n_arrays]*/);
int egs_densify_apply(int capacity, int32_t* active_count /*device, in/out*/, const int32_t* src_index, const uint8_t* kind,
                      const int32_t* split_rank, const uint64_t* totals /*device [5]*/, const egs_densify_rules_dev* rules /*device or NULL*/,
                      int n_arrays, const egs_densify_array* arrays /*HOST [n_arrays]*/, int xyz_index, int scaling_index,
                      int rotation_index, const float* z /*[2 capacity, 3] or NULL*/, void* scratch, uint32_t* status /*device [4]*/,
                      void* stream);

/* ---- f-2: mean squared distance of every point to its 3 nearest neighbours (self excluded by index).
 *      Replaces simple_knn._C.distCUDA2 (un-vendored submodule, /root/reference/.gitmodules:4-6), imported at
 *      /root/reference/scene/gaussian_model.py:21 and called at :301.  Exact (all pairs).  A point with fewer than three
 *      neighbours (a cloud of fewer than four finite points) gets +inf, in this call and in the grid search. */
int egs_knn3_mean_dist2(int N, const float* points /*[N,3]*/, float* mean_dist2 /*[N] out*/, void* stream);
/* The same statistic, bit for bit, through a uniform-grid search (counting sort of the points by cell, then rings of cells around
 * every query until the third neighbour is provably inside): O(N) for clouds of roughly even density instead of O(N^2) -- the
 * all-pairs call takes 0.4 s at 1 M points.  Points with a NaN / inf coordinate are nobody's neighbour and get +inf, in both
 * calls.  `scratch`: egs_knn3_grid_scratch_bytes(N) bytes of device memory. */
size_t egs_knn3_grid_scratch_bytes(int N);
int egs_knn3_grid(int N, const float* points /*[N,3]*/, float* mean_dist2 /*[N] out*/, void* scratch, void* stream);

/* Whether a forward of this size, given a placement buffer and these EGS_CALL_* flags, folds the count pass of its bucketing into the
 * preprocess launch (1) or not (0: very large images, or EGS_CALL_SEPARATE_COUNT). */
int egs_forward_fuses_count(int P, int width, int height, int flags);

/* ---- which launches sort the tile lists of a forward (added within ABI 6: new entries only).
 * The per-tile sort has two instantiations (four waves for lists of up to 1 792 instances, eight waves beyond) and two launch sites (launches
 * of its own, or inside the forward blend's launch).  Which of them a frame gets is host arithmetic on the model size, the CAPACITY the
 * binning buffer was laid out for (not the frame's instance count), the image size and the call's EGS_CALL_* flags; this entry returns the
 * decision the library acts on -- the same function decides inside the forward -- as a set of EGS_SORT_* bits, 0 when nothing is bucketed
 * (P == 0 or capacity == 0).  It launches no device work and needs no device.
 *   EGS_SORT_IN_BLEND              the forward blend's workgroups sort their own tile; no sort launch.  Only when the second instantiation is not
 *                                  needed (capacity <= 2048 x tiles) and the call has neither EGS_CALL_SEPARATE_SORT nor EGS_CALL_SYNC
 *   EGS_SORT_SECOND_INSTANTIATION  capacity > 2048 x tiles: the eight-wave instantiation is launched behind the four-wave one and takes the
 *                                  lists beyond 1 792; without it the four-wave instantiation sorts every list itself
 *   EGS_SORT_BALLOT_RANK           the call asks for the ballot-based ranker (EGS_CALL_BALLOT_RANK)
 * `flags` are read as the sort sees them: egs_forward_render passes the call's word on unchanged; egs_forward and egs_forward_enqueue never
 * synchronise inside their chain and mask EGS_CALL_SYNC out first, so for those two that bit does not keep the sort out of the blend.
 * NOT part of the answer: the one-time device check of the LDS lane order (the second item of process-wide state listed at the top).  A device
 * that fails it ranks with ballots whatever the call requests; EGS_SORT_BALLOT_RANK clear means "not requested", not "atomic ranker ran". */
#define EGS_SORT_IN_BLEND              0x1
#define EGS_SORT_SECOND_INSTANTIATION  0x2
#define EGS_SORT_BALLOT_RANK           0x4
int egs_forward_sort_plan(int P, int64_t capacity, int width, int height, int flags);

/* ---- the launch geometry of the tile bucketing of a forward (added within ABI 6: new entries only).
 * The bucketing (count pass, table scan, scatter pass) deals the model's 256-Gaussian blocks to `nblocks` workgroups, which take their
 * 64-Gaussian groups `gpr` at a time.  All of it is host arithmetic on the model size, the image size and the call's EGS_CALL_* flags (of
 * which only EGS_CALL_KEEP_ALL_INSTANCES is read); this entry returns what the launches of such a forward act on -- the same function
 * decides inside the forward.  It launches no device work and needs no device.
 *   n_tiles, gx        tiles of the image, tiles per row
 *   nblocks            bucketing workgroups = columns of the [tile][workgroup] count table that are in use
 *   stride             row pitch of that table in words (a power of two >= 4 and >= nblocks)
 *   n_chunks           2048-entry scan chunks of the table = workgroups of its scan
 *   gpr                groups a workgroup sets up per round
 *   cull               1: the walk drops the instances whose tile the splat cannot reach (0 with EGS_CALL_KEEP_ALL_INSTANCES)
 *   use_map            1: the walk finds a slot's Gaussian through the owner map in LDS, 0: by binary search only
 *   lds                bytes of dynamic LDS of the bucketing workgroups
 *   groups_per_block   groups of the busiest workgroup;  rounds = ceil(groups_per_block / gpr)
 *   prefixed           1: the table is large enough for its scan to be preceded by a prefix pass over the chunk sums
 *   can_fuse           1: the count pass of this geometry can run inside the preprocess launch (what egs_forward_fuses_count answers for a
 *                      call without EGS_CALL_SEPARATE_COUNT)
 * P == 0: nothing is bucketed, every field but n_tiles and gx is 0.
 * -> 0, EGS_ERR_ARG (out == NULL, P < 0, an image side <= 0) or EGS_ERR_RANGE (an image the forwards refuse). */
typedef struct egs_bin_geometry_info {
    int32_t n_tiles, gx, nblocks, stride, n_chunks, gpr, cull, use_map, groups_per_block, rounds, prefixed, can_fuse;
    int64_t lds;
} egs_bin_geometry_info;
int egs_forward_bin_geometry(int P, int width, int height, int flags, egs_bin_geometry_info* out);

/* ---- optional per-stage timing with HIP events on the caller's stream (bench / profiling aid) ------
 * The only process-wide state in the library; off by default.  egs_profile_begin allocates an event pool and
 * turns recording on; every stage launched afterwards is bracketed by two events on its stream;
 * egs_profile_end waits for the events, returns per-stage total milliseconds and launch counts, frees the pool. */
enum {
    EGS_K_PREPROCESS = 0, EGS_K_SCAN, EGS_K_DUPLICATE, EGS_K_SORT, EGS_K_RANGES, EGS_K_RENDER_FWD,
    EGS_K_RENDER_BWD, EGS_K_PREPROCESS_BWD, EGS_K_COUNT
};
int         egs_profile_begin(int max_records);
int         egs_profile_end(double* total_ms /*HOST [EGS_K_COUNT]*/, int* launches /*HOST [EGS_K_COUNT]*/);
const char* egs_profile_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* EGS_RASTER_H */
