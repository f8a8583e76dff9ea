// api.hip -- the C ABI of libegs_raster.so (declared in include/egs_raster.h): argument checks, carving
// of the three caller-owned byte buffers, and the launch sequence on the caller's stream.
// Replaces the pybind `_C` entry points of the upstream extension bound at
// /root/reference/gaussian_renderer/__init__.py:14.
#include "egs_common.h"
#include "object_motion.h"
#include "backward_prologue.h"
#include "loss_window.h"
#include "label_bce.h"
#include "opacity_entropy.h"
#include <string.h>
#include <vector>
#include <mutex>
#include <unordered_map>
#include <stdlib.h>

namespace {

struct GeomLayout { egs_geom_layout o; size_t bytes; };
struct BinLayout { egs_binning_layout o; size_t bytes; };
struct ImgLayout { egs_image_layout o; size_t bytes; };

GeomLayout geom_layout(int P) {
    GeomLayout L; size_t off = 0; const size_t n = (size_t)(P > 0 ? P : 0);
    L.o.rec = off;          off = egs_align(off + n * sizeof(float4) * EGS_SPLAT_REC_F4);
    L.o.rect = off;         off = egs_align(off + n * sizeof(uint2));
    L.o.offsets = off;      off = egs_align(off + n * sizeof(uint32_t));
    L.o.clamped = off;      off = egs_align(off + n);
    L.o.visible = off;      off = egs_align(off + n);
    L.o.scan_scratch = off; off = egs_align(off + (2 * ((n + 255) / 256) + 64) * sizeof(uint32_t)); // per-block instance counts, 64 spare words, per-block hot counts
    L.o.total = off;        off = egs_align(off + sizeof(uint64_t));
    L.bytes = off; return L;
}
BinLayout bin_layout(int P, int64_t R, int W, int H) {
    BinLayout L; size_t off = 0; const size_t n = (size_t)(R > 0 ? R : 0);
    const size_t nt = egs_tiles(W, H);
    const size_t nblocks = egs_bin_blocks(P > 0 ? P : 0), stride = egs_table_stride((uint32_t)nblocks), tab = nt * stride;
    const size_t sums = EGS_BIN_GROUPS * egs_table_chunks(nt, (uint32_t)stride);
    L.o.key_bits = egs_key_bits_for_tiles((int)nt);
    L.o.bin_blocks = (int)nblocks;
    L.o.table_stride = (int)stride;
    int ib = 0; while (P > 1 && (((unsigned)(P - 1)) >> ib) != 0) ib++;
    L.o.index_passes = (ib + 8) / 9;
    L.o.point_list = off; off = egs_align(off + n * sizeof(uint32_t));          // first: the backward needs nothing else
    L.o.pairs = off;      off = egs_align(off + n * sizeof(uint64_t));
    L.o.scratch = off;    off = egs_align(off + n * sizeof(uint64_t));
    L.o.table = off;      off = egs_align(off + (n ? tab : 0) * sizeof(uint32_t));
    L.o.spine = off;      off = egs_align(off + (n ? sums + 64 + 4 : 0) * sizeof(uint32_t));
    L.o.total = L.o.spine + ((sums + 32 + 1) & ~(size_t)1) * sizeof(uint32_t);
    L.bytes = off; return L;
}
ImgLayout img_layout(int W, int H) {
    ImgLayout L; size_t off = 0;
    const size_t nt = egs_tiles(W, H), px = (size_t)W * H;
    L.o.ranges = off;    off = egs_align(off + nt * sizeof(uint2));
    L.o.final_T = off;   off = egs_align(off + px * sizeof(float));
    L.o.n_contrib = off; off = egs_align(off + px * sizeof(uint32_t));
    L.o.quad_work = off; off = egs_align(off + nt * 4 * sizeof(uint32_t));
    L.o.tile_order = off; off = egs_align(off + (size_t)egs_blocks_for_tiles((int)nt) * sizeof(uint32_t));       // EGS_XCDS bands of egs_tiles_per_xcd() slots
    L.o.quad_pairs = off; off = egs_align(off + nt * 8 * sizeof(uint32_t));                 // pairs [tiles][4], then visits [tiles][4]
    L.bytes = off; return L;
}
EgsGeomPtrs geom_ptrs(void* buf, int P) {
    const GeomLayout L = geom_layout(P); char* b = (char*)buf; EgsGeomPtrs g;
    g.rec = (float4*)(b + L.o.rec); g.rect = (uint2*)(b + L.o.rect); g.offsets = (uint32_t*)(b + L.o.offsets);
    g.clamped = (uint8_t*)(b + L.o.clamped); g.visible = (uint8_t*)(b + L.o.visible); g.scan_scratch = (uint32_t*)(b + L.o.scan_scratch);
    g.total = (uint64_t*)(b + L.o.total);
    g.block_hot = g.scan_scratch + ((size_t)(P > 0 ? P : 0) + 255) / 256 + 64;
    return g;
}
EgsBinPtrs bin_ptrs(void* buf, int P, int64_t R, int W, int H) {
    const BinLayout L = bin_layout(P, R, W, H); char* b = (char*)buf; EgsBinPtrs p;
    p.pairs = (uint64_t*)(b + L.o.pairs); p.scratch = (uint64_t*)(b + L.o.scratch);
    p.point_list = (uint32_t*)(b + L.o.point_list); p.table = (uint32_t*)(b + L.o.table); p.chunk_sum = (uint32_t*)(b + L.o.spine);
    p.total = (uint64_t*)(b + L.o.total);
    p.flag = (uint32_t*)p.total - 32;                                 // (the 32 words before `total`)
    p.zero_after = nullptr; p.zero_after_n = 0;
    return p;
}
EgsImgPtrs img_ptrs(void* buf, int W, int H) {
    const ImgLayout L = img_layout(W, H); char* b = (char*)buf; EgsImgPtrs p;
    p.ranges = (uint2*)(b + L.o.ranges); p.final_T = (float*)(b + L.o.final_T);
    p.n_contrib = (uint32_t*)(b + L.o.n_contrib); p.quad_work = (uint32_t*)(b + L.o.quad_work);
    p.tile_order = (uint32_t*)(b + L.o.tile_order); p.quad_pairs = (uint32_t*)(b + L.o.quad_pairs);
    p.fwd_cost = nullptr; p.fwd_order = nullptr; return p;                // (set from the caller's placement buffer, forward_impl)
}

int check_dims(int P, int W, int H) {
    if (P < 0 || W <= 0 || H <= 0) return EGS_ERR_ARG;
    if (W > 32767 || H > 32767) return EGS_ERR_RANGE;                    // 15-bit pixel coordinates in the record's box (egs_common.h)
    if (egs_tiles(W, H) > EGS_MAX_TILES) return EGS_ERR_RANGE;
    return 0;
}
// The three opaque buffers hold 16-byte vectors at 256-byte-aligned offsets (float4 records, uint4 table words, 64-bit pairs): their
// base addresses must be 256-byte aligned (include/egs_raster.h, Conventions).  NULL passes: emptiness is checked where it matters.
static inline bool misaligned(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 255u) != 0;
}
int check_modes(const EgsScene& sc) {
    const float* shs = sc.shs; const float* colors = sc.colors; const float* scales = sc.scales; const float* rots = sc.rots; const float* cov = sc.cov3D;
    const int act = sc.act;
    if (act & ~(EGS_ACT_LOG_SCALES | EGS_ACT_RAW_QUATS | EGS_ACT_LOGIT_OPACITY | EGS_ACT_OBJECT_MOTION | EGS_ACT_SCALAR_COLOR)) return EGS_ERR_MODE;
    if ((act & EGS_ACT_SCALAR_COLOR) && !colors) return EGS_ERR_MODE;                               // one value per Gaussian: of colors_precomp
    if ((act & (EGS_ACT_LOG_SCALES | EGS_ACT_RAW_QUATS)) && cov != nullptr) return EGS_ERR_MODE;   // nothing to activate: the covariance is given
    if ((shs != nullptr) == (colors != nullptr)) return EGS_ERR_MODE;
    const bool sr = scales != nullptr && rots != nullptr;
    if ((scales != nullptr) != (rots != nullptr)) return EGS_ERR_MODE;
    if (sr == (cov != nullptr)) return EGS_ERR_MODE;
    return 0;
}
// split spherical harmonics: shs_rest goes with shs = the DC block and at least two coefficients
inline bool split_sh_malformed(const EgsScene& sc) { return sc.shs_rest && (!sc.shs || sc.M < 2); }
// pointers every rasterizer call with P > 0 needs (the forwards add the opacities: the backwards read them in the record)
inline bool lacks_pointers(const EgsScene& sc, const EgsCamera& cam, const void* radii, const void* geom) {
    return !sc.means3D || !cam.view || !cam.proj || !cam.campos || !radii || !geom;
}

#define EGS_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)
#define EGS_SYNC_IF_DEBUG(s) do { if (debug & EGS_CALL_SYNC) { EGS_TRY(hipStreamSynchronize(s)); EGS_TRY(hipGetLastError()); } } while (0)

// ---- stage timing pool -----------------------------------------------------------------------------
struct ProfRec { int stage; hipEvent_t a, b; bool closed; };
ProfRec* g_prof = nullptr; int g_prof_cap = 0, g_prof_n = 0; int g_prof_open[EGS_K_COUNT];

}  // namespace

void egs_prof_start(int stage, hipStream_t s) {
    if (!g_prof || g_prof_n >= g_prof_cap) return;
    ProfRec& r = g_prof[g_prof_n];
    r.stage = stage; r.closed = false;
    if (hipEventRecord(r.a, s) != hipSuccess) return;
    g_prof_open[stage] = g_prof_n++;
}
void egs_prof_stop(int stage, hipStream_t s) {
    if (!g_prof) return;
    const int i = g_prof_open[stage];
    if (i < 0) return;
    if (hipEventRecord(g_prof[i].b, s) == hipSuccess) g_prof[i].closed = true;
    g_prof_open[stage] = -1;
}

extern "C" {

int egs_profile_begin(int max_records) {
    if (g_prof || max_records <= 0) return EGS_ERR_ARG;
    g_prof = new ProfRec[max_records];
    for (int i = 0; i < max_records; i++) {
        if (hipEventCreate(&g_prof[i].a) != hipSuccess || hipEventCreate(&g_prof[i].b) != hipSuccess) return EGS_ERR_NO_DEVICE;
        g_prof[i].closed = false;
    }
    for (int k = 0; k < EGS_K_COUNT; k++) g_prof_open[k] = -1;
    g_prof_cap = max_records; g_prof_n = 0;
    return 0;
}
int egs_profile_end(double* total_ms, int* launches) {
    if (!g_prof || !total_ms || !launches) return EGS_ERR_ARG;
    for (int k = 0; k < EGS_K_COUNT; k++) { total_ms[k] = 0.0; launches[k] = 0; }
    for (int i = 0; i < g_prof_n; i++) {
        if (!g_prof[i].closed) continue;
        float ms = 0.f;
        if (hipEventSynchronize(g_prof[i].b) == hipSuccess && hipEventElapsedTime(&ms, g_prof[i].a, g_prof[i].b) == hipSuccess) {
            total_ms[g_prof[i].stage] += ms; launches[g_prof[i].stage]++;
        }
    }
    for (int i = 0; i < g_prof_cap; i++) { (void)hipEventDestroy(g_prof[i].a); (void)hipEventDestroy(g_prof[i].b); }
    delete[] g_prof; g_prof = nullptr; g_prof_cap = g_prof_n = 0;
    return 0;
}
const char* egs_profile_stage_name(int stage) {
    static const char* n[EGS_K_COUNT] = { "preprocess", "scan", "tile_bucket", "tile_sort", "tile_ranges", "render_forward",
                                          "render_backward", "preprocess_backward" };
    return stage >= 0 && stage < EGS_K_COUNT ? n[stage] : "?";
}

int egs_abi_version(void) { return EGS_ABI_VERSION; }
#ifndef EGS_SOURCE_HASH
#define EGS_SOURCE_HASH "unknown"
#endif
const char* egs_source_hash(void) { return EGS_SOURCE_HASH; }

#ifdef EGS_LG_CHECK
// experiment hook: the next backward blends compute the image-loss gradient themselves (all NULL: off)
int egs_debug_set_lossgrad(const float* img, const float* gt, const float* m0, const float* m1, const float* m2, const float* gate,
                           const float* upstream, float lambda_dssim) {
    egs_debug_lossgrad = EgsLossGradHost{ img, gt, m0, m1, m2, gate, upstream, nullptr, 1.f - lambda_dssim, lambda_dssim };
    return 0;
}
#endif
// Per-call flags (include/egs_raster.h EGS_CALL_*, ABI 6): what used to be process-wide switches (egs_debug_set_tile_culling / _fused_count /
// _sort_in_blend / egs_debug_force_ballot_rank through ABI 5) travels in the last argument of the call it applies to; the library keeps none of it.
static inline bool fused_count_on(int flags) { return !(flags & EGS_CALL_SEPARATE_COUNT); }
static inline int cull_on(int flags) { return (flags & EGS_CALL_KEEP_ALL_INSTANCES) ? 0 : 1; }
int egs_forward_fuses_count(int P, int width, int height, int flags) { return (fused_count_on(flags) && egs_can_fuse_count(P, width, height, cull_on(flags))) ? 1 : 0; }
// (the rule itself: binning.hip egs_sort_plan, which egs_launch_binning acts on)
int egs_forward_sort_plan(int P, int64_t capacity, int width, int height, int flags) {
    if (P <= 0 || capacity <= 0 || width <= 0 || height <= 0) return 0;
    return egs_sort_plan(P, capacity, (int)egs_tiles(width, height), flags);
}
// (the rules themselves: binning.hip egs_bin_geometry / egs_table_scan_prefixed, bin_walk.h bin_groups_per_block, preprocess.hip egs_can_fuse_count)
int egs_forward_bin_geometry(int P, int width, int height, int flags, egs_bin_geometry_info* out) {
    if (!out) return EGS_ERR_ARG;
    if (int rc = check_dims(P, width, height)) return rc;
    const int cull = cull_on(flags);
    const EgsBinGeometry q = egs_bin_geometry(P, width, height, cull);
    egs_bin_geometry_info o = {};
    o.n_tiles = q.n_tiles; o.gx = q.gx;
    if (P > 0) {
        o.nblocks = (int32_t)q.nblocks; o.stride = (int32_t)q.stride; o.n_chunks = (int32_t)q.n_chunks;
        o.gpr = q.gpr; o.cull = q.cull; o.use_map = q.use_map; o.lds = (int64_t)q.lds;
        o.groups_per_block = (int32_t)egs_bin_groups_per_block(P);
        o.rounds = (o.groups_per_block + q.gpr - 1) / q.gpr;
        o.prefixed = egs_table_scan_prefixed(q.n_chunks);
        o.can_fuse = egs_can_fuse_count(P, width, height, cull) ? 1 : 0;
    }
    *out = o;
    return 0;
}

const char* egs_error_string(int code) {
    switch (code) {
        case 0: return "ok";
        case EGS_ERR_ARG: return "egs: invalid argument (null pointer or negative size)";
        case EGS_ERR_MODE: return "egs: provide exactly one of {shs, colors_precomp} and exactly one of {cov3D_precomp, (scales, rotations)}";
        case EGS_ERR_RANGE: return "egs: size outside the supported range";
        case EGS_ERR_NO_DEVICE: return "egs: no usable HIP device";
        case EGS_RETRY_LARGER: return "egs: binning capacity too small for this frame; call egs_forward_render with a buffer for R";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "egs: unknown error";
    }
}

int egs_device_info(char* name, int name_len, char* arch, int arch_len, int* compute_units) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return EGS_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    EGS_TRY(hipGetDeviceProperties(&prop, dev));
    if (name && name_len > 0) { strncpy(name, prop.name, (size_t)name_len - 1); name[name_len - 1] = 0; }
    if (arch && arch_len > 0) { strncpy(arch, prop.gcnArchName, (size_t)arch_len - 1); arch[arch_len - 1] = 0; }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    return 0;
}

size_t egs_geom_bytes(int P) { return geom_layout(P).bytes; }
size_t egs_binning_bytes(int P, int64_t R, int width, int height) { return bin_layout(P, R, width, height).bytes; }
size_t egs_image_bytes(int width, int height) { return img_layout(width, height).bytes; }
size_t egs_backward_scratch_bytes(int P) { return egs_align(egs_acc_floats((size_t)(P > 0 ? P : 0)) * sizeof(float)); }
size_t egs_backward_scratch_bytes_ex(int P, int flags) {
    return egs_backward_scratch_bytes(P) + ((flags & EGS_CALL_DETERMINISTIC) ? egs_det_bytes((size_t)(P > 0 ? P : 0)) : 0);
}
// EGS_CALL_DETERMINISTIC: the mode's lines behind the float accumulator, cleared here (the prologue, which the loss launch may have carried, clears
// the float lines only) -> where they are; NULL without the bit
static int det_lines_clear(void* scratch, int P, int flags, hipStream_t s, void** lines) {
    *lines = nullptr;
    if (!(flags & EGS_CALL_DETERMINISTIC)) return 0;
    *lines = (char*)scratch + egs_backward_scratch_bytes(P);
    EGS_TRY(egs_launch_zero_f4((float4*)*lines, egs_det_bytes((size_t)P) / 16, s));
    return 0;
}

int egs_get_geom_layout(int P, egs_geom_layout* out) { if (!out || P < 0) return EGS_ERR_ARG; *out = geom_layout(P).o; return 0; }
int egs_get_binning_layout(int P, int64_t R, int width, int height, egs_binning_layout* out) {
    if (!out || P < 0 || R < 0 || width <= 0 || height <= 0) return EGS_ERR_ARG;
    *out = bin_layout(P, R, width, height).o; return 0;
}
// placement buffer: [4 n_tiles] quadrant costs, [egs_blocks_for_tiles] the forward's tile order, then (256-byte aligned, ABI 5) the chunk sums
// of a fused count pass: EGS_BIN_GROUPS x n_tiles words (a table row never spans more than one scan chunk: n_chunks <= n_tiles)
static size_t placement_sums_offset(size_t nt) { return egs_align((nt * 4 + (size_t)egs_blocks_for_tiles((int)nt)) * sizeof(uint32_t)); }
static size_t placement_sums_words(size_t nt) { return (size_t)EGS_BIN_GROUPS * nt; }
size_t egs_placement_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t nt = egs_tiles(width, height);
    return egs_align(placement_sums_offset(nt) + placement_sums_words(nt) * sizeof(uint32_t));
}
// The sums region of a placement buffer must be ZERO when a fused forward starts: egs_placement_init() once per (buffer, image size), the
// chain itself leaves it zero again (include/egs_raster.h).  The library keeps no record of buffers (ABI 6; through ABI 5 a process-wide
// map of "clean" addresses stood here, which a freed-and-reallocated address could fool).
int egs_placement_init(void* placement, int width, int height, void* stream) {
    if (!placement || check_dims(0, width, height)) return EGS_ERR_ARG;
    const size_t nt = egs_tiles(width, height);
    EGS_TRY(egs_launch_zero_u32((uint32_t*)((char*)placement + placement_sums_offset(nt)), placement_sums_words(nt), (hipStream_t)stream));
    return 0;
}
// A chain that fails between the fused count pass and the launch that clears the sums would leave them dirty for the next frame: the failing
// call clears them itself on its way out (best effort; the caller gets the error code either way).
struct PlacementClearOnError {
    void* p = nullptr; int w = 0, h = 0; hipStream_t s = nullptr;
    ~PlacementClearOnError() { if (p) (void)egs_placement_init(p, w, h, (void*)s); }
};
static void placement_sums(void* placement, int width, int height, uint32_t** sums, uint32_t* words) {
    const size_t nt = egs_tiles(width, height);
    *sums = (uint32_t*)((char*)placement + placement_sums_offset(nt)); *words = (uint32_t)placement_sums_words(nt);
}
int egs_order_words(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return egs_blocks_for_tiles((int)egs_tiles(width, height));
}
static void placement_ptrs(void* placement, int width, int height, EgsImgPtrs& im) {
    const size_t nt = egs_tiles(width, height);
    im.fwd_cost = (uint32_t*)placement; im.fwd_order = placement ? (uint32_t*)placement + nt * 4 : nullptr;
}

int egs_get_image_layout(int width, int height, egs_image_layout* out) {
    if (!out || width <= 0 || height <= 0) return EGS_ERR_ARG;
    *out = img_layout(width, height).o; return 0;
}

// egs_object_rotation (HOST struct) -> kernel argument; needs the scales + rotations mode
static int obj_rot_args(const egs_object_rotation* rot, const float* scales, EgsObjRot& r) {
    r = EgsObjRot{ nullptr, nullptr, 1.f, nullptr };
    if (!rot || !rot->M9) return 0;
    if (!scales) return EGS_ERR_MODE;
    r.M = rot->M9; r.sel = rot->selected; r.mult = rot->row0_grad_mult; r.mult_dev = rot->row0_grad_mult_dev;
    return 0;
}
// With EGS_ACT_OBJECT_MOTION the `rot` argument points to an egs_object_motion (HOST struct): the rotation as above (rot.M9 may be NULL:
// covariances are not turned) plus the placement of the positions and, optionally, where the pose gradient goes.
struct MotionHost { EgsMotion k; float* grad; };
static int obj_motion_args(const EgsScene& sc, const egs_object_rotation* rot, EgsObjRot& r, MotionHost& m) {
    const float* scales = sc.scales; const int P = sc.P;
    m = MotionHost{ EgsMotion{ nullptr, nullptr, nullptr, nullptr }, nullptr };
    if (!(sc.act & EGS_ACT_OBJECT_MOTION)) return obj_rot_args(rot, scales, r);
    const egs_object_motion* om = reinterpret_cast<const egs_object_motion*>(rot);
    if (!om) return EGS_ERR_MODE;                                     // the bit without its struct: no such mode
    if (!om->A12 || (om->grad && !om->scratch)) return EGS_ERR_ARG;
    int rc = obj_rot_args(&om->rot, scales, r); if (rc) return rc;
    m.k.A = om->A12; m.k.moved = om->moved; m.grad = om->grad;
    if (om->grad) {
        m.k.pose_partial = (float*)om->scratch;
        if (r.M) m.k.dM_partial = (float*)om->scratch + egs_motion_rot_offset(P);
    }
    return 0;
}

// ---- the forwards: one record for the call ------------------------------------------------------------------------------------------
// What the two forwards ask of a scene of P > 0 Gaussians before they launch anything, in the order callers have always met it: pointers,
// modes, spherical-harmonics ranges, then the object rotation / motion (-> kernel arguments).
static int check_forward_scene(const EgsScene& sc, const EgsCamera& cam, const void* radii, const void* geom, const egs_object_rotation* rot,
                               EgsObjRot& orot, MotionHost& mh) {
    if (lacks_pointers(sc, cam, radii, geom) || !sc.opac) return EGS_ERR_ARG;
    int rc = check_modes(sc); if (rc) return rc;
    if (sc.shs && (sc.D < 0 || sc.D > EGS_MAX_SH_DEGREE || sc.M < (sc.D + 1) * (sc.D + 1))) return EGS_ERR_RANGE;
    if (split_sh_malformed(sc)) return EGS_ERR_MODE;
    return obj_motion_args(sc, rot, orot, mh);
}
// The three forwards name their scene and camera parameters alike (include/egs_raster.h): the run each copies into its records
#define FWD_SCENE { P, sh_degree, sh_coeffs, means3D, shs, shs_rest, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, activation_flags }
#define FWD_CAMERA { viewmatrix, projmatrix, campos, width, height, tan_fovx, tan_fovy }

int egs_forward_geometry(int P, int sh_degree, int sh_coeffs, const float* means3D, const float* shs, const float* shs_rest,
                         const float* colors_precomp, const float* opacities, const float* scales,
                         float scale_modifier, const float* rotations, const float* cov3D_precomp, int activation_flags,
                         const float* viewmatrix, const float* projmatrix, const float* campos, int width, int height,
                         float tan_fovx, float tan_fovy, int prefiltered, int32_t* radii, void* geom_buffer,
                         int64_t* num_rendered, const int32_t* active_count, const egs_object_rotation* rot, void* stream, int debug) {
    (void)prefiltered;
    const EgsScene sc = FWD_SCENE; const EgsCamera cam = FWD_CAMERA;
    int rc = check_dims(P, width, height); if (rc) return rc;
    if (!num_rendered) return EGS_ERR_ARG;
    *num_rendered = 0;
    if (P == 0) return 0;
    if (misaligned(geom_buffer)) return EGS_ERR_ARG;
    EgsObjRot orot; MotionHost mh; rc = check_forward_scene(sc, cam, radii, geom_buffer, rot, orot, mh); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    EgsGeomPtrs g = geom_ptrs(geom_buffer, P);
    egs_prof_start(EGS_K_PREPROCESS, s);
    EGS_TRY(egs_launch_preprocess(sc, cam, radii, g, nullptr, 0, active_count, nullptr, orot, mh.k, s));
    if (egs_sh_apart(sc)) EGS_TRY(egs_launch_sh_forward(sc, cam, g, mh.k, s));
    egs_prof_stop(EGS_K_PREPROCESS, s);
    EGS_SYNC_IF_DEBUG(s);
    // R = sum of the per-block instance counts (a few KB device->host; the only host wait of the forward)
    const size_t nb = ((size_t)P + 255) / 256;
    std::vector<uint32_t> sums(nb);
    EGS_TRY(hipMemcpyAsync(sums.data(), g.scan_scratch, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    EGS_TRY(hipStreamSynchronize(s));
    uint64_t R = 0;
    for (size_t k = 0; k < nb; k++) R += sums[k];
    if (R >= (1ull << 31)) return EGS_ERR_RANGE;
    *num_rendered = (int64_t)R;
    return 0;
}

// One call of egs_forward / egs_forward_enqueue: the scene, the camera, and everything else the prototypes list (include/egs_raster.h)
struct ForwardCall {
    EgsScene sc; EgsCamera cam;
    const float* background; int32_t* radii; void* geom_buffer; int64_t capacity; void* binning_buffer; void* image_buffer;
    float* out_color; float* out_depth; float* out_alpha; uint32_t* pinned_host_counts;
    bool wait_for_count;                 // egs_forward: the host waits for the instance count; egs_forward_enqueue: nothing waits (capturable)
    uint64_t* running_max; int64_t* num_rendered; const int32_t* active_count; uint32_t* overflow_flag; void* placement;
    const egs_object_rotation* rot; void* stream; int debug;
};
// One-call forward: preprocess, then -- without waiting for R -- the whole binning + blend chain is enqueued against
// the caller's capacity guess while the host waits only for the copy of the per-block instance counts.  The GPU never
// idles on the host round trip.  If the guess was too small nothing valid was produced: the true R is returned and the
// caller finishes with egs_forward_render on a buffer of the right size.
static int forward_impl(const ForwardCall& c) {
    const EgsScene& sc = c.sc; const EgsCamera& cam = c.cam;
    const int P = sc.P, width = cam.W, height = cam.H, debug = c.debug;
    const int64_t capacity = c.capacity;
    void* const placement = c.placement; uint32_t* const pinned_host_counts = c.pinned_host_counts;
    int rc = check_dims(P, width, height); if (rc) return rc;
    if (!c.num_rendered || capacity < 0 || capacity >= (1ll << 31)) return EGS_ERR_ARG;
    *c.num_rendered = 0;
    if (!c.background || !c.image_buffer || !c.out_color || ((c.out_depth != nullptr) != (c.out_alpha != nullptr))) return EGS_ERR_ARG;     // (depth and alpha: both or neither, ABI 4)
    if (misaligned(c.geom_buffer, c.binning_buffer, c.image_buffer)) return EGS_ERR_ARG;
    hipStream_t s = (hipStream_t)c.stream;
    if (P == 0) return egs_forward_render(0, 0, c.background, width, height, c.geom_buffer, c.binning_buffer, c.image_buffer, c.out_color,
                                          c.out_depth, c.out_alpha, c.stream, debug);
    if (c.wait_for_count && !pinned_host_counts) return EGS_ERR_ARG;
    if (capacity > 0 && !c.binning_buffer) return EGS_ERR_ARG;
    if (!c.wait_for_count && capacity <= 0) return EGS_ERR_ARG;
    EgsObjRot orot; MotionHost mh; rc = check_forward_scene(sc, cam, c.radii, c.geom_buffer, c.rot, orot, mh); if (rc) return rc;
    static thread_local hipEvent_t ev = nullptr;
    if (c.wait_for_count && !ev) EGS_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    EgsGeomPtrs g = geom_ptrs(c.geom_buffer, P);
    egs_prof_start(EGS_K_PREPROCESS, s);
    // the speculative bucketing that follows needs its chunk sums cleared: the preprocess launch does that on the side (a launch of
    // its own costs ~4.5 us of GPU time whatever it does)
    EgsBinPtrs b_spec = {};
    size_t n_sums = 0;
    if (capacity > 0) {
        b_spec = bin_ptrs(c.binning_buffer, P, capacity, width, height);
        n_sums = EGS_BIN_GROUPS * egs_table_chunks(egs_tiles(width, height), egs_table_stride(egs_bin_blocks(P)));
    }
    // ... and carries the placement of the forward blend's tiles (backward_prologue.h), computed from the costs the image buffer holds
    EgsImgPtrs im_spec = img_ptrs(c.image_buffer, width, height);
    placement_ptrs(placement, width, height, im_spec);
    // With a persistent placement buffer the count pass of the bucketing rides in the preprocess launch (k_preprocess_count) and adds its
    // chunk sums into that buffer's sums region, which is zero between frames (egs_common.h EgsBinPtrs); egs_debug_set_fused_count: A/B switch
    const bool fuse = capacity > 0 && placement && fused_count_on(debug) && egs_can_fuse_count(P, width, height, cull_on(debug));
    PlacementClearOnError dirty_guard;
    if (fuse) {
        dirty_guard.p = placement; dirty_guard.w = width; dirty_guard.h = height; dirty_guard.s = s;      // (disarmed once the bucketing chain is enqueued)
        placement_sums(placement, width, height, &b_spec.chunk_sum, &b_spec.zero_after_n);
        b_spec.zero_after = b_spec.chunk_sum;
        EGS_TRY(egs_launch_preprocess_count(sc, cam, c.radii, g, b_spec, c.active_count, &im_spec, orot, mh.k, cull_on(debug), s));
    } else
    EGS_TRY(egs_launch_preprocess(sc, cam, c.radii, g, capacity > 0 ? b_spec.chunk_sum : nullptr, n_sums, c.active_count,
                                  (capacity > 0 && placement) ? &im_spec : nullptr, orot, mh.k, s));
    if (egs_sh_apart(sc)) EGS_TRY(egs_launch_sh_forward(sc, cam, g, mh.k, s));
    egs_prof_stop(EGS_K_PREPROCESS, s);
    const size_t nb = ((size_t)P + 255) / 256;
    if (pinned_host_counts) EGS_TRY(hipMemcpyAsync(pinned_host_counts, g.scan_scratch, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (c.wait_for_count) EGS_TRY(hipEventRecord(ev, s));
    if (capacity > 0) {                                              // speculative: sized by the caller's guess
        EgsBinPtrs b = b_spec;
        EgsImgPtrs im = im_spec;
        // the per-tile sort inside the forward blend's launch (render_fwd.hip SORT): egs_launch_binning then makes no sort launch and says what the
        // blend needs; with the sums of a fused count pass to clear, a failure before the blend is enqueued leaves them dirty (dirty_guard)
        EgsSortArgs sort_args = {};
        EGS_TRY(egs_launch_binning(P, capacity, width, height, g, b, im, c.running_max, c.overflow_flag, 1, fuse ? 1 : 0,
                                   &sort_args, s, debug & ~EGS_CALL_SYNC));      // (speculative chain: never synchronised mid-way, so SYNC does not move its sort plan either)
        egs_prof_start(EGS_K_RENDER_FWD, s);
        EGS_TRY(egs_launch_render_forward(width, height, c.background, g, b.point_list, im, c.out_color, c.out_depth, c.out_alpha, placement ? 1 : 0, &sort_args, s));
        dirty_guard.p = nullptr;
        egs_prof_stop(EGS_K_RENDER_FWD, s);
        // a caller that checks LATER (egs_forward_enqueue outside a graph: the eager loop without a host wait per forward) also gets the
        // overflow word -- [0] clipped, [1] instances bucketed -- behind the counts, once the chain that writes it has run
        if (!c.wait_for_count && pinned_host_counts && c.overflow_flag)
            EGS_TRY(hipMemcpyAsync(pinned_host_counts + nb, c.overflow_flag, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    if (!c.wait_for_count) { *c.num_rendered = -1; return 0; }          // graph-capturable: no host wait at all
    EGS_TRY(hipEventSynchronize(ev));
    uint64_t R = 0;
    for (size_t k = 0; k < nb; k++) R += pinned_host_counts[k];
    if (R >= (1ull << 31)) return EGS_ERR_RANGE;
    *c.num_rendered = (int64_t)R;
    if ((int64_t)R > capacity || capacity == 0) return EGS_RETRY_LARGER;       // caller: egs_forward_render with a buffer for R
    EGS_SYNC_IF_DEBUG(s);
    return 0;
}
// ... the run the two one-call forwards share after the scene and the camera
#define FWD_RENDER background, radii, geom_buffer, capacity, binning_buffer, image_buffer, out_color, out_depth, out_alpha, pinned_host_counts

int egs_forward(int P, int sh_degree, int sh_coeffs, const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix, const float* campos,
                const float* background, int width, int height, float tan_fovx, float tan_fovy, int prefiltered,
                int32_t* radii, void* geom_buffer, int64_t capacity, void* binning_buffer, void* image_buffer,
                float* out_color, float* out_depth, float* out_alpha, uint32_t* pinned_host_counts, int64_t* num_rendered,
                const int32_t* active_count, void* placement, const egs_object_rotation* rot, void* stream, int debug) {
    (void)prefiltered;
    return forward_impl({ FWD_SCENE, FWD_CAMERA, FWD_RENDER, true, nullptr, num_rendered, active_count, nullptr, placement, rot, stream, debug });
}

// Same chain with NO host wait: everything is only enqueued, so the call can be captured into a hipGraph.  Overflow of
// `capacity` is detected afterwards, either from pinned_host_counts (optional copy of the per-workgroup rectangle counts;
// egs_sum_counts after synchronising) or from `running_max` (optional device uint64 that the chain raises to the number
// of instances it bucketed whenever that is larger -- one word a caller can read after any number of replays).
int egs_forward_enqueue(int P, int sh_degree, int sh_coeffs, const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
                        const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                        const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix, const float* campos,
                        const float* background, int width, int height, float tan_fovx, float tan_fovy, int prefiltered,
                        int32_t* radii, void* geom_buffer, int64_t capacity, void* binning_buffer, void* image_buffer,
                        float* out_color, float* out_depth, float* out_alpha, uint32_t* pinned_host_counts, uint64_t* running_max,
                        const int32_t* active_count, uint32_t* overflow_flag, void* placement, const egs_object_rotation* rot, void* stream, int flags) {
    (void)prefiltered;
    int64_t unused = 0;
    return forward_impl({ FWD_SCENE, FWD_CAMERA, FWD_RENDER, false, running_max, &unused, active_count, overflow_flag, placement, rot, stream,
                          flags & ~EGS_CALL_SYNC });                   // (nothing may wait: capturable)
}
#undef FWD_RENDER
#undef FWD_CAMERA
#undef FWD_SCENE

int64_t egs_sum_counts(int P, const uint32_t* pinned_host_counts) {
    if (P <= 0 || !pinned_host_counts) return 0;
    uint64_t R = 0;
    for (size_t k = 0, nb = ((size_t)P + 255) / 256; k < nb; k++) R += pinned_host_counts[k];
    return (int64_t)R;
}

int egs_forward_render(int P, int64_t R, const float* background, int width, int height, const void* geom_buffer,
                       void* binning_buffer, void* image_buffer, float* out_color, float* out_depth, float* out_alpha,
                       void* stream, int debug) {
    int rc = check_dims(P, width, height); if (rc) return rc;
    if (R < 0 || R >= (1ll << 31)) return EGS_ERR_RANGE;
    if (!background || !image_buffer || !out_color || ((out_depth != nullptr) != (out_alpha != nullptr))) return EGS_ERR_ARG;     // (depth and alpha: both or neither, ABI 4)
    if (P > 0 && !geom_buffer) return EGS_ERR_ARG;
    if (R > 0 && !binning_buffer) return EGS_ERR_ARG;
    if (misaligned(geom_buffer, binning_buffer, image_buffer)) return EGS_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    EgsGeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    EgsBinPtrs b = bin_ptrs(binning_buffer, P, R, width, height);
    EgsImgPtrs im = img_ptrs(image_buffer, width, height);
    EgsSortArgs sort_args = {};
    EGS_TRY(egs_launch_binning(P, R, width, height, g, b, im, nullptr, nullptr, 0, 0, &sort_args, s, debug));
    const uint32_t* point_list = b.point_list;
    egs_prof_start(EGS_K_RENDER_FWD, s);
    EGS_TRY(egs_launch_render_forward(width, height, background, g, point_list, im, out_color, out_depth, out_alpha, 0, &sort_args, s));
    egs_prof_stop(EGS_K_RENDER_FWD, s);
    EGS_SYNC_IF_DEBUG(s);
    return 0;
}

// egs_adam_sink (HOST struct of the C ABI) -> what the kernels take by value
static void sink_to_kernel_args(const egs_adam_sink* sink, const uint32_t* skip_flag, EgsSink& ks, EgsAdamTick& tick) {
    for (int l = 0; l < EGS_SINK_LEAVES; l++) {
        if (!sink->leaf[l].param) continue;
        ks.leaf[l].p = sink->leaf[l].param; ks.leaf[l].m = sink->leaf[l].exp_avg; ks.leaf[l].v = sink->leaf[l].exp_avg_sq;
        tick.step[l] = sink->leaf[l].step; tick.lr[l] = sink->leaf[l].lr;
    }
    ks.coef = sink->coef; ks.active_rows = sink->active_rows; ks.skip = skip_flag; ks.b1 = sink->beta1; ks.b2 = sink->beta2; ks.eps = sink->eps;
    tick.coef = sink->coef; tick.skip = skip_flag; tick.b1 = sink->beta1; tick.b2 = sink->beta2;
}

// egs_object_loss (HOST struct) -> what the kernels read (loss_window.h)
static int obj_loss_args(const egs_object_loss* o, int channels, int height, int width, float lambda_dssim, EgsObjLossK& k) {
    if (!o || !o->alpha || !o->obj_mask || channels <= 0 || height <= 0 || width <= 0) return EGS_ERR_ARG;
    const float hw = (float)height * (float)width, n = (float)channels * hw;
    k = EgsObjLossK{};
    k.alpha = o->alpha; k.mask = o->obj_mask; k.apartial = o->alpha_partial_sums; k.terms = o->terms;
    k.w_l1a = o->lambda_l1_alpha / hw; k.w_l2a2 = (2.f * o->lambda_l2_alpha) / hw;
    k.l_img = o->lambda_image; k.l_l1a = o->lambda_l1_alpha; k.l_l2a = o->lambda_l2_alpha; k.inv_hw = 1.f / hw;
    k.fin_w_l1 = (1.f - lambda_dssim) / n; k.fin_w_ssim = lambda_dssim / n;
    k.n_astrips = (unsigned)(egs_l1_ssim_partial_count(1, height, width) / 2);
    return 0;
}

// ---- the backwards: one record for the call -------------------------------------------------------------------------------------------
// One call of any of the five rasterizer backwards (include/egs_raster.h): the scene, the camera, the forward's buffers, the upstream
// gradients, where the gradients and statistics go, the fused optimizer and the loss terms an entry point may add (NULL: not this route).
struct BackwardCall {
    EgsScene sc; EgsCamera cam;
    const float* background; int64_t R; const int32_t* radii; const void* geom_buffer; const void* binning_buffer; const void* image_buffer;
    const float* dL_dout_color; const float* dL_dout_depth; const float* dL_dout_alpha;
    EgsGrads d; EgsStats st;
    const egs_adam_sink* sink; int prologue_done; const egs_object_rotation* rot; int grad_mask; void* scratch; void* stream; int debug;
    const egs_loss_grad* loss_grad; const egs_object_loss* obj_loss; const egs_opacity_entropy* entropy;
};
static int backward_impl(const BackwardCall& c) {
    const EgsScene& sc = c.sc; const EgsCamera& cam = c.cam; const EgsGrads& d = c.d; const EgsStats& st = c.st;
    const int P = sc.P, width = cam.W, height = cam.H, debug = c.debug;
    const int64_t R = c.R;
    const egs_adam_sink* sink = c.sink; const egs_opacity_entropy* entropy = c.entropy;
    const float* dL_dout_color = c.dL_dout_color;
    hipStream_t s = (hipStream_t)c.stream;
    int rc = check_dims(P, width, height); if (rc) return rc;
    if (sc.act & EGS_ACT_SCALAR_COLOR) return EGS_ERR_MODE;           // a scalar colour's gradient is egs_backward_label's: dL_dcolors here is [P,3]
    // the opacity-entropy term (egs_backward_entropy_lossgrad): the static stages' -- no object motion, and the opacities must get their gradient
    if (entropy) {
        if (!entropy->weight || !entropy->n_vis || (P > 0 && !entropy->scratch) || c.obj_loss) return EGS_ERR_ARG;
        if (sc.act & EGS_ACT_OBJECT_MOTION) return EGS_ERR_MODE;
    }
    EgsObjRot orot; MotionHost mh; rc = obj_motion_args(sc, c.rot, orot, mh); if (rc) return rc;
    // the image loss's gradient computed by the blend itself (egs_backward_lossgrad): colour gradients only, three channels
    EgsLossGradHost lgh = {}; const EgsLossGradHost* lgp = nullptr; EgsObjLossK olk = {};
    if (c.obj_loss && !c.loss_grad) return EGS_ERR_ARG;
    if (c.loss_grad) {
        const egs_loss_grad& q = *c.loss_grad;
        if (!q.image || !q.gt || !q.dm_dmu1 || !q.dm_dexx || !q.dm_dexy || !q.upstream_grad) return EGS_ERR_ARG;
        if (c.dL_dout_depth || c.dL_dout_alpha || (c.grad_mask == EGS_GRAD_COLORS && sc.colors && !sink && !st.grad_accum)) return EGS_ERR_MODE;
        lgh = EgsLossGradHost{ q.image, q.gt, q.dm_dmu1, q.dm_dexx, q.dm_dexy, q.gate, q.upstream_grad, nullptr, 1.f - q.lambda_dssim, q.lambda_dssim,
                               q.deferred_partial_sums, q.deferred_partial_sums ? egs_l1_ssim_partial_count(3, height, width) / 2 : 0, q.lambda_dssim,
                               q.deferred_loss, q.deferred_partial_sums ? q.loss_running_sum : nullptr };
        lgp = &lgh;
        if (!dL_dout_color) dL_dout_color = q.image;                 // (never read: the checks below want a pointer)
        if (c.obj_loss) {
            // the object stages' loss: the image weights carry lambda_image, the blend also forms dL/dalpha (k_render_backward<2, true>)
            if (q.deferred_partial_sums && !c.obj_loss->alpha_partial_sums) return EGS_ERR_ARG;
            rc = obj_loss_args(c.obj_loss, 3, height, width, q.lambda_dssim, olk); if (rc) return rc;
            lgh.w_l1_n = c.obj_loss->lambda_image * (1.f - q.lambda_dssim); lgh.w_ssim_n = c.obj_loss->lambda_image * q.lambda_dssim;
            lgh.obj = &olk;
        }
    }
    if (P == 0) {
        if (lgp) EGS_TRY(egs_launch_loss_finish(lgh, width, height, s));
        if (entropy) EGS_TRY(egs_launch_entropy_reduce(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, entropy->n_vis, entropy->value, s));
        if (mh.grad) EGS_TRY(egs_launch_zero_u32((uint32_t*)mh.grad, EGS_MOTION_SUMS, s));
        return 0;
    }
    if (R < 0 || R >= (1ll << 31)) return EGS_ERR_RANGE;
    if (c.grad_mask & ~EGS_GRAD_MASK_BITS) return EGS_ERR_ARG;
    // Only the precomputed colours' gradient is wanted (the reference's label call): a blend that sums w dL/dC alone, no preprocess backward
    const bool colors_only = c.grad_mask == EGS_GRAD_COLORS && sc.colors && !sink && !st.grad_accum;
    if (!c.background || lacks_pointers(sc, cam, c.radii, c.geom_buffer) || !c.image_buffer || !dL_dout_color || (!d.means2D && !colors_only) || !c.scratch)
        return EGS_ERR_ARG;
    if (misaligned(c.geom_buffer, c.binning_buffer, c.image_buffer) || ((uintptr_t)c.scratch & 63u)) return EGS_ERR_ARG;      // (accumulator lines: 64 bytes on 64-byte boundaries)
    EgsGeomPtrs g = geom_ptrs(const_cast<void*>(c.geom_buffer), P);
    float* grad_acc = (float*)c.scratch;
    if (colors_only) {
        if (entropy) return EGS_ERR_MODE;                             // (no opacity gradient on this path)
        if (!d.colors || (R > 0 && !c.binning_buffer)) return EGS_ERR_ARG;
        rc = check_modes(sc); if (rc) return rc;
        if (R == 0) return (int)egs_launch_zero_u32((uint32_t*)d.colors, (size_t)P * 3, s);
        EgsBinPtrs b = bin_ptrs(const_cast<void*>(c.binning_buffer), P, R, width, height);
        EgsImgPtrs im = img_ptrs(const_cast<void*>(c.image_buffer), width, height);
        if (!c.prologue_done) EGS_TRY(egs_launch_backward_prologue(P, width, height, im, grad_acc, g.block_hot, nullptr, s));
        void* det = nullptr; rc = det_lines_clear(c.scratch, P, debug, s, &det); if (rc) return rc;
        egs_prof_start(EGS_K_RENDER_BWD, s);
        EGS_TRY(egs_launch_render_backward(P, width, height, c.background, g, b.point_list, im, dL_dout_color, nullptr, nullptr, grad_acc, 1, nullptr, s, det));
        egs_prof_stop(EGS_K_RENDER_BWD, s);
        EGS_SYNC_IF_DEBUG(s);
        egs_prof_start(EGS_K_PREPROCESS_BWD, s);
        EGS_TRY(egs_launch_colors_from_acc(P, grad_acc, g.clamped, c.radii, d.colors, s));
        if (mh.grad) EGS_TRY(egs_launch_zero_u32((uint32_t*)mh.grad, EGS_MOTION_SUMS, s));       // (the positions carry no gradient on this path)
        egs_prof_stop(EGS_K_PREPROCESS_BWD, s);
        EGS_SYNC_IF_DEBUG(s);
        return 0;
    }
    // leaves a fused optimizer owns: their gradient arrays are optional
    const bool sh_apart = egs_sh_apart(sc);
    bool own[EGS_SINK_LEAVES] = { false, false, false, false, false, false };
    const bool sh_sink_ok = sh_apart && egs_sh_backward_can_sink(sc.M, sc.shs, sc.shs_rest);      // the split M = 16 kernel steps dc / rest / positions
    if (sink) {
        if (!sink->coef) return EGS_ERR_ARG;
        for (int l = 0; l < EGS_SINK_LEAVES; l++) {
            const egs_adam_leaf& f = sink->leaf[l];
            own[l] = f.param != nullptr;
            if (own[l] && (!f.exp_avg || !f.exp_avg_sq || !f.lr || !f.step)) return EGS_ERR_ARG;
        }
        if ((own[EGS_SINK_SCALES] || own[EGS_SINK_ROTATIONS]) && sc.cov3D) return EGS_ERR_MODE;
        if (own[EGS_SINK_SH] && (!sc.shs || (sh_apart && !sh_sink_ok))) return EGS_ERR_MODE;
        if (own[EGS_SINK_SH_REST] && (!sh_sink_ok || sink->leaf[EGS_SINK_SH_REST].param != sc.shs_rest)) return EGS_ERR_MODE;
        if (own[EGS_SINK_MEANS3D] && sh_apart && (!sh_sink_ok || !d.means3D)) return EGS_ERR_MODE;
        if (sh_apart && (own[EGS_SINK_SH] || own[EGS_SINK_SH_REST]) && ((d.sh != nullptr) != (d.sh_rest != nullptr))) return EGS_ERR_ARG;
        if ((own[EGS_SINK_MEANS3D] && sink->leaf[EGS_SINK_MEANS3D].param != sc.means3D) || (own[EGS_SINK_SCALES] && sink->leaf[EGS_SINK_SCALES].param != sc.scales) ||
            (own[EGS_SINK_ROTATIONS] && sink->leaf[EGS_SINK_ROTATIONS].param != sc.rots) || (own[EGS_SINK_SH] && sink->leaf[EGS_SINK_SH].param != sc.shs))
            return EGS_ERR_ARG;
    }
    if ((!d.colors && (sc.colors || sh_apart)) || (!d.opacity && !own[EGS_SINK_OPACITY]) || (!d.means3D && !own[EGS_SINK_MEANS3D]))
        return EGS_ERR_ARG;
    if (R > 0 && !c.binning_buffer) return EGS_ERR_ARG;
    rc = check_modes(sc); if (rc) return rc;
    if (sc.shs && !d.sh && !own[EGS_SINK_SH]) return EGS_ERR_ARG;
    if (sh_apart && !d.sh && !(own[EGS_SINK_SH] && (own[EGS_SINK_SH_REST] || !sc.shs_rest))) return EGS_ERR_ARG;
    if (split_sh_malformed(sc)) return EGS_ERR_MODE;
    if (!sc.shs_rest && d.sh_rest) return EGS_ERR_ARG;
    if (sc.shs_rest && !d.sh_rest && !own[EGS_SINK_SH_REST]) return EGS_ERR_ARG;
    if ((st.grad_accum != nullptr) != (st.denom != nullptr) || (st.max_radii && !st.grad_accum)) return EGS_ERR_ARG;
    if (!sc.cov3D && ((!d.scales && !own[EGS_SINK_SCALES]) || (!d.rotations && !own[EGS_SINK_ROTATIONS]))) return EGS_ERR_ARG;
    if (sc.cov3D && !d.cov3D) return EGS_ERR_ARG;
    EgsBinPtrs b = bin_ptrs(const_cast<void*>(c.binning_buffer), P, R, width, height);
    EgsImgPtrs im = img_ptrs(const_cast<void*>(c.image_buffer), width, height);
    EgsSink ks = {}, ks_sh = {}; EgsAdamTick tick = {};
    bool pp_sinks = false, sh_sinks = false;
    if (sink) {
        sink_to_kernel_args(sink, st.skip_flag, ks, tick);
        ks_sh = ks;
        for (int l = 0; l < EGS_SINK_LEAVES; l++) {                    // who finishes which gradient: the spherical-harmonics launch, or the one before it
            const bool by_sh = sh_apart && (l == EGS_SINK_SH || l == EGS_SINK_SH_REST || l == EGS_SINK_MEANS3D);
            if (by_sh) ks.leaf[l] = EgsSinkLeaf{ nullptr, nullptr, nullptr }; else ks_sh.leaf[l] = EgsSinkLeaf{ nullptr, nullptr, nullptr };
            pp_sinks = pp_sinks || ks.leaf[l].p; sh_sinks = sh_sinks || ks_sh.leaf[l].p;
        }
    }
    // the accumulator is cleared by a kernel, not a memset node (see egs_launch_zero_f4): fused into the blend's prologue
    if (R == 0 && !c.prologue_done) {
        EGS_TRY(egs_launch_zero_f4((float4*)grad_acc, egs_acc_floats((size_t)P) / 4, s));
        if (sink) EGS_TRY(egs_launch_adam_tick(tick, s));
    }
    if (R == 0 && lgp) EGS_TRY(egs_launch_loss_finish(lgh, width, height, s));
    if (R > 0) {
        if (!c.prologue_done) EGS_TRY(egs_launch_backward_prologue(P, width, height, im, grad_acc, g.block_hot, sink ? &tick : nullptr, s));
        void* det = nullptr; rc = det_lines_clear(c.scratch, P, debug, s, &det); if (rc) return rc;
        egs_prof_start(EGS_K_RENDER_BWD, s);                         // (the stage is the blend kernel alone; deterministic: its two passes and the decode)
        EGS_TRY(egs_launch_render_backward(P, width, height, c.background, g, b.point_list, im, dL_dout_color, c.dL_dout_depth, c.dL_dout_alpha, grad_acc, 0, lgp, s, det));
        egs_prof_stop(EGS_K_RENDER_BWD, s);
        EGS_SYNC_IF_DEBUG(s);
    }
    egs_prof_start(EGS_K_PREPROCESS_BWD, s);
    // the entropy term: n_vis and the value from the records and radii of this frame, then the instantiation that adds the rows' shares
    EgsEntropy ek = {};
    if (entropy) {
        EGS_TRY(egs_launch_entropy_reduce(P, nullptr, g.rec, 0, c.radii, nullptr, nullptr, entropy->scratch, entropy->n_vis, entropy->value, s));
        ek = EgsEntropy{ entropy->n_vis, entropy->weight, entropy->upstream };
    }
    EGS_TRY(egs_launch_preprocess_backward(sc, cam, c.radii, g, grad_acc, d, st, pp_sinks ? &ks : nullptr, orot, mh.k, s, entropy ? &ek : nullptr));
    if (sh_apart) EGS_TRY(egs_launch_sh_backward(sc, cam, c.radii, g, d, sh_sinks ? &ks_sh : nullptr, mh.k, s));
    // the pose gradient: the lines the launch that finished the positions' gradient wrote (one per 64 rows from the spherical-harmonics
    // launch, per 256 otherwise), and the rotation lines of the preprocess backward, added up by one workgroup
    if (mh.grad) EGS_TRY(egs_launch_motion_finish(mh.k.pose_partial, (int)(sh_apart ? egs_motion_pose_lines_max(P) : egs_motion_rot_lines(P)),
                                                  mh.k.dM_partial, mh.k.dM_partial ? (int)egs_motion_rot_lines(P) : 0, mh.grad, s));
    egs_prof_stop(EGS_K_PREPROCESS_BWD, s);
    EGS_SYNC_IF_DEBUG(s);
    return 0;
}

// The five backwards name their shared parameters alike (include/egs_raster.h): the runs each copies into its call record.  Between
// BWD_SCENE and BWD_OUTPUTS stands what an entry point has of its own -- upstream gradients, or the loss whose gradient the blend forms.
#define BWD_SCENE { P, sh_degree, sh_coeffs, means3D, shs, shs_rest, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp, activation_flags }, \
                  { viewmatrix, projmatrix, campos, width, height, tan_fovx, tan_fovy }, background, R, radii, geom_buffer, binning_buffer, image_buffer
#define BWD_OUTPUTS { dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dsh_rest, dL_dscales, dL_drotations }, \
                    { stat_grad_accum, stat_denom, stat_max_radii, skip_flag }
#define BWD_SINK_TAIL sink, prologue_done, rot, grad_mask, scratch, stream, debug

int egs_backward(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                 const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                 const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                 const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                 const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha, float* dL_dmeans2D,
                 float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                 float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                 const uint32_t* skip_flag, int grad_mask, void* scratch, void* stream, int debug) {
    if (grad_mask == EGS_GRAD_COLORS && colors_precomp && !stat_grad_accum) { if (!dL_dcolors) return P == 0 ? 0 : EGS_ERR_ARG; }
    else if (!dL_dcolors || !dL_dopacity || !dL_dmeans3D) return P == 0 ? 0 : EGS_ERR_ARG;
    return backward_impl({ BWD_SCENE, dL_dout_color, dL_dout_depth, dL_dout_alpha, BWD_OUTPUTS, nullptr, 0, nullptr, grad_mask, scratch, stream, debug,
                           nullptr, nullptr, nullptr });
}

int egs_backward_adam(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                      const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                      const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                      const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                      const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha, float* dL_dmeans2D,
                      float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                      float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                      const uint32_t* skip_flag, const egs_adam_sink* sink, int prologue_done, const egs_object_rotation* rot, int grad_mask, void* scratch,
                      void* stream, int debug) {
    return backward_impl({ BWD_SCENE, dL_dout_color, dL_dout_depth, dL_dout_alpha, BWD_OUTPUTS, BWD_SINK_TAIL, nullptr, nullptr, nullptr });
}

int egs_backward_lossgrad(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                          const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                          const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const egs_loss_grad* loss_grad,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                          float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                          const uint32_t* skip_flag, const egs_adam_sink* sink, int prologue_done, const egs_object_rotation* rot, int grad_mask, void* scratch,
                          void* stream, int debug) {
    if (!loss_grad) return EGS_ERR_ARG;
    return backward_impl({ BWD_SCENE, nullptr, nullptr, nullptr, BWD_OUTPUTS, BWD_SINK_TAIL, loss_grad, nullptr, nullptr });
}

int egs_backward_entropy_lossgrad(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                          const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                          const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const egs_loss_grad* loss_grad,
                          const egs_opacity_entropy* entropy, const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                          float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                          const uint32_t* skip_flag, const egs_adam_sink* sink, int prologue_done, const egs_object_rotation* rot, int grad_mask, void* scratch,
                          void* stream, int debug) {
    if (!entropy) return EGS_ERR_ARG;
    if (loss_grad && (dL_dout_color || dL_dout_depth || dL_dout_alpha)) return EGS_ERR_MODE;      // (the blend forms the image gradient itself)
    return backward_impl({ BWD_SCENE, dL_dout_color, dL_dout_depth, dL_dout_alpha, BWD_OUTPUTS, BWD_SINK_TAIL, loss_grad, nullptr, entropy });
}

// egs_backward_prologue (HOST struct) -> the side jobs a loss backward launch carries
static int prologue_args(const egs_backward_prologue* side, EgsPrologueArgs& pa) {
    int rc = check_dims(side->P, side->width, side->height); if (rc) return rc;
    if (side->P <= 0 || !side->image_buffer || !side->scratch || ((uintptr_t)side->scratch & 63u)) return EGS_ERR_ARG;
    EgsImgPtrs im = img_ptrs(side->image_buffer, side->width, side->height);
    pa.n_tiles = (int)egs_tiles(side->width, side->height);
    pa.quad_work = im.quad_work; pa.tile_order = im.tile_order;
    if (side->geom_buffer && misaligned(side->geom_buffer)) return EGS_ERR_ARG;
    egs_prologue_acc(pa, (float*)side->scratch, (size_t)side->P,
                     side->geom_buffer ? geom_ptrs(const_cast<void*>(side->geom_buffer), side->P).block_hot : nullptr);
    if (side->sink) {
        if (!side->sink->coef) return EGS_ERR_ARG;
        EgsSink ks = {};
        sink_to_kernel_args(side->sink, side->skip_flag, ks, pa.tick);
        pa.has_tick = 1;
    }
    return 0;
}

int egs_l1_ssim_backward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                            const float* upstream_grad, const float* gate, const float* dm_dmu1, const float* dm_dexx,
                            const float* dm_dexy, float* dL_dimg, const float* deferred_partial_sums, float* deferred_loss,
                            float* loss_running_sum, const egs_backward_prologue* side, void* stream) {
    if (!side)
        return egs_launch_l1_ssim_backward(channels, height, width, img, gt, lambda_dssim, upstream_grad, gate, dm_dmu1, dm_dexx, dm_dexy, dL_dimg,
                                           deferred_partial_sums, deferred_loss, loss_running_sum, nullptr, (hipStream_t)stream);
    EgsPrologueArgs pa = {};
    int rc = prologue_args(side, pa); if (rc) return rc;
    return egs_launch_l1_ssim_backward(channels, height, width, img, gt, lambda_dssim, upstream_grad, gate, dm_dmu1, dm_dexx, dm_dexy, dL_dimg,
                                       deferred_partial_sums, deferred_loss, loss_running_sum, &pa, (hipStream_t)stream);
}

int egs_l1_ssim_forward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                           float* partial_sums, float* dm_dmu1, float* dm_dexx, float* dm_dexy, float* loss, float* loss_running_sum,
                           const egs_backward_prologue* side, void* stream) {
    EgsPrologueArgs pa = {};
    if (side) { int rc = prologue_args(side, pa); if (rc) return rc; }
    return egs_launch_l1_ssim_forward(channels, height, width, img, gt, lambda_dssim, partial_sums, dm_dmu1, dm_dexx, dm_dexy, loss, loss_running_sum,
                                      side ? &pa : nullptr, (hipStream_t)stream);
}

int egs_object_loss_forward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                               float* partial_sums, float* dm_dmu1, float* dm_dexx, float* dm_dexy, float* loss, float* loss_running_sum,
                               const egs_object_loss* obj, const egs_backward_prologue* side, void* stream) {
    EgsObjLossK ok; int rc = obj_loss_args(obj, channels, height, width, lambda_dssim, ok); if (rc) return rc;
    if (!obj->alpha_partial_sums) return EGS_ERR_ARG;
    EgsPrologueArgs pa = {};
    if (side) { rc = prologue_args(side, pa); if (rc) return rc; }
    return egs_launch_l1_ssim_forward(channels, height, width, img, gt, lambda_dssim, partial_sums, dm_dmu1, dm_dexx, dm_dexy, loss, loss_running_sum,
                                      side ? &pa : nullptr, (hipStream_t)stream, &ok);
}

int egs_object_loss_forward(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                            float* partial_sums, float* dm_dmu1, float* dm_dexx, float* dm_dexy, float* loss, float* loss_running_sum,
                            const egs_object_loss* obj, void* stream) {
    return egs_object_loss_forward_ex(channels, height, width, img, gt, lambda_dssim, partial_sums, dm_dmu1, dm_dexx, dm_dexy, loss, loss_running_sum, obj,
                                      nullptr, stream);
}

int egs_object_loss_backward_ex(int channels, int height, int width, const float* img, const float* gt, float lambda_dssim,
                                const float* upstream_grad, const float* gate, const float* dm_dmu1, const float* dm_dexx,
                                const float* dm_dexy, float* dL_dimg, float* dL_dalpha, const float* deferred_partial_sums, float* deferred_loss,
                                float* loss_running_sum, const egs_object_loss* obj, const egs_backward_prologue* side, void* stream) {
    EgsObjLossK ok; int rc = obj_loss_args(obj, channels, height, width, lambda_dssim, ok); if (rc) return rc;
    if (!dL_dalpha || (deferred_partial_sums && !obj->alpha_partial_sums)) return EGS_ERR_ARG;
    EgsPrologueArgs pa = {};
    if (side) { rc = prologue_args(side, pa); if (rc) return rc; }
    // the image weights carry lambda_image; the value's own weights travel in `ok`
    return egs_launch_l1_ssim_backward_w(channels, height, width, img, gt, obj->lambda_image * (1.f - lambda_dssim), obj->lambda_image * lambda_dssim, lambda_dssim,
                                         upstream_grad, nullptr, gate, dm_dmu1, dm_dexx, dm_dexy, dL_dimg, deferred_partial_sums, deferred_loss,
                                         loss_running_sum, side ? &pa : nullptr, (hipStream_t)stream, &ok, dL_dalpha);
}

int egs_backward_object_lossgrad(int P, int sh_degree, int sh_coeffs, int64_t R, const float* background, const float* means3D,
                          const float* shs, const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, int activation_flags, const float* viewmatrix, const float* projmatrix,
                          const float* campos, int width, int height, float tan_fovx, float tan_fovy, const int32_t* radii,
                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const egs_loss_grad* loss_grad,
                          const egs_object_loss* obj,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                          float* dL_dscales, float* dL_drotations, float* stat_grad_accum, float* stat_denom, float* stat_max_radii,
                          const uint32_t* skip_flag, const egs_adam_sink* sink, int prologue_done, const egs_object_rotation* rot, int grad_mask, void* scratch,
                          void* stream, int debug) {
    if (!loss_grad || !obj) return EGS_ERR_ARG;
    return backward_impl({ BWD_SCENE, nullptr, nullptr, nullptr, BWD_OUTPUTS, BWD_SINK_TAIL, loss_grad, obj, nullptr });
}
#undef BWD_SINK_TAIL
#undef BWD_OUTPUTS
#undef BWD_SCENE

// ---- the label phase (include/egs_raster.h; label_loss.hip, render_bwd.hip k_render_backward<3>) ----
size_t egs_label_bce_partial_count(int height, int width) {
    if (height <= 0 || width <= 0) return 0;
    return (size_t)4 * egs_tiles(width, height);
}
int egs_label_bce_forward(int height, int width, const float* img, const float* obj_mask, float* partial_sums, float* loss, float* loss_running_sum,
                          void* stream) {
    int rc = check_dims(0, width, height); if (rc) return rc;
    if (!img || !obj_mask || !partial_sums) return EGS_ERR_ARG;
    EGS_TRY(egs_launch_label_bce_forward(height, width, img, obj_mask, partial_sums, loss, loss_running_sum, loss != nullptr, (hipStream_t)stream));
    return 0;
}
int egs_label_bce_backward(int height, int width, const float* img, const float* obj_mask, const float* gate, const float* upstream_grad, float* dL_dimg,
                           const float* deferred_partial_sums, float* deferred_loss, float* loss_running_sum, void* stream) {
    int rc = check_dims(0, width, height); if (rc) return rc;
    if (!img || !obj_mask || !upstream_grad || !dL_dimg) return EGS_ERR_ARG;
    EGS_TRY(egs_launch_label_bce_backward(height, width, img, obj_mask, gate, upstream_grad, dL_dimg, deferred_partial_sums, deferred_loss,
                                          deferred_partial_sums ? loss_running_sum : nullptr, (hipStream_t)stream));
    return 0;
}
int egs_backward_label(int P, int64_t R, int width, int height, const int32_t* radii, const void* geom_buffer, const void* binning_buffer,
                       const void* image_buffer, const float* dL_dout_color, const egs_label_loss* loss, float* dL_dlabel, const egs_adam_leaf* adam,
                       float beta1, float beta2, float eps, float* coef, const int32_t* active_rows, const uint32_t* skip_flag, void* scratch,
                       void* stream, int flags) {
    const int debug = flags;
    int rc = check_dims(P, width, height); if (rc) return rc;
    if ((dL_dout_color != nullptr) == (loss != nullptr)) return EGS_ERR_MODE;
    if (R < 0 || R >= (1ll << 31)) return EGS_ERR_RANGE;
    const size_t n_partial = egs_label_bce_partial_count(height, width);
    if (loss && (!loss->img || !loss->mask || !loss->upstream || !loss->partial || loss->n_partial < n_partial)) return EGS_ERR_ARG;
    if (adam && (!adam->param || !adam->exp_avg || !adam->exp_avg_sq || !adam->lr || !adam->step || !coef)) return EGS_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float inv_hw = 1.f / ((float)height * (float)width);
    EgsAdamTick tick = {}; EgsLabelAdam la = {};
    if (adam) {
        tick.step[0] = adam->step; tick.lr[0] = adam->lr; tick.coef = coef; tick.skip = skip_flag; tick.b1 = beta1; tick.b2 = beta2;
        la = EgsLabelAdam{ adam->param, adam->exp_avg, adam->exp_avg_sq, coef, active_rows, skip_flag, beta1, beta2, eps };
    }
    if (P == 0) {                                                     // nothing to blend: the value of the background image, no step
        if (loss) EGS_TRY(egs_launch_label_bce_forward(height, width, loss->img, loss->mask, loss->partial, loss->loss, loss->running,
                                                       (loss->loss || loss->running) ? 1 : 0, s));
        return 0;
    }
    if (!radii || !geom_buffer || !image_buffer || !scratch || (R > 0 && !binning_buffer)) return EGS_ERR_ARG;
    if (misaligned(geom_buffer, binning_buffer, image_buffer) || ((uintptr_t)scratch & 63u)) return EGS_ERR_ARG;
    EgsGeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    EgsImgPtrs im = img_ptrs(const_cast<void*>(image_buffer), width, height);
    float* grad_acc = (float*)scratch;
    if (R == 0) {                                                     // no instance: every gradient is 0 (radii <= 0 everywhere); the step is still taken
        EGS_TRY(egs_launch_zero_f4((float4*)grad_acc, egs_acc_floats((size_t)P) / 4, s));
        if (adam) EGS_TRY(egs_launch_adam_tick(tick, s));
        if (loss) EGS_TRY(egs_launch_label_bce_forward(height, width, loss->img, loss->mask, loss->partial, nullptr, nullptr, 0, s));
    } else {
        EgsBinPtrs b = bin_ptrs(const_cast<void*>(binning_buffer), P, R, width, height);
        EGS_TRY(egs_launch_backward_prologue(P, width, height, im, grad_acc, g.block_hot, adam ? &tick : nullptr, s));
        void* det = nullptr; rc = det_lines_clear(scratch, P, debug, s, &det); if (rc) return rc;
        EgsLabelLossK lk = {}; EgsLossGradHost lgh = {};
        if (loss) { lk = EgsLabelLossK{ loss->img, loss->mask, loss->gate, loss->upstream, loss->partial, inv_hw }; lgh.lab = &lk; }
        egs_prof_start(EGS_K_RENDER_BWD, s);
        EGS_TRY(egs_launch_render_backward(P, width, height, nullptr, g, b.point_list, im, dL_dout_color, nullptr, nullptr, grad_acc, 2, loss ? &lgh : nullptr, s, det));
        egs_prof_stop(EGS_K_RENDER_BWD, s);
        EGS_SYNC_IF_DEBUG(s);
    }
    egs_prof_start(EGS_K_PREPROCESS_BWD, s);
    EGS_TRY(egs_launch_label_finish(P, grad_acc, g.clamped, radii, dL_dlabel, adam ? &la : nullptr, skip_flag, loss ? loss->partial : nullptr, n_partial, inv_hw,
                                    loss ? loss->loss : nullptr, loss ? loss->running : nullptr, s));
    egs_prof_stop(EGS_K_PREPROCESS_BWD, s);
    EGS_SYNC_IF_DEBUG(s);
    return 0;
}

int egs_l1_ssim_pair_backward(int channels, int height, int width, const float* img, const float* gt, const float* upstream_l1,
                              const float* upstream_ssim, const float* gate, const float* dm_dmu1, const float* dm_dexx, const float* dm_dexy,
                              float* dL_dimg, const egs_backward_prologue* side, void* stream) {
    if (!upstream_l1 || !upstream_ssim) return EGS_ERR_ARG;
    EgsPrologueArgs pa = {};
    if (side) { int rc = prologue_args(side, pa); if (rc) return rc; }
    // d(mean SSIM) = -d(1 - mean SSIM): weight -1 on the kernel's (1 - SSIM) term, each term times its own upstream scalar (read on the device)
    return egs_launch_l1_ssim_backward_w(channels, height, width, img, gt, 1.f, -1.f, 0.f, upstream_l1, upstream_ssim, gate, dm_dmu1, dm_dexx, dm_dexy, dL_dimg,
                                         nullptr, nullptr, nullptr, side ? &pa : nullptr, (hipStream_t)stream);
}

int egs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream) {
    (void)projmatrix;
    if (P < 0) return EGS_ERR_ARG;
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !present) return EGS_ERR_ARG;
    EGS_TRY(egs_launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
