"""ctypes binding of libegs_raster.so (C ABI: include/egs_raster.h).

There is no fallback: if the shared library is missing or cannot be loaded this module raises, and so
does every op built on it.  Build it with `python __graft_entry__.py` or `make -C egogaussian_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EGS_RASTER_LIB", os.path.join(_HERE, "libegs_raster.so"))      # override for A/B builds
ABI_VERSION = 6
RETRY_LARGER = -100
# per-call flags (include/egs_raster.h EGS_CALL_*, ABI 6): bits of the `debug` / `flags` word of the forwards
CALL_SYNC, CALL_KEEP_ALL_INSTANCES, CALL_SEPARATE_COUNT, CALL_SEPARATE_SORT, CALL_BALLOT_RANK = 1, 2, 4, 8, 16
CALL_DETERMINISTIC = 0x20      # backwards only: order-independent gradient sums (scratch of egs_backward_scratch_bytes_ex)
# egs_forward_sort_plan's answer (EGS_SORT_*)
SORT_IN_BLEND, SORT_SECOND_INSTANTIATION, SORT_BALLOT_RANK = 1, 2, 4

vp, f32, i32, i64 = C.c_void_p, C.c_float, C.c_int, C.c_int64


class GeomLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("rec", "rect", "offsets", "clamped", "visible", "scan_scratch", "total")]


class BinningLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("point_list", "pairs", "scratch", "table", "spine", "total")] + \
               [(n, C.c_int) for n in ("bin_blocks", "key_bits", "index_passes", "table_stride")]


class BinGeometry(C.Structure):
    """egs_bin_geometry_info: the launch geometry of a forward's tile bucketing (egs_forward_bin_geometry)"""
    _fields_ = [(n, C.c_int32) for n in ("n_tiles", "gx", "nblocks", "stride", "n_chunks", "gpr", "cull", "use_map", "groups_per_block", "rounds",
                                         "prefixed", "can_fuse")] + [("lds", C.c_int64)]


class ImageLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("ranges", "final_T", "n_contrib", "quad_work", "tile_order", "quad_pairs")]


class AdamLeaf(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("param", "exp_avg", "exp_avg_sq", "lr", "step")]


class AdamSink(C.Structure):                     # egs_adam_sink
    _fields_ = [("leaf", AdamLeaf * 6), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("coef", C.c_void_p),
                ("active_rows", C.c_void_p)]


class ObjectRotation(C.Structure):               # egs_object_rotation
    _fields_ = [("M9", C.c_void_p), ("selected", C.c_void_p), ("row0_grad_mult", C.c_float), ("row0_grad_mult_dev", C.c_void_p)]


class ObjectMotion(C.Structure):                 # egs_object_motion; goes where an egs_object_rotation* goes when ACT_OBJECT_MOTION is set
    _fields_ = [("rot", ObjectRotation), ("A12", C.c_void_p), ("moved", C.c_void_p), ("grad", C.c_void_p), ("scratch", C.c_void_p)]


class DensifyRuleBlock(C.Structure):              # egs_densify_rules_dev: twelve words of device memory
    _fields_ = [(n, C.c_float) for n in ("max_grad", "min_opacity", "dense_extent", "big_extent", "max_screen_size")] + \
               [(n, C.c_int32) for n in ("clone", "split", "has_curr_gen", "curr_gen", "prune_prev_gen", "has_which_object", "which_object")]


class DensifyArray(C.Structure):                 # egs_densify_array
    _fields_ = [("data", C.c_void_p), ("row_floats", C.c_int32), ("role", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


DENSIFY_MAX_ARRAYS = 32
DENSIFY_PARAM, DENSIFY_MOMENT, DENSIFY_STAT, DENSIFY_TAG = 0, 1, 2, 3      # EGS_DENSIFY_* roles
DENSIFY_TAG_I32, DENSIFY_TAG_CLONE_GEN = 1, 2                              # EGS_DENSIFY_TAG_* flags

# include/egs_raster.h EGS_ACT_*: activation flags of the raw-parameter mode (_C re-exports them)
ACT_LOG_SCALES, ACT_RAW_QUATS, ACT_LOGIT_OPACITY, ACT_OBJECT_MOTION, ACT_SCALAR_COLOR = 1, 2, 4, 8, 16
ACT_RAW_PARAMETERS = ACT_LOG_SCALES | ACT_RAW_QUATS | ACT_LOGIT_OPACITY
# include/egs_raster.h EGS_GRAD_*: which inputs' gradients the caller of a backward reads (0 = all)
GRAD_MEANS3D, GRAD_MEANS2D, GRAD_SH, GRAD_COLORS, GRAD_OPACITY, GRAD_SCALES, GRAD_ROTATIONS, GRAD_COV3D = 1, 2, 4, 8, 16, 32, 64, 128


def rot_pointer(st):
    """The `rot` argument for an ObjectRotation or an ObjectMotion struct (None -> NULL)."""
    if st is None:
        return None
    return C.byref(st.rot if isinstance(st, ObjectMotion) else st)         # (`rot` is the motion struct's first member: the same address)


class BackwardPrologue(C.Structure):             # egs_backward_prologue
    _fields_ = [("P", C.c_int), ("width", C.c_int), ("height", C.c_int), ("image_buffer", C.c_void_p), ("scratch", C.c_void_p),
                ("sink", C.POINTER(AdamSink)), ("skip_flag", C.c_void_p), ("geom_buffer", C.c_void_p)]


class LossGrad(C.Structure):                     # egs_loss_grad
    _fields_ = [("image", C.c_void_p), ("gt", C.c_void_p), ("dm_dmu1", C.c_void_p), ("dm_dexx", C.c_void_p), ("dm_dexy", C.c_void_p),
                ("gate", C.c_void_p), ("upstream_grad", C.c_void_p), ("lambda_dssim", C.c_float), ("deferred_partial_sums", C.c_void_p),
                ("deferred_loss", C.c_void_p), ("loss_running_sum", C.c_void_p)]


class ObjectLoss(C.Structure):                   # egs_object_loss
    _fields_ = [("alpha", C.c_void_p), ("obj_mask", C.c_void_p), ("lambda_image", C.c_float), ("lambda_l1_alpha", C.c_float),
                ("lambda_l2_alpha", C.c_float), ("alpha_partial_sums", C.c_void_p), ("terms", C.c_void_p)]


class LabelLoss(C.Structure):                    # egs_label_loss
    _fields_ = [("img", C.c_void_p), ("mask", C.c_void_p), ("gate", C.c_void_p), ("upstream", C.c_void_p), ("partial", C.c_void_p),
                ("n_partial", C.c_size_t), ("loss", C.c_void_p), ("running", C.c_void_p)]


class OpacityEntropy(C.Structure):               # egs_opacity_entropy
    _fields_ = [("weight", C.c_void_p), ("upstream", C.c_void_p), ("scratch", C.c_void_p), ("n_vis", C.c_void_p), ("value", C.c_void_p)]


class MaskRow(C.Structure):                      # egs_mask_row
    _fields_ = [(n, C.c_int64) for n in ("predicted", "target", "intersection", "kept", "clipped", "instances")]


class FrameLayout(C.Structure):                  # egs_frame_layout
    _fields_ = [(n, C.c_int64) for n in ("frame_floats", "image_floats", "small_begin", "small_floats", "gate_begin", "obj_mask_begin",
                                         "image_stride", "plane_words", "n_planes")]


class PoseSequence(C.Structure):                 # egs_pose_sequence
    _fields_ = [("K", C.c_int32)] + [(n, C.c_void_p) for n in ("rel", "valid", "accum", "pose", "exp_avg", "exp_avg_sq", "step", "lr")] + \
               [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class LpipsWeights(C.Structure):               # egs_lpips_weights
    _fields_ = [("conv_w", C.c_void_p * 13), ("conv_b", C.c_void_p * 13), ("lin", C.c_void_p * 5)]


FRAME_DYNAMIC, FRAME_MOTION, FRAME_GATED, FRAME_OBJECT_LOSS, FRAME_LABEL_PHASE = 1, 2, 4, 8, 16      # EGS_FRAME_*
FRAME_POSE_ROWS = 32                             # EGS_FRAME_POSE_ROWS
INGEST_IMAGE, INGEST_HAND_MASK, INGEST_OBJ_MASK = 0, 1, 2      # EGS_INGEST_*
SINK_MEANS3D, SINK_OPACITY, SINK_SCALES, SINK_ROTATIONS, SINK_SH, SINK_SH_REST = range(6)      # EGS_SINK_*

# ---- the long rasterizer entry points: their parameter lists are runs of the same few segments (include/egs_raster.h) ----------------
_ROT = C.POINTER(ObjectRotation)
# scene prefix of the forwards: P, sh_degree, sh_coeffs, means3D, shs, shs_rest, colors_precomp, opacities, scales, scale_modifier, rotations,
# cov3D_precomp, activation_flags, viewmatrix, projmatrix, campos
_FWD_SCENE = [i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, vp, vp, vp]
_FWD_VIEW = [i32, i32, f32, f32, i32]                            # width, height, tan_fovx, tan_fovy, prefiltered
# background + view, then radii, geom_buffer, capacity, binning_buffer, image_buffer, out_color, out_depth, out_alpha, pinned_host_counts
_FWD_RENDER = [vp] + _FWD_VIEW + [vp, vp, i64, vp, vp, vp, vp, vp, vp]
_FWD_TAIL = [_ROT, vp, i32]                                      # rot, stream, flags
# scene prefix of the backwards: P, sh_degree, sh_coeffs, R, background, means3D, shs, shs_rest, colors_precomp, scales, scale_modifier, rotations,
# cov3D_precomp, activation_flags, viewmatrix, projmatrix, campos, width, height, tan_fovx, tan_fovy, radii
_BWD_SCENE = [i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, vp, vp, vp, i32, i32, f32, f32, vp]
_STATE = [vp, vp, vp]                                            # geom_buffer, binning_buffer, image_buffer
_UPSTREAM = [vp, vp, vp]                                         # dL_dout_color, dL_dout_depth, dL_dout_alpha
_GRADS = [vp] * 9                                                # dL_d{means2D, colors, opacity, means3D, cov3D, sh, sh_rest, scales, rotations}
_STATS = [vp, vp, vp, vp]                                        # stat_grad_accum, stat_denom, stat_max_radii, skip_flag
_BWD_TAIL = [C.POINTER(AdamSink), i32, _ROT, i32, vp, vp, i32]   # sink, prologue_done, rot, grad_mask, scratch, stream, flags


def _backward(middle, tail=_BWD_TAIL):
    """A backward differs from the others in its middle segment only (egs_backward, the oldest, also lacks sink, prologue_done and rot)."""
    return (C.c_int, _BWD_SCENE + _STATE + middle + _GRADS + _STATS + tail)


# name -> (restype, argtypes); every symbol include/egs_raster.h declares
SIGNATURES = {
    "egs_abi_version": (C.c_int, []),
    "egs_source_hash": (C.c_char_p, []),
    "egs_error_string": (C.c_char_p, [C.c_int]),
    "egs_device_info": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "egs_geom_bytes": (C.c_size_t, [i32]),
    "egs_binning_bytes": (C.c_size_t, [i32, i64, i32, i32]),
    "egs_image_bytes": (C.c_size_t, [i32, i32]),
    "egs_backward_scratch_bytes": (C.c_size_t, [i32]),
    "egs_backward_scratch_bytes_ex": (C.c_size_t, [i32, i32]),
    "egs_order_words": (C.c_int, [i32, i32]),
    "egs_get_geom_layout": (C.c_int, [i32, C.POINTER(GeomLayout)]),
    "egs_get_binning_layout": (C.c_int, [i32, i64, i32, i32, C.POINTER(BinningLayout)]),
    "egs_get_image_layout": (C.c_int, [i32, i32, C.POINTER(ImageLayout)]),
    "egs_forward_geometry": (C.c_int, _FWD_SCENE + _FWD_VIEW + [vp, vp, C.POINTER(i64), vp] + _FWD_TAIL),     # radii, geom_buffer, num_rendered, active_count
    "egs_forward": (C.c_int, _FWD_SCENE + _FWD_RENDER + [C.POINTER(i64), vp, vp] + _FWD_TAIL),                 # num_rendered, active_count, placement
    "egs_forward_enqueue": (C.c_int, _FWD_SCENE + _FWD_RENDER + [vp, vp, vp, vp] + _FWD_TAIL),                 # running_max, active_count, overflow_flag, placement
    "egs_placement_bytes": (C.c_size_t, [i32, i32]),
    "egs_placement_init": (C.c_int, [vp, i32, i32, vp]),
    "egs_sum_counts": (C.c_int64, [i32, vp]),
    "egs_forward_render": (C.c_int, [i32, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32]),
    "egs_backward": _backward(_UPSTREAM, _BWD_TAIL[3:]),
    "egs_backward_adam": _backward(_UPSTREAM),
    "egs_mark_visible": (C.c_int, [i32, vp, vp, vp, vp, vp]),
    "egs_cov3d_forward": (C.c_int, [i32, vp, i32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "egs_cov3d_dm_scratch_floats": (C.c_size_t, [i32]),
    "egs_cov3d_backward": (C.c_int, [i32, vp, i32, f32, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "egs_object_motion_scratch_bytes": (C.c_size_t, [i32]),
    "egs_object_move_points": (C.c_int, [i32, vp, vp, vp, vp, vp, vp]),
    "egs_object_move_points_backward": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "egs_l1_ssim_partial_count": (C.c_size_t, [i32, i32, i32]),
    "egs_l1_ssim_forward": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp]),
    "egs_l1_ssim_backward": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "egs_l1_ssim_pair_forward": (C.c_int, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "egs_eval_metrics_partial_bytes": (C.c_size_t, [i32, i32, i32]),
    "egs_eval_metrics": (C.c_int, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
    "egs_lpips_workspace_bytes": (C.c_size_t, [i32, i32]),
    "egs_lpips_tap_offsets": (C.c_int, [i32, i32, C.POINTER(i64)]),
    "egs_lpips_forward": (C.c_int, [i32, i32, vp, vp, vp, C.POINTER(LpipsWeights), vp, vp, i32, vp, vp]),
    "egs_conv3x3_relu_nhwc": (C.c_int, [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "egs_label_mask_partial_bytes": (C.c_size_t, [i32, i32]),
    "egs_label_mask": (C.c_int, [i32, i32, vp, f32, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
    "egs_interaction_gate": (C.c_int, [i32, i32, vp, vp, i32, vp, vp]),
    "egs_frame_store_layout": (C.c_int, [i32, i32, i32, C.POINTER(FrameLayout)]),
    "egs_frame_decode": (C.c_int, [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "egs_resample_ksize": (C.c_int, [i32, i32]),
    "egs_resample_tables": (C.c_int, [i32, i32, vp, vp]),
    "egs_frame_ingest": (C.c_int, [i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "egs_png_bound": (C.c_size_t, [i32, i32, i32]),
    "egs_png_scratch_bytes": (C.c_size_t, [i32, i32, i32, i32]),
    "egs_png_encode": (C.c_int, [i32, i32, i32, i32, vp, i64, i64, vp, i64, vp, vp, vp]),
    "egs_png_decode_scratch_bytes": (C.c_size_t, [i32, C.c_size_t, C.c_size_t]),
    "egs_png_decode": (C.c_int, [i32, vp, C.c_size_t, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, C.c_size_t, vp]),
    "egs_png_decode_phases": (C.c_int, [i32, vp, C.c_size_t, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, C.c_size_t, vp, i32]),
    "egs_png_decode_scratch_bytes_ex": (C.c_size_t, [i32, C.c_size_t, C.c_size_t, i32]),
    "egs_png_decode_ex": (C.c_int, [i32, vp, C.c_size_t, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, C.c_size_t, vp, i32, i32, vp]),
    "egs_jpeg_decode_scratch_bytes": (C.c_size_t, [i32, i32, C.c_size_t, C.c_size_t]),
    "egs_jpeg_decode": (C.c_int, [i32, vp, C.c_size_t, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, C.c_size_t, vp]),
    "egs_jpeg_decode_phases": (C.c_int, [i32, vp, C.c_size_t, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, C.c_size_t, vp, i32]),
    "egs_pose_head": (C.c_int, [C.POINTER(PoseSequence), vp, vp, vp, vp]),
    "egs_pose_tail": (C.c_int, [C.POINTER(PoseSequence), vp, vp, vp, vp, vp]),
    "egs_pose_accumulate": (C.c_int, [C.POINTER(PoseSequence), vp]),
    "egs_pose_interpolate": (C.c_int, [C.POINTER(PoseSequence), C.POINTER(PoseSequence), vp, i32, i32, f32, vp, vp, vp]),

    "egs_l1_ssim_pair_backward": (C.c_int, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(BackwardPrologue), vp]),
    "egs_l1_ssim_backward_ex": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(BackwardPrologue), vp]),
    "egs_l1_ssim_forward_ex": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, C.POINTER(BackwardPrologue), vp]),
    "egs_backward_lossgrad": _backward([C.POINTER(LossGrad)]),
    "egs_object_loss_forward": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, C.POINTER(ObjectLoss), vp]),
    "egs_object_loss_forward_ex": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, C.POINTER(ObjectLoss), C.POINTER(BackwardPrologue), vp]),
    "egs_object_loss_backward_ex": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(ObjectLoss),
                                              C.POINTER(BackwardPrologue), vp]),
    "egs_backward_object_lossgrad": _backward([C.POINTER(LossGrad), C.POINTER(ObjectLoss)]),
    "egs_label_bce_partial_count": (C.c_size_t, [i32, i32]),
    "egs_label_bce_forward": (C.c_int, [i32, i32, vp, vp, vp, vp, vp, vp]),
    "egs_label_bce_backward": (C.c_int, [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "egs_backward_label": (C.c_int, [i32, i64, i32, i32, vp, vp, vp, vp, vp, C.POINTER(LabelLoss), vp, C.POINTER(AdamLeaf), f32, f32, f32, vp, vp, vp,
                                     vp, vp, i32]),
    "egs_opacity_entropy_scratch_bytes": (C.c_size_t, [i32]),
    "egs_opacity_entropy_forward": (C.c_int, [i32, vp, i32, vp, vp, vp, C.POINTER(OpacityEntropy), vp]),
    "egs_opacity_entropy_backward": (C.c_int, [i32, vp, i32, vp, vp, C.POINTER(OpacityEntropy), vp, vp]),
    "egs_backward_entropy_lossgrad": _backward([C.POINTER(LossGrad), C.POINTER(OpacityEntropy)] + _UPSTREAM),
    "egs_adam_step": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, vp]),
    "egs_adam_workgroups": (C.c_int64, [i64]),
    "egs_adam_step_capturable": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, vp, vp, vp, vp]),
    "egs_densify_stats": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp]),
    "egs_densify_plan_scratch_bytes": (C.c_size_t, [i32]),
    "egs_densify_plan": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp,
                                    vp, vp, vp]),
    "egs_prune_plan": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp]),
    "egs_gather_rows_f32": (C.c_int, [i64, i32, vp, vp, i32, vp, vp, vp]),
    "egs_gather_i32": (C.c_int, [i64, vp, vp, i32, i32, vp, vp, vp]),
    "egs_split_children": (C.c_int, [i64, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "egs_densify_plan_dev": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "egs_prune_plan_dev": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "egs_densify_apply_scratch_bytes": (C.c_size_t, [i32, i32, vp]),
    "egs_densify_apply": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(DensifyArray), i32, i32, i32, vp, vp, vp, vp]),
    "egs_knn3_mean_dist2": (C.c_int, [i32, vp, vp, vp]),
    "egs_knn3_grid_scratch_bytes": (C.c_size_t, [i32]),
    "egs_knn3_grid": (C.c_int, [i32, vp, vp, vp, vp]),
    "egs_forward_fuses_count": (C.c_int, [i32, i32, i32, i32]),
    "egs_forward_sort_plan": (C.c_int, [i32, i64, i32, i32, i32]),
    "egs_forward_bin_geometry": (C.c_int, [i32, i32, i32, i32, vp]),
    "egs_profile_begin": (C.c_int, [i32]),
    "egs_profile_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "egs_profile_stage_name": (C.c_char_p, [i32]),
}
N_STAGES = 8


def profile_begin(max_records=65536):
    check(load().egs_profile_begin(max_records))


def profile_end():
    """-> {stage: (total_ms, launches)}"""
    ms = (C.c_double * N_STAGES)()
    n = (C.c_int * N_STAGES)()
    L = load()
    check(L.egs_profile_end(ms, n))
    return {L.egs_profile_stage_name(k).decode(): (float(ms[k]), int(n[k])) for k in range(N_STAGES)}

_lib = None


def kernel_source_hash():
    """sha256 (first 16 hex digits) over the library's sources -- csrc/*.hip, csrc/*.h, include/egs_raster.h, the Makefile -- in
    name order.  Counter files under profiles/ carry the hash they were collected at; bench.py reports their numbers only
    while it still equals this one (a profile of other kernels describes other kernels).  The library embeds the same hash at build
    time: built_source_hash()."""
    from .srchash import source_hash
    return source_hash()


def built_source_hash():
    """The source hash `make` embedded into the loaded library (egs_source_hash()): equal to kernel_source_hash() unless the build is stale."""
    return load().egs_source_hash().decode()


def library_path():
    """Path of the shared library this process loads (EGS_RASTER_LIB overrides the in-tree build)."""
    return LIB_PATH


def load():
    """Load (once) and return the ctypes handle.  Raises RuntimeError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the MI355X rasterizer has no CPU or PyTorch fallback. "
            "Build it first (python -c 'import __graft_entry__ as g; g.build()' or make -C egogaussian_amd/csrc).")
    # PyTorch-ROCm bundles its own libamdhip64.so while this library links the system one (libamdhip64.so.7): two copies of the HIP
    # runtime live in the process.  That works as long as TORCH's copy is the one that opened the device first; the other way round --
    # this library loaded (its kernels registered) before torch's first HIP call -- every launch of ours then fails with
    # hipErrorNoDevice (found by running build() and smoke() in one process).  So: bring torch's runtime up first when a device exists.
    # ... and, since this creates the HIP context, first export what a later multi-process RCCL group needs from the environment while
    # it can still be set (dist.REQUIRED_ENV; dmabuf-only hosts fail with hipIpcGetMemHandle otherwise) -- only if the caller left it unset.
    for k, v in (("HSA_ENABLE_IPC_MODE_LEGACY", "0"),):
        os.environ.setdefault(k, v)
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:                  # (a C-ABI user without torch: nothing to order)
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    if lib.egs_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libegs_raster.so ABI {lib.egs_abi_version()} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise RuntimeError(f"libegs_raster: {load().egs_error_string(code).decode()} (code {code})")
