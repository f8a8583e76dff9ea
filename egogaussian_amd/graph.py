"""Whole-training-step hipGraph capture (PyTorch's torch.cuda.graph on ROCm = hipGraph).

Once the kernels are fast the iteration of /root/reference/trainers/train_static.py:67-138 is bound by the host: ~60
kernel launches, three Python autograd Functions and the optimizer cost ~0.75 ms of CPU per step against ~0.55 ms of GPU
work at 500k Gaussians.  The step has static shapes (the data-dependent instance count is handled by the capacity-bounded
`egs_forward_enqueue`, the optimizer by `FusedAdam(capturable=True)`), so it is captured ONCE -- covariance, render
forward, loss, backward, Adam -- and replayed with one launch per iteration; per-iteration inputs (camera matrices,
ground-truth image and, for the `fine_all` call shape, the object's accumulated rotation and the hand-mask gate) are
copied into static device tensors first, as ONE copy when the caller keeps them packed (`pack_frame`).

Overflow safety.  A replayed frame whose instance count exceeds the captured capacity is clipped, hence wrong.  The
forward chain writes an overflow word on the device (`_C.StepGuard`); the backward's fused densification statistics and
the Adam launch read it and do NOTHING for such a frame -- parameters, moments, step counts and statistics stay bit for
bit what they were, so every optimizer step follows a complete render, as in the reference (train_static.py:110-138).
The frame is merely lost.  `ok()` (one host read of the running maximum) tells whether that ever happened; with
`check_every=K` the object looks itself every K calls and re-captures with a larger capacity.

What is baked into the captured launches and therefore needs `recapture()` when it changes: the tensors themselves
(densification and pruning of a plain model replace them; a capacity.CapacityGaussians model keeps them, and its live row
count is a device word the kernels read), the image size, `pc.active_sh_degree` (the reference raises it every 1000
iterations, scene/gaussian_model.py:176-178), the background tensor's address, `lambda_dssim`.  What does not: camera,
ground truth, accum_R / accum_T, gate and object-mask contents (copied in per call), the VALUES of a trainable pose's two parameters
(pose=: they are tensors of the captured step like the model's), the weight of the entropy term (entropy_reg=: a device scalar pushed
like a learning rate) and the learning rates (device scalars; `__call__` pushes
host-side edits of `param_groups[i]["lr"]` -- the reference's per-iteration `update_learning_rate` -- before each replay).
"""
import gc

import torch

from . import _C
from .fused import l1_ssim_loss, object_stage_loss
from .renderer import label_forward, render
from .scene_synth import Pipe


def pack_camera(cam):
    """The three camera tensors render() reads, as one float32[35] block: world_view_transform, full_proj_transform, camera_center."""
    return torch.cat([cam.world_view_transform.reshape(-1), cam.full_proj_transform.reshape(-1), cam.camera_center.reshape(-1)]).float()


def frame_layout(n_img, n_pix, dynamic=False, gated=False, motion=False, object_loss=False, label_phase=False, pose_rows=False):
    """Float offsets of the segments of a packed frame (each starts on a 16-byte boundary): -> ({name: (begin, end)}, size).
    object_loss: an `obj_mask` segment of n_pix floats follows everything else (the other segments keep their offsets).
    label_phase: the frame of a label step -- no image segment (n_img is not read): camera[, gate], obj_mask.
    pose_rows: a 4-word segment `pose_rows` follows accum_T -- the frame word (fixed_row, train_row, reload, 0) of a poses.PoseSequence,
    int32 carried in the float buffer.  Without it every layout is what it was."""
    up4 = lambda x: (x + 3) & ~3
    off, end = {}, 0
    if not label_phase:                                             # (the label frame has no "gt" key at all: FrameStore tests `name in off`)
        off["gt"] = (0, n_img); end = up4(n_img)
    off["cam"] = (end, end + 35); end = up4(end + 35)
    if dynamic:
        off["accum_R"] = (end, end + 9); end = up4(end + 9)
    if motion:
        off["accum_T"] = (end, end + 12); end = up4(end + 12)      # the object's accumulated pose as A12 = [A | b], row-major 3x4
    if pose_rows:
        off["pose_rows"] = (end, end + 4); end = up4(end + 4)
    if gated:
        off["gate"] = (end, end + n_pix); end = up4(end + n_pix)
    if object_loss or label_phase:
        off["obj_mask"] = (end, end + n_pix); end = up4(end + n_pix)
    return off, end


def frame_views(frame, off, H, W):
    """The named views of ONE packed frame (a flat float32 tensor of the layout `off`): dict(gt [3,H,W], cam [35] -- the storage of a
    _StaticCamera --, accum_R [3,3], accum_T [3,4], gate [H,W], obj_mask [H,W]); None where the layout has no such segment."""
    seg = lambda name, *shape: frame[off[name][0]:off[name][1]].view(*shape) if name in off else None
    views = dict(gt=seg("gt", 3, H, W), cam=seg("cam", 35), accum_R=seg("accum_R", 3, 3), accum_T=seg("accum_T", 3, 4),
                 gate=seg("gate", H, W), obj_mask=seg("obj_mask", H, W))
    if "pose_rows" in off:                                          # the frame word of a pose sequence, as the int32[4] it is
        views["pose_rows"] = frame[off["pose_rows"][0]:off["pose_rows"][1]].view(torch.int32)
    return views


def dynamic_kwargs(f, which_object, pose=None, pose_grad=None):
    """render()'s keywords of the `fine_all` call shape from the static views `f` of a frame (frame_views): rot_cov with the frame's accum_R
    and, where the frame carries an accum_T, the object placed by it inside the rasterizer -- with `pose`, a trainable pose on top.
    pose_grad (float32[21] on the device; pose_sequence=): the rasterizer's backward leaves dL/dA12, dL/dM9 of the static buffers there."""
    kw = dict(rot_cov=True, accum_R=f["accum_R"], which_object=which_object, during_training=False)
    if f["accum_T"] is not None:
        from .motion import ComposedMotion, ObjectMotion
        if pose is not None:
            # composed INSIDE the capture from the static buffers and the two parameters: autograd carries dL/dA12, dL/dM9 back to them
            kw["object_motion"] = ObjectMotion(f["accum_T"], pose, f["accum_R"])
        else:
            kw["object_motion"] = ComposedMotion(f["accum_T"], f["accum_R"], grad_out=pose_grad)      # the static buffers themselves: no launch, follows every copy
    return kw


def pose_word(rows):
    """(fixed_row, train_row[, reload]) -> the frame word of a poses.PoseSequence as a host int32[4]; -1 = no such row."""
    rows = [int(r) for r in rows]
    if len(rows) not in (2, 3):
        raise ValueError("pose_rows: (fixed_row, train_row[, reload])")
    return torch.tensor(rows + [0] * (4 - len(rows)), dtype=torch.int32)


def pack_frame(cam, gt, accum_R=None, gate=None, accum_T=None, obj_mask=None, pose_rows=None):
    """One resident tensor per training frame: the ground-truth image, the camera block and -- for a step captured with
    dynamic=True / gated=True -- the object's accumulated rotation (3x3) and the per-pixel gradient gate (1 - hand mask, [H,W]).
    accum_T (a step captured with motion=True): the object's accumulated pose, 4x4 or 3x4 -- its first three rows travel as 12 floats.
    obj_mask (a step captured with object_loss=): the object mask [H,W] or [1,H,W]; the frame then stores gt * obj_mask -- the image the object
    stages compare against -- and the mask.
    The background stage's gate, 1 - dilate_k(hand mask | object mask), can be written into the frame afterwards without a tensor of its own:
    fused.interaction_gate(hand, obj, k, out=frame[off["gate"][0]:off["gate"][1]]) with off from frame_layout(..., gated=True).
    GraphedTrainStep(frame) then refreshes every static input of the captured step with ONE device copy."""
    if pose_rows is not None:
        # (fixed_row, train_row[, reload]): a step captured with pose_sequence= -- its head kernel WRITES the frame's accum_R / accum_T in
        # the static buffer, so what travels in those two segments is not read: the identity unless given
        accum_R = torch.eye(3) if accum_R is None else accum_R
        accum_T = torch.eye(4) if accum_T is None else accum_T
    off, size = frame_layout(gt.numel(), gt.shape[-2] * gt.shape[-1], accum_R is not None, gate is not None, accum_T is not None, obj_mask is not None,
                             pose_rows=pose_rows is not None)
    f = torch.zeros(size, device=gt.device, dtype=torch.float32)
    if pose_rows is not None:
        f[off["pose_rows"][0]:off["pose_rows"][1]].view(torch.int32).copy_(pose_word(pose_rows))
    if obj_mask is not None:
        m = obj_mask.to(gt.device, torch.float32).reshape(gt.shape[-2], gt.shape[-1])
        f[off["obj_mask"][0]:off["obj_mask"][1]] = m.reshape(-1)
        gt = gt * m
    f[off["gt"][0]:off["gt"][1]] = gt.reshape(-1)
    f[off["cam"][0]:off["cam"][1]] = pack_camera(cam).to(gt.device)
    if accum_R is not None:
        f[off["accum_R"][0]:off["accum_R"][1]] = accum_R.reshape(-1).to(gt.device)
    if accum_T is not None:
        f[off["accum_T"][0]:off["accum_T"][1]] = accum_T.reshape(-1, 4)[:3].reshape(-1).to(gt.device)
    if gate is not None:
        f[off["gate"][0]:off["gate"][1]] = gate.reshape(-1).to(gt.device)
    return f


def pack_label_frame(cam, obj_mask, gate=None):
    """One resident tensor per frame of the label phase (GraphedTrainStep(label_phase=True)): the camera block, the gate (1 - hand mask,
    [H,W]; a step captured with gated=True) and the object mask ([H,W] or [1,H,W]).  No image: the label loss reads none."""
    H, W = obj_mask.shape[-2], obj_mask.shape[-1]
    off, size = frame_layout(0, H * W, gated=gate is not None, label_phase=True)
    f = torch.zeros(size, device=obj_mask.device, dtype=torch.float32)
    f[off["cam"][0]:off["cam"][1]] = pack_camera(cam).to(obj_mask.device)
    if gate is not None:
        f[off["gate"][0]:off["gate"][1]] = gate.reshape(-1).to(obj_mask.device)
    f[off["obj_mask"][0]:off["obj_mask"][1]] = obj_mask.to(torch.float32).reshape(-1)
    return f


_gc_was_enabled = []


def begin_capture(graph):
    """graph.capture_begin with the cyclic garbage collector paused until end_capture.  A collection that starts while the capture is open
    may finalise CUDAGraph objects and device allocations of steps dropped earlier, and their HIP calls are not allowed on a capturing
    thread: the process aborts.  torch.cuda.graph avoids that with a gc.collect() before every capture, which costs milliseconds per
    re-capture; pausing the collector for the capture costs nothing, and what it would have freed is freed at the next collection."""
    _gc_was_enabled.append(gc.isenabled())
    gc.disable()
    try:
        # thread_local: calls other threads make meanwhile (e.g. the RCCL watchdog polling its events) must not abort the capture
        graph.capture_begin(capture_error_mode="thread_local")
    except BaseException:
        if _gc_was_enabled.pop():
            gc.enable()
        raise


def end_capture(graph):
    try:
        graph.capture_end()
    finally:
        if _gc_was_enabled.pop():
            gc.enable()


def record_graph(body, side, dev):
    """Records body() -- without executing it -- into a new CUDAGraph on the side stream `side` -> (graph, what body returned).
    capture_begin / capture_end directly (begin_capture): the torch.cuda.graph context manager also runs gc.collect() and
    torch.cuda.empty_cache() (3 ms at 500k Gaussians), which a trainer that re-captures after every densification pays each time."""
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        begin_capture(graph)
        try:
            out = body()
        finally:
            end_capture(graph)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    return graph, out


def warm_up(calls, side, dev):
    """Runs every callable of `calls` eagerly on the side stream `side` (the stream the capture will use) -> the largest instance count
    (`_C.stats["num_rendered"]`) any of them left.  Eager calls set the capacity hint, the allocator pools and the lazy state."""
    r_seen = 0
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for call in calls:
            call()
            r_seen = max(r_seen, _C.stats["num_rendered"])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    return r_seen


def capture_capacity(r_seen, margin, dev, floor=0, capacity=None):
    """The instance capacity to capture with, made the library's hint: `margin` x the largest count the warm-up saw, at least what the
    library holds already and `floor`; `capacity` overrides the rule, as is."""
    cap = max(int(r_seen * margin), _C.stats["capacity"], floor) if capacity is None else max(int(capacity), 1)
    _C.set_capacity_hint(cap, dev)
    return cap


class _StaticCamera:
    """Camera whose tensors are fixed device buffers; `load(cam)` copies another camera of the same intrinsics in."""

    def __init__(self, cam, storage=None):
        """storage: an existing float32[35] device view to live in (part of a packed frame), else its own block."""
        self.image_height, self.image_width, self.FoVx, self.FoVy = cam.image_height, cam.image_width, cam.FoVx, cam.FoVy
        packed = pack_camera(cam)
        if storage is None:
            self.packed = packed
        else:
            self.packed = storage
            self.packed.copy_(packed)
        self.world_view_transform = self.packed[0:16].view(4, 4)
        self.full_proj_transform = self.packed[16:32].view(4, 4)
        self.camera_center = self.packed[32:35]

    def load(self, cam):
        same = (cam.image_height, cam.image_width, cam.FoVx, cam.FoVy) == (self.image_height, self.image_width, self.FoVx, self.FoVy)
        assert same, "a captured step is specific to one image size and field of view"
        packed = getattr(cam, "packed", None)
        if packed is not None and packed.shape == self.packed.shape:   # cameras that keep the three in one block: one copy
            self.packed.copy_(packed, non_blocking=True)
            return
        self.world_view_transform.copy_(cam.world_view_transform, non_blocking=True)
        self.full_proj_transform.copy_(cam.full_proj_transform, non_blocking=True)
        self.camera_center.copy_(cam.camera_center, non_blocking=True)


class GraphedTrainStep:
    def __init__(self, pc, optimizer, bg, lambda_dssim=0.2, pipe=Pipe, render_kwargs=None, densify_stats=False, dynamic=False,
                 which_object=1, gated=False, check_every=0, steps_per_replay=1, fuse_optimizer=True, double_buffer=False, loss_grad_in_blend=True,
                 motion=False, object_loss=None, pose=None, label_phase=False, entropy_reg=False, frame_store=None, ring_capacity=4096,
                 pose_sequence=None, deterministic=False):
        """deterministic: every backward of the step -- warm-up and captured -- runs with CALL_DETERMINISTIC (include/egs_raster.h: the backward
                       blend's sums as integer atomics in two passes): parameters, moments and statistics after N replays from one seeded
                       start are the same bits in every run.  Goes with every other option; costs a second pass of the backward blend
                       and two small launches per iteration (profiles/deterministic_backward.md).
        pose_sequence: (with dynamic=True, motion=True; not with pose=: ValueError) a poses.PoseSequence -- the object stages' pose table on
                       the device.  Every frame carries the word `pose_rows` = (fixed_row, train_row, reload) (pack_frame(pose_rows=),
                       PoseSequence.rows); per iteration the capture holds, in order, egs_pose_head (reads the slot's word, WRITES the
                       slot's accum_T / accum_R -- the buffers the rasterizer reads), the step, whose backward leaves dL/dA12, dL/dM9 in
                       a static float32[21], and egs_pose_tail (dL/dpose, the pose's own Adam step, the frame's table row, the
                       accumulated rows after it).  No torch launch for the pose on either side and no optimizer group for it:
                       the pose's learning rates are PoseSequence.set_lr's device scalars.  A frame with train_row = -1 is a fixed-pose
                       frame: the same captured step renders it with accum[fixed_row] and leaves the pose and its Adam state alone --
                       the coarse stage's alternation.  `pose_sequence.dpose` holds dL/dpose of the last trainable frame.
        frame_store:   a frames.FrameStore of this step's layout (dynamic, motion, gated, object_loss, label_phase as given here, else
                       ValueError): the dataset stays on the device in 8 bits and the captured graph BEGINS with one decode launch that
                       writes the static frames of all `steps_per_replay` iterations from it, by index (include/egs_raster.h
                       egs_frame_decode) -- no frame copy, no host work per replay beyond the launch.  capture(cam, index=i0): `cam` gives
                       the image size and field of view, the warm-up steps run on frame i0.  step(indices) -- an int (steps_per_replay = 1),
                       a sequence of S ints or an int32 device tensor of S entries -- writes them to the step's ring (`ring_capacity`
                       entries, its own: a sweep over the same store leaves it alone) and replays; set_schedule(indices) writes K = a
                       multiple of S entries once, after which step() only pushes learning rates and replays: replay n trains on entries
                       nS .. nS + S - 1, wrapping at K.  Host indices are range-checked (IndexError); store_ok() tells whether the kernel
                       ever had to clamp one.  Not with double_buffer (ValueError): nothing is left to hide.  None: packed float frames.
        entropy_reg:   the static image step with the entropy-regularisation phase available (/root/reference/trainers/train_static.py:97-102,
                       trainers/train_static_bg.py:105-110: between std_train_iter and std_train_iter + entropy_reg_iter the loss also holds
                       0.1 * the mean binary entropy of the visible opacities).  The rasterizer's backward adds the term's share to the
                       gradient of the opacity logits itself (render(opacity_entropy=)), so the opacity stays a fused leaf and the step
                       stays the captured one.  The weight is a DEVICE scalar pushed before each replay like the learning rates:
                       `step.entropy_weight = 0.1` at std_train_iter, `= 0.0` when the phase ends -- no re-capture; it starts at 0, and with
                       weight 0 a replay leaves every parameter and moment bit-identical to the step captured without this option.
                       `step.entropy` (device float32[1]) holds the last replay's UNWEIGHTED mean entropy.  `step.loss` and `loss_sum` stay
                       the image loss alone: the term's value is not added to them.  Goes with gated, densify_stats, steps_per_replay,
                       double_buffer and capacity-sized models; not with dynamic, motion, pose, object_loss, label_phase (ValueError).
        label_phase:   the label phase of the static stage (/root/reference/trainers/train_static.py:104-109) instead of the image step:
                       the label render with the label as one value per Gaussian, BCE-with-logits of its channel mean against the frame's
                       object mask (gated: the hand-mask hook), Adam on the label ALONE -- forward chain, backward prologue, the scalar
                       colours-only blend that forms the loss gradient itself, and one launch that reads dL/dlabel out, takes the step and
                       assembles the value (include/egs_raster.h egs_backward_label).  No colour render() runs: in that phase its image
                       reaches no loss.  The optimizer must have a "label" group; no other group is touched (their .grad is None in the
                       reference too).  capture(cam, obj_mask=, gate=) / __call__(cam, obj_mask=, gate=) or pack_label_frame() frames.
                       `self.image` is the label render, `self.label_grad` the dL/dlabel [P] of the last replay.
        densify_stats: the captured step also keeps the per-iteration densification statistics (trainers/train_static.py:125-127:
                       max_radii2D, xyz_gradient_accum, denom) -- updated by the rasterizer's backward itself, no launch of their own.
        dynamic:       the `fine_all` call shape (/root/reference/trainers/fine_all.py:88-93): render(..., rot_cov=True,
                       accum_R=<static 3x3, refreshed per call>, which_object=which_object, during_training=False).
        motion:        (with dynamic) the real `fine_all` step: the object's Gaussians are also PLACED by the frame's accumulated pose
                       (<static 3x4 accum_T, refreshed per call like accum_R>) inside the rasterizer -- render(..., object_motion=) --
                       instead of by apply_trans_rot_new / reverse_trans_rot_new around the render (fine_all.py:88-116), which would
                       re-seat `_xyz` every iteration and could not be captured.  Without `pose` the pose is a constant of the captured step.
        pose:          (with motion) the trainable pose of the object stages ON TOP of the frame's accumulated one: a module with
                       `obj_translation`, `obj_rotation_6d` and `rot_L` (the reference's ObjectMove, utils/geometry_utils.py:14-33;
                       coarse_obj_pose.py, fine_obj.py).  The captured step composes motion.ObjectMotion(accum_T, pose, accum_R) from the
                       static buffers (a few tiny torch launches), the rasterizer returns dL/dA12 and dL/dM9, autograd carries them to the
                       two parameters, and `optimizer.step()` inside the capture steps them: they must be ordinary groups of the SAME
                       FusedAdam(capturable=True).  Their learning rates are device scalars like every other group's: zeroing or restoring
                       groups' "lr" (the stages' zero_gaussians_lr / zero_pose_lr / load_lrs) needs no re-capture.
        object_loss:   dict(lambda_image=, lambda_l1_alpha=, lambda_l2_alpha=): the object stages' loss (fused.object_stage_loss) instead of
                       the image loss -- the render composites alpha, the frame carries an `obj_mask` segment and stores gt * obj_mask
                       (pack_frame(obj_mask=)), the gate (gated=True) applies to the image's AND alpha's gradient.  `self.loss_terms`
                       (device float32[3]) holds the last step's image loss, mean|m - alpha| and mean (m - alpha)^2.
        gated:         the image gradient is multiplied by a per-pixel gate refreshed per call -- the reference's
                       `render_image.register_hook(lambda grad: grad * (1 - hand_mask))` (train_static.py:91, fine_all.py:94).
        check_every:   K > 0: every K calls read the overflow maximum (one host synchronisation) and re-capture with a larger
                       instance capacity if a frame was clipped (its update was skipped, see the module docstring).
        steps_per_replay: S > 1 captures S complete iterations back to back, each on its own static frame; one launch then runs
                       S training steps on S frames (`__call__` takes the S packed frames as one [S, frame] tensor or a list).  A
                       graph launch leaves the GPU idle for ~9 us before its first node; this divides that by S.
        double_buffer: capture the step TWICE, on two sets of static frame buffers, and alternate between the two graphs: the copy of
                       call k + 1's frames then runs on a side stream while call k's replay is still working (it only has to wait for
                       replay k - 1, the last user of its buffer), instead of between two replays (packed frames only; 31 MB per five
                       960x540 frames: 2.7 us per step).  Results are those of the single-buffered step.  MEASURED at config C: 1.6 % slower than
                       the single graph (3 175 vs 3 225 it/s) -- the event waits between the streams cost more than the hidden copy --,
                       so it is off by default and bench.py does not use it.
        loss_grad_in_blend: the captured step has NO loss-backward launch: the rasterizer's backward blend computes the image loss's gradient
                       for its tile itself, from the maps the loss forward leaves, bit-identical to the launch it replaces
                       (fused.l1_ssim_loss(raster_lossgrad=True), include/egs_raster.h egs_backward_lossgrad): nine launches per step -> eight.
        fuse_optimizer: the parameters render() hands to the rasterizer as stored take their Adam step inside its backward
                       (renderer.render, optimizer=): no gradient arrays, no optimizer launch for them; the step's loss must then
                       depend on the model through that one render only -- which is the step this class captures.  Results are
                       bit-identical either way."""
        self.frame_store, self._ring = frame_store, None
        self.deterministic = bool(deterministic)
        if frame_store is not None:
            if double_buffer:
                raise ValueError("GraphedTrainStep(frame_store=) does not go with double_buffer: the decode is part of the graph, no copy is left to hide")
            mine = dict(dynamic=bool(dynamic), motion=bool(motion), gated=bool(gated), object_loss=object_loss is not None, label_phase=bool(label_phase))
            if pose_sequence is not None:
                mine["pose_rows"] = True
            if frame_store.layout != mine:
                raise ValueError(f"GraphedTrainStep(frame_store=): the store's layout {frame_store.layout} is not this step's {mine}")
            self._ring_capacity = int(ring_capacity)
            if self._ring_capacity < max(1, int(steps_per_replay)):
                raise ValueError("GraphedTrainStep(frame_store=): ring_capacity >= steps_per_replay")
        self.entropy_reg = bool(entropy_reg)
        if self.entropy_reg:
            for name, on in (("dynamic", dynamic), ("motion", motion), ("pose", pose is not None), ("object_loss", object_loss is not None),
                             ("label_phase", label_phase)):
                if on:
                    raise ValueError(f"GraphedTrainStep(entropy_reg=True) does not go with {name}: the entropy term belongs to the static image step")
        self._entropy_weight_host, self._entropy_weight_dev, self._entropy_weight_pushed = 0.0, None, None
        self.entropy = None
        self.label_phase = bool(label_phase)
        if self.label_phase:
            for name, on in (("dynamic", dynamic), ("motion", motion), ("pose", pose is not None), ("object_loss", object_loss is not None),
                             ("densify_stats", densify_stats), ("double_buffer", double_buffer)):
                if on:
                    raise ValueError(f"GraphedTrainStep(label_phase=True) does not go with {name}: the label step renders the static model, "
                                     "trains the label alone and keeps one set of frame buffers")
            groups = [g for g in optimizer.param_groups if g.get("name") == "label"]
            if len(groups) != 1 or len(groups[0]["params"]) != 1:
                raise ValueError('GraphedTrainStep(label_phase=True) needs a "label" parameter group (one tensor) in the optimizer given')
            self._label_group = groups[0]
        self.label_grad = None
        self.fuse_optimizer = bool(fuse_optimizer)
        import os
        self.loss_grad_in_blend = bool(loss_grad_in_blend) and not os.environ.get("EGS_NO_LOSS_GRAD_IN_BLEND")      # (A/B switch for bench.py)
        self.double_buffer = bool(double_buffer)
        if not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedTrainStep needs FusedAdam(capturable=True)")
        self.pc, self.opt, self.bg, self.lam, self.pipe = pc, optimizer, bg, lambda_dssim, pipe
        self.densify_stats = densify_stats
        self.dynamic, self.which_object, self.gated = bool(dynamic), which_object, bool(gated)
        self.motion = bool(motion)
        if self.motion and not self.dynamic:
            raise ValueError("GraphedTrainStep(motion=True) goes with dynamic=True (the pose's rotation turns the covariances)")
        self.pose = pose
        if pose is not None:
            if not self.motion:
                raise ValueError("GraphedTrainStep(pose=) goes with dynamic=True, motion=True (the trainable pose sits on top of the frame's)")
            owned = {id(p) for g in optimizer.param_groups for p in g["params"]}
            if id(pose.obj_translation) not in owned or id(pose.obj_rotation_6d) not in owned:
                raise ValueError("GraphedTrainStep(pose=): obj_translation and obj_rotation_6d must be parameter groups of the optimizer "
                                 "given (its step() inside the capture is what moves them)")
        self.pose_sequence, self._pose_grads = pose_sequence, None
        if pose_sequence is not None:
            if pose is not None:
                raise ValueError("GraphedTrainStep(pose_sequence=) does not go with pose=: the sequence owns the trainable pose and its Adam state")
            if not self.motion:
                raise ValueError("GraphedTrainStep(pose_sequence=) goes with dynamic=True, motion=True (its head writes the frame's accum_T / accum_R)")
        self.object_loss = None if object_loss is None else dict(object_loss)
        if self.object_loss is not None and set(self.object_loss) - {"lambda_image", "lambda_l1_alpha", "lambda_l2_alpha"}:
            raise ValueError("GraphedTrainStep(object_loss=): a dict of lambda_image, lambda_l1_alpha, lambda_l2_alpha")
        self.loss_terms = None
        self.render_kwargs = dict(render_kwargs or {})
        self.check_every = int(check_every)
        self.steps_per_replay = max(1, int(steps_per_replay))
        self.graph = None
        self._sets = None
        self.guard = None
        self.loss_sum = None
        self.recaptures = 0               # re-captures this object did on its own (overflow)
        self.skipped_frames_seen = 0      # overflow events noticed by check()
        self._calls = 0

    @property
    def entropy_weight(self):
        """The weight of the entropy term (entropy_reg=True): a host float, pushed into the device scalar the captured kernels read
        before the next replay -- the reference's 0.1 during its entropy phase, 0 outside."""
        return self._entropy_weight_host

    @entropy_weight.setter
    def entropy_weight(self, w):
        if not self.entropy_reg:
            raise ValueError("entropy_weight: this step was built without entropy_reg=True")
        self._entropy_weight_host = float(w)

    def _sync_entropy_weight(self):
        """A fill when the weight was edited since the last push (as FusedAdam.sync_lr for the learning rates)."""
        if self._entropy_weight_dev is not None and self._entropy_weight_pushed != self._entropy_weight_host:
            self._entropy_weight_dev.fill_(self._entropy_weight_host)
            self._entropy_weight_pushed = self._entropy_weight_host

    def _label_body(self, k=0):
        old = _C.deterministic_backward(True) if self.deterministic else None      # (the bit travels in the calls the body makes; captured, it stays in the graph)
        try:
            return self._label_body_(k)
        finally:
            if old is not None:
                _C.deterministic_backward(old)

    def _body(self, k=0):
        old = _C.deterministic_backward(True) if self.deterministic else None
        try:
            return self._body_(k)
        finally:
            if old is not None:
                _C.deterministic_backward(old)

    def _label_body_(self, k=0):
        """One iteration of the label phase on static frame k: no autograd, the library's calls in order."""
        from . import lib as _lib
        from .optim import _touched
        f, pc, opt, group = self._slots[k], self.pc, self.opt, self._label_group
        p = group["params"][0]
        cam = f["cam"]
        dev = p.device
        capturing = torch.cuda.is_current_stream_capturing()
        with torch.no_grad():
            H, W = int(cam.image_height), int(cam.image_width)
            R, color, radii, geom, binning, img = label_forward(cam, pc, p, self.bg, guard=self.guard)
            m, v, step, lr_t = opt._capturable_state(p, group)
            coef = opt._coef.get(dev)
            if coef is None:
                coef = opt._coef[dev] = torch.zeros(12, device=dev)
            leaf = _lib.AdamLeaf()
            leaf.param, leaf.exp_avg, leaf.exp_avg_sq, leaf.lr, leaf.step = p.data_ptr(), m.data_ptr(), v.data_ptr(), lr_t.data_ptr(), step.data_ptr()
            rows = None
            if opt.active_rows is not None and p.shape[0] == opt.active_rows[1]:
                rows = opt.active_rows[0]
            loss = torch.empty((), device=dev)
            st, keep = _C.label_loss_struct(color, f["obj_mask"], self._one.view(1), f["gate"] if self.gated else None, None, loss.view(1), self.loss_sum.view(1))
            # (the overflow word is written by CAPTURED forwards only: an eager warm-up step follows a complete render)
            dl = _C.backward_label(radii, geom, R, binning, img, H, W, label_loss=st, adam=(leaf, float(group["betas"][0]), float(group["betas"][1]),
                                   float(group["eps"]), coef), active_rows=rows, guard=self.guard if capturing else None)
            opt._aux_of(p)["counter_stale"] = True        # k_adam's own step counters do not follow a step taken here (optim.AdamSink.mark_stepped)
            _touched(p)
        self._label_keep = (keep, m, v, step, lr_t, coef, geom, binning, img)
        return loss, {"render": color, "radii": radii, "label_grad": dl}

    def _body_(self, k=0):
        """One training iteration on static frame k."""
        f = self._slots[k]
        kw = dict(self.render_kwargs)
        seq = self.pose_sequence
        if seq is not None:
            seq.head(f["pose_rows"], f["accum_T"], f["accum_R"])     # the frame's pose, composed on the device into the buffers the rasterizer reads
        if self.dynamic:
            kw.update(dynamic_kwargs(f, self.which_object, self.pose, None if seq is None else self._pose_grads[k]))
        if self.entropy_reg:
            kw["opacity_entropy"] = self._entropy_weight_dev         # the device scalar itself: the kernels read it at every replay
        out = render(f["cam"], self.pc, self.pipe, self.bg, fused_densify_stats=self.densify_stats, guard=self.guard,
                     optimizer=self.opt if self.fuse_optimizer else None, color_only=self.object_loss is None, **kw)      # (the image loss reads the colour image only)
        # the loss value and the running sum are produced by the loss BACKWARD kernel (nothing reads them before): two launches less
        if self.object_loss is not None:
            loss = object_stage_loss(out["render"], out["alpha"], f["gt"], f["obj_mask"], self.lam, grad_gate=f["gate"] if self.gated else None,
                                     running_sum=self.loss_sum, terms=self.loss_terms, defer_value=True, raster_prologue=True,
                                     raster_lossgrad=self.loss_grad_in_blend, gt_premasked=True, **self.object_loss)
        else:
            loss = l1_ssim_loss(out["render"], f["gt"], self.lam, grad_gate=f["gate"] if self.gated else None, running_sum=self.loss_sum,
                                defer_value=True, raster_prologue=True, raster_lossgrad=self.loss_grad_in_blend)
        loss.backward(gradient=self._one)                            # a resident 1.0: no fill kernel per iteration
        if seq is not None:
            # (the overflow word is written by CAPTURED forwards only: an eager warm-up step follows a complete render)
            seq.tail(f["pose_rows"], self._pose_grads[k], skip=self.guard.overflow if torch.cuda.is_current_stream_capturing() else None)
        self.opt.step()                                             # whatever the backward did not step itself (fuse_optimizer)
        return loss.detach(), out

    def _layout(self, H, W):
        return frame_layout(0 if self.label_phase else 3 * H * W, H * W, self.dynamic, self.gated, self.motion, self.object_loss is not None,
                            self.label_phase, pose_rows=self.pose_sequence is not None)

    def _decode_frames(self):
        """frame_store=: the first launch of the captured graph -- every static frame from the store, by the ring; the cursor advances on the device."""
        if self.frame_store is not None:
            self.frame_store.decode(self._frames, ring=self._ring)

    def _store_frame(self, index, given):
        """frame_store=: the inputs of capture() from frame `index` of the store (the static frames are filled from them, the warm-up runs on them)."""
        if any(v is not None for v in given):
            raise ValueError("GraphedTrainStep(frame_store=).capture(cam, index=i0): the frame's contents come from the store")
        store = self.frame_store
        parts = store.parts(0 if index is None else index)
        if self._ring is None:
            self._ring = store.new_ring(self._ring_capacity)
        self._ring.set([0 if index is None else int(index)] * self.steps_per_replay)
        self._ring_set = False
        return parts

    def _make_slots(self, frames, cams):
        """The static inputs of the captured iterations: per row k of `frames` its named views (frame_views), the camera segment as a
        _StaticCamera filled from cams[k]."""
        H, W = int(cams[0].image_height), int(cams[0].image_width)
        off, _ = self._layout(H, W)
        slots = []
        for fr, cam in zip(frames, cams):
            slot = frame_views(fr, off, H, W)
            slot["cam"] = _StaticCamera(cam, storage=slot["cam"])
            slots.append(slot)
        return slots

    def _record(self):
        """The body of the captured graph on the current slots: the decode of a frame store, then `steps_per_replay` iterations ->
        what a replay leaves behind, under the attribute names it is published by."""
        self._decode_frames()
        losses, label_grads, keeps = [], [], []
        for k in range(self.steps_per_replay):
            if self.label_phase:
                loss, out = self._label_body(k)
                label_grads.append(out["label_grad"]); keeps.append(self._label_keep)
            else:
                if k:
                    self.opt.zero_grad(set_to_none=True)             # (the next backward writes fresh gradients instead of accumulating)
                loss, out = self._body(k)
            losses.append(loss)
        if self.label_phase:
            return dict(loss=loss, losses=losses, image=out["render"], radii=out["radii"], label_grad=out["label_grad"], label_grads=label_grads,
                        _label_keeps=keeps, visibility_filter=None, viewspace_grad=None)
        return dict(loss=loss, losses=losses, image=out["render"].detach(), radii=out["radii"],
                    entropy=out.get("opacity_entropy"),                  # (entropy_reg: written by every replay's backward)
                    visibility_filter=out["visibility_filter"],          # follows every replay (a view of the rasterizer's saved state)
                    viewspace_grad=out["viewspace_points"].grad)

    def _publish(self, out):
        for name, value in out.items():
            setattr(self, name, value)

    def capture(self, cam, gt=None, warmup=3, capacity_margin=1.25, accum_R=None, gate=None, capacity_cams=None, capacity=None, accum_T=None,
                obj_mask=None, index=None, pose_rows=None):
        """Runs `warmup` eager iterations on (cam, gt) -- they are real training steps -- then records (without executing) one
        more into the graph.  pose_rows (pose_sequence=): the (fixed_row, train_row[, reload]) of the frame the warm-up runs on (default:
        no row at all -- the identity, nothing trained, the table untouched).  capacity_cams: further cameras whose instance counts size the captured capacity (a forward-only
        render each); without them the capacity is `capacity_margin` x the count of `cam` alone, and R varies across views.
        capacity: the instance capacity to capture with, as is (overrides the margin rule; tests use it to provoke an overflow).
        obj_mask (object_loss=): the frame's object mask; `gt` is the frame as loaded, the static buffer stores gt * obj_mask.
        A label step (label_phase=True) takes capture(cam, obj_mask=, gate=): its static frame holds camera[, gate], obj_mask."""
        label, fresh = self.label_phase, not isinstance(cam, _StaticCamera)
        if self.frame_store is not None and fresh:
            if (int(cam.image_height), int(cam.image_width)) != (self.frame_store.H, self.frame_store.W):
                raise ValueError(f"GraphedTrainStep(frame_store=).capture: the camera is {cam.image_width}x{cam.image_height}, the store's frames "
                                 f"{self.frame_store.W}x{self.frame_store.H}")
            parts = self._store_frame(index, (gt, accum_R, gate, accum_T, obj_mask, pose_rows))
            gt, accum_R, gate, accum_T, obj_mask = parts["gt"], parts["accum_R"], parts["gate"], parts["accum_T"], parts["obj_mask"]
            pose_rows = parts.get("pose_rows")                           # (the stored word itself, an int32[4] tensor)
        elif index is not None:
            raise ValueError("capture(index=) goes with GraphedTrainStep(frame_store=)")
        if label and obj_mask is None and fresh:
            raise ValueError("GraphedTrainStep(label_phase=True).capture(cam, obj_mask=...): the label step's frame is camera[, gate], obj_mask")
        dev = self._label_group["params"][0].device if label else gt.device
        H, W = int(cam.image_height), int(cam.image_width)
        if obj_mask is not None and (label or self.object_loss is not None):
            obj_mask = obj_mask.to(dev, torch.float32).reshape(H, W)
            if not label:
                gt = gt * obj_mask
        if not fresh:                                                # recapture: keep the static buffers
            if not label and gt is not self.gt:
                self.gt.copy_(gt)
        else:
            # per captured iteration: image, camera[, accum_R][, accum_T][, gate][, obj_mask] -- ONE copy target for all of them
            self._frames = torch.zeros((self.steps_per_replay, self._layout(H, W)[1]), device=dev, dtype=torch.float32)
            self._slots = self._make_slots(self._frames, [cam] * self.steps_per_replay)
            ones = lambda: torch.ones((H, W), device=dev)
            given = (("gt", gt, None), ("accum_R", accum_R, lambda: torch.eye(3, device=dev)),
                     ("accum_T", None if accum_T is None else accum_T.reshape(-1, 4)[:3], lambda: torch.eye(4, device=dev)[:3]),
                     ("gate", gate.reshape(H, W) if gate is not None and gate.numel() == H * W else gate, ones), ("obj_mask", obj_mask, ones))
            for slot in self._slots:
                for name, value, default in given:
                    if slot[name] is not None:
                        slot[name].copy_(default() if value is None else value)
                if self.pose_sequence is not None:
                    slot["pose_rows"].copy_(pose_rows if torch.is_tensor(pose_rows) else pose_word((-1, -1) if pose_rows is None else pose_rows))
            if self.pose_sequence is not None:
                self._pose_grads = torch.zeros((self.steps_per_replay, 21), device=dev, dtype=torch.float32)      # dL/dA12, dL/dM9 per captured iteration
            self._frame = self._frames[0]
            first = self._slots[0]                                   # (the single-iteration names)
            self.gt, self.cam, self.accum_R, self.accum_T, self.gate, self.obj_mask = (first[n] for n in ("gt", "cam", "accum_R", "accum_T", "gate", "obj_mask"))
        self._one = torch.ones((), device=dev)
        if self.entropy_reg and self._entropy_weight_dev is None:
            self._entropy_weight_dev = torch.zeros((), device=dev)
        self._sync_entropy_weight()
        if getattr(self, "loss_sum", None) is None:
            self.loss_sum = torch.zeros((), device=dev)                  # sum of the losses of every iteration run through this object
        if self.object_loss is not None and self.loss_terms is None:
            self.loss_terms = torch.zeros(3, device=dev)
        self.guard = _C.StepGuard(dev)
        self.opt.guard = self.guard                                  # the Adam launch of an overflowed frame does nothing
        if label:
            self.opt.sync_lr()                                       # (the label body reads the device learning rate itself)
        calls = []
        if capacity_cams and not label:                              # (a label step sizes its capacity on `cam` alone)
            kw = dict(self.render_kwargs)
            if self.dynamic:
                kw.update(dynamic_kwargs(self._slots[0], self.which_object, self.pose))

            def look(c):
                with torch.no_grad():
                    render(c, self.pc, self.pipe, self.bg, **kw)
            calls += [lambda c=c: look(c) for c in capacity_cams]

        def one_step():                                              # eager: a real step; sets the capacity hint, allocator pools, lazy state
            if label:
                return self._label_body()
            self.opt.zero_grad(set_to_none=True)
            self._body()
        side = torch.cuda.Stream(device=dev)
        r_seen = warm_up(calls + [one_step] * max(1, warmup), side, dev)
        self.capacity = capture_capacity(r_seen, capacity_margin, dev, getattr(self, "_min_capacity", 0), capacity)
        self.P = self.pc.get_xyz.shape[0]
        self._model_version = getattr(self.pc, "model_version", 0)
        if not label:
            self.opt.zero_grad(set_to_none=True)
        self.graph, out = record_graph(self._record, side, dev)
        self._publish(out)
        self._sets = None
        if self.double_buffer:
            # the same iterations recorded once more on a second set of static frames; what the two captures share -- parameters,
            # optimizer state, guard words, loss_sum -- is shared by address
            first = dict(graph=self.graph, frames=self._frames, slots=self._slots, out=out)
            frames2 = self._frames.clone()
            self._slots = self._make_slots(frames2, [s["cam"] for s in first["slots"]])
            self.opt.zero_grad(set_to_none=True)
            g2, out2 = record_graph(self._record, side, dev)
            second = dict(graph=g2, frames=frames2, slots=self._slots, out=out2)
            self._slots = first["slots"]
            self._sets = [first, second]
            self._copy_stream = torch.cuda.Stream(device=dev)
            self._done = [torch.cuda.Event(), torch.cuda.Event()]       # replay of set b finished reading its frames
            self._copied = [torch.cuda.Event(), torch.cuda.Event()]
            self._used = [False, False]
        self.guard.running_max.zero_(); self.guard.overflow.zero_()
        return self

    def recapture(self, cam=None, gt=None, warmup=1, capacity_margin=1.25, capacity_cams=None):
        """Capture again with the model as it is now -- after densification / pruning replaced the parameters, or after ok()
        reported a frame that outgrew the capacity.  Like capture(), the `warmup` eager iterations are real training steps."""
        cam = self.cam if cam is None else cam
        gt = self.gt if gt is None else gt
        self.graph = None                                            # drop the old graph and its private memory pool first
        self._sets = None
        if self.label_phase:
            return self.capture(cam, None, warmup=warmup, capacity_margin=capacity_margin, obj_mask=self.obj_mask, gate=self.gate)
        return self.capture(cam, gt, warmup=warmup, capacity_margin=capacity_margin, capacity_cams=capacity_cams)

    def __call__(self, cam=None, gt=None, accum_R=None, gate=None, ready=None, accum_T=None, obj_mask=None, pose_rows=None):
        """One training iteration (steps_per_replay of them): copy inputs in, replay.  Returns the (device, static) loss tensor of
        the last iteration (`self.losses` has all).  Either (camera, ground-truth image[, accum_R][, gate]) or packed frames from
        pack_frame(): one for a single-iteration step, a [S, frame] tensor (one copy) or a list of S for steps_per_replay = S.
        ready (double_buffer only): a torch.cuda.Event recorded after the packed frames were COMPLETELY written; the side-stream copy
        waits for it.  Without it the copy waits for everything enqueued on the current stream so far -- always correct, but frames
        produced on the current stream right before the call then serialise behind the replay that is still running."""
        if self.frame_store is not None:
            if any(v is not None for v in (gt, accum_R, gate, ready, accum_T, obj_mask)):
                raise ValueError("GraphedTrainStep(frame_store=): step(indices) or, after set_schedule(), step()")
            if cam is not None:                                          # frame indices: ring[0:S], ctl = {0, S} as one small copy
                k = 1 if isinstance(cam, int) else int(cam.numel()) if torch.is_tensor(cam) else len(cam)
                if k != self.steps_per_replay:
                    raise ValueError(f"step(indices): {k} indices given, {self.steps_per_replay} frames per replay")
                self._ring.set(cam)
                self._ring_set = True
            elif not self._ring_set:
                raise ValueError("step(): no frame indices yet -- step(indices) or set_schedule(indices) first")
        elif cam is None:
            raise ValueError("GraphedTrainStep: a camera or packed frames (step() without arguments goes with frame_store=)")
        elif gt is None and self._sets is not None:
            return self._call_double_buffered(cam, ready)
        elif self.label_phase and obj_mask is not None:
            if self.steps_per_replay != 1:
                raise ValueError("steps_per_replay > 1 takes packed frames")
            self.cam.load(cam)
            self.obj_mask.copy_(obj_mask.reshape(self.obj_mask.shape), non_blocking=True)
            if self.gated and gate is not None:
                self.gate.copy_(gate.reshape(self.gate.shape), non_blocking=True)
        elif gt is None:
            if isinstance(cam, (list, tuple)):
                for k, fr in enumerate(cam):
                    self._frames[k].copy_(fr, non_blocking=True)
            else:
                self._frames.copy_(cam.view(self._frames.shape), non_blocking=True)
        else:
            if self.steps_per_replay != 1:
                raise ValueError("steps_per_replay > 1 takes packed frames")
            self.cam.load(cam)
            if self.object_loss is not None and obj_mask is not None:
                self.obj_mask.copy_(obj_mask.reshape(self.obj_mask.shape), non_blocking=True)
                torch.mul(gt, self.obj_mask, out=self.gt)                # (object_loss=: the static image is gt * obj_mask)
            else:
                self.gt.copy_(gt, non_blocking=True)
            if self.dynamic and accum_R is not None:
                self.accum_R.copy_(accum_R, non_blocking=True)
            if self.motion and accum_T is not None:
                self.accum_T.copy_(accum_T.reshape(-1, 4)[:3], non_blocking=True)
            if self.gated and gate is not None:
                self.gate.copy_(gate, non_blocking=True)
            if self.pose_sequence is not None and pose_rows is not None:
                self._slots[0]["pose_rows"].copy_(pose_word(pose_rows), non_blocking=True)
        self._before_replay()
        self.graph.replay()
        return self._after_replay()

    def _before_replay(self):
        if getattr(self.pc, "model_version", 0) != self._model_version:
            raise RuntimeError("GraphedTrainStep: the model reallocated its arrays (CapacityGaussians.grow) after this step was captured; "
                               "the captured launches point at freed memory -- call recapture() first")
        self.opt.sync_lr()                                           # a fill per group whose learning rate was edited since the last call
        self._sync_entropy_weight()

    def _after_replay(self):
        self._calls += 1
        if self.check_every > 0 and self._calls % self.check_every == 0:
            self.check()
        return self.loss

    def set_schedule(self, indices):
        """frame_store=: the frames of the coming replays, once: a 1-D sequence (or int32 device tensor) whose length K is a multiple of
        steps_per_replay and at most the ring's capacity (ValueError), range-checked on the host (IndexError), written to the ring with
        ctl = {0, K} as one small copy.  step() then only replays: replay n trains on entries nS .. nS + S - 1, wrapping at K."""
        if self.frame_store is None:
            raise ValueError("set_schedule: this step was built without frame_store=")
        if self._ring is None:
            raise ValueError("set_schedule: capture() first (the ring is made there)")
        k = int(indices.numel()) if torch.is_tensor(indices) else len(indices)
        if k < 1 or k % self.steps_per_replay or k > self._ring.capacity:
            raise ValueError(f"set_schedule: {k} indices; a positive multiple of steps_per_replay = {self.steps_per_replay}, at most the ring's "
                             f"capacity {self._ring.capacity}")
        self._ring.set(indices)
        self._ring_set = True

    def store_ok(self):
        """frame_store=: True while the decode never had to clamp a frame index (reads the store's status word: synchronises)."""
        return self.frame_store.ok()

    def _call_double_buffered(self, frames, ready=None):
        """Packed frames, two captured graphs: the copy into set b's static frames runs on a side stream as soon as set b's previous
        replay has finished, i.e. under the replay of the other set that is still running.  The copy reads the caller's tensors on
        that side stream, so it must be ordered after whatever WROTE them: the caller's `ready` event, else the current stream as it
        stands now; and the tensors are marked as used by the side stream so that the allocator does not recycle them under the copy."""
        b = self._calls & 1
        st = self._sets[b]
        main = torch.cuda.current_stream(st["frames"].device)
        if self._used[b]:
            self._copy_stream.wait_event(self._done[b])
        if ready is not None:
            self._copy_stream.wait_event(ready)
        else:
            self._copy_stream.wait_stream(main)                      # whatever produced the frames (and, the first time, the capture)
        with torch.cuda.stream(self._copy_stream):
            if isinstance(frames, (list, tuple)):
                for k, fr in enumerate(frames):
                    st["frames"][k].copy_(fr, non_blocking=True)
                    fr.record_stream(self._copy_stream)
            else:
                st["frames"].copy_(frames.view(st["frames"].shape), non_blocking=True)
                frames.record_stream(self._copy_stream)
            self._copied[b].record(self._copy_stream)
        self._before_replay()
        main.wait_event(self._copied[b])
        st["graph"].replay()
        self._done[b].record(main)
        self._used[b] = True
        self._publish(st["out"])
        return self._after_replay()

    def check(self, capacity_margin=1.25):
        """Reads the running maximum of the instance count (synchronises).  If a replayed frame was clipped -- its parameter
        update was skipped on the device -- re-captures with room for it and returns False; True otherwise."""
        if self.ok():
            return True
        self.skipped_frames_seen += 1
        self._min_capacity = int(self.max_instances() * capacity_margin) + 65536
        self.recaptures += 1
        self.recapture(warmup=1, capacity_margin=capacity_margin)
        return False

    def last_instance_count(self):
        """Instances the most recent replay bucketed; call after synchronising.  More than `capacity` means that frame was
        clipped (and its update skipped)."""
        return int(self.guard.overflow[1].item()) & 0xffffffff

    def last_frame_overflowed(self):
        return bool(int(self.guard.overflow[0].item()))

    def max_instances(self):
        """Largest R over every replay since the capture (reads a device scalar: synchronises)."""
        return int(self.guard.running_max.item())

    def ok(self):
        """True if no replayed frame exceeded the captured capacity (i.e. every one of them was rendered completely)."""
        return self.max_instances() <= self.capacity
