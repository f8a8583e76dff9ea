"""Rigid object motion as an INPUT of the render instead of a mutation of the model (PyTorch, autograd).

Every EgoGaussian stage after the static one poses the object's Gaussians per frame: `gaussians.apply_trans_rot_new(...)` rebuilds
`_xyz` out of place before the render and `reverse_trans_rot_new(...)` undoes it through a matrix inverse afterwards
(/root/reference/scene/gaussian_model.py:939-986,1037-1060; /root/reference/trainers/coarse_obj_pose.py:229-239,313-317,
/root/reference/trainers/fine_all.py:88-116).  Here the same rule yields a small value, an ObjectMotion, and nothing is touched:

    select_motion(accum_T_seq, accum_R_seq, image_name, during_training, trainable)   which pose the frame gets (None: no motion)
    ObjectMotion.compose()        (A12 [3,4], M [3,3]) with autograd:  p' = A p + b for the moved rows, L' = M L for the rotated ones
    move_points / unmove_points   the placement and its inverse as tensor expressions -- CPU tensors, tests, the oracle of the HIP
                                  kernels (egogaussian_amd.fused.object_move_points), the role covariance.py plays for cov3d.hip

The composition is deliberately plain torch on 3x3 tensors: the kernels see ONE general affine form, autograd carries dL/dA12 and
dL/dM back to `obj_translation` and `obj_rotation_6d`, and the same code serves the fixed pose (fine_all) and the trainable pose
(coarse_obj_pose, fine_obj).
"""
import torch


def exact_mask(is_object, which_object):
    """The rows the reference MOVES: torch.where(is_object == which_object, ...) -- the exact mask, every row when which_object is
    None.  (The rows whose covariance it ROTATES are a different set: fused.object_selection, the [N,1]-index quirk.)"""
    if which_object is None or is_object is None:
        return None
    return is_object.reshape(-1) == which_object


class ObjectMotion:
    """A frame's object pose: the accumulated 4x4 `fixed_T` (with its rotation `fixed_R`, the reference keeps the two in separate
    sequences; default: the rotation block of fixed_T) and, during pose training, an ObjectMove-shaped module on top of it
    (/root/reference/utils/geometry_utils.py:14-33).  The module is read through `rot_L(eye)` and `obj_translation` only."""

    def __init__(self, fixed_T=None, trainable=None, fixed_R=None):
        self.fixed_T = torch.eye(4) if fixed_T is None else fixed_T
        self.fixed_R = self.fixed_T[:3, :3] if fixed_R is None else fixed_R
        self.trainable = trainable

    def triple(self):
        """What apply_trans_rot_new returns for this pose: (trainable capture or None, fixed T, fixed R)."""
        cap = None
        if self.trainable is not None:
            with torch.no_grad():
                cap = (self.trainable.obj_translation.detach(), self.trainable.rot_L(torch.eye(3, device=self.trainable.obj_translation.device)))
        return cap, self.fixed_T, self.fixed_R

    def compose(self, device=None):
        """-> (A12 [3,4], M [3,3]), float32 on `device`:  A = R_t A_f, b = R_t b_f + t, M = R_t fixed_R  (R_t = I, t = 0 without a
        trainable module).  Differentiable w.r.t. the module's parameters."""
        if device is None:
            device = self.trainable.obj_translation.device if self.trainable is not None else self.fixed_T.device
        T = self.fixed_T.to(device, torch.float32)
        R = self.fixed_R.to(device, torch.float32)
        A, b = T[:3, :3], T[:3, 3]
        if self.trainable is not None:
            Rt = self.trainable.rot_L(torch.eye(3, device=device))
            A, b, R = Rt @ A, Rt @ b + self.trainable.obj_translation.to(device), Rt @ R
        return torch.cat([A, b[:, None]], dim=1), R


class ComposedMotion:
    """A pose already in the kernels' form: compose() hands back the very tensors it was given (A12 [3,4], M [3,3] or None) -- static
    device buffers of a captured step (graph.GraphedTrainStep(motion=True)), or a caller's own composition.
    grad_out: a float32[21] device tensor the rasterizer's backward WRITES dL/dA12 [12], dL/dM9 [9] to -- the pose gradient without
    autograd, for a consumer that is a kernel itself (poses.PoseSequence.tail)."""

    def __init__(self, A12, M=None, grad_out=None):
        self.A12, self.M, self.grad_out = A12, M, grad_out

    def compose(self, device=None):
        return self.A12, self.M


def select_motion(accum_T_seq, accum_R_seq, image_name, during_training=False, trainable=None):
    """The frame rule of apply_trans_rot_new (/root/reference/scene/gaussian_model.py:939-986) with nothing mutated.
    accum_T_seq / accum_R_seq: {frame key: 4x4 / 3x3}.  -> ObjectMotion, or None where the reference applies nothing (a frame
    before the first key; during training also a frame past the last key, where the reference falls off its loop).
      not training: the pose OF the frame's key, else of the last key before the frame, else (past the end) of the last key
      training:     the pose of the last key strictly BEFORE the frame (identity if none), with `trainable` on top"""
    keys = sorted(accum_T_seq)
    if int(image_name) < int(keys[0]):
        return None
    prev_T, prev_R = torch.eye(4), torch.eye(3)
    for key in keys:
        if int(key) >= int(image_name):
            if during_training:
                return ObjectMotion(prev_T, trainable, prev_R)
            if int(key) == int(image_name):
                return ObjectMotion(accum_T_seq[key], None, accum_R_seq[key])
            return ObjectMotion(prev_T, None, prev_R)
        prev_T, prev_R = accum_T_seq[key], accum_R_seq[key]
    if during_training:
        return None
    return ObjectMotion(accum_T_seq[keys[-1]], None, accum_R_seq[keys[-1]])


def _split(A12):
    A12 = A12.reshape(3, 4)
    return A12[:, :3], A12[:, 3]


def move_points(xyz, A12, moved=None):
    """p' = A p + b for the rows of `moved` (bool / uint8 [N] or [N,1]; None = every row), the others as they are."""
    A, b = _split(A12.to(xyz.dtype))
    out = xyz @ A.t() + b
    return out if moved is None else torch.where(moved.reshape(-1, 1).bool(), out, xyz)


def unmove_points(xyz, A12, moved=None):
    """The inverse placement, p = A^-1 (p' - b): what reverse_trans_rot_new computes.  Only for comparisons -- a render that takes
    the motion as an input never needs it."""
    A, b = _split(A12.to(xyz.dtype))
    out = (xyz - b) @ torch.inverse(A).t()
    return out if moved is None else torch.where(moved.reshape(-1, 1).bool(), out, xyz)
