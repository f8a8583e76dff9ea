"""CPU: the object pose as an input of the render (egogaussian_amd.motion) against tests/golden/motion.npz -- the reference's own
GaussianModel.apply_trans_rot_new / reverse_trans_rot_new and ObjectMove run on CPU (tests/golden/make_golden_motion.py) -- and the C ABI
of the feature: symbols, sizes, argument errors before any device work.  No compute calls (there is no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "motion.npz"))
CASES = [str(c) for c in GOLD["cases"]]
BAR = 1e-6          # max-norm relative: float32 3x3 algebra in a different association order


class Move(torch.nn.Module):
    """ObjectMove-shaped (/root/reference/utils/geometry_utils.py:14-33): obj_translation [3], obj_rotation_6d [3,2], rot_L."""

    def __init__(self, t, r6):
        super().__init__()
        self.obj_translation = torch.nn.Parameter(torch.tensor(t))
        self.obj_rotation_6d = torch.nn.Parameter(torch.tensor(r6))

    def rot_L(self, L):
        a1, a2 = self.obj_rotation_6d[:, 0], self.obj_rotation_6d[:, 1]
        b1 = a1 / a1.norm()
        b2 = a2 - (b1 * a2).sum() * b1
        b2 = b2 / b2.norm()
        return torch.stack((b1, b2, torch.linalg.cross(b1, b2)), dim=-1) @ L


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _select(case):
    from egogaussian_amd import motion
    k = CASES.index(case)
    keys = [str(x) for x in GOLD["keys"]]
    T = {key: torch.tensor(GOLD["T_" + key]) for key in reversed(keys)}          # (unordered on purpose: the rule sorts)
    R = {key: torch.tensor(GOLD["R_" + key]) for key in keys}
    tom = Move(GOLD["obj_translation"], GOLD["obj_rotation_6d"])
    training = bool(GOLD["during_training"][k])
    return motion.select_motion(T, R, str(GOLD["image_names"][k]), training, tom), tom, training


def test_before_the_first_key_there_is_no_motion():
    m, _, _ = _select("before_first")
    assert m is None and not bool(GOLD["before_first_has_fixed"]) and not bool(GOLD["before_first_has_trainable"])
    assert np.array_equal(GOLD["before_first_moved_xyz"], GOLD["xyz"])


@pytest.mark.parametrize("case", [c for c in CASES if c != "before_first"])
def test_select_compose_move_reproduce_the_reference(case):
    from egogaussian_amd import motion
    m, tom, training = _select(case)
    assert m is not None
    cap, fixed_T, fixed_R = m.triple()
    assert (cap is not None) == bool(GOLD[case + "_has_trainable"]) == training
    assert np.array_equal(fixed_T.numpy(), GOLD[case + "_fixed_T"]) and np.array_equal(fixed_R.numpy(), GOLD[case + "_fixed_R"])
    if training:
        assert rel(cap[0], GOLD[case + "_cap_t"]) <= BAR and rel(cap[1], GOLD[case + "_cap_R"]) <= BAR
    xyz = torch.tensor(GOLD["xyz"], requires_grad=True)
    is_object = torch.tensor(GOLD["is_object"])
    moved = motion.exact_mask(is_object, int(GOLD["which_object"]))
    assert not bool(moved[0]) and 0 < int(moved.sum()) < moved.numel()
    A12, M = m.compose()
    out = motion.move_points(xyz, A12, moved)
    assert rel(out.detach(), GOLD[case + "_moved_xyz"]) <= BAR
    assert torch.equal(out.detach()[~moved], xyz.detach()[~moved])                 # unmoved rows: untouched
    (out * torch.tensor(GOLD["w"])).sum().backward()
    assert rel(xyz.grad, GOLD[case + "_g_xyz"]) <= BAR
    if training:
        assert rel(tom.obj_translation.grad, GOLD[case + "_g_translation"]) <= BAR
        assert rel(tom.obj_rotation_6d.grad, GOLD[case + "_g_rotation_6d"]) <= BAR
        assert rel(M.detach(), cap[1] @ fixed_R) <= BAR                             # M = R_t accum_R
    else:
        assert torch.equal(M, fixed_R)
    # nothing was mutated, so nothing needs reversing; the inverse exists for comparisons: the reference's round trip (asserted there at 1e-3)
    back = motion.unmove_points(out.detach(), A12.detach(), moved)
    assert float((back - xyz.detach()).abs().max()) <= 1e-5
    assert float(np.abs(GOLD[case + "_reversed_xyz"] - GOLD["xyz"]).max()) <= 1e-5


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "egs_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_the_motion_symbols_and_stays_6():
    from egogaussian_amd import lib
    L = lib.load()
    text, names = _declared_symbols()
    for n in ("egs_object_motion_scratch_bytes", "egs_object_move_points", "egs_object_move_points_backward"):
        assert n in names and n in lib.SIGNATURES and hasattr(L, n), n
    assert re.search(r"#define\s+EGS_ACT_OBJECT_MOTION\s+8\b", text) and "typedef struct egs_object_motion" in text
    assert lib.ACT_OBJECT_MOTION == 8 and L.egs_abi_version() == 6 == lib.ABI_VERSION
    # the struct starts with the rotation it extends: the same pointer serves both
    assert lib.ObjectMotion.rot.offset == 0 and lib.ObjectMotion.A12.offset == C.sizeof(lib.ObjectRotation)


def test_scratch_size_grows_with_the_rows():
    from egogaussian_amd import lib
    L = lib.load()
    assert L.egs_object_motion_scratch_bytes(0) == 0 and L.egs_object_motion_scratch_bytes(-3) == 0
    sizes = [L.egs_object_motion_scratch_bytes(p) for p in (1, 300, 12000, 500000)]
    assert sizes == sorted(sizes) and sizes[0] >= 21 * 4 and sizes[1] < sizes[2] < sizes[3]
    assert sizes[3] >= (500000 // 256) * 21 * 4


def test_motion_argument_errors_precede_device_work():
    from egogaussian_amd import lib
    L = lib.load()
    R = C.c_int64(-7)
    p, none = C.c_void_p(4096), None
    om = lib.ObjectMotion()                                                         # A12 == NULL
    call = lambda act, rot: L.egs_forward_geometry(10, 0, 1, p, p, none, none, p, p, 1.0, p, none, act, p, p, p, 64, 64, 1.0, 1.0, 0, p, p,
                                                   C.byref(R), none, rot, none, 0)
    assert call(lib.ACT_OBJECT_MOTION, lib.rot_pointer(om)) == -1                   # EGS_ERR_ARG (the parent: EGS_ERR_MODE, an unknown bit)
    om.A12, om.grad = 4096, 4096                                                    # a gradient without its scratch
    assert call(lib.ACT_OBJECT_MOTION, lib.rot_pointer(om)) == -1
    assert call(lib.ACT_OBJECT_MOTION, none) == -2                                  # the bit without a struct: no such mode
    assert call(16, none) == -2                                                     # still unknown
    # the stand-alone entry points
    assert L.egs_object_move_points(5, none, none, none, none, none, none) == -1 and L.egs_object_move_points(0, none, none, none, none, none, none) == 0
    assert L.egs_object_move_points(-1, p, p, none, none, p, none) == -1
    assert L.egs_object_move_points_backward(5, p, p, none, none, p, none, none, none, none) == -1      # nothing asked for
    assert L.egs_object_move_points_backward(5, p, p, none, none, p, none, p, none, none) == -1         # pose sums without scratch
    assert L.egs_object_move_points_backward(-1, p, p, none, none, p, p, none, none, none) == -1


def test_python_surface_refuses_cpu_tensors_and_both_arguments():
    from egogaussian_amd import fused
    from egogaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.object_move_points(torch.zeros(4, 3), torch.eye(4)[:3])
    rs = GaussianRasterizationSettings(image_height=32, image_width=32, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0,
                                       viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False)
    x, o = torch.zeros(4, 3), torch.ones(4, 1)
    with pytest.raises(Exception, match="mutually exclusive"):
        GaussianRasterizer(rs)(means3D=x, means2D=x, opacities=o, shs=torch.zeros(4, 1, 3), scales=torch.ones(4, 3), rotations=torch.ones(4, 4),
                               object_rotation=(torch.eye(3), None, 1.0), object_motion=(torch.eye(4)[:3], None, None, None, 1.0))
