"""GPU: rigid object motion inside the rasterizer (include/egs_raster.h egs_object_motion, egs_object_move_points).

What it replaces in the reference: gaussians.apply_trans_rot_new(...) before every render of a dynamic frame and
reverse_trans_rot_new(...) after it (/root/reference/scene/gaussian_model.py:939-986,1037-1060; trainers/coarse_obj_pose.py:229-239,
trainers/fine_all.py:88-116).  The COMPARISON path of these tests does what the reference does -- it renders a model whose positions
are the placed ones -- and the INSIDE path hands the pose to the rasterizer.  Shapes: N = 12 000 at 96 x 160 (47 workgroups, the last
one ragged), N = 300 for the reduction's edge (two workgroups, ragged); `is_object` [N,1] at 30 %, row 0 unselected; a pose well away
from the identity (0.4 rad about the scene centre, a translation of a tenth of the scene's extent)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float32).eps)
N, H, W = 12000, 96, 160
LEAVES = ("_features_dc", "_opacity", "_scaling", "_rotation")
# the colour inputs a render can have, each its own set of spherical-harmonics kernels: (stored degree, active degree, concatenated array)
VARIANTS = {"sh0": (0, 0, False),              # one coefficient: no spherical-harmonics launch
            "sh1": (1, 1, False),              # four coefficients: the generic kernels
            "sh3": (3, 3, False),              # sixteen, the two stored arrays: the 16-coefficient kernels, split
            "sh3_active0": (3, 0, False),      # sixteen stored, degree 0 active: the start of every training run
            "sh3_cat": (3, 3, True)}           # sixteen in one concatenated array (a model without the split hook)
KRUNS = 4                                      # comparison runs behind the run-to-run term


def _rot(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _pose(angle=0.4, t=(0.5, -0.3, 0.4), axis=(0.3, 1.0, 0.2), world=None):
    """4x4: a rotation about the scene centre (0, 0, 6) and a translation of ~0.7 (the scene spans ~6 x 4 x 8).
    world: the 4x4 that carries the scene into a general camera's world (tests/cameras.py): the same motion expressed there."""
    R, c = _rot(axis, angle), np.array([0.0, 0.0, 6.0])
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = c - R @ c + np.asarray(t)
    if world is not None:
        T = world @ T @ np.linalg.inv(world)
    return torch.tensor(T, dtype=torch.float32)


class Move(torch.nn.Module):
    """ObjectMove-shaped (/root/reference/utils/geometry_utils.py:14-33)."""

    def __init__(self, t, r6, device):
        super().__init__()
        self.obj_translation = torch.nn.Parameter(torch.tensor(t, dtype=torch.float32, device=device))
        self.obj_rotation_6d = torch.nn.Parameter(torch.tensor(r6, dtype=torch.float32, device=device))

    @staticmethod
    def matrix(r6):
        a1, a2 = r6[:, 0], r6[:, 1]
        b1 = a1 / a1.norm()
        b2 = a2 - (b1 * a2).sum() * b1
        b2 = b2 / b2.norm()
        return torch.stack((b1, b2, torch.linalg.cross(b1, b2)), dim=-1)

    def rot_L(self, L):
        return self.matrix(self.obj_rotation_6d) @ L


def _modifier(camera):
    """The scaling modifier every render of a general camera's runs is called with (1 on the orbit)."""
    from tests.cameras import CAMERAS
    return 1.0 if camera is None else CAMERAS[camera]["scale_modifier"]


def _scene(sh_degree=0, camera=None):
    return _scene_cached(sh_degree, camera)                              # (one cache entry however the call is spelt)


@functools.lru_cache(maxsize=None)
def _scene_cached(sh_degree, camera):
    """camera: None -> frame 30 of the orbit; a name of tests/cameras.py CAMERAS -> the scene carried into that camera's world, seen
    by it, rendered with its scale modifier, the pose expressed in that world."""
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd import motion
    teacher = make_scene(N, H, W, 3, sh_degree=sh_degree); teacher["log_scale"] += math.log(2.0)
    world = None
    if camera is not None:
        from tests.cameras import build_camera, world_positions
        cam_general, Q, shift, _ = build_camera(camera, H, W, device=DEV)
        teacher["xyz"] = world_positions(teacher["xyz"], Q, shift)
        world = np.eye(4); world[:3, :3] = Q; world[:3, 3] = shift
    student = perturb_student(teacher)
    gen = torch.Generator().manual_seed(4)
    is_obj = (torch.rand(N, 1, generator=gen) < 0.3).float().to(DEV)
    is_obj[0, 0] = 0.0                                                   # row 0 is background: only the covariance quirk touches it
    cam, bg = (make_camera(30, H, W, device=DEV) if camera is None else cam_general), torch.zeros(3, device=DEV)
    T = _pose(world=world).to(DEV)
    # the ground truth: the teacher with its object a little further along -- the loss then pulls the pose one way (no cancellation)
    T_gt = _pose(0.45, (0.62, -0.3, 0.4), world=world).to(DEV)
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=DEV, sh_degree=sh_degree, requires_grad=False)
        tpc._xyz = motion.move_points(tpc._xyz, T_gt[:3], is_obj == 1)
        gt = render(cam, tpc, Pipe, bg, scaling_modifier=_modifier(camera))["render"].clone()
    return student, is_obj, cam, bg, T, gt


def _model(variant=0, camera=None):
    """`variant`: a key of VARIANTS, or a degree (stored = active, the two stored arrays)."""
    from egogaussian_amd.scene_synth import SynthGaussians
    sh_degree, active, cat = VARIANTS.get(variant, (variant, variant, False))
    student, is_obj = _scene(sh_degree, camera)[:2]
    pc = SynthGaussians(student, device=DEV, sh_degree=sh_degree)
    pc._is_object = is_obj
    pc.active_sh_degree = active
    if cat:
        pc.get_features_split = lambda: None
    return pc


def _degree(variant):
    return VARIANTS.get(variant, (variant,))[0]


def _f64(t):
    return t.detach().double().cpu().numpy()


# ---- 1. moved points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, N])
def test_moved_points_against_float64(n):
    """|delta| <= 4 eps32 (|A||p| + |b|) per component -- three fused multiply-adds; unmoved rows and rows >= active_count bit-identical."""
    from egogaussian_amd import fused
    g = torch.Generator().manual_seed(n)
    p = (torch.randn(n, 3, generator=g) * 3).to(DEV)
    moved = (torch.rand(n, generator=g) < 0.3).to(DEV)
    A12 = _pose()[:3].to(DEV)
    live = n - 37
    for mask, count in ((moved, None), (None, None), (moved, torch.tensor([live], dtype=torch.int32, device=DEV))):
        out = fused.object_move_points(p, A12, mask, count)
        torch.cuda.synchronize()
        sel = (torch.ones(n, dtype=torch.bool, device=DEV) if mask is None else mask).clone()
        if count is not None:
            sel[live:] = False
        assert torch.equal(out[~sel], p[~sel])
        A, b, P64 = _f64(A12[:, :3]), _f64(A12[:, 3]), _f64(p)
        ref = P64 @ A.T + b
        bound = 4 * EPS * (np.abs(P64) @ np.abs(A).T + np.abs(b))
        s = sel.cpu().numpy()
        assert int(s.sum()) > 0 and np.all(np.abs(_f64(out) - ref)[s] <= bound[s])
        assert not torch.equal(out[sel], p[sel])


# ---- 4. the reduction on exact inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, N])
def test_pose_reduction_on_exact_inputs(n):
    """Each of the 12 sums within 12 eps32 sum|term_i| (one product rounding, the eight-deep float32 tree of a 256-row workgroup -- six
    shuffle levels + two through LDS --, a float64 finish); two calls give identical bits; an empty mask gives exact zeros."""
    from egogaussian_amd import fused
    gen = torch.Generator().manual_seed(7 + n)
    p = (torch.randn(n, 3, generator=gen) * 3).to(DEV)
    g = torch.randn(n, 3, generator=gen).to(DEV)
    moved = (torch.rand(n, generator=gen) < 0.3).to(DEV)
    A0 = _pose()[:3].to(DEV)
    res = []
    for rep in range(2):
        x, A12 = p.clone().requires_grad_(True), A0.clone().requires_grad_(True)
        fused.object_move_points(x, A12, moved).backward(g)
        torch.cuda.synchronize()
        res.append((x.grad.clone(), A12.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    m = moved.cpu().numpy()
    G, P64, A = _f64(g), _f64(p), _f64(A0[:, :3])
    terms = np.concatenate([G[m][:, :, None] * P64[m][:, None, :], G[m][:, :, None]], axis=2)      # [rows, 3, 4] in A12's layout
    assert np.all(np.abs(_f64(res[0][1]) - terms.sum(0)) <= 12 * EPS * np.abs(terms).sum(0))
    ref = np.where(m[:, None], G @ A, G)                                                            # A^T g
    bound = 4 * EPS * (np.abs(G) @ np.abs(A))
    assert np.all(np.abs(_f64(res[0][0]) - ref) <= np.where(m[:, None], bound, 0.0))
    x, A12 = p.clone().requires_grad_(True), A0.clone().requires_grad_(True)
    fused.object_move_points(x, A12, torch.zeros(n, dtype=torch.bool, device=DEV)).backward(g)
    assert torch.equal(A12.grad, torch.zeros_like(A12)) and torch.equal(x.grad, g)


# ---- the three paths of 2, 3, 5 ----------------------------------------------------------------------------------------------------
def _inside(variant, T, R, which_object=1, grad_A=True, grad_M=False, backward=True, camera=None):
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.motion import ComposedMotion
    _, _, cam, bg, _, gt = _scene(_degree(variant), camera)
    pc = _model(variant, camera)
    A12 = T[:3].clone().requires_grad_(grad_A)
    M = R.clone().requires_grad_(grad_M)
    xyz_ptr = pc._xyz.data_ptr()
    with torch.enable_grad() if backward else torch.no_grad():
        out = render(cam, pc, Pipe, bg, scaling_modifier=_modifier(camera), rot_cov=True, which_object=which_object, object_motion=ComposedMotion(A12, M))
        if backward:
            l1_ssim_loss(out["render"], gt, 0.2).backward()
    torch.cuda.synchronize()
    assert pc._xyz.data_ptr() == xyz_ptr
    return out, pc, A12, M


def _comparison(variant, T, R, which_object=1, cov_path=False, backward=True, camera=None):
    """What the reference does: the model's positions ARE the placed ones (here through egs_object_move_points, kept in the autograd graph so
    that the stand-alone backward turns g = xyz'.grad into the canonical gradient and the pose sums), same rotation, no motion."""
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd import fused, motion
    _, is_obj, cam, bg, _, gt = _scene(_degree(variant), camera)
    pc = _model(variant, camera)
    leaf = pc._xyz
    A12 = T[:3].clone().requires_grad_(True)
    M = R.clone().requires_grad_(cov_path)              # (a rotation that requires a gradient takes the covariance producer: egs_cov3d_backward's dL_dM9)
    keep = {}
    if cov_path:
        orig = pc.get_rotated_covariance_and_opacity

        def spy(*a, **k):
            cov, op = orig(*a, **k)
            cov.retain_grad(); keep["cov"] = cov
            return cov, op
        pc.get_rotated_covariance_and_opacity = spy
    with torch.enable_grad() if backward else torch.no_grad():
        placed = fused.object_move_points(leaf, A12, motion.exact_mask(is_obj, which_object))
        if backward:
            placed.retain_grad()
        pc._xyz = placed
        out = render(cam, pc, Pipe, bg, scaling_modifier=_modifier(camera), rot_cov=True, accum_R=M, which_object=which_object, during_training=False)
        if backward:
            fused.l1_ssim_loss(out["render"], gt, 0.2).backward()
    torch.cuda.synchronize()
    pc._xyz = leaf
    return out, pc, A12, M, placed, keep.get("cov")


def _runs(variant, camera=None):
    return _runs_cached(variant, camera)


@functools.lru_cache(maxsize=None)
def _runs_cached(variant, camera):
    """(the inside path, KRUNS runs of the comparison path) of one colour variant."""
    T = _scene(_degree(variant), camera)[4]
    R = T[:3, :3].contiguous()
    return _inside(variant, T, R, camera=camera), tuple(_comparison(variant, T, R, camera=camera) for _ in range(KRUNS))


def _pose_terms(g, p, moved):
    """float64 terms of dL/dA12, [rows, 3, 4]."""
    G, P64, m = _f64(g), _f64(p), moved.cpu().numpy()
    return np.concatenate([G[m][:, :, None] * P64[m][:, None, :], G[m][:, :, None]], axis=2)


# ---- 2. forward, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_is_the_render_of_the_placed_model_bit_for_bit(variant):
    (oa, *_), ((ob, *_), *_) = _runs(variant)
    assert torch.equal(oa["radii"], ob["radii"]) and int((oa["radii"] > 0).sum()) > 1000
    for k in ("render", "depth", "alpha"):
        assert torch.equal(oa[k], ob[k]), k


def test_forward_with_every_row_and_with_no_row_moved():
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    _, _, cam, bg, T, _ = _scene(0)
    R = T[:3, :3].contiguous()
    for which in (None, 7):                                              # every row (moved = NULL); a mask that selects nothing
        oa = _inside(0, T, R, which, backward=False)[0]
        ob = _comparison(0, T, R, which, backward=False)[0]
        assert torch.equal(oa["radii"], ob["radii"]) and int((oa["radii"] > 0).sum()) > 1000
        for k in ("render", "depth", "alpha"):
            assert torch.equal(oa[k], ob[k]), (which, k)
    with torch.no_grad():
        plain = render(cam, _model(0), Pipe, bg)                         # nothing selected == no motion (and no rotation) at all
    assert torch.equal(oa["radii"], plain["radii"]) and all(torch.equal(oa[k], plain[k]) for k in ("render", "depth", "alpha"))


def test_turned_covariances_need_the_raw_parameter_route():
    """A model without the raw-parameter hook would have its covariances turned by `accum_R` (the producers do not see the motion's M)
    while its positions follow the motion: an error, not a render of two poses."""
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.motion import ComposedMotion
    _, _, cam, bg, T, _ = _scene(0)
    pc = _model(0)
    pc.get_raw_parameters = lambda: None
    with pytest.raises(RuntimeError, match="get_raw_parameters"):
        render(cam, pc, Pipe, bg, rot_cov=True, which_object=1, object_motion=ComposedMotion(T[:3], T[:3, :3].contiguous()))


# ---- 3. position gradients, 5. pose gradient ---------------------------------------------------------------------------------------
def _check_position_gradient(variant, xyz_grad, label, camera=None):
    """`xyz_grad` (a render of `variant`'s model with the pose inside) against A^T g in float64, g = xyz'.grad of the comparison path's run 1.
    Per row and component:  |err| <= 4 eps32 (|A^T||g|)  [moved rows; 0 for the others]  +  4 x the row's OWN run-to-run term.

    Where this departs from the issue, and why.  The issue takes the run-to-run term as |g1 - g2| of two comparison runs, per component.
    That noise is the order of the blend's float32 atomic adds, one per (8x8 pixel wave, splat): a splat seen by one or two waves sums
    exactly, any other draws one of several roundings per run.  Two draws of one row often coincide where the third -- the run under test --
    does not, so |g1 - g2| alone is no envelope; it would ask bit-equality of rows that are not reproducible.  Taking the largest distance
    over the whole array instead would let every row off by the noisiest row's noise.  So each row is held to its own envelope:
      * the range of the row's component over KRUNS = 4 comparison runs, and at least
      * 8 eps32 |g_i|inf: a row whose four draws coincide is one with few partial sums (three or four waves) and no cancellation between
        them -- cancellation amplifies the reordering error and makes coincidence unlikely --, and reassociating four float32 terms of
        one sign moves their sum by at most 3 eps32 of it, per accumulator; the moments and the projection Jacobian mix the three
        components of the row, hence |g_i|inf and the factor 8 rather than 3.
    Both are pushed through |A^T| for the moved rows, as the noise of g is.  A share of the gradient that is missing on faint rows is an
    error of the order of |g_i| itself, seven decimal orders above this."""
    from egogaussian_amd import motion
    runs = _runs(variant, camera)[1]
    is_obj, T = _scene(_degree(variant), camera)[1], _scene(_degree(variant), camera)[4]
    m = motion.exact_mask(is_obj, 1).cpu().numpy()[:, None]
    A = _f64(T[:3, :3])
    g = np.stack([_f64(r[4].grad) for r in runs])
    g1 = g[0]
    ref = np.where(m, g1 @ A, g1)
    own = g.max(0) - g.min(0)
    floor = 8 * EPS * np.abs(g1).max(1, keepdims=True)
    derived = np.where(m, 4 * EPS * (np.abs(g1) @ np.abs(A)), 0.0)

    def through(x):
        return np.where(m, x @ np.abs(A), x)
    bound = derived + 4 * through(np.maximum(own, floor))
    err = np.abs(_f64(xyz_grad) - ref)
    as_written = derived + 4 * through(np.abs(g[0] - g[1]))
    no_floor = derived + 4 * through(own)
    worst = (err / np.maximum(bound, 1e-300)).max()
    print(f"  {label} {variant}: xyz max err {err.max():.3e}, worst err/bound {worst:.3f}; rows whose {KRUNS} draws coincide "
          f"{int((own == 0).all(1).sum())} of {len(own)}; rows over: the issue's |g1-g2| {int((err > as_written).any(1).sum())}, "
          f"range of {KRUNS} runs {int((err > no_floor).any(1).sum())}, with the floor {int((err > bound).any(1).sum())}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_position_and_pose_gradients(variant):
    """_xyz.grad of the inside path == A^T g (float64) within 4 eps32 |A^T||g| + the row's run-to-run term (_check_position_gradient);
    dL/dA12 against the stand-alone backward applied to the comparison path's g: |A - B1| <= 4 |B1 - B2| + 12 eps32 sum|term_i| (B1, B2:
    two runs of the comparison path, whose distance is the atomics-order noise of the blend; with more than one coefficient the
    spherical-harmonics launch finishes the gradient, one line per 64 rows -- a six-deep tree, inside the same constant).  Every other
    parameter gradient: 2e-5 max + 1e-9."""
    position_and_pose_gradients(variant)


def position_and_pose_gradients(variant, camera=None):
    """The body of the test above, on the orbit or at a general camera (tests/test_gpu_cameras.py: scale modifier other than 1)."""
    from egogaussian_amd import motion
    (oa, pa, Aa, _), ((o1, p1, A1, _, x1, _), (o2, p2, A2, _, x2, _), *_) = _runs(variant, camera)
    is_obj = _scene(_degree(variant), camera)[1]
    moved = motion.exact_mask(is_obj, 1)
    g1 = x1.grad
    # guard against a pose gradient that is a cancellation
    sums, abss = g1[moved].sum(0).abs().max(), g1[moved].abs().sum(0).max()
    print(f"{variant}: |sum g|inf {float(sums):.3e}  sum|g|inf {float(abss):.3e}  ratio {float(sums / abss):.3f}")
    assert float(sums) >= 0.05 * float(abss)
    _check_position_gradient(variant, pa._xyz.grad, "inside", camera)
    assert float(pa._xyz.grad[moved].abs().max()) > 0 and torch.equal(p1._xyz.grad[~moved], g1[~moved])
    for name in LEAVES + (("_features_rest",) if _degree(variant) else ()):
        ga, gb = getattr(pa, name).grad, getattr(p1, name).grad
        assert float((ga - gb).abs().max()) <= 2e-5 * float(gb.abs().max()) + 1e-9, name
    terms = _pose_terms(g1, p1._xyz, moved)
    spread = np.abs(_f64(A1.grad) - _f64(A2.grad))
    err = np.abs(_f64(Aa.grad) - _f64(A1.grad))
    print(f"  dL/dA12: inside vs stand-alone max {err.max():.3e}; spread of two comparison runs max {spread.max():.3e}; |dL/dA12| max {np.abs(_f64(A1.grad)).max():.3e}")
    assert np.all(err <= 4 * spread + 12 * EPS * np.abs(terms).sum(0))
    assert np.all(np.abs(_f64(A1.grad) - terms.sum(0)) <= 12 * EPS * np.abs(terms).sum(0))         # (the stand-alone sums are the float64 sums of g1)


def _rot_terms(pc, dcov, M, is_obj):
    """float64 terms of dL/dM = sum gL L0^T over the rotated rows (fused.object_selection: the exact rows + row 0, its gradient times the
    count), [rows, 3, 3], from the comparison path's dL/dcov."""
    from egogaussian_amd import covariance, fused
    sel, mult = fused.object_selection(is_obj, 1, is_obj.shape[0])
    L0 = covariance.scaling_rotation(torch.exp(pc._scaling.detach().double()), pc._rotation.detach().double())
    d = dcov.detach().double()
    Gs = torch.stack([d[:, 0], 0.5 * d[:, 1], 0.5 * d[:, 2], 0.5 * d[:, 1], d[:, 3], 0.5 * d[:, 4], 0.5 * d[:, 2], 0.5 * d[:, 4], d[:, 5]], 1).view(-1, 3, 3)
    gL = 2.0 * Gs @ (M.detach().double() @ L0)
    gL[0] *= float(mult)
    return (gL[:, :, None, :] * L0[:, None, :, :])[sel.bool()].cpu().numpy()                        # [rows, a, b, k]: summed over k and rows


def test_rotation_gradient_against_the_covariance_producer():
    """dL/dM9 of the inside path against egs_cov3d_backward's dL_dM9 on the cov3D_precomp path, same scheme as the pose gradient."""
    T = _scene(0)[4]
    R = T[:3, :3].contiguous()
    _, pa, _, Ma = _inside(0, T, R, grad_A=False, grad_M=True)
    _, p1, _, M1, _, cov1 = _comparison(0, T, R, cov_path=True)
    _, p2, _, M2, _, _ = _comparison(0, T, R, cov_path=True)
    t = _rot_terms(p1, cov1.grad, R, _scene(0)[1])
    spread = np.abs(_f64(M1.grad) - _f64(M2.grad))
    err = np.abs(_f64(Ma.grad) - _f64(M1.grad))
    print(f"dL/dM9: inside vs producer max {err.max():.3e}; spread of two producer runs max {spread.max():.3e}; |dL/dM9| max {np.abs(_f64(M1.grad)).max():.3e}")
    assert float(M1.grad.abs().max()) > 0
    assert np.all(err <= 4 * spread + 12 * EPS * np.abs(t).sum((0, 3)))


# ---- 6. through autograd to the 6-D pose -------------------------------------------------------------------------------------------
def test_trainable_pose_gradients_reach_the_six_d_parameters():
    """obj_translation.grad / obj_rotation_6d.grad of the inside path (raw-parameter path: the covariance producer does not run) against
    the all-torch path -- motion.move_points + the covariance producer with the trainable rotation -- run twice: |A - B1| <= 4 |B1 - B2| +
    the derived bounds of dL/dA12 and dL/dM9 carried through the float64 Jacobian of the composition."""
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd import motion, adapter
    _, is_obj, cam, bg, T, gt = _scene(0)
    Tf = _pose(0.25, (0.3, -0.2, 0.25)).to(DEV)                          # the accumulated pose; the trainable one sits on top of it
    t0, r6 = [0.15, -0.08, 0.1], (_rot((0.2, 0.4, 1.0), 0.18)[:, :2] + 0.03).tolist()
    moved = motion.exact_mask(is_obj, 1)
    # inside: the loss's gradient handed over as a tensor, and formed by the blend itself (egs_backward_lossgrad writes the pose gradient too)
    def inside(**loss_kw):
        pa = adapter.attach(_model(0), optimizer=False)
        tom = Move(t0, r6, DEV)
        pa.trainable_object_move = tom
        calls = pa.build_covariance_from_scaling_rotation_w_rot.calls
        out = render(cam, pa, Pipe, bg, rot_cov=True, which_object=1, during_training=True, object_motion=motion.ObjectMotion(Tf, tom))
        l1_ssim_loss(out["render"], gt, 0.2, **loss_kw).backward()
        torch.cuda.synchronize()
        assert pa.build_covariance_from_scaling_rotation_w_rot.calls == calls and int((out["radii"] > 0).sum()) > 1000
        return tom
    toma, toma_blend = inside(), inside(raster_prologue=True, raster_lossgrad=True)
    # all torch, twice
    res = []
    for rep in range(2):
        pb = _model(0)
        tomb = Move(t0, r6, DEV)
        pb.trainable_object_move = tomb
        leaf = pb._xyz
        A12, _ = motion.ObjectMotion(Tf, tomb).compose(DEV)
        A12.retain_grad()
        keep = {}
        orig = pb.get_rotated_covariance_and_opacity

        def spy(*a, _orig=orig, _keep=keep, **k):
            cov, op = _orig(*a, **k)
            cov.retain_grad(); _keep["cov"] = cov
            return cov, op
        pb.get_rotated_covariance_and_opacity = spy
        placed = motion.move_points(leaf, A12, moved)
        placed.retain_grad()
        pb._xyz = placed
        ob = render(cam, pb, Pipe, bg, rot_cov=True, accum_R=Tf[:3, :3].contiguous(), which_object=1, during_training=True)
        l1_ssim_loss(ob["render"], gt, 0.2).backward()
        torch.cuda.synchronize()
        pb._xyz = leaf
        res.append((tomb, placed.grad, keep["cov"].grad, pb))
    (b1, g1, dcov1, pb1), (b2, _, _, _) = res
    # derived term: the float64 bounds of the 21 sums, through |d(A12, M)/d(t, r6)|
    M_now = (Move.matrix(toma.obj_rotation_6d.detach()) @ Tf[:3, :3]).contiguous()
    eA = 12 * EPS * np.abs(_pose_terms(g1, pb1._xyz, moved)).sum(0)
    eM = 12 * EPS * np.abs(_rot_terms(pb1, dcov1, M_now, is_obj)).sum((0, 3))
    e21 = torch.tensor(np.concatenate([eA.reshape(-1), eM.reshape(-1)]))

    def composed(t, r):
        Rt = Move.matrix(r)
        Tf64 = Tf.double().cpu()
        return torch.cat([torch.cat([Rt @ Tf64[:3, :3], (Rt @ Tf64[:3, 3] + t)[:, None]], 1).reshape(-1), (Rt @ Tf64[:3, :3]).reshape(-1)])
    Jt, Jr = torch.autograd.functional.jacobian(composed, (toma.obj_translation.detach().double().cpu(), toma.obj_rotation_6d.detach().double().cpu()))
    for name, J in (("obj_translation", Jt), ("obj_rotation_6d", Jr)):
        a, ab, x1, x2 = (_f64(getattr(m, name).grad) for m in (toma, toma_blend, b1, b2))
        derived = (J.abs() * e21.view(21, *([1] * (J.dim() - 1)))).sum(0).numpy()
        print(f"{name}: inside vs torch max {np.abs(a - x1).max():.3e}, with the loss gradient formed in the blend {np.abs(ab - x1).max():.3e}; "
              f"spread of two torch runs max {np.abs(x1 - x2).max():.3e}; |grad| max {np.abs(x1).max():.3e}; derived max {derived.max():.3e}")
        assert np.abs(x1).max() > 0
        assert np.all(np.abs(a - x1) <= 4 * np.abs(x1 - x2) + derived), name
        assert np.all(np.abs(ab - x1) <= 4 * np.abs(x1 - x2) + derived), name + " (loss gradient formed in the blend)"


# ---- 7. fused Adam under motion ----------------------------------------------------------------------------------------------------
def _groups(pc):
    g = [{"params": [pc._xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [pc._features_dc], "lr": 2.5e-3, "name": "f_dc"},
         {"params": [pc._opacity], "lr": 0.05, "name": "opacity"}, {"params": [pc._scaling], "lr": 5e-3, "name": "scaling"},
         {"params": [pc._rotation], "lr": 1e-3, "name": "rotation"}]
    if pc._features_rest.numel():
        g.append({"params": [pc._features_rest], "lr": 2.5e-3 / 20, "name": "f_rest"})
    return g


@pytest.mark.parametrize("variant", ["sh0", "sh3"])
def test_fused_adam_steps_the_canonical_positions(variant):
    """render(object_motion=m, optimizer=FusedAdam(capturable=True)) for three iterations: the backward steps `_xyz` with A^T dL/dp' itself
    (sh_degree 3: the spherical-harmonics launch does) AND writes the gradients; a twin on copies steps with those gradients through the
    stand-alone kernel (egs_adam_step_capturable).  The bar of test_gpu_fused_adam.py for this comparison: equal bit for bit.  `_xyz`
    keeps its address throughout."""
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.motion import ObjectMotion
    _, _, cam, bg, T, gt = _scene(_degree(variant))
    pa, pb = _model(variant), _model(variant)
    oa = FusedAdam(_groups(pa), lr=0.0, eps=1e-15, capturable=True)
    ob = FusedAdam(_groups(pb), lr=0.0, eps=1e-15, capturable=True)
    leaves = ("_xyz",) + LEAVES + (("_features_rest",) if _degree(variant) else ())
    real_make = oa.make_sink

    def keeping(**kw):
        sink = real_make(**kw)
        sink.keep_grads = True
        keeping.last = sink
        return sink
    oa.make_sink = keeping
    ptr = pa._xyz.data_ptr()
    for it in range(3):
        m = ObjectMotion(_pose(0.4 + 0.05 * it, (0.5, -0.3 + 0.1 * it, 0.4)).to(DEV))
        for a in leaves:
            with torch.no_grad():
                getattr(pb, a).copy_(getattr(pa, a))
        before = pa._xyz.detach().clone()
        out = render(cam, pa, Pipe, bg, rot_cov=True, which_object=1, optimizer=oa, object_motion=m)
        l1_ssim_loss(out["render"], gt, 0.2).backward()
        assert 0 in keeping.last.owned and not torch.equal(before, pa._xyz.detach())
        if it == 0:
            # the launch that steps `_xyz` also computes A^T g: iteration 0 is the pose and the model of _runs, so the gradient it kept
            # answers to the comparison path's float64 A^T g like the one of the launch that only writes it
            _check_position_gradient(variant, pa._xyz.grad, "stepping launch")
        for a in leaves:
            getattr(pb, a).grad = getattr(pa, a).grad.clone()
        oa.step(); oa.zero_grad(set_to_none=True)
        ob.step(); ob.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        assert pa._xyz.data_ptr() == ptr
        for a in leaves:
            assert torch.equal(getattr(pa, a).detach(), getattr(pb, a).detach()), f"iteration {it}: {a} differs"
        assert float(oa.state[pa._xyz]["step"]) == float(ob.state[pb._xyz]["step"]) == it + 1


# ---- 8. graph ----------------------------------------------------------------------------------------------------------------------
def test_graphed_step_with_the_motion_inside():
    """GraphedTrainStep(dynamic=True, motion=True): one captured step replayed on three further frames with their own accum_T against the
    eager loop on the same frames (the bar of test_double_buffered_graph_step_matches_single_buffered); and a replay with accum_T =
    accum_R = identity renders the image of dynamic=False bit for bit."""
    from egogaussian_amd.scene_synth import make_camera, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    from egogaussian_amd.motion import ObjectMotion
    _, _, _, bg, _, gt = _scene(0)
    cams = [make_camera(k, H, W, device=DEV) for k in (30, 60, 90, 120)]
    Ts = [_pose(0.4 + 0.03 * k, (0.5 - 0.05 * k, -0.3, 0.4 + 0.04 * k)).to(DEV) for k in range(4)]
    pa, pb = _model(0), _model(0)
    oa = FusedAdam(_groups(pa), lr=0.0, eps=1e-15, capturable=True)
    ob = FusedAdam(_groups(pb), lr=0.0, eps=1e-15, capturable=True)
    ptr = pa._xyz.data_ptr()
    step = GraphedTrainStep(pa, oa, bg, 0.2, dynamic=True, motion=True).capture(cams[0], gt, warmup=1, accum_R=Ts[0][:3, :3], accum_T=Ts[0],
                                                                               capacity_margin=2.0)
    la = []
    for k in (1, 2, 3):
        frame = pack_frame(cams[k], gt, Ts[k][:3, :3], None, Ts[k])
        la.append(float(step(frame) if k != 2 else step(cams[k], gt, accum_R=Ts[k][:3, :3], accum_T=Ts[k])))
    torch.cuda.synchronize()
    assert step.ok() and pa._xyz.data_ptr() == ptr and float(oa.state[pa._xyz]["step"]) == 4.0
    lb = []
    for k in range(4):
        out = render(cams[k], pb, Pipe, bg, rot_cov=True, which_object=1, optimizer=ob, object_motion=ObjectMotion(Ts[k]))
        loss = l1_ssim_loss(out["render"], gt, 0.2)
        loss.backward()
        ob.step(); ob.zero_grad(set_to_none=True)
        lb.append(float(loss))
    torch.cuda.synchronize()
    assert all(abs(u - v) <= 2e-3 * abs(u) for u, v in zip(lb[1:], la)), (lb, la)
    for a in ("_xyz",) + LEAVES:
        u, v = getattr(pa, a).detach(), getattr(pb, a).detach()
        assert float((u - v).abs().mean()) <= 2e-4 * float(u.abs().mean()) + 1e-7, a
    # identity pose == no pose (learning rates zero: the captured steps leave the parameters alone, so both graphs render the same model)
    imgs = []
    for dyn in (True, False):
        pc = _model(0)
        groups = _groups(pc)
        for g in groups:
            g["lr"] = 0.0
        opt = FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True)
        st = GraphedTrainStep(pc, opt, bg, 0.2, dynamic=dyn, motion=dyn).capture(cams[0], gt, warmup=1)
        st(cams[1], gt, **(dict(accum_R=torch.eye(3, device=DEV), accum_T=torch.eye(4, device=DEV)) if dyn else {}))
        torch.cuda.synchronize()
        imgs.append(st.image.clone())
    assert torch.equal(imgs[0], imgs[1])
