"""GPU: the object stages' loss (image + alpha against the object mask; include/egs_raster.h egs_object_loss) -- the loss kernels alone
against the torch mirror in float64, through the rasterizer against the reference's captured pose step and against its own backward
launch, and inside the captured training step, with a fixed and with a trainable pose."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
LAM = 0.2
UP = 3.0                                       # the upstream scalar of the backward: (UP * loss).backward()

# ---- 1. the loss kernels alone ------------------------------------------------------------------------------------------------------
SHAPES = [(48, 80), (37, 53), (7, 9)]          # whole tiles and strips; ragged tiles and strips; narrower than the 11-tap window
WEIGHTS = [(0.0, 0.5), (0.3, 0.2), (0.0, 0.0)]           # (lambda_l1_alpha, lambda_l2_alpha): the coarse default, both terms, none
CASES = [(s, gated, w) for s in SHAPES for gated in (False, True) for w in WEIGHTS]
IDS = [f"{s[0]}x{s[1]}-{'gate' if gated else 'plain'}-{w[0]}-{w[1]}" for s, gated, w in CASES]


def _lambda_image(w):
    return 1.0 if w == (0.0, 0.0) else 0.7


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    """image, gt [3,H,W]; alpha in [0,1), binary mask, binary gate [H,W]; `tie`: a quarter of the pixels has alpha = mask = 0 exactly (what
    every pixel no splat reaches looks like); a patch in the middle has mask = 1 and alpha >= 0.5."""
    gen = torch.Generator().manual_seed(1000 * H + W)
    img = torch.rand(3, H, W, generator=gen)
    gt = (img + 0.1 * torch.randn(3, H, W, generator=gen)).clamp(0, 1)
    alpha = torch.rand(H, W, generator=gen)
    mask = (torch.rand(H, W, generator=gen) < 0.45).float()
    patch = torch.zeros(H, W, dtype=torch.bool)
    patch[H // 3:2 * H // 3 + 1, W // 3:2 * W // 3 + 1] = True
    mask[patch] = 1.0
    alpha[patch] = 0.5 + 0.499 * alpha[patch]
    outside = torch.nonzero(~patch.reshape(-1)).reshape(-1)
    pick = outside[torch.randperm(outside.numel(), generator=gen)[:(H * W + 3) // 4]]
    tie = torch.zeros(H * W, dtype=torch.bool)
    tie[pick] = True
    tie = tie.reshape(H, W)
    alpha[tie] = 0.0
    mask[tie] = 0.0
    gate = (torch.rand(H, W, generator=gen) < 0.8).float()
    assert float(tie.float().mean()) >= 0.2 and bool((alpha[patch] >= 0.5).all()) and bool((alpha < 1).all()) and set(mask.unique().tolist()) <= {0.0, 1.0}
    return img, gt, alpha, mask, gate, tie


@functools.lru_cache(maxsize=None)
def _reference(H, W, gated, w):
    """The torch mirror in float64 with the reference's two hooks: value, the three terms, both gradients.  Computed once per case."""
    from egogaussian_amd.losses import object_stage_loss, training_loss, l1_loss, l2_loss
    img, gt, alpha, mask, gate, _ = _inputs(H, W)
    x, a = img.double().requires_grad_(True), alpha.double().requires_grad_(True)
    if gated:
        x.register_hook(lambda g: g * gate.double())
        a.register_hook(lambda g: g * gate.double())
    l = object_stage_loss(x, a, gt.double(), mask.double(), LAM, _lambda_image(w), w[0], w[1])
    (UP * l).backward()
    terms = (float(training_loss(x.detach(), gt.double() * mask.double(), LAM)), float(l1_loss(mask.double(), alpha.double())),
             float(l2_loss(mask.double(), alpha.double())))
    return float(l), terms, x.grad, a.grad


def _run(H, W, gated, w, defer=False):
    from egogaussian_amd.fused import object_stage_loss
    img, gt, alpha, mask, gate, _ = _inputs(H, W)
    x, a = img.to(DEV).requires_grad_(True), alpha.to(DEV).requires_grad_(True)
    terms, run = torch.full((3,), -1.0, device=DEV), torch.full((1,), 0.25, device=DEV)
    l = object_stage_loss(x, a, gt.to(DEV), mask.to(DEV), LAM, _lambda_image(w), w[0], w[1], grad_gate=gate.to(DEV) if gated else None,
                          running_sum=run, terms=terms, defer_value=defer)
    (UP * l).backward()
    torch.cuda.synchronize()
    return dict(loss=l.detach().cpu(), terms=terms.cpu(), run=run.cpu(), gx=x.grad.cpu(), ga=a.grad.cpu())


@functools.lru_cache(maxsize=None)
def _kernel(H, W, gated, w):
    return _run(H, W, gated, w), _run(H, W, gated, w), _run(H, W, gated, w, defer=True)


@pytest.mark.parametrize("shape,gated,w", CASES, ids=IDS)
def test_value_and_terms_against_float64(shape, gated, w):
    """|l - l64| <= 1e-5 max(1, |l64|) for the value and each of the three terms (the bar of test_fused_loss_on_flat_and_small_variance_images),
    assembled right away (the 1024-thread finishing kernel) and deferred to the backward launch (one wave)."""
    l64, t64, _, _ = _reference(*shape, gated, w)
    for r in (_kernel(*shape, gated, w)[0], _kernel(*shape, gated, w)[2]):
        print("value", float(r["loss"]), l64, "terms", r["terms"].tolist(), t64)
        assert abs(float(r["loss"]) - l64) <= 1e-5 * max(1.0, abs(l64))
        for k in range(3):
            assert abs(float(r["terms"][k]) - t64[k]) <= 1e-5 * max(1.0, abs(t64[k])), k
        assert abs(float(r["run"]) - 0.25 - float(r["loss"])) <= 1e-6


@pytest.mark.parametrize("shape,gated,w", CASES, ids=IDS)
def test_image_gradient_against_float64(shape, gated, w):
    """1e-4 max-norm relative; the unit is never less than one pixel's share of the L1 term (here lambda_image * UP * 0.8 / n)."""
    H, W = shape
    g64 = _reference(H, W, gated, w)[2]
    g = _kernel(H, W, gated, w)[0]["gx"].double()
    scale = max(float(g64.abs().max()), _lambda_image(w) * UP * (1.0 - LAM) / (3 * H * W))
    print("image gradient", float((g - g64).abs().max()) / scale)
    assert float((g - g64).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize("shape,gated,w", CASES, ids=IDS)
def test_alpha_gradient_against_float64_and_exact_zero_on_ties(shape, gated, w):
    """Per pixel |g - g64| <= 8 eps32 (|l1a| + 2 |l2a|) |up| / (H W): the expression is pointwise and alpha - m is exact or within half an
    ulp for m in {0, 1}.  Where alpha = m (every pixel no splat reached: alpha = 0 on a mask of 0) the gradient is EXACTLY 0, as torch's."""
    H, W = shape
    g64 = _reference(H, W, gated, w)[3]
    g = _kernel(H, W, gated, w)[0]["ga"].double()
    tie = _inputs(H, W)[5]
    bound = 8 * EPS32 * (abs(w[0]) + 2 * abs(w[1])) * abs(UP) / (H * W)
    print("alpha gradient", float((g - g64).abs().max()), "bound", bound)
    assert g.shape == g64.shape and float((g - g64).abs().max()) <= bound
    assert float(g[tie].abs().max()) == 0.0 and float(g64[tie].abs().max()) == 0.0
    if w != (0.0, 0.0):
        assert float(g.abs().max()) > 0


@pytest.mark.parametrize("shape,gated,w", CASES, ids=IDS)
def test_two_runs_are_bit_identical(shape, gated, w):
    a, b, _ = _kernel(*shape, gated, w)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("defer", [False, True], ids=["value right away", "deferred value"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_without_alpha_weights_it_is_the_image_loss_bit_for_bit(shape, gated, defer):
    from egogaussian_amd.fused import l1_ssim_loss
    H, W = shape
    img, gt, alpha, mask, gate, _ = _inputs(H, W)
    r = _run(H, W, gated, (0.0, 0.0), defer=defer)
    x = img.to(DEV).requires_grad_(True)
    l = l1_ssim_loss(x, gt.to(DEV) * mask.to(DEV), LAM, grad_gate=gate.to(DEV) if gated else None, defer_value=defer)
    (UP * l).backward()
    torch.cuda.synchronize()
    assert torch.equal(l.detach().cpu(), r["loss"]) and torch.equal(x.grad.cpu(), r["gx"])
    assert float(r["ga"].abs().max()) == 0.0


# ---- 2. through the rasterizer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossgrad", [False, True], ids=["backward launch", "in the blend"])
def test_pose_training_step_with_the_fused_object_loss_matches_reference(lossgrad):
    """test_pose_training_step_through_hip_matches_reference_end_to_end (path `producer`) with fused.object_stage_loss in place of the image loss
    + five torch launches each way + the hook on alpha: the same fixture keys, the same bars (loss 1e-5, every gradient and pose_g_rot6d 2e-4)."""
    from tests.test_golden_host import load, _model_from_train, _cam_from_train, _object_move
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.fused import object_stage_loss
    g = load("boundary_train.npz")
    pc = _model_from_train(g, "pose_", DEV, fused=True)
    pc.rotate_in_rasterizer = False
    pc.trainable_object_move = tom = _object_move(g, DEV)
    cam = _cam_from_train(g, "pose_", DEV)
    out = render(cam, pc, Pipe, torch.zeros(3, device=DEV), rot_cov=True, accum_R=torch.tensor(g["pose_accum_R"], device=DEV), which_object=1,
                 during_training=True)
    lam, l1a, l2a = [float(x) for x in g["pose_lambdas"]]
    hand = torch.tensor(g["pose_hand"], device=DEV)
    loss = object_stage_loss(out["render"], out["alpha"], torch.tensor(g["pose_gt"], device=DEV), torch.tensor(g["pose_obj_mask"], device=DEV), lam,
                             1.0, l1a, l2a, grad_gate=(1 - hand)[0], raster_prologue=lossgrad, raster_lossgrad=lossgrad)
    loss.backward()
    close = lambda a, b, tol=1e-4: np.abs(a.detach().cpu().numpy() - b).max() <= tol * max(np.abs(b).max(), 1e-12)
    assert np.array_equal(out["radii"].cpu().numpy(), g["pose_radii"])
    assert close(out["render"], g["pose_render"]) and close(out["alpha"], g["pose_alpha"]) and close(out["depth"], g["pose_depth"])
    print("loss", float(loss.detach()), float(g["pose_loss"]))
    assert abs(float(loss.detach()) - float(g["pose_loss"])) <= 1e-5 * abs(float(g["pose_loss"]))
    for p, name in ((pc._xyz, "g_xyz"), (pc._features_dc, "g_features_dc"), (pc._scaling, "g_scaling"), (pc._rotation, "g_rotation"),
                    (pc._opacity, "g_opacity"), (out["viewspace_points"], "g_viewspace")):
        assert close(p.grad, g["pose_" + name], 2e-4), name
    assert tom.obj_rotation_6d.grad is not None and float(np.abs(g["pose_g_rot6d"]).max()) > 0
    assert close(tom.obj_rotation_6d.grad, g["pose_g_rot6d"], 2e-4)


W_OBJ = dict(lambda_image=0.7, lambda_l1_alpha=0.3, lambda_l2_alpha=0.2)


def _box_mask(H, W):
    m = torch.zeros(H, W)
    m[H // 4:3 * H // 4, W // 4:3 * W // 4] = 1.0                    # a quarter of the frame
    return m.to(DEV)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "hand-mask gate"])
@pytest.mark.parametrize("N,H,W", [(3000, 48, 80), (6000, 135, 250)], ids=["48x80", "ragged 135x250"])
def test_gradients_formed_in_the_blend_match_the_backward_launch(N, H, W, gated):
    """raster_lossgrad=True: no loss-backward launch, the blend (k_render_backward<2, true>) forms dL/dimage and dL/dalpha itself.  Loss, running
    sum and terms are equal; every parameter gradient is within 2e-5 of its array's maximum (the order of the accumulator atomics) -- the bar
    of test_loss_gradient_inside_the_blend_matches_the_loss_backward_launch."""
    _blend_against_launch(N, H, W, gated)


def test_gradients_formed_in_the_blend_with_split_harmonics():
    """The same on a model of 16 coefficients handed over as its two stored arrays: the spherical-harmonics launches follow the preprocess
    backward of the object stages' route (5 leaves + features_rest)."""
    _blend_against_launch(3000, 48, 80, False, sh_degree=3)


def _blend_against_launch(N, H, W, gated, **model):
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import object_stage_loss
    teacher = make_scene(N, H, W, 0, sh_degree=model.get("sh_degree", 0)); teacher["log_scale"] += math.log(2.0)
    cam = make_camera(7, H, W, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        gt = render(cam, SynthGaussians(teacher, device=DEV, requires_grad=False, **model), Pipe, bg)["render"].clone()
    mask = _box_mask(H, W)
    gate = (torch.rand((H, W), generator=torch.Generator().manual_seed(3)) < 0.8).float().to(DEV) if gated else None
    res = []
    for mode in (False, True, True):
        pc = SynthGaussians(perturb_student(teacher), device=DEV, **model)
        run, terms = torch.full((1,), 0.25, device=DEV), torch.zeros(3, device=DEV)
        out = render(cam, pc, Pipe, bg)
        loss = object_stage_loss(out["render"], out["alpha"], gt, mask, LAM, grad_gate=gate, running_sum=run, terms=terms, defer_value=True,
                                 raster_prologue=True, raster_lossgrad=mode, **W_OBJ)
        loss.backward()
        torch.cuda.synchronize()
        res.append(([p.grad.clone() for p in pc.parameters() if p.grad is not None], float(loss.detach()), float(run), terms.cpu()))
    ref = res[0]
    assert len(ref[0]) >= (6 if model.get("sh_degree") else 5) and math.isfinite(ref[1]) and ref[1] > 0 and float(ref[3][1]) > 0 and float(ref[3][2]) > 0
    for got in res[1:]:
        assert got[1] == ref[1] and got[2] == ref[2] and torch.equal(got[3], ref[3]) and abs(ref[2] - 0.25 - ref[1]) < 1e-6
        assert len(got[0]) == len(ref[0])
        for a, b in zip(got[0], ref[0]):
            scale = float(b.abs().max()) + 1e-30
            print("in-blend vs launch", float((a - b).abs().max()) / scale)
            assert float((a - b).abs().max()) <= 2e-5 * scale


def test_object_loss_in_the_blend_on_a_frame_with_no_instance():
    """R == 0: no blend launch; the deferred value with its alpha terms (alpha = 0 everywhere) is still assembled and every gradient is zero."""
    from egogaussian_amd.scene_synth import make_scene, make_camera, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import object_stage_loss
    N, H, W = 2000, 64, 96
    scene = make_scene(N, H, W, 0)
    cam = make_camera(0, H, W, device=DEV)
    bg = torch.tensor([0.3, 0.1, 0.2], device=DEV)
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = _box_mask(H, W)
    vals = []
    for mode in (False, True):
        pc = SynthGaussians(scene, device=DEV)
        with torch.no_grad():
            pc._xyz += 1.0e4
        out = render(cam, pc, Pipe, bg)
        assert int(out["radii"].max()) == 0
        run, terms = torch.zeros(1, device=DEV), torch.zeros(3, device=DEV)
        loss = object_stage_loss(out["render"], out["alpha"], gt, mask, LAM, running_sum=run, terms=terms, defer_value=True, raster_prologue=True,
                                 raster_lossgrad=mode, **W_OBJ)
        loss.backward()
        torch.cuda.synchronize()
        assert all(float(p.grad.abs().max()) == 0.0 for p in pc.parameters() if p.grad is not None)
        vals.append((float(loss.detach()), float(run), terms.cpu().tolist()))
    assert vals[0] == vals[1] and vals[0][0] > 0 and vals[0][0] == vals[0][1]
    assert abs(vals[0][2][1] - float(mask.mean())) <= 1e-6 and abs(vals[0][2][2] - float(mask.mean())) <= 1e-6      # alpha = 0: both terms are mean(mask)


def test_object_loss_in_the_blend_refuses_every_other_gradient_contribution():
    """With raster_lossgrad=True BOTH gradient tensors the loss hands to the rasterizer are uninitialised and unread: a second consumer of
    alpha, a hook on alpha, a second consumer of the image, or any gradient into the depth output would be dropped silently -- refused
    instead; the plain case runs."""
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import object_stage_loss
    N, H, W = 3000, 48, 80
    teacher = make_scene(N, H, W, 0); teacher["log_scale"] += math.log(2.0)
    cam = make_camera(7, H, W, device=DEV)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    gt = torch.rand((3, H, W), device=DEV)
    mask = _box_mask(H, W)

    def step(extra):
        pc = SynthGaussians(perturb_student(teacher), device=DEV)
        out = render(cam, pc, Pipe, bg)
        loss = object_stage_loss(out["render"], out["alpha"], gt, mask, LAM, defer_value=True, raster_prologue=True, raster_lossgrad=True, **W_OBJ)
        if extra == "second consumer of alpha":
            loss = loss + 0.1 * out["alpha"].mean()
        elif extra == "hook on alpha":
            out["alpha"].register_hook(lambda g: g * 0.5)
        elif extra == "second consumer of the image":
            loss = loss + 0.1 * out["render"].mean()
        elif extra == "gradient into depth":
            loss = loss + 0.1 * out["depth"].mean()
        loss.backward()
        torch.cuda.synchronize()
        return pc

    pc = step(None)
    assert all(torch.isfinite(p.grad).all() for p in pc.parameters() if p.grad is not None)
    for extra in ("second consumer of alpha", "hook on alpha", "second consumer of the image", "gradient into depth"):
        with pytest.raises(RuntimeError, match="another gradient contribution"):
            step(extra)


# ---- 3. the captured step -----------------------------------------------------------------------------------------------------------
def _frames():
    """The scene of test_gpu_motion.py (N = 12 000 at 96 x 160, `is_object` at 30 %): four cameras, each with its own accumulated pose; one
    ground truth, an object mask of a quarter of the frame, a hand-mask gate."""
    from tests.test_gpu_motion import _scene, _pose, H, W
    from egogaussian_amd.scene_synth import make_camera
    _, _, _, bg, _, gt = _scene(0)
    cams = [make_camera(k, H, W, device=DEV) for k in (30, 60, 90, 120)]
    Ts = [_pose(0.4 + 0.03 * k, (0.5 - 0.05 * k, -0.3, 0.4 + 0.04 * k)).to(DEV) for k in range(4)]
    gate = (torch.rand((H, W), generator=torch.Generator().manual_seed(5)) < 0.85).float().to(DEV)
    return cams, Ts, bg, gt, _box_mask(H, W), gate


def _eager_step(pc, opt, cam, T, bg, gt, mask, gate, pose=None):
    """The route of the commit before: render with alpha, the torch mirror of the loss with the reference's two hooks, backward, step."""
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.losses import object_stage_loss
    from egogaussian_amd.motion import ObjectMotion
    out = render(cam, pc, Pipe, bg, rot_cov=True, which_object=1, optimizer=opt, object_motion=ObjectMotion(T, pose, T[:3, :3]))
    out["render"].register_hook(lambda g: g * gate)
    out["alpha"].register_hook(lambda g: g * gate)
    loss = object_stage_loss(out["render"], out["alpha"], gt, mask, LAM, **W_OBJ)
    loss.backward()
    opt.step(); opt.zero_grad(set_to_none=True)
    return float(loss)


def test_graphed_step_with_the_object_loss_and_a_fixed_pose():
    """GraphedTrainStep(dynamic=True, motion=True, gated=True, object_loss=...): captured on one frame, replayed on three further ones, against
    the eager loop -- the bars of test_graphed_step_with_the_motion_inside (loss 2e-3, parameters 2e-4 mean-relative + 1e-7); `_xyz` keeps its address."""
    from tests.test_gpu_motion import _model, _groups, LEAVES
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    cams, Ts, bg, gt, mask, gate = _frames()
    pa, pb = _model(0), _model(0)
    oa = FusedAdam(_groups(pa), lr=0.0, eps=1e-15, capturable=True)
    ob = FusedAdam(_groups(pb), lr=0.0, eps=1e-15, capturable=True)
    ptr = pa._xyz.data_ptr()
    step = GraphedTrainStep(pa, oa, bg, LAM, dynamic=True, motion=True, gated=True, object_loss=W_OBJ).capture(
        cams[0], gt, warmup=1, accum_R=Ts[0][:3, :3], accum_T=Ts[0], gate=gate, obj_mask=mask, capacity_margin=2.0)
    la, terms = [], []
    for k in (1, 2, 3):
        if k != 2:
            la.append(float(step(pack_frame(cams[k], gt, Ts[k][:3, :3], gate, Ts[k], obj_mask=mask))))
        else:
            la.append(float(step(cams[k], gt, accum_R=Ts[k][:3, :3], gate=gate, accum_T=Ts[k], obj_mask=mask)))
        terms.append(step.loss_terms.cpu().tolist())
    torch.cuda.synchronize()
    assert step.ok() and pa._xyz.data_ptr() == ptr and float(oa.state[pa._xyz]["step"]) == 4.0
    lb = [_eager_step(pb, ob, cams[k], Ts[k], bg, gt, mask, gate) for k in range(4)]
    torch.cuda.synchronize()
    print("losses", la, lb[1:])
    assert all(abs(u - v) <= 2e-3 * abs(u) for u, v in zip(lb[1:], la)), (lb, la)
    for t, l in zip(terms, la):
        assert abs(W_OBJ["lambda_image"] * t[0] + W_OBJ["lambda_l1_alpha"] * t[1] + W_OBJ["lambda_l2_alpha"] * t[2] - l) <= 1e-5 * max(1.0, abs(l))
    for a in ("_xyz",) + LEAVES:
        u, v = getattr(pa, a).detach(), getattr(pb, a).detach()
        print(a, float((u - v).abs().mean()), float(u.abs().mean()))
        assert float((u - v).abs().mean()) <= 2e-4 * float(u.abs().mean()) + 1e-7, a


POSE_LR, K_STEPS = 1e-3, 4


def _pose_module():
    from tests.test_gpu_motion import Move
    return Move((0.02, -0.01, 0.03), [[1.0, 0.02], [-0.01, 1.0], [0.03, 0.01]], DEV)


def _pose_groups(pc, pose):
    from tests.test_gpu_motion import _groups
    return _groups(pc) + [{"params": [pose.obj_translation], "lr": POSE_LR, "name": "obj_translation"},
                          {"params": [pose.obj_rotation_6d], "lr": POSE_LR, "name": "obj_rotation_6d"}]


def test_graphed_step_with_a_trainable_pose():
    """GraphedTrainStep(..., pose=module): compose() runs inside the capture, dL/dA12 and dL/dM9 reach obj_translation / obj_rotation_6d through
    autograd, and the optimizer's step() inside the capture moves them.  After one warm-up step and K = 4 replays the two parameters are compared
    against two eager runs b1, b2 of the same five steps:  |a - b1| <= 4 |b1 - b2| + 1e-4 lr K  (the floor: the project's 1e-4 gradient bar
    carried through K normalised Adam steps).  Both parameters moved; the step counts are K + warm-up; with the Gaussians' learning rates set
    to 0 by param_groups edits (no re-capture) further replays leave every Gaussian parameter bit-identical while the pose keeps moving."""
    from tests.test_gpu_motion import _model, LEAVES
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    cams, Ts, bg, gt, mask, gate = _frames()
    order = [0] + [k % 4 for k in range(1, K_STEPS + 1)]
    pa, pose_a = _model(0), _pose_module()
    t0, r0 = pose_a.obj_translation.detach().clone(), pose_a.obj_rotation_6d.detach().clone()
    oa = FusedAdam(_pose_groups(pa, pose_a), lr=0.0, eps=1e-15, capturable=True)
    ptr = pa._xyz.data_ptr()
    step = GraphedTrainStep(pa, oa, bg, LAM, dynamic=True, motion=True, gated=True, object_loss=W_OBJ, pose=pose_a).capture(
        cams[0], gt, warmup=1, accum_R=Ts[0][:3, :3], accum_T=Ts[0], gate=gate, obj_mask=mask, capacity_margin=2.0)
    for k in order[1:]:
        step(pack_frame(cams[k], gt, Ts[k][:3, :3], gate, Ts[k], obj_mask=mask))
    torch.cuda.synchronize()
    assert step.ok() and pa._xyz.data_ptr() == ptr
    for p in (pa._xyz, pose_a.obj_translation, pose_a.obj_rotation_6d):
        assert float(oa.state[p]["step"]) == K_STEPS + 1
    ta, ra = pose_a.obj_translation.detach().clone(), pose_a.obj_rotation_6d.detach().clone()
    assert float((ta - t0).abs().max()) > 0 and float((ra - r0).abs().max()) > 0
    runs = []
    for _ in range(2):
        pb, pose_b = _model(0), _pose_module()
        ob = FusedAdam(_pose_groups(pb, pose_b), lr=0.0, eps=1e-15, capturable=True)
        for k in order:
            _eager_step(pb, ob, cams[k], Ts[k], bg, gt, mask, gate, pose=pose_b)
        torch.cuda.synchronize()
        runs.append((pose_b.obj_translation.detach().clone(), pose_b.obj_rotation_6d.detach().clone()))
    for name, a, b1, b2 in (("obj_translation", ta, runs[0][0], runs[1][0]), ("obj_rotation_6d", ra, runs[0][1], runs[1][1])):
        bound = 4 * (b1 - b2).abs() + 1e-4 * POSE_LR * K_STEPS
        print(name, "|a - b1|", (a - b1).abs().flatten().tolist(), "|b1 - b2|", (b1 - b2).abs().flatten().tolist(), "floor", 1e-4 * POSE_LR * K_STEPS)
        assert bool(((a - b1).abs() <= bound).all()), name
    # the stages' zero_gaussians_lr: an edit of param_groups, picked up by the next replay
    for g in oa.param_groups:
        if not g["name"].startswith("obj_"):
            g["lr"] = 0.0
    leaves = ("_xyz",) + LEAVES
    before = {a: getattr(pa, a).detach().clone() for a in leaves}
    for k in (1, 2):
        step(pack_frame(cams[k], gt, Ts[k][:3, :3], gate, Ts[k], obj_mask=mask))
    torch.cuda.synchronize()
    for a in leaves:
        assert torch.equal(getattr(pa, a).detach(), before[a]), a
    assert float((pose_a.obj_translation.detach() - ta).abs().max()) > 0 and float((pose_a.obj_rotation_6d.detach() - ra).abs().max()) > 0
    assert float(oa.state[pose_a.obj_translation]["step"]) == K_STEPS + 3
