"""GPU: opacity-entropy regularisation (include/egs_raster.h egs_opacity_entropy_*, egs_backward_entropy_lossgrad; csrc/opacity_entropy.h).

What it replaces in the reference: between std_train_iter and std_train_iter + entropy_reg_iter both static trainers add
0.1 * mean(-o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10)) over get_opacity[visibility_filter] to the image loss
(/root/reference/trainers/train_static.py:97-102, trainers/train_static_bg.py:105-110) and prune get_opacity < 0.5 when the phase ends.
The anchor and the bars are tests/entropy_anchor.py's (float64 on the float32 activated opacity; the torch expression clears half of each bar
on CPU, tests/test_entropy_cpu.py)."""
import math

import numpy as np
import pytest
import torch

from tests import entropy_anchor as EA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAVES = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")
W_ENT = 0.1


# ---- 1. the stand-alone kernels against the anchor -------------------------------------------------------------------------------------
def _radii_of(vis, seed):
    r = np.where(vis, 1 + (np.arange(vis.size) % 37), np.where(np.arange(vis.size) % 2 == 0, 0, -1)).astype(np.int32)      # radii <= 0: both kinds
    return torch.tensor(r, device=DEV)


def _standalone(x_in, radii, logit, weight, upstream, active_count=None):
    """-> (value float, n_vis int, activated float32[P] numpy, gradient float32[P] numpy), three times over: the same bits every time."""
    from egogaussian_amd import _C
    runs = []
    for _ in range(3):
        term = _C.EntropyTerm(weight, torch.device(DEV), upstream=torch.tensor([upstream], device=DEV))
        act = _C.opacity_entropy_forward(x_in, radii, term, logit=logit, active_count=active_count, want_activated=True)
        g = _C.opacity_entropy_backward(x_in, radii, term, logit=logit, active_count=active_count)
        torch.cuda.synchronize()
        runs.append((term.value.clone(), term.n_vis.clone(), act.clone(), g.clone()))
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(r[1], runs[0][1]), "the value is not the same bits on every launch"
        assert torch.equal(r[2].view(torch.int32), runs[0][2].view(torch.int32)) and torch.equal(r[3].view(torch.int32), runs[0][3].view(torch.int32))
    v, n, act, g = runs[0]
    return float(v), int(n), act.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("visible", [1.0, 0.0, 0.6], ids=["all-visible", "none-visible", "60pct"])
@pytest.mark.parametrize("logit", [True, False], ids=["logit", "activated"])
@pytest.mark.parametrize("P", [1, 255, 257, 2000, 20011, 70001])
def test_standalone_kernels_against_the_anchor(P, logit, visible):
    """(70 001 rows: 274 workgroup lines, more than the finish has lanes -- its spans loop.)"""
    x, vis = EA.inputs(P, seed=P % 7, visible=visible)
    x_in = torch.tensor(x) if logit else torch.sigmoid(torch.tensor(x))
    radii = _radii_of(vis, P)
    value, n_vis, act, g = _standalone(x_in.to(DEV), radii, logit, W_ENT, 2.5)
    if not logit:
        assert np.array_equal(act, x_in.numpy()), "an activated input is used as it is"
    ref = EA.anchor(act, vis, W_ENT, 2.5, logit=logit)
    ex = EA.grad_excess(g, ref)
    print(f"\n  [{P} rows, {'logit' if logit else 'activated'}, {int(vis.sum())} visible] value {value:.9g} (float64 {ref['value']:.9g}), "
          f"worst gradient error {ex:.2f} x 2^-24 of the unit (bar {EA.GRAD_ULPS})")
    assert n_vis == ref["n_vis"] == int(vis.sum())
    assert EA.value_ok(value, ref), (value, ref["value"])
    assert np.isfinite(g).all() and (g[~vis] == 0).all()
    assert EA.grad_ok(g, ref), ex


def test_capacity_model_dead_rows_are_skipped_whatever_they_hold():
    P, live = 2000, 1500
    x, vis = EA.inputs(P, seed=4)
    vis_live = vis.copy(); vis_live[live:] = False
    radii = _radii_of(vis, 0)
    radii[live:] = 9                                                 # stale radii of rows that are no Gaussians
    ac = torch.tensor([live], dtype=torch.int32, device=DEV)
    for logit in (True, False):
        x_in = (torch.tensor(x) if logit else torch.sigmoid(torch.tensor(x))).clone()
        x_in[live:] = float("nan")
        value, n_vis, act, g = _standalone(x_in.to(DEV), radii, logit, W_ENT, 1.0, active_count=ac)
        ref = EA.anchor(np.where(np.arange(P) < live, act, 0.0).astype(np.float32), vis_live, W_ENT, 1.0, logit=logit)
        assert n_vis == int(vis_live.sum()) and (act[live:] == 0).all() and (g[live:] == 0).all() and np.isfinite(g).all()
        assert EA.value_ok(value, ref) and EA.grad_ok(g, ref)


def test_autograd_function_over_the_standalone_kernels():
    """fused.opacity_entropy: weight * H as a differentiable scalar, [P,1] logits as the model stores them, an upstream factor from autograd."""
    from egogaussian_amd import fused
    from egogaussian_amd.losses import opacity_entropy as torch_expr
    P = 5003
    x, vis = EA.inputs(P, seed=2)
    radii = _radii_of(vis, 1)
    raw = torch.tensor(x, device=DEV).reshape(P, 1).requires_grad_(True)
    out = fused.opacity_entropy(raw, radii, weight=W_ENT, logit=True)
    (3.0 * out).backward()
    mirror = float(torch_expr(torch.sigmoid(raw.detach().double()), torch.tensor(vis, device=DEV)))
    assert abs(float(out.detach()) - W_ENT * mirror) <= 2e-5 * W_ENT and raw.grad.shape == raw.shape
    from egogaussian_amd import _C
    term = _C.EntropyTerm(1.0, torch.device(DEV))
    act = _C.opacity_entropy_forward(raw.detach(), radii, term, logit=True, want_activated=True).cpu().numpy()
    assert EA.grad_ok(raw.grad.cpu().numpy(), EA.anchor(act, vis, W_ENT, 3.0, logit=True))
    act_in = torch.tensor(act, device=DEV).requires_grad_(True)
    fused.opacity_entropy(act_in, radii, weight=torch.tensor(W_ENT, device=DEV)).backward()
    assert EA.grad_ok(act_in.grad.cpu().numpy(), EA.anchor(act, vis, np.float32(W_ENT), 1.0, logit=False))
    none = fused.opacity_entropy(raw, torch.zeros_like(radii), weight=W_ENT, logit=True)
    assert math.isnan(float(none.detach()))
    g0, = torch.autograd.grad(none, raw)
    assert float(g0.abs().max()) == 0.0                              # no visible row: NaN value, no gradient anywhere


# ---- 2. the rasterizer's backward with the term inside ---------------------------------------------------------------------------------
def _frame(N, H, W, seed, smul=2.0, hot=False):
    from egogaussian_amd.scene_synth import make_scene, make_camera
    sc = make_scene(N, H, W, seed)
    sc["log_scale"] += np.float32(math.log(smul))
    if hot:
        sc["log_scale"][7] = math.log(10.0); sc["opacity_logit"][7] = 0.0; sc["xyz"][7] = (0.0, 0.0, 5.0)      # one screen-filling splat
    g = torch.Generator().manual_seed(seed + 1)
    return sc, make_camera(3, H, W, device=DEV), torch.rand(3, H, W, generator=g).to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _backward_once(sc, cam, gt, bg, entropy, stats=False, lossgrad=True, **model):
    """One render + image loss + backward of a fresh model -> (gradients by leaf, screen-space gradient, radii, the term's value tensor, statistics)."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    pc = SynthGaussians(sc, device=DEV, **model)
    kw = {} if entropy is None else {"opacity_entropy": entropy}
    out = render(cam, pc, Pipe, bg, fused_densify_stats=stats, **kw)
    l1_ssim_loss(out["render"], gt, 0.2, raster_prologue=True, raster_lossgrad=lossgrad).backward()
    torch.cuda.synchronize()
    grads = {a: getattr(pc, a).grad.clone() for a in LEAVES}
    st = (pc.xyz_gradient_accum.clone(), pc.denom.clone(), pc.max_radii2D.clone())
    return grads, out["viewspace_points"].grad.clone(), out["radii"].clone(), out.get("opacity_entropy"), st, pc


def _equal_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _raw_call(sc, cam, bg):
    """The frame through _C with the RAW parameters (log-scales, raw quaternions, opacity logits) -> (backward(R, **kw) closure, forward outputs)."""
    from egogaussian_amd import _C
    t = lambda a: torch.tensor(a, device=DEV)
    xyz, sh, opac, scales, rots = t(sc["xyz"]), t(sc["features"][:, :1].copy()), t(sc["opacity_logit"]), t(sc["log_scale"]), t(sc["quat"])
    e = torch.empty(0, device=DEV)
    H, W = int(cam.image_height), int(cam.image_width)
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    out = _C.rasterize_gaussians(bg, xyz, e, opac, scales, rots, 1.0, e, cam.world_view_transform, cam.full_proj_transform, tx, ty, H, W, sh, 0,
                                 cam.camera_center, False, False, _C.ACT_RAW_PARAMETERS)
    R, color, depth, alpha, radii, geom, binning, img = out

    def backward(gcol, R_arg, **kw):
        return _C.rasterize_gaussians_backward(bg, xyz, radii, e, scales, rots, 1.0, e, cam.world_view_transform, cam.full_proj_transform, tx, ty, gcol, e, e,
                                               sh, 0, cam.camera_center, geom, R_arg, binning, img, alpha, False, _C.ACT_RAW_PARAMETERS, **kw)
    return backward, out, opac.reshape(-1)


NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


@pytest.mark.parametrize("case", ["2000@96x128", "hot", "densify_stats"])
def test_entropy_instantiation_changes_the_opacity_gradient_and_nothing_else(case):
    """2 000 Gaussians @ 96x128, raw parameters, tile culling on.  The backward blend adds into its accumulator with float atomics, so two
    backward calls of one frame differ in last bits whatever they are (printed below: plain against plain) -- "bit-identical to the plain call's"
    is only a statement about the per-Gaussian launch when both calls read the SAME sums.  They do here: one full plain call leaves the
    blend's accumulator in a caller-owned scratch; the plain per-Gaussian launch and the new entry point's (reduction + the entropy
    instantiation) then run on it alone (R = 0, prologue done: no blend, nothing cleared).
      * dL/dopacity of the new entry point against the plain one's plus the stand-alone entropy gradient: 2e-6 max-norm relative (the bar
        tests/test_gpu_label.py holds for two routes that add the same terms in another order);
      * every other gradient array bit-identical; rows with radii <= 0 exactly zero;
      * "hot": 300 Gaussians, one over >= 256 tiles -- the replica lines of pp_bwd_one;  "densify_stats": the statistics bit-identical."""
    from egogaussian_amd import _C, lib
    hot = case == "hot"
    N, H, W = (300, 272, 256) if hot else (2000, 96, 128)
    sc, cam, gt, bg = _frame(N, H, W, 3, hot=hot)
    backward, out, logits = _raw_call(sc, cam, bg)
    R, radii, geom = out[0], out[4], out[5]
    if hot:
        assert int(_C.geom_views(geom, N)["clamped"][7] >> 3) != 0, "the screen-filling Gaussian accumulates through replica lines"
    # an upstream image gradient of the size a mean loss has (0.8 / (3 H W) per pixel for the L1 part): the term is then a visible part of dL/dopacity
    gcol = ((torch.rand(3, H, W, generator=torch.Generator().manual_seed(9)) - 0.5) * (2.0 / (3 * H * W))).to(DEV)
    S = torch.empty((lib.load().egs_backward_scratch_bytes(N),), device=DEV, dtype=torch.uint8)
    full = backward(gcol, R, scratch=S)
    again = backward(gcol, R)
    torch.cuda.synchronize()
    noise = {n: int((a.view(torch.int32) != b.view(torch.int32)).sum()) for n, a, b in zip(NAMES, full, again) if a is not None and a.numel()}
    print(f"\n  [{case}] two plain calls of one frame, entries that differ (the blend's atomics): {noise}")
    stats = lambda: tuple(torch.zeros(N, device=DEV) for _ in range(3)) if case == "densify_stats" else None
    st_p, st_e = stats(), stats()
    plain = backward(gcol, 0, prologue_scratch=S, densify_stats=st_p)
    term = _C.EntropyTerm(W_ENT, torch.device(DEV))
    ent = backward(gcol, 0, prologue_scratch=S, densify_stats=st_e, opacity_entropy=term)
    alone = _C.EntropyTerm(W_ENT, torch.device(DEV))
    act = _C.opacity_entropy_forward(logits, radii, alone, logit=True, want_activated=True)
    g_ent = _C.opacity_entropy_backward(logits, radii, alone, logit=True)
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, full, plain):
        if a is not None and a.numel():
            assert _equal_bits(a, b), f"{n}: the per-Gaussian launch alone does not reproduce the full call on the same sums"
    want = plain[2].reshape(-1).double() + g_ent.double()
    err = float((ent[2].reshape(-1).double() - want).abs().max() / want.abs().max())
    share = float(g_ent.abs().max() / plain[2].abs().max())
    print(f"  [{case}] dL/dopacity with the term vs plain + stand-alone: {err:.1e} (the term is {share:.2g} of the plain gradient's maximum); "
          f"value {float(term.value):.6f}, {int(term.n_vis)} visible")
    assert err < 2e-6
    assert share > 1e-3, "the term must be visible in the gradient it joins"
    assert _equal_bits(term.value, alone.value) and int(term.n_vis) == int(alone.n_vis) == int((radii > 0).sum()), \
        "the fused reduction reads the same opacities in the same order as the stand-alone one"
    assert EA.value_ok(float(term.value), EA.anchor(act.cpu().numpy(), (radii > 0).cpu().numpy()))
    assert float(ent[2].reshape(-1)[radii <= 0].abs().max()) == 0.0 and int((radii <= 0).sum()) > 0
    for k, n in enumerate(NAMES):
        if k != 2 and plain[k] is not None and plain[k].numel():
            assert _equal_bits(plain[k], ent[k]), f"{n}: the term changed a gradient it has no part in"
    if st_p is not None:
        for a, b in zip(st_p, st_e):
            assert _equal_bits(a, b), "the densification statistics differ from the plain call's"
        assert float(st_e[1].sum()) == float((radii > 0).sum()) and float(st_e[0].sum()) > 0


@pytest.mark.parametrize("lossgrad", [True, False], ids=["gradient-formed-in-the-blend", "loss-backward-launch"])
def test_render_option_adds_the_standalone_term_to_the_opacity_gradient(lossgrad):
    """render(..., opacity_entropy=w) without optimizer=, through autograd: `_opacity.grad` against the plain render's (egs_backward_lossgrad, or
    the loss backward launch in front of egs_backward_adam) plus the stand-alone entropy gradient, 2e-6 max-norm relative; the unweighted
    value in the returned dict; the other leaves within what two plain calls differ by (the blend's atomics: 1e-5 of the array's maximum)."""
    from egogaussian_amd import _C
    N, H, W = 2000, 96, 128
    sc, cam, gt, bg = _frame(N, H, W, 3)
    plain, scr_p, radii, none, _, _ = _backward_once(sc, cam, gt, bg, None, False, lossgrad)
    ent, scr_e, radii_e, value, _, _ = _backward_once(sc, cam, gt, bg, W_ENT, False, lossgrad)
    assert none is None and torch.equal(radii, radii_e)
    term = _C.EntropyTerm(W_ENT, torch.device(DEV))
    logits = torch.tensor(sc["opacity_logit"], device=DEV).reshape(-1)
    _C.opacity_entropy_forward(logits, radii, term, logit=True)
    g_ent = _C.opacity_entropy_backward(logits, radii, term, logit=True)
    torch.cuda.synchronize()
    want = plain["_opacity"].reshape(-1).double() + g_ent.double()
    err = float((ent["_opacity"].reshape(-1).double() - want).abs().max() / want.abs().max())
    print(f"\n  render(opacity_entropy={W_ENT}): _opacity.grad vs plain + stand-alone {err:.1e}; value {float(value):.6f}")
    assert err < 2e-6 and _equal_bits(value, term.value)
    assert float(ent["_opacity"].reshape(-1)[radii <= 0].abs().max()) == 0.0
    for a in LEAVES:
        if a != "_opacity":
            assert float((plain[a] - ent[a]).abs().max()) <= 1e-5 * float(plain[a].abs().max()), a
    with torch.no_grad():                                            # no backward will run: the value comes from the stand-alone kernels, now
        from egogaussian_amd.scene_synth import SynthGaussians, Pipe
        from egogaussian_amd.renderer import render
        out = render(cam, SynthGaussians(sc, device=DEV, requires_grad=False), Pipe, bg, opacity_entropy=W_ENT)
    assert _equal_bits(out["opacity_entropy"], term.value)


def test_render_option_on_a_model_that_hands_over_a_covariance():
    """The same through the covariance route (no raw-parameter hooks: torch builds cov3D_precomp and activates the opacity, the library is
    handed both): the term's share joins dL/d(activated opacity) and autograd carries it through the sigmoid.  `_opacity.grad` against the plain
    render's of the same route plus the stand-alone gradient w.r.t. the activated opacity times s (1 - s), 2e-6 max-norm relative (the bar
    above); the value bit-identical to the stand-alone reduction over the same activated opacities; the other leaves as above."""
    from egogaussian_amd import _C
    N, H, W = 2000, 96, 128
    sc, cam, gt, bg = _frame(N, H, W, 3)
    plain, _, radii, none, _, _ = _backward_once(sc, cam, gt, bg, None, fused=False)
    ent, _, radii_e, value, _, pc = _backward_once(sc, cam, gt, bg, W_ENT, fused=False)
    assert none is None and torch.equal(radii, radii_e)
    assert pc.get_raw_parameters() is None, "the model must take the covariance route"
    act = pc.get_opacity.detach().reshape(-1).contiguous()
    term = _C.EntropyTerm(W_ENT, torch.device(DEV))
    _C.opacity_entropy_forward(act, radii, term, logit=False)
    g_ent = _C.opacity_entropy_backward(act, radii, term, logit=False) * (act * (1.0 - act))
    torch.cuda.synchronize()
    want = plain["_opacity"].reshape(-1).double() + g_ent.double()
    err = float((ent["_opacity"].reshape(-1).double() - want).abs().max() / want.abs().max())
    print(f"\n  render(opacity_entropy={W_ENT}), covariance given: _opacity.grad vs plain + stand-alone {err:.1e}; value {float(value):.6f}")
    assert err < 2e-6 and _equal_bits(value, term.value)
    assert float(g_ent.abs().max() / plain["_opacity"].abs().max()) > 1e-3, "the term must be visible in the gradient it joins"
    assert float(ent["_opacity"].reshape(-1)[radii <= 0].abs().max()) == 0.0
    for a in LEAVES:
        if a != "_opacity":
            assert float((plain[a] - ent[a]).abs().max()) <= 1e-5 * float(plain[a].abs().max()), a


def _geom_of(sc, cam, bg):
    """The geometry buffer of a forward of this frame (the hot codes live there)."""
    from egogaussian_amd import _C
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    geoms = []
    orig = _C.rasterize_gaussians

    def spy(*a, **k):
        res = orig(*a, **k)
        geoms.append(res[5])
        return res
    _C.rasterize_gaussians = spy
    try:
        with torch.no_grad():
            render(cam, SynthGaussians(sc, device=DEV, requires_grad=False), Pipe, bg)
    finally:
        _C.rasterize_gaussians = orig
    return geoms[-1]


# ---- 3. Adam inside the backward ----------------------------------------------------------------------------------------------------------
def _groups(pc):
    g = [{"params": [pc._xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [pc._features_dc], "lr": 2.5e-3, "name": "f_dc"},
         {"params": [pc._opacity], "lr": 0.05, "name": "opacity"}, {"params": [pc._scaling], "lr": 5e-3, "name": "scaling"},
         {"params": [pc._rotation], "lr": 1e-3, "name": "rotation"}]
    if pc._features_rest.numel():
        g.append({"params": [pc._features_rest], "lr": 2.5e-3 / 20, "name": "f_rest"})
    return g


def _scene(N, H, W, seed=0, sh_degree=0, n_cams=4, smul=2.0):
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    teacher = make_scene(N, H, W, seed, sh_degree=sh_degree); teacher["log_scale"] += np.float32(math.log(smul))
    cams = [make_camera(k * 40, H, W, device=DEV) for k in range(n_cams)]
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=DEV, sh_degree=sh_degree, requires_grad=False)
        gts = [render(c, tpc, Pipe, bg)["render"].clone() for c in cams]
    return perturb_student(teacher), cams, gts, bg


@pytest.mark.parametrize("sh_degree", [0, 3], ids=["one-coefficient", "split-16"])
def test_adam_inside_the_backward_steps_on_the_whole_gradient(sh_degree):
    """The pattern of tests/test_gpu_fused_adam.py: with keep_grads the backward steps the leaves AND writes their gradients -- the opacity's
    with the entropy share --, a twin optimizer replays the written gradients through the stand-alone k_adam: parameters and both moments
    bit-identical.  Both colour layouts (the opacity is stepped by the preprocess backward in either)."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.optim import FusedAdam
    student, cams, gts, bg = _scene(4000, 96, 160, sh_degree=sh_degree)
    pa = SynthGaussians(student, device=DEV, sh_degree=sh_degree)
    oa = FusedAdam(_groups(pa), lr=0.0, eps=1e-15, capturable=True)
    pb = SynthGaussians(student, device=DEV, sh_degree=sh_degree)
    ob = FusedAdam(_groups(pb), lr=0.0, eps=1e-15, capturable=True)
    leaves = LEAVES + (("_features_rest",) if sh_degree else ())
    real_make = oa.make_sink

    def keeping(**kw):
        sink = real_make(**kw)
        sink.keep_grads = True
        keeping.last = sink
        return sink
    oa.make_sink = keeping
    for it in range(3):
        for a in leaves:
            with torch.no_grad():
                getattr(pb, a).copy_(getattr(pa, a))
        with torch.no_grad():
            plain_o = pa._opacity.detach().clone()
        out = render(cams[it], pa, Pipe, bg, optimizer=oa, opacity_entropy=W_ENT)
        l1_ssim_loss(out["render"], gts[it], 0.2, raster_prologue=True, raster_lossgrad=True).backward()
        assert 1 in keeping.last.owned                              # the opacity stays a fused leaf
        for a in leaves:
            g = getattr(pa, a).grad
            assert g is not None and float(g.abs().max()) > 0
            getattr(pb, a).grad = g.clone()
        # the written opacity gradient holds the term: it differs from the image loss's alone by the stand-alone gradient
        from egogaussian_amd import _C
        term = _C.EntropyTerm(W_ENT, torch.device(DEV))
        _C.opacity_entropy_forward(plain_o, out["radii"], term, logit=True)
        g_ent = _C.opacity_entropy_backward(plain_o, out["radii"], term, logit=True)
        assert float(g_ent.abs().max()) > 1e-3 * float(pa._opacity.grad.abs().max())
        oa.step(); oa.zero_grad(set_to_none=True)
        ob.step(); ob.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        for a in leaves:
            x, y = getattr(pa, a), getattr(pb, a)
            assert torch.equal(x.detach(), y.detach()), f"iteration {it}: {a} differs"
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[x][key], ob.state[y][key]), f"iteration {it}: {a} {key} differs"
            assert float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == it + 1


def test_the_torch_expression_on_a_fused_opacity_is_still_refused():
    """The entropy term written in torch next to render(optimizer=) remains a second path the library cannot see: FusedAdam raises and names
    render(opacity_entropy=)."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.losses import opacity_entropy
    from egogaussian_amd.optim import FusedAdam
    student, cams, gts, bg = _scene(2000, 96, 128, n_cams=1)
    pc = SynthGaussians(student, device=DEV)
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    out = render(cams[0], pc, Pipe, bg, optimizer=opt)
    (l1_ssim_loss(out["render"], gts[0], 0.2) + W_ENT * opacity_entropy(pc.get_opacity, out["visibility_filter"])).backward()
    with pytest.raises(RuntimeError, match="opacity_entropy=w"):
        opt.step()


# ---- 4. the captured step ------------------------------------------------------------------------------------------------------------------
def _one_wave_scene(H=96, W=128, per_quadrant=10, seed=5):
    """A frame whose backward blend is deterministic: every Gaussian sits on the centre of an 8x8 pixel quadrant with a footprint of
    0.5 px (radius 3: its 3-sigma rectangle and its alpha >= 1/255 box stay inside the quadrant, 1 px from its border), so exactly ONE
    wave of the blend contributes to its accumulator line -- one float atomic onto a cleared line, no order to vary.  Two runs of the same
    step are then bit-identical, and "bit-identical" between two differently captured steps is a statement about the steps.
    -> (teacher scene, student scene: colours and opacities perturbed, positions kept), camera, background."""
    from egogaussian_amd.scene_synth import make_scene, make_camera
    cam = make_camera(0, H, W, device=DEV)
    qy, qx = H // 8, W // 8
    N = qy * qx * per_quadrant
    sc = make_scene(N, H, W, seed)
    rng = np.random.default_rng(seed)
    z = rng.uniform(3.0, 8.0, N)
    px = np.tile(np.repeat(np.arange(qx) * 8 + 3.5, 1), qy * per_quadrant)
    py = np.tile(np.repeat(np.arange(qy) * 8 + 3.5, qx), per_quadrant)
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    view = np.stack([((2 * px + 1) / W - 1) * tx * z, ((2 * py + 1) / H - 1) * ty * z, z, np.ones(N)], 1)
    world = view @ np.linalg.inv(cam.world_view_transform.cpu().double().numpy())
    sc["xyz"] = world[:, :3].astype(np.float32)
    focal = W / (2 * tx)
    sc["log_scale"] = np.repeat(np.log(0.5 * z / focal)[:, None], 3, 1).astype(np.float32)
    student = {k: v.copy() for k, v in sc.items()}
    student["features"] += rng.normal(0, 0.2, student["features"].shape).astype(np.float32)
    student["opacity_logit"] += rng.normal(0, 0.5, student["opacity_logit"].shape).astype(np.float32)
    return sc, student, cam, torch.zeros(3, device=DEV)


def _one_wave_frames():
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    teacher, student, cam, bg = _one_wave_scene()
    with torch.no_grad():
        out = render(cam, SynthGaussians(teacher, device=DEV, requires_grad=False), Pipe, bg)
    radii = out["radii"]
    assert int((radii > 0).sum()) > 0.9 * radii.numel() and int(radii.max()) <= 3, "the scene is not the one-wave scene it is meant to be"
    return student, [cam], [out["render"].clone()], bg


def _state(pc, opt):
    out = {}
    for a in LEAVES:
        p = getattr(pc, a)
        out[a] = p.detach().clone()
        for key in ("exp_avg", "exp_avg_sq", "step"):
            out[a + "." + key] = opt.state[p][key].clone()
    return out


def _captured(student, cams, gts, bg, entropy_reg, fuse, weight=None, replays=3, **kw):
    from egogaussian_amd.scene_synth import SynthGaussians
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep
    pc = SynthGaussians(student, device=DEV)
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    step = GraphedTrainStep(pc, opt, bg, 0.2, fuse_optimizer=fuse, entropy_reg=entropy_reg, **kw)
    if weight is not None:
        step.entropy_weight = weight
    step.capture(cams[0], gts[0], warmup=1)
    for i in range(replays):
        step(cams[(i + 1) % len(cams)], gts[(i + 1) % len(gts)])
    torch.cuda.synchronize()
    assert step.ok()
    return pc, opt, step


def _differing(a, b):
    return {k: int((a[k].contiguous().view(torch.int32) != b[k].contiguous().view(torch.int32)).sum()) for k in a if not _equal_bits(a[k], b[k])}


def test_captured_step_fused_and_unfused_optimizer_are_bit_identical():
    """GraphedTrainStep(entropy_reg=True), weight 0.1 from the capture on: fuse_optimizer=True and False after 3 replays, bit for bit -- on the
    one-wave scene, where the blend's float atomics have no order to vary (two runs of ONE configuration are bit-identical there, asserted
    first: without that, bit-identity of two configurations is not a property of the code)."""
    student, cams, gts, bg = _one_wave_frames()
    pa, oa, sa = _captured(student, cams, gts, bg, True, True, W_ENT)
    pa2, oa2, _ = _captured(student, cams, gts, bg, True, True, W_ENT)
    assert not _differing(_state(pa, oa), _state(pa2, oa2)), "two runs of one configuration differ: the scene does not make the blend deterministic"
    pb, ob, sb = _captured(student, cams, gts, bg, True, False, W_ENT)
    assert not torch.equal(pa._opacity.detach().cpu(), torch.tensor(student["opacity_logit"])), "nothing was trained"
    assert all(getattr(pa, a).grad is None for a in LEAVES) and pb._opacity.grad is not None
    assert _equal_bits(sa.entropy, sb.entropy) and 0.0 < float(sa.entropy) < math.log(2.0) + 1e-6
    diff = _differing(_state(pa, oa), _state(pb, ob))
    print(f"\n  fused vs unfused after 3 replays: {'bit-identical' if not diff else 'entries that differ: ' + str(diff)}")
    assert not diff, diff


def test_weight_zero_is_the_step_captured_without_the_option():
    """With weight 0 a replay leaves every parameter and moment bit-identical to the same step captured without entropy_reg (on the one-wave
    scene: see test_captured_step_fused_and_unfused_optimizer_are_bit_identical), while a weight of 0.1 does not."""
    student, cams, gts, bg = _one_wave_frames()
    pw, ow, _ = _captured(student, cams, gts, bg, True, True, W_ENT)
    p0, o0, _ = _captured(student, cams, gts, bg, False, True, None)
    assert "_opacity" in _differing(_state(pw, ow), _state(p0, o0)), "the term at weight 0.1 moved no opacity"
    for fuse in (True, False):
        pa, oa, sa = _captured(student, cams, gts, bg, True, fuse, 0.0, densify_stats=True)
        pb, ob, sb = _captured(student, cams, gts, bg, False, fuse, None, densify_stats=True)
        assert sb.entropy is None and float(sa.entropy) > 0.0       # the value is still reported
        diff = _differing(_state(pa, oa), _state(pb, ob))
        print(f"\n  weight 0 vs no entropy_reg (fuse_optimizer={fuse}): {'bit-identical' if not diff else 'entries that differ: ' + str(diff)}")
        assert not diff, (fuse, diff)
        assert _equal_bits(sa.loss, sb.loss) and _equal_bits(sa.loss_sum, sb.loss_sum), "loss and loss_sum stay the image loss"
        assert _equal_bits(pa.denom, pb.denom) and _equal_bits(pa.xyz_gradient_accum, pb.xyz_gradient_accum)


def test_entropy_reg_goes_with_several_steps_per_replay_double_buffer_and_a_gate():
    """steps_per_replay=2, the same doubled-buffered, and gated=True (a gate of ones) with the term on: four iterations on packed frames leave
    every parameter and moment where four single-step replays leave them -- bit for bit on the one-wave scene --, and `step.entropy` is the
    last iteration's value."""
    from egogaussian_amd.scene_synth import SynthGaussians
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    student, cams, gts, bg = _one_wave_frames()
    gate = torch.ones(gts[0].shape[-2:], device=DEV)
    res = {}
    for name, kw in (("single", {}), ("two-per-replay", dict(steps_per_replay=2)), ("double-buffer", dict(steps_per_replay=2, double_buffer=True)),
                     ("gated", dict(gated=True))):
        pc = SynthGaussians(student, device=DEV)
        opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
        step = GraphedTrainStep(pc, opt, bg, 0.2, entropy_reg=True, **kw)
        step.entropy_weight = W_ENT
        gated = bool(kw.get("gated"))
        step.capture(cams[0], gts[0], warmup=1, gate=gate if gated else None)
        frame = pack_frame(cams[0], gts[0], gate=gate if gated else None)
        spr = kw.get("steps_per_replay", 1)
        for _ in range(4 // spr):
            step(frame if spr == 1 else torch.stack([frame] * spr))
        torch.cuda.synchronize()
        assert step.ok() and float(opt.state[pc._opacity]["step"]) == 5.0
        res[name] = (_state(pc, opt), step.entropy.clone())
    for name in ("two-per-replay", "double-buffer", "gated"):
        diff = _differing(res["single"][0], res[name][0])
        assert not diff, (name, diff)
        assert _equal_bits(res["single"][1], res[name][1]) and 0.0 < float(res[name][1]) < math.log(2.0) + 1e-6


def test_replayed_opacity_gradient_against_the_float64_chain():
    """fuse_optimizer=False: the replay's `_opacity.grad` against oracle render (float64) + torch loss (float64) + the anchor, every row held to
    its own magnitude under the rule of tests/common.py (yardstick: the same chain through the float32 oracle and float32 torch)."""
    from oracle.oracle import Oracle
    from egogaussian_amd import _C, losses
    from egogaussian_amd.scene_synth import SynthGaussians
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep
    from tests.common import check_grad_rows_vs_float64, flip_pixels, gaussians_contributing_to
    N, H, W = 2000, 96, 128
    student, cams, gts, bg = _scene(N, H, W, n_cams=2)
    pc = SynthGaussians(student, device=DEV)
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    step = GraphedTrainStep(pc, opt, bg, 0.2, fuse_optimizer=False, entropy_reg=True)
    step.entropy_weight = W_ENT
    step.capture(cams[0], gts[0], warmup=1)
    img_buf = _C.stats["image_buffer"]
    snap = {a: getattr(pc, a).detach().clone().cpu() for a in LEAVES}       # what the replay renders (its update comes after)
    step(cams[1], gts[1])
    torch.cuda.synchronize()
    got = pc._opacity.grad.detach().clone().reshape(-1)
    cam, gt = cams[1], gts[1].cpu()
    chains = {}
    for dt, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        raw = snap["_opacity"].to(dt)
        d = dict(means3D=snap["_xyz"].to(dt), opacities=torch.sigmoid(raw), shs=snap["_features_dc"].to(dt), scales=torch.exp(snap["_scaling"].to(dt)),
                 rotations=torch.nn.functional.normalize(snap["_rotation"].to(dt)), viewmatrix=cam.world_view_transform.cpu().to(dt),
                 projmatrix=cam.full_proj_transform.cpu().to(dt), campos=cam.camera_center.cpu().to(dt), bg=bg.cpu().to(dt), image_height=H,
                 image_width=W, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2), sh_degree=0, scale_modifier=1.0)
        o = Oracle(npdt, nthreads=8)
        st = o.forward(**d)
        img = torch.tensor(np.asarray(st["color"]), dtype=dt).requires_grad_(True)
        losses.training_loss(img, gt.to(dt), 0.2).backward()
        gb = o.backward(st, img.grad, None, None)
        s = torch.sigmoid(raw).reshape(-1)
        g_img = torch.tensor(np.asarray(gb["dL_dopacity"]), dtype=dt).reshape(-1) * s * (1 - s)
        chains[dt] = (st, gb, g_img)
    st32, gb32, gi32 = chains[torch.float32]
    st64, gb64, gi64 = chains[torch.float64]
    vis = np.asarray(st32["radii"]) > 0
    assert np.array_equal(vis, step.radii.cpu().numpy() > 0)
    # the entropy share: float64 = the anchor on the float32 activated opacity as the kernels form it (the fused reduction reads the same bits
    # from the forward's records: test_fused_gradient_is_the_plain_gradient_plus_the_standalone_term); float32 = torch autograd of the
    # reference's expression
    probe = _C.EntropyTerm(1.0, torch.device(DEV))
    o32 = _C.opacity_entropy_forward(snap["_opacity"].to(DEV), step.radii, probe, logit=True, want_activated=True).cpu().numpy()
    ref = EA.anchor(o32, vis, W_ENT, 1.0, logit=True)
    xt = snap["_opacity"].clone().reshape(-1).requires_grad_(True)
    (W_ENT * losses.opacity_entropy(torch.sigmoid(xt), torch.tensor(vis))).backward()
    g32 = {"dL_dopacity": (gi32 + xt.grad).numpy()}
    g64 = {"dL_dopacity": gi64.numpy() + ref["grad"]}
    flip_px = flip_pixels(step.image.cpu().numpy(), _C.image_views(img_buf, W, H)["final_T"].cpu().numpy(), st32)
    print("\n" + check_grad_rows_vs_float64(["dL_dopacity"], [got], st32, g32, st64, g64, gaussians_contributing_to(st32, flip_px, 0),
                                            what=f"[captured step, {N}@{W}x{H}, weight {W_ENT}]"))
    assert EA.value_ok(float(step.entropy), ref)
    share = float(np.abs(ref["grad"]).max() / np.abs(g64["dL_dopacity"]).max())
    assert share > 1e-3, share                                       # the term is a visible part of what is being checked


def test_weight_changes_between_replays_without_recapture():
    """The weight is a device scalar pushed like a learning rate: from identical states, a replay at weight 0.1 differs from one at weight 0 in
    `_opacity.grad` by the anchor's gradient, nothing was re-captured, and `step.entropy` follows the opacities."""
    from egogaussian_amd import _C
    student, cams, gts, bg = _scene(2000, 96, 128, n_cams=2)
    res = {}
    for w in (0.0, W_ENT):
        pc, opt, step = _captured(student, cams, gts, bg, True, False, 0.0, replays=1)
        graph0 = step.graph
        before = pc._opacity.detach().clone().reshape(-1)
        h_prev = float(step.entropy)
        step.entropy_weight = w                                      # (no capture() / recapture() from here on)
        step(cams[0], gts[0])
        torch.cuda.synchronize()
        assert step.graph is graph0 and step.recaptures == 0
        term = _C.EntropyTerm(1.0, torch.device(DEV))
        act = _C.opacity_entropy_forward(before, step.radii, term, logit=True, want_activated=True).cpu().numpy()
        ref = EA.anchor(act, (step.radii > 0).cpu().numpy(), W_ENT, 1.0, logit=True)
        assert EA.value_ok(float(step.entropy), ref) and float(step.entropy) != h_prev
        res[w] = (pc._opacity.grad.detach().clone().reshape(-1), ref)
    delta = (res[W_ENT][0].double() - res[0.0][0].double()).cpu().numpy()
    ref = res[W_ENT][1]
    scale = np.abs(ref["grad"]).max()
    err = float(np.abs(delta - ref["grad"]).max() / scale)
    print(f"\n  gradient(weight 0.1) - gradient(weight 0) vs the anchor: {err:.1e} of its maximum")
    assert scale > 0 and err < 1e-3, "the new weight did not take effect"


def test_overflowed_frame_leaves_parameters_and_moments_untouched():
    """capacity= forced small, as tests/test_gpu_capacity.py does: the clipped frame's step is skipped on the device, entropy term and all."""
    from egogaussian_amd import _C
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep
    student, cams, gts, bg = _scene(2000, 96, 128, n_cams=1)
    for fuse in (True, False):
        pc = SynthGaussians(student, device=DEV)
        opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
        with torch.no_grad():
            r_now = render(cams[0], pc, Pipe, bg) and _C.stats["num_rendered"]
        step = GraphedTrainStep(pc, opt, bg, 0.2, fuse_optimizer=fuse, entropy_reg=True)
        step.entropy_weight = W_ENT
        step.capture(cams[0], gts[0], warmup=1, capacity=int(r_now * 1.1))
        step(cams[0], gts[0])
        torch.cuda.synchronize()
        assert step.ok() and not step.last_frame_overflowed()
        with torch.no_grad():
            pc._scaling += math.log(3.0)                             # same tensors, several times the footprint: the next frame cannot fit
        torch.cuda.synchronize()
        before = _state(pc, opt)
        step(cams[0], gts[0])
        torch.cuda.synchronize()
        assert step.last_frame_overflowed() and not step.ok()
        diff = _differing(before, _state(pc, opt))
        assert not diff, (fuse, diff)


# ---- 5. behaviour ---------------------------------------------------------------------------------------------------------------------------
def test_entropy_phase_lowers_the_entropy_and_prunes_without_recapture():
    """10 000 Gaussians @ 64x64 on a capacity model: 60 plain steps then 60 at weight 0.1, against 120 plain steps from the same seed.  The mean
    entropy of the visible opacities ends lower with the term; prune_points(get_opacity < 0.5) then runs in place and the SAME graph keeps
    replaying the pruned model."""
    from egogaussian_amd import densify
    from egogaussian_amd.capacity import CapacityGaussians
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.losses import opacity_entropy
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    N, H, W = 10000, 64, 64
    student, cams, gts, bg = _scene(N, H, W, n_cams=4, smul=1.5)
    ends = {}
    for with_term in (False, True):
        pc = CapacityGaussians(student, 12000, device=DEV)
        pc.training_setup(capturable=True)
        step = GraphedTrainStep(pc, pc.optimizer, bg, 0.2, densify_stats=True, entropy_reg=True).capture(cams[0], gts[0], warmup=1)
        graph0, ptr0 = step.graph, pc._opacity.data_ptr()
        for it in range(119):
            if it == 59 and with_term:
                step.entropy_weight = W_ENT
            step(cams[it % 4], gts[it % 4])
        torch.cuda.synchronize()
        assert step.ok()
        with torch.no_grad():
            out = render(cams[0], pc, Pipe, bg)
            ends[with_term] = float(opacity_entropy(pc.get_opacity[:pc.n_active], out["visibility_filter"][:pc.n_active]))
        if with_term:
            n0 = pc.n_active
            with torch.no_grad():
                mask = (pc.get_opacity < 0.5).squeeze(-1)
            densify.prune_points(pc, mask)
            assert 0 < pc.n_active < n0 and pc._opacity.data_ptr() == ptr0
            with torch.no_grad():
                assert float(pc.get_opacity[:pc.n_active].min()) >= 0.5
                eager = render(cams[1], pc, Pipe, bg)["render"].clone()
            step.entropy_weight = 0.0
            step(cams[1], gts[1])
            torch.cuda.synchronize()
            assert step.graph is graph0 and step.recaptures == 0 and step.ok()
            assert torch.equal(step.image, eager), "the captured step does not render the pruned model"
            print(f"\n  pruned opacity < 0.5: {n0} -> {pc.n_active} Gaussians, no re-capture")
    print(f"  mean entropy of the visible opacities after 120 steps: plain {ends[False]:.4f}, with the term from step 60 {ends[True]:.4f}")
    assert ends[True] < ends[False]
