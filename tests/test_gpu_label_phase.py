"""GPU: the label phase (include/egs_raster.h: EGS_ACT_SCALAR_COLOR, egs_label_bce_*, egs_backward_label; csrc/label_bce.h, label_loss.hip,
render_bwd.hip k_render_backward<3, LG>).

The reference trains the per-Gaussian label for 30 000 iterations on BCEWithLogits(mean_c(label render), obj_mask) with the hand-mask hook and
Adam on the label alone (/root/reference/trainers/train_static.py:104-109).  Checked here, piece by piece: the loss kernels against the float64
torch mirror, the scalar colour input against the expanded one (bit for bit), the scalar backward blend against the C oracle and against the
three-sum blend it replaces, hot replica lines, the loss gradient formed inside the blend against the stand-alone launches, and the Adam step
taken by the last launch against egs_adam_step_capturable (bit for bit).

Tolerances.  Loss value: 1e-5 * max(1, |l64|), the bar of tests/test_gpu_object_loss.py (float32 sums of <= 64 terms, then float64).  dL/dC: 1e-4
max-norm relative with the unit never below UP / (3 H W) (the size of a saturated pixel's gradient).  Gradients of the label: 1e-4 against the
oracle and 2e-6 between two routes that add the same per-pixel terms in another order -- the bars tests/test_gpu_label.py holds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.common import make_inputs, seeded_grads, rel_err, tile_culling
from tests.test_gpu_parity import hip_forward, oracle_forward, _dev, _to

pytestmark = pytest.mark.gpu
UP = 3.0


def _mirror64(img, mask, gate, up):
    """float64 torch mirror with the reference's hook -> (value, dL/dimg [3,H,W])"""
    from egogaussian_amd.losses import label_bce_loss
    x = img.detach().double().cpu().requires_grad_(True)
    m = mask.double().cpu()
    mean = x.mean(0, keepdim=True)
    if gate is not None:
        mean.register_hook(lambda g: g * gate.double().cpu().reshape(g.shape))
    ref = torch.nn.BCEWithLogitsLoss()(mean, m.reshape(mean.shape))
    assert float(ref.detach()) == float(label_bce_loss(x.detach(), m))          # the package's mirror IS that expression
    (ref * up).backward()
    return float(ref.detach()), x.grad


def _loss_inputs(H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(3, H, W, generator=g) * 2.0                       # three different planes: the mean is really taken
    mask = (torch.rand(H, W, generator=g) > 0.5).float()
    sel = torch.rand(H, W, generator=g)
    img[:, sel < 0.25] = 0.0; mask[sel < 0.25] = 0.0                    # a quarter of the pixels: x = 0, m = 0 (no splat, no object)
    img[:, (sel >= 0.25) & (sel < 0.30)] = 30.0                         # saturated logits, both signs, against both mask values
    img[:, (sel >= 0.30) & (sel < 0.35)] = -30.0
    gate = (torch.rand(H, W, generator=g) > 0.3).float() * torch.rand(H, W, generator=g)
    return img.to(dev), mask.to(dev), gate.to(dev)


@pytest.mark.parametrize("H,W", [(48, 80), (37, 53), (7, 9)])
@pytest.mark.parametrize("gated", [False, True])
def test_loss_kernels_against_float64_mirror(H, W, gated):
    from egogaussian_amd import _C
    dev = _dev()
    img, mask, gate = _loss_inputs(H, W, H * 100 + W, dev)
    gate = gate if gated else None
    up = torch.full((1,), UP, device=dev)
    l64, g64 = _mirror64(img, mask, gate, UP)
    vals = []
    for _ in range(3):
        loss, _ = _C.label_bce_forward(img, mask)
        vals.append(loss.clone())
    _, partial = _C.label_bce_forward(img, mask, defer_value=True)
    dloss = torch.full((1,), -1.0, device=dev)
    dimg = _C.label_bce_backward(img, mask, up, gate, deferred_partial=partial, deferred_loss=dloss)
    torch.cuda.synchronize()
    tol = 1e-5 * max(1.0, abs(l64))
    print(f"\n[{H}x{W} gated={gated}] loss {float(vals[0]):.8f} (float64 {l64:.8f}), deferred {float(dloss):.8f}")
    assert abs(float(vals[0]) - l64) <= tol and abs(float(dloss) - l64) <= tol
    assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2]) and torch.equal(vals[0], dloss), "fixed order: the same bits every run, either way"
    unit = max(float(g64.abs().max()), UP / (3 * H * W))
    err = float((dimg.double().cpu() - g64).abs().max()) / unit
    print(f"    dL/dC max-norm relative error {err:.2e}")
    assert err < 1e-4
    assert torch.equal(dimg[0], dimg[1]) and torch.equal(dimg[0], dimg[2])


def _forward(d, dev, scalar_label=None):
    """hip_forward, or -- scalar_label [P] -- the same call with the label as one value per Gaussian"""
    from egogaussian_amd import _C
    if scalar_label is None:
        return hip_forward(d, dev)
    g = _to(d, dev)
    e = torch.empty(0, device=dev)
    out = _C.rasterize_gaussians(g["bg"], g["means3D"], scalar_label.to(dev), g["opacities"], g.get("scales", e), g.get("rotations", e),
                                 g["scale_modifier"], g.get("cov3D_precomp", e), g["viewmatrix"], g["projmatrix"], g["tanfovx"], g["tanfovy"],
                                 g["image_height"], g["image_width"], e, g["sh_degree"], g["campos"], False, False, _C.ACT_SCALAR_COLOR)
    return g, out


def test_scalar_colour_forward_is_the_expanded_one_bit_for_bit():
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 2000, 96, 128
    d = make_inputs(N, H, W, 3, 0, "col_sr", scale_mul=2.0)
    label = torch.randn(N, 1, generator=torch.Generator().manual_seed(9))
    d["colors_precomp"] = label.expand(-1, 3).contiguous()
    _, a = _forward(d, dev)
    _, b = _forward(d, dev, scalar_label=label.reshape(-1))
    torch.cuda.synchronize()
    assert a[0] == b[0] and a[0] > 0
    assert torch.equal(a[1], b[1]) and torch.equal(a[4], b[4]), "image and radii"
    R = a[0]
    va, vb = _C.binning_views(a[6], N, R, W, H, _C.stats["capacity"]), _C.binning_views(b[6], N, R, W, H, _C.stats["capacity"])
    ia, ib = _C.image_views(a[7], W, H), _C.image_views(b[7], W, H)
    # the lists tile by tile (what lies between and behind them in the array -- culled instances' slots -- is not written by either call)
    assert torch.equal(ia["ranges"], ib["ranges"]) and torch.equal(ia["final_T"], ib["final_T"]) and torch.equal(ia["n_contrib"], ib["n_contrib"])
    pa, pb, n_listed = va["point_list"].cpu(), vb["point_list"].cpu(), 0
    for r0, r1 in ia["ranges"].cpu().tolist():
        assert 0 <= r0 <= r1 <= R and torch.equal(pa[r0:r1], pb[r0:r1])
        n_listed += r1 - r0
    assert n_listed > 0
    # the packed records of the Gaussians that were preprocessed to the end (a culled row's record is not written), colour slots included
    seen = a[4] > 0
    assert int(seen.sum()) > 0 and torch.equal(_C.geom_views(a[5], N)["rec"][seen], _C.geom_views(b[5], N)["rec"][seen])
    rec = _C.geom_views(b[5], N)["rec"][seen]
    assert torch.equal(rec[:, 6], label.reshape(-1).to(dev)[seen]) and torch.equal(rec[:, 6], rec[:, 7]) and torch.equal(rec[:, 6], rec[:, 8])


def _colors_sum(g, out, gc, dev):
    """the MODE 0 route: dL/dcolors_precomp [P,3] of the three-sum blend, added up over the channels"""
    from egogaussian_amd import _C
    R, color, depth, alpha, radii, geom, binning, img = out
    e = torch.empty(0, device=dev)
    res = _C.rasterize_gaussians_backward(g["bg"], g["means3D"], radii, g["colors_precomp"], g.get("scales", e), g.get("rotations", e),
                                          g["scale_modifier"], g.get("cov3D_precomp", e), g["viewmatrix"], g["projmatrix"], g["tanfovx"],
                                          g["tanfovy"], gc.to(dev), e, e, e, g["sh_degree"], g["campos"], geom, R, binning, img, alpha, False,
                                          grad_mask=_C.GRAD_COLORS)
    return res[1].double().sum(1)


def _label_backward(out, H, W, **kw):
    from egogaussian_amd import _C
    R, color, depth, alpha, radii, geom, binning, img = out
    return _C.backward_label(radii, geom, R, binning, img, H, W, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_case(N, H, W, seed, mode, smul):
    d = make_inputs(N, H, W, seed, 0, mode, scale_mul=smul)
    o, st = oracle_forward(d)
    grads = seeded_grads(H, W, seed + 10)
    gb = o.backward(st, grads[0], None, None)
    return d, grads, np.asarray(gb["dL_dcolor"], dtype=np.float64).sum(1)


@pytest.mark.parametrize("N,H,W,seed,mode,smul", [(2000, 96, 128, 3, "col_sr", 2.0), (3000, 70, 100, 1, "col_sr", 4.0), (2000, 64, 80, 5, "col_cov", 3.0)])
@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "tile-culling"])
def test_scalar_backward_with_upstream_planes(N, H, W, seed, mode, smul, cull):
    dev = _dev()
    d, grads, ref = _oracle_case(N, H, W, seed, mode, smul)
    with tile_culling(cull):
        g, out = hip_forward(d, dev)
        dl = _label_backward(out, H, W, dL_dout_color=grads[0].to(dev))
        three = _colors_sum(g, out, grads[0], dev)
    torch.cuda.synchronize()
    e_or = rel_err(dl.cpu().numpy(), ref)
    e_three = rel_err(dl.cpu().numpy(), three.cpu().numpy())
    print(f"\n[{N}@{W}x{H} {mode}] scalar dL/dlabel: vs oracle {e_or:.1e}, vs the three sums of the colours-only blend {e_three:.1e}")
    assert e_three < 2e-6 and e_or < 1e-4
    radii = out[4]
    assert int((radii <= 0).sum()) > 0 and float(dl[radii <= 0].abs().max()) == 0.0


def test_hot_replica_lines():
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 300, 272, 256                                             # 16 x 17 = 272 tiles: a box over the image is hot (>= 256 tiles)
    d = make_inputs(N, H, W, 2, 0, "col_sr", scale_mul=1.0)
    _, first = hip_forward(d, dev)
    big = torch.nonzero(first[4] > 0).reshape(-1)[:3].cpu()
    assert big.numel() == 3
    d["scales"][big] = 10.0; d["opacities"][big] = 0.5
    g, out = hip_forward(d, dev)
    code = _C.geom_views(out[5], N)["clamped"][big.to(dev)] >> 3
    assert bool((code != 0).all()), "the three screen-filling Gaussians accumulate through replica lines"
    gc = seeded_grads(H, W, 4)[0]
    dl = _label_backward(out, H, W, dL_dout_color=gc.to(dev))
    three = _colors_sum(g, out, gc, dev)
    torch.cuda.synchronize()
    e = rel_err(dl.cpu().numpy(), three.cpu().numpy())
    e_hot = float((dl[big.to(dev)].double() - three[big.to(dev)]).abs().max() / three[big.to(dev)].abs().max())
    print(f"\nhot lines: dL/dlabel vs the three-sum route {e:.1e} (hot rows alone {e_hot:.1e})")
    assert e < 2e-6 and e_hot < 2e-6


def _label_scene(N, H, W, seed, smul, dev, border=False):
    """a label render through the scalar colour path -> (out, label, mask, gate)"""
    from egogaussian_amd import _C
    d = make_inputs(N, H, W, seed, 0, "col_sr", scale_mul=smul)
    gen = torch.Generator().manual_seed(seed + 5)
    label = torch.randn(N, generator=gen) * 3.0
    if border:
        # keep only the splats whose centre lies in the middle third of the image: the tiles along the border get empty lists
        _, probe = _forward(d, dev, scalar_label=label)
        rec = _C.geom_views(probe[5], N)["rec"].cpu()
        keep = (rec[:, 0] > W / 3) & (rec[:, 0] < 2 * W / 3) & (rec[:, 1] > H / 3) & (rec[:, 1] < 2 * H / 3) & (probe[4].cpu() > 0)
        d["opacities"] = torch.where(keep.reshape(-1, 1), d["opacities"], torch.zeros_like(d["opacities"]))
    _, out = _forward(d, dev, scalar_label=label)
    mask = (torch.rand(H, W, generator=gen) > 0.5).float().to(dev)
    gate = torch.rand(H, W, generator=gen)
    gate[: min(16, H), : min(32, W)] = 0.0                              # whole quadrant-waves under the hand mask: they leave early
    return out, label, mask, gate.to(dev)


@pytest.mark.parametrize("N,H,W,seed,smul,border", [(2000, 96, 128, 3, 2.0, False), (1500, 37, 53, 4, 3.0, False), (3000, 112, 144, 6, 0.5, True)],
                         ids=["whole-tiles", "ragged-37x53", "empty-border-tiles"])
@pytest.mark.parametrize("gated", [False, True])
def test_loss_gradient_formed_in_the_blend(N, H, W, seed, smul, border, gated):
    """k_render_backward<3, true> against "k_label_bce_backward's planes, then <3, false>" on the same forward; the value the blend's partial
    sums give is BIT-IDENTICAL to the stand-alone forward's deferred value (both use the tile x quadrant partition and one finishing function)."""
    from egogaussian_amd import _C
    dev = _dev()
    out, label, mask, gate = _label_scene(N, H, W, seed, smul, dev, border)
    gate = gate if gated else None
    image = out[1]
    if border:
        rng = _C.image_views(out[7], W, H)["ranges"]
        assert int((rng[:, 0] == rng[:, 1]).sum()) > 0, "the case needs tiles no splat reaches"
    up = torch.full((1,), UP, device=dev)
    _, partial = _C.label_bce_forward(image, mask, defer_value=True)
    ref_loss = torch.full((1,), -1.0, device=dev)
    planes = _C.label_bce_backward(image, mask, up, gate, deferred_partial=partial, deferred_loss=ref_loss)
    dl_ref = _label_backward(out, H, W, dL_dout_color=planes)
    loss = torch.full((1,), -2.0, device=dev); run = torch.full((1,), 10.0, device=dev)
    st, keep = _C.label_loss_struct(image, mask, up, gate, None, loss, run)
    dl = _label_backward(out, H, W, label_loss=st)
    torch.cuda.synchronize()
    l64, _ = _mirror64(image, mask, gate, UP)
    e = rel_err(dl.cpu().numpy(), dl_ref.cpu().numpy())
    print(f"\n[{N}@{W}x{H} gated={gated}] in-blend dL/dlabel vs planes route {e:.1e}; loss {float(loss):.8f} (float64 mirror {l64:.8f})")
    assert float(dl_ref.abs().max()) > 0 and e < 2e-6
    assert torch.equal(loss, ref_loss), "same partition, same finishing function: the same bits"
    assert torch.equal(keep[4], partial), "every quadrant partial, the ones of empty tiles and of quadrants outside the image included"
    assert abs(float(loss) - l64) <= 1e-5 * max(1.0, abs(l64))
    assert torch.equal(run, torch.full((1,), 10.0, device=dev) + loss)


@pytest.mark.parametrize("active_rows", ["N-17", -1, 0, 1, 256, "N", "N+9"])
def test_adam_step_in_the_finish_launch_is_bit_identical(active_rows):
    """active_rows: the live-row word -- below zero, zero, one row, a workgroup edge of k_label_finish, all rows, more rows than there are.
    The rows that take the step are those below min(N, max(word, 0)); the step is counted whatever the word holds, by the prologue's
    egs_adam_tick as by k_adam."""
    from egogaussian_amd import _C, lib, _hip
    dev = _dev()
    N, H, W = 3000, 70, 100
    word = {"N-17": N - 17, "N": N, "N+9": N + 9}.get(active_rows, active_rows)
    live = min(N, max(word, 0))
    out, label0, mask, gate = _label_scene(N, H, W, 1, 4.0, dev)
    radii = out[4]
    assert int((radii <= 0).sum()) > 17, "rows that were never rendered: their gradient is 0, their moments still decay"
    L = lib.load()
    b1, b2, eps = 0.9, 0.999, 1e-15
    gen = torch.Generator().manual_seed(11)
    p = label0.clone().to(dev); m = (torch.randn(N, generator=gen) * 1e-3).to(dev); v = (torch.rand(N, generator=gen) * 1e-6).to(dev)
    step = torch.full((1,), 4.0, device=dev); lr = torch.full((1,), 2.5e-3, device=dev); coef = torch.zeros(12, device=dev)
    active = torch.tensor([word], dtype=torch.int32, device=dev)
    m0, v0 = m.clone(), v.clone()
    leaf = lib.AdamLeaf(); leaf.param, leaf.exp_avg, leaf.exp_avg_sq, leaf.lr, leaf.step = p.data_ptr(), m.data_ptr(), v.data_ptr(), lr.data_ptr(), step.data_ptr()
    G = int(L.egs_adam_workgroups(N))
    for it in range(3):
        rp, rm, rv, rstep = p.clone(), m.clone(), v.clone(), step.clone()
        counters = torch.full((G,), int(round(float(step))), dtype=torch.int32, device=dev)
        up = torch.full((1,), 1.0 + it, device=dev)
        st, keep = _C.label_loss_struct(out[1], mask, up, gate)
        g = _label_backward(out, H, W, label_loss=st, adam=(leaf, b1, b2, eps, coef), active_rows=active)
        arr = lambda t: (C.c_void_p * 1)(t.data_ptr())
        lib.check(L.egs_adam_step_capturable(1, arr(rp), arr(g), arr(rm), arr(rv), (C.c_int64 * 1)(N), arr(rstep), arr(lr), arr(counters), b1, b2, eps,
                                             None, C.c_void_p(active.data_ptr()), (C.c_int32 * 1)(1), _hip.stream_of(dev)))
        torch.cuda.synchronize()
        assert float(g[radii <= 0].abs().max()) == 0.0 and float(g.abs().max()) > 0
        assert float(step) == 5.0 + it and torch.equal(step, rstep)
        assert torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv), f"call {it}: fused and stand-alone Adam disagree"
        never = (radii <= 0)[:live]
        assert live < N - 17 or bool(never.any())
        if bool(never.any()):
            assert bool((m[:live][never] != 0).any()) and bool((p[:live][never] != label0.to(dev)[:live][never]).any()), "dense Adam: zero-gradient rows move on momentum"
        assert bool((m[:live] != m0[:live]).all()), "every live row is stepped: its first moment decays whatever its gradient"
    assert torch.equal(p[live:], label0.to(dev)[live:]), "rows at and beyond active_rows are untouched"
    assert torch.equal(m[live:], m0[live:]) and torch.equal(v[live:], v0[live:]), "... and so are their moments"


def test_overflow_word_voids_the_step():
    from egogaussian_amd import _C, lib
    dev = _dev()
    N, H, W = 1500, 37, 53
    out, label0, mask, gate = _label_scene(N, H, W, 4, 3.0, dev)
    p = label0.clone().to(dev); m = torch.zeros(N, device=dev); v = torch.zeros(N, device=dev)
    step = torch.full((1,), 7.0, device=dev); lr = torch.full((1,), 1e-2, device=dev); coef = torch.zeros(12, device=dev)
    leaf = lib.AdamLeaf(); leaf.param, leaf.exp_avg, leaf.exp_avg_sq, leaf.lr, leaf.step = p.data_ptr(), m.data_ptr(), v.data_ptr(), lr.data_ptr(), step.data_ptr()
    guard = _C.StepGuard(dev); guard.overflow[0] = 1
    g = torch.full((N,), 123.0, device=dev)
    st, keep = _C.label_loss_struct(out[1], mask, torch.ones(1, device=dev), gate)
    _label_backward(out, H, W, label_loss=st, adam=(leaf, 0.9, 0.999, 1e-15, coef), guard=guard, dlabel=g)
    torch.cuda.synchronize()
    assert float(step) == 7.0 and torch.equal(p, label0.to(dev)) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    assert bool((g == 123.0).all()), "an overflowed frame writes no gradient"
    rc = lib.load().egs_backward_label(N, out[0], W, H, None, None, None, None, None, None, None, None, 0.9, 0.999, 1e-15, None, None, None, None, None, 0)
    assert rc == -2, "neither upstream planes nor a loss: EGS_ERR_MODE"


# ---- the captured label step -----------------------------------------------------------------------------------------------------
NG, HG, WG = 3000, 70, 100
OTHERS = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def _label_model(dev, lr=1e-2, seed=1):
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.scene_synth import make_scene, SynthGaussians
    scene = make_scene(NG, HG, WG, seed); scene["log_scale"] += np.log(4.0).astype(np.float32)
    pc = SynthGaussians(scene, device=dev)
    with torch.no_grad():
        pc._label += (torch.randn(NG, 1, generator=torch.Generator().manual_seed(seed + 3)) * 0.5).to(dev)
    opt = pc.training_setup(FusedAdam, capturable=True)
    for g in opt.param_groups:
        if g["name"] == "label":
            g["lr"] = lr
    return pc, opt


def _frames(dev, n, seed=20):
    """n frames: camera, object mask (the label render of a "true" labelling, thresholded), gate"""
    from egogaussian_amd.renderer import get_render_label
    from egogaussian_amd.scene_synth import make_camera
    pc, _ = _label_model(dev)
    gen = torch.Generator().manual_seed(seed)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        pc._label.copy_(torch.where(pc._xyz[:, :1] > pc._xyz[:, :1].median(), 4.0, -4.0))
        out = []
        for k in range(n):
            cam = make_camera(k + 1, HG, WG, device=dev)
            mask = (get_render_label(cam, pc, bg).mean(0) > 0).float()
            gate = (torch.rand(HG, WG, generator=gen) > 0.2).float().to(dev)
            out.append((cam, mask, gate))
    return out


def _adam_reference(p, m, v, step, lr_t, g, betas, eps, dev):
    """egs_adam_step_capturable on (clones of) the state with gradient g"""
    from egogaussian_amd import lib, _hip
    L = lib.load()
    n = p.numel()
    counters = torch.full((int(L.egs_adam_workgroups(n)),), int(round(float(step))), dtype=torch.int32, device=dev)
    arr = lambda t: (C.c_void_p * 1)(t.data_ptr())
    lib.check(L.egs_adam_step_capturable(1, arr(p), arr(g.contiguous()), arr(m), arr(v), (C.c_int64 * 1)(n), arr(step), arr(lr_t), arr(counters),
                                         float(betas[0]), float(betas[1]), float(eps), None, None, None, _hip.stream_of(dev)))


def _label_state(pc, opt):
    st = opt.state[pc._label]
    return pc._label.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone()


def test_captured_label_step():
    from egogaussian_amd import _C
    from egogaussian_amd.graph import GraphedTrainStep, pack_label_frame
    dev = _dev()
    bg = torch.zeros(3, device=dev)
    frames = _frames(dev, 4)
    pc, opt = _label_model(dev)
    group = [g for g in opt.param_groups if g["name"] == "label"][0]
    step = GraphedTrainStep(pc, opt, bg, label_phase=True, gated=True).capture(frames[0][0], obj_mask=frames[0][1], gate=frames[0][2], warmup=1,
                                                                               capacity_margin=2.0)
    others = {a: getattr(pc, a).detach().clone() for a in OTHERS}
    other_state = {a: {k: (t.clone() if torch.is_tensor(t) else t) for k, t in opt.state.get(getattr(pc, a), {}).items()} for a in OTHERS}
    lr_t = opt._aux_of(pc._label)["lr"]
    one = torch.ones(1, device=dev)
    for k in (1, 2, 3):
        cam, mask, gate = frames[k]
        p0, m0, v0, s0 = _label_state(pc, opt)
        if k == 2:
            step(pack_label_frame(cam, mask, gate))
        else:
            step(cam, obj_mask=mask, gate=gate)
        torch.cuda.synchronize()
        g = step.label_grad.clone()
        # the gradient against the eager pieces on the image the replay left: the stand-alone planes, then the scalar blend without the loss
        keep = step._label_keeps[-1]
        planes = _C.label_bce_backward(step.image, mask, one, gate)
        g_ref = _C.backward_label(step.radii, keep[6], step.capacity, keep[7], keep[8], HG, WG, dL_dout_color=planes)
        torch.cuda.synchronize()
        e = rel_err(g.cpu().numpy(), g_ref.cpu().numpy())
        l64, _ = _mirror64(step.image, mask, gate, 1.0)
        print(f"\nreplay {k}: dL/dlabel vs eager pieces {e:.1e}; loss {float(step.loss):.8f} (float64 mirror {l64:.8f}); R = {step.last_instance_count()}")
        assert float(g.abs().max()) > 0 and e < 2e-6
        assert abs(float(step.loss) - l64) <= 1e-5 * max(1.0, abs(l64))
        _adam_reference(p0, m0, v0, s0, lr_t, g, group["betas"], group["eps"], dev)
        torch.cuda.synchronize()
        p1, m1, v1, s1 = _label_state(pc, opt)
        assert float(s1) == float(s0) == 1.0 + k
        assert torch.equal(p1.view(-1), p0.view(-1)) and torch.equal(m1, m0) and torch.equal(v1, v0), f"replay {k}: the step is not egs_adam_step_capturable's"
    assert step.ok()
    for a in OTHERS:
        assert torch.equal(getattr(pc, a).detach(), others[a]) and getattr(pc, a).grad is None, f"{a} moved"
        now = opt.state.get(getattr(pc, a), {})
        assert set(now) == set(other_state[a]) and all(torch.equal(now[k], t) if torch.is_tensor(t) else now[k] == t for k, t in other_state[a].items()), f"optimizer state of {a}"
    # a frame that outgrows the captured capacity: nothing of the label moves, ok() says so
    small = max(step.last_instance_count() // 2, 1)
    step = GraphedTrainStep(pc, opt, bg, label_phase=True, gated=True).capture(frames[0][0], obj_mask=frames[0][1], gate=frames[0][2], warmup=1, capacity=small)
    before = _label_state(pc, opt)
    step(frames[1][0], obj_mask=frames[1][1], gate=frames[1][2])
    torch.cuda.synchronize()
    assert step.capacity == small and step.last_frame_overflowed() and not step.ok()
    assert all(torch.equal(a, b) for a, b in zip(before, _label_state(pc, opt))), "a clipped frame takes no step and counts none"


def test_captured_label_step_recaptures_after_an_overflow():
    """check() of a label step whose replayed frame outgrew the (forced-small) capacity: it re-captures once with room, on the SAME static
    buffers, and the step works afterwards -- a further replay moves the label and nothing else."""
    from egogaussian_amd.graph import GraphedTrainStep
    dev = _dev()
    bg = torch.zeros(3, device=dev)
    frames = _frames(dev, 3)
    pc, opt = _label_model(dev)
    cap = dict(obj_mask=frames[0][1], gate=frames[0][2], warmup=1)
    sized = GraphedTrainStep(pc, opt, bg, label_phase=True, gated=True).capture(frames[0][0], capacity_margin=2.0, **cap)
    sized(frames[1][0], obj_mask=frames[1][1], gate=frames[1][2])
    torch.cuda.synchronize()
    count = sized.last_instance_count()
    small = max(count // 2, 1)
    step = GraphedTrainStep(pc, opt, bg, label_phase=True, gated=True).capture(frames[0][0], capacity=small, **cap)
    ptrs = (step.obj_mask.data_ptr(), step.gate.data_ptr(), step.cam.packed.data_ptr())
    step(frames[1][0], obj_mask=frames[1][1], gate=frames[1][2])
    torch.cuda.synchronize()
    assert step.capacity == small and step.last_frame_overflowed() and not step.ok()
    assert step.check() is False
    print(f"\ninstances {count}, capacity {small} -> {step.capacity}")
    assert step.recaptures == 1 and step.skipped_frames_seen == 1 and step.capacity > small and step.capacity >= count and step.ok()
    assert (step.obj_mask.data_ptr(), step.gate.data_ptr(), step.cam.packed.data_ptr()) == ptrs
    assert torch.equal(step.obj_mask, frames[1][1]) and torch.equal(step.gate, frames[1][2])      # the buffers kept their contents too
    assert step.visibility_filter is None and step.viewspace_grad is None and len(step.label_grads) == len(step._label_keeps) == 1
    others = {a: getattr(pc, a).detach().clone() for a in OTHERS}
    p0, _, _, s0 = _label_state(pc, opt)
    step(frames[2][0], obj_mask=frames[2][1], gate=frames[2][2])
    torch.cuda.synchronize()
    p1, _, _, s1 = _label_state(pc, opt)
    assert step.ok() and step.check() is True and step.recaptures == 1 and not step.last_frame_overflowed()
    assert float(s1) == float(s0) + 1.0 and not torch.equal(p1, p0) and float(step.label_grad.abs().max()) > 0
    for a in OTHERS:
        assert torch.equal(getattr(pc, a).detach(), others[a]) and getattr(pc, a).grad is None, f"{a} moved"


def test_captured_label_step_two_iterations_per_replay():
    from egogaussian_amd.graph import GraphedTrainStep, pack_label_frame
    dev = _dev()
    bg = torch.zeros(3, device=dev)
    frames = _frames(dev, 3)
    pa, oa = _label_model(dev)
    pb, ob = _label_model(dev)
    cap = dict(obj_mask=frames[0][1], gate=frames[0][2], warmup=1, capacity_margin=2.0)
    one = GraphedTrainStep(pa, oa, bg, label_phase=True, gated=True).capture(frames[0][0], **cap)
    two = GraphedTrainStep(pb, ob, bg, label_phase=True, gated=True, steps_per_replay=2).capture(frames[0][0], **cap)
    packed = [pack_label_frame(*frames[k]) for k in (1, 2)]
    la = [float(one(packed[0])), float(one(packed[1]))]
    p0, m0, v0, s0 = _label_state(pb, ob)
    two(torch.stack(packed))
    torch.cuda.synchronize()
    lb = [float(t) for t in two.losses]
    print("\nlosses: two single replays", la, "one replay of two", lb)
    assert all(abs(a - b) <= 1e-5 * max(1.0, abs(a)) for a, b in zip(la, lb))
    group = [g for g in ob.param_groups if g["name"] == "label"][0]
    for g in two.label_grads:                                           # the relation of every single step, step by step
        _adam_reference(p0, m0, v0, s0, ob._aux_of(pb._label)["lr"], g, group["betas"], group["eps"], dev)
    torch.cuda.synchronize()
    p1, m1, v1, s1 = _label_state(pb, ob)
    assert float(s1) == 3.0 and torch.equal(p1.view(-1), p0.view(-1)) and torch.equal(m1, m0) and torch.equal(v1, v0)
    assert float(oa.state[pa._label]["step"]) == 3.0 and one.ok() and two.ok()
    assert rel_err(pa._label.detach().cpu().numpy(), pb._label.detach().cpu().numpy()) < 1e-3


def test_captured_label_phase_trains_like_the_eager_route():
    """200 steps over the same 8 frames in the same order: the captured label step against the eager route (get_render_label + torch's BCE with
    the hook + FusedAdam, code this pull request does not change).  Adam with eps = 1e-15 turns a sign flip of a near-zero gradient into a
    2 lr difference of the parameter, so the mean loss of the last 20 steps is compared, within max(3 x the eager route's own spread over three
    runs, 1e-3 relative)."""
    from egogaussian_amd.graph import GraphedTrainStep, pack_label_frame
    from egogaussian_amd.renderer import get_render_label
    dev = _dev()
    bg = torch.zeros(3, device=dev)
    frames = _frames(dev, 8)
    STEPS = 200

    def eager():
        pc, opt = _label_model(dev)
        bce = torch.nn.BCEWithLogitsLoss()
        losses = []
        for i in range(STEPS):
            cam, mask, gate = frames[i % 8]
            x = get_render_label(cam, pc, bg).mean(0, keepdim=True)
            x.register_hook(lambda gr, gate=gate: gr * gate)
            loss = bce(x, mask[None])
            loss.backward()
            opt.step(); opt.zero_grad()
            losses.append(loss.detach())
        return float(torch.stack(losses[-20:]).mean()), float(losses[0])

    runs = [eager() for _ in range(3)]
    tails = [r[0] for r in runs]
    spread = max(tails) - min(tails)
    pc, opt = _label_model(dev)
    step = GraphedTrainStep(pc, opt, bg, label_phase=True, gated=True).capture(frames[0][0], obj_mask=frames[0][1], gate=frames[0][2], warmup=1,
                                                                               capacity_margin=2.0)
    packed = [pack_label_frame(*f) for f in frames]
    losses = []
    for i in range(1, STEPS):                                           # (the warm-up step of capture() was step 0, on frame 0)
        losses.append(step(packed[i % 8]).clone())
    torch.cuda.synchronize()
    tail = float(torch.stack(losses[-20:]).mean())
    allowed = max(3 * spread, 1e-3 * abs(sum(tails) / 3))
    print(f"\nmean loss of the last 20 of {STEPS} steps: eager {tails} (spread {spread:.2e}; first step {runs[0][1]:.5f}), captured {tail:.6f}; allowed {allowed:.2e}")
    assert step.ok() and float(opt.state[pc._label]["step"]) == STEPS
    assert tails[0] < 0.8 * runs[0][1], "the phase trains: the loss fell"
    assert abs(tail - sum(tails) / 3) <= allowed


def test_autograd_route_scalar_label_render_and_fused_loss():
    """get_render_label(scalar=True) + fused.label_bce_loss through autograd, the loss gradient formed in the blend or by the loss launch, against
    the unchanged route (get_render_label + torch's BCE with the hook).  The per-pixel gradient differs by float32 rounding of the sigmoid
    (a few ulp of 6e-8) and the sums run in another order: 1e-5 max-norm relative.  A second consumer of the image is refused."""
    from egogaussian_amd import fused
    from egogaussian_amd.renderer import get_render_label
    dev = _dev()
    bg = torch.zeros(3, device=dev)
    cam, mask, gate = _frames(dev, 1)[0]
    pc, _ = _label_model(dev)
    ref_img = get_render_label(cam, pc, bg)
    x = ref_img.mean(0, keepdim=True)
    x.register_hook(lambda gr: gr * gate)
    ref = torch.nn.BCEWithLogitsLoss()(x, mask[None])
    ref.backward()
    g_ref = pc._label.grad.clone(); pc._label.grad = None
    run = torch.zeros((), device=dev)
    for in_blend, defer in ((True, True), (True, False), (False, False)):
        img = get_render_label(cam, pc, bg, scalar=True)
        assert torch.equal(img, ref_img.detach())
        loss = fused.label_bce_loss(img, mask, grad_gate=gate, running_sum=run, defer_value=defer, raster_lossgrad=in_blend)
        loss.backward()
        torch.cuda.synchronize()
        g = pc._label.grad.clone(); pc._label.grad = None
        assert g.shape == pc._label.shape
        e = rel_err(g.cpu().numpy(), g_ref.cpu().numpy())
        print(f"\nin_blend={in_blend} deferred={defer}: loss {float(loss):.8f} (torch {float(ref):.8f}), dL/dlabel vs the unchanged route {e:.1e}")
        assert e < 1e-5 and abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    assert abs(float(run) - 3 * float(ref)) <= 1e-4
    assert all(getattr(pc, a).grad is None for a in OTHERS)
    img = get_render_label(cam, pc, bg, scalar=True)
    loss = fused.label_bce_loss(img, mask, raster_lossgrad=True) + img.sum() * 1e-3
    with pytest.raises(RuntimeError, match="another gradient contribution"):
        loss.backward()
