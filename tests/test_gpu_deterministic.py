"""GPU: the deterministic mode of the backward blend (EGS_CALL_DETERMINISTIC, include/egs_raster.h; egogaussian_amd/csrc/det_accum.h).

By default the quadrant-waves of the backward blend add their per-splat sums into the Gaussian's accumulator line with float atomics, in an
order that differs from run to run.  With the flag the blend runs as two integer passes and every output of every backward is the same bits
on every run.  The scenes here are chosen so that the DEFAULT path does differ between runs (splats four times the usual size: most of
them span several tiles and quadrants; screen-filling splats): the module's last test asserts that it did, otherwise "bit-identical" would
be a statement about the scenes and not about the mode.  tests/test_det_accum_cpu.py covers the arithmetic itself."""
import math

import numpy as np
import pytest
import torch

from tests.common import make_inputs, seeded_grads, flip_pixels, check_grads_isolating_flips
from tests.test_gpu_parity import hip_forward, hip_backward, oracle_forward, float64_oracle, check_rows, _dev, TOL
from tests.test_gpu_entropy import _scene, _groups, LEAVES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DET = 0x20                                                            # EGS_CALL_DETERMINISTIC
RUNS = 5
NAMES = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"]
OVERLAP = (3000, 64, 64)                                              # make_inputs(..., scale_mul=4): most splats span several tiles and quadrants
DEFAULT_DIFFERED = {}                                                 # test -> the same runs with the flag clear differed in at least one bit


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    """two lists of tensors (None allowed), bit for bit -- NaN patterns included"""
    return len(a) == len(b) and all((x is None and y is None) or (x.shape == y.shape and torch.equal(_bits(x), _bits(y))) for x, y in zip(a, b))


def _snap(ts):
    return [None if t is None else t.detach().clone() for t in ts]


class deterministic:
    """Run a block with the module default of the backwards set (egogaussian_amd._C.deterministic_backward), as tests/common.py tile_culling does."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from egogaussian_amd import _C
        self.old = _C.deterministic_backward(self.on)

    def __exit__(self, *exc):
        from egogaussian_amd import _C
        _C.deterministic_backward(self.old)


def _upstream(H, W, seed, mode_2, dev):
    gc, gd, ga = seeded_grads(H, W, seed)
    e = torch.empty(0)
    return (gc, gd, ga) if mode_2 else (gc, e, e)                    # MODE 2: depth + alpha gradients exist; MODE 1: colour only


def _repeat(fn, n):
    res = [fn() for _ in range(n)]
    torch.cuda.synchronize()
    return res


def _lists(out, N, W, H):
    """the forward's state a backward reads, as comparable tensors: images, radii, ranges, final_T, n_contrib, the listed part of point_list"""
    from egogaussian_amd import _C
    R, color, depth, alpha, radii, geom, binning, img = out
    iv, bv = _C.image_views(img, W, H), _C.binning_views(binning, N, R, W, H, _C.stats["capacity"])
    rng = iv["ranges"].cpu().numpy().view(np.uint32).astype(np.int64)
    pl = bv["point_list"].cpu()
    listed = torch.cat([pl[a:b] for a, b in rng.tolist()]) if rng.size else pl[:0]
    return [color, depth, alpha, radii, iv["ranges"], iv["final_T"], iv["n_contrib"], listed]


# ---- 1. the overlap scene ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sh_cov", "col_sr"], ids=["sh_cov", "scales-rotations"])
@pytest.mark.parametrize("mode_2", [False, True], ids=["colour-only (MODE 1)", "depth+alpha (MODE 2)"])
def test_overlap_scene_is_bit_identical_run_to_run(mode, mode_2):
    dev = _dev()
    N, H, W = OVERLAP
    d = make_inputs(N, H, W, 0, 0, mode, scale_mul=4.0)
    g, out = hip_forward(d, dev)
    g2, out_flag = hip_forward(d, dev, debug=DET)                     # forwards ignore the bit: image and lists are the default call's
    assert out[0] == out_flag[0] and out[0] > 1.5 * int((out[4] > 0).sum()), "the scene is meant to overlap: several tiles (4 quadrants each) per visible Gaussian"
    assert _same(_lists(out, N, W, H), _lists(out_flag, N, W, H))
    grads = _upstream(H, W, 11, mode_2, dev)
    det = _repeat(lambda: _snap(hip_backward(g, out, grads, dev, debug=DET)), RUNS)
    assert all(float(t.abs().max()) > 0 for t in det[0] if t.numel()), "a gradient array is all zero"
    for k in range(1, RUNS):
        assert _same(det[0], det[k]), f"run {k} differs from run 0 with the flag set"
    plain = _repeat(lambda: _snap(hip_backward(g, out, grads, dev)), RUNS)
    DEFAULT_DIFFERED[f"overlap {mode} {mode_2}"] = any(not _same(plain[0], p) for p in plain[1:])
    # the two paths add the same terms in another order: the standing bar for "the order of the accumulator atomics" (2e-5 of the array's
    # maximum, tests/test_gpu_object_loss.py, tests/test_gpu_fused.py); the parity bars are tests 2 and 3
    for a, b in zip(det[0], plain[0]):
        if a.numel():
            assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max())


# ---- 2. the hot scene: replica lines in use on the default path ----------------------------------------------------------------------
def _hot_scene():
    N, H, W = 1504, 272, 272                                          # 17 x 17 = 289 tiles
    d = make_inputs(N, H, W, 21, 0, "col_sr", scale_mul=1.0)
    big = [0, 1, 2, 700]
    gen = torch.Generator().manual_seed(9)
    d["means3D"][big, 0] = 0.3 * (torch.rand(len(big), generator=gen) - 0.5)
    d["means3D"][big, 1] = 0.3 * (torch.rand(len(big), generator=gen) - 0.5)
    d["means3D"][big, 2] = 3.0 + 3.0 * torch.rand(len(big), generator=gen)
    d["scales"][big] = 3.0 + 2.0 * torch.rand(len(big), 3, generator=gen)
    d["opacities"][big] = (0.3 + 0.3 * torch.rand(len(big), generator=gen)).view(-1, *d["opacities"].shape[1:])
    return d, big, N, H, W


def test_hot_scene_is_bit_identical_and_holds_the_parity_bars():
    from egogaussian_amd import _C
    from tests.test_gpu_trained_scene import _hot_codes
    dev = _dev()
    d, big, N, H, W = _hot_scene()
    o, st = oracle_forward(d)
    rects = st["rects"][big]
    assert ((rects[:, 2] - rects[:, 0]) * (rects[:, 3] - rects[:, 1]) >= 256).all(), "the four large splats' 3-sigma boxes cover 256 tiles or more"
    g, out = hip_forward(d, dev)
    assert out[0] == st["R"] and np.array_equal(out[4].cpu().numpy(), st["radii"])
    assert (_hot_codes(out[5], N, out[4])[big] != 0).all(), "the four large splats accumulate through replica lines on the default path"
    grads = seeded_grads(H, W, 31)
    det = _repeat(lambda: _snap(hip_backward(g, out, grads, dev, debug=DET)), RUNS)
    for k in range(1, RUNS):
        assert _same(det[0], det[k]), f"run {k} differs from run 0 with the flag set"
    plain = _repeat(lambda: _snap(hip_backward(g, out, grads, dev)), RUNS)
    DEFAULT_DIFFERED["hot"] = any(not _same(plain[0], p) for p in plain[1:])
    # parity, at the standing bars.  The harness finds the threshold flips on the float32 oracle's state (its images are the HIP path's to
    # 2e-6; the float64 state's are not, by the float32 rounding of the preprocess); the gradients are held to the float64 oracle's AND,
    # as in every parity test of the suite, to the float32 oracle's.
    iv = _C.image_views(out[7], W, H)
    flip_px = flip_pixels(out[1].cpu().numpy(), iv["final_T"].cpu().numpy(), st)
    st64, g64 = float64_oracle(d, grads)
    gb = o.backward(st, *grads)
    print("\n   hot, deterministic vs float64 oracle: " + check_grads_isolating_flips(NAMES, det[0], g64, st, flip_px, TOL, what="hot / float64")[0])
    print("   hot, deterministic vs float32 oracle: " + check_grads_isolating_flips(NAMES, det[0], gb, st, flip_px, TOL, what="hot / float32")[0])


# ---- 3. config A through the row harness -----------------------------------------------------------------------------------------------
def test_config_A_rows_against_float64():
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 10000, 64, 64
    d = make_inputs(N, H, W, 0, 0, "sh_cov")
    grads = seeded_grads(H, W, 10)
    o, st = oracle_forward(d)
    gb = o.backward(st, *grads)
    g, out = hip_forward(d, dev)
    hb = hip_backward(g, out, grads, dev, debug=DET)
    torch.cuda.synchronize()
    assert out[0] == st["R"] and np.array_equal(out[4].cpu().numpy(), st["radii"])
    flip_px = flip_pixels(out[1].cpu().numpy(), _C.image_views(out[7], W, H)["final_T"].cpu().numpy(), st)
    near = []
    rep = check_grads_isolating_flips(NAMES, hb, gb, st, flip_px, TOL, what="config A, deterministic", near_out=near)[0]
    print("\n   grads: " + rep)
    print("   " + check_rows(d, grads, NAMES, hb, st, gb, near[0], "config A, deterministic"))


# ---- 4. the other entry points --------------------------------------------------------------------------------------------------------
def _three(fn):
    res = _repeat(fn, 3)
    assert all(t is None or bool(torch.isfinite(t).all()) for t in res[0]) and any(t is not None and t.numel() and float(t.abs().max()) > 0 for t in res[0])
    assert _same(res[0], res[1]) and _same(res[0], res[2]), "three runs with the flag set differ"


def test_colours_only_backward_of_the_label_call():
    """get_render_label's backward (MODE 0): colors_precomp the only differentiable input."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = OVERLAP
    d = make_inputs(N, H, W, 0, 0, "col_sr", scale_mul=4.0)
    g, out = hip_forward(d, dev)
    R, color, depth, alpha, radii, geom, binning, img = out
    gc = seeded_grads(H, W, 12)[0].to(dev)
    e = torch.empty(0, device=dev)

    def run():
        res = _C.rasterize_gaussians_backward(g["bg"], g["means3D"], radii, g["colors_precomp"], g["scales"], g["rotations"], g["scale_modifier"], e,
                                              g["viewmatrix"], g["projmatrix"], g["tanfovx"], g["tanfovy"], gc, e, e, e, g["sh_degree"], g["campos"],
                                              geom, R, binning, img, alpha, DET, grad_mask=_C.GRAD_COLORS)
        assert res[0] is None and res[2] is None, "the colours-only route was not taken"
        return _snap([res[1]])
    _three(run)


def _model_frame():
    """the overlap scene as a model: (student scene, cameras, ground truths, background)"""
    return _scene(OVERLAP[0], OVERLAP[1], OVERLAP[2], seed=0, n_cams=2, smul=4.0)


def test_label_step_with_the_loss_formed_in_the_blend():
    """get_render_label(scalar=True) + fused.label_bce_loss(raster_lossgrad=True): the scalar blend (MODE 3, LG) and dL/dlabel."""
    from egogaussian_amd.scene_synth import SynthGaussians
    from egogaussian_amd.renderer import get_render_label
    from egogaussian_amd import fused
    student, cams, gts, bg = _model_frame()
    H, W = OVERLAP[1], OVERLAP[2]
    gen = torch.Generator().manual_seed(4)
    label0 = torch.randn(OVERLAP[0], 1, generator=gen).to(DEV)
    mask = (torch.rand(H, W, generator=gen) > 0.5).float().to(DEV)

    def run():
        pc = SynthGaussians(student, device=DEV)
        with torch.no_grad():
            pc._label.copy_(label0)
        with deterministic():
            loss = fused.label_bce_loss(get_render_label(cams[0], pc, bg, scalar=True), mask, raster_lossgrad=True)
            loss.backward()
        return _snap([pc._label.grad, loss])
    _three(run)


def _leaf_grads(pc):
    return _snap([getattr(pc, a).grad for a in LEAVES])


def test_object_stage_loss_formed_in_the_blend():
    """fused.object_stage_loss(raster_lossgrad=True): the blend forms dL/dimage and dL/dalpha itself (MODE 2, LG)."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import object_stage_loss
    student, cams, gts, bg = _model_frame()
    H, W = OVERLAP[1], OVERLAP[2]
    mask = torch.zeros(H, W, device=DEV)
    mask[H // 4:3 * H // 4, W // 4:3 * W // 4] = 1.0

    def run():
        pc = SynthGaussians(student, device=DEV)
        with deterministic():
            out = render(cams[0], pc, Pipe, bg)
            loss = object_stage_loss(out["render"], out["alpha"], gts[0], mask, 0.2, lambda_image=0.7, lambda_l1_alpha=0.3, lambda_l2_alpha=0.2,
                                     defer_value=True, raster_prologue=True, raster_lossgrad=True)
            loss.backward()
        return _leaf_grads(pc) + _snap([out["viewspace_points"].grad, loss])
    _three(run)


def test_entropy_variant():
    """render(opacity_entropy=) with the image loss's gradient formed in the blend (egs_backward_entropy_lossgrad), statistics included."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    student, cams, gts, bg = _model_frame()

    def run():
        pc = SynthGaussians(student, device=DEV)
        with deterministic():
            out = render(cams[0], pc, Pipe, bg, fused_densify_stats=True, opacity_entropy=0.1)
            l1_ssim_loss(out["render"], gts[0], 0.2, raster_prologue=True, raster_lossgrad=True).backward()
        return _leaf_grads(pc) + _snap([out["viewspace_points"].grad, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D])
    _three(run)


def _adam_state(pc, opt, stats=False):
    out = []
    for a in LEAVES:
        p = getattr(pc, a)
        out += [p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"]]
    if stats:
        out += [pc.xyz_gradient_accum, pc.denom, pc.max_radii2D]
    return _snap(out)


def test_adam_inside_the_backward():
    """egs_backward_adam: parameters and moments after one step taken inside the backward."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.optim import FusedAdam
    student, cams, gts, bg = _model_frame()

    def run():
        pc = SynthGaussians(student, device=DEV)
        opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
        with deterministic():
            out = render(cams[0], pc, Pipe, bg, optimizer=opt)
            l1_ssim_loss(out["render"], gts[0], 0.2, raster_prologue=True, raster_lossgrad=True).backward()
            opt.step()
        assert all(getattr(pc, a).grad is None for a in LEAVES), "the leaves were meant to step inside the backward"
        assert not torch.equal(pc._opacity.detach().cpu().reshape(-1), torch.tensor(student["opacity_logit"]).reshape(-1)), "nothing was stepped"
        return _adam_state(pc, opt)
    _three(run)


# ---- 5. the captured step ---------------------------------------------------------------------------------------------------------------
def _captured(student, cams, gts, bg, deterministic_flag, replays=30, **kw):
    from egogaussian_amd.scene_synth import SynthGaussians
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    pc = SynthGaussians(student, device=DEV)
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    step = GraphedTrainStep(pc, opt, bg, 0.2, deterministic=deterministic_flag, **kw)
    step.capture(cams[0], gts[0], warmup=1, capacity_cams=cams)
    spr = kw.get("steps_per_replay", 1)
    frames = [pack_frame(c, t) for c, t in zip(cams, gts)]
    for i in range(replays):
        step(frames[i % len(frames)] if spr == 1 else torch.stack([frames[(i + k) % len(frames)] for k in range(spr)]))
    torch.cuda.synchronize()
    assert step.ok()
    assert float(opt.state[pc._opacity]["step"]) == 1 + replays * spr
    return _adam_state(pc, opt, stats=bool(kw.get("densify_stats")))


@pytest.mark.parametrize("kw", [{}, dict(steps_per_replay=3), dict(densify_stats=True)], ids=["single", "three-per-replay", "densify-stats"])
def test_captured_step_replays_to_the_same_bits(kw):
    """GraphedTrainStep(deterministic=True): 30 replays from the seeded start, twice in one process with fresh models."""
    student, cams, gts, bg = _model_frame()
    a = _captured(student, cams, gts, bg, True, **kw)
    b = _captured(student, cams, gts, bg, True, **kw)
    assert all(bool(torch.isfinite(t).all()) for t in a)
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if not _same([x], [y])]
    assert not bad, f"state tensors {bad} differ between two runs of the deterministic captured step"
    if not kw:
        p, q = _captured(student, cams, gts, bg, False), _captured(student, cams, gts, bg, False)
        DEFAULT_DIFFERED["captured"] = not _same(p, q)


# ---- 6. non-finite upstream gradients -------------------------------------------------------------------------------------------------
def test_nan_pixel_gives_the_same_nan_rows_and_leaves_the_others_alone():
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = OVERLAP
    d = make_inputs(N, H, W, 0, 0, "sh_cov", scale_mul=4.0)
    g, out = hip_forward(d, dev)
    clean_up = _upstream(H, W, 11, False, dev)
    y, x = 20, 37
    bad_up = tuple(t.clone() for t in clean_up)
    bad_up[0][1, y, x] = float("nan")
    clean = _snap(hip_backward(g, out, clean_up, dev, debug=DET))
    runs = _repeat(lambda: _snap(hip_backward(g, out, bad_up, dev, debug=DET)), 2)
    assert _same(runs[0], runs[1]), "the NaN rows differ between two runs"
    # the rows the pixel's chain can reach: the list of its tile
    iv, bv = _C.image_views(out[7], W, H), _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"])
    r0, r1 = iv["ranges"].cpu().numpy().view(np.uint32).astype(np.int64)[(y // 16) * ((W + 15) // 16) + x // 16].tolist()
    reach = torch.zeros(N, dtype=torch.bool, device=dev)
    reach[bv["point_list"][r0:r1].long()] = True
    assert 0 < int(reach.sum()) < N
    nan_rows = torch.zeros(N, dtype=torch.bool, device=dev)
    for t, c in zip(runs[0], clean):
        if t.shape[0] != N:
            continue
        assert bool(torch.isfinite(c).all())
        row_nan = ~torch.isfinite(t.reshape(N, -1)).all(1)
        assert not bool((row_nan & ~reach).any()), "a row the NaN pixel's chain does not reach is not finite"
        same = (_bits(t).reshape(N, -1) == _bits(c).reshape(N, -1)).all(1)
        assert bool(same[~row_nan].all()), "a finite row differs from the clean run's bits"
        nan_rows |= row_nan
    assert int(nan_rows.sum()) > 0, "the NaN reached no row"


# ---- 7. the condition on the scenes ------------------------------------------------------------------------------------------------------
def test_zz_default_path_differed_on_these_scenes():
    """Not a measurement: the runs of tests 1, 2 and 5 repeated with the flag clear must have differed in at least one bit somewhere --
    otherwise the scenes are too tame to show anything and have to be made denser.  (Run alone, it makes the overlap comparison itself.)"""
    if not DEFAULT_DIFFERED:
        test_overlap_scene_is_bit_identical_run_to_run("sh_cov", True)
    print("\n   default path differed run to run: " + ", ".join(f"{k}: {v}" for k, v in DEFAULT_DIFFERED.items()))
    assert any(DEFAULT_DIFFERED.values()), "the default path was bit-identical on every scene: the scenes show nothing"
