"""GPU: the evaluation sweep (egogaussian_amd/evaluate.py EvalPass) on a small posed scene -- ~2 000 Gaussians at 64x48, six frames with their
own camera, object pose and hand mask: captured against eager, both against losses.eval_metrics on the host, an overflowed frame rendered
again, the project's 0.05 dB against the oracle chain, one host read per sweep."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import eval_anchor as EA
from tests.test_gpu_motion import _pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, W, F = 2000, 48, 64, 6
FRAMES = (10, 60, 110, 160, 210, 260)
N_EL = 3 * H * W


@functools.lru_cache(maxsize=None)
def _scene():
    """-> dict: student scene, is_object, cameras, poses, ground truths (8-bit values, as read from a PNG), keeps, packed frames."""
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.graph import pack_frame
    from egogaussian_amd.losses import quantize8
    from egogaussian_amd import motion
    teacher = make_scene(N, H, W, 3); teacher["log_scale"] += math.log(3.0)
    student = perturb_student(teacher)
    gen = torch.Generator().manual_seed(11)
    is_obj = (torch.rand(N, 1, generator=gen) < 0.3).float().to(DEV)
    is_obj[0, 0] = 0.0
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in FRAMES]
    Ts = [_pose(0.1 + 0.07 * k, (0.5 - 0.1 * k, -0.3 + 0.05 * k, 0.4)).to(DEV) for k in range(F)]
    gts, keeps = [], []
    with torch.no_grad():
        for k in range(F):
            tpc = SynthGaussians(teacher, device=DEV, requires_grad=False)
            tpc._xyz = motion.move_points(tpc._xyz, Ts[k][:3], is_obj == 1)
            gts.append(quantize8(render(cams[k], tpc, Pipe, bg)["render"]).float() / 255)
            keep = torch.ones(H, W, device=DEV)
            y0, x0 = int(torch.randint(0, H - 16, (1,), generator=gen)), int(torch.randint(0, W - 20, (1,), generator=gen))
            keep[y0:y0 + 10 + 2 * k, x0:x0 + 12 + 3 * k] = 0.0             # the hand: a rectangle of its own per frame
            keeps.append(keep)
    frames = [pack_frame(cams[k], gts[k], accum_R=Ts[k][:3, :3].contiguous(), gate=keeps[k], accum_T=Ts[k]) for k in range(F)]
    return dict(student=student, is_obj=is_obj, bg=bg, cams=cams, Ts=Ts, gts=gts, keeps=keeps, frames=frames)


def _model():
    from egogaussian_amd.scene_synth import SynthGaussians
    s = _scene()
    pc = SynthGaussians(s["student"], device=DEV)
    pc._is_object = s["is_obj"]
    return pc


def _pass(graphed, **kw):
    from egogaussian_amd.evaluate import EvalPass
    s = _scene()
    ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1, graphed=graphed, keep_images=True)
    return ev, ev.run(s["frames"], s["cams"][0], **kw)


@functools.lru_cache(maxsize=None)
def _sweeps():
    """(captured, eager, the eager renders on the host and losses.eval_metrics of them in float64) -- computed once, read-only."""
    from egogaussian_amd.scene_synth import Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.motion import ObjectMotion
    from egogaussian_amd.losses import eval_metrics
    s = _scene()
    ev_g, g = _pass(True)
    ev_e, e = _pass(False)
    pc = _model()
    host = []
    with torch.no_grad():
        for k in range(F):
            img = render(s["cams"][k], pc, Pipe, s["bg"], rot_cov=True, which_object=1, object_motion=ObjectMotion(s["Ts"][k]), color_only=True)["render"]
            host.append((img.cpu(), eval_metrics(img.cpu().double(), s["gts"][k].cpu().double(), s["keeps"][k].cpu())))
    torch.cuda.synchronize()
    return (ev_g, g), (ev_e, e), host


def test_captured_rows_equal_eager_rows_and_the_host_figures():
    (ev_g, g), (ev_e, e), host = _sweeps()
    s = _scene()
    assert g["rerendered"] == [] and e["rerendered"] == [] and (g["instances"] > 0).all() and (e["instances"] == 0).all()
    assert len(set(int(v) for v in g["sse"])) == F, "the six frames are not distinct"
    for k in range(F):
        print(f"frame {k}: sse {int(g['sse'][k])} / {int(e['sse'][k])} / {int(host[k][1]['sse'])}, ssim {g['ssim'][k]:.9f} / {e['ssim'][k]:.9f} / "
              f"{float(host[k][1]['ssim']):.9f}, psnr {g['psnr'][k]:.4f}, instances {int(g['instances'][k])}")
        assert int(g["sse"][k]) == int(e["sse"][k]) == int(host[k][1]["sse"])
        assert abs(g["ssim"][k] - e["ssim"][k]) <= EA.SSIM_BAR and abs(e["ssim"][k] - float(host[k][1]["ssim"])) <= EA.SSIM_BAR
        assert abs(g["psnr"][k] - float(host[k][1]["psnr"])) <= 1e-9
    assert g["mean_psnr"] == float(np.mean(g["psnr"])) and g["mean_ssim"] == float(np.mean(g["ssim"]))
    # the uint8 renders: losses.quantize8 of the eager render, byte for byte
    from egogaussian_amd.losses import quantize8
    assert g["images"].dtype == torch.uint8 and tuple(g["images"].shape) == (F, 3, H, W)
    for k in range(F):
        assert torch.equal(g["images"][k].cpu(), quantize8(host[k][0])) and torch.equal(e["images"][k].cpu(), quantize8(host[k][0]))
    assert s["keeps"][0].min() == 0.0                                       # (the hand masks do gate something)


def test_one_host_read_per_sweep():
    """Counted by wrapping the result read: one per sweep, of all F rows at once -- also on a second sweep through the same captured graph."""
    from egogaussian_amd.evaluate import EvalPass
    s = _scene()
    ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1)
    calls, inner = [], ev._read_rows
    ev._read_rows = lambda rows: (calls.append(int(rows.shape[0])), inner(rows))[1]
    r1 = ev.run(s["frames"], s["cams"][0])
    graph = ev.graph
    assert calls == [F] and ev.host_reads == 1 and graph is not None
    r2 = ev.run(s["frames"], s["cams"][0])
    assert calls == [F, F] and ev.host_reads == 2 and ev.graph is graph, (calls, ev.host_reads)      # no re-capture either
    assert np.array_equal(r1["sse"], r2["sse"]) and np.array_equal(r1["ssim"], r2["ssim"])           # bit-identical rows, sweep to sweep


def test_overflowed_frame_is_flagged_rendered_again_and_matches_eager():
    """Captured with an instance capacity between the two largest frames' counts: exactly the largest frame is clipped on the device, comes
    back flagged, is rendered again eagerly and then carries the eager figure."""
    (_, g), (_, e), _ = _sweeps()
    order = np.argsort(g["instances"])
    top, second = int(g["instances"][order[-1]]), int(g["instances"][order[-2]])
    assert top > second + 1, (top, second)
    ev, r = _pass(True, capacity=(top + second) // 2)
    print(f"instances {list(map(int, g['instances']))}, capacity {(top + second) // 2}, rendered again {r['rerendered']}")
    assert r["rerendered"] == [int(order[-1])] and ev.host_reads == 2
    assert np.array_equal(r["sse"], e["sse"]) and np.abs(r["ssim"] - e["ssim"]).max() <= EA.SSIM_BAR
    assert torch.equal(r["images"], e["images"])


def test_mean_psnr_within_the_projects_bar_of_the_oracle_chain():
    """The HIP chain (captured sweep) against the oracle chain: oracle/ renders the posed model in float64, losses.eval_metrics measures it in
    float64.  0.05 dB is the project's bar; no pixel is excused."""
    from oracle.oracle import Oracle
    from egogaussian_amd import covariance, motion
    from egogaussian_amd.losses import eval_metrics
    (_, g), _, _ = _sweeps()
    s = _scene()
    pc = _model()
    o = Oracle(np.float64)
    psnr, ssim = [], []
    with torch.no_grad():
        xyz, io = pc.get_xyz.detach().cpu().double(), s["is_obj"].cpu()
        scaling, rot, opac, feats = (t.detach().cpu().double() for t in (pc.get_scaling, pc._rotation, pc.get_opacity, pc.get_features))
        for k in range(F):
            T, cam = s["Ts"][k].cpu().double(), s["cams"][k]
            placed = motion.move_points(xyz, T[:3], io == 1)
            cov = covariance.rotated_covariance_from_scaling_rotation(scaling, 1.0, rot, T[:3, :3], io, 1)
            st = o.forward(means3D=placed, opacities=opac, shs=feats, cov3D_precomp=cov, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                           campos=cam.camera_center, bg=s["bg"], image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2))
            m = eval_metrics(torch.from_numpy(np.asarray(st["color"], np.float64)), s["gts"][k].cpu().double(), s["keeps"][k].cpu())
            psnr.append(float(m["psnr"])); ssim.append(float(m["ssim"]))
    d = abs(g["mean_psnr"] - float(np.mean(psnr)))
    print(f"mean PSNR: HIP chain {g['mean_psnr']:.5f} dB, oracle chain {float(np.mean(psnr)):.5f} dB, |difference| {d:.2e} dB (bar 0.05); "
          f"per frame {np.abs(g['psnr'] - np.asarray(psnr)).max():.2e}; mean SSIM {g['mean_ssim']:.7f} vs {float(np.mean(ssim)):.7f}")
    assert np.isfinite(d) and d <= 0.05


def test_reallocated_model_is_refused_until_recapture():
    from egogaussian_amd.evaluate import EvalPass
    s = _scene()
    pc = _model()
    ev = EvalPass(pc, s["bg"], dynamic=True, motion=True, which_object=1)
    ev.run(s["frames"][:2], s["cams"][0])
    pc.model_version = getattr(pc, "model_version", 0) + 1                  # what CapacityGaussians.grow does after replacing the arrays
    with pytest.raises(RuntimeError, match="reallocated its arrays"):
        ev.run(s["frames"][:2], s["cams"][0])
    ev.recapture()
    assert ev.run(s["frames"][:2], s["cams"][0])["rerendered"] == []
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.run([f.cpu() for f in s["frames"][:2]], s["cams"][0])
