"""CPU: the label phase's host side -- the torch mirror of the loss, the packed frame of a label step, the argument combinations
GraphedTrainStep(label_phase=True) refuses, and the additions to the C ABI (declared, exported, argument errors before any device work)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirror_is_bce_with_logits_of_the_channel_mean_with_the_hook():
    from egogaussian_amd.losses import label_bce_loss
    g = torch.Generator().manual_seed(0)
    H, W = 9, 11
    x = torch.randn(3, H, W, generator=g, dtype=torch.float64) * 3
    x[:, 0, :4] = 40.0; x[:, 1, :4] = -40.0                             # saturated logits, both signs ...
    mask = (torch.rand(1, H, W, generator=g) > 0.5).double()
    mask[0, 0, :2] = 0.0; mask[0, 0, 2:4] = 1.0; mask[0, 1, :2] = 0.0; mask[0, 1, 2:4] = 1.0      # ... against both mask values
    hand = (torch.rand(H, W, generator=g) > 0.7).double()
    up = 3.0

    def run(fn):
        xx = x.clone().requires_grad_(True)
        mean_holder = {}
        loss = fn(xx, mean_holder)
        (loss * up).backward()
        return loss.detach(), xx.grad

    def reference(xx, _):
        render_label = xx.mean(0, keepdim=True)
        render_label.register_hook(lambda gr: gr * (1 - hand))
        return torch.nn.BCEWithLogitsLoss()(render_label, mask)

    def mirror(xx, _):
        # the mirror takes the image; the hook of the reference sits on the mean -- expressed on the image it is the same factor per pixel
        xx.register_hook(lambda gr: gr * (1 - hand))
        return label_bce_loss(xx, mask[0])

    l_ref, g_ref = run(reference)
    l_mir, g_mir = run(mirror)
    assert float(l_ref) == float(l_mir) and torch.isfinite(l_ref)
    assert torch.allclose(g_ref, g_mir, rtol=1e-14, atol=0)
    # ... and the closed form the kernels implement (csrc/label_bce.h): dL/dx = up * gate * (sigmoid(x) - m) / (H W), a third of it per plane
    xm = x.mean(0)
    closed = up * (1 - hand) * (torch.sigmoid(xm) - mask[0]) / (H * W) / 3
    assert torch.allclose(g_ref, closed.expand(3, H, W), rtol=1e-12, atol=1e-18)
    l_closed = (xm.clamp_min(0) - xm * mask[0] + torch.log1p(torch.exp(-xm.abs()))).mean()
    assert abs(float(l_closed) - float(l_ref)) < 1e-14


def test_label_frame_layout_round_trip_and_old_offsets():
    from egogaussian_amd.graph import frame_layout, pack_frame, pack_label_frame
    from egogaussian_amd.scene_synth import make_camera
    # the layouts that existed before keep their offsets (the numbers below are the parent's)
    assert frame_layout(60, 20) == ({"gt": (0, 60), "cam": (60, 95)}, 96)
    assert frame_layout(60, 20, dynamic=True, gated=True, motion=True, object_loss=True) == (
        {"gt": (0, 60), "cam": (60, 95), "accum_R": (96, 105), "accum_T": (108, 120), "gate": (120, 140), "obj_mask": (140, 160)}, 160)
    assert frame_layout(61, 21, gated=True) == ({"gt": (0, 61), "cam": (64, 99), "gate": (100, 121)}, 124)
    # the label step's: camera[, gate], obj_mask -- no image segment
    assert frame_layout(0, 21, label_phase=True) == ({"cam": (0, 35), "obj_mask": (36, 57)}, 60)
    off, size = frame_layout(12345, 21, gated=True, label_phase=True)
    assert off == {"cam": (0, 35), "gate": (36, 57), "obj_mask": (60, 81)} and size == 84 and all(b % 4 == 0 for b, _ in off.values())
    H, W = 3, 7
    cam = make_camera(2, H, W)
    g = torch.Generator().manual_seed(1)
    mask, gate = (torch.rand(1, H, W, generator=g) > 0.5), torch.rand(H, W, generator=g)
    f = pack_label_frame(cam, mask, gate)
    assert f.shape == (size,) and f.dtype == torch.float32
    assert torch.equal(f[off["obj_mask"][0]:off["obj_mask"][1]].view(H, W), mask[0].float())
    assert torch.equal(f[off["gate"][0]:off["gate"][1]].view(H, W), gate)
    assert torch.equal(f[0:16].view(4, 4), cam.world_view_transform.float()) and torch.equal(f[32:35], cam.camera_center.float())
    f2 = pack_label_frame(cam, mask)
    assert f2.numel() == 60 and torch.equal(f2[36:57].view(H, W), mask[0].float())
    # pack_frame is what it was
    gt = torch.rand(3, H, W, generator=g)
    pf = pack_frame(cam, gt, gate=gate)
    assert pf.numel() == frame_layout(63, 21, gated=True)[1] and torch.equal(pf[:63].view(3, H, W), gt)


def _optimizer(with_label=True):
    from egogaussian_amd.optim import FusedAdam
    groups = [{"params": [torch.zeros(4, 3, requires_grad=True)], "lr": 1e-3, "name": "xyz"}]
    if with_label:
        groups.append({"params": [torch.zeros(4, 1, requires_grad=True)], "lr": 1e-2, "name": "label"})
    return FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True)


@pytest.mark.parametrize("kw,word", [(dict(dynamic=True), "dynamic"), (dict(dynamic=True, motion=True), "dynamic"), (dict(object_loss=dict(lambda_image=1.0)), "object_loss"),
                                     (dict(densify_stats=True), "densify_stats"), (dict(double_buffer=True), "double_buffer"),
                                     (dict(dynamic=True, motion=True, pose=object()), "dynamic")])
def test_label_phase_refuses_what_it_cannot_capture(kw, word):
    from egogaussian_amd.graph import GraphedTrainStep
    with pytest.raises(ValueError, match=word):
        GraphedTrainStep(None, _optimizer(), torch.zeros(3), label_phase=True, **kw)


def test_label_phase_refuses_motion_and_pose_by_name_and_needs_a_label_group():
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    # each conflicting argument is named, whichever others come with it
    for kw, word in ((dict(motion=True), "motion"), (dict(pose=object()), "pose")):
        with pytest.raises(ValueError, match=word):
            GraphedTrainStep(None, _optimizer(), torch.zeros(3), label_phase=True, **kw)
    with pytest.raises(ValueError, match='"label"'):
        GraphedTrainStep(None, _optimizer(with_label=False), torch.zeros(3), label_phase=True)
    with pytest.raises(ValueError, match="capturable"):
        GraphedTrainStep(None, FusedAdam([{"params": [torch.zeros(2, 1, requires_grad=True)], "name": "label"}]), torch.zeros(3), label_phase=True)
    step = GraphedTrainStep(None, _optimizer(), torch.zeros(3), label_phase=True, gated=True, steps_per_replay=2)
    assert step.label_phase and step.gated and step.steps_per_replay == 2 and step.label_grad is None
    with pytest.raises(ValueError, match="obj_mask"):
        step.capture(object())


def test_abi_additions_are_declared_exported_and_check_their_arguments():
    import ctypes as C
    from egogaussian_amd import lib
    text = open(os.path.join(ROOT, "include", "egs_raster.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = lib.load()
    for name in ("egs_label_bce_partial_count", "egs_label_bce_forward", "egs_label_bce_backward", "egs_backward_label"):
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/egs_raster.h"
        assert hasattr(L, name) and name in lib.SIGNATURES
    assert re.search(r"#define\s+EGS_ACT_SCALAR_COLOR\s+16\b", code) and lib.ACT_SCALAR_COLOR == 16
    assert re.search(r"typedef struct egs_label_loss \{[^}]*img;[^}]*mask;[^}]*gate;[^}]*upstream;[^}]*partial;[^}]*n_partial;[^}]*loss;[^}]*running;", code)
    assert [n for n, _ in lib.LabelLoss._fields_] == ["img", "mask", "gate", "upstream", "partial", "n_partial", "loss", "running"]
    assert L.egs_abi_version() == 6, "additions only"
    assert L.egs_label_bce_partial_count(540, 960) == 4 * 60 * 34 and L.egs_label_bce_partial_count(7, 9) == 4 and L.egs_label_bce_partial_count(0, 9) == 0
    p = C.c_void_p(4096)
    none = None
    # exactly one of the upstream planes and the loss struct
    ll = lib.LabelLoss()
    assert L.egs_backward_label(10, 5, 64, 64, p, p, p, p, none, none, p, none, 0.9, 0.999, 1e-15, none, none, none, p, none, 0) == -2
    assert L.egs_backward_label(10, 5, 64, 64, p, p, p, p, p, C.byref(ll), p, none, 0.9, 0.999, 1e-15, none, none, none, p, none, 0) == -2
    assert L.egs_backward_label(10, 5, 64, 64, p, p, p, p, none, C.byref(ll), p, none, 0.9, 0.999, 1e-15, none, none, none, p, none, 0) == -1      # an empty loss struct
    assert L.egs_backward_label(10, 5, 70000, 64, p, p, p, p, p, none, p, none, 0.9, 0.999, 1e-15, none, none, none, p, none, 0) == -3
    leaf = lib.AdamLeaf()
    assert L.egs_backward_label(10, 5, 64, 64, p, p, p, p, p, none, p, C.byref(leaf), 0.9, 0.999, 1e-15, none, none, none, p, none, 0) == -1       # an empty leaf
    assert L.egs_backward_label(10, 5, 64, 64, none, p, p, p, p, none, p, none, 0.9, 0.999, 1e-15, none, none, none, p, none, 0) == -1             # no radii
    assert L.egs_label_bce_forward(64, 64, none, p, p, p, none, none) == -1 and L.egs_label_bce_backward(64, 64, p, p, none, none, p, none, none, none, none) == -1
    # the scalar colour flag goes with colors_precomp only, and its gradient is egs_backward_label's
    R = C.c_int64(0)
    assert L.egs_forward_geometry(10, 0, 1, p, p, none, none, p, p, 1.0, p, none, 16, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R), none, none, none, 0) == -2
    assert L.egs_backward(10, 0, 0, 5, p, p, none, none, p, p, 1.0, p, none, 16, p, p, p, 64, 64, 1.0, 1.0, p, p, p, p, p, none, none, p, p, p, p, none, none,
                          none, p, p, none, none, none, none, 0, p, none, 0) == -2
