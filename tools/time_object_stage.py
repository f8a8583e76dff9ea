#!/usr/bin/env python
"""Rate of the object stages' training step (coarse_obj_pose / fine_obj: image + alpha loss against the object mask, hand-mask gate,
trainable pose on top of the frame's accumulated one), two routes in ONE process, alternating:

  captured   GraphedTrainStep(dynamic=True, motion=True, gated=True, object_loss=..., pose=...): fused object loss, both loss gradients
             formed in the backward blend, Adam inside the backward, graph replay
  eager      the best route without them: render(color_only=False, object_motion=...), l1_ssim_loss(grad_gate=..., raster_prologue=True),
             the alpha terms and the alpha hook in torch, backward(), optimizer.step()

Workload: an object-sized model of N Gaussians (default 100 000) at 960 x 540, a binary object mask over a quarter of the frame, four
frames with their own camera and accumulated pose.  Every shape is warmed up; a repetition is at least --seconds of timed steps per side,
ended by a device synchronise; --reps repetitions, whose spread is reported.  Writes a markdown record (--out) and prints it.

    python tools/time_object_stage.py --out profiles/object_stage_step.md
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
LAM = 0.2
WEIGHTS = dict(lambda_image=1.0, lambda_l1_alpha=0.0, lambda_l2_alpha=0.5)       # the coarse stage's defaults


class Pose(torch.nn.Module):
    """ObjectMove-shaped: obj_translation [3], obj_rotation_6d [3,2] (columns orthonormalised in order), rot_L(L) = R @ L."""

    def __init__(self):
        super().__init__()
        self.obj_translation = torch.nn.Parameter(torch.tensor([0.02, -0.01, 0.03], device=DEV))
        self.obj_rotation_6d = torch.nn.Parameter(torch.tensor([[1.0, 0.02], [-0.01, 1.0], [0.03, 0.01]], device=DEV))

    def rot_L(self, L):
        a1, a2 = self.obj_rotation_6d[:, 0], self.obj_rotation_6d[:, 1]
        b1 = a1 / a1.norm()
        b2 = a2 - (b1 * a2).sum() * b1
        b2 = b2 / b2.norm()
        return torch.stack((b1, b2, torch.linalg.cross(b1, b2)), dim=-1) @ L


def rigid(angle, t):
    c, s = math.cos(angle), math.sin(angle)
    T = torch.eye(4)
    T[:3, :3] = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    T[:3, 3] = torch.tensor([0.0, 0.0, 6.0]) - T[:3, :3] @ torch.tensor([0.0, 0.0, 6.0]) + torch.tensor(t)
    return T.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.losses import l1_loss, l2_loss
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    from egogaussian_amd.motion import ObjectMotion
    from egogaussian_amd import lib
    N, H, W = a.n, a.height, a.width
    teacher = make_scene(N, H, W, 0)
    teacher["log_scale"] += math.log(2.0)
    student = perturb_student(teacher)
    is_obj = (torch.rand(N, 1, generator=torch.Generator().manual_seed(4)) < 0.3).float().to(DEV)
    is_obj[0, 0] = 0.0
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in (30, 60, 90, 120)]
    Ts = [rigid(0.05 + 0.01 * k, (0.1 - 0.01 * k, -0.05, 0.02 * k)) for k in range(4)]
    with torch.no_grad():
        gts = [render(c, SynthGaussians(teacher, device=DEV, requires_grad=False), Pipe, bg)["render"].clone() for c in cams]
    mask = torch.zeros(H, W, device=DEV)
    mask[H // 4:3 * H // 4, W // 4:3 * W // 4] = 1.0                      # a quarter of the frame
    gate = (torch.rand((H, W), generator=torch.Generator().manual_seed(5)) < 0.9).float().to(DEV)

    def model():
        pc = SynthGaussians(student, device=DEV)
        pc._is_object = is_obj
        pose = Pose()
        groups = [{"params": [pc._xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [pc._features_dc], "lr": 2.5e-3, "name": "f_dc"},
                  {"params": [pc._opacity], "lr": 0.05, "name": "opacity"}, {"params": [pc._scaling], "lr": 5e-3, "name": "scaling"},
                  {"params": [pc._rotation], "lr": 1e-3, "name": "rotation"},
                  {"params": [pose.obj_translation], "lr": 1e-4, "name": "obj_translation"},
                  {"params": [pose.obj_rotation_6d], "lr": 1e-4, "name": "obj_rotation_6d"}]
        return pc, pose, FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True)

    # captured
    pc_a, pose_a, opt_a = model()
    step = GraphedTrainStep(pc_a, opt_a, bg, LAM, dynamic=True, motion=True, gated=True, object_loss=WEIGHTS, pose=pose_a).capture(
        cams[0], gts[0], warmup=3, accum_R=Ts[0][:3, :3], accum_T=Ts[0], gate=gate, obj_mask=mask, capacity_cams=cams, capacity_margin=1.5)
    frames = [pack_frame(cams[k], gts[k], Ts[k][:3, :3], gate, Ts[k], obj_mask=mask) for k in range(4)]

    def captured(k):
        step(frames[k % 4])

    # eager: the route that needs none of this
    pc_b, pose_b, opt_b = model()
    gtm = [g * mask for g in gts]
    m1 = mask[None]

    def eager(k):
        k = k % 4
        out = render(cams[k], pc_b, Pipe, bg, rot_cov=True, which_object=1, optimizer=opt_b, object_motion=ObjectMotion(Ts[k], pose_b, Ts[k][:3, :3]))
        alpha = out["alpha"]
        alpha.register_hook(lambda g: g * gate)
        loss = WEIGHTS["lambda_image"] * l1_ssim_loss(out["render"], gtm[k], LAM, grad_gate=gate, raster_prologue=True) \
            + WEIGHTS["lambda_l1_alpha"] * l1_loss(m1, alpha) + WEIGHTS["lambda_l2_alpha"] * l2_loss(m1, alpha)
        loss.backward()
        opt_b.step(); opt_b.zero_grad(set_to_none=True)

    def timed(fn, seconds):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while True:
            for _ in range(20):
                fn(n); n += 1
            if time.perf_counter() - t0 >= seconds:
                break
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for k in range(8):                                                    # every frame, both routes
        captured(k); eager(k)
    torch.cuda.synchronize()
    assert step.ok()
    rates = {"captured": [], "eager": []}
    for _ in range(a.reps):
        rates["captured"].append(timed(captured, a.seconds))
        rates["eager"].append(timed(eager, a.seconds))
    assert step.ok()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    mc, me = med(rates["captured"]), med(rates["eager"])
    sp = max(spread(rates["captured"]), spread(rates["eager"]))
    ratio = mc / me
    verdict = (f"The captured step is faster by {100 * (ratio - 1):.1f} %, more than the spread of the repetitions ({100 * sp:.1f} %)." if ratio - 1 > sp else
               f"The captured step is NOT faster by more than the spread of the repetitions: ratio {ratio:.3f}, spread {100 * sp:.1f} %.")
    name = torch.cuda.get_device_name(0)
    lines = ["# Object-stage training step: captured step against the eager route", "",
             f"`python tools/time_object_stage.py --n {N} --height {H} --width {W} --seconds {a.seconds} --reps {a.reps}` on {name}, library "
             f"source hash {lib.built_source_hash()}.", "",
             f"Workload: {N} Gaussians (30 % the object) at {W} x {H}, a binary object mask over a quarter of the frame, hand-mask gate, four frames "
             f"with their own camera and accumulated pose, a trainable pose on top; loss weights {WEIGHTS}, lambda_dssim {LAM}.  Both routes run in one "
             f"process and alternate; each repetition is at least {a.seconds} s of steps per side, ended by a device synchronise.", "",
             "| route | steps / s, each repetition | median | spread (max - min) / median |", "|---|---|---|---|"]
    for r in ("captured", "eager"):
        lines.append(f"| {r} | {', '.join(f'{v:.0f}' for v in rates[r])} | {med(rates[r]):.0f} | {100 * spread(rates[r]):.1f} % |")
    lines += ["", verdict, "",
              "captured: `GraphedTrainStep(dynamic=True, motion=True, gated=True, object_loss=..., pose=...)`.  eager: `render(color_only=False, "
              "object_motion=..., optimizer=...)`, `l1_ssim_loss(grad_gate=..., raster_prologue=True)`, the alpha terms and the alpha hook in torch, "
              "`backward()`, `optimizer.step()`.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
