#!/usr/bin/env python
"""Rate of the object stages' step over DYNAMIC frames (fine_obj: every frame trains its own pose on top of the poses before it), two routes
in ONE process, alternating:

  (a) host table   GraphedTrainStep(pose=module) plus the bookkeeping fine_obj does on the host around every dynamic iteration: the `.data`
                   reload of the frame's stored pose, the read-back of the stepped pose into the table (get_obj_trans_rot), the
                   re-accumulation over all K keys (get_accum_T_seq / get_accum_R_seq: poses.accumulate on the CPU) and the rewrite of the
                   accum segments of the packed frames that lie after the trained key
  (b) device table GraphedTrainStep(pose_sequence=seq): the frames carry their pose_rows word, nothing else happens between replays

Workload: N Gaussians (default 100 000) at 960 x 540, K = 300 keys, four dynamic frames with their own camera spread over the keys.  A
repetition is at least --seconds of timed steps per side, ended by a device synchronise; --reps repetitions; side (b) is measured twice per
repetition (b, b'): the distance of the two medians is the A/A spread.  Also: the head's and tail's own durations by HIP events (back-to-back
launches; K = 300 with train_row in the middle and the worst case train_row = 0), and the kernels of one replay of each side.

    python tools/time_pose_sequence.py --out profiles/pose_sequence_step.md
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_object_stage import DEV, LAM, WEIGHTS, Pose, rigid      # noqa: E402

POSE_LR = 1e-4


def kernels_of(fn):
    """The device kernels one call of fn() runs, in order of their start (torch.profiler); None when the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memcpy" not in e.name and "Memset" not in e.name]
        ev.sort(key=lambda e: e.time_range.start)
        short = lambda s: s.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]      # the name alone
        return [("Cijk_* (a Tensile GEMM)" if e.name.startswith("Cijk_") else short(e.name)) for e in ev] or None
    except Exception as exc:                                            # (recorded in the profile, not hidden)
        return [f"<profiler failed: {type(exc).__name__}: {exc}>"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--keys", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, frame_layout, pack_frame
    from egogaussian_amd import lib, poses
    N, H, W, K = a.n, a.height, a.width, a.keys
    teacher = make_scene(N, H, W, 0)
    teacher["log_scale"] += math.log(2.0)
    student = perturb_student(teacher)
    is_obj = (torch.rand(N, 1, generator=torch.Generator().manual_seed(4)) < 0.3).float().to(DEV)
    is_obj[0, 0] = 0.0
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in (30, 60, 90, 120)]
    with torch.no_grad():
        gts = [render(c, SynthGaussians(teacher, device=DEV, requires_grad=False), Pipe, bg)["render"].clone() for c in cams]
    mask = torch.zeros(H, W, device=DEV)
    mask[H // 4:3 * H // 4, W // 4:3 * W // 4] = 1.0
    gate = (torch.rand((H, W), generator=torch.Generator().manual_seed(5)) < 0.9).float().to(DEV)
    train_rows = [max(1, K // 30), K // 3, 2 * K // 3, K - 1]            # the four dynamic frames' keys
    rel0 = torch.stack([rigid(2e-4 * (1 + k % 5), (1e-4 * (k % 7), -5e-5, 1e-4 * (k % 3)))[:3].reshape(12).cpu() for k in range(K)])

    def gaussians():
        pc = SynthGaussians(student, device=DEV)
        pc._is_object = is_obj
        groups = [{"params": [pc._xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [pc._features_dc], "lr": 2.5e-3, "name": "f_dc"},
                  {"params": [pc._opacity], "lr": 0.05, "name": "opacity"}, {"params": [pc._scaling], "lr": 5e-3, "name": "scaling"},
                  {"params": [pc._rotation], "lr": 1e-3, "name": "rotation"}]
        return pc, groups

    # (a) the table on the host
    pc_a, groups = gaussians()
    pose_a = Pose()
    opt_a = FusedAdam(groups + [{"params": [pose_a.obj_translation], "lr": POSE_LR, "name": "obj_translation"},
                                {"params": [pose_a.obj_rotation_6d], "lr": POSE_LR, "name": "obj_rotation_6d"}], lr=0.0, eps=1e-15, capturable=True)
    rel_a, valid_a = rel0.clone(), torch.ones(K, dtype=torch.uint8)
    accum_a = poses.accumulate(rel_a, valid_a)
    eye = torch.eye(4)
    step_a = GraphedTrainStep(pc_a, opt_a, bg, LAM, dynamic=True, motion=True, gated=True, object_loss=WEIGHTS, pose=pose_a).capture(
        cams[0], gts[0], warmup=3, accum_R=eye[:3, :3].to(DEV), accum_T=eye.to(DEV), gate=gate, obj_mask=mask, capacity_cams=cams, capacity_margin=1.5)
    off, _ = frame_layout(3 * H * W, H * W, True, True, True, True)
    fixed_of = lambda i: accum_a[train_rows[i] - 1].reshape(3, 4)
    frames_a = torch.stack([pack_frame(cams[i], gts[i], fixed_of(i)[:, :3], gate, fixed_of(i), obj_mask=mask) for i in range(4)])

    def host_table(n):
        i = n % 4
        k = train_rows[i]
        row = rel_a[k].reshape(3, 4)
        pose_a.obj_translation.data.copy_(row[:, 3], non_blocking=True)                        # fine_obj.py:118-119
        pose_a.obj_rotation_6d.data.copy_(row[:, :2], non_blocking=True)
        step_a(frames_a[i])
        t, r6 = pose_a.obj_translation.detach().cpu(), pose_a.obj_rotation_6d.detach().cpu()      # get_obj_trans_rot: waits for the step
        rel_a[k] = torch.cat([poses.rot6d_to_matrix(r6), t[:, None]], dim=1).reshape(12)
        accum_a.copy_(poses.accumulate(rel_a, valid_a))                                       # get_accum_T_seq / get_accum_R_seq over all keys
        for j in range(4):                                                                    # the packed frames after the trained key
            if train_rows[j] - 1 >= k:
                f = fixed_of(j)
                frames_a[j, off["accum_R"][0]:off["accum_R"][1]].copy_(f[:, :3].reshape(9), non_blocking=True)
                frames_a[j, off["accum_T"][0]:off["accum_T"][1]].copy_(f.reshape(12), non_blocking=True)

    # (b) the table on the device
    pc_b, groups = gaussians()
    opt_b = FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True)
    seq = poses.PoseSequence(range(K), DEV)
    seq.rel.copy_(rel0); seq.valid.fill_(1)
    seq.accumulate()
    seq.set_lr(POSE_LR, POSE_LR)
    step_b = GraphedTrainStep(pc_b, opt_b, bg, LAM, dynamic=True, motion=True, gated=True, object_loss=WEIGHTS, pose_sequence=seq).capture(
        cams[0], gts[0], warmup=3, gate=gate, obj_mask=mask, capacity_cams=cams, capacity_margin=1.5, pose_rows=(train_rows[0] - 1, train_rows[0], 1))
    frames_b = [pack_frame(cams[i], gts[i], gate=gate, obj_mask=mask, pose_rows=(train_rows[i] - 1, train_rows[i], 1)) for i in range(4)]

    def device_table(n):
        step_b(frames_b[n % 4])

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

    for n in range(8):
        host_table(n); device_table(n)
    torch.cuda.synchronize()
    assert step_a.ok() and step_b.ok()
    rates = {"a": [], "b": [], "b'": []}
    for _ in range(a.reps):
        rates["b"].append(timed(device_table, a.seconds))
        rates["a"].append(timed(host_table, a.seconds))
        rates["b'"].append(timed(device_table, a.seconds))
    assert step_a.ok() and step_b.ok()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    aa = abs(med(rates["b"]) - med(rates["b'"])) / med(rates["b"])
    noise = max(aa, spread(rates["a"]), spread(rates["b"]), spread(rates["b'"]))
    ratio = med(rates["b"] + rates["b'"]) / med(rates["a"])
    verdict = (f"(b) is ahead of (a) by {100 * (ratio - 1):.1f} %, more than the A/A spread and the spread of the repetitions ({100 * noise:.1f} %)."
               if ratio - 1 > noise else
               f"(b) is NOT ahead of (a) by more than the A/A spread and the spread of the repetitions: ratio {ratio:.3f}, {100 * noise:.1f} %.")

    # the two kernels alone, by HIP events: back-to-back launches on a copy of the table
    def event_us(fn, n=400):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    solo = poses.PoseSequence(range(K), DEV)
    solo.rel.copy_(rel0); solo.valid.fill_(1); solo.accumulate(); solo.set_lr(POSE_LR, POSE_LR)
    A12, M9, g21 = torch.zeros(12, device=DEV), torch.zeros(9, device=DEV), torch.randn(21, device=DEV) * 1e-3
    word = lambda f, t: torch.tensor([f, t, 1, 0], dtype=torch.int32, device=DEV)
    w_mid, w_first, w_last, w_fixed = word(K // 2 - 1, K // 2), word(-1, 0), word(K - 2, K - 1), word(K // 2, -1)
    kernel_rows = [("head, trainable frame", event_us(lambda: solo.head(w_mid, A12, M9))),
                   ("head, fixed-pose frame", event_us(lambda: solo.head(w_fixed, A12, M9))),
                   (f"tail, train_row = {K - 1} (last of {K})", event_us(lambda: solo.tail(w_last, g21))),
                   (f"tail, train_row = {K // 2}", event_us(lambda: solo.tail(w_mid, g21))),
                   (f"tail, train_row = 0 (worst case: all {K} rows re-accumulated)", event_us(lambda: solo.tail(w_first, g21))),
                   ("tail, fixed-pose frame", event_us(lambda: solo.tail(w_fixed, g21))),
                   (f"egs_pose_accumulate, K = {K}", event_us(solo.accumulate)),
                   ("(an empty stream: two events around nothing, per 400)", event_us(lambda: None))]
    ka, kb = kernels_of(lambda: step_a(frames_a[1])), kernels_of(lambda: step_b(frames_b[1]))

    name = torch.cuda.get_device_name(0)
    lines = ["# Object-stage step over dynamic frames: pose table on the host against the pose sequence on the device", "",
             f"`python tools/time_pose_sequence.py --n {N} --height {H} --width {W} --keys {K} --seconds {a.seconds} --reps {a.reps}` on {name}, library "
             f"source hash {lib.built_source_hash()}.", "",
             f"Workload: {N} Gaussians (30 % the object) at {W} x {H}, K = {K} keys, four dynamic frames (keys {train_rows}) with their own camera, "
             f"object mask over a quarter of the frame, hand-mask gate; loss weights {WEIGHTS}, lambda_dssim {LAM}.  Both routes run in one process "
             f"and alternate (b, a, b'); each repetition is at least {a.seconds} s of steps per side, ended by a device synchronise.", "",
             "| route | steps / s, each repetition | median | spread (max - min) / median |", "|---|---|---|---|"]
    label = {"a": "(a) `pose=module` + host bookkeeping", "b": "(b) `pose_sequence=`", "b'": "(b') the same again"}
    for r in ("a", "b", "b'"):
        lines.append(f"| {label[r]} | {', '.join(f'{v:.0f}' for v in rates[r])} | {med(rates[r]):.0f} | {100 * spread(rates[r]):.1f} % |")
    lines += ["", f"A/A spread (medians of b and b'): {100 * aa:.2f} %.  {verdict}", "",
              "## The two kernels alone", "",
              "HIP events around 400 back-to-back launches on one stream (so a figure below the launch interval of the stream shows that interval, "
              "not the kernel), microseconds per launch:", "", "| launch | us |", "|---|---|"]
    lines += [f"| {n} | {v:.2f} |" for n, v in kernel_rows]
    lines += ["", "## Kernels of one replay", ""]
    for title, ks in (("(a) `pose=module`", ka), ("(b) `pose_sequence=`", kb)):
        lines += [f"{title}: {len(ks) if ks else 0} launches, in order:", "", ", ".join(f"`{k}`" for k in (ks or [])), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
