#!/usr/bin/env python
"""A miniature of /root/reference/trainers/train_static.py:67-138 on the synthetic scene, wired entirely to this package:
render -> 0.8 L1 + 0.2 (1 - SSIM) -> backward -> densification statistics -> [densify / prune, opacity reset] -> Adam,
with the steady-state iterations replayed from a hipGraph and the point cloud written as a PLY at the end.

    python examples/train_synth.py --gaussians 20000 --height 270 --width 480 --iters 600 --out /tmp/synth.ply

The model is capacity-sized (egogaussian_amd/capacity.py): densification and pruning rewrite the same arrays in place and the
number of live Gaussians is a device word, so the captured step is NOT re-captured when the model grows (`--plain` keeps the
reference's behaviour -- new tensors per densification, one re-capture each).  The step voids frames that outgrow its instance
capacity on the device and re-captures itself with more room (GraphedTrainStep(check_every=...)).

`--device-densify` densifies through densify.DeviceDensify: plan and in-place apply replayed from a hipGraph of their own, no count read
back.  Its status words are read where the loop calls step.check() anyway; a densification the capacity refused wrote nothing, and the
loop grows the model, re-captures and densifies again.

`--entropy-iters K` appends the reference's entropy phase (trainers/train_static.py:97-102,139-141): K more iterations of the SAME
captured step with the weight of the opacity-entropy term switched on (`step.entropy_weight = --entropy-weight`: a device scalar, no
re-capture), then `prune_points(get_opacity < 0.5)` on the capacity model (in place: no re-capture either).

`--mask-handoff` appends the hand-off between the reference's static stage and its background stage (trainers/train_static.py:104-109,
167-197, train.py:80-90, trainers/train_static_bg.py:81-99): a short label phase (GraphedTrainStep(label_phase=True)) against object masks
rendered from the teacher, the predicted masks of every frame by one captured sweep (masks.MaskPass), is_object from the labels, the split
into an object and a background model, and a few background-stage steps on the background model, their image gradient gated by
fused.interaction_gate(hand mask, predicted mask, 5) written straight into the packed frame.

It shows the order of calls a trainer needs; it is not part of the measured path.  `--log` appends a line per report interval
(iteration, live Gaussians, it/s so far, held-out PSNR), which is how profiles/r2_train_synth_*.log were produced.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egogaussian_amd import densify, fused, masks, ply                            # noqa: E402
from egogaussian_amd.capacity import CapacityGaussians                            # noqa: E402
from egogaussian_amd.evaluate import EvalPass                                     # noqa: E402
from egogaussian_amd.graph import GraphedTrainStep, frame_layout, pack_frame, pack_label_frame      # noqa: E402
from egogaussian_amd.losses import psnr                                           # noqa: E402
from egogaussian_amd.renderer import get_render_label, render                     # noqa: E402
from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe, N_FRAMES   # noqa: E402


def mask_handoff(pc, teacher, cams, gts, bg, a, report):
    """The hand-off between the static stage and the background stage on the trained model `pc` -> dict of what happened."""
    import numpy as np
    dev, (H, W), F = bg.device, gts[0].shape[-2:], len(cams)
    # the dataset's side: the object is the 30 % of the teacher with the smallest x; its masks are the teacher's label renders, thresholded;
    # the hand is a rectangle of its own per frame
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=dev, sh_degree=a.sh_degree, requires_grad=False)
        x = tpc._xyz[:, :1]
        tpc._label = torch.where(x < torch.quantile(x, 0.3), 4.0, -4.0)
        obj_masks = [(get_render_label(c, tpc, bg, scalar=True).mean(0) > 0.5).float() for c in cams]
        del tpc
    hands = []
    for k in range(F):
        h = torch.zeros(H, W, device=dev)
        y0, x0 = (H // 8) + (k * 7) % (H // 2), (W // 8) + (k * 13) % (W // 2)
        h[y0:y0 + H // 5, x0:x0 + W // 6] = 1.0
        hands.append(h)
    # 1. the label phase: only the labels move, the hand is gated out of the loss (train_static.py:104-109)
    for g in pc.optimizer.param_groups:
        if g["name"] == "label":
            g["lr"] = a.label_lr
    lstep = GraphedTrainStep(pc, pc.optimizer, bg, label_phase=True, gated=True)
    lstep.capture(cams[0], obj_mask=obj_masks[0], gate=1.0 - hands[0], warmup=1, capacity_margin=1.5)
    lframes = [pack_label_frame(cams[k], obj_masks[k], gate=1.0 - hands[k]) for k in range(F)]
    for j in range(a.label_iters):
        lstep(lframes[j % F])
    torch.cuda.synchronize()
    lstep.check()
    # 2. the predicted masks of every frame: one captured sweep, one host read (train_static.py:183-196)
    mp = masks.MaskPass(pc, bg)
    res = mp.run(lframes, cams[0], capacity_margin=1.5)
    report(f"mask hand-off: {a.label_iters} label iterations (loss {float(lstep.loss):.4f}); predicted masks of {F} frames, mean IoU against the "
           f"object masks {res['mean_iou']:.4f} over the pixels outside the hand, {len(res['rerendered'])} frame(s) rendered again, {mp.host_reads} host read(s)")
    # 3. is_object from the labels, the two models (train_static.py:167-178)
    masks.infer_is_object_from_label(pc)
    obj, bgm = masks.split_object_background(pc)
    report(f"mask hand-off: {obj._xyz.shape[0]} object + {bgm._xyz.shape[0]} background Gaussians")
    # 4. a few background-stage steps (train_static_bg.py:81-110): the image gradient gated by 1 - dilate_5(hand | predicted mask), the gate
    #    written by the kernel into the packed frame's own segment
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_label"):
        setattr(bgm, name, getattr(bgm, name).detach().clone().requires_grad_(True))
    bgm.training_setup(capturable=True)
    off, _ = frame_layout(gts[0].numel(), H * W, gated=True)
    bframes = []
    for k in range(F):
        fr = pack_frame(cams[k], gts[k], gate=hands[k])
        fused.interaction_gate(hands[k], res["masks"][k], a.dilate_size, out=fr[off["gate"][0]:off["gate"][1]])
        bframes.append(fr)
    gated = float(np.mean([float((fr[off["gate"][0]:off["gate"][1]] == 0).float().mean()) for fr in bframes]))
    bstep = GraphedTrainStep(bgm, bgm.optimizer, bg, lambda_dssim=0.2, gated=True, densify_stats=True, entropy_reg=True)
    bstep.capture(cams[0], gts[0], warmup=1, capacity_margin=1.5, gate=bframes[0][off["gate"][0]:off["gate"][1]].view(H, W))
    for j in range(a.bg_iters):
        bstep(bframes[j % F])
    torch.cuda.synchronize()
    bstep.check()
    report(f"mask hand-off: {a.bg_iters} background-stage steps, {100 * gated:.1f} % of the pixels gated (dilate {a.dilate_size}), loss {float(bstep.loss):.4f}")
    return dict(mean_iou=res["mean_iou"], rerendered=len(res["rerendered"]), host_reads=mp.host_reads, n_object=int(obj._xyz.shape[0]),
                n_background=int(bgm._xyz.shape[0]), gated_fraction=gated, object=obj, background=bgm, masks=res["masks"])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--densify-from", type=int, default=100)
    ap.add_argument("--densify-until", type=int, default=400)
    ap.add_argument("--densify-interval", type=int, default=100)
    ap.add_argument("--opacity-reset-interval", type=int, default=300)
    ap.add_argument("--grad-threshold", type=float, default=2e-4)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--sh-degree", type=int, default=0, help="spherical-harmonics degree of the colour model (0..3)")
    ap.add_argument("--sh-up-interval", type=int, default=0,
                    help="start at active degree 0 and raise it every this many iterations (the reference: 1000, scene/gaussian_model.py:176-178)")
    ap.add_argument("--out", default="")
    ap.add_argument("--plain", action="store_true", help="plain model: densification replaces the tensors, the step is re-captured each time")
    ap.add_argument("--capacity-factor", type=float, default=3.0, help="rows allocated = this x the initial number of Gaussians")
    ap.add_argument("--device-densify", action="store_true",
                    help="densify through densify.DeviceDensify: plan and in-place apply replayed from a hipGraph, no count read back; the status "
                         "words are read at the step.check() points, and a densification the capacity refused is made up for after grow()")
    ap.add_argument("--report-every", type=int, default=0, help="print (and --log) progress every this many iterations")
    ap.add_argument("--log", default="")
    ap.add_argument("--min-opacity", type=float, default=0.005)
    ap.add_argument("--knn-init", action="store_true",
                    help="initialise the student as GaussianModel.create_from_pcd does (/root/reference/scene/gaussian_model.py:301-318): isotropic scales "
                         "from simple_knn.distCUDA2 of the (perturbed) teacher positions, identity rotations, opacity 0.1")
    ap.add_argument("--entropy-iters", type=int, default=0,
                    help="after --iters, this many iterations with the opacity-entropy term on, then prune opacity < 0.5 (train_static.py:97-102,139-141)")
    ap.add_argument("--entropy-weight", type=float, default=0.1, help="weight of the entropy term during that phase (the reference: 0.1)")
    ap.add_argument("--mask-handoff", action="store_true",
                    help="after training: a label phase, the predicted object masks of every frame (masks.MaskPass), the object / background split "
                         "and a few background-stage steps gated by fused.interaction_gate(hand, predicted mask, --dilate-size)")
    ap.add_argument("--label-iters", type=int, default=200, help="iterations of the label phase of --mask-handoff")
    ap.add_argument("--label-lr", type=float, default=0.1, help="learning rate of the labels during that phase")
    ap.add_argument("--bg-iters", type=int, default=50, help="background-stage steps of --mask-handoff")
    ap.add_argument("--dilate-size", type=int, default=5, help="dilation of the background stage's gate (the reference's train.py: 5)")
    a = ap.parse_args(argv)
    if a.device_densify and a.plain:
        ap.error("--device-densify needs the capacity-sized model (drop --plain)")
    dev = torch.device("cuda", 0)
    H, W = a.height, a.width
    teacher = make_scene(a.gaussians, H, W, seed=0, sh_degree=a.sh_degree)
    if a.gaussians < 100_000:
        teacher["log_scale"] += math.log(2.0)                       # few splats: make them larger so the image is covered
    cams = [make_camera(k * (N_FRAMES // a.frames), H, W, device=dev) for k in range(a.frames)]
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=dev, sh_degree=a.sh_degree, requires_grad=False)
        gts = [render(c, tpc, Pipe, bg)["render"].clone() for c in cams]
    student = perturb_student(teacher)
    if a.knn_init:
        from simple_knn._C import distCUDA2                      # the drop-in module name (egs_knn3_mean_dist2, csrc/knn.hip)
        dist2 = torch.clamp_min(distCUDA2(torch.from_numpy(student["xyz"]).float().to(dev)), 0.0000001)
        student["log_scale"] = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3).cpu().numpy()
        student["quat"][:] = 0.0; student["quat"][:, 0] = 1.0
        student["opacity_logit"][:] = math.log(0.1 / 0.9)
    if a.plain:
        pc = SynthGaussians(student, device=dev, sh_degree=a.sh_degree)
    else:
        pc = CapacityGaussians(student, int(a.gaussians * a.capacity_factor), device=dev, sh_degree=a.sh_degree)
    pc.training_setup(capturable=True)
    live = lambda: getattr(pc, "n_active", pc._xyz.shape[0])
    held = [make_camera(k * (N_FRAMES // a.frames) + 0.5 * (N_FRAMES // a.frames), H, W, device=dev) for k in range(0, a.frames, max(1, a.frames // 6))]
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=dev, sh_degree=a.sh_degree, requires_grad=False)
        held_gts = [render(c, tpc, Pipe, bg)["render"].clone() for c in held]
        del tpc
    if a.sh_up_interval > 0:
        pc.active_sh_degree = 0
    extent = 10.0

    def quality():
        """mean PSNR over held-out views between the training cameras"""
        with torch.no_grad():
            return float(sum(psnr(render(c, pc, Pipe, bg)["render"][None], g[None]) for c, g in zip(held, held_gts)) / len(held))

    log = open(a.log, "a") if a.log else None

    def report(msg):
        print(msg, flush=True)
        if log:
            log.write(msg + "\n"); log.flush()

    report(f"# {' '.join(sys.argv)}")
    report(f"start: {live()} Gaussians, held-out PSNR {quality():.2f} dB, {'plain model' if a.plain else f'capacity {pc.capacity} rows'}")
    step = GraphedTrainStep(pc, pc.optimizer, bg, lambda_dssim=0.2, densify_stats=True, check_every=50, entropy_reg=a.entropy_iters > 0)
    step.capture(cams[0], gts[0], warmup=2, capacity_margin=1.5, capacity_cams=cams[::max(1, a.frames // 6)])
    manual_recaptures, t_eval, next_report = 0, 0.0, a.report_every
    dd, last_rules, refusals = None, None, 0

    def regrow_if_refused(dd):
        """--device-densify: the one read of the densifier's status words.  A densification that needed more rows than the capacity wrote
        nothing; the model grows to hold it (new arrays) and a new DeviceDensify is captured on them -> the object to go on with."""
        nonlocal refusals
        st = dd.check()
        if not st["refused_since_last_check"]:
            return dd
        refusals += 1
        pc.grow(max(int(st["rows_needed"] * 1.5), st["rows_needed"] + 1024))
        report(f"densify refused on the device: {st['rows_needed']} rows needed; capacity grown to {pc.capacity}")
        return densify.DeviceDensify(pc).capture()

    t0, it = time.perf_counter(), 2
    while it < a.iters:
        k = it % a.frames
        step(cams[k], gts[k])                                        # render, loss, backward, statistics, Adam: one graph launch
        it += 1
        if a.sh_up_interval > 0 and it % a.sh_up_interval == 0 and pc.active_sh_degree < pc.max_sh_degree:
            pc.active_sh_degree += 1                                 # oneupSHdegree: a launch argument of the captured kernels -> re-capture
            step.recapture(warmup=1); manual_recaptures += 1
            it += 1
            report(f"iter {it}: active SH degree {pc.active_sh_degree}")
        if it <= a.densify_until and it > a.densify_from and it % a.densify_interval == 0:
            step.check()                                             # a frame that outgrew the capacity was voided on the device; make room now
            size_threshold = 20 if it > a.opacity_reset_interval else None
            ptr = pc._xyz.data_ptr()
            if a.device_densify:
                # plan and apply stay on the device: one graph launch, nothing read back.  What the previous densification did is read
                # here, where step.check() has synchronised anyway; one that did not fit wrote nothing and is made up for first.
                if dd is None:
                    dd = densify.DeviceDensify(pc).capture()
                dd = regrow_if_refused(dd)                           # (new arrays: the address test below re-captures the step)
                last_rules = (a.grad_threshold, a.min_opacity, extent, size_threshold)
                dd.replay(*last_rules)
                n0 = n1 = None                                       # known at the next check()
            else:
                n0, n1 = densify.densify_and_prune(pc, a.grad_threshold, a.min_opacity, extent, size_threshold)
            if it % a.opacity_reset_interval == 0:
                densify.reset_opacity(pc)
            if a.plain or pc._xyz.data_ptr() != ptr:                 # new parameter tensors (plain model, or the capacity had to grow) -> new graph
                step.recapture(warmup=1); manual_recaptures += 1
                it += 1
            if not a.report_every:
                report(f"iter {it}: densify {n0} -> {n1} Gaussians" if n0 is not None else f"iter {it}: densify enqueued on the device")
        if a.report_every and it >= next_report:
            next_report += a.report_every
            torch.cuda.synchronize()
            te = time.perf_counter()
            q = quality()
            t_eval += time.perf_counter() - te
            report(f"iter {it:6d}  live {live():8d}  {it / (time.perf_counter() - t0 - t_eval):8.1f} it/s so far  held-out PSNR {q:.3f} dB  "
                   f"re-captures {manual_recaptures + step.recaptures} (overflow {step.recaptures})  instance capacity {step.capacity}")
    entropy_report = None
    if a.entropy_iters > 0:
        # the entropy phase: the same captured step, the term's weight switched on in its device scalar
        graph0, recaptures0 = step.graph, manual_recaptures + step.recaptures
        step.entropy_weight = a.entropy_weight
        for j in range(a.entropy_iters):
            step(cams[(it + j) % a.frames], gts[(it + j) % a.frames])
        step.entropy_weight = 0.0
        torch.cuda.synchronize()
        h_end, n_before = float(step.entropy.item()), live()
        with torch.no_grad():
            mask = (pc.get_opacity < 0.5).squeeze(-1)                # (a capacity model: prune_points reads its live rows only)
        ptr = pc._xyz.data_ptr()
        densify.prune_points(pc, mask)
        if a.plain or pc._xyz.data_ptr() != ptr:
            step.recapture(warmup=1); manual_recaptures += 1
        entropy_report = dict(iterations=a.entropy_iters, mean_entropy_end=h_end, pruned=n_before - live(),
                              recaptures=manual_recaptures + step.recaptures - recaptures0, same_graph=step.graph is graph0)
        report(f"entropy phase: {a.entropy_iters} iterations at weight {a.entropy_weight}, mean entropy of the visible opacities {h_end:.4f}; "
               f"pruned opacity < 0.5: {n_before} -> {live()} Gaussians, {entropy_report['recaptures']} re-capture(s)")
    torch.cuda.synchronize()
    if dd is not None:                                               # the last densification's status; one that was refused is done again
        dd2 = regrow_if_refused(dd)
        if dd2 is not dd:
            step.recapture(warmup=1); manual_recaptures += 1
            dd2.replay(*last_rules)
            torch.cuda.synchronize()
    dt = time.perf_counter() - t0 - t_eval
    step.check()
    # (what the run was, for callers that assert on it: tests/test_gpu_densify.py runs the reference's full schedule through this function)
    pc.train_report = dict(gaussians_start=a.gaussians, gaussians_end=live(), psnr_end=quality(), its_per_s=a.iters / dt, recaptures=manual_recaptures + step.recaptures,
                           recaptures_after_overflow=step.recaptures, overflow_events=step.skipped_frames_seen, iterations=it, instance_capacity=step.capacity,
                           entropy_phase=entropy_report, densify_refusals=refusals)
    report(f"end: {live()} Gaussians, held-out PSNR {quality():.2f} dB, {a.iters / dt:.0f} it/s including densification, opacity resets and "
           f"{manual_recaptures + step.recaptures} re-capture(s) ({step.recaptures} after an instance-capacity overflow, {step.skipped_frames_seen} overflow events)")
    # the evaluation pass over the training cameras: 8-bit PSNR / SSIM as the reference's eval_and_metric reports them (no hand here: every
    # pixel kept), one captured graph replayed per frame, one host read at the end
    ev = EvalPass(pc, bg).run([pack_frame(c, g) for c, g in zip(cams, gts)], cams[0])
    pc.train_report["eval"] = dict(mean_psnr=ev["mean_psnr"], mean_ssim=ev["mean_ssim"], rerendered=len(ev["rerendered"]))
    report(f"evaluation pass over {len(cams)} cameras: PSNR {ev['mean_psnr']:.3f} dB, SSIM {ev['mean_ssim']:.5f} (8-bit images; "
           f"{len(ev['rerendered'])} frame(s) rendered again)")
    if a.mask_handoff:
        pc.train_report["mask_handoff"] = mask_handoff(pc, teacher, cams, gts, bg, a, report)
    if a.out:
        ply.save_ply(pc, a.out)
        back = ply.load_ply(SynthGaussians(teacher, device=dev, sh_degree=a.sh_degree), a.out, device=dev)
        assert torch.equal(back._xyz.detach(), pc._xyz.detach()[:live()])
        print(f"wrote {a.out} ({os.path.getsize(a.out) / 1e6:.1f} MB) and read it back")
    return pc


if __name__ == "__main__":
    main()
