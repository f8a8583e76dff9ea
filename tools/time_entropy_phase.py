#!/usr/bin/env python
"""Rate of the static stages' training step during the entropy-regularisation phase (/root/reference/trainers/train_static.py:97-102,
trainers/train_static_bg.py:105-110), four routes in ONE process, alternating:

  (a)   the plain captured step: GraphedTrainStep() -- what runs outside the phase, and the yardstick for "the other instantiations did not move"
  (b)   the captured step with the term: GraphedTrainStep(entropy_reg=True), weight 0.1 -- the reduction (two launches) in front of the
        entropy instantiation of the preprocess backward, the opacity still a fused leaf
  (c)   what a trainer had for this phase before: eager, render() WITHOUT optimizer= (the term is a second path into the opacities), the fused
        image loss, the torch expression of the term, backward, FusedAdam(capturable=True).step()
  (c')  the same with fused.opacity_entropy (the stand-alone kernels) in place of the torch expression

Workload: N Gaussians (default 500 000: config C) at 960 x 540, 32 cameras and ground-truth frames of a teacher scene.  Every learning rate is 0:
each side takes its full step -- moments, step counts, every launch -- on a model that stays where it is, so the rates compare the STEP and not
where a side's training went (at weight 0.1 the opacities saturate within a few thousand iterations, and a model with fewer translucent splats
renders faster: the first record of this tool had (b) 11 % AHEAD of (a) for that reason).  Every route is warmed
up; a repetition is at least --seconds of timed steps per side, ended by a device synchronise; --reps repetitions, whose spread is reported.
(b) - (a) per step is what the term costs inside the captured step.  Writes a markdown record (--out).

    python tools/time_entropy_phase.py --out profiles/entropy_phase_step.md
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd import lib, fused, losses
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    N, H, W = a.n, a.height, a.width
    teacher = make_scene(N, H, W, seed=0)
    student = perturb_student(teacher)
    bg = torch.zeros(3, device=DEV)
    n_fr = 32
    cams = [make_camera(k, H, W, device=DEV) for k in range(n_fr)]
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=DEV, requires_grad=False)
        gts = [render(c, tpc, Pipe, bg)["render"].clone() for c in cams]
        del tpc

    def captured_side(entropy):
        pc = SynthGaussians(student, device=DEV)
        opt = pc.training_setup(FusedAdam, capturable=True)
        for g in opt.param_groups:
            g["lr"] = 0.0
        gs = GraphedTrainStep(pc, opt, bg, 0.2, entropy_reg=entropy)
        if entropy:
            gs.entropy_weight = a.weight
        gs.capture(cams[0], gts[0], warmup=2, capacity_margin=1.5, capacity_cams=cams[::8])
        frames = [pack_frame(cams[k], gts[k]) for k in range(n_fr)]
        return (lambda i: gs(frames[i % n_fr])), gs

    def eager_side(standalone):
        pc = SynthGaussians(student, device=DEV)
        opt = pc.training_setup(FusedAdam, capturable=True)
        for g in opt.param_groups:
            g["lr"] = 0.0

        def step(i):
            k = i % n_fr
            out = render(cams[k], pc, Pipe, bg)                        # no optimizer=: the term below is a second path into the opacities
            loss = fused.l1_ssim_loss(out["render"], gts[k], 0.2, raster_prologue=True)
            if standalone:
                loss = loss + fused.opacity_entropy(pc._opacity, out["radii"], weight=a.weight, logit=True)
            else:
                loss = loss + a.weight * losses.opacity_entropy(pc.get_opacity, out["visibility_filter"])
            loss.backward()
            opt.step(); opt.zero_grad(set_to_none=True)
        return step, pc

    sides, steps = {}, {}
    sides["(a) captured step, plain"], steps["a"] = captured_side(False)
    sides["(b) captured step, entropy_reg, weight %g" % a.weight], steps["b"] = captured_side(True)
    sides["(c) eager: render without optimizer=, torch expression, FusedAdam.step()"], _ = eager_side(False)
    sides["(c') eager: the same with fused.opacity_entropy"], _ = eager_side(True)
    for fn in sides.values():
        for i in range(30):
            fn(i)
    torch.cuda.synchronize()
    rates = {k: [] for k in sides}
    for _ in range(a.reps):
        for name, fn in sides.items():
            n, t0 = 0, time.perf_counter()
            while True:
                for i in range(50):
                    fn(n + i)
                n += 50
                if time.perf_counter() - t0 >= a.seconds:
                    break
            torch.cuda.synchronize()
            rates[name].append(n / (time.perf_counter() - t0))
    ok = steps["a"].ok() and steps["b"].ok()
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    names = list(sides)
    us = lambda k: 1e6 / med[k]
    lines = ["# Entropy phase: the captured step with the term against the plain step and the eager routes", "",
             f"`python tools/time_entropy_phase.py` -- {N} Gaussians at {W} x {H}, one process, the sides alternating; {a.reps} repetitions of >= {a.seconds:.0f} s "
             f"per side; every learning rate 0 (the sides render the same model throughout).  Library source hash {lib.built_source_hash()}.", "",
             "| side | it/s (median) | min | max | spread | us per step |", "|---|---|---|---|---|---|"]
    for k, v in rates.items():
        s = sorted(v)
        lines.append(f"| {k} | {s[len(s) // 2]:.0f} | {s[0]:.0f} | {s[-1]:.0f} | {100 * (s[-1] - s[0]) / s[len(s) // 2]:.1f} % | {us(k):.1f} |")
    lines += ["", f"Every replayed frame of (a) and (b) fit the captured capacity: {ok}.  Mean entropy of the visible opacities at the end of (b): "
              f"{float(steps['b'].entropy):.4f}.", "",
              f"(b) - (a): {us(names[1]) - us(names[0]):+.1f} us per step -- the reduction's two launches and the entropy instantiation of k_preprocess_backward.",
              f"(b) against (c): {med[names[1]] / med[names[2]]:.2f} x the rate; against (c'): {med[names[1]] / med[names[3]]:.2f} x.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
