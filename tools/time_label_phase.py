#!/usr/bin/env python
"""Rate of the label phase's training step (/root/reference/trainers/train_static.py:78,104-110), three routes in ONE process, alternating:

  (i)    eager, as bench.py's `label_phase_shape` leg runs it (that loop, copied): render() forward whose image reaches no loss,
         get_render_label() forward, channel mean, hand-mask hook, BCEWithLogits, backward (colours only), loss.item(), Adam on the label
  (ii)   the same without the unused colour render()
  (iii)  captured: GraphedTrainStep(label_phase=True, gated=True) -- scalar colour input, the loss gradient formed in the backward blend,
         Adam and the loss value in the finishing launch, graph replay (no loss.item(): the value stays on the device)

Workload: N Gaussians (default 100 000) at 960 x 540, 32 cameras, four hand masks (10 % gated) and four object masks (30 % set), as the bench
leg's.  Every route is warmed up; a repetition is at least --seconds of timed steps per side, ended by a device synchronise; --reps
repetitions, whose spread is reported.  Also: the backward's two kernels by the library's HIP events on one frame --
k_render_backward<0, false> + k_colors_from_acc against k_render_backward<3, true> + k_label_finish.  Writes a markdown record (--out).

    python tools/time_label_phase.py --out profiles/label_phase_step.md
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
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch.nn as nn
    from egogaussian_amd import lib, _C
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render, get_render_label
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_label_frame
    N, H, W = a.n, a.height, a.width
    student = perturb_student(make_scene(N, H, W, seed=0))
    bg = torch.zeros(3, device=DEV)
    n_fr = 32
    cams = [make_camera(k, H, W, device=DEV) for k in range(n_fr)]
    gen = torch.Generator().manual_seed(11)
    hand = [(torch.rand(1, H, W, generator=gen) < 0.1).float().to(DEV) for _ in range(4)]
    objm = [(torch.rand(1, H, W, generator=gen) < 0.3).float().to(DEV) for _ in range(4)]
    crit = nn.BCEWithLogitsLoss()

    def eager_side(with_render):
        pc = SynthGaussians(student, device=DEV)
        pc._label = torch.zeros(N, 1, device=DEV).requires_grad_(True)
        opt = FusedAdam([{"params": [pc._label], "lr": 0.01, "name": "label"}], lr=0.0, eps=1e-15)

        def step(i):
            k = i % n_fr
            if with_render:
                render(cams[k], pc, Pipe, bg)                           # train_static.py:78 (not part of this phase's loss)
            lab = torch.mean(get_render_label(cams[k], pc, bg), dim=0, keepdim=True)
            hm = hand[k % 4]
            lab.register_hook(lambda grad: grad * (1 - hm))
            loss = crit(input=lab, target=objm[k % 4])
            loss.backward()
            loss.item()
            opt.step(); opt.zero_grad(set_to_none=True)
        return step, pc

    def captured_side():
        pc = SynthGaussians(student, device=DEV)
        opt = pc.training_setup(FusedAdam, capturable=True)
        for g in opt.param_groups:
            if g["name"] == "label":
                g["lr"] = 0.01
        gs = GraphedTrainStep(pc, opt, bg, label_phase=True, gated=True).capture(cams[0], obj_mask=objm[0], gate=1 - hand[0], warmup=2,
                                                                                capacity_margin=2.0)
        frames = [pack_label_frame(cams[k], objm[k % 4], 1 - hand[k % 4]) for k in range(n_fr)]
        return (lambda i: gs(frames[i % n_fr])), gs

    sides = {}
    sides["(i) eager, with the unused render()"], pc_i = eager_side(True)
    sides["(ii) eager, label render only"], _ = eager_side(False)
    sides["(iii) captured label step"], gs = captured_side()
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
    ok = gs.ok()

    # the backward's two kernels on one frame, by the library's HIP events
    def stage_ms(run, n=12):
        lib.profile_begin(max_records=64 * n)
        for _ in range(n):
            run()
        torch.cuda.synchronize()
        st = lib.profile_end()
        return {k: v[0] / max(v[1], 1) for k, v in st.items() if k in ("render_backward", "preprocess_backward")}

    def colours_only():
        lab = get_render_label(cams[3], pc_i, bg)
        lab.backward(torch.ones_like(lab)); pc_i._label.grad = None
    old = stage_ms(colours_only)
    up = torch.ones(1, device=DEV)

    def scalar_in_blend():
        lab = get_render_label(cams[3], pc_i, bg, scalar=True)
        from egogaussian_amd.fused import label_bce_loss
        label_bce_loss(lab, objm[3], grad_gate=(1 - hand[3])[0], defer_value=True, raster_lossgrad=True).backward(); pc_i._label.grad = None
    new = stage_ms(scalar_in_blend)

    lines = ["# Label phase: the captured step against the eager routes", "",
             f"`python tools/time_label_phase.py` -- {N} Gaussians at {W} x {H}, one process, the sides alternating; {a.reps} repetitions of >= {a.seconds:.0f} s "
             f"per side.  Library source hash {lib.built_source_hash()}.", "",
             "| side | it/s (median) | min | max | spread |", "|---|---|---|---|---|"]
    for k, v in rates.items():
        s = sorted(v)
        lines.append(f"| {k} | {s[len(s) // 2]:.0f} | {s[0]:.0f} | {s[-1]:.0f} | {100 * (s[-1] - s[0]) / s[len(s) // 2]:.1f} % |")
    lines += ["", f"Captured step: every replayed frame fit the captured capacity: {ok}.", "",
              "Backward kernels on one frame (HIP events around the launches, mean of 12):", "",
              "| route | blend | per-Gaussian launch | sum |", "|---|---|---|---|",
              f"| k_render_backward<0, false> + k_colors_from_acc | {1e3 * old['render_backward']:.1f} us | {1e3 * old['preprocess_backward']:.1f} us | "
              f"{1e3 * (old['render_backward'] + old['preprocess_backward']):.1f} us |",
              f"| k_render_backward<3, true> + k_label_finish | {1e3 * new['render_backward']:.1f} us | {1e3 * new['preprocess_backward']:.1f} us | "
              f"{1e3 * (new['render_backward'] + new['preprocess_backward']):.1f} us |", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
