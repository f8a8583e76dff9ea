#!/usr/bin/env python
"""Cost of the deterministic backward blend (EGS_CALL_DETERMINISTIC, include/egs_raster.h): the captured training step with and without it,
two routes in ONE process, alternating:

  (a) default        GraphedTrainStep(...)                      the backward blend publishes with float atomics
  (b) deterministic  GraphedTrainStep(..., deterministic=True)  two integer passes of the blend, a clear and a decode launch

Workload: config C of BASELINE.md by default -- N = 500 000 Gaussians at 960 x 540, SH degree 0, frames of the synthetic orbit.  A
repetition is at least --seconds of timed replays per side, ended by a device synchronise; --reps repetitions; side (a) is measured twice per
repetition (a, a'): the distance of the two medians is the A/A spread.  Also: the kernels of one replay of each side with their durations
(torch.profiler, mean of --profile-replays replays), the scratch bytes of both modes, and -- the point of the mode -- whether two runs of each
route from the same seeded start end on the same bits.

    python tools/time_deterministic_backward.py --out profiles/deterministic_backward.md
"""
import argparse
import collections
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
LEAVES = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")


def kernel_times(fn, replays):
    """[(kernel name, launches per replay, mean microseconds per launch)] of fn(), in order of first start (torch.profiler)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(replays):
                fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memcpy" not in e.name and "Memset" not in e.name]
        ev.sort(key=lambda e: e.time_range.start)
        short = lambda s: s.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        acc = collections.OrderedDict()
        for e in ev:
            n, us = acc.get(short(e.name), (0, 0.0))
            acc[short(e.name)] = (n + 1, us + (e.time_range.end - e.time_range.start))
        return [(k, n / replays, us / n) for k, (n, us) in acc.items()]
    except Exception as exc:                                            # (recorded in the profile, not hidden)
        return [(f"<profiler failed: {type(exc).__name__}: {exc}>", 0, 0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-replays", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame
    from egogaussian_amd import lib
    N, H, W = a.n, a.height, a.width
    teacher = make_scene(N, H, W, 0)
    student = perturb_student(teacher)
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in (0, 40, 80, 120)]
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=DEV, requires_grad=False)
        gts = [render(c, tpc, Pipe, bg)["render"].clone() for c in cams]
        del tpc
    frames = [pack_frame(c, g) for c, g in zip(cams, gts)]

    def build(det):
        pc = SynthGaussians(student, device=DEV)
        groups = [{"params": [pc._xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [pc._features_dc], "lr": 2.5e-3, "name": "f_dc"},
                  {"params": [pc._opacity], "lr": 0.05, "name": "opacity"}, {"params": [pc._scaling], "lr": 5e-3, "name": "scaling"},
                  {"params": [pc._rotation], "lr": 1e-3, "name": "rotation"}]
        opt = FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True)
        step = GraphedTrainStep(pc, opt, bg, 0.2, deterministic=det).capture(cams[0], gts[0], warmup=2, capacity_cams=cams, capacity_margin=1.5)
        return pc, opt, step

    def state(pc, opt):
        return [t.detach().clone() for a_ in LEAVES for t in (getattr(pc, a_), opt.state[getattr(pc, a_)]["exp_avg"], opt.state[getattr(pc, a_)]["exp_avg_sq"])]

    same = lambda x, y: all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))

    # 1. the point of the mode: two runs of 20 replays from the seeded start, each route
    repro = {}
    for det in (False, True):
        ends = []
        for _ in range(2):
            pc, opt, step = build(det)
            for i in range(20):
                step(frames[i % 4])
            torch.cuda.synchronize()
            assert step.ok()
            ends.append(state(pc, opt))
            del pc, opt, step
        repro[det] = same(ends[0], ends[1])

    # 2. the rates, alternating
    pc_a, opt_a, step_a = build(False)
    pc_b, opt_b, step_b = build(True)

    def timed(step, seconds):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while True:
            for _ in range(20):
                step(frames[n % 4]); n += 1
            if time.perf_counter() - t0 >= seconds:
                break
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for n in range(8):
        step_a(frames[n % 4]); step_b(frames[n % 4])
    torch.cuda.synchronize()
    rates = {"a": [], "b": [], "a'": []}
    for _ in range(a.reps):
        rates["a"].append(timed(step_a, a.seconds))
        rates["b"].append(timed(step_b, a.seconds))
        rates["a'"].append(timed(step_a, a.seconds))
    assert step_a.ok() and step_b.ok()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    aa = abs(med(rates["a"]) - med(rates["a'"])) / med(rates["a"])
    us = lambda r: 1e6 / r
    extra_us = us(med(rates["b"])) - us(med(rates["a"] + rates["a'"]))
    ratio = med(rates["a"] + rates["a'"]) / med(rates["b"])
    ka = kernel_times(lambda: step_a(frames[1]), a.profile_replays)
    kb = kernel_times(lambda: step_b(frames[1]), a.profile_replays)
    base, det_bytes = lib.load().egs_backward_scratch_bytes(N), lib.load().egs_backward_scratch_bytes_ex(N, lib.CALL_DETERMINISTIC)

    name = torch.cuda.get_device_name(0)
    lines = ["# Deterministic backward blend: the captured step with and without EGS_CALL_DETERMINISTIC", "",
             f"`python tools/time_deterministic_backward.py --n {N} --height {H} --width {W} --seconds {a.seconds} --reps {a.reps}` on {name}, library "
             f"source hash {lib.built_source_hash()}.", "",
             f"Workload: {N} Gaussians at {W} x {H}, SH degree 0, four frames of the synthetic orbit, `GraphedTrainStep` defaults (optimizer and loss "
             f"gradient inside the rasterizer's backward).  Both routes run in one process and alternate (a, b, a'); each repetition is at least "
             f"{a.seconds} s of replays per side, ended by a device synchronise.", "",
             "| route | steps / s, each repetition | median | us / step | spread (max - min) / median |", "|---|---|---|---|---|"]
    label = {"a": "(a) default", "b": "(b) `deterministic=True`", "a'": "(a') default again"}
    for r in ("a", "b", "a'"):
        lines.append(f"| {label[r]} | {', '.join(f'{v:.0f}' for v in rates[r])} | {med(rates[r]):.0f} | {us(med(rates[r])):.1f} | {100 * spread(rates[r]):.1f} % |")
    lines += ["", f"A/A spread (medians of a and a'): {100 * aa:.2f} %.  The deterministic step takes {extra_us:+.1f} us more per iteration than the default "
              f"one: the default step runs at {ratio:.3f} x its rate.", "",
              f"Scratch of one backward: {base} bytes by default, {det_bytes} bytes with the flag ({det_bytes - base} more: 12 uint32 maxima and 12 int64 "
              f"sums per Gaussian).", "",
              "Two runs of 20 replays from the same seeded start end on the same bits (parameters and both moments of the five leaves): "
              f"default **{'yes' if repro[False] else 'no'}**, deterministic **{'yes' if repro[True] else 'no'}**.", "",
              "## Kernels of one replay", "",
              f"torch.profiler, mean over {a.profile_replays} replays; launches per replay and microseconds per launch, in order of first start.", ""]
    for title, ks in (("(a) default", ka), ("(b) `deterministic=True`", kb)):
        lines += [f"{title}: {sum(n for _, n, _ in ks):.0f} launches, {sum(n * t for _, n, t in ks):.1f} us of kernel time", "", "| kernel | launches | us / launch |", "|---|---|---|"]
        lines += [f"| `{k}` | {n:g} | {t:.1f} |" for k, n, t in ks] + [""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
