#!/usr/bin/env python
"""Timing record of the evaluation pass, everything in ONE process, the routes alternating:

  (a) kernel: egs_eval_metrics (strips + the one-wave finish) at 3 x 540 x 960 by device events, against egs_l1_ssim_forward (k_l1_ssim_forward
      + k_l1_ssim_finish) at the same shape -- the loss forward walks the same strips and additionally stores three derivative maps, so the
      metric kernel is expected to take no longer.  With and without `keep`, with and without the two byte images.
  (b) sweep, frames/s over 32 posed frames (rot_cov, the object placed by the frame's pose, a hand mask per frame):
        (i)   EvalPass(graphed=True)      one copy + one graph replay per frame, one host read per sweep
        (ii)  EvalPass(graphed=False)     the same calls eagerly
        (iii) the reference's formulation with the pieces the package had before: render(), the quantisation and the masking as torch ops,
              losses.ssim / losses.psnr, .item() per frame

Workload: N Gaussians (default 100 000) at 960 x 540, 32 cameras.  Every route is warmed up; a repetition is at least --seconds of timed work
per route, ended by a device synchronise; --reps repetitions, whose spread is reported.  Writes a markdown record (--out); --resources FILE
appends the compiler's resource report of csrc/eval_metrics.hip (hipcc -Rpass-analysis=kernel-resource-usage, collected at build time).

    python tools/time_eval_pass.py --out profiles/eval_pass.md --resources <report>
"""
import argparse
import math
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
HBM_PEAK = 8.0e12            # bytes/s, the MI355X's specified HBM3E rate


def _pose(angle, t):
    a = np.array([0.3, 1.0, 0.2]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R, c = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K), np.array([0.0, 0.0, 6.0])
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = c - R @ c + np.asarray(t)
    return torch.tensor(T, dtype=torch.float32)


def _stats(v):
    s = sorted(v)
    med = s[len(s) // 2]
    return med, s[0], s[-1], 100.0 * (s[-1] - s[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    from egogaussian_amd import fused, lib, losses, motion
    from egogaussian_amd.evaluate import EvalPass
    from egogaussian_amd.graph import pack_frame
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    if not torch.cuda.is_available():
        raise SystemExit("time_eval_pass.py measures on a HIP device; none is available")
    L = lib.load()
    N, H, W, F = a.n, a.height, a.width, a.frames
    p = lambda t: None if t is None else t.data_ptr()
    stream = fused._stream(torch.device(DEV))

    # ---- (a) the kernel -----------------------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(3)
    img = torch.rand(3, H, W, generator=gen).to(DEV)
    gt = (img.cpu() + 0.1 * torch.randn(3, H, W, generator=gen)).clamp(0, 1).to(DEV)
    keep = (torch.rand(H, W, generator=gen) > 0.3).float().to(DEV)
    partial = torch.empty(int(L.egs_eval_metrics_partial_bytes(3, H, W)), dtype=torch.uint8, device=DEV)
    rows, cursor = fused.eval_rows(1, DEV)
    q1, q2 = (torch.empty((3, H, W), dtype=torch.uint8, device=DEV) for _ in range(2))
    lpart = torch.empty(L.egs_l1_ssim_partial_count(3, H, W), device=DEV)
    maps = torch.empty((3, 3, H, W), device=DEV)
    lval = torch.empty(1, device=DEV)

    def ev_call(k, qa, qb):
        return lambda: lib.check(L.egs_eval_metrics(3, H, W, p(img), p(gt), p(k), None, p(partial), p(qa), p(qb), p(rows), 0, p(cursor), stream))
    kernels = {
        "egs_l1_ssim_forward (k_l1_ssim_forward + finish; stores 3 maps)":
            lambda: lib.check(L.egs_l1_ssim_forward(3, H, W, p(img), p(gt), 0.2, p(lpart), p(maps[0]), p(maps[1]), p(maps[2]), p(lval), None, stream)),
        "egs_l1_ssim_forward, value deferred (k_l1_ssim_forward alone)":
            lambda: lib.check(L.egs_l1_ssim_forward(3, H, W, p(img), p(gt), 0.2, p(lpart), p(maps[0]), p(maps[1]), p(maps[2]), None, None, stream)),
        "egs_eval_metrics, keep, no byte images": ev_call(keep, None, None),
        "egs_eval_metrics, keep, both byte images": ev_call(keep, q1, q2),
        "egs_eval_metrics, all kept, no byte images": ev_call(None, None, None),
    }
    for fn in kernels.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ktimes = {k: [] for k in kernels}
    calls = 200
    for _ in range(a.reps):
        for name, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ktimes[name].append(1e3 * e0.elapsed_time(e1) / calls)             # us per call (two launches each), back to back on one stream

    # ---- (b) the sweep ------------------------------------------------------------------------------------------------------------
    teacher = make_scene(N, H, W, seed=0)
    student = perturb_student(teacher)
    bg = torch.zeros(3, device=DEV)
    g2 = torch.Generator().manual_seed(11)
    is_obj = (torch.rand(N, 1, generator=g2) < 0.3).float().to(DEV)
    is_obj[0, 0] = 0.0
    cams = [make_camera(k * 9, H, W, device=DEV) for k in range(F)]
    Ts = [_pose(0.1 + 0.01 * k, (0.3 - 0.01 * k, -0.2, 0.3)).to(DEV) for k in range(F)]
    keeps = []
    for k in range(F):
        m = torch.ones(H, W, device=DEV)
        m[100 + 5 * k:300 + 5 * k, 200 + 10 * k:500 + 10 * k] = 0.0
        keeps.append(m)
    with torch.no_grad():
        gts = []
        for k in range(F):
            tpc = SynthGaussians(teacher, device=DEV, requires_grad=False)
            tpc._xyz = motion.move_points(tpc._xyz, Ts[k][:3], is_obj == 1)
            gts.append(losses.quantize8(render(cams[k], tpc, Pipe, bg)["render"]).float() / 255)
        del tpc
    frames = torch.stack([pack_frame(cams[k], gts[k], accum_R=Ts[k][:3, :3].contiguous(), gate=keeps[k], accum_T=Ts[k]) for k in range(F)])

    def model():
        pc = SynthGaussians(student, device=DEV, requires_grad=False)
        pc._is_object = is_obj
        return pc
    ev_g = EvalPass(model(), bg, dynamic=True, motion=True, which_object=1, graphed=True)
    ev_e = EvalPass(model(), bg, dynamic=True, motion=True, which_object=1, graphed=False)
    pc_r = model()
    last = {}

    def reference_route():
        ps, ss = [], []
        with torch.no_grad():
            for k in range(F):
                x = render(cams[k], pc_r, Pipe, bg, rot_cov=True, which_object=1, object_motion=motion.ObjectMotion(Ts[k]))["render"]
                q = lambda v: v.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).float().div(255)
                u, v = q(x) * keeps[k], q(gts[k]) * keeps[k]
                ss.append(losses.ssim(u, v).item())
                ps.append(losses.psnr(u[None], v[None]).mean().item())
        last["ref"] = (float(np.mean(ps)), float(np.mean(ss)))
    routes = {
        "(i) EvalPass(graphed=True)": lambda: last.__setitem__("graphed", ev_g.run(frames, cams[0], capacity_margin=1.5)),
        "(ii) EvalPass(graphed=False)": lambda: last.__setitem__("eager", ev_e.run(frames, cams[0])),
        "(iii) render() + torch quantise / mask + losses.ssim / psnr, .item() per frame": reference_route,
    }
    for fn in routes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rates = {k: [] for k in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():
            n, t0 = 0, time.perf_counter()
            while True:
                fn()
                n += F
                if time.perf_counter() - t0 >= a.seconds:
                    break
            torch.cuda.synchronize()
            rates[name].append(n / (time.perf_counter() - t0))
    g, e, ref = last["graphed"], last["eager"], last["ref"]

    # ---- the record -----------------------------------------------------------------------------------------------------------------
    props = torch.cuda.get_device_properties(0)
    read_b, write_b = 3 * H * W * 8 + H * W * 4, 3 * H * W * 2
    lines = ["# Evaluation pass: the metric kernel and the captured sweep", "",
             f"`python tools/time_eval_pass.py` -- one process, the routes alternating, every route warmed up; {a.reps} repetitions.  "
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  Library source hash {lib.built_source_hash()}.", "",
             f"## (a) Kernel at 3 x {H} x {W}", "",
             f"Device events around {calls} back-to-back calls (two launches per call: the strips and a finishing launch), us per call.", "",
             "| call | us (median) | min | max | spread |", "|---|---|---|---|---|"]
    for k, v in ktimes.items():
        med, lo, hi, sp = _stats(v)
        lines.append(f"| {k} | {med:.2f} | {lo:.2f} | {hi:.2f} | {sp:.1f} % |")
    t_keep = _stats(ktimes["egs_eval_metrics, keep, no byte images"])[0] * 1e-6
    t_both = _stats(ktimes["egs_eval_metrics, keep, both byte images"])[0] * 1e-6
    t_loss = _stats(ktimes["egs_l1_ssim_forward (k_l1_ssim_forward + finish; stores 3 maps)"])[0] * 1e-6
    lines += ["", f"Algorithmic bytes: 3HW*8 + HW*4 = {read_b / 1e6:.2f} MB read (+ 3HW*2 = {write_b / 1e6:.2f} MB written with both byte images).  Over the call time: "
              f"{read_b / t_keep / 1e12:.3f} TB/s = {100 * read_b / t_keep / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak without the byte images, "
              f"{(read_b + write_b) / t_both / 1e12:.3f} TB/s = {100 * (read_b + write_b) / t_both / HBM_PEAK:.1f} % with them (algorithmic: the halo re-reads "
              f"are not counted, and the call includes the finishing launch).",
              f"Against the loss forward: {t_keep * 1e6:.2f} us vs {t_loss * 1e6:.2f} us ({100 * (t_keep / t_loss - 1):+.1f} %).", "",
              f"## (b) Sweep: {N} Gaussians at {W} x {H}, {F} posed frames, a hand mask per frame", "",
              f"frames/s; a repetition is whole sweeps for >= {a.seconds:.0f} s, ended by a device synchronise.", "",
              "| route | frames/s (median) | min | max | spread |", "|---|---|---|---|---|"]
    for k, v in rates.items():
        med, lo, hi, sp = _stats(v)
        lines.append(f"| {k} | {med:.0f} | {lo:.0f} | {hi:.0f} | {sp:.1f} % |")
    lines += ["", f"Figures of the last sweep: captured PSNR {g['mean_psnr']:.4f} dB, SSIM {g['mean_ssim']:.6f} ({len(g['rerendered'])} frame(s) rendered again, "
              f"instance capacity {ev_g.capacity}); eager {e['mean_psnr']:.4f} dB, {e['mean_ssim']:.6f}; route (iii), float32 torch: {ref[0]:.4f} dB, {ref[1]:.6f}.", ""]
    if a.resources and os.path.exists(a.resources):
        keep_words = ("Function Name", "SGPRs:", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy", "LDS Size", "Spill")
        lines += ["## Compiler resource report (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/eval_metrics.hip)", "", "```"]
        for ln in open(a.resources):
            if "remark:" in ln and any(w in ln for w in keep_words):
                text = ln.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
                lines.append(re.sub(r"^\S+:\d+:\d+:\s*", "", text))           # (drop the source location the compiler puts in front)
        lines += ["```", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
