#!/usr/bin/env python
"""Timing record of the mask hand-off, everything in ONE process, the routes alternating:

  (a) kernels at 540 x 960 by device events: egs_label_mask (pixels + the one-wave finish; with target / keep / mask bytes, and the counts
      alone) against its torch formulation (mean over channels, >, the four masked counts, the byte mask), and egs_interaction_gate at k = 5
      (and 1, 15, 31) against the reference's formulation (logical_or, conv2d(ones(k, k), padding = k // 2) > 0, 1 - that).
  (b) sweep, frames/s over 32 frames with their own camera, hand mask and object mask:
        (i)   MaskPass(graphed=True)      one copy + one graph replay per frame, one host read per sweep
        (ii)  MaskPass(graphed=False)     the same calls eagerly
        (iii) the torch route: get_render_label() + mean + > + .cpu() per frame (what a trainer built on the label step did before)
  (c) interaction_gate against conv2d(...) > 0 at k = 5: the first table's two k = 5 rows, set side by side.

Workload: N Gaussians (default 100 000) at 960 x 540, 32 cameras.  Every route is warmed up; a repetition is at least --seconds of timed work
per route, ended by a device synchronise; --reps repetitions, whose spread is reported.  Writes a markdown record (--out); --resources FILE
appends the compiler's resource report of csrc/masks.hip (hipcc -Rpass-analysis=kernel-resource-usage, collected at build time).

    python tools/time_mask_pass.py --out profiles/mask_pass.md --resources <report>
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
HBM_PEAK = 8.0e12            # bytes/s, the MI355X's specified HBM3E rate


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
    from egogaussian_amd import fused, lib
    from egogaussian_amd.masks import MaskPass
    from egogaussian_amd.graph import pack_label_frame
    from egogaussian_amd.renderer import get_render_label
    from egogaussian_amd.scene_synth import make_scene, make_camera, SynthGaussians
    if not torch.cuda.is_available():
        raise SystemExit("time_mask_pass.py measures on a HIP device; none is available")
    L = lib.load()
    N, H, W, F = a.n, a.height, a.width, a.frames
    p = lambda t: None if t is None else t.data_ptr()
    stream = fused._stream(torch.device(DEV))

    # ---- (a) the kernels ----------------------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(3)
    img = (torch.randn(1, H, W, generator=gen) * 2).expand(3, H, W).contiguous().to(DEV)
    target = (torch.rand(H, W, generator=gen) > 0.6).float().to(DEV)
    keep = (torch.rand(H, W, generator=gen) > 0.3).float().to(DEV)
    hand = torch.zeros(H, W); hand[150:400, 300:650] = 1.0
    obj = torch.zeros(H, W); obj[200:330, 600:800] = 1.0
    hand, obj = hand.to(DEV), obj.to(DEV)
    partial = torch.empty(int(L.egs_label_mask_partial_bytes(H, W)), dtype=torch.uint8, device=DEV)
    rows, cursor = fused.mask_rows(1, DEV)
    m8 = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    gate = torch.empty((H, W), device=DEV)
    ones = {k: torch.ones(1, 1, k, k, device=DEV) for k in (5, 15, 31)}

    def lm_call(t, k, m):
        return lambda: lib.check(L.egs_label_mask(H, W, p(img), 0.5, p(t), p(k), None, p(partial), p(m), p(rows), 0, p(cursor), stream))

    def lm_torch():
        on = img.mean(0) > 0.5
        kept, tgt = keep >= 0.5, target >= 0.5
        return on.to(torch.uint8) * 255, torch.stack([(kept & on).sum(), (kept & tgt).sum(), (kept & on & tgt).sum(), kept.sum()])

    def gate_call(k):
        return lambda: lib.check(L.egs_interaction_gate(H, W, p(hand), p(obj), k, p(gate), stream))

    def gate_torch(k):
        def fn():
            m = torch.logical_or(hand, obj).int()
            if k > 1:
                m = (torch.nn.functional.conv2d(m.unsqueeze(0).unsqueeze(0).float(), ones[k], padding=k // 2) > 0).int()[0, 0]
            return 1 - m
        return fn
    kernels = {
        "egs_label_mask, target + keep + mask bytes": lm_call(target, keep, m8),
        "egs_label_mask, counts alone (no target, no keep, no bytes)": lm_call(None, None, None),
        "torch: mean(0) > 0.5, byte mask, four masked counts": lm_torch,
        "egs_interaction_gate, k = 1": gate_call(1),
        "egs_interaction_gate, k = 5": gate_call(5),
        "egs_interaction_gate, k = 15": gate_call(15),
        "egs_interaction_gate, k = 31": gate_call(31),
        "torch: 1 - (conv2d(logical_or, ones(5, 5), padding 2) > 0)": gate_torch(5),
        "torch: the same at k = 31": gate_torch(31),
    }
    # the two formulations of the gate agree on these inputs (the record is of equal work)
    gate_call(5)()
    assert torch.equal(gate, gate_torch(5)().float())
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
            ktimes[name].append(1e3 * e0.elapsed_time(e1) / calls)             # us per call, back to back on one stream

    # ---- (b) the sweep ------------------------------------------------------------------------------------------------------------
    scene = make_scene(N, H, W, seed=0)
    x = scene["xyz"][:, 0]
    label = torch.from_numpy(np.where(x < np.quantile(x, 0.3), 2.0, -2.0).astype(np.float32)[:, None]).to(DEV)
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k * 9, H, W, device=DEV) for k in range(F)]
    keeps, objs = [], []
    for k in range(F):
        m = torch.ones(H, W, device=DEV)
        m[100 + 5 * k:300 + 5 * k, 200 + 10 * k:500 + 10 * k] = 0.0
        o = torch.zeros(H, W, device=DEV)
        o[60 + 3 * k:420 + 3 * k, 0:300 + 4 * k] = 1.0
        keeps.append(m); objs.append(o)
    frames = torch.stack([pack_label_frame(cams[k], objs[k], gate=keeps[k]) for k in range(F)])

    def model():
        pc = SynthGaussians(scene, device=DEV, requires_grad=False)
        pc._label = label
        return pc
    mp_g, mp_e, pc_r = MaskPass(model(), bg, graphed=True), MaskPass(model(), bg, graphed=False), model()
    last = {}

    def torch_route():
        out = []
        with torch.no_grad():
            for k in range(F):
                binary = (get_render_label(cams[k], pc_r, bg).mean(0, keepdim=True) > 0.5)
                out.append(binary.cpu())
        last["torch"] = out
    routes = {
        "(i) MaskPass(graphed=True)": lambda: last.__setitem__("graphed", mp_g.run(frames, cams[0], capacity_margin=1.5)),
        "(ii) MaskPass(graphed=False)": lambda: last.__setitem__("eager", mp_e.run(frames, cams[0])),
        "(iii) get_render_label() + mean + > + .cpu() per frame": torch_route,
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
    g, e = last["graphed"], last["eager"]
    gm = g["masks"].cpu()
    differing = sum(int(((gm[k] == 255) != last["torch"][k][0]).sum()) for k in range(F))
    same = torch.equal(g["masks"], e["masks"]) and all(np.array_equal(g[k], e[k]) for k in ("predicted", "target", "intersection", "kept"))

    # ---- the record -----------------------------------------------------------------------------------------------------------------
    props = torch.cuda.get_device_properties(0)
    lines = ["# Mask hand-off: the two kernels and the captured sweep", "",
             f"`python tools/time_mask_pass.py` -- one process, the routes alternating, every route warmed up; {a.reps} repetitions.  "
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  Library source hash {lib.built_source_hash()}.", "",
             f"## (a) Kernels at {H} x {W}", "",
             f"Device events around {calls} back-to-back calls, us per call (egs_label_mask: two launches per call, the pixels and a finishing "
             f"launch; the torch rows: every launch of the expression).", "",
             "| call | us (median) | min | max | spread |", "|---|---|---|---|---|"]
    for k, v in ktimes.items():
        med, lo, hi, sp = _stats(v)
        lines.append(f"| {k} | {med:.2f} | {lo:.2f} | {hi:.2f} | {sp:.1f} % |")
    med = lambda name: _stats(ktimes[name])[0]
    t_lm, t_lm_t = med("egs_label_mask, target + keep + mask bytes"), med("torch: mean(0) > 0.5, byte mask, four masked counts")
    t_g5, t_g5_t = med("egs_interaction_gate, k = 5"), med("torch: 1 - (conv2d(logical_or, ones(5, 5), padding 2) > 0)")
    lm_bytes, g_bytes = H * W * (5 * 4 + 1), H * W * 3 * 4
    lines += ["", f"egs_label_mask moves 5 HW floats in and HW bytes out = {lm_bytes / 1e6:.2f} MB: {lm_bytes / (t_lm * 1e-6) / 1e12:.3f} TB/s = "
              f"{100 * lm_bytes / (t_lm * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak over the call time (which includes the finishing "
              f"launch); against the torch formulation {t_lm:.2f} us vs {t_lm_t:.2f} us ({t_lm_t / t_lm:.1f} x).",
              f"egs_interaction_gate moves 2 HW floats in and HW out = {g_bytes / 1e6:.2f} MB (algorithmic: the rows a wave re-reads above and below its "
              f"own are not counted): {g_bytes / (t_g5 * 1e-6) / 1e12:.3f} TB/s = {100 * g_bytes / (t_g5 * 1e-6) / HBM_PEAK:.1f} % of peak at k = 5.", "",
              "## (c) interaction_gate against conv2d(...) > 0 at k = 5", "",
              f"{t_g5:.2f} us vs {t_g5_t:.2f} us ({t_g5_t / t_g5:.1f} x), same inputs, same process; the two outputs are equal (checked before timing).", "",
              f"## (b) Sweep: {N} Gaussians at {W} x {H}, {F} frames with their own camera, hand mask and object mask", "",
              f"frames/s; a repetition is whole sweeps for >= {a.seconds:.0f} s, ended by a device synchronise.", "",
              "| route | frames/s (median) | min | max | spread |", "|---|---|---|---|---|"]
    for k, v in rates.items():
        m_, lo, hi, sp = _stats(v)
        lines.append(f"| {k} | {m_:.0f} | {lo:.0f} | {hi:.0f} | {sp:.1f} % |")
    r_g, r_t = _stats(rates["(i) MaskPass(graphed=True)"])[0], _stats(rates["(iii) get_render_label() + mean + > + .cpu() per frame"])[0]
    lines += ["", f"Captured against the torch route: {r_g / r_t:.2f} x.  Last sweep: mean IoU {g['mean_iou']:.4f}, {len(g['rerendered'])} frame(s) rendered again "
              f"(instance capacity {mp_g.capacity}), captured and eager sweeps {'byte-identical' if same else 'DIFFER'}; pixels where the captured mask and "
              f"route (iii)'s differ, all frames: {differing} (route (iii) renders from the activated parameters and takes torch's mean).", ""]
    if a.resources and os.path.exists(a.resources):
        keep_words = ("Function Name", "SGPRs:", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy", "LDS Size", "Spill")
        lines += ["## Compiler resource report (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/masks.hip)", "", "```"]
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
