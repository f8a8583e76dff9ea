#!/usr/bin/env python
"""Stage 4 (pose interpolation, PoseSequence.interpolated) timed: the one launch of egs_pose_interpolate over all gaps of a sequence against
the float32 torch mirror (poses.decompose_transform, the algorithm the reference runs through Python autograd) on the same box's CPU.

Workloads.  (1) 300 frames, two dynamic phases, every fourth dynamic frame held out: each held-out frame and the key after it form a gap of
2.  (2) a table with gaps of 8 and of 32.  The keys' poses are slow rigid motions (a few mrad and a few 1e-3 per frame).
The launch is timed by device events around back-to-back launches (the entry reads its status word back, so each call ends with a stream
synchronise: its cost is inside the figure); interpolated(check=False) as a whole -- plan, table, launch, accumulation -- by the wall clock.
The mirror is timed on --mirror-gaps gaps per workload and reported per gap.

    python tools/time_pose_interpolation.py --out profiles/pose_interpolation.md
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_object_stage import DEV, rigid      # noqa: E402

PHASES = [(60, 139), (160, 259)]


def sequence(keys, poses_mod, per_frame=1.0):
    """A table over `keys` whose entry k is the motion since the key before it: slow, and longer over a longer distance."""
    seq = poses_mod.PoseSequence(keys, DEV)
    prev = None
    for i, k in enumerate(sorted(keys)):
        d = per_frame * (1 if prev is None else k - prev)
        T = rigid(3e-3 * d * (1 + i % 3), (2e-3 * d, -1e-3 * d * (1 + i % 2), 1.5e-3 * d))
        seq.set(k, T[:3, 3], T[:3, :3])
        prev = k
    seq.accumulate()
    return seq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--mirror-gaps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd import lib, poses, _hip
    L = lib.load()
    dev = torch.device(DEV)

    frames1 = list(range(300))
    dynamic = [f for p in PHASES for f in range(p[0], p[1] + 1)]
    held = {f for i, f in enumerate(dynamic) if i % 4 == 2}
    keys1 = [f for f in dynamic if f not in held]
    # (2): keys every 8 frames over the first phase, every 32 over the second (whose first frame is a key: the walk loses it otherwise)
    keys2 = [PHASES[0][0] - 1 + 8 * j for j in range(0, 11)] + [PHASES[1][0]] + [PHASES[1][0] + 32 * j for j in range(1, 4)]
    workloads = [("300 frames, every fourth dynamic frame held out", frames1, keys1, 1.0),
                 ("gaps of 8 and of 32", frames1, keys2, 0.25)]

    rows, notes = [], []
    for title, frames, keys, per_frame in workloads:
        old = sequence(keys, poses, per_frame)
        new = old.interpolated(frames, PHASES, check=False)                  # (also the warm-up)
        torch.cuda.synchronize()
        gaps = new.gaps
        G = len(gaps)
        lengths = sorted({n for _, n, _ in gaps})
        t0 = time.perf_counter()
        for _ in range(5):
            new = old.interpolated(frames, PHASES, check=False)
        torch.cuda.synchronize()
        whole_ms = (time.perf_counter() - t0) * 1e3 / 5
        words = torch.tensor(gaps, dtype=torch.int32).to(DEV)
        res, status = torch.zeros(G, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)

        def launch():
            with _hip.device_ctx(dev):
                lib.check(L.egs_pose_interpolate(old.struct(), new.struct(), words.data_ptr(), G, poses.DESCENT_ITERS, poses.DESCENT_LR, res.data_ptr(),
                                                 status.data_ptr(), _hip.stream_of(dev)))
        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        torch.cuda.synchronize()
        launch_ms = e0.elapsed_time(e1) / a.launches
        residual = new.gap_residual.cpu()
        # the float32 mirror on the CPU, on a few gaps of every length
        rel = old.rel.cpu()
        mirror = {}
        for n in lengths:
            some = [g for g in gaps if g[1] == n][:a.mirror_gaps]
            t0 = time.perf_counter()
            worst = 0.0
            for first, _, old_row in some:
                t, R, _ = poses.decompose_transform(rel[old_row], n)
                row = torch.cat([R, t[:, None]], dim=1).reshape(12)
                worst = max(worst, float((row - new.rel[first].cpu()).abs().max()))
            mirror[n] = ((time.perf_counter() - t0) / len(some), len(some), worst)
        count = {n: sum(1 for g in gaps if g[1] == n) for n in lengths}
        mirror_all = sum(mirror[n][0] * count[n] for n in lengths)
        rows.append((title, G, ", ".join(f"{count[n]} x n = {n}" for n in lengths), launch_ms, whole_ms, mirror_all))
        for n in lengths:
            notes.append(f"| {title} | {n} | {mirror[n][1]} | {mirror[n][0]:.2f} | {mirror[n][2]:.1e} |")
        notes.append(f"| {title} | residuals of the launch: max {float(residual.max()):.2e}, min {float(residual.min()):.2e} | | | |")

    name = torch.cuda.get_device_name(0)
    lines = ["# Stage 4, pose interpolation: one launch over all gaps against the float32 torch mirror on the CPU", "",
             f"`python tools/time_pose_interpolation.py --launches {a.launches} --mirror-gaps {a.mirror_gaps}` on {name}, library source hash "
             f"{lib.built_source_hash()}; {poses.DESCENT_ITERS} iterations, lr {poses.DESCENT_LR}.", "",
             f"Dynamic phases {PHASES} of 300 frames.  `launch`: device events around {a.launches} back-to-back calls of `egs_pose_interpolate` (each "
             "call ends with the read-back of its status word, so the figure includes one stream synchronise).  `interpolated()`: the whole method "
             "with check=False -- plan, new table, launch, accumulation -- by the wall clock, mean of 5.  `mirror, all gaps`: the per-gap time of "
             "`poses.decompose_transform` in float32 on this box's CPU (measured on a few gaps per length, table below) times the number of gaps.", "",
             "| workload | gaps | lengths | launch, ms | interpolated(), ms | mirror, all gaps, s |", "|---|---|---|---|---|---|"]
    lines += [f"| {t} | {G} | {ls} | {lm:.3f} | {wm:.2f} | {ma:.1f} |" for t, G, ls, lm, wm, ma in rows]
    lines += ["", "The mirror per gap (and the largest distance of its end point from the launch's rows, over the twelve floats):", "",
              "| workload | n | gaps timed | s per gap | max distance from the launch's row |", "|---|---|---|---|---|"] + notes
    lines += ["", "The reference itself (Python autograd, 1500 iterations) is not on this machine; measured in the build container on the CPU it took "
              "3.8 s, 2.0 s, 1.9 s and 2.6 s per gap at n = 2, 5, 10 and 30."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
