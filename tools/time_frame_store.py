#!/usr/bin/env python
"""Record of the 8-bit frame store at BASELINE config C (500 000 Gaussians, 960 x 540, the 300-frame orbit, five iterations per replay, the
benched static step), everything in ONE process:

  Memory.    Resident dataset bytes, store against packed float32 frames: a count.
  Step rate. (A) today's path: one [S, frame] copy + replay, on packed float frames;
             (B) GraphedTrainStep(frame_store=): set_schedule() once, then bare replays -- the decode is the graph's first launch.
             The frames are quantised to 8 bits once and A's float frames are built FROM the store: both train on the same data, in the same
             order.  Regions alternate A, B, A, B, ...; a region is --replays replays closed by a device synchronise; --regions of them each,
             after a warm-up of both.  The spread between A's own regions is reported next to the A/B difference: A is this commit's
             packed-frame path, which the store does not touch.
  Calls.     Device events around back-to-back calls: the decode of S frames (two launches) and the [S, frame] copy it replaces, each with
             the bytes it needs (from the shapes) and its share of the achievable HBM rate.
  Kernels.   --kernel-trace FILE: the kernel_trace.csv of a separate `rocprofv3 --kernel-trace --stats --output-format csv -- python
             tools/time_frame_store.py --trace-only` run (nothing else traced in it): the decode's two kernels and the runtime's copy kernel.
  Results.   After the timed windows: is B's static frame buffer bit-identical to the float frames of its last replay (the same data), and
             are A's and B's parameters bit-identical (the same sequence of steps; at this size the backward's float atomics have no fixed
             order, so a difference here is reported with its size and with the difference between two A runs of the same frames).

    python tools/time_frame_store.py --out profiles/frame_store.md
"""
import argparse
import csv
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12      # bytes/s: the achievable HBM rate of the MI355X (8 TB/s specified)


def _stats(v):
    s = sorted(v)
    med = s[len(s) // 2]
    return med, s[0], s[-1], 100.0 * (s[-1] - s[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps-per-replay", type=int, default=5)
    ap.add_argument("--replays", type=int, default=300, help="replays per timed region")
    ap.add_argument("--regions", type=int, default=5, help="timed regions per variant (at least five)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="kernel_trace.csv of a separate rocprofv3 --kernel-trace --stats run of --trace-only")
    ap.add_argument("--trace-only", action="store_true", help="a short run of both variants for the profiler: no timing, no record")
    a = ap.parse_args()
    from egogaussian_amd import lib
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    if not torch.cuda.is_available():
        raise SystemExit("time_frame_store.py measures on a HIP device; none is available")
    N, H, W, F, S = a.n, a.height, a.width, a.frames, a.steps_per_replay
    if F % S or a.regions < 1:
        raise SystemExit("--frames must be a multiple of --steps-per-replay")
    if a.trace_only:
        F = min(F, 4 * S)
    teacher = make_scene(N, H, W, seed=0)
    student = perturb_student(teacher)
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in range(F)]
    store = FrameStore(H, W, F, DEV)                                      # the benched step's layout: image + camera
    with torch.no_grad():
        tpc = SynthGaussians(teacher, device=DEV, requires_grad=False)
        for k, c in enumerate(cams):
            store.put(k, c, gt=render(c, tpc, Pipe, bg)["render"], quantize=True)      # quantised once
        del tpc
    floats = store.frames()                                               # A's resident dataset, built from the store
    floats = torch.cat([floats, floats[:S - 1]]) if S > 1 else floats      # (frame order = step order, as bench.py keeps it)
    size = store.frame_floats

    def variant(kind):
        pc = SynthGaussians(student, device=DEV)
        opt = FusedAdam([{"params": [pc._xyz], "lr": 1.6e-4}, {"params": [pc._features_dc], "lr": 2.5e-3}, {"params": [pc._opacity], "lr": 0.05},
                         {"params": [pc._scaling], "lr": 5e-3}, {"params": [pc._rotation], "lr": 1e-3}], lr=0.0, eps=1e-15, capturable=True)
        kw = dict(capacity_cams=cams[::max(1, F // 6)], warmup=2)
        if kind == "B":
            step = GraphedTrainStep(pc, opt, bg, 0.2, steps_per_replay=S, frame_store=store).capture(cams[0], index=0, **kw)
            step.set_schedule(list(range(F)))
            return dict(pc=pc, opt=opt, step=step, run=lambda n: step(), n=0)
        step = GraphedTrainStep(pc, opt, bg, 0.2, steps_per_replay=S).capture(cams[0], store.parts(0)["gt"], **kw)
        return dict(pc=pc, opt=opt, step=step, run=lambda n: step(floats[(n * S) % F:(n * S) % F + S]), n=0)

    def replay(v, count):
        for _ in range(count):
            v["run"](v["n"])
            v["n"] += 1

    A, B = variant("A"), variant("B")
    if a.trace_only:
        for v in (A, B):
            replay(v, 8)
        torch.cuda.synchronize()
        print("trace-only run done")
        return
    A2 = variant("A")                                                     # a second A on the same frames: what two runs of ONE path differ by
    for v in (A, B, A2):
        replay(v, 20)
    torch.cuda.synchronize()
    rates = {"A": [], "B": []}
    for _ in range(max(5, a.regions)):
        for name, v in (("A", A), ("B", B)):
            t0 = time.perf_counter()
            replay(v, a.replays)
            torch.cuda.synchronize()
            rates[name].append(a.replays * S / (time.perf_counter() - t0))
    replay(A2, A["n"] - A2["n"])
    torch.cuda.synchronize()
    assert A["n"] == B["n"] == A2["n"]
    ok = A["step"].ok() and B["step"].ok() and A2["step"].ok() and B["step"].store_ok()

    # ---- results --------------------------------------------------------------------------------------------------------------------
    last = ((B["n"] - 1) * S) % F
    same_data = torch.equal(B["step"]._frames.view(torch.int32), floats[last:last + S].view(torch.int32))
    names = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")

    def compare(u, v):
        differing, worst = 0, 0.0
        for nm in names:
            x, y = getattr(u["pc"], nm).detach(), getattr(v["pc"], nm).detach()
            differing += int((x.view(torch.int32) != y.view(torch.int32)).sum())
            worst = max(worst, float((x - y).abs().max() / x.abs().max()))
        return differing, worst
    ab, aa = compare(A, B), compare(A, A2)
    total = sum(getattr(A["pc"], nm).numel() for nm in names)

    # ---- the two calls by device events ------------------------------------------------------------------------------------------------
    out = torch.empty((S, size), device=DEV)
    ring = store.new_ring(F)
    ring.set(list(range(F)))
    calls = {"decode of S frames from the store (two launches)": lambda: store.decode(out, ring=ring),
             "copy of S packed float frames": lambda: out.copy_(floats[0:S], non_blocking=True)}
    ctimes = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    n_calls = 200
    for _ in range(5):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ctimes[name].append(1e3 * e0.elapsed_time(e1) / n_calls)
    decode_bytes = S * (store.nbytes // F + 4 * size)                     # reads the stored frame, writes the float frame
    copy_bytes = S * 8 * size                                             # reads and writes the float frame
    cbytes = dict(zip(calls, (decode_bytes, copy_bytes)))

    # ---- the record ----------------------------------------------------------------------------------------------------------------------
    props = torch.cuda.get_device_properties(0)
    mA, mB = _stats(rates["A"]), _stats(rates["B"])
    lines = ["# 8-bit frame store: memory, step rate, the decode against the copy", "",
             f"`python tools/time_frame_store.py` -- one process; {N} Gaussians at {W} x {H}, {F} frames of the orbit, {S} iterations per replay, the "
             f"benched static step.  Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  Library source hash "
             f"{lib.built_source_hash()}.", "",
             "## Memory (a count, not a timing)", "",
             "| dataset | bytes | per frame |", "|---|---|---|",
             f"| packed float32 frames | {store.float_nbytes} | {store.float_nbytes // F} |",
             f"| 8-bit store | {store.nbytes} | {store.nbytes // F} |", "",
             f"Ratio {store.nbytes / store.float_nbytes:.4f} (this layout has no bit plane: 3 bytes against 12 per pixel, the camera block in float on both sides).", "",
             "## Step rate", "",
             f"(A) one [{S}, frame] copy + replay on packed float frames; (B) set_schedule() once, then bare replays on the store.  Regions alternate "
             f"A, B; a region is {a.replays} replays = {a.replays * S} iterations closed by a device synchronise; {len(rates['A'])} regions each after "
             f"20 warm-up replays of each.", "",
             "| variant | it/s (median) | min | max | spread between its regions |", "|---|---|---|---|---|",
             f"| A: copy + replay | {mA[0]:.0f} | {mA[1]:.0f} | {mA[2]:.0f} | {mA[3]:.2f} % |",
             f"| B: store, bare replay | {mB[0]:.0f} | {mB[1]:.0f} | {mB[2]:.0f} | {mB[3]:.2f} % |", "",
             f"B against A: {100.0 * (mB[0] - mA[0]) / mA[0]:+.2f} % in the medians; A's own regions spread over {mA[3]:.2f} % (A/A).  "
             f"Per region, in order: A {', '.join(f'{r:.0f}' for r in rates['A'])}; B {', '.join(f'{r:.0f}' for r in rates['B'])}.", "",
             "## The two calls", "",
             f"Device events around {n_calls} back-to-back calls on one stream, us per call; bytes from the shapes; share of the achievable HBM rate "
             f"({HBM_ACHIEVABLE / 1e12:.1f} TB/s).  Back-to-back calls on {S} frames re-read what the 256 MiB Infinity Cache may still hold: the share is of "
             f"the HBM rate as a yardstick, not a claim about where the bytes came from.", "",
             "| call | us (median) | min | max | bytes | TB/s | share |", "|---|---|---|---|---|---|---|"]
    for k, v in ctimes.items():
        med, lo, hi, _ = _stats(v)
        rate = cbytes[k] / (med * 1e-6)
        lines.append(f"| {k} | {med:.2f} | {lo:.2f} | {hi:.2f} | {cbytes[k]} | {rate / 1e12:.3f} | {100 * rate / HBM_ACHIEVABLE:.1f} % |")
    lines += ["", "## Kernels (rocprofv3 --kernel-trace --stats, a run of its own)", ""]
    if a.kernel_trace and os.path.exists(a.kernel_trace):
        rows = list(csv.DictReader(open(a.kernel_trace)))
        dur = lambda name: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
        dec, adv = dur("k_frame_decode"), dur("k_frame_advance")
        cp = sorted(dur("__amd_rocclr_copyBuffer"))[-len(dec):] if dec else []
        lines += [f"The `--trace-only` run replays A and B {len(dec)} times each on {S} different frames per replay.  The runtime's copy kernel serves every "
                  f"device copy of the run; the {len(cp)} longest of its {len(dur('__amd_rocclr_copyBuffer'))} dispatches are A's [{S}, frame] copies (nothing else in "
                  f"that run copies as much).", "",
                  "| kernel | dispatches | median ns | min | max | bytes | TB/s at the median | share of the achievable HBM rate |", "|---|---|---|---|---|---|---|---|"]
        for name, v, nbytes in (("k_frame_decode_vec (the decode launch)", dec, decode_bytes), ("k_frame_advance (the cursor)", adv, 0),
                                ("__amd_rocclr_copyBuffer (the copy it replaces)", cp, copy_bytes)):
            if v:
                med = sorted(v)[len(v) // 2]
                rate = nbytes / (med * 1e-9)
                lines.append(f"| {name} | {len(v)} | {med} | {min(v)} | {max(v)} | {nbytes or '-'} | " +
                             (f"{rate / 1e12:.3f} | {100 * rate / HBM_ACHIEVABLE:.1f} % |" if nbytes else "- | - |"))
    else:
        lines.append("Not measured in this record.")
    lines += ["", "## Results", "",
              f"B's static frames after its last replay against the float frames of the same schedule entries: "
              f"{'bit-identical' if same_data else 'DIFFERENT'}.  Every replay complete (no overflow, no clamped index): {ok}.",
              f"Parameters after {A['n']} replays ({A['n'] * S} iterations) of the same frames in the same order: A against B {ab[0]} of {total} values "
              f"differ (largest difference {ab[1]:.2e} of the array's largest magnitude); A against a second A {aa[0]} differ ({aa[1]:.2e})."
              + ("" if ab[0] == 0 else "  At this size the backward's float atomics have no fixed order, so two runs of ONE path differ as well; "
                 "tests/test_gpu_frames.py holds the two paths to bit-identity on a scene whose steps are deterministic."), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
