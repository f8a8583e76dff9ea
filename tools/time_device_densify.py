#!/usr/bin/env python
"""What one densification costs, both ways, on the same state (profiles/device_densify.md):

    python tools/time_device_densify.py --out profiles/device_densify.md

Config C's model (500k Gaussians, SH degree 0) in a capacity-sized allocation with Adam moments and densification statistics
such that about one row in ten clones or splits.  Per round the state is restored in place and one densification runs through
  host    densify.densify_and_prune: the plan, one host read of the counts, ~60 torch launches (the parent's route), measured twice
          per round (the A/A spread of the method);
  device  densify.DeviceDensify.replay: the rule block, one graph launch, nothing read back.
Wall time is taken around the call (and again up to the point the device is idle); device time is taken with events around the
enqueued chain.  Then examples/train_synth.py's schedule runs both ways, alternating, in it/s."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from egogaussian_amd import densify                                             # noqa: E402
from egogaussian_amd.capacity import CapacityGaussians                          # noqa: E402
from egogaussian_amd.scene_synth import make_scene                              # noqa: E402


def build(n, capacity, sh_degree, dev):
    pc = CapacityGaussians(make_scene(n, 540, 960, 0, sh_degree=sh_degree), capacity, device=dev, sh_degree=sh_degree)
    pc.training_setup(capturable=True)
    for g in pc.optimizer.param_groups:                                         # one step: the moments exist, at their final addresses
        g["params"][0].grad = torch.zeros_like(g["params"][0])
    pc.optimizer.step(); pc.optimizer.zero_grad(set_to_none=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        pc.denom[:n] = torch.randint(1, 5, (n, 1), device=dev, generator=gen).float()
        pc.xyz_gradient_accum[:n] = torch.rand(n, 1, device=dev, generator=gen) * 1e-3 * pc.denom[:n]
        pc.max_radii2D[:n] = torch.rand(n, device=dev, generator=gen) * 15
        for st in pc.optimizer.state.values():
            if "exp_avg" in st:
                st["exp_avg"].normal_(generator=gen); st["exp_avg_sq"].uniform_(generator=gen)
    return pc


def arrays_of(pc):
    out = [getattr(pc, a) for a in densify._ATTR.values()] + [pc._generation, pc._is_object, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D]
    for st in pc.optimizer.state.values():
        out += [st[m] for m in ("exp_avg", "exp_avg_sq") if m in st]
    return [t.detach() for t in out if t.numel()]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--capacity-factor", type=float, default=1.5)
    ap.add_argument("--sh-degree", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--share", type=float, default=0.10, help="fraction of the rows whose mean gradient is over the threshold")
    ap.add_argument("--schedule-runs", type=int, default=2, help="runs of examples/train_synth.py per route (0: skip)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n, cap = a.gaussians, int(a.gaussians * a.capacity_factor)
    pc = build(n, cap, a.sh_degree, dev)
    arrays = arrays_of(pc)
    pristine = [t.clone() for t in arrays]
    mean_grad = (pc.xyz_gradient_accum[:n] / pc.denom[:n]).flatten()
    max_grad = float(torch.quantile(mean_grad[:min(n, 1 << 20)], 1.0 - a.share))
    extent = float(torch.exp(pc._scaling.detach()[:n]).max(1).values.median()) / pc.percent_dense      # half of the selected rows clone, half split
    rules = dict(max_grad=max_grad, min_opacity=0.005, extent=extent, max_screen_size=None)
    dd = densify.DeviceDensify(pc).capture()

    def restore():
        with torch.no_grad():
            for t, p in zip(arrays, pristine):
                t.copy_(p)
        pc.set_active(n)
        torch.cuda.synchronize()

    def host():
        restore()
        t0 = time.perf_counter()
        n0, n1 = densify.densify_and_prune(pc, **rules)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return dict(call_ms=(t1 - t0) * 1e3, idle_ms=(time.perf_counter() - t0) * 1e3, n_new=n1)

    def device():
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(); dd.replay(**rules); e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return dict(call_ms=(t1 - t0) * 1e3, idle_ms=(t2 - t0) * 1e3, device_ms=e0.elapsed_time(e1), n_new=pc.n_active)

    for _ in range(2):
        host(); device()
    rows = [(host(), device(), host()) for _ in range(a.rounds)]
    med = lambda xs: statistics.median(xs)
    h_idle = med([r[0]["idle_ms"] for r in rows] + [r[2]["idle_ms"] for r in rows])
    aa = med([abs(r[0]["idle_ms"] - r[2]["idle_ms"]) for r in rows]) / h_idle
    d_idle, d_call, d_dev = med([r[1]["idle_ms"] for r in rows]), med([r[1]["call_ms"] for r in rows]), med([r[1]["device_ms"] for r in rows])
    st = dd.check()
    lines = ["# One densification: host-driven route and device route on the same state", "",
             f"`python tools/time_device_densify.py` on {torch.cuda.get_device_name(0)}; medians over {a.rounds} rounds, each round host / device / host "
             "on the state restored in place.", "",
             f"Model: {n} live Gaussians in {cap} rows, SH degree {a.sh_degree}, {len(arrays)} per-Gaussian arrays; "
             f"{rows[0][0]['n_new']} rows afterwards (host) / {rows[0][1]['n_new']} (device; its own draws), threshold at the {100 * (1 - a.share):.0f}th "
             f"percentile of the mean gradient, half of the selected rows clone and half split.",
             f"Apply scratch: {dd.scratch_bytes / 2 ** 20:.1f} MiB = {dd.scratch_bytes // cap} bytes per row of capacity (the bytes of the arrays it rewrites); "
             f"plan buffers {(dd.plan_scratch.numel() + 19 * cap + 40) / 2 ** 20:.1f} MiB; z {dd.z.numel() * 4 / 2 ** 20:.1f} MiB.", "",
             "| route | wall, call returns (ms) | wall, device idle (ms) | device events around the chain (ms) |", "|---|---|---|---|",
             f"| host-driven `densify_and_prune` | {med([r[0]['call_ms'] for r in rows]):.3f} | {h_idle:.3f} | -- (reads the counts mid-way) |",
             f"| `DeviceDensify.replay` | {d_call:.3f} | {d_idle:.3f} | {d_dev:.3f} |", "",
             f"A/A spread of the host route (median |first - second| of a round / median): {100 * aa:.1f} %.  "
             f"Device route / host route, wall to idle: {d_idle / h_idle:.2f}x.  Status after the runs: {st}.", ""]
    if a.schedule_runs > 0:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
        import train_synth
        argv0, sys.argv = sys.argv, ["train_synth.py"]
        res = {False: [], True: []}
        train_synth.main(["--iters", "600"])                                      # (the process's first run pays for every lazy start: not counted)
        for _ in range(a.schedule_runs):
            for flag in (False, True):
                m = train_synth.main(["--iters", "600"] + (["--device-densify"] if flag else []))
                res[flag].append((m.train_report["its_per_s"], m.train_report["gaussians_end"], m.train_report["psnr_end"]))
        sys.argv = argv0
        lines += ["## examples/train_synth.py, default schedule (20k Gaussians, 270 x 480, 600 iterations, densify at 200, 300, 400)", "",
                  "| route | it/s per run | Gaussians at the end | held-out PSNR (dB) |", "|---|---|---|---|"]
        for flag, name in ((False, "host-driven (default)"), (True, "`--device-densify`")):
            lines.append(f"| {name} | {', '.join(f'{r[0]:.0f}' for r in res[flag])} | {', '.join(str(r[1]) for r in res[flag])} | "
                         f"{', '.join(f'{r[2]:.2f}' for r in res[flag])} |")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
