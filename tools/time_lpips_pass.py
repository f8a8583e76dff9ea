#!/usr/bin/env python
"""Timing record of the LPIPS pass (egogaussian_amd/lpips.py LPIPS, csrc/lpips.hip), everything in ONE process:

  (a) the whole pass -- egs_lpips_forward, 20 launches -- on one pair of 8-bit images with a hand mask, and the torch statement
      (lpips.lpips_vgg, float32, weights resident) on the same device if F.conv2d runs there, the two ALTERNATING within each repetition;
      the fraction of the MI355X's 157.3 TFLOP/s fp32 matrix peak that the convolutions' FLOP over the pass's time amount to;
  (b) each of the 13 convolutions by itself (egs_conv3x3_relu_nhwc on a batch of 2 at the layer's size, output allocated once), with its
      own fraction of the peak and its store rate; what remains of (a) is the input kernel, the five tap kernels and the finishing wave.

What the figures are: device events around --calls (pass) / --layer-calls (layer) back-to-back launches from Python on one stream, divided
by the count -- wall time on the device's clock INCLUDING the gaps between launches, not kernel-trace durations; a kernel's own time is
at most this.  Random weights (LPIPSWeights.random): timing does not depend on the values.  Every route is warmed up; --reps repetitions,
whose spread is reported.  Writes a markdown record (--out).

    python tools/time_lpips_pass.py --out profiles/lpips_pass.md
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
MATRIX_PEAK = 157.3e12       # FLOP/s, fp32-input MFMA


def _stats(v):
    s = sorted(v)
    med = s[len(s) // 2]
    return med, s[0], s[-1], 100.0 * (s[-1] - s[0]) / med


def _time(fn, reps, calls):
    """ms per call: `reps` repetitions of `calls` back-to-back calls between two device events."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)               # ~0.3 s per window of the pass
    ap.add_argument("--layer-calls", type=int, default=200)        # 16 ms (conv1_1) .. 180 ms per window
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd import fused, lib, lpips as LP
    if not torch.cuda.is_available():
        raise SystemExit("time_lpips_pass.py measures on a HIP device; none is available")
    H, W = a.height, a.width
    weights = LP.LPIPSWeights.random(1)
    net = LP.LPIPS(weights, DEV)
    g = torch.Generator().manual_seed(5)
    qx = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    qy = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    keep = (torch.rand(H, W, generator=g) >= 0.2).float().to(DEV)
    rows, cursor = fused.lpips_rows(1, DEV)

    # ---- (a) the pass ---------------------------------------------------------------------------------------------------------------
    def whole():
        net(qx, qy, keep=keep, rows=rows, cursor=cursor)
    note, stmt = None, None
    try:
        x32, y32 = qx.float() / 255 * keep, qy.float() / 255 * keep
        wdev = weights.to(DEV)

        def stmt():
            with torch.no_grad():
                return LP.lpips_vgg(x32, y32, wdev)
        for _ in range(3):
            val = stmt()
        torch.cuda.synchronize()
        note = f"its value {float(val[1]):.8f}"
    except Exception as exc:                                                   # (MIOpen absent or refusing the shape: said, not hidden)
        note, stmt = f"F.conv2d does not run on this device here: {type(exc).__name__}: {str(exc).splitlines()[0][:200]}", None
    for _ in range(3):
        whole()
    torch.cuda.synchronize()
    t_all, t_torch = [], ([] if stmt is not None else None)
    for _ in range(a.reps):                                                    # alternating: a drift of the clocks meets both routes
        t_all += _time(whole, 1, a.calls)
        if stmt is not None:
            t_torch += _time(stmt, 1, a.calls)
    row = rows.cpu().numpy()[0]
    if stmt is not None:
        note += f" against the kernels' {row[5]:.8f}"

    # ---- (b) the layers -------------------------------------------------------------------------------------------------------------
    L = lib.load()
    stream = fused._stream(torch.device(DEV))
    layers, k = [], 0
    for block, n in enumerate(LP.BLOCKS):
        for _ in range(n):
            layers.append((k, block, H >> block, W >> block) + LP.CONV_CHANNELS[k])
            k += 1
    t_layer, flop, stored = [], [], []
    for k, block, h, w, cin, cout in layers:
        x = torch.randn(2, h, w, max(cin, 4), device=DEV)
        out = torch.empty(2, h, w, cout, device=DEV)

        def fn():
            lib.check(L.egs_conv3x3_relu_nhwc(2, h, w, max(cin, 4), cout, x.data_ptr(), net._w[k].data_ptr(), net._b[k].data_ptr(), out.data_ptr(), stream))
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t_layer.append(_time(fn, a.reps, a.layer_calls))
        flop.append(2 * 2.0 * 9 * cin * cout * h * w)                         # both images; the first layer's three real input channels
        stored.append(out.numel() * 4)
        del x, out
    total_flop = sum(flop)

    # ---- the record -----------------------------------------------------------------------------------------------------------------
    props = torch.cuda.get_device_properties(0)
    med, lo, hi, sp = _stats(t_all)
    conv_ms = sum(_stats(t)[0] for t in t_layer)
    lines = ["# LPIPS pass: VGG-16 features by fp32 MFMA kernels", "",
             f"`python tools/time_lpips_pass.py` -- one process, every route warmed up; {a.reps} repetitions; a figure is the time between two device events around "
             f"{a.calls} (pass) / {a.layer_calls} (layer) back-to-back launches from Python, divided by the count: launch gaps included, not kernel-trace durations.  "
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  Library source hash {lib.built_source_hash()}.", "",
             f"## (a) The pass on one {W} x {H} pair (hand mask given); the two routes alternate within each repetition", "",
             "| route | ms per frame (median) | min | max | spread |", "|---|---|---|---|---|",
             f"| egs_lpips_forward (20 launches) | {med:.2f} | {lo:.2f} | {hi:.2f} | {sp:.1f} % |"]
    if t_torch is not None:
        m2, l2, h2, s2 = _stats(t_torch)
        lines.append(f"| lpips.lpips_vgg, float32 torch on the device | {m2:.2f} | {l2:.2f} | {h2:.2f} | {s2:.1f} % |")
    lines += ["", f"The torch statement on the device: {note}.", "",
              f"Convolution FLOP of the pair: {total_flop / 1e9:.1f} GFLOP ({total_flop / 4e9:.1f} GMAC per image).  Over the pass: "
              f"{total_flop / (med * 1e-3) / 1e12:.1f} TFLOP/s = {100 * total_flop / (med * 1e-3) / MATRIX_PEAK:.1f} % of the {MATRIX_PEAK / 1e12:.1f} TFLOP/s fp32 matrix peak "
              f"(floor at the peak: {1e3 * total_flop / MATRIX_PEAK:.2f} ms).  Workspace {net.workspace(H, W).numel() / 1e9:.2f} GB.", "",
              "## (b) The layers by themselves (batch of 2)", "",
              "| layer | map | Cin -> Cout | GFLOP | ms (median) | spread | TFLOP/s | of peak | stores, TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for (k, block, h, w, cin, cout), t, f, sb in zip(layers, t_layer, flop, stored):
        m, _, _, s = _stats(t)
        lines.append(f"| conv{block + 1}_{k - sum(LP.BLOCKS[:block]) + 1} | {w} x {h} | {cin} -> {cout} | {f / 1e9:.1f} | {m:.3f} | {s:.1f} % | "
                     f"{f / (m * 1e-3) / 1e12:.1f} | {100 * f / (m * 1e-3) / MATRIX_PEAK:.1f} % | {sb / (m * 1e-3) / 1e12:.2f} |")
    lines += ["", f"Sum of the 13 convolutions: {conv_ms:.2f} ms; the input kernel, the five tap kernels (norms, weighted difference, pooled map) and the finishing "
              f"wave are the remaining {med - conv_ms:.2f} ms of (a).", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
