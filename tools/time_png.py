#!/usr/bin/env python
"""Record of the PNG writer at the workload's shape: 960 x 540 RGB frames (a render of the committed trained scene, 8-bit) and 960 x 540 masks
(the render's channel mean thresholded at its median: the blob shape a predicted mask has), everything in ONE process:

  (a) the kernel: png.encode of a batch into preallocated buffers, device events around back-to-back calls, per frame.
  (b) the device-to-host copy: the batch's sizes read once, then the used prefix of every slot into pinned memory; wall time closed by a
      synchronise, per frame.
  (c) the file write of those bytes from the pool (a temporary directory), per frame.
  (d) PngWriter.save in all, per frame.
  (e) the host path it replaces: PIL.Image.fromarray(...).save(...) at Pillow's default level and at level 1, one thread, the same bytes
      already on the host.  Skipped with a note when Pillow is absent.
  sizes: kernel / encode_statement (zlib level 6 restricted to the kernel's segments) / Pillow.

Every figure is median (min .. max) over --regions repeats of the same call: the spread of A against A.

    python tools/time_png.py --out profiles/png_encode.md
"""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def _fmt(v, unit="ms"):
    m, lo, hi = _stats(v)
    return f"{m:.3f} ({lo:.3f} .. {hi:.3f}) {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back encodes per timed region of (a)")
    ap.add_argument("--host-frames", type=int, default=3, help="frames per region of the Pillow path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_png.py measures on a HIP device; none is available")
    from egogaussian_amd import lib, png
    from egogaussian_amd.losses import quantize8
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_camera, SynthGaussians, Pipe
    H, W, F = a.height, a.width, a.batch
    z = np.load(os.path.join(ROOT, "bench_data", "trained_scene.npz"))
    pc = SynthGaussians({k: z[k] for k in ("xyz", "log_scale", "quat", "opacity_logit", "features")}, device=DEV, requires_grad=False)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        frames = torch.stack([quantize8(render(make_camera(7 * k, H, W, device=DEV), pc, Pipe, bg)["render"]) for k in range(F)]).to(DEV)
    mean = frames.float().mean(1)
    masks = ((mean > mean.flatten(1).median(1).values.view(F, 1, 1)) * 255).to(torch.uint8)
    sets = {"RGB frame": (frames, 3), "mask": (masks, 1)}
    try:
        import PIL
        from PIL import Image
    except ImportError:
        Image = None

    rec, sizes_rec = {}, {}
    for name, (imgs, C) in sets.items():
        wr = png.PngWriter(H, W, C, DEV, batch=F)
        enc = lambda: png.encode(imgs, out=wr.buf, sizes=wr.sizes, scratch=wr.scratch)
        for _ in range(3):
            enc()
        torch.cuda.synchronize()
        kern, copy, write, save = [], [], [], []
        for _ in range(a.regions):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                enc()
            e1.record()
            torch.cuda.synchronize()
            kern.append(e0.elapsed_time(e1) / (a.calls * F))
            t0 = time.perf_counter()
            sz = wr.sizes[:F].cpu().tolist()
            for i in range(F):
                wr.staging[i, :sz[i]].copy_(wr.buf[i, :sz[i]], non_blocking=True)
            torch.cuda.synchronize()
            copy.append(1e3 * (time.perf_counter() - t0) / F)
            with tempfile.TemporaryDirectory() as d:
                paths = [os.path.join(d, f"{i}.png") for i in range(F)]
                host = wr.staging.numpy()
                from concurrent.futures import ThreadPoolExecutor
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=wr.threads) as pool:
                    list(pool.map(png._write, paths, [memoryview(host[i])[:sz[i]] for i in range(F)]))
                write.append(1e3 * (time.perf_counter() - t0) / F)
                t0 = time.perf_counter()
                wr.save(imgs, paths)
                save.append(1e3 * (time.perf_counter() - t0) / F)
        files = [wr.staging[i, :sz[i]].numpy().tobytes() for i in range(F)]
        x = imgs.cpu().numpy()
        ok = all(np.array_equal(png.decode(files[i]), x[i]) for i in range(min(F, 2)))
        st = [len(png.encode_statement(x[i] if C == 3 else x[i][None])) for i in range(min(F, 4))]
        pil = {}
        if Image is not None:
            hwc = [np.ascontiguousarray(x[i].transpose(1, 2, 0)) if C == 3 else x[i] for i in range(F)]
            for label, kw in (("default level", {}), ("level 1", {"compress_level": 1})):
                ms, nbytes = [], []
                for _ in range(a.regions):
                    t0 = time.perf_counter()
                    for i in range(a.host_frames):
                        b = io.BytesIO()
                        Image.fromarray(hwc[i]).save(b, format="PNG", **kw)
                        nbytes.append(b.tell())
                    ms.append(1e3 * (time.perf_counter() - t0) / a.host_frames)
                pil[label] = (ms, nbytes[:a.host_frames])
        rec[name] = dict(kern=kern, copy=copy, write=write, save=save, ok=ok, pil=pil)
        sizes_rec[name] = dict(kernel=sz[:4], statement=st, filtered=H * (W * C + 1), pil={k: v[1] for k, v in pil.items()})

    props = torch.cuda.get_device_properties(0)
    lines = ["# PNG files from device tensors", "",
             f"`python tools/time_png.py` -- one process; {W} x {H}, batches of {F}.  RGB frames: 8-bit renders of the committed trained scene "
             f"(bench_data/trained_scene.npz) from {F} cameras; masks: the render's channel mean thresholded at its median.  Device: {props.name} "
             f"({props.multi_processor_count} CUs), torch {torch.__version__}.  Library source hash {lib.built_source_hash()}.  Every figure is the median "
             f"(min .. max) of {a.regions} repeats of the same call: the spread of A against A.", ""]
    for name, r in rec.items():
        lines += [f"## Per {name}", "", "| step | per frame |", "|---|---|",
                  f"| (a) kernel: three launches per batch, device events, {a.calls} back-to-back encodes | {_fmt(r['kern'])} |",
                  f"| (b) sizes read once + used prefixes into pinned memory, wall | {_fmt(r['copy'])} |",
                  f"| (c) file write from the pool (temporary directory) | {_fmt(r['write'])} |",
                  f"| (d) PngWriter.save in all, wall | {_fmt(r['save'])} |"]
        if r["pil"]:
            for label, (ms, _) in r["pil"].items():
                lines.append(f"| (e) Pillow {PIL.__version__} fromarray + save to memory, {label}, one thread | {_fmt(ms)} |")
            k = _stats(r["save"])[0]
            for label, (ms, _) in r["pil"].items():
                m = _stats(ms)[0]
                lines.append(f"| (e) / (d), {label} | {m / k:.1f}x {'(the writer is NOT faster)' if m <= k else ''} |")
        else:
            lines.append("| (e) Pillow | not measured: Pillow is not installed on this machine |")
        s = sizes_rec[name]
        lines += ["", f"The files decode to the input: {'yes' if r['ok'] else 'NO'}.  Bytes of the first frames (filtered data: {s['filtered']}): kernel "
                  f"{s['kernel']}, statement {s['statement']}" + "".join(f", Pillow {k} {v}" for k, v in s["pil"].items()) + ".", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
