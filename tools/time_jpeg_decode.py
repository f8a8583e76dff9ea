#!/usr/bin/env python
"""Record of the JPEG reader at the dataset's shape: a 1920 x 1080 RGB frame (a render of the committed trained scene, 8-bit) as a 4:2:0
file and a 1920 x 1080 binary mask (the render's channel mean thresholded at its median) as a mode-L file, each as Pillow writes it at its
default quality without restart markers and with a restart marker per MCU row.  Everything in ONE process:

  (a) the decode on the device, egs_jpeg_decode on a batch that is already uploaded: device events around back-to-back calls, the four
      launches together and each alone (egs_jpeg_decode_phases), for batches of 1, 32 and 256 copies of the file.
  (b) JpegReader.read in all (segment walk, upload, launches, the read of the status words), wall.
  (c) the host reader, same files, same run: Pillow's Image.open(BytesIO(b)).load() on one thread (how the reference's loop runs it) and on
      a pool of 16 threads.

The files come from Pillow; --cache DIR keeps them (and reads them back where Pillow is not installed: section (c) is then skipped).  The
legs alternate inside every repeat and every figure is median (min .. max) over --regions repeats of the same call: the spread of A
against A.

    python tools/time_jpeg_decode.py --out profiles/jpeg_decode.md
"""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
PHASES = (("all", 15), ("intervals", 1), ("entropy", 2), ("idct", 4), ("colour", 8))


def _stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def _fmt(v, digits=3):
    m, lo, hi = _stats(v)
    return f"{m:.{digits}f} ({lo:.{digits}f} .. {hi:.{digits}f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--cache", default=None, help="directory that keeps the four files between runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg_decode.py measures on a HIP device; none is available")
    from egogaussian_amd import _hip, jpeg, lib
    from egogaussian_amd.losses import quantize8
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_camera, SynthGaussians, Pipe
    L = lib.load()
    H, W = a.height, a.width
    try:
        import PIL
        from PIL import Image
    except ImportError:
        Image = None
    kinds = {"RGB 4:2:0": ("rgb", {}), "RGB 4:2:0, restart per MCU row": ("rgb", {"restart_marker_rows": 1}),
             "mask L": ("mask", {}), "mask L, restart per MCU row": ("mask", {"restart_marker_rows": 1})}
    files, images = {}, None
    for k, (name, (which, kw)) in enumerate(kinds.items()):
        path = os.path.join(a.cache, f"{which}_{W}x{H}_{'rr1' if kw else 'rr0'}.jpg") if a.cache else None
        if path and os.path.exists(path):
            with open(path, "rb") as fh:
                files[name] = fh.read()
            continue
        if Image is None:
            raise SystemExit("time_jpeg_decode.py writes its files with Pillow, which is not installed here, and --cache does not hold them")
        if images is None:
            z = np.load(os.path.join(ROOT, "bench_data", "trained_scene.npz"))
            pc = SynthGaussians({k: z[k] for k in ("xyz", "log_scale", "quat", "opacity_logit", "features")}, device=DEV, requires_grad=False)
            with torch.no_grad():
                frame = quantize8(render(make_camera(7, H, W, device=DEV), pc, Pipe, torch.zeros(3, device=DEV))["render"]).to(torch.uint8)
            mean = frame.float().mean(0)
            images = {"rgb": np.ascontiguousarray(frame.permute(1, 2, 0).cpu().numpy()), "mask": ((mean > mean.median()) * 255).to(torch.uint8).cpu().numpy()}
        b = io.BytesIO()
        Image.fromarray(images[which]).save(b, format="JPEG", **(dict(subsampling=2) if which == "rgb" else {}), **kw)
        files[name] = b.getvalue()
        if path:
            os.makedirs(a.cache, exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(files[name])
    batches = [int(b) for b in a.batches.split(",")]

    # ---- (a), (b): the decode --------------------------------------------------------------------------------------------------------------
    rec, readers, shapes = {}, {}, {}
    for name, data in files.items():
        want = None
        if Image is not None:
            arr = np.asarray(Image.open(io.BytesIO(data)))
            want = torch.from_numpy(np.ascontiguousarray(arr.reshape(arr.shape[0], arr.shape[1], -1))).to(DEV)
        for F in batches:
            rd = jpeg.JpegReader(DEV, batch=F)
            outs = rd.read([data] * F)                               # warm-up, and the check
            assert torch.equal(outs[0], outs[-1]) and (want is None or torch.equal(outs[0], want)), name
            shapes[name] = tuple(outs[0].shape)
            readers[name, F] = rd
            print(f"warmed: {name}, batch {F}", file=sys.stderr, flush=True)
            rec[name, F] = {k: [] for k in [p[0] for p in PHASES] + ["read"]}
    for region in range(a.regions):
        print(f"decode: repeat {region + 1} of {a.regions}", file=sys.stderr, flush=True)
        for (name, F), rd in readers.items():                        # the legs alternate inside a repeat
            calls = max(1, 4 // F)
            for key, phases in PHASES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    lib.check(L.egs_jpeg_decode_phases(*rd.last_call, _hip.stream_of(torch.device(DEV)), phases))
                e1.record()
                torch.cuda.synchronize()
                rec[name, F][key].append(e0.elapsed_time(e1) / calls)
            t0 = time.perf_counter()
            rd.read([files[name]] * F)
            torch.cuda.synchronize()
            rec[name, F]["read"].append(1e3 * (time.perf_counter() - t0))

    # ---- (c): the host reader ----------------------------------------------------------------------------------------------------------------
    host = {}
    for name, data in files.items() if Image is not None else []:
        one, pool16 = [], []
        for _ in range(a.regions):
            t0 = time.perf_counter()
            for _ in range(4):
                Image.open(io.BytesIO(data)).load()
            one.append(1e3 * (time.perf_counter() - t0) / 4)
            with ThreadPoolExecutor(max_workers=16) as pool:
                t0 = time.perf_counter()
                list(pool.map(lambda b: Image.open(io.BytesIO(b)).load(), [data] * 32))
                pool16.append(1e3 * (time.perf_counter() - t0) / 32)
        host[name] = (one, pool16)

    props = torch.cuda.get_device_properties(0)
    lines = ["# Baseline JPEG files read on the device", "",
             f"`python tools/time_jpeg_decode.py` -- one process; {W} x {H}.  RGB frame: an 8-bit render of the committed trained scene "
             f"(bench_data/trained_scene.npz) as a 4:2:0 file; mask: its channel mean thresholded at its median, as a mode-L file; Pillow's default "
             f"quality, without restart markers and with one per MCU row.  Device: {props.name} ({props.multi_processor_count} CUs), torch "
             f"{torch.__version__}" + (f", Pillow {PIL.__version__}" if Image is not None else "; Pillow is NOT installed here: its legs are skipped")
             + f".  Library source hash {lib.built_source_hash()}.  A batch is that many copies of one file.  Every figure is the median "
             f"(min .. max) of {a.regions} repeats, the legs alternating inside each repeat: the spread of A against A.  Times in ms.",
             "", "## (a), (b) The decode, per batch", "",
             "| file | file bytes / raw bytes | restart intervals | batch | four launches | intervals | entropy | idct | colour | files/s | decoded MB/s | "
             "JpegReader.read, wall |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for (name, F), r in rec.items():
        data = files[name]
        raw = int(np.prod(shapes[name]))
        n_int = jpeg.geometry(jpeg.parse(data))[3]
        m = _stats(r["all"])[0]
        lines.append(f"| {name} | {len(data)} / {raw} ({100.0 * len(data) / raw:.1f} %) | {n_int} | {F} | " + " | ".join(_fmt(r[k]) for k, _ in PHASES)
                     + f" | {1e3 * F / m:.0f} | {F * raw / m / 1e3:.0f} | {_fmt(r['read'])} |")
    lines += ["", "## (c) The host reader, per file", ""]
    if host:
        lines += ["| file | Pillow open + load, one thread | Pillow, 16 threads over 32 files, per file | device, four launches, per file at the largest batch |",
                  "|---|---|---|---|"]
        for name, (one, pool16) in host.items():
            lines.append(f"| {name} | {_fmt(one)} | {_fmt(pool16)} | {_stats(rec[name, batches[-1]]['all'])[0] / batches[-1]:.3f} |")
    else:
        lines.append("Pillow is not installed here.")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
