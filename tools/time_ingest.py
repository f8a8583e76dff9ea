#!/usr/bin/env python
"""Record of frame ingest at the workload's shape: one frame of 1080 x 1920 sources (RGB image, L hand mask, L object mask) into a
1600 x 900 store with gate and object mask, everything in ONE process:

  (a) the host path it replaces: PIL.Image.resize x 3, / 255 and binarise as the reference's loadCam does, FrameStore.put.  Needs Pillow on
      the machine that runs this tool; skipped with a note when it is absent.
  (b) FrameIngest.put from pinned host arrays, upload included: wall time per frame over --frames frames closed by one device synchronise.
  (c) the three launches alone (object mask, hand mask, image; each mask launch with its memset node), sources resident on the device:
      device events around back-to-back calls.
  (d) the upload of their input alone: device events around back-to-back non_blocking copies of the three pinned arrays.
  bytes: from the shapes.  File decoding stays on the host and is in NO figure here.

--bench-parent / --bench-this: files holding the JSON result lines of `python bench.py --full ...` on the parent commit and on this one, run
alternately; quoted in the record next to the spread that tool reports for its own five regions.

    python tools/time_ingest.py --out profiles/ingest.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def _stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def _bench_line(path):
    if not path or not os.path.exists(path):
        return None
    for line in reversed(open(path).read().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            try:
                return json.loads(line)
            except ValueError:
                continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src-height", type=int, default=1080)
    ap.add_argument("--src-width", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=40, help="frames per timed region of (b)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=5, help="frames of the host path (a)")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files holding the result line of bench.py --full on the parent commit")
    ap.add_argument("--bench-this", nargs="*", default=[], help="the same on this commit, run alternately with the parent's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egogaussian_amd import ingest, lib
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.scene_synth import make_camera
    if not torch.cuda.is_available():
        raise SystemExit("time_ingest.py measures on a HIP device; none is available")
    h, w = a.src_height, a.src_width
    W, H = ingest.target_size(w, h)
    F = 4
    g = torch.Generator().manual_seed(3)
    blocks = lambda p: (torch.rand((h // 8 + 1, w // 8 + 1, 1), generator=g) < p).repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w]
    image = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).pin_memory()
    hand = (blocks(0.3) * torch.randint(1, 256, (h, w, 1), generator=g, dtype=torch.uint8)).contiguous().pin_memory()
    obj = (blocks(0.3) * torch.randint(1, 256, (h, w, 1), generator=g, dtype=torch.uint8)).contiguous().pin_memory()
    cam = make_camera(0, H, W)
    lay = dict(gated=True, object_loss=True)
    store = FrameStore(H, W, F, DEV, **lay)
    ing = ingest.FrameIngest(store, (h, w))

    # ---- (b) FrameIngest.put from pinned host arrays ----------------------------------------------------------------------------------------
    for i in range(F):
        ing.put(i, cam, image=image, hand_mask=hand, obj_mask=obj)
    torch.cuda.synchronize()
    put_ms = []
    for _ in range(max(5, a.regions)):
        t0 = time.perf_counter()
        for n in range(a.frames):
            ing.put(n % F, cam, image=image, hand_mask=hand, obj_mask=obj)
        torch.cuda.synchronize()
        put_ms.append(1e3 * (time.perf_counter() - t0) / a.frames)

    # ---- (c), (d) by device events --------------------------------------------------------------------------------------------------------------
    d_image, d_hand, d_obj = image.to(DEV), hand.to(DEV), obj.to(DEV)
    stage = [torch.empty_like(d_image), torch.empty_like(d_hand), torch.empty_like(d_obj)]

    def launches():
        ing.plane(1, "obj_mask", d_obj)
        ing.plane(1, "hand_mask", d_hand)
        ing.plane(1, "image", d_image)

    def uploads():
        for dst, src in zip(stage, (image, hand, obj)):
            dst.copy_(src, non_blocking=True)
    calls = {"three launches, sources on the device": launches, "upload of the three pinned sources": uploads}
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    n_calls = 50
    for _ in range(5):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / n_calls)                # us per call
    per_plane = {}
    for which, src in (("obj_mask", d_obj), ("hand_mask", d_hand), ("image", d_image)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_calls):
            ing.plane(1, which, src)
        e1.record()
        torch.cuda.synchronize()
        per_plane[which] = 1e3 * e0.elapsed_time(e1) / n_calls

    # ---- the result of (b) is the statement's ----------------------------------------------------------------------------------------------------
    bits_obj = ingest.binarize(ingest.resize_u8(d_obj, (W, H)))
    want = (ingest.resize_u8(d_image, (W, H)) * bits_obj.unsqueeze(-1).to(torch.uint8)).permute(2, 0, 1).reshape(-1)
    same = all(torch.equal(store.img[i, :store.n_img], want) for i in range(F))

    # ---- (a) the host path ---------------------------------------------------------------------------------------------------------------------------
    host = None
    try:
        import PIL
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        pil = [Image.fromarray(image.numpy()), Image.fromarray(hand.numpy()[:, :, 0]), Image.fromarray(obj.numpy()[:, :, 0])]
        ref = FrameStore(H, W, F, DEV, **lay)
        parts = {"resize x 3": [], "/ 255, binarise": [], "FrameStore.put": []}
        total = []
        for n in range(a.host_frames + 1):
            t0 = time.perf_counter()
            resized = [torch.from_numpy(np.array(p.resize((W, H)))).float() for p in pil]
            t1 = time.perf_counter()
            gt = (resized[0] / 255.0).clamp(0.0, 1.0).permute(2, 0, 1)
            hm, om = (torch.where(m / 255.0 > 0, 1.0, 0.0) for m in resized[1:])
            t2 = time.perf_counter()
            ref.put(n % F, cam, gt=gt, gate=1.0 - hm, obj_mask=om)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if n:                                                                  # (the first frame warms the allocator)
                for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
                    parts[k].append(1e3 * v)
                total.append(1e3 * (t3 - t0))
        host = dict(parts={k: _stats(v) for k, v in parts.items()}, total=_stats(total),
                    same=torch.equal(ref.img[1], store.img[1]) and torch.equal(ref.bits[1], store.bits[1]), pillow=PIL.__version__)

    # ---- the record ----------------------------------------------------------------------------------------------------------------------------------
    props = torch.cuda.get_device_properties(0)
    in_bytes = h * w * 3 + 2 * h * w
    out_bytes = 3 * H * W + 2 * ((H * W + 31) // 32) * 4
    b_med, b_lo, b_hi = _stats(put_ms)
    c_med, c_lo, c_hi = _stats(times["three launches, sources on the device"])
    d_med, d_lo, d_hi = _stats(times["upload of the three pinned sources"])
    lines = ["# Frame ingest: the load in front of the frame store", "",
             f"`python tools/time_ingest.py` -- one process; sources {w} x {h} (RGB image, L hand mask, L object mask) -> a {W} x {H} store with gate and "
             f"object mask (object_loss: the image bytes times the object plane).  Device: {props.name} ({props.multi_processor_count} CUs), torch "
             f"{torch.__version__}.  Library source hash {lib.built_source_hash()}.  File decoding stays on the host and is in no figure below: every "
             f"path starts from decoded 8-bit arrays in host memory.", "",
             f"Bytes per frame, from the shapes: {in_bytes} in ({in_bytes / 1e6:.2f} MB), {out_bytes} out ({out_bytes / 1e6:.2f} MB).", "",
             "## Per frame", "",
             "| path | ms (median) | min | max |", "|---|---|---|---|"]
    if host:
        for k, (med, lo, hi) in host["parts"].items():
            lines.append(f"| (a) host: {k} | {med:.2f} | {lo:.2f} | {hi:.2f} |")
        lines.append(f"| (a) host path in all (Pillow {host['pillow']}, one thread, {a.host_frames} frames) | {host['total'][0]:.2f} | {host['total'][1]:.2f} | {host['total'][2]:.2f} |")
    else:
        lines.append("| (a) host path | not measured: Pillow is not installed on this machine | | |")
    lines += [f"| (b) FrameIngest.put from pinned host arrays, upload included ({a.frames} frames per region, {len(put_ms)} regions) | {b_med:.3f} | {b_lo:.3f} | {b_hi:.3f} |",
              f"| (c) the three launches alone, sources on the device (device events, {n_calls} back-to-back) | {c_med / 1e3:.3f} | {c_lo / 1e3:.3f} | {c_hi / 1e3:.3f} |",
              f"| (d) the upload of their input alone (device events, {n_calls} back-to-back) | {d_med / 1e3:.3f} | {d_lo / 1e3:.3f} | {d_hi / 1e3:.3f} |", "",
              f"(c) by launch, us: object mask {per_plane['obj_mask']:.1f}, hand mask {per_plane['hand_mask']:.1f}, image {per_plane['image']:.1f} "
              f"(a mask launch includes the memset node that clears its plane).  (c) moves {(in_bytes + out_bytes) / 1e6:.2f} MB in {c_med:.0f} us = "
              f"{(in_bytes + out_bytes) / (c_med * 1e-6) / 1e9:.0f} GB/s; (d) moves {in_bytes / 1e6:.2f} MB in {d_med:.0f} us = {in_bytes / (d_med * 1e-6) / 1e9:.1f} GB/s.",
              ("The kernels take LONGER than the copy of their own input: " if c_med > d_med else "The kernels take less time than the copy of their own input: ")
              + f"{c_med:.0f} us against {d_med:.0f} us ({c_med / d_med:.2f}x).", ""]
    if host:
        lines += [f"(a) against (b): {host['total'][0] / b_med:.1f}x.  The store rows FrameIngest.put wrote are "
                  f"{'bit-identical to' if host['same'] else 'DIFFERENT from'} the rows the host path wrote (img and bits of one frame).", ""]
    lines += [f"The image rows of all {F} frames against the torch statement on the device: {'bit-identical' if same else 'DIFFERENT'}.", "",
              "## bench.py against the parent commit", ""]
    bp, bt = [_bench_line(f) for f in a.bench_parent], [_bench_line(f) for f in a.bench_this]
    if bp and bt and all(bp) and all(bt):
        sp = lambda d: (f"{d['value']} (median of its five regions {d.get('value_median')}, the regions from "
                        f"{d.get('value_spread', [None, None])[0]} to {d.get('value_spread', [None, None])[1]})")
        lines += ["The library gains a unit and no existing kernel changes.  The headline (it/s) of `bench.py --full` on both trees, on this machine, "
                  "run alternately (parent, this, parent, this, ...); the spread is the one the tool reports for its own five regions (A/A):", ""]
        for k, (x, y) in enumerate(zip(bp, bt)):
            lines += [f"- run {k + 1}, parent: {sp(x)}", f"- run {k + 1}, this commit: {sp(y)}"]
        lines.append("")
    else:
        lines += ["Not measured in this record.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
