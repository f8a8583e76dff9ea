#!/usr/bin/env python
"""Record of the PNG reader at the dataset's shape: a 1920 x 1080 RGB frame (a render of the committed trained scene, 8-bit) and a
1920 x 1080 binary mask (the render's channel mean thresholded at its median), each as the device encoder writes it (png.encode) and -- where
Pillow is importable -- as Pillow writes it at its default level.  Everything in ONE process:

  (a) the decode on the device, egs_png_decode on a batch that is already uploaded: device events around back-to-back calls, the three
      launches together and each alone (egs_png_decode_phases), for batches of 1, 32 and 256 copies of the file.
  (b) PngReader.read in all (chunk walk, upload, launches, the read of the status words), wall.
  (c) FrameIngest.put_files (image + hand mask + object mask, 1080p -> 1600 x 900) against FrameIngest.put of the same three arrays
      already decoded on the host, wall per frame, closed by a synchronise.
  (d) the host readers, same files, same run: Pillow's Image.open(BytesIO(b)).load() on one thread (how the reference's loop runs it)
      and on a pool of 16 threads; zlib.decompress of the stream alone (a lower bound of any host reader; the only yardstick without Pillow).

  (e) egs_png_decode_ex with EGS_PNG_SEGMENTS against the calls above, same process, same files, same uploaded batch: the inflate launches
      (measure, scan, place, and the serial inflate of what fell back) against the serial inflate launch; all launches and PngReader.read
      with the flag against without; FrameIngest.put_files per frame likewise.  --sections e --append adds this section alone to a record
      that holds the others.

The legs alternate inside every repeat (device-encoded file, Pillow's file, ...) and every figure is median (min .. max) over --regions
repeats of the same call: the spread of A against A.

    python tools/time_png_decode.py --out profiles/png_decode.md
"""
import argparse
import io
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="abcde", help="which sections to measure: a (with b), c, d, e")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_png_decode.py measures on a HIP device; none is available")
    from egogaussian_amd import _hip, ingest, lib, png
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.losses import quantize8
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_camera, SynthGaussians, Pipe
    L = lib.load()
    H, W = a.height, a.width
    z = np.load(os.path.join(ROOT, "bench_data", "trained_scene.npz"))
    pc = SynthGaussians({k: z[k] for k in ("xyz", "log_scale", "quat", "opacity_logit", "features")}, device=DEV, requires_grad=False)
    with torch.no_grad():
        frame = quantize8(render(make_camera(7, H, W, device=DEV), pc, Pipe, torch.zeros(3, device=DEV))["render"]).to(torch.uint8)
    mean = frame.float().mean(0)
    mask = ((mean > mean.median()) * 255).to(torch.uint8)[None]
    try:
        import PIL
        from PIL import Image
    except ImportError:
        Image = None

    def device_file(x):
        buf, sizes = png.encode(x[None])
        return buf[0, :int(sizes[0])].cpu().numpy().tobytes()

    def pillow_file(x):
        b = io.BytesIO()
        arr = x.cpu().numpy()
        Image.fromarray(arr[0] if arr.shape[0] == 1 else np.ascontiguousarray(arr.transpose(1, 2, 0))).save(b, format="PNG")
        return b.getvalue()

    files = {"RGB frame, device encoder": (device_file(frame), frame), "mask, device encoder": (device_file(mask), mask)}
    if Image is not None:
        files["RGB frame, Pillow"] = (pillow_file(frame), frame)
        files["mask, Pillow"] = (pillow_file(mask), mask)
    batches = [int(b) for b in a.batches.split(",")]

    # ---- (a), (b): the decode --------------------------------------------------------------------------------------------------------------
    rec = {}
    readers = {}
    for name, (data, x) in files.items():
        want = x.permute(1, 2, 0).contiguous()
        for F in batches if "a" in a.sections else []:
            rd = png.PngReader(DEV, batch=F)
            outs = rd.read([data] * F)                               # warm-up, and the check
            assert all(torch.equal(o, want) for o in (outs[0], outs[-1])), name
            readers[name, F] = rd
            print(f"warmed: {name}, batch {F}", file=sys.stderr, flush=True)
            rec[name, F] = {k: [] for k in ("all", "gather", "inflate", "unfilter", "read")}
    for region in range(a.regions if "a" in a.sections else 0):
        print(f"decode: repeat {region + 1} of {a.regions}", file=sys.stderr, flush=True)
        for (name, F), rd in readers.items():                        # the legs alternate inside a repeat
            calls = max(1, 8 // F)
            for key, phases in (("all", 7), ("gather", 1), ("inflate", 2), ("unfilter", 4)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    lib.check(L.egs_png_decode_phases(*rd.last_call, _hip.stream_of(torch.device(DEV)), phases))
                e1.record()
                torch.cuda.synchronize()
                rec[name, F][key].append(e0.elapsed_time(e1) / calls)
            t0 = time.perf_counter()
            rd.read([files[name][0]] * F)
            torch.cuda.synchronize()
            rec[name, F]["read"].append(1e3 * (time.perf_counter() - t0))

    # ---- (d): the host readers ---------------------------------------------------------------------------------------------------------------
    host = {}
    for name, (data, x) in files.items() if "d" in a.sections else []:
        chunks = png.parse(data)[3]
        zs = b"".join(data[o:o + n] for o, n in chunks)
        one, pool16, zl = [], [], []
        for _ in range(a.regions):
            t0 = time.perf_counter()
            zlib.decompress(zs)
            zl.append(1e3 * (time.perf_counter() - t0))
            if Image is not None:
                t0 = time.perf_counter()
                for _ in range(4):
                    Image.open(io.BytesIO(data)).load()
                one.append(1e3 * (time.perf_counter() - t0) / 4)
                with ThreadPoolExecutor(max_workers=16) as pool:
                    t0 = time.perf_counter()
                    list(pool.map(lambda b: Image.open(io.BytesIO(b)).load(), [data] * 32))
                    pool16.append(1e3 * (time.perf_counter() - t0) / 32)
        host[name] = dict(one=one, pool16=pool16, zlib=zl, stream=len(zs))

    # ---- (c): put_files against put -----------------------------------------------------------------------------------------------------------
    SH, SW = 900, 1600
    store = FrameStore(SH, SW, 2, DEV, gated=True, object_loss=True, dynamic=True, motion=True)
    ing = ingest.FrameIngest(store, (H, W))
    cam = make_camera(0, SH, SW)
    kw = dict(accum_R=torch.eye(3), accum_T=torch.eye(4))
    arrays = dict(image=frame.permute(1, 2, 0).contiguous().cpu().numpy(), hand_mask=mask[0].cpu().numpy(), obj_mask=mask[0].cpu().numpy())
    put_rec = {}
    for label in ("device encoder", "Pillow") if "c" in a.sections else []:
        if label == "Pillow" and Image is None:
            continue
        f_img, f_mask = files[f"RGB frame, {label}"][0], files[f"mask, {label}"][0]
        for _ in range(2):
            ing.put(0, cam, **arrays, **kw)
            ing.put_files(1, cam, image=f_img, hand_mask=f_mask, obj_mask=f_mask, **kw)
        torch.cuda.synchronize()
        assert torch.equal(store.img[0], store.img[1]) and torch.equal(store.bits[0], store.bits[1])
        p, pf = [], []
        for _ in range(a.regions):
            t0 = time.perf_counter()
            ing.put(0, cam, **arrays, **kw)
            torch.cuda.synchronize()
            p.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            ing.put_files(1, cam, image=f_img, hand_mask=f_mask, obj_mask=f_mask, **kw)
            torch.cuda.synchronize()
            pf.append(1e3 * (time.perf_counter() - t0))
        put_rec[label] = (p, pf, len(f_img) + 2 * len(f_mask))

    # ---- (e): the segmented route against the serial wave ------------------------------------------------------------------------------------
    flag_rec, flag_readers, flag_put = {}, {}, {}
    for name, (data, x) in files.items() if "e" in a.sections else []:
        want = x.permute(1, 2, 0).contiguous()
        for F in batches:
            plain, both = png.PngReader(DEV, batch=F), png.PngReader(DEV, batch=F, segments=True)
            for rd in (plain, both):
                outs = rd.read([data] * F)                           # warm-up, and the check
                assert all(torch.equal(o, want) for o in (outs[0], outs[-1])), name
            flag_readers[name, F] = (plain, both, both.last_route[0])
            flag_rec[name, F] = {k: [] for k in ("inflate0", "inflate1", "all0", "all1", "read0", "read1")}
            print(f"warmed: {name}, batch {F}, route {png.route_text(both.last_route[0])}", file=sys.stderr, flush=True)
    for region in range(a.regions if "e" in a.sections else 0):
        print(f"flags: repeat {region + 1} of {a.regions}", file=sys.stderr, flush=True)
        for (name, F), (plain, both, _) in flag_readers.items():     # the legs alternate inside a repeat; every call is on `both`'s batch
            st = _hip.stream_of(torch.device(DEV))
            for key, phases, flags in (("inflate0", 2, 0), ("inflate1", 2, png.SEGMENTS), ("all0", 7, 0), ("all1", 7, png.SEGMENTS)):
                calls = max(1, (2 if (phases & 2) and not flags else 8) // F)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    lib.check(L.egs_png_decode_ex(*both.last_call, st, phases, flags, both.last_route_ptr if flags & png.SEGMENTS else None))
                e1.record()
                torch.cuda.synchronize()
                flag_rec[name, F][key].append(e0.elapsed_time(e1) / calls)
            for key, rd in (("read0", plain), ("read1", both)):
                t0 = time.perf_counter()
                rd.read([files[name][0]] * F)
                torch.cuda.synchronize()
                flag_rec[name, F][key].append(1e3 * (time.perf_counter() - t0))
    if "e" in a.sections:
        SH, SW = 900, 1600
        store = FrameStore(SH, SW, 2, DEV, gated=True, object_loss=True, dynamic=True, motion=True)
        ing = ingest.FrameIngest(store, (H, W))
        cam = make_camera(0, SH, SW)
        kw = dict(accum_R=torch.eye(3), accum_T=torch.eye(4))
        for label in ("device encoder", "Pillow"):
            if label == "Pillow" and Image is None:
                continue
            f_img, f_mask = files[f"RGB frame, {label}"][0], files[f"mask, {label}"][0]
            off, on = [], []
            for k in range(a.regions + 1):                           # (the first turn warms)
                for out, frame_i, seg in ((off, 0, False), (on, 1, True)):
                    t0 = time.perf_counter()
                    ing.put_files(frame_i, cam, image=f_img, hand_mask=f_mask, obj_mask=f_mask, segments=seg, **kw)
                    torch.cuda.synchronize()
                    if k:
                        out.append(1e3 * (time.perf_counter() - t0))
            assert torch.equal(store.img[0], store.img[1]) and torch.equal(store.bits[0], store.bits[1])
            flag_put[label] = (off, on)

    props = torch.cuda.get_device_properties(0)
    lines = ["# PNG files read on the device", "",
             f"`python tools/time_png_decode.py` -- one process; {W} x {H}.  RGB frame: an 8-bit render of the committed trained scene "
             f"(bench_data/trained_scene.npz); mask: its channel mean thresholded at its median.  Device: {props.name} "
             f"({props.multi_processor_count} CUs), torch {torch.__version__}"
             + (f", Pillow {PIL.__version__}" if Image is not None else "; Pillow is NOT installed here: its files and its legs are skipped")
             + f".  Library source hash {lib.built_source_hash()}.  A batch is that many copies of one file.  Every figure is the median "
             f"(min .. max) of {a.regions} repeats, the legs alternating inside each repeat: the spread of A against A.  Times in ms."]
    if a.append:
        lines = []
    if "a" in a.sections:
        lines += ["", "## (a), (b) The decode, per batch", "",
             "| file | file bytes / raw bytes | batch | three launches | gather + CRC | inflate | unfilter | files/s | decoded MB/s | PngReader.read, wall |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for (name, F), r in rec.items():
        data, x = files[name]
        raw = x.numel()
        m = _stats(r["all"])[0]
        lines.append(f"| {name} | {len(data)} / {raw} ({100.0 * len(data) / raw:.1f} %) | {F} | {_fmt(r['all'])} | {_fmt(r['gather'])} | {_fmt(r['inflate'])} | "
                     f"{_fmt(r['unfilter'])} | {1e3 * F / m:.0f} | {F * raw / m / 1e3:.0f} | {_fmt(r['read'])} |")
    if "d" in a.sections:
        lines += ["", "## (d) The host readers, per file", "",
                  "| file | Pillow open + load, one thread | Pillow, 16 threads over 32 files, per file | zlib.decompress of the stream alone |", "|---|---|---|---|"]
    for name, h in host.items():
        lines.append(f"| {name} | {_fmt(h['one']) if h['one'] else 'no Pillow'} | {_fmt(h['pool16']) if h['pool16'] else 'no Pillow'} | {_fmt(h['zlib'])} |")
    if "c" in a.sections:
        lines += ["", "## (c) One frame into the store: image + hand mask + object mask, " + f"{W} x {H} -> {SW} x {SH}", "",
                  "| files | uploaded bytes, put_files / put | FrameIngest.put of host-decoded arrays, wall | FrameIngest.put_files, wall |", "|---|---|---|---|"]
    for label, (p, pf, nbytes) in put_rec.items():
        lines.append(f"| {label} | {nbytes} / {5 * H * W} | {_fmt(p)} | {_fmt(pf)} |")
    if "c" in a.sections:
        lines += ["", "put() starts from arrays that a host reader has already decoded: the time of that decode is the table above, not part of its column."]
    if "e" in a.sections:
        lines += ["", "## (e) The segmented route (EGS_PNG_SEGMENTS) against the serial wave", "",
                  f"egs_png_decode_ex on one uploaded batch, the flag off against the flag on in the same alternating repeats ({props.name}, library source hash "
                  f"{lib.built_source_hash()}).  Inflate: the launches of phase 2 -- with the flag measure, scan, place and the serial wave for what fell "
                  "back.  The factor is median off / median on.", "",
                  "| file | route | batch | inflate, serial | inflate, segments | factor | all launches, no flag | all launches, segments | "
                  "PngReader.read wall, no flag | PngReader.read wall, segments |", "|---|---|---|---|---|---|---|---|---|---|"]
        for (name, F), r in flag_rec.items():
            m = lambda k: _stats(r[k])[0]
            lines.append(f"| {name} | {png.route_text(flag_readers[name, F][2])} | {F} | {_fmt(r['inflate0'])} | {_fmt(r['inflate1'])} | "
                         f"{m('inflate0') / m('inflate1'):.2f}x | {_fmt(r['all0'])} | {_fmt(r['all1'])} | {_fmt(r['read0'])} | {_fmt(r['read1'])} |")
        lines += ["", f"FrameIngest.put_files per frame (image + hand mask + object mask, {W} x {H} -> 1600 x 900), wall:", "",
                  "| files | no flag | segments |", "|---|---|---|"]
        for label, (off, on) in flag_put.items():
            lines.append(f"| {label} | {_fmt(off)} | {_fmt(on)} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
