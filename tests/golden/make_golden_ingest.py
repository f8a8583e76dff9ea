#!/usr/bin/env python
"""Generates tests/golden/ingest.npz by IMPORTING the reference's Python (read-only, /root/reference) in the build container, as its
siblings do: what loadCam (utils/camera_utils.py:21-94) makes of a frame's 8-bit sources,

    utils.general_utils.PILtoTorch      (:22-39)   PIL.Image.resize with the default filter, then / 255
    utils.general_utils.binarize_mask   (:41-60)   any channel > 0
    utils.camera_utils.loadCam          (:24-41)   the size rule, with stand-in cam_info / args (its Camera replaced by a recorder)

on seeded images and masks.  Only data is recorded -- the sources, the resized bytes, the binarised masks, the sizes -- never program text.
Run:  python tests/golden/make_golden_ingest.py      (needs Pillow; the tests that read the fixture do not)
"""
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                    # noqa: E402  (puts the reference on sys.path)

# source h x w -> target W x H
CASES = [((54, 96), (80, 45)),       # the 1080p -> 1600 ratio
         ((37, 53), (41, 29)),       # W = 41: mask words straddle rows
         ((64, 64), (32, 32)),
         ((64, 256), (32, 8)),       # scale 8, ksize 33
         ((20, 31), (64, 50)),       # upscale
         ((50, 50), (50, 20)),       # horizontal pass skipped
         ((17, 1), (1, 5)),          # single column: 17 rows of one pixel -> 5 rows (scale 3.4)
         ((29, 41), (41, 29)),       # W = w and H = h: nothing resized
         ((29, 41), (29, 41))]       # the width down, the height up
# (orig_w, orig_h, resolution, resolution_scale)
SIZE_ROWS = [(1920, 1080, -1, 1.0), (456, 256, -1, 1.0), (1921, 1081, -1, 1.0), (1920, 1080, 2, 1.0), (1002, 701, 4, 1.0),
             (1920, 1080, 800, 1.0), (1920, 1080, -1, 2.0)]
MASK_KINDS = ["rect", "pixels", "ones", "blue", "zero", "full", "blobs"]


def image(rng, h, w):
    """Blocks of one colour (the fixture stays small), hard 0 / 255 edges (the clamp of both passes) and single-pixel noise."""
    b = 3
    coarse = rng.integers(0, 256, ((h + b - 1) // b, (w + b - 1) // b, 3), dtype=np.uint8)
    a = np.repeat(np.repeat(coarse, b, axis=0), b, axis=1)[:h, :w].copy()
    a[: h // 3, w // 2:] = 255
    a[h // 2:, : w // 3] = 0
    n = max(1, h * w // 40)
    a[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    return a


def mask(rng, h, w, kind):
    """-> uint8 [h, w, 3]; an L mask takes channel 2 of it (so that `blue` is a mask there too)."""
    m = np.zeros((h, w, 3), dtype=np.uint8)
    if kind == "rect":
        m[h // 4: max(h // 4 + 1, 3 * h // 4), w // 5: max(w // 5 + 1, 2 * w // 3)] = 255
    elif kind == "pixels":
        n = max(1, h * w // 60)
        m[rng.integers(0, h, n), rng.integers(0, w, n)] = 255
    elif kind == "ones":
        m[h // 3: max(h // 3 + 1, 2 * h // 3), : max(1, w // 2)] = 1
        m[rng.integers(0, h, 3), rng.integers(0, w, 3)] = 1
    elif kind == "blue":
        m[h // 5: max(h // 5 + 1, h // 2), w // 3:, 2] = 200
    elif kind == "full":
        m[:] = 255
    elif kind == "blobs":
        coarse = (rng.random(((h + 4) // 5, (w + 4) // 5)) < 0.4).astype(np.uint8) * rng.integers(1, 256, ((h + 4) // 5, (w + 4) // 5), dtype=np.uint8)
        m[:] = np.repeat(np.repeat(coarse, 5, axis=0), 5, axis=1)[:h, :w, None]
    return m


def main():
    scene = mg.stub("scene")                                 # (scene/__init__.py pulls in the whole trainer: only scene.cameras is wanted)
    scene.__path__ = [os.path.join(mg.REF, "scene")]
    from utils.general_utils import PILtoTorch, binarize_mask
    import utils.camera_utils as cu

    rng = np.random.default_rng(2110)
    u8 = lambda t: t.round().to(torch.uint8).numpy()
    out = dict(cases=np.array([[h, w, W, H] for (h, w), (W, H) in CASES], dtype=np.int32))
    kinds = []
    for k, ((h, w), (W, H)) in enumerate(CASES):
        img = image(rng, h, w)
        kind_l, kind_rgb = MASK_KINDS[k % len(MASK_KINDS)], MASK_KINDS[(k + 3) % len(MASK_KINDS)]
        m_l = mask(rng, h, w, kind_l)[:, :, 2].copy()
        m_rgb = mask(rng, h, w, kind_rgb)
        kinds.append([kind_l, kind_rgb])
        pil_img, pil_l, pil_rgb = Image.fromarray(img), Image.fromarray(m_l), Image.fromarray(m_rgb)
        assert (pil_img.mode, pil_l.mode, pil_rgb.mode) == ("RGB", "L", "RGB")
        raw = PILtoTorch(pil_img, (W, H), normalize=False)                         # float bytes, [3, H, W]
        got = PILtoTorch(pil_img, (W, H), normalize=True)
        if float(raw.max()) > 1.0:
            assert torch.equal(got, raw.to(torch.uint8).float() / 255.0)           # what the store's table decodes a byte to
        out[f"img_{k}"], out[f"img_out_{k}"] = img, u8(raw).transpose(1, 2, 0)     # [H, W, 3], as np.array(resized) is
        for name, pil, src in (("l", pil_l, m_l), ("rgb", pil_rgb, m_rgb)):
            resized = PILtoTorch(pil, (W, H), normalize=False)
            binary = binarize_mask(PILtoTorch(pil, (W, H), normalize=True))        # loadCam's expression
            out[f"mask_{name}_{k}"] = src
            out[f"mask_{name}_out_{k}"] = u8(resized).transpose(1, 2, 0) if name == "rgb" else u8(resized)[0]
            out[f"mask_{name}_bin_{k}"] = binary[0].to(torch.uint8).numpy()        # [H, W] of 0 / 1
        print(k, (h, w), "->", (W, H), kinds[-1], "set bits", int(out[f"mask_l_bin_{k}"].sum()), int(out[f"mask_rgb_bin_{k}"].sum()))
    out["mask_kinds"] = np.array(kinds)

    # ---- the size rule: loadCam itself, its Camera replaced by a recorder -------------------------------------------------------------
    seen = {}
    cu.Camera = lambda **kw: seen.update(shape=tuple(kw["gt_image"].shape), hand=tuple(kw["hand_mask"].shape))
    rows = []
    for ow, oh, res, res_scale in SIZE_ROWS:
        info = types.SimpleNamespace(image=Image.new("RGB", (ow, oh)), hand_mask=Image.new("L", (ow, oh)), obj_mask=None, est_depth=None,
                                     pred_cb=None, uid=0, R=None, T=None, FovX=1.0, FovY=1.0, image_name="golden")
        cu.loadCam(types.SimpleNamespace(resolution=res, data_device="cpu"), 0, info, res_scale)
        _, H, W = seen["shape"]
        assert seen["hand"] == (1, H, W)
        rows.append([ow, oh, res, W, H])
        print("size", (ow, oh, res, res_scale), "->", (W, H))
    out["size_rows"] = np.array(rows, dtype=np.int32)
    out["size_resolution_scale"] = np.array([r[3] for r in SIZE_ROWS], dtype=np.float64)
    path = os.path.join(HERE, "ingest.npz")
    np.savez_compressed(path, **out)
    print("ingest.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
