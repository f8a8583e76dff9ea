"""numpy statements of the mask hand-off's two definitions (include/egs_raster.h egs_label_mask / egs_interaction_gate), written from the
definitions and from nothing else: what the HIP kernels, the torch statements (egogaussian_amd/losses.py) and the sweep are held to.  Both are
integer-exact, so every comparison against them is an equality."""
import numpy as np


def label_mask_np(img, thr=0.5, target=None, keep=None):
    """img: float32 [3,H,W] -> dict(mask: uint8[H,W] (255 / 0, every pixel), predicted, target, intersection, kept: python ints over the
    pixels with keep >= 0.5 (None: all)).  The mean is ((c0 + c1) + c2) / 3 in float32; the comparison is strict, so NaN is not set."""
    img = np.asarray(img)
    assert img.dtype == np.float32 and img.ndim == 3 and img.shape[0] == 3
    H, W = img.shape[1:]
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((img[0] + img[1]) + img[2]) / np.float32(3)
        assert x.dtype == np.float32
        on = x > np.float32(thr)
    kept = np.ones((H, W), bool) if keep is None else np.asarray(keep, np.float32).reshape(H, W) >= np.float32(0.5)
    tgt = np.zeros((H, W), bool) if target is None else np.asarray(target, np.float32).reshape(H, W) >= np.float32(0.5)
    return dict(mask=np.where(on, 255, 0).astype(np.uint8), predicted=int((kept & on).sum()), target=int((kept & tgt).sum()),
                intersection=int((kept & on & tgt).sum()), kept=int(kept.sum()))


def gate_np(a, b, k):
    """a, b: [H,W] arrays or None (not both) -> float32 [H,W]: 0 where any pixel of the k x k window around it, clipped to the image, has
    a != 0 or b != 0 (NaN and negative values count), else 1.  An explicit window, pixel by pixel."""
    assert (a is not None or b is not None) and k >= 1 and k % 2 == 1
    on = None
    for m in (a, b):
        if m is not None:
            s = np.asarray(m) != 0                     # NaN != 0 is True
            on = s if on is None else (on | s)
    H, W = on.shape
    r = k // 2
    out = np.ones((H, W), np.float32)
    for y in range(H):
        y0, y1 = max(y - r, 0), min(y + r, H - 1)
        for x in range(W):
            x0, x1 = max(x - r, 0), min(x + r, W - 1)
            if on[y0:y1 + 1, x0:x1 + 1].any():
                out[y, x] = 0.0
    return out


def special_label_image(H, W, thr, seed):
    """float32 [3,H,W] around the threshold with planted pixels: channels whose mean is exactly thr (not set), the next float above it (set),
    NaN (not set) and three differing channels; -> (img, dict name -> (y, x) of the planted pixels that fit)."""
    rng = np.random.default_rng(seed)
    img = (np.float32(thr) + rng.standard_normal((3, H, W)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    t = np.float32(thr)
    up = np.nextafter(t, np.float32(np.inf), dtype=np.float32)
    # ((t + t) + t) / 3 == t for the thresholds used (checked below): equal channels put the mean exactly there
    spots = {}
    flat = [(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)]
    plant = [("exact", (t, t, t)), ("next", (up, up, up)), ("nan", (np.float32(np.nan), np.float32(1e3), np.float32(1e3))),
             ("differ", (np.float32(thr + 3.0), np.float32(thr - 1.0), np.float32(thr - 1.5)))]
    used = set()
    for (name, vals), pos in zip(plant, [p for p in dict.fromkeys(flat)]):
        if pos in used:
            continue
        used.add(pos)
        img[:, pos[0], pos[1]] = vals
        spots[name] = pos
    for v, want in ((t, False), (up, True)):
        m = ((v + v) + v) / np.float32(3)
        assert (m > t) == want, (thr, v, m)
    return img, spots
