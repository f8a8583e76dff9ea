"""Images shared by the PNG tests (tests/test_png_cpu.py, tests/test_gpu_png.py): the smallest shapes at which the encoder can go wrong.
Every image is uint8 [C,H,W], seeded, built once and left unchanged."""
import functools

import numpy as np


def _noise(seed, C, H, W):
    return np.random.default_rng(seed).integers(0, 256, (C, H, W), dtype=np.uint8)


def _arbitrary(seed, C, H, W):
    """Neither noise nor flat: a coarse gradient, a few flat runs and some noise -- literals, runs and every filter have something to do."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(3 * xx + 5 * yy + 40 * c) & 255 for c in range(C)]).astype(np.uint8)
    img[:, :, W // 3:W // 3 + max(1, W // 4)] = 200
    k = rng.random((C, H, W)) < 0.2
    img[k] = rng.integers(0, 256, int(k.sum()), dtype=np.uint8)
    return img


def half_plane(H=512, W=512):
    """A 0 / 255 mask cut by a slanted line: rows of two long runs, each longer than 258, the edge moving from row to row."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (((2 * xx + yy) > W + H // 2) * 255).astype(np.uint8)[None]


def ramp(H=256, W=256):
    """A smooth ramp with slopes below one level per pixel, a different one per channel: the filtered rows are small residuals."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(200 * xx) // (W - 1), (170 * yy) // (H - 1), (120 * (xx + yy)) // (W + H - 2)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> uint8 [C,H,W] (names give W x H x C)."""
    out = {}
    for C in (1, 3):
        out[f"1x1x{C}"] = _noise(1, C, 1, 1)
        out[f"1x7x{C}"] = _arbitrary(2, C, 7, 1)
        out[f"7x1x{C}"] = _arbitrary(3, C, 1, 7)
        out[f"67x5x{C}"] = _arbitrary(4, C, 5, 67)
        out[f"130x3x{C}"] = _arbitrary(5, C, 3, 130)
        out[f"zeros64x{C}"] = np.zeros((C, 64, 64), dtype=np.uint8)
        out[f"full64x{C}"] = np.full((C, 64, 64), 255, dtype=np.uint8)
    out["half_plane512"] = half_plane()
    out["noise256x3"] = _noise(6, 3, 256, 256)
    out["ramp256x3"] = ramp()
    out["dither256x3"] = (ramp() + _noise(8, 3, 256, 256) // 64).astype(np.uint8)      # the ramp under two bits of noise: literals of a small alphabet
    yy, xx = np.mgrid[0:4, 0:1200]                                                      # rows of 3601 stream bytes, nearly all literals: more
    out["dither1200x4x3"] = (np.stack([xx // 6, yy * 9 + xx // 11, (xx + yy) // 8]) + _noise(9, 3, 4, 1200) // 16).astype(np.uint8)      # than 2583 tokens per segment (four bits of noise: ~3100)
    out["long22000x2x3"] = _arbitrary(7, 3, 2, 22000)
    for v in out.values():
        v.setflags(write=False)
    return out


def unfilter_reference(rows, W, C):
    """A plain loop written from the PNG specification (section 9, filter types 0 .. 4): filtered rows [H, 1 + W*C] -> raw rows [H, W*C]."""
    H = rows.shape[0]
    out = np.zeros((H, W * C), dtype=np.uint8)
    for y in range(H):
        f = int(rows[y, 0])
        for j in range(W * C):
            a = int(out[y, j - C]) if j >= C else 0
            b = int(out[y - 1, j]) if y else 0
            c = int(out[y - 1, j - C]) if (y and j >= C) else 0
            if f == 0:
                pred = 0
            elif f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            out[y, j] = (int(rows[y, 1 + j]) + pred) & 255
    return out


def filter_reference(img):
    """The filtered stream of uint8 [C,H,W] by a plain numpy loop from the specification and the project's selection rule (minimum sum of
    min(v, 256 - v), ties to the lowest type) -> uint8 [H, 1 + W*C]."""
    C, H, W = img.shape
    raw = img.transpose(1, 2, 0).reshape(H, W * C).astype(np.int64)
    out = np.zeros((H, 1 + W * C), dtype=np.uint8)
    for y in range(H):
        cand = np.zeros((5, W * C), dtype=np.int64)
        for j in range(W * C):
            x = raw[y, j]
            a = raw[y, j - C] if j >= C else 0
            b = raw[y - 1, j] if y else 0
            c = raw[y - 1, j - C] if (y and j >= C) else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pae = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cand[:, j] = [x, x - a, x - b, x - (a + b) // 2, x - pae]
        cand &= 255
        score = np.minimum(cand, 256 - cand).sum(1)
        f = int(np.flatnonzero(score == score.min())[0])
        out[y, 0] = f
        out[y, 1:] = cand[f]
    return out
