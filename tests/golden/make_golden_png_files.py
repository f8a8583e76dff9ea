"""Writes tests/golden/png_files.npz: a dozen small PNG files as Pillow writes them (default, optimize=True, compress_level 1 and 9; modes L
and RGB; the small shapes of tests/png_cases.py) with their pixel arrays.  Run once where Pillow is installed:
    python tests/golden/make_golden_png_files.py
The decoder tests read the archive and need no Pillow."""
import io
import os
import sys

import numpy as np
from PIL import Image
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import png_cases as PC  # noqa: E402

SETTINGS = [("default", {}), ("optimize", {"optimize": True}), ("level1", {"compress_level": 1}), ("level9", {"compress_level": 9})]
IMAGES = ["67x5x1", "130x3x3", "7x1x3", "1x7x1", "zeros64x1", "full64x3"]


def main():
    out = {}
    k = 0
    for name in IMAGES:
        img = PC.cases()[name]
        a = img[0] if img.shape[0] == 1 else img.transpose(1, 2, 0)
        for label, kw in (SETTINGS[k % 4], SETTINGS[(k + 1) % 4]):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(a), "L" if img.shape[0] == 1 else "RGB").save(buf, format="PNG", **kw)
            out[f"{name}-{label}.file"] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
            out[f"{name}-{label}.pixels"] = np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1))
        k += 1
    out["pillow_version"] = np.frombuffer(PIL.__version__.encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "png_files.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(IMAGES) * 2, "files")


if __name__ == "__main__":
    main()
