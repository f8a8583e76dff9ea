"""Writes tests/golden/jpeg_files.npz: small baseline JPEG files as Pillow writes them, with np.asarray(Image.open(...)) of each -- what
libjpeg-turbo's default decode path (islow IDCT, fancy upsampling, fixed-point colour) makes of them -- and the versions of both libraries.
Run once where Pillow is installed:
    python tests/golden/make_golden_jpeg_files.py
All images are generated (no photographs).  The decoder tests read the archive and need no Pillow."""
import io
import os

import numpy as np
import PIL
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (17, 33), (31, 15), (37, 53), (4, 3), (5, 6)]      # (W, H); the last two: chroma width 2 and 3
SUB = {"444": 0, "422": 1, "420": 2}


def image(W, H, C, seed, noise=6):
    """A coarse gradient with an edge and some noise: every frequency has a coefficient, chroma changes from sample to sample."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([7 * xx + 3 * yy + 60 * c + 90 * ((xx + c) // 5 % 2) for c in range(C)], -1) + rng.integers(0, noise, (H, W, C))
    a = (a & 255).astype(np.uint8)
    return a if C == 3 else a[:, :, 0]


def save(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a, "L" if a.ndim == 2 else "RGB").save(buf, format="JPEG", **kw)
    data = buf.getvalue()
    got = np.asarray(Image.open(io.BytesIO(data)))
    return np.frombuffer(data, dtype=np.uint8), np.ascontiguousarray(got.reshape(got.shape[0], got.shape[1], -1))


def main():
    out = {}

    def add(name, a, **kw):
        out[name + ".file"], out[name + ".pixels"] = save(a, **kw)

    for k, (W, H) in enumerate(SIZES):
        for sub, code in SUB.items():
            add(f"{W}x{H}-{sub}", image(W, H, 3, 10 + k), subsampling=code)
        add(f"{W}x{H}-L", image(W, H, 1, 30 + k))
    big, mid = image(37, 53, 3, 50), image(17, 33, 3, 51)
    add("37x53-420-rb1", big, subsampling=2, restart_marker_blocks=1)              # 12 intervals: the marker number wraps
    add("37x53-420-rb2", big, subsampling=2, restart_marker_blocks=2)
    add("37x53-444-rr1", big, subsampling=0, restart_marker_rows=1)
    add("17x33-422-rb1", mid, subsampling=1, restart_marker_blocks=1)
    add("31x15-L-rb2", image(31, 15, 1, 52), restart_marker_blocks=2)
    add("37x53-L-rr1", image(37, 53, 1, 53), restart_marker_rows=1)
    add("37x53-444-opt30", big, subsampling=0, optimize=True, quality=30)
    add("37x53-420-opt30", big, subsampling=2, optimize=True, quality=30)
    add("17x33-422-opt30", mid, subsampling=1, optimize=True, quality=30)
    add("37x53-L-opt30", image(37, 53, 1, 54), optimize=True, quality=30)
    noise = np.random.default_rng(60).integers(0, 256, (40, 24, 3), dtype=np.uint8)
    for sub, code in SUB.items():
        add(f"24x40-{sub}-q100-noise", noise, subsampling=code, quality=100)
        assert b"\xff\x00" in out[f"24x40-{sub}-q100-noise.file"].tobytes(), "the noise files are there for the stuffed bytes"
    wave = image(72, 72, 3, 61)
    add("72x72-444-rb1", wave, subsampling=0, restart_marker_blocks=1)             # 81 intervals: more than a wave
    add("72x72-444", wave, subsampling=0)                                          # its restart-free twin: the same coefficients
    assert np.array_equal(out["72x72-444-rb1.pixels"], out["72x72-444.pixels"]) and out["72x72-444-rb1.file"].size != out["72x72-444.file"].size
    add("16x16-420-app1-com", image(16, 16, 3, 62), subsampling=2, exif=b"Exif\x00\x00MM\x00*\x00\x00\x00\x08\x00\x00\x00\x00\x00\x00",
        comment=b"generated")
    data = out["16x16-420-app1-com.file"].tobytes()
    assert b"\xff\xe1" in data and b"\xff\xfe" in data
    add("130x67-420", image(130, 67, 3, 63), subsampling=2)                        # the source frame of the ingest tests
    out["16x16-progressive.refused"] = save(image(16, 16, 3, 64), progressive=True)[0]
    assert b"\xff\xc2" in out["16x16-progressive.refused"].tobytes()
    out["pillow_version"] = np.frombuffer(PIL.__version__.encode(), dtype=np.uint8)
    out["libjpeg_turbo_version"] = np.frombuffer(str(features.version("libjpeg_turbo")).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_files.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", sum(k.endswith(".file") for k in out), "files, Pillow", PIL.__version__, "libjpeg-turbo",
          features.version("libjpeg_turbo"))


if __name__ == "__main__":
    main()
