"""CPU: the host statements of the PNG writer (egogaussian_amd/png.py filter_rows, encode_statement, decode) and the argument checks and the
capacity formula of its C entries (include/egs_raster.h egs_png_*).  No device is touched."""
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import png_cases as PC

SMALL = [n for n, v in PC.cases().items() if v.size <= 2000]


def _five():
    """Six rows of 24 grey pixels, each built so that one filter type predicts it best."""
    W = 24
    x = np.arange(W)
    r0 = np.where(x % 2 == 0, 1, 255)                            # +-1 around zero: None scores 1 per byte, every difference 2
    r1 = (7 * x + 30) & 255                                      # a steep horizontal gradient over an unrelated row: Sub
    r2 = np.concatenate([r1[:12], np.full(12, 250)])             # half the row above, half a flat run: only Paeth switches between Up and Sub
    r3 = r2 + np.array([0, 1, 2] * 8)                            # the row above plus a small pattern: Up (Paeth ties with it and loses)
    r4 = np.zeros(W, dtype=np.int64)
    for j in range(W):
        r4[j] = ((r4[j - 1] if j else 0) + r3[j]) >> 1           # the mean of left and above: Average leaves nothing
    r5 = np.full(W, 9)
    return np.stack([r0, r1, r2, r3, r4, r5]).astype(np.uint8)[None]


@pytest.mark.parametrize("name", list(PC.cases()))
def test_statement_round_trip(name):
    from egogaussian_amd import png
    x = PC.cases()[name]
    data = png.encode_statement(torch.from_numpy(x.copy()))
    got = png.decode(data)
    assert got.dtype == np.uint8 and np.array_equal(got, x[0] if x.shape[0] == 1 else x)
    W, H, Cn, rows = png.inflate(data)
    assert (W, H, Cn) == (x.shape[2], x.shape[1], x.shape[0])
    assert np.array_equal(rows, png.filter_rows(torch.from_numpy(x.copy())).numpy())
    # one IDAT per segment and one for the final block
    assert data.count(b"IDAT") >= len(png.segments(H, W * Cn)) + 1


@pytest.mark.parametrize("name", list(PC.cases()))
def test_statement_opens_in_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    import io
    from egogaussian_amd import png
    x = PC.cases()[name]
    im = Image.open(io.BytesIO(png.encode_statement(x)))
    im.load()
    assert im.mode == ("L" if x.shape[0] == 1 else "RGB")
    a = np.asarray(im)
    assert np.array_equal(a if x.shape[0] == 1 else a.transpose(2, 0, 1), x[0] if x.shape[0] == 1 else x)


@pytest.mark.parametrize("name", SMALL + ["five"])
def test_filter_rows_equals_the_specification_loop(name):
    from egogaussian_amd import png
    x = _five() if name == "five" else PC.cases()[name]
    want = PC.filter_reference(x)
    got = png.filter_rows(torch.from_numpy(x.copy())).numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(PC.unfilter_reference(got, x.shape[2], x.shape[0]), x.transpose(1, 2, 0).reshape(x.shape[1], -1))


def test_every_filter_wins_somewhere_and_ties_go_to_the_lower_type():
    from egogaussian_amd import png
    types = png.filter_rows(_five())[:, 0].tolist()
    print("filter types of the six rows:", types)
    assert types[:5] == [0, 1, 4, 2, 3] and set(types) == {0, 1, 2, 3, 4}
    # a black row: every score is 0 -> None.  Rows of 255 under a row of 255: Up and Paeth both leave zeros -> Up.
    assert png.filter_rows(np.zeros((1, 1, 9), dtype=np.uint8))[0, 0] == 0
    full = png.filter_rows(np.full((3, 4, 9), 255, dtype=np.uint8))
    assert full[:, 0].tolist() == [1, 2, 2, 2] and int(full[1:, 1:].max()) == 0
    ref = PC.filter_reference(np.full((3, 4, 9), 255, dtype=np.uint8))
    assert np.array_equal(full.numpy(), ref)
    # the two-dimensional form is the one-channel image
    g = PC.cases()["67x5x1"]
    assert torch.equal(png.filter_rows(g[0]), png.filter_rows(g))


def _chunks(data):
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((kind, pos, n))
        pos += 12 + n
    return out


def _rebuild(data, payloads):
    """The file `data` with the zlib stream replaced by `payloads` (one IDAT each), CRCs right."""
    from egogaussian_amd import png
    ch = _chunks(data)
    ihdr = data[8:8 + 12 + ch[0][2]]
    return png.SIGNATURE + ihdr + b"".join(png._chunk(b"IDAT", p) for p in payloads) + png._chunk(b"IEND", b"")


def test_decode_rejects_broken_files():
    from egogaussian_amd import png
    x = PC.cases()["67x5x3"]
    data = png.encode_statement(x)
    assert np.array_equal(png.decode(data), x)
    ch = _chunks(data)
    # a flipped CRC bit, in IHDR and in an IDAT
    for kind, pos, n in (ch[0], ch[2]):
        bad = bytearray(data)
        bad[pos + 8 + n + 3] ^= 1
        with pytest.raises(ValueError, match="CRC"):
            png.decode(bytes(bad))
    # a truncated file, and a truncated stream in a well-formed container
    with pytest.raises(ValueError):
        png.decode(data[:len(data) - 20])
    stream = b"".join(data[pos + 8:pos + 8 + n] for kind, pos, n in ch if kind == b"IDAT")
    with pytest.raises(ValueError, match="truncated"):
        png.decode(_rebuild(data, [stream[:-7]]))
    # a wrong Adler-32
    wrong = bytearray(stream)
    wrong[-1] ^= 0x10
    with pytest.raises(ValueError, match="png.decode"):
        png.decode(_rebuild(data, [bytes(wrong)]))
    # a filter byte of 5
    rows = png.filter_rows(x).numpy().copy()
    rows[2, 0] = 5
    with pytest.raises(ValueError, match="filter type 5"):
        png.decode(_rebuild(data, [zlib.compress(rows.tobytes())]))
    # a wrong inflated length, bytes behind IEND, another chunk, a 16-bit header
    with pytest.raises(ValueError, match="inflated"):
        png.decode(_rebuild(data, [zlib.compress(rows.tobytes()[:-1])]))
    with pytest.raises(ValueError, match="behind IEND"):
        png.decode(data + b"\0")
    with pytest.raises(ValueError, match="chunks"):
        png.decode(data[:-12] + png._chunk(b"tEXt", b"a\0b") + data[-12:])
    hdr16 = png._chunk(b"IHDR", struct.pack(">IIBBBBB", 67, 5, 16, 2, 0, 0, 0))
    with pytest.raises(ValueError, match="IHDR"):
        png.decode(png.SIGNATURE + hdr16 + data[8 + 25:])
    with pytest.raises(ValueError, match="signature"):
        png.decode(b"\x89PNG\r\n\x1a\r" + data[8:])


def test_constant_image_statement_is_inside_the_size_condition():
    """The size condition of constant images, on the host: with one row per segment a constant 960x540 image needs far less than 100 + 64 H bytes (a
    literal-only encoder needs >= 360 bytes per black RGB row)."""
    from egogaussian_amd import png
    H, W = 540, 960
    for Cn, v in ((3, 0), (1, 0), (3, 255), (1, 255)):
        n = len(png.encode_statement(np.full((Cn, H, W), v, dtype=np.uint8)))
        print(f"constant {v} {W}x{H}x{Cn}: statement {n} bytes, limit {100 + 64 * H}")
        assert n <= 100 + 64 * H
        assert n < 360 * H // 4


def test_bound_agrees_with_its_formula_and_argument_errors_precede_device_work():
    from egogaussian_amd import lib, png
    L = lib.load()
    for W, H, Cn in ((1, 1, 1), (1, 1, 3), (960, 540, 3), (960, 540, 1), (4095, 3, 1), (4096, 3, 1), (1365, 2, 3), (1366, 2, 3), (22000, 2, 3),
                     (32767, 32767, 3)):
        rb = W * Cn + 1
        want = 77 + H * rb + 17 * H * ((rb + 4095) // 4096)
        assert L.egs_png_bound(W, H, Cn) == want == png.bound(W, H, Cn), (W, H, Cn)
    assert L.egs_png_bound(960, 540, 3) <= 1.05 * 540 * 2881
    for W, H, Cn in ((0, 4, 1), (4, 0, 1), (32768, 4, 1), (4, 32768, 3), (4, 4, 2), (4, 4, 4)):
        assert L.egs_png_bound(W, H, Cn) == 0 and L.egs_png_scratch_bytes(1, W, H, Cn) == 0
    assert L.egs_png_scratch_bytes(0, 4, 4, 1) == 0
    assert L.egs_png_scratch_bytes(2, 960, 540, 3) == 2 * L.egs_png_scratch_bytes(1, 960, 540, 3) >= 2 * 540 * 2881
    p = 4096                                                            # (fake non-null pointers are never dereferenced before the checks)
    W, H = 8, 4
    b = L.egs_png_bound(W, H, 3)
    ok = dict(n=1, W=W, H=H, C=3, src=p, image_stride=3 * W * H, plane_stride=W * H, out=p, out_stride=b, sizes=p, scratch=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.egs_png_encode(a["n"], a["W"], a["H"], a["C"], a["src"], a["image_stride"], a["plane_stride"], a["out"], a["out_stride"],
                                a["sizes"], a["scratch"], None)
    ARG, RANGE = -1, -3
    for kw in (dict(n=0), dict(src=None), dict(out=None), dict(sizes=None), dict(scratch=None), dict(scratch=p + 8), dict(sizes=p + 2),
               dict(plane_stride=W * H - 1), dict(out_stride=b - 1), dict(n=2, image_stride=3 * W * H - 1)):
        assert call(**kw) == ARG, kw
    for kw in (dict(W=0), dict(H=0), dict(W=32768), dict(H=32768), dict(C=2), dict(C=4), dict(C=0), dict(n=65536)):
        assert call(**kw) == RANGE, kw
    # CPU tensors are refused by the Python layer, as elsewhere
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode(torch.zeros((1, 3, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.PngWriter(4, 4, 3, "cpu")


def test_segments_cover_the_stream_once():
    from egogaussian_amd import png
    for H, rb, k in ((5, 201, 1), (2, 66000, 1), (7, 30, 3), (3, 4095, 1), (3, 4096, 1)):
        seg = png.segments(H, rb, k)
        assert seg[0][0] == 0 and seg[-1][1] == H * (rb + 1) and all(a[1] == b[0] for a, b in zip(seg, seg[1:]))
        assert all(0 < hi - lo <= k * png.SEGMENT_BYTES for lo, hi in seg)
    assert len(png.segments(2, 66000, 1)) == 2 * 17
