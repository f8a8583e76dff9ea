"""GPU: the PNG encoder (csrc/png.hip, egogaussian_amd/png.py encode / PngWriter) over the smallest shapes at which it can go wrong.  PNG is
lossless: every file must decode -- by png.decode, a strict reader on stdlib zlib -- to exactly the input, its inflated stream must be
png.filter_rows byte for byte, and nothing outside a slot's first sizes[i] bytes may be touched."""
import functools
import io

import numpy as np
import pytest
import torch

from tests import png_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5


def _encode_with_canaries(x, pad_out=37, pad_src=0):
    """x: uint8 [F,C,H,W] numpy.  Encodes from a source whose image stride is pad_src bytes larger than an image and into slots of
    bound + pad_out bytes, everything around the used bytes preset to CANARY -> (files, sizes, bound, slots as numpy)."""
    from egogaussian_amd import lib, png
    F, C, H, W = x.shape
    b = png.bound(W, H, C)
    src = torch.full((F, C * H * W + pad_src), CANARY, dtype=torch.uint8, device=DEV)
    src[:, :C * H * W] = torch.from_numpy(x.reshape(F, -1).copy()).to(DEV)
    out = torch.full((F + 1, b + pad_out), CANARY, dtype=torch.uint8, device=DEV)
    sizes = torch.full((F + 1,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.empty(png.scratch_bytes(F, W, H, C), dtype=torch.uint8, device=DEV)
    imgs = src[:, :C * H * W].view(F, C, H, W)                                # image stride C H W + pad_src, the rest dense
    got, sz = png.encode(imgs, out=out, sizes=sizes, scratch=scratch)
    assert got.data_ptr() == out.data_ptr() and (pad_src == 0 or imgs.stride(0) > C * H * W)
    torch.cuda.synchronize()
    slots, sz = out.cpu().numpy(), sizes.cpu().numpy()
    assert sz[F] == -7 and (slots[F] == CANARY).all(), "the slot and the size behind the last image were written"
    files = []
    for i in range(F):
        assert 0 < sz[i] <= b, (i, int(sz[i]), b)
        assert (slots[i, b:] == CANARY).all(), f"image {i}: bytes beyond bound were written"
        files.append(slots[i, :sz[i]].tobytes())
    assert lib.load().egs_png_bound(W, H, C) == b
    return files, sz[:F], b, slots


@functools.lru_cache(maxsize=None)
def _encoded(name):
    x = PC.cases()[name]
    files, sz, b, slots = _encode_with_canaries(x[None])
    return files[0], int(sz[0]), b, slots


def _check_file(data, x):
    """data: file bytes; x: uint8 [C,H,W] numpy."""
    from egogaussian_amd import png
    got = png.decode(data)
    assert np.array_equal(got, x[0] if x.shape[0] == 1 else x)
    W, H, C, rows = png.inflate(data)
    assert np.array_equal(rows, png.filter_rows(torch.from_numpy(x.copy())).numpy()), "the inflated stream is not filter_rows"


@pytest.mark.parametrize("name", list(PC.cases()))
def test_file_decodes_to_the_input_and_its_stream_is_filter_rows(name):
    from egogaussian_amd import png
    x = PC.cases()[name]
    data, n, b, slots = _encoded(name)
    kinds = {0: "stored", 1: "fixed", 2: "dynamic"}
    W, H, C = x.shape[2], x.shape[1], x.shape[0]
    print(f"{name}: {n} bytes (bound {b}, filtered {H * (W * C + 1)}, statement {len(png.encode_statement(x))}), block kinds "
          f"{sorted(set(kinds[k] for k in _block_kinds(data)))}")
    _check_file(data, x)


def _block_kinds(data):
    """BTYPE of the first block of every segment's chunk (the chunks between the zlib header's and the final block's)."""
    from tests.test_png_cpu import _chunks
    ch = [(pos, n) for kind, pos, n in _chunks(data) if kind == b"IDAT"]
    return [(data[pos + 8] >> 1) & 3 for pos, n in ch[1:-1]]


def test_block_kinds_reach_every_path():
    """Noise must fall back to stored blocks in every segment, flat images use fixed codes, and a ramp under two bits of noise -- literals of
    a small alphabet -- dynamic codes.  (The clean ramp is periodic along a row: zlib and the kernel both spend it on a few long matches in
    fixed blocks; its kinds are printed.)"""
    assert set(_block_kinds(_encoded("noise256x3")[0])) == {0}
    assert set(_block_kinds(_encoded("zeros64x3")[0])) == {1}
    print("ramp256x3 block kinds:", sorted(set(_block_kinds(_encoded("ramp256x3")[0]))))
    assert set(_block_kinds(_encoded("dither256x3")[0])) == {2}
    assert set(_block_kinds(_encoded("dither1200x4x3")[0])) == {2}        # more than 2583 tokens in a segment: the Huffman counts are halved first
    assert len(_block_kinds(_encoded("long22000x2x3")[0])) == 2 * 17      # a row of 66 001 stream bytes: 17 segments, none beyond one stored block
    assert len(_block_kinds(_encoded("half_plane512")[0])) == 512


@pytest.mark.parametrize("name", list(PC.cases()))
def test_pillow_opens_the_file(name):
    Image = pytest.importorskip("PIL.Image")
    x = PC.cases()[name]
    im = Image.open(io.BytesIO(_encoded(name)[0]))
    im.load()
    a = np.asarray(im)
    assert im.mode == ("L" if x.shape[0] == 1 else "RGB")
    assert np.array_equal(a if x.shape[0] == 1 else a.transpose(2, 0, 1), x[0] if x.shape[0] == 1 else x)


@pytest.mark.parametrize("name", ["67x5x3", "half_plane512", "ramp256x3", "dither256x3", "dither1200x4x3", "noise256x3", "long22000x2x3"])
def test_two_encodes_give_identical_bytes(name):
    x = PC.cases()[name]
    again = _encode_with_canaries(x[None])[0][0]
    assert again == _encoded(name)[0]


@pytest.mark.parametrize("C", [1, 3])
def test_three_images_with_strides_larger_than_needed(C):
    """F = 3, different contents and different resulting sizes, image_stride and out_stride larger than needed."""
    H, W = 37, 150
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([(xx + c) & 255 for c in range(C)]).astype(np.uint8)                      # a gradient
    b = rng.integers(0, 256, (C, H, W), dtype=np.uint8)                                  # noise
    c = np.zeros((C, H, W), dtype=np.uint8); c[:, 5:20, 30:90] = 255                     # a rectangle
    x = np.stack([a, b, c])
    files, sz, bnd, slots = _encode_with_canaries(x, pad_out=101, pad_src=53)
    print("sizes", sz.tolist(), "bound", bnd)
    assert len(set(sz.tolist())) == 3
    for i in range(3):
        _check_file(files[i], x[i])


def test_captured_encode_replays_on_new_input():
    from egogaussian_amd import png
    x0, x1 = PC.cases()["130x3x3"], PC.cases()["130x3x3"][:, ::-1, ::-1].copy()
    C, H, W = x0.shape
    src = torch.from_numpy(x0.copy()).to(DEV)[None].contiguous()
    out = torch.zeros((1, png.bound(W, H, C)), dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(png.scratch_bytes(1, W, H, C), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        png.encode(src, out=out, sizes=sizes, scratch=scratch)                          # warm: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        png.encode(src, out=out, sizes=sizes, scratch=scratch)
    first = out[0, :int(sizes[0])].cpu().numpy().tobytes()
    src.copy_(torch.from_numpy(x1).to(DEV)[None])
    out.zero_(); sizes.zero_()
    g.replay()
    torch.cuda.synchronize()
    second = out[0, :int(sizes[0])].cpu().numpy().tobytes()
    _check_file(first, x0)
    _check_file(second, x1)
    assert first != second


@pytest.mark.parametrize("C,v", [(3, 0), (1, 0), (3, 255), (1, 255)])
def test_constant_image_size_condition(C, v):
    """A constant 960x540 image: the file is <= 100 + 64 H bytes -- per row 12 bytes of chunk framing, 5 of byte alignment and a block of
    <= 12 maximal matches at <= 13 bits plus header and end code.  A literal-only encoder needs >= 360 bytes per black RGB row."""
    H, W = 540, 960
    x = np.full((1, C, H, W), v, dtype=np.uint8)
    files, sz, bnd, _ = _encode_with_canaries(x)
    print(f"constant {v} {W}x{H}x{C}: {int(sz[0])} bytes, limit {100 + 64 * H}")
    assert int(sz[0]) <= 100 + 64 * H
    _check_file(files[0], x[0])


@pytest.mark.parametrize("name", ["ramp256x3", "half_plane512"])
def test_size_against_the_statement(name):
    """The kernel's file is no larger than 1.10 x encode_statement with the same segmentation (zlib restricted to the same independent
    segments)."""
    from egogaussian_amd import png
    x = PC.cases()[name]
    n, s = _encoded(name)[1], len(png.encode_statement(x, segment_rows=1))
    d = PC.cases()["dither256x3"]
    print(f"{name}: kernel {n} bytes, statement {s} bytes, ratio {n / s:.4f}  (not held to the bar: the dithered ramp, kernel "
          f"{_encoded('dither256x3')[1]}, statement {len(png.encode_statement(d))})")
    assert n <= 1.10 * s


def test_writer_saves_five_small_frames(tmp_path):
    from egogaussian_amd import png
    rng = np.random.default_rng(5)
    H, W = 19, 45
    x = rng.integers(0, 4, (5, 3, H, W), dtype=np.uint8) * 60
    x[3] = 7
    paths = [tmp_path / f"f{i}.png" for i in range(5)]
    wr = png.PngWriter(H, W, 3, DEV, batch=2)                                          # three batches: 2 + 2 + 1
    assert wr.threads <= 16
    written = wr.save(torch.from_numpy(x).to(DEV), paths)
    assert wr.host_reads == 3 and len(written) == 5
    for i in range(5):
        data = paths[i].read_bytes()
        assert len(data) == written[i]
        _check_file(data, x[i])
    with pytest.raises(RuntimeError, match="no CPU path"):
        wr.save(torch.from_numpy(x), paths)
    m = (rng.random((3, H, W)) < 0.5).astype(np.uint8) * 255                             # masks: [F,H,W]
    mp = [tmp_path / f"m{i}.png" for i in range(3)]
    png.PngWriter(H, W, 1, DEV).save(torch.from_numpy(m).to(DEV), mp)
    for i in range(3):
        assert np.array_equal(png.decode(mp[i].read_bytes()), m[i])


def test_eval_pass_saves_its_renders(tmp_path):
    from egogaussian_amd import png
    from egogaussian_amd.evaluate import EvalPass
    from tests.test_gpu_eval_pass import _scene, _model, F
    s = _scene()
    ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1, keep_images=True)
    paths = [tmp_path / f"render_{k}.png" for k in range(F)]
    res = ev.run(s["frames"], s["cams"][0], save_renders=paths)
    imgs = res["images"].cpu().numpy()
    for k in range(F):
        assert np.array_equal(png.decode(paths[k].read_bytes()), imgs[k])
    assert len(set(p.read_bytes() for p in paths)) == F and int(imgs.max()) > 0
    plain = ev.run(s["frames"], s["cams"][0])                                          # the default is unchanged
    assert "png_bytes" not in plain and torch.equal(plain["images"], res["images"])
    with pytest.raises(ValueError, match="keep_images"):
        EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1).run(s["frames"], s["cams"][0], save_renders=paths)


def test_mask_pass_saves_its_masks(tmp_path):
    from egogaussian_amd import png
    from egogaussian_amd.masks import MaskPass
    from tests.test_gpu_masks import _scene, _model, F
    s = _scene()
    paths = [tmp_path / f"mask_{k}.png" for k in range(F)]
    res = MaskPass(_model(), s["bg"]).run(s["frames"], s["cams"][0], save_masks=paths)
    masks = res["masks"].cpu().numpy()
    for k in range(F):
        assert np.array_equal(png.decode(paths[k].read_bytes()), masks[k])
    assert 0 < int((masks == 255).sum()) < masks.size


def test_frame_store_png_decodes_to_the_stored_bytes():
    from egogaussian_amd import png
    from egogaussian_amd.frames import FrameStore
    H, W, F = 21, 34, 5
    rng = np.random.default_rng(9)
    store = FrameStore(H, W, F, device=DEV)
    gts = rng.integers(0, 256, (F, 3, H, W), dtype=np.uint8)
    gts[2] = (gts[2] // 64) * 64
    for i in range(F):
        store.put(i, torch.zeros(35), gt=torch.from_numpy(gts[i]))
    buf, sizes = store.png([0, 1, 2, 4, 3])                                          # a run of three, then two single frames
    torch.cuda.synchronize()
    b, n = buf.cpu().numpy(), sizes.cpu().numpy()
    for k, i in enumerate([0, 1, 2, 4, 3]):
        stored = store.img[i, :store.n_img].view(3, H, W).cpu().numpy()
        assert np.array_equal(stored, gts[i])
        assert np.array_equal(png.decode(b[k, :n[k]].tobytes()), stored)
    with pytest.raises(ValueError, match="gt"):
        store.png([0], what="gate")
    with pytest.raises(RuntimeError, match="no CPU path"):
        FrameStore(H, W, 1).png([0])
