"""GPU: the JPEG decoder (csrc/jpeg_decode.hip; egogaussian_amd/jpeg.py JpegReader / decode_device) over the golden Pillow files and the
crafted files of tests/jpeg_cases.py.  Every equality is exact: a file decodes to the bytes Pillow gave and jpeg.decode states, a refused
file gives its status word, and nothing outside a file's own slots is written (guard bytes around every buffer and between the output slots)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _corpus_decoded():
    """The whole corpus -- grey and colour, every sampling, with and without restarts -- in ONE batch."""
    from egogaussian_amd import jpeg
    names = list(JC.golden())
    rd = jpeg.JpegReader(DEV, batch=64, guard=256)
    outs = rd.read([JC.golden()[n][0] for n in names])
    got = {n: o.cpu().numpy() for n, o in zip(names, outs)}
    return got, rd.check_guards(), rd.host_reads, list(rd.last_status)


def test_every_fixture_decodes_to_the_golden_pixels_in_one_batch():
    got, guards, reads, status = _corpus_decoded()
    assert status == [0] * len(got) and len(got) <= 64 and reads == 1, "one read of the status words per batch"
    bad = [n for n, a in got.items() if a.shape != JC.golden()[n][1].shape or not np.array_equal(a, JC.golden()[n][1])]
    assert not bad, bad
    assert guards, "bytes outside a slot, the scratch or the status words were written"


def test_every_fixture_decodes_to_the_statement():
    from egogaussian_amd import jpeg
    got = _corpus_decoded()[0]
    bad = [n for n, a in got.items() if not np.array_equal(a, jpeg.decode(JC.golden()[n][0]))]
    assert not bad, bad


def test_batches_of_one():
    from egogaussian_amd import jpeg
    rd = jpeg.JpegReader(DEV, batch=1, guard=256)
    names = list(JC.golden())
    outs = rd.read([JC.golden()[n][0] for n in names])
    assert rd.host_reads == len(names) and rd.last_status == [0] * len(names)
    for n, o in zip(names, outs):
        assert o.dtype == torch.uint8 and o.is_cuda and np.array_equal(o.cpu().numpy(), JC.golden()[n][1]), n
    assert rd.check_guards()
    assert rd.read([]) == []


def test_decode_device_and_no_cpu_path():
    from egogaussian_amd import jpeg
    for n in ("17x33-420", "31x15-L-rb2", "1x1-444"):
        data, pixels = JC.golden()[n]
        out = jpeg.decode_device(data, DEV)
        assert out.is_cuda and np.array_equal(out.cpu().numpy(), pixels), n
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.JpegReader("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.decode_device(JC.golden()["1x1-L"][0], "cpu")


def test_files_by_path(tmp_path):
    from egogaussian_amd import jpeg
    data, pixels = JC.golden()["37x53-422"]
    p = tmp_path / "a.jpg"
    p.write_bytes(data)
    rd = jpeg.JpegReader(DEV, guard=256)
    out = rd.read([p, data])
    assert np.array_equal(out[0].cpu().numpy(), pixels) and torch.equal(out[0], out[1]) and rd.check_guards()
    with pytest.raises(ValueError, match=r"file 1 \(.*b\.jpg\): jpeg\.parse: SOF2"):
        q = tmp_path / "b.jpg"
        q.write_bytes(JC.refusals()["SOF2"][0])
        rd.read([p, q])


def test_the_writers_files_decode_to_the_statement():
    from egogaussian_amd import jpeg
    rd = jpeg.JpegReader(DEV, batch=8, guard=256)
    names = list(JC.written())
    outs = rd.read([JC.written()[n][0] for n in names])
    for n, o in zip(names, outs):
        assert np.array_equal(o.cpu().numpy(), jpeg.decode(JC.written()[n][0])), n
    assert rd.check_guards()


def test_a_restart_per_mcu_file_and_its_twin_give_identical_pixels():
    from egogaussian_amd import jpeg
    a, b = JC.golden()["72x72-444-rb1"], JC.golden()["72x72-444"]
    assert a[0] != b[0]
    rd = jpeg.JpegReader(DEV, guard=256)
    x, y = rd.read([a[0], b[0]])
    assert torch.equal(x, y) and np.array_equal(x.cpu().numpy(), a[1]) and rd.check_guards()


@pytest.mark.parametrize("name", list(JC.malformed()))
def test_malformed_file_gives_its_status_and_harms_nothing_else(name):
    from egogaussian_amd import jpeg
    data, status = JC.malformed()[name]
    a, b = JC.golden()["37x53-420-rb1"], JC.golden()["31x15-L"]
    rd = jpeg.JpegReader(DEV, batch=4, guard=256)
    with pytest.raises(ValueError, match=r"file 1: .*\(status %d\)" % status) as e:
        rd.read([a[0], data, b[0]])
    assert "file 0" not in str(e.value) and "file 2" not in str(e.value)
    assert rd.last_status == [0, status, 0]
    assert jpeg.status_text(status) in str(e.value)
    assert np.array_equal(rd.last_results[0].cpu().numpy(), a[1]) and np.array_equal(rd.last_results[2].cpu().numpy(), b[1])
    assert bool((rd.last_results[1] == rd.GUARD_BYTE).all()), "a refused file receives no pixel"
    assert rd.check_guards()


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------------
def _tables(copies=1):
    from egogaussian_amd import jpeg
    data = JC.golden()["37x53-420-rb1"][0]
    return data, jpeg.plan([dict(jpeg.parse(data), nbytes=len(data))] * copies)


def _raw_call(mutate=None, shift=None, copies=1, **override):
    """`copies` of one file through the C entry with buffers preset to 0xA5; `mutate(desc, tables)` edits the host tables first, `shift` moves the
    named default pointers by that many bytes, the other keywords replace arguments.  -> (return code, True when no device buffer changed)."""
    from egogaussian_amd import lib, _hip
    L = lib.load()
    data, p = _tables(copies)
    desc, tables = p["desc"].copy(), p["tables"].copy()
    if mutate:
        mutate(desc, tables)
    override.setdefault("n_files", copies)
    bufs = {k: torch.full((131072,), 0xA5, dtype=torch.uint8, device=DEV) for k in ("files", "tables", "out", "status", "scratch")}
    args = dict(n_files=1, files=bufs["files"].data_ptr(), files_bytes=65536, desc_host=desc.ctypes.data, desc_device=bufs["tables"].data_ptr(),
                tables_host=tables.ctypes.data, tables_device=bufs["tables"].data_ptr() + 1024, n_intervals=p["n_intervals"],
                out=bufs["out"].data_ptr(), out_bytes=32768, status=bufs["status"].data_ptr(), scratch=bufs["scratch"].data_ptr(), scratch_bytes=131072)
    for k, v in (shift or {}).items():
        args[k] += v
    args.update(override)
    order = ("n_files", "files", "files_bytes", "desc_host", "desc_device", "tables_host", "tables_device", "n_intervals", "out", "out_bytes",
             "status", "scratch", "scratch_bytes")
    with _hip.device_ctx(torch.device(DEV)):
        rc = L.egs_jpeg_decode(*[args[k] for k in order], _hip.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, all(bool((bufs[k] == 0xA5).all()) for k in ("out", "status", "scratch"))


def _set(field, value, row=0):
    def f(desc, tables):
        desc[field][row] = value
    return f


def _table(kind, index, field, at, value):
    def f(desc, tables):
        (tables["quant"] if kind == "quant" else tables[kind][field])[0, index, at] = value
    return f


def test_the_two_file_call_the_error_cases_start_from_decodes():
    """The unmodified two-file tables, with the files and the device copy of the tables uploaded as the contract asks: accepted, both
    decoded, nothing else written.  (The error cases below differ from this call by one field of the host tables or one argument.)"""
    from egogaussian_amd import lib, _hip
    L = lib.load()
    data, p = _tables(2)
    pixels = JC.golden()["37x53-420-rb1"][1]
    desc, tables = p["desc"], p["tables"]
    host = np.full(65536, 0xA5, dtype=np.uint8)
    host[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    host[1024:1024 + tables.nbytes] = tables.view(np.uint8).reshape(-1)
    assert desc.nbytes <= 1024 and 1024 + tables.nbytes <= 8192
    for d in desc:
        at = 8192 + int(d["file_offset"])
        host[at:at + len(data)] = np.frombuffer(data, dtype=np.uint8)
    blob = torch.from_numpy(host).to(DEV)
    out, status, scratch = (torch.full((k,), 0xA5, dtype=torch.uint8, device=DEV) for k in (32768, 256, 131072))
    need = L.egs_jpeg_decode_scratch_bytes(2, p["n_intervals"], p["coef_bytes"], p["plane_bytes"])
    assert need <= 131072 and p["out_bytes"] <= 32768 and 8192 + p["files_bytes"] <= 65536
    with _hip.device_ctx(torch.device(DEV)):
        rc = L.egs_jpeg_decode(2, blob.data_ptr() + 8192, p["files_bytes"], desc.ctypes.data, blob.data_ptr(), tables.ctypes.data,
                               blob.data_ptr() + 1024, p["n_intervals"], out.data_ptr(), 32768, status.data_ptr(), scratch.data_ptr(), 131072,
                               _hip.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    assert status[:8].view(torch.int32).tolist() == [0, 0] and bool((status[8:] == 0xA5).all()) and bool((scratch[need:] == 0xA5).all())
    got = out.cpu().numpy()
    second = int(desc[1]["out_offset"])
    for o in (0, second):
        assert np.array_equal(got[o:o + pixels.size].reshape(pixels.shape), pixels)
    assert (got[pixels.size:second] == 0xA5).all() and (got[second + pixels.size:] == 0xA5).all()


@pytest.mark.parametrize("what,mutate", [
    ("second file over the first", _set("file_offset", 0, row=1)),
    ("second coefficients over the first", _set("coef_offset", 0, row=1)),
    ("second coefficients inside the first", _set("coef_offset", 128, row=1)),
    ("second planes over the first", _set("plane_offset", 0, row=1)),
    ("second output over the first", _set("out_offset", 0, row=1)),
    ("second output inside the first", _set("out_offset", 100, row=1)),
    ("coefficient offset that wraps", _set("coef_offset", (1 << 64) - (1 << 30), row=1)),
    ("first coefficient offset that wraps", _set("coef_offset", (1 << 64) - 1024)),
    ("plane offset that wraps", _set("plane_offset", (1 << 64) - 4096, row=1)),
    ("coefficient offset past the scratch", _set("coef_offset", 1 << 20, row=1)),
    ("file offset that wraps", _set("file_offset", (1 << 64) - 16, row=1)),
    ("output offset that wraps", _set("out_offset", (1 << 64) - 16, row=1)),
    ("second file's intervals over the first's", _set("interval_begin", 0, row=1)),
])
def test_overlapping_and_wrapping_descriptors_precede_device_work(what, mutate):
    rc, clean = _raw_call(mutate, None, copies=2)
    assert rc == -1, what                                             # EGS_ERR_ARG
    assert clean, what


@pytest.mark.parametrize("what,kw,shift,mutate", [
    ("n_files 0", dict(n_files=0), None, None), ("n_intervals 0", dict(n_intervals=0), None, None),
    ("NULL files", dict(files=None), None, None), ("NULL out", dict(out=None), None, None), ("NULL status", dict(status=None), None, None),
    ("NULL scratch", dict(scratch=None), None, None), ("NULL host table", dict(desc_host=None), None, None),
    ("NULL device table", dict(tables_device=None), None, None),
    ("misaligned scratch", {}, dict(scratch=4), None), ("misaligned status", {}, dict(status=2), None),
    ("misaligned device table", {}, dict(desc_device=4), None),
    ("file leaves the buffer", dict(files_bytes=100), None, None), ("output leaves the buffer", dict(out_bytes=100), None, None),
    ("scratch too small", dict(scratch_bytes=4096), None, None),
    ("coefficient offset not aligned", {}, None, _set("coef_offset", 8)), ("plane offset not aligned", {}, None, _set("plane_offset", 4)),
    ("mcus_x disagrees with the width", {}, None, _set("mcus_x", 4)), ("mcus_y disagrees with the height", {}, None, _set("mcus_y", 3)),
    ("n_intervals disagrees with the restart interval", {}, None, _set("n_intervals", 11)),
    ("more intervals than the call has", dict(n_intervals=11), None, None), ("fewer intervals than the call has", dict(n_intervals=13), None, None),
    ("interval_begin", {}, None, _set("interval_begin", 1)),
    ("entropy data leaves the file", {}, None, _set("entropy_bytes", 100000)), ("entropy data begins behind the file", {}, None, _set("entropy_begin", 1 << 20)),
    ("table index 4", {}, None, lambda d, t: d["ta"][0].__setitem__(1, 4)),
    ("zero divisor", {}, None, _table("quant", 0, None, 5, 0)),
    ("over-subscribed table in use", {}, None, _table("ac", 0, "counts", 0, 3)),
    ("DC symbol above 15", {}, None, _table("dc", 0, "values", 0, 16)),
])
def test_argument_errors_precede_device_work(what, kw, shift, mutate):
    rc, clean = _raw_call(mutate, shift, **kw)
    assert rc == -1, what                                             # EGS_ERR_ARG
    assert clean, what


@pytest.mark.parametrize("what,kw,mutate", [
    ("width 0", {}, _set("width", 0)), ("width 32768", {}, _set("width", 32768)), ("height 0", {}, _set("height", 0)),
    ("channels 2", {}, _set("channels", 2)), ("channels 4", {}, _set("channels", 4)), ("n_files 65536", dict(n_files=65536), None),
    ("luma 1x2", {}, lambda d, t: (_set("hs", 1)(d, t), _set("vs", 2)(d, t))), ("luma 4x1", {}, _set("hs", 4)),
    ("restart interval 65536", {}, _set("restart_interval", 65536)), ("restart interval -1", {}, _set("restart_interval", -1)),
    ("output of 2 GiB", {}, lambda d, t: (_set("width", 32767)(d, t), _set("height", 32767)(d, t))),
    ("file of 2 GiB", {}, _set("file_bytes", 1 << 31)),
])
def test_range_errors_precede_device_work(what, kw, mutate):
    rc, clean = _raw_call(mutate, None, **kw)
    assert rc == -3, what                                             # EGS_ERR_RANGE
    assert clean, what


def test_scratch_bytes_is_host_arithmetic():
    from egogaussian_amd import lib
    L = lib.load()
    assert L.egs_jpeg_decode_scratch_bytes(0, 5, 100, 100) == 0 and L.egs_jpeg_decode_scratch_bytes(3, 0, 100, 100) == 0
    assert L.egs_jpeg_decode_scratch_bytes(3, 40, 1000, 300) == 256 + 512 + 1024 + 512
    assert L.egs_jpeg_decode_scratch_bytes(17, 32, 256, 256) == 512 + 256 + 256 + 256


# ---- FrameIngest.put_files: a JPEG image with PNG masks leaves the store put() with the golden pixels leaves ---------------------------------------
SRC_H, SRC_W = 67, 130


def _as_png(a):
    from egogaussian_amd import png
    a = np.asarray(a)
    return png.encode_statement(a if a.ndim == 2 else a.transpose(2, 0, 1))


@pytest.mark.parametrize("target", [(53, 29), (SRC_W, SRC_H)], ids=["130x67-to-53x29", "130x67-kept"])
@pytest.mark.parametrize("layout", ["plain", "gated", "dynamic-motion-gated", "object-loss", "label-gated", "pose-rows"])
def test_put_files_with_a_jpeg_image_leaves_the_store_put_leaves(layout, target):
    """The layouts of tests/test_gpu_png_decode.py's put_files test; the image is the golden 130 x 67 JPEG file, the masks are PNG files."""
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    from egogaussian_amd.scene_synth import make_camera
    from tests.test_gpu_ingest import LAYOUTS
    from tests.test_gpu_png_decode import _sources
    lay = LAYOUTS[layout]
    W, H = target
    jpeg_file, jpeg_pixels = JC.golden()["130x67-420"]
    a, b = FrameStore(H, W, 2, DEV, **lay), FrameStore(H, W, 2, DEV, **lay)
    ing_a, ing_b = FrameIngest(a, (SRC_H, SRC_W)), FrameIngest(b, (SRC_H, SRC_W))
    for i in (1, 0):
        cam, src = make_camera(7 + i, H, W), _sources(lay, seed=100 + i)
        if "image" in src:
            src["image"] = jpeg_pixels
        files = {n: (_as_png(v) if isinstance(v, np.ndarray) else v) for n, v in src.items()}
        if "image" in src:
            files["image"] = jpeg_file
        ing_a.put(i, cam, **src)
        ing_b.put_files(i, cam, **files)
    for name in ("img", "bits", "small"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), (layout, target, name)
    assert (a.img is not None and bool(a.img.any())) or bool(a.bits.any())
    if "image" in src:
        assert ing_b._jpeg_reader.host_reads == 2, "one read of the JPEG status words per frame"
    else:
        assert ing_b._jpeg_reader is None, "the JPEG reader is created by the first JPEG file"


def test_put_files_with_jpeg_masks_too():
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    from egogaussian_amd.scene_synth import make_camera
    H, W = 53, 37
    image, hand = JC.golden()["37x53-420-rb1"], JC.golden()["37x53-L-rr1"]
    cam = make_camera(0, H, W)
    a, b = FrameStore(H, W, 1, DEV, gated=True), FrameStore(H, W, 1, DEV, gated=True)
    FrameIngest(a, (H, W)).put(0, cam, image=image[1], hand_mask=hand[1])
    FrameIngest(b, (H, W)).put_files(0, cam, image=image[0], hand_mask=hand[0])
    assert torch.equal(a.img, b.img) and torch.equal(a.bits, b.bits) and torch.equal(a.small, b.small)


def test_put_files_checks_jpeg_headers_before_device_work():
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    from egogaussian_amd.scene_synth import make_camera
    H, W = 53, 37
    store = FrameStore(H, W, 1, DEV, gated=True)
    ing = FrameIngest(store, (H, W))
    cam = make_camera(0, H, W)
    hand = _as_png(JC.golden()["37x53-L"][1][:, :, 0])
    before = store.img.clone()
    with pytest.raises(ValueError, match="source resolution"):
        ing.put_files(0, cam, image=JC.golden()["17x33-420"][0], hand_mask=hand)
    with pytest.raises(ValueError, match="image has 3"):
        ing.put_files(0, cam, image=JC.golden()["37x53-L"][0], hand_mask=hand)
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_files.npz"))
    with pytest.raises(ValueError, match=r"file 1: jpeg\.parse: SOF2 \(progressive\).*file 1 is image"):
        ing.put_files(0, cam, image=z["16x16-progressive.refused"].tobytes(), hand_mask=hand)
    assert ing._jpeg_reader is None and ing._reader.host_reads == 0, "a header refusal precedes every device decode"
    bad, status = JC.malformed()["bytes left over"]
    with pytest.raises(ValueError, match="file 1 is image"):
        ing.put_files(0, cam, image=bad.replace(b"\x00\x13\x00\x15", b"\x00\x35\x00\x25", 1), hand_mask=hand)      # (its SOF0 says 21 x 19)
    assert torch.equal(store.img, before), "a refused frame changed the store"
