"""GPU: the PNG decoder (csrc/png_decode.hip, csrc/png_inflate.h; egogaussian_amd/png.py PngReader / decode_device) over the corpus of
tests/png_decode_cases.py -- every stream kind, filter, chunking and hand-assembled edge, whose paths tests/test_png_decode_cpu.py asserts
and whose every file the sanitized host build of the same inflater has read first.  PNG is lossless: a file decodes to exactly its image, the
status word is 0, and nothing outside a file's own slots is written (guard bytes around every buffer and between the output slots)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import png_cases as PC
from tests import png_decode_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hwc(img):
    return np.ascontiguousarray(img.transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def _corpus_decoded():
    """The whole corpus through one reader whose batch is smaller than the corpus: grey and RGB files of every size share batches."""
    from egogaussian_amd import png
    names = list(DC.corpus())
    rd = png.PngReader(DEV, batch=64, guard=256)
    outs = rd.read([DC.corpus()[n][0] for n in names])
    got = {n: o.cpu().numpy() for n, o in zip(names, outs)}
    return got, rd.check_guards(), rd.host_reads, list(rd.last_status)


def test_every_corpus_file_decodes_to_its_image():
    got, guards, reads, status = _corpus_decoded()
    assert status == [0] * len(got)
    assert reads == -(-len(got) // 64) and reads > 1, "one read of the status words per batch"
    bad = [n for n, a in got.items() if not np.array_equal(a, _hwc(DC.corpus()[n][1]))]
    assert not bad, bad
    assert guards, "bytes outside a slot, the scratch or the status words were written"


def test_batches_of_one_and_decode_device():
    from egogaussian_amd import png
    rd = png.PngReader(DEV, batch=1, guard=256)
    names = ["67x5x3-fcycle-", "hand-dist32768", "1x1x1-f0-"]
    for stem in names:
        n = sorted(k for k in DC.corpus() if k.startswith(stem))[0]
        data, img, _ = DC.corpus()[n]
        out = rd.read([data])
        assert len(out) == 1 and out[0].dtype == torch.uint8 and out[0].is_cuda and tuple(out[0].shape) == _hwc(img).shape
        assert np.array_equal(out[0].cpu().numpy(), _hwc(img)) and rd.check_guards()
        assert np.array_equal(png.decode_device(data, DEV).cpu().numpy(), _hwc(img))
    assert rd.read([]) == []
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.PngReader("cpu")


def test_files_by_path(tmp_path):
    from egogaussian_amd import png
    n = sorted(k for k in DC.corpus() if k.startswith("130x3x3-fown"))[0]
    p = tmp_path / "a.png"
    p.write_bytes(DC.corpus()[n][0])
    out = png.PngReader(DEV).read([p, DC.corpus()[n][0]])
    assert np.array_equal(out[0].cpu().numpy(), _hwc(DC.corpus()[n][1])) and torch.equal(out[0], out[1])


def test_files_of_the_device_encoder_decode_back():
    from egogaussian_amd import png
    files, imgs = [], []
    for name, x in PC.cases().items():
        buf, sizes = png.encode(torch.from_numpy(x.copy()).to(DEV)[None])
        files.append(buf[0, :int(sizes[0])].cpu().numpy().tobytes())
        imgs.append(x)
    rd = png.PngReader(DEV, batch=32, guard=256)
    outs = rd.read(files)
    for name, o, x in zip(PC.cases(), outs, imgs):
        assert np.array_equal(o.cpu().numpy(), _hwc(x)), name
    assert rd.check_guards()


def test_golden_pillow_files_decode_to_their_pixels():
    from egogaussian_amd import png
    z = np.load(os.path.join(ROOT, "tests", "golden", "png_files.npz"))
    names = sorted(k[:-5] for k in z.files if k.endswith(".file"))
    assert len(names) == 12
    outs = png.PngReader(DEV).read([z[n + ".file"].tobytes() for n in names])
    for n, o in zip(names, outs):
        assert np.array_equal(o.cpu().numpy(), z[n + ".pixels"]), n


@pytest.mark.parametrize("name", list(DC.malformed()))
def test_malformed_file_gives_its_status_and_harms_nothing_else(name):
    from egogaussian_amd import png
    data, status, _, _ = DC.malformed()[name]
    a = sorted(k for k in DC.corpus() if k.startswith("67x5x3-f4"))[0]
    b = sorted(k for k in DC.corpus() if k.startswith("130x3x1-fcycle"))[0]
    rd = png.PngReader(DEV, batch=4, guard=256)
    with pytest.raises(ValueError, match=r"file 1: .*\(status %d\)" % status) as e:
        rd.read([DC.corpus()[a][0], data, DC.corpus()[b][0]])
    assert "file 0" not in str(e.value) and "file 2" not in str(e.value)
    assert rd.last_status == [0, status, 0]
    assert png.status_text(status) in str(e.value)
    assert np.array_equal(rd.last_results[0].cpu().numpy(), _hwc(DC.corpus()[a][1]))
    assert np.array_equal(rd.last_results[2].cpu().numpy(), _hwc(DC.corpus()[b][1]))
    assert rd.check_guards()


def _raw_call(mutate=None, shift=None, copies=1, **override):
    """`copies` of one small file through the C entry with buffers preset to 0xA5; `mutate(desc, idat)` edits the host tables first, `shift` moves the
    named default pointers by that many bytes, the other keywords replace arguments.  -> (return code, True when no device buffer changed)."""
    from egogaussian_amd import lib, png, _hip
    L = lib.load()
    n = sorted(k for k in DC.corpus() if k.startswith("67x5x3-f4"))[0]
    data = DC.corpus()[n][0]
    p = png.plan([png.parse(data) + (len(data),)] * copies)
    desc, idat = p["desc"].copy(), p["idat"].copy()
    if mutate:
        mutate(desc, idat)
    override.setdefault("n_files", copies)
    bufs = {k: torch.full((65536,), 0xA5, dtype=torch.uint8, device=DEV) for k in ("files", "tables", "out", "status", "scratch")}
    args = dict(n_files=1, files=bufs["files"].data_ptr(), files_bytes=65536, desc_host=desc.ctypes.data, desc_device=bufs["tables"].data_ptr(),
                idat_host=idat.ctypes.data, idat_device=bufs["tables"].data_ptr() + 1024, n_idat=len(idat), out=bufs["out"].data_ptr(),
                out_bytes=8192, status=bufs["status"].data_ptr(), scratch=bufs["scratch"].data_ptr(), scratch_bytes=32768)
    for k, v in (shift or {}).items():
        args[k] += v
    args.update(override)
    order = ("n_files", "files", "files_bytes", "desc_host", "desc_device", "idat_host", "idat_device", "n_idat", "out", "out_bytes", "status",
             "scratch", "scratch_bytes")
    with _hip.device_ctx(torch.device(DEV)):
        rc = L.egs_png_decode(*[args[k] for k in order], _hip.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, all(bool((bufs[k] == 0xA5).all()) for k in ("out", "status", "scratch"))


def _set(field, value, table="desc", row=0):
    def f(desc, idat):
        (desc if table == "desc" else idat)[field][row] = value
    return f


def test_the_two_file_call_the_overlap_cases_start_from_decodes():
    """The unmodified two-file tables, with the files and the device copy of the tables uploaded as the contract asks: accepted, both
    decoded, nothing else written.  (The error cases below differ from this call by one field of the host tables.)"""
    from egogaussian_amd import lib, png, _hip
    L = lib.load()
    n = sorted(k for k in DC.corpus() if k.startswith("67x5x3-f4"))[0]
    data, img, _ = DC.corpus()[n]
    p = png.plan([png.parse(data) + (len(data),)] * 2)
    desc, idat = p["desc"], p["idat"]
    host = np.full(65536, 0xA5, dtype=np.uint8)
    host[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    host[1024:1024 + idat.nbytes] = idat.view(np.uint8).reshape(-1)
    assert 1024 + idat.nbytes <= 8192
    for d in desc:
        at = 8192 + int(d["file_offset"])
        host[at:at + len(data)] = np.frombuffer(data, dtype=np.uint8)
    blob = torch.from_numpy(host).to(DEV)
    out, status, scratch = (torch.full((k,), 0xA5, dtype=torch.uint8, device=DEV) for k in (8192, 256, 32768))
    need = L.egs_png_decode_scratch_bytes(len(idat), p["stream_bytes"], p["inflate_bytes"])
    assert need <= 32768 and p["out_bytes"] <= 8192 and 8192 + p["files_bytes"] <= 65536
    with _hip.device_ctx(torch.device(DEV)):
        rc = L.egs_png_decode(2, blob.data_ptr() + 8192, p["files_bytes"], desc.ctypes.data, blob.data_ptr(), idat.ctypes.data,
                              blob.data_ptr() + 1024, len(idat), out.data_ptr(), 8192, status.data_ptr(), scratch.data_ptr(), 32768,
                              _hip.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    assert status[:8].view(torch.int32).tolist() == [0, 0] and bool((status[8:] == 0xA5).all()) and bool((scratch[need:] == 0xA5).all())
    got = out.cpu().numpy()
    for d in desc:
        o = int(d["out_offset"])
        assert np.array_equal(got[o:o + img.size].reshape(img.shape[1], img.shape[2], 3), _hwc(img))
    assert (got[img.size:int(desc[1]["out_offset"])] == 0xA5).all() and (got[int(desc[1]["out_offset"]) + img.size:] == 0xA5).all()


@pytest.mark.parametrize("what,mutate", [
    ("second file over the first", _set("file_offset", 0, row=1)),
    ("second stream over the first", _set("stream_offset", 0, row=1)),
    ("second stream inside the first", _set("stream_offset", 16, row=1)),
    ("second inflated data over the first", _set("inflate_offset", 0, row=1)),
    ("second output over the first", _set("out_offset", 0, row=1)),
    ("second output inside the first", _set("out_offset", 100, row=1)),
    ("stream offset that wraps", _set("stream_offset", (1 << 64) - (1 << 30), row=1)),
    ("first stream offset that wraps", _set("stream_offset", (1 << 64) - 1024)),
    ("inflate offset that wraps", _set("inflate_offset", (1 << 64) - 4096, row=1)),
    ("stream offset past the scratch", _set("stream_offset", 1 << 20, row=1)),
    ("file offset that wraps", _set("file_offset", (1 << 64) - 16, row=1)),
    ("output offset that wraps", _set("out_offset", (1 << 64) - 16, row=1)),
])
def test_overlapping_and_wrapping_descriptors_precede_device_work(what, mutate):
    rc, clean = _raw_call(mutate, None, copies=2)
    assert rc == -1, what                                             # EGS_ERR_ARG
    assert clean, what


@pytest.mark.parametrize("what,kw,shift,mutate", [
    ("n_files 0", dict(n_files=0), None, None), ("n_idat 0", dict(n_idat=0), None, None),
    ("NULL files", dict(files=None), None, None), ("NULL out", dict(out=None), None, None), ("NULL status", dict(status=None), None, None),
    ("NULL scratch", dict(scratch=None), None, None), ("NULL host table", dict(desc_host=None), None, None),
    ("NULL device table", dict(idat_device=None), None, None),
    ("misaligned scratch", {}, dict(scratch=4), None), ("misaligned status", {}, dict(status=2), None),
    ("file leaves the buffer", dict(files_bytes=100), None, None), ("output leaves the buffer", dict(out_bytes=100), None, None),
    ("scratch too small", dict(scratch_bytes=512), None, None),
    ("stream offset not aligned", {}, None, _set("stream_offset", 8)), ("chunk leaves the file", {}, None, _set("length", 4000, "idat")),
    ("chunks do not tile the stream", {}, None, _set("dst", 3, "idat")), ("chunk of another file", {}, None, _set("file", 1, "idat")),
    ("idat_begin", {}, None, _set("idat_begin", 1)),
])
def test_argument_errors_precede_device_work(what, kw, shift, mutate):
    rc, clean = _raw_call(mutate, shift, **kw)
    assert rc == -1, what                                             # EGS_ERR_ARG
    assert clean, what


@pytest.mark.parametrize("what,kw,mutate", [
    ("width 0", {}, _set("width", 0)), ("width 32768", {}, _set("width", 32768)), ("height 0", {}, _set("height", 0)),
    ("channels 2", {}, _set("channels", 2)), ("channels 4", {}, _set("channels", 4)), ("n_files 65536", dict(n_files=65536), None),
    ("output of 2 GiB", {}, lambda d, i: (_set("width", 32767)(d, i), _set("height", 32767)(d, i))),
    ("stream of 2 GiB", {}, _set("stream_bytes", 1 << 31)),
])
def test_range_errors_precede_device_work(what, kw, mutate):
    rc, clean = _raw_call(mutate, None, **kw)
    assert rc == -3, what                                             # EGS_ERR_RANGE
    assert clean, what


def test_scratch_bytes_is_host_arithmetic():
    from egogaussian_amd import lib
    L = lib.load()
    assert L.egs_png_decode_scratch_bytes(0, 100, 100) == 0
    assert L.egs_png_decode_scratch_bytes(3, 100, 1000) == 256 + 256 + 1024


# ---- FrameIngest.put_files: the same store as put() with the arrays ---------------------------------------------------------------------------
def _as_png(a):
    """uint8 [h,w], [h,w,1] or [h,w,3] -> file bytes by the host statement (png.encode_statement)."""
    from egogaussian_amd import png
    a = np.asarray(a)
    return png.encode_statement(a if a.ndim == 2 else a.transpose(2, 0, 1))


SRC_H, SRC_W = 67, 130


def _sources(lay, seed):
    """-> (cam maker arguments, FrameIngest.put keywords): seeded 130 x 67 source arrays for what the layout holds."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    src = {}
    if not lay.get("label_phase"):
        yy, xx = np.mgrid[0:SRC_H, 0:SRC_W]
        src["image"] = (np.stack([3 * xx + yy, 2 * yy + 40, xx + 2 * yy], -1) + rng.integers(0, 32, (SRC_H, SRC_W, 3))).astype(np.uint8)
    if lay.get("gated"):
        src["hand_mask"] = (rng.random((SRC_H, SRC_W)) < 0.3).astype(np.uint8) * 255
    if lay.get("object_loss") or lay.get("label_phase"):
        src["obj_mask"] = np.repeat(((rng.random((SRC_H, SRC_W, 1)) < 0.5) * 255).astype(np.uint8), 3, axis=2)      # an RGB mask file
    if lay.get("dynamic"):
        src["accum_R"] = torch.rand(3, 3, generator=g)
    if lay.get("motion"):
        src["accum_T"] = torch.rand(4, 4, generator=g)
    if lay.get("pose_rows"):
        src["pose_rows"] = (1, 2, 1)
    return src


@pytest.mark.parametrize("target", [(53, 29), (SRC_W, SRC_H)], ids=["130x67-to-53x29", "130x67-kept"])
@pytest.mark.parametrize("layout", ["plain", "gated", "dynamic-motion-gated", "object-loss", "label-gated", "pose-rows"])
def test_put_files_leaves_the_store_put_leaves(layout, target):
    """The layouts of tests/test_gpu_ingest.py; a 130 x 67 source resized down, and one kept at size."""
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    from egogaussian_amd.scene_synth import make_camera
    from tests.test_gpu_ingest import LAYOUTS
    lay = LAYOUTS[layout]
    W, H = target
    a, b = FrameStore(H, W, 2, DEV, **lay), FrameStore(H, W, 2, DEV, **lay)
    ing_a, ing_b = FrameIngest(a, (SRC_H, SRC_W)), FrameIngest(b, (SRC_H, SRC_W))
    for i in (1, 0):
        cam, src = make_camera(7 + i, H, W), _sources(lay, seed=100 + i)
        files = {n: (_as_png(v) if isinstance(v, np.ndarray) else v) for n, v in src.items()}
        ing_a.put(i, cam, **src)
        ing_b.put_files(i, cam, **files)
    for name in ("img", "bits", "small"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), (layout, target, name)
    assert (a.img is not None and bool(a.img.any())) or bool(a.bits.any())
    assert getattr(ing_b, "_reader").host_reads == 2, "one read of the status words per frame"


def test_put_files_checks_before_device_work(tmp_path):
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    from egogaussian_amd.scene_synth import make_camera
    H, W = 20, 30
    store = FrameStore(H, W, 1, DEV, gated=True)
    ing = FrameIngest(store, (H, W))
    rng = np.random.default_rng(3)
    img, hand = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (rng.random((H, W)) < 0.3).astype(np.uint8) * 255
    cam = make_camera(0, H, W)
    before = store.img.clone()
    with pytest.raises(ValueError, match="source resolution"):
        ing.put_files(0, cam, image=_as_png(img[:, :-1]), hand_mask=_as_png(hand))
    with pytest.raises(ValueError, match="image has 3"):
        ing.put_files(0, cam, image=_as_png(hand), hand_mask=_as_png(hand))
    with pytest.raises(ValueError, match="signature.*file 0 is hand_mask"):
        ing.put_files(0, cam, image=_as_png(img), hand_mask=b"JFIF")
    bad = bytearray(_as_png(hand))
    bad[-20] ^= 1                                                     # inside the last IDAT chunk: its CRC, or the Adler-32 it carries
    with pytest.raises(ValueError, match="file 0 is hand_mask"):
        ing.put_files(0, cam, image=_as_png(img), hand_mask=bytes(bad))
    assert getattr(ing, "_reader", None) is not None and torch.equal(store.img, before), "a refused frame changed the store"
    p = tmp_path / "hand.png"
    p.write_bytes(_as_png(hand))
    ing.put_files(0, cam, image=_as_png(img), hand_mask=p)             # a path and bytes
    ref = FrameStore(H, W, 1, DEV, gated=True)
    FrameIngest(ref, (H, W)).put(0, cam, image=img, hand_mask=hand)
    assert torch.equal(store.img, ref.img) and torch.equal(store.bits, ref.bits) and torch.equal(store.small, ref.small)


# ---- evaluate.metrics_from_files: the figures of the files an evaluation sweep wrote ----------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_files(tmp_path_factory):
    from egogaussian_amd import png
    from egogaussian_amd.evaluate import EvalPass
    from egogaussian_amd.losses import quantize8
    from tests.test_gpu_eval_pass import _scene, _model, H, W
    from tests.test_gpu_lpips import _net
    s, F = _scene(), 3
    d = str(tmp_path_factory.mktemp("png_metrics"))
    paths = {n: [os.path.join(d, f"{n}_{k}.png") for k in range(F)] for n in ("render", "gt", "hand")}
    ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1, keep_images=True, lpips=_net())
    res = ev.run(s["frames"][:F], s["cams"][0], save_renders=paths["render"])
    gts = torch.stack([quantize8(s["gts"][k]) for k in range(F)]).to(torch.uint8)
    png.PngWriter(H, W, 3, DEV).save(gts, paths["gt"])
    hands = torch.stack([(s["keeps"][k] * 255).to(torch.uint8) for k in range(F)])
    png.PngWriter(H, W, 1, DEV).save(hands, paths["hand"])
    return res, paths


def test_metrics_from_files_equal_the_sweeps_rows(sweep_files):
    from egogaussian_amd.evaluate import metrics_from_files
    from tests.test_gpu_lpips import _net
    res, paths = sweep_files
    got = metrics_from_files(paths["render"], paths["gt"], paths["hand"], lpips=_net(), device=DEV)
    assert np.array_equal(got["sse"], res["sse"]) and (got["sse"] > 0).all()
    assert got["ssim"].tobytes() == res["ssim"].tobytes()             # ssim = ssim_sum / n with the same n: the sums are the same bits
    assert got["psnr"].tobytes() == res["psnr"].tobytes()
    assert got["lpips_taps"].tobytes() == res["lpips_taps"].tobytes() and got["lpips"].tobytes() == res["lpips"].tobytes()
    assert got["means"] == (res["mean_ssim"], res["mean_psnr"], res["mean_lpips"])
    assert got["rows"][1] == (float(res["ssim"][1]), float(res["psnr"][1]), float(res["lpips"][1]))
    plain = metrics_from_files(paths["render"], paths["gt"], [open(p, "rb").read() for p in paths["hand"]], device=DEV)
    assert "lpips" not in plain and len(plain["means"]) == 2 and plain["ssim"].tobytes() == res["ssim"].tobytes()


def test_metrics_from_files_refuses_a_grey_hand_mask_and_uneven_lists(sweep_files):
    from egogaussian_amd import png
    from egogaussian_amd.evaluate import metrics_from_files
    res, paths = sweep_files
    hand = png.decode(open(paths["hand"][1], "rb").read()).copy()
    hand[5, 7] = 128
    with pytest.raises(ValueError, match=r"hand mask\(s\) \[1\].*binary"):
        metrics_from_files(paths["render"], paths["gt"], [paths["hand"][0], png.encode_statement(hand), paths["hand"][2]], device=DEV)
    with pytest.raises(ValueError, match="one of each"):
        metrics_from_files(paths["render"], paths["gt"][:2], paths["hand"], device=DEV)
