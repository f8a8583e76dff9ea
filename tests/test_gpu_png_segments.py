"""GPU: the segmented route of the PNG decoder (csrc/png_decode.hip k_pngd_measure / scan / place, csrc/png_segments.h;
png.PngReader(segments=), egs_png_decode_ex) over the cases of
tests/png_segments_cases.py -- each states its route word and its status -- and the corpus of tests/png_decode_cases.py.  The route
only ever accepts: pixels and status words are the serial route's for every file, and the route word says which wave inflated it.  The
sanitized host build of the same header has run the same files first (tests/test_png_segments_cpu.py)."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from tests import png_cases as PC
from tests import png_decode_cases as DC
from tests import png_segments_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hwc(img):
    return np.ascontiguousarray(img.transpose(1, 2, 0))


def _height_files():
    """Heights around the unfilter's 64-row block, filters cycling and forced: files of many rows that no case above has."""
    out = {}
    for k, (H, W, C, mode) in enumerate([(1, 5, 3, 4), (63, 64, 1, "cycle"), (64, 65, 3, "cycle"), (65, 200, 3, 3), (129, 63, 1, 4), (129, 130, 3, "cycle"),
                                         (65, 5, 1, 2), (64, 129, 1, 1)]):
        img = PC._arbitrary(40 + k, C, H, W)
        out[f"h{H}-w{W}-c{C}-f{mode}"] = (DC.make_file(W, H, C, zlib.compress(DC.filtered(img, mode).tobytes(), 6)), img)
    return out


@functools.lru_cache(maxsize=None)
def _files():
    """name -> (file bytes, image or None, stated route or None, stated status or None): the new cases, the corpus, the malformed corpus, the heights."""
    out = {"case-" + k: v for k, v in SC.cases().items()}
    out.update({"corpus-" + k: (f, img, None, 0) for k, (f, img, s) in DC.corpus().items()})
    out.update({"malformed-" + k: (v[0], None, None, v[1]) for k, v in DC.malformed().items()})
    out.update({"height-" + k: (f, img, None, 0) for k, (f, img) in _height_files().items()})
    return out


@functools.lru_cache(maxsize=None)
def _decoded(segments):
    """Every file through one reader in batches of 64 -> (name -> pixels, statuses, routes, guards intact, reads of the status words)."""
    from egogaussian_amd import png
    names = list(_files())
    rd = png.PngReader(DEV, batch=64, guard=256, segments=segments)
    with pytest.raises(ValueError):
        rd.read([_files()[n][0] for n in names])
    got = {n: o.cpu().numpy() for n, o in zip(names, rd.last_results)}
    return got, dict(zip(names, rd.last_status)), dict(zip(names, rd.last_route)), rd.check_guards(), rd.host_reads


def test_every_file_decodes_as_the_serial_route_does_and_takes_its_stated_route():
    from egogaussian_amd import png
    got, status, route, guards, reads = _decoded(True)
    ref, ref_status, ref_route, ref_guards, _ = _decoded(False)
    assert guards and ref_guards, "bytes outside a slot, the scratch, the status or the route words were written"
    assert reads == -(-len(got) // 64), "one read of the status and route words per batch"
    assert set(ref_route.values()) == {0}
    for n, (data, img, want_route, want_status) in _files().items():
        assert status[n] == ref_status[n], (n, status[n], ref_status[n])
        if want_status is not None:
            assert status[n] == want_status, (n, status[n], want_status)
        if want_route is not None:
            assert route[n] == want_route, f"{n}: {png.route_text(route[n])}, stated {png.route_text(want_route)}"
        assert route[n] == SC.SEGMENTS or route[n] in SC.REASONS, (n, route[n])
        if status[n] == 0:
            want = _hwc(png.decode(data).reshape(img.shape)) if img.size <= 70000 and n.startswith("case-") else _hwc(img)
            assert np.array_equal(want, _hwc(img)), n
            assert np.array_equal(got[n], want), n
            assert np.array_equal(ref[n], want), n
    taken = sum(1 for r in route.values() if r == SC.SEGMENTS)
    print(taken, "of", len(route), "files took the segmented route")
    assert {r for n, r in route.items() if n.startswith("case-")} == {SC.SEGMENTS} | set(SC.REASONS)


def test_files_of_the_device_encoder_take_the_segmented_route():
    from egogaussian_amd import png
    files, imgs = [], []
    for name, x in SC.size_images().items():
        buf, sizes = png.encode(torch.from_numpy(x.copy()).to(DEV)[None])
        files.append(buf[0, :int(sizes[0])].cpu().numpy().tobytes())
        imgs.append(x)
    assert {tuple(x.shape) for x in imgs} >= {(1, 1, 1), (1, 7, 1), (3, 1, 7), (3, 5, 67), (1, 3, 130), (3, 70, 300), (3, 3, 1400)}
    rd = png.PngReader(DEV, batch=32, guard=256, segments=True)
    outs = rd.read(files)
    assert rd.last_route == [SC.SEGMENTS] * len(files) and rd.last_status == [0] * len(files)
    for o, x in zip(outs, imgs):
        assert np.array_equal(o.cpu().numpy(), _hwc(x)), x.shape
    assert rd.check_guards()
    assert np.array_equal(png.decode_device(files[-1], DEV, segments=True).cpu().numpy(), _hwc(imgs[-1]))


def test_a_mixed_batch_routes_and_fails_file_by_file():
    from egogaussian_amd import png
    c, corpus = SC.cases(), DC.corpus()
    serial = "hand-header_across_idat"                                  # a block header across two chunks: never segments
    names = ["size-300x70x3", serial, "wrong-adler", "tiny-0", "bad-chunk-crc", "zlib-sync-flush", "mixed-blocks"]
    files = [corpus[n][0] if n == serial else c[n][0] for n in names]
    rd = png.PngReader(DEV, batch=8, guard=256, segments=True)
    with pytest.raises(ValueError, match=r"file 2: .*\(status 13\); file 4: .*\(status 513\)") as e:
        rd.read(files)
    assert "file 0" not in str(e.value) and "file 6" not in str(e.value)
    assert rd.last_status == [0, 0, DC.ADLER, 0, DC.IDAT_CRC | (2 << 8), 0, 0]
    assert rd.last_route[0] == rd.last_route[3] == rd.last_route[6] == SC.SEGMENTS
    assert rd.last_route[2] == SC.ADLER and rd.last_route[4] == SC.CRC and rd.last_route[5] == SC.DISTANCE
    assert rd.last_route[1] != SC.SEGMENTS and rd.last_route[1] in SC.REASONS
    for k, n in enumerate(names):
        img = corpus[n][1] if n == serial else c[n][1]
        if img is not None:
            assert np.array_equal(rd.last_results[k].cpu().numpy(), _hwc(img)), n
    assert rd.check_guards()
    assert png.route_text(rd.last_route[0]) == "segments" and "Adler" in png.route_text(rd.last_route[2])


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------------
class _Call:
    """Files uploaded with their tables as the contract asks, every buffer preset to 0xA5; run(entry, ...) enqueues one call."""

    def __init__(self, files, flags=0, scratch_flags=None):
        from egogaussian_amd import lib, png
        self.L = lib.load()
        self.p = p = png.plan([png.parse(f) + (len(f),) for f in files])
        self.n, self.n_idat = len(files), len(p["idat"])
        self.t_idat = 4096
        self.t_files = self.t_idat + (p["idat"].nbytes + 255) // 256 * 256
        assert p["desc"].nbytes <= 4096
        self.host = torch.full((self.t_files + p["files_bytes"] + 256,), 0xA5, dtype=torch.uint8).pin_memory()
        self.fill(files)
        self.blob = torch.empty(self.host.numel(), dtype=torch.uint8, device=DEV)
        self.need = int(self.L.egs_png_decode_scratch_bytes_ex(self.n_idat, p["stream_bytes"], p["inflate_bytes"], flags if scratch_flags is None else scratch_flags))
        self.out = torch.full((p["out_bytes"] + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        self.status = torch.full((256 + 8 * self.n,), 0xA5, dtype=torch.uint8, device=DEV)
        self.scratch = torch.full((self.need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        self.flags = flags

    def fill(self, files):
        h, p = self.host.numpy(), self.p
        h[:p["desc"].nbytes] = p["desc"].view(np.uint8).reshape(-1)
        h[self.t_idat:self.t_idat + p["idat"].nbytes] = p["idat"].view(np.uint8).reshape(-1)
        for d, f in zip(p["desc"], files):
            at = self.t_files + int(d["file_offset"])
            assert len(f) == int(d["file_bytes"])
            h[at:at + len(f)] = np.frombuffer(f, dtype=np.uint8)

    def upload(self):
        self.blob.copy_(self.host, non_blocking=True)

    def args(self):
        p = self.p
        return [self.n, self.blob.data_ptr() + self.t_files, p["files_bytes"], p["desc"].ctypes.data, self.blob.data_ptr(), p["idat"].ctypes.data,
                self.blob.data_ptr() + self.t_idat, self.n_idat, self.out.data_ptr(), p["out_bytes"], self.status.data_ptr(), self.scratch.data_ptr(), self.need]

    def run(self, ex=True, flags=None, route=True, route_shift=0, phases=7):
        from egogaussian_amd import _hip
        dev = torch.device(DEV)
        flags = self.flags if flags is None else flags
        with _hip.device_ctx(dev):
            if ex:
                return self.L.egs_png_decode_ex(*self.args(), _hip.stream_of(dev), phases, flags,
                                                self.status.data_ptr() + 4 * self.n + route_shift if route else None)
            return self.L.egs_png_decode(*self.args(), _hip.stream_of(dev))

    def words(self):
        w = self.status[:8 * self.n].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        return w[:self.n].tolist(), w[self.n:].tolist()

    def clean(self):
        return all(bool((t == 0xA5).all()) for t in (self.out, self.status, self.scratch))


def _entry_files():
    c = SC.cases()
    serial = "hand-header_across_idat"
    return [c["size-67x5x3"][0], DC.corpus()[serial][0], c["wrong-adler"][0], c["tiny-1"][0]]


def test_flags_zero_is_the_old_entry_byte_for_byte():
    files = _entry_files()
    a, b = _Call(files), _Call(files)
    a.upload(); b.upload()
    assert a.need == int(a.L.egs_png_decode_scratch_bytes(a.n_idat, a.p["stream_bytes"], a.p["inflate_bytes"]))
    assert a.run(ex=False) == 0 and b.run(ex=True, flags=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(a.status, b.status), "status words, and the route words flags = 0 must not touch"
    assert a.words()[0] == [0, 0, DC.ADLER, 0] and bool((a.status[4 * a.n:] == 0xA5).all())
    ok = torch.ones_like(a.out, dtype=torch.bool)
    d = a.p["desc"][2]
    ok[int(d["out_offset"]):int(d["out_offset"]) + int(d["width"]) * int(d["height"]) * int(d["channels"])] = False      # a failed file's own slot is unspecified
    assert torch.equal(a.out[ok], b.out[ok])
    assert torch.equal(a.scratch, b.scratch), "flag words, streams and inflated data"


def test_the_new_entry_decodes_and_writes_nothing_else():
    c = _Call(_entry_files(), flags=1)
    c.upload()
    assert c.run() == 0
    torch.cuda.synchronize()
    status, route = c.words()
    assert status == [0, 0, DC.ADLER, 0] and route[0] == route[3] == SC.SEGMENTS and route[2] == SC.ADLER and route[1] in SC.REASONS
    assert bool((c.status[8 * c.n:] == 0xA5).all()) and bool((c.scratch[c.need:] == 0xA5).all()) and bool((c.out[c.p["out_bytes"]:] == 0xA5).all())
    img = SC.cases()["size-67x5x3"][1]
    assert np.array_equal(c.out[:img.size].cpu().numpy().reshape(5, 67, 3), _hwc(img))
    again = _Call(_entry_files(), flags=1)
    again.upload()
    assert again.run(route=False) == 0                                # route may be NULL
    torch.cuda.synchronize()
    assert again.words()[0] == status and bool((again.status[4 * again.n:] == 0xA5).all())


@pytest.mark.parametrize("what,kw,scratch_flags", [
    ("a flag that is not defined", dict(flags=2), None), ("another", dict(flags=5), None), ("a negative flags word", dict(flags=-1), None),
    ("scratch sized without the records", dict(flags=1), 0), ("a misaligned route", dict(flags=1, route_shift=2), None),
    ("phases 0", dict(flags=1, phases=0), None), ("phases 8", dict(flags=1, phases=8), None),
])
def test_argument_errors_of_the_new_entry_precede_device_work(what, kw, scratch_flags):
    c = _Call(_entry_files(), flags=1, scratch_flags=scratch_flags)
    c.upload()
    assert c.run(**kw) == -1, what                                    # EGS_ERR_ARG
    torch.cuda.synchronize()
    assert c.clean(), what


def test_scratch_bytes_ex_is_host_arithmetic():
    from egogaussian_amd import lib
    L = lib.load()
    assert L.egs_png_decode_scratch_bytes_ex(3, 100, 1000, 0) == L.egs_png_decode_scratch_bytes(3, 100, 1000) == 256 + 256 + 1024
    assert L.egs_png_decode_scratch_bytes_ex(3, 100, 1000, 1) == 256 + 256 + 1024 + 256 + 256
    assert L.egs_png_decode_scratch_bytes_ex(17, 100, 1000, 1) == 256 + 256 + 1024 + 512 + 256
    assert L.egs_png_decode_scratch_bytes_ex(0, 100, 1000, 1) == 0 and L.egs_png_decode_scratch_bytes_ex(3, 100, 1000, 2) == 0


def test_captured_call_replays_on_new_file_bytes_of_the_same_plan():
    """One egs_png_decode_ex call, captured on a single stream; the replays read new file bytes through the same tables.  The route is
    decided on the device at every replay: the third file set carries a wrong Adler-32 and falls back to the serial wave's status 13."""
    imgs = [PC._arbitrary(60 + k, 3, 5, 67) for k in range(2)]

    def stored(img, spoil=False):
        raw = SC.rows_of(img)
        return SC.file_of(67, 5, 3, [SC.HEADER] + SC.by_rows(raw, 5, "stored") + [SC.FINAL + SC.adler(raw + (b"x" if spoil else b""))])

    sets = [[stored(imgs[0]), SC.cases()["tiny-0"][0]], [stored(imgs[1]), SC.cases()["tiny-0"][0]], [stored(imgs[1], True), SC.cases()["tiny-0"][0]]]
    assert len({tuple(len(f) for f in s) for s in sets}) == 1
    c = _Call(sets[0], flags=1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.upload()
        assert c.run() == 0                                           # warm: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        assert c.run() == 0
    tiny = SC.cases()["tiny-0"][1]
    o1 = int(c.p["desc"][1]["out_offset"])
    for k, files in enumerate(sets):
        c.fill(files)
        c.upload()
        c.out.fill_(0xA5); c.status.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        status, route = c.words()
        if k < 2:
            assert status == [0, 0] and route == [SC.SEGMENTS, SC.SEGMENTS], (k, status, route)
            assert np.array_equal(c.out[:imgs[k].size].cpu().numpy().reshape(5, 67, 3), _hwc(imgs[k])), k
        else:
            assert status == [DC.ADLER, 0] and route == [SC.ADLER, SC.SEGMENTS], (status, route)
        assert np.array_equal(c.out[o1:o1 + tiny.size].cpu().numpy().reshape(2, 10, 1), _hwc(tiny)), k
        assert bool((c.scratch[c.need:] == 0xA5).all()) and bool((c.status[8 * c.n:] == 0xA5).all())


# ---- the callers ------------------------------------------------------------------------------------------------------------------------------
def test_put_files_with_segments_leaves_the_same_store():
    from egogaussian_amd import png
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    from egogaussian_amd.scene_synth import make_camera
    from tests.test_gpu_ingest import LAYOUTS
    from tests.test_gpu_png_decode import _sources, _as_png, SRC_H, SRC_W
    lay = LAYOUTS["object-loss"]                                      # the layout with both masks
    assert lay.get("gated") and lay.get("object_loss")
    H, W = 29, 53
    a, b = FrameStore(H, W, 2, DEV, **lay), FrameStore(H, W, 2, DEV, **lay)
    ing_a, ing_b = FrameIngest(a, (SRC_H, SRC_W)), FrameIngest(b, (SRC_H, SRC_W))
    for i in (1, 0):
        cam, src = make_camera(7 + i, H, W), _sources(lay, seed=200 + i)
        assert {"image", "hand_mask", "obj_mask"} <= set(src)
        files = {n: (_as_png(v) if isinstance(v, np.ndarray) else v) for n, v in src.items()}
        ing_a.put_files(i, cam, **files)
        assert ing_a._reader.last_route == [0, 0, 0]
        ing_b.put_files(i, cam, segments=True, **files)
        assert ing_b._reader.last_route == [png.ROUTE_SEGMENTS] * 3
    for name in ("img", "bits", "small"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), name
    assert bool(a.img.any()) and ing_b._reader.host_reads == 2


def test_metrics_from_files_with_segments_returns_the_same_rows(tmp_path):
    from egogaussian_amd import png
    from egogaussian_amd.evaluate import metrics_from_files
    rng = np.random.default_rng(8)
    H, W, F = 40, 56, 3
    gts = rng.integers(0, 256, (F, 3, H, W), dtype=np.uint8)
    renders = np.clip(gts.astype(np.int64) + rng.integers(-9, 10, gts.shape), 0, 255).astype(np.uint8)
    hands = ((rng.random((F, H, W)) < 0.8) * 255).astype(np.uint8)
    paths = {n: [str(tmp_path / f"{n}_{k}.png") for k in range(F)] for n in ("render", "gt", "hand")}
    png.PngWriter(H, W, 3, DEV).save(torch.from_numpy(renders).to(DEV), paths["render"])
    png.PngWriter(H, W, 3, DEV).save(torch.from_numpy(gts).to(DEV), paths["gt"])
    png.PngWriter(H, W, 1, DEV).save(torch.from_numpy(hands).to(DEV), paths["hand"])
    ref = metrics_from_files(paths["render"], paths["gt"], paths["hand"], device=DEV)
    got = metrics_from_files(paths["render"], paths["gt"], paths["hand"], device=DEV, segments=True)
    assert got["rows"] == ref["rows"] and got["means"] == ref["means"] and (ref["sse"] > 0).all()
    for n in ("sse", "ssim_sum", "ssim", "psnr"):
        assert got[n].tobytes() == ref[n].tobytes(), n
