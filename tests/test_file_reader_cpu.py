"""CPU: the host half of the device file reader (egogaussian_amd/file_reader.py) -- load_files, the readers' load() on their classes, the
layout of a batch's one upload -- and egogaussian_amd/csrc/decode_args.h, the argument checks the two C entries share, compiled by the host
compiler with -fsanitize=address,undefined into tests/decode_args_host.cpp and run as a child process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_cases as JC
from tests import png_decode_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _png_golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "png_files.npz"))
    names = sorted(k[:-5] for k in z.files if k.endswith(".file"))[:2]
    return [z[n + ".file"].tobytes() for n in names]


def _same(a, b):
    """Equality through tuples, lists, dicts and arrays."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


# ---- load_files ---------------------------------------------------------------------------------------------------------------------------
def test_load_files_takes_bytes_bytearrays_memoryviews_and_paths(tmp_path):
    from egogaussian_amd.file_reader import load_files
    data = _png_golden()[0]
    path = tmp_path / "a.png"
    path.write_bytes(data)
    seen = []
    blobs, names, parsed = load_files([data, bytearray(data), memoryview(data), path, str(path)], lambda b: seen.append(b) or len(b))
    assert all(bytes(b) == data for b in blobs) and len(blobs) == 5
    assert names == ["file 0", "file 1", "file 2", f"file 3 ({path})", f"file 4 ({path})"]
    assert parsed == [len(data)] * 5 and all(s is b for s, b in zip(seen, blobs))
    assert load_files([], len) == ([], [], [])


def test_load_files_raises_a_refusal_again_under_the_files_name(tmp_path):
    from egogaussian_amd import jpeg, png
    from egogaussian_amd.file_reader import load_files
    good_png, good_jpeg = _png_golden()[0], JC.golden()["31x15-L"][0]
    with pytest.raises(ValueError, match=r"^file 1: png\.parse: no PNG signature$"):
        load_files([good_png, b"\x89PNX" + good_png[4:]], png.parse)
    with pytest.raises(ValueError, match=r"^file 1: jpeg\.parse: no SOI marker$"):
        load_files([good_jpeg, b"\xff\xd9" + good_jpeg[2:]], jpeg.parse)
    with pytest.raises(ValueError, match=r"^file 1: png\.parse: ") as e:
        png.PngReader.load([good_png, good_png[:-1]])
    assert "file 0" not in str(e.value)
    path = tmp_path / "b.jpg"
    path.write_bytes(JC.refusals()["SOF2"][0])
    with pytest.raises(ValueError, match=r"^file 1 \(.*b\.jpg\): jpeg\.parse: SOF2"):
        jpeg.JpegReader.load([good_jpeg, path])


def test_load_on_the_classes_returns_the_parsed_entries_of_each_format():
    """What the readers' load() returned before they shared it: PNG parse(blob) + (len(blob),), JPEG dict(parse(blob), nbytes=len(blob))."""
    from egogaussian_amd import jpeg, png
    files = _png_golden()
    blobs, names, parsed = png.PngReader.load(files)
    assert blobs == files and names == ["file 0", "file 1"]
    assert _same(parsed, [png.parse(b) + (len(b),) for b in files])
    assert [png.PngReader._shape(p) for p in parsed] == [png.parse(b)[:3] for b in files]
    files = [JC.golden()[n][0] for n in ("37x53-420-rb1", "31x15-L")]
    blobs, names, parsed = jpeg.JpegReader.load(files)
    assert blobs == files and names == ["file 0", "file 1"]
    assert _same(parsed, [dict(jpeg.parse(b), nbytes=len(b)) for b in files])
    assert list(parsed[0])[-1] == "nbytes"
    assert [jpeg.JpegReader._shape(p) for p in parsed] == [(37, 53, 3), (31, 15, 1)]


# ---- the staging layout ---------------------------------------------------------------------------------------------------------------------
def _up(v, a):
    return -(-v // a) * a


def _staged_by_hand(desc, second, blobs, total):
    """desc at 0, the second table at the next multiple of 256, the files behind the next multiple of 256 at their file_offset; 0xA5 elsewhere."""
    host = np.full(total, 0xA5, dtype=np.uint8)
    at_second = _up(desc.nbytes, 256)
    at_files = at_second + _up(second.nbytes, 256)
    host[:desc.nbytes] = np.frombuffer(desc.tobytes(), dtype=np.uint8)
    host[at_second:at_second + second.nbytes] = np.frombuffer(second.tobytes(), dtype=np.uint8)
    for d, b in zip(desc, blobs):
        at = at_files + int(d["file_offset"])
        host[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return host, at_second, at_files


def _batches():
    from egogaussian_amd import jpeg, png
    a = sorted(k for k in DC.corpus() if k.startswith("67x5x3-f4"))[0]
    b = sorted(k for k in DC.corpus() if k.startswith("130x3x1-fcycle"))[0]
    files = [DC.corpus()[a][0], DC.corpus()[b][0]]
    p = png.plan(png.PngReader.load(files)[2], 256)
    yield "png", files, p, p["idat"], len(p["idat"]), png.PngReader
    files = [JC.golden()[n][0] for n in ("37x53-420-rb1", "31x15-L")]
    p = jpeg.plan(jpeg.JpegReader.load(files)[2], 256)
    yield "jpeg", files, p, p["tables"], p["n_intervals"], jpeg.JpegReader


def test_the_staged_upload_is_the_stated_layout_and_touches_nothing_between_the_pieces():
    from egogaussian_amd.file_reader import stage, upload_layout
    for what, files, p, second, count, cls in _batches():
        desc = p["desc"]
        at_second, at_files = upload_layout(desc, second)
        up_bytes = at_files + p["files_bytes"]
        want, want_second, want_files = _staged_by_hand(desc, second, files, up_bytes + 512)
        assert (at_second, at_files) == (want_second, want_files), what
        assert at_second % 256 == 0 and at_files % 256 == 0 and desc.nbytes <= at_second < desc.nbytes + 256, what
        assert int(desc["file_offset"][0]) == 0 and int(desc["file_offset"][1]) == _up(len(files[0]), 16), what
        host = np.full(up_bytes + 512, 0xA5, dtype=np.uint8)
        stage(host, desc, second, files)
        assert np.array_equal(host, want), what
        used = np.zeros(host.size, dtype=bool)                         # the pieces; every other byte still holds 0xA5
        used[:desc.nbytes] = True
        used[at_second:at_second + second.nbytes] = True
        for d, b in zip(desc, files):
            used[at_files + int(d["file_offset"]):at_files + int(d["file_offset"]) + len(b)] = True
        assert (host[~used] == 0xA5).all() and (~used).sum() >= 512, what
        assert host[at_files:at_files + len(files[0])].tobytes() == files[0], what
        # the reader's hooks hand the loop these very pieces
        rd = cls.__new__(cls)
        rd.flags = 0
        got_second, got_count = rd._second_table(p)
        assert got_second is second and got_count == count, what


# ---- decode_args.h under the sanitizers --------------------------------------------------------------------------------------------------------
def test_the_shared_argument_checks_decide_as_the_entries_lines_did(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the test needs a host C++ compiler"
    exe = str(tmp_path / "decode_args_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "decode_args_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, f"the sanitized program: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.strip().endswith(", 0 failures"), r.stdout[-3000:]
