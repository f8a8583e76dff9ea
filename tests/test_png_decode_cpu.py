"""CPU: the PNG decoder's host side -- png.parse and its refusals, the corpus of tests/png_decode_cases.py and the paths it must reach, and
the inflater itself: egogaussian_amd/csrc/png_inflate.h, the header the device kernel includes, compiled by the host compiler with
-fsanitize=address,undefined into tests/png_inflate_host.cpp and run as a child process over the corpus, the malformed corpus, every
truncation of the short streams and a seeded set of mutations.  Verdict and bytes must equal zlib's."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_decode_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITER_SLACK = 8                                                        # csrc/png_inflate.h PNGI_ITER_SLACK


# ---- png.parse ------------------------------------------------------------------------------------------------------------------------------
def _file(**kw):
    raw = bytes(4 * (1 + 5))
    return DC.make_file(5, 4, 1, zlib.compress(raw), **kw)


def _ihdr(W=5, H=4, depth=8, colour=0, comp=0, filt=0, lace=0, size=13):
    body = struct.pack(">IIBBBBB", W, H, depth, colour, comp, filt, lace)[:size] + bytes(max(0, size - 13))
    return DC.SIGNATURE + DC.chunk(b"IHDR", body) + DC.chunk(b"IDAT", zlib.compress(bytes(24))) + DC.chunk(b"IEND", b"")


def test_parse_returns_the_size_and_the_idat_table():
    from egogaussian_amd import png
    for name, (data, img, stream) in DC.corpus().items():
        W, H, C, idat = png.parse(data)
        assert (C, H, W) == img.shape, name
        assert b"".join(data[o:o + n] for o, n in idat) == stream, name
        for o, n in idat:
            assert data[o - 4:o] == b"IDAT" and struct.unpack(">I", data[o - 8:o - 4])[0] == n
    short = [k for k, v in DC.corpus().items() if len(v[2]) <= 100 and not k.endswith("-bytes")]
    assert len(short) > 50, "few short streams"
    for k in short:                                                   # every file of at most 100 stream bytes also exists in 1-byte IDAT chunks
        W, H, C, idat = png.parse(DC.corpus()[k + "-bytes"][0])
        assert len(idat) == len(DC.corpus()[k][2]) and all(n == 1 for _, n in idat), k


@pytest.mark.parametrize("name,data,match", [
    ("signature", b"\x89PNX" + _file()[4:], "signature"),
    ("empty", b"", "signature"),
    ("truncated header", _file()[:8 + 25 + 6], "truncated"),
    ("chunk past the end", _file()[:-14], "past the end"),
    ("behind IEND", _file() + b"\x00", "behind IEND"),
    ("no IEND", _file()[:-12], "IEND"),
    ("IHDR not first", DC.SIGNATURE + DC.ANCILLARY[0] + _file()[8:], "IHDR"),
    ("IHDR twice", _file()[:33] + _file()[8:], "IHDR"),
    ("IHDR of 14 bytes", _ihdr(size=14), "13 bytes"),
    ("IHDR CRC", _file()[:30] + b"\x00" + _file()[31:], "CRC"),
    ("IEND CRC", _file()[:-1] + b"\x00", "CRC"),
    ("IEND with data", _file()[:-12] + DC.chunk(b"IEND", b"x"), "IEND"),
    ("no IDAT", DC.SIGNATURE + DC.chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 4, 8, 0, 0, 0, 0)) + DC.chunk(b"IEND", b""), "IDAT"),
    ("IDAT not consecutive", _file()[:-12] + DC.ANCILLARY[0] + DC.chunk(b"IDAT", b"") + DC.chunk(b"IEND", b""), "consecutive"),
    ("unknown critical chunk", _file(before=[DC.chunk(b"ABCD", b"")]), "critical"),
    ("PLTE CRC", _file(before=[DC.chunk(b"PLTE", bytes(6))[:-1] + b"\x00"]), "CRC"),
    ("zero width", _ihdr(W=0), "width"),
    ("zero height", _ihdr(H=0), "height"),
    ("side of 32768", _ihdr(W=32768), "width"),
    ("bit depth 16", _ihdr(depth=16), "bit depth"),
    ("bit depth 1", _ihdr(depth=1), "bit depth"),
    ("palette", _ihdr(colour=3), "colour type"),
    ("grey alpha", _ihdr(colour=4), "colour type"),
    ("RGBA", _ihdr(colour=6), "colour type"),
    ("compression method", _ihdr(comp=1), "compression"),
    ("filter method", _ihdr(filt=1), "filter method"),
    ("interlace", _ihdr(lace=1), "interlace"),
])
def test_parse_refuses(name, data, match):
    from egogaussian_amd import png
    with pytest.raises(ValueError, match=match):
        png.parse(data)


def test_parse_refusals_of_modes_carry_the_advice_of_ingest():
    from egogaussian_amd import png, ingest
    for data in (_ihdr(depth=16), _ihdr(colour=3), _ihdr(colour=6), _ihdr(lace=1)):
        with pytest.raises(ValueError) as e:
            png.parse(data)
        assert ingest._ADVICE in str(e.value)


def test_a_valid_plte_in_an_rgb_file_is_walked_over():
    from egogaussian_amd import png
    data = DC.make_file(2, 2, 3, zlib.compress(bytes(2 * 7)), before=[DC.chunk(b"PLTE", bytes(6))])
    assert png.parse(data)[:3] == (2, 2, 3)


# ---- the corpus reaches its paths ------------------------------------------------------------------------------------------------------------
def test_corpus_reaches_every_path():
    corpus = DC.corpus()
    tot = dict(kinds=set(), max_lit=0, max_dist_code=0, max_match=0, max_dist=0, dist1=False, lone=False, none=False, stored=set(), multi=False)
    dist_at_least_32507 = False
    for name, (data, img, stream) in corpus.items():
        d = DC.describe(stream)
        assert d["out"] == DC.expected_raw(name), name                # the plain-loop inflater agrees with zlib
        C, H, W = img.shape
        rows = np.frombuffer(d["out"], dtype=np.uint8).reshape(H, 1 + W * C)
        from tests.png_cases import unfilter_reference
        if img.size <= 4096:
            assert np.array_equal(unfilter_reference(rows, W, C).reshape(H, W, C).transpose(2, 0, 1), img), name
        tot["kinds"] |= d["kinds"]
        tot["max_lit"] = max(tot["max_lit"], d["max_lit_code"])
        tot["max_dist_code"] = max(tot["max_dist_code"], d["max_dist_code"])
        tot["max_match"] = max(tot["max_match"], d["max_match"])
        tot["max_dist"] = max(tot["max_dist"], d["max_dist"])
        dist_at_least_32507 |= d["max_dist"] >= 32507
        tot["dist1"] |= d["dist1_overlap"]
        tot["lone"] |= d["lone_dist"]
        tot["none"] |= d["no_dist"]
        tot["stored"] |= d["stored_lens"]
        tot["multi"] |= d["blocks"] > 1
        if name == "hand-header_across_idat":
            first = data.index(b"IDAT") + 4
            n0 = struct.unpack(">I", data[first - 8:first - 4])[0]
            start = d["block_starts"][1]
            assert start < 8 * n0 < start + 17, "the cut is not inside the second block's header"
    print({k: (sorted(v) if isinstance(v, set) and len(v) < 9 else (len(v) if isinstance(v, set) else v)) for k, v in tot.items()}, len(corpus), "files")
    assert tot["kinds"] == {0, 1, 2}
    assert tot["max_lit"] == 15
    assert tot["max_match"] == 258
    assert tot["dist1"]
    assert dist_at_least_32507 and tot["max_dist"] == 32768
    assert tot["lone"] and tot["none"]
    assert 0 in tot["stored"] and 65535 in tot["stored"]
    assert tot["multi"]
    assert DC.describe(corpus["hand-lone_distance_code"][2])["lone_dist"] and DC.describe(corpus["hand-no_distance_code"][2])["no_dist"]
    assert DC.describe(corpus["fibonacci-huff"][2])["max_lit_code"] == 15
    print("fibonacci at zlib's default strategy: longest code", DC.describe(corpus["fibonacci-l6"][2])["max_lit_code"])      # (matches thin the counts: reported, not held)


def test_malformed_streams_are_refused_by_the_arbiter():
    codes = set()
    for name, (data, status, stream, expect) in DC.malformed().items():
        codes.add(status & 255)
        if stream is not None:
            assert DC.arbiter(stream, expect) is None, name
    assert codes == set(range(1, 16)), "one file per status code"


# ---- the header under the sanitizers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("png_inflate") / "png_inflate_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "png_inflate_host.cpp"), "-o", exe])
    return exe


def _run(host, tmp_path, records):
    """records: [(stream, expect)] -> [(status, produced, iterations, bytes or None)]."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        for stream, expect in records:
            fh.write(struct.pack("<II", len(stream), expect) + bytes(stream))
    r = subprocess.run([host, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, f"the sanitized program: exit {r.returncode}\n{r.stderr[-3000:]}"
    blob, pos, out = open(dst, "rb").read(), 0, []
    for stream, expect in records:
        status, produced, iters = struct.unpack("<IIQ", blob[pos:pos + 16])
        pos += 16
        data = None
        if status == 0:
            data = blob[pos:pos + expect]
            pos += expect
        out.append((status, produced, iters, data))
    assert pos == len(blob)
    return out


def _hold(records, results, what):
    """Verdict and bytes equal zlib's; the loop count stays inside the bound the header derives: 8 n + PNGI_ITER_SLACK."""
    worst = 0.0
    for (stream, expect), (status, produced, iters, data) in zip(records, results):
        want = DC.arbiter(stream, expect)
        assert (status == 0) == (want is not None), f"{what}: status {status}, zlib {'accepts' if want is not None else 'refuses'} ({len(stream)} bytes)"
        if want is not None:
            assert data == want and produced == expect, what
        assert iters <= 8 * len(stream) + ITER_SLACK, (what, iters, len(stream))
        worst = max(worst, iters / (8 * len(stream) + ITER_SLACK))
    return worst


def test_header_over_the_corpus(host, tmp_path):
    recs = [(s, len(DC.expected_raw(k))) for k, (f, img, s) in DC.corpus().items()]
    res = _run(host, tmp_path, recs)
    assert all(r[0] == 0 for r in res), [k for k, r in zip(DC.corpus(), res) if r[0]]
    print("iterations / bound, worst:", _hold(recs, res, "corpus"))


def test_header_over_the_malformed_corpus(host, tmp_path):
    items = [(k, v) for k, v in DC.malformed().items() if v[2] is not None]
    recs = [(v[2], v[3]) for k, v in items]
    res = _run(host, tmp_path, recs)
    _hold(recs, res, "malformed")
    for (k, v), r in zip(items, res):
        assert r[0] == v[1], f"{k}: status {r[0]}, expected {v[1]}"


def _short_streams():
    seen, out = set(), []
    for k, (f, img, s) in DC.corpus().items():
        if len(s) <= 300 and s not in seen:
            seen.add(s)
            out.append((k, s, len(DC.expected_raw(k))))
    return out


def test_header_over_every_truncation(host, tmp_path):
    short = _short_streams()
    recs = [(s[:n], e) for k, s, e in short for n in range(len(s))]
    assert len(recs) > 1000
    res = _run(host, tmp_path, recs)
    _hold(recs, res, "truncation")
    assert all(r[0] == DC.TRUNCATED for r in res), sorted(set(r[0] for r in res))
    print(len(recs), "truncations of", len(short), "streams")


def test_header_over_mutations(host, tmp_path):
    """2 000 single-bit and single-byte changes spread over five small streams (stored, fixed, dynamic, hand-assembled)."""
    corpus = DC.corpus()
    names = ["67x5x1-fown-l0-c", "67x5x1-fown-fixed-c", "67x5x3-f4-l6-c", "hand-lone_distance_code", "hand-header_across_idat"]
    picked = []
    for stem in names:
        k = sorted(n for n in corpus if n.startswith(stem))
        assert k, stem
        picked.append(k[0])
    rng = np.random.default_rng(2024)
    recs = []
    for i in range(2000):
        k = picked[i % 5]
        s = bytearray(corpus[k][2])
        at = int(rng.integers(0, len(s)))
        if i % 2:
            s[at] ^= 1 << int(rng.integers(0, 8))
        else:
            s[at] = (s[at] + int(rng.integers(1, 256))) & 255
        recs.append((bytes(s), len(DC.expected_raw(k))))
    res = _run(host, tmp_path, recs)
    _hold(recs, res, "mutation")
    kinds = {}
    for r in res:
        kinds[r[0]] = kinds.get(r[0], 0) + 1
    print("statuses over the mutations:", dict(sorted(kinds.items())))
    assert len(kinds) >= 8, "the mutations reach few checks"
