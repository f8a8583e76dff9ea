"""CPU: the segmented route of the PNG decoder -- egogaussian_amd/csrc/png_segments.h, the header the device kernels include, compiled by
the host compiler with -fsanitize=address,undefined into tests/png_segments_host.cpp and run as a child process.  The program emulates the
measure, scan and placement passes chunk by chunk and the serial inflater next to them, over the cases of tests/png_segments_cases.py, the
corpus and the malformed corpus of tests/png_decode_cases.py in their chunkings, every truncation of the short streams and seeded mutations.
One property everywhere: a file the route accepts is one pngi_inflate -- and zlib -- accepts, with identical bytes and Adler-32."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import png_decode_cases as DC
from tests import png_segments_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("png_segments") / "png_segments_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "png_segments_host.cpp"), "-o", exe])
    return exe


def _run(host, tmp_path, records):
    """records: [(expect, [(length, CRC flag)], stream)] -> [(route, serial status, bytes or None)].  The program itself refuses (exit 1) an
    accepted file that pngi_inflate does not accept with the same bytes and Adler-32."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        for expect, table, stream in records:
            assert sum(n for n, _ in table) == len(stream)
            fh.write(struct.pack("<II", expect, len(table)) + b"".join(struct.pack("<II", n, c) for n, c in table) + bytes(stream))
    r = subprocess.run([host, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and not r.stderr, f"the sanitized program: exit {r.returncode}\n{r.stderr[-3000:]}"
    blob, pos, out = open(dst, "rb").read(), 0, []
    for expect, table, stream in records:
        route, status = struct.unpack("<II", blob[pos:pos + 8])
        pos += 8
        data = None
        if route == SC.SEGMENTS:
            data = blob[pos:pos + expect]
            pos += expect
        out.append((route, status, data))
    assert pos == len(blob)
    return out


def _hold(records, results, what):
    """Never accepts what zlib refuses; accepted bytes are zlib's; the serial verdict is zlib's whatever the route.  -> the route words seen."""
    seen = {}
    for i, ((expect, table, stream), (route, status, data)) in enumerate(zip(records, results)):
        want = None if any(c for _, c in table) else DC.arbiter(stream, expect)
        if route == SC.SEGMENTS:
            assert want is not None and data == want and status == 0, f"{what} {i}: accepted what zlib refuses, or other bytes"
        else:
            assert route in SC.REASONS, (what, i, route)
        if not any(c for _, c in table):
            assert (status == 0) == (want is not None), (what, i, status)
        seen[route] = seen.get(route, 0) + 1
    return seen


def _cuts(stream, step):
    edges = list(range(0, len(stream), step)) + [len(stream)] if len(stream) else [0, 0]
    return [(b - a, 0) for a, b in zip(edges[:-1], edges[1:])]


def test_new_cases_take_their_stated_route(host, tmp_path):
    cases = SC.cases()
    recs = [SC.chunk_table(v[0]) for v in cases.values()]
    res = _run(host, tmp_path, recs)
    seen = _hold(recs, res, "cases")
    for (name, (data, img, route, status)), (got, serial, _) in zip(cases.items(), res):
        assert got == route, f"{name}: route {got:#x}, stated {route:#x}"
        if (status & 255) != DC.IDAT_CRC:                             # (the CRC word is the device's: the host program inflates whatever the flags say)
            assert serial == status, f"{name}: serial status {serial}, stated {status}"
        assert (img is not None) == (status == 0)
    print({(k if k == 1 else SC.REASONS[k]): v for k, v in sorted(seen.items())})
    assert set(seen) == {SC.SEGMENTS} | set(SC.REASONS), "every reason code is reached, and the route itself"


def test_new_cases_reach_the_placement_edges():
    """What the tiny cases are for: segment starts on all four residues mod 4, three segments in one 32-bit word, one strictly inside it."""
    expect, table, stream = SC.chunk_table(SC.cases()["tiny-0"][0])
    d = DC.describe(stream)
    assert d["kinds"] == {0, 1, 2} and len(d["out"]) == expect == 22
    lengths = [1, 2, 1, 0, 3, 5, 2, 3, 5]
    starts = [sum(lengths[:k]) for k in range(len(lengths))]
    assert {s % 4 for s in starts} == {0, 1, 2, 3}
    assert sorted(set(lengths)) == [0, 1, 2, 3, 5]
    in_word0 = [k for k, (s, n) in enumerate(zip(starts, lengths)) if n and s < 4]
    assert len(in_word0) == 3 and starts[1] > 0 and starts[1] + lengths[1] < 4
    two = SC.chunk_table(SC.cases()["size-1400x3x3"][0])[1]
    assert len(two) == 2 * 3 + 1, "a row over 4096 stream bytes is two pieces (the header shares chunk 0; the final block has its own)"


def test_route_over_the_corpus_in_its_chunkings(host, tmp_path):
    corpus = DC.corpus()
    recs = [SC.chunk_table(f) for f, img, s in corpus.values()]
    res = _run(host, tmp_path, recs)
    seen = _hold(recs, res, "corpus")
    assert all(r[1] == 0 for r in res)
    print({(k if k == 1 else SC.REASONS[k]): v for k, v in sorted(seen.items())}, len(recs), "files")
    assert seen.get(SC.SEGMENTS, 0) > 0, "single-block files in one chunk are segments too"


def test_route_over_the_malformed_corpus(host, tmp_path):
    items = list(DC.malformed().items())
    recs = [SC.chunk_table(v[0]) for k, v in items]
    res = _run(host, tmp_path, recs)
    _hold(recs, res, "malformed")
    for (k, v), (route, status, _), rec in zip(items, res, recs):
        if v[1] == DC.FILTER:                                         # (a good stream: the filter byte is the unfilter pass's to refuse)
            continue
        assert route != SC.SEGMENTS, k
        if v[2] is not None:
            assert status == v[1], k


def test_route_over_every_truncation(host, tmp_path):
    seen_streams, recs = set(), []
    for k, (f, img, s) in DC.corpus().items():
        if len(s) <= 300 and s not in seen_streams:
            seen_streams.add(s)
            e = len(DC.expected_raw(k))
            recs += [(e, _cuts(s[:n], 7 if n % 2 else 1 << 20), s[:n]) for n in range(len(s))]
    for name in ("tiny-0", "tiny-1", "tiny-2", "distance-equals-produced", "zlib-full-flush"):      # segmentable files: the chunk table stays, its end is cut
        expect, table, s = SC.chunk_table(SC.cases()[name][0])
        for n in range(len(s)):
            left, cut = n, []
            for length, _ in table:
                cut.append((min(length, left), 0))
                left -= cut[-1][0]
            recs.append((expect, cut, s[:n]))
    assert len(recs) > 1000
    res = _run(host, tmp_path, recs)
    _hold(recs, res, "truncation")
    assert all(r[0] != SC.SEGMENTS and r[1] == DC.TRUNCATED for r in res)
    print(len(recs), "truncations")


def test_route_over_mutations(host, tmp_path):
    """4 000 single-bit and single-byte changes: over five segmentable files, whose chunk tables stay, and over five streams of the corpus."""
    rng = np.random.default_rng(2025)
    picked = [SC.chunk_table(SC.cases()[n][0]) for n in ("tiny-0", "mixed-blocks", "zlib-full-flush", "statement-rows1", "distance-equals-produced")]
    corpus = DC.corpus()
    for stem in ("67x5x1-fown-l0-c", "67x5x1-fown-fixed-c", "67x5x3-f4-l6-c", "hand-lone_distance_code", "hand-header_across_idat"):
        k = sorted(n for n in corpus if n.startswith(stem))[0]
        picked.append(SC.chunk_table(corpus[k][0]))
    recs = []
    for i in range(4000):
        expect, table, stream = picked[i % 10]
        s = bytearray(stream)
        at = int(rng.integers(0, len(s)))
        if i % 2:
            s[at] ^= 1 << int(rng.integers(0, 8))
        else:
            s[at] = (s[at] + int(rng.integers(1, 256))) & 255
        recs.append((expect, table, bytes(s)))
    res = _run(host, tmp_path, recs)
    seen = _hold(recs, res, "mutation")
    print({(k if k == 1 else SC.REASONS[k]): v for k, v in sorted(seen.items())})
    assert len(seen) >= 5, "the mutations reach few rules"
