"""Files for the segmented route of the PNG decoder (tests/test_png_segments_cpu.py, tests/test_gpu_png_segments.py): seeded, built once,
left unchanged.  Each case states what it expects: the route word (1, or 0 | reason << 8 with the reasons of csrc/png_segments.h) and the
status word of the serial route, which stands whatever the route.

The files are built from tests/png_decode_cases.py's BitWriter and block writers, from png.encode_statement and from stdlib zlib; a file
is a list of IDAT payloads, so that empty chunks and any cut can be stated."""
import functools
import struct
import zlib

import numpy as np

from tests import png_cases as PC
from tests import png_decode_cases as DC

SEGMENT_MAX = 8192                                                    # include/egs_raster.h EGS_PNG_SEGMENT_MAX
SEGMENTS = 1
(HEADER_SPLIT, BLOCK_END, DISTANCE, CAP, TRAILER, SUM, ADLER, INFLATE, CRC) = (r << 8 for r in range(1, 10))
REASONS = {HEADER_SPLIT: "header split", BLOCK_END: "chunk does not end on a block end", DISTANCE: "distance before the segment", CAP: "segment over the cap",
           TRAILER: "final block or trailer placement", SUM: "length sum", ADLER: "Adler-32", INFLATE: "inflate error inside a segment", CRC: "IDAT CRC"}
HEADER = b"\x78\x9c"
FINAL = b"\x01\x00\x00\xff\xff"                                       # the empty final stored block, the shape the device encoder ends with


def file_of(W, H, C, pieces):
    """A PNG file whose IDAT chunks carry `pieces` (bytes each, empty ones too)."""
    out = [DC.SIGNATURE, DC.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0))]
    return b"".join(out + [DC.chunk(b"IDAT", bytes(p)) for p in pieces] + [DC.chunk(b"IEND", b"")])


def adler(raw):
    return struct.pack(">I", zlib.adler32(bytes(raw)) & 0xFFFFFFFF)


def segment(data, kind):
    """One independent segment of `data` ending on a byte boundary: 'stored'; 'fixed' / 'dynamic' (literals, then the empty stored block of a
    full flush); 'mixed' (a stored, a fixed and a dynamic block, then the flush); or a token list for a fixed block."""
    bw = DC.BitWriter()
    data = bytes(data or b"")
    if kind == "stored":
        DC.stored_block(bw, data)
        return bytes(bw.out)
    if kind == "fixed":
        DC.fixed_block(bw, list(data))
    elif kind == "dynamic":
        DC.dynamic_block(bw, list(data))
    elif kind == "mixed":
        a, b = len(data) // 3, 2 * len(data) // 3
        DC.stored_block(bw, data[:a])
        DC.fixed_block(bw, list(data[a:b]))
        DC.dynamic_block(bw, list(data[b:]))
    else:
        DC.fixed_block(bw, kind)
    DC.stored_block(bw, b"")
    return bytes(bw.out)


def rows_of(img, mode="own"):
    return DC.filtered(img, mode).tobytes()


def by_lengths(raw, lengths, kinds=("stored", "fixed", "dynamic")):
    """Segments of the given byte counts over `raw`, the block kinds in rotation."""
    assert sum(lengths) == len(raw)
    at, out = 0, []
    for i, n in enumerate(lengths):
        out.append(segment(raw[at:at + n], kinds[i % len(kinds)]))
        at += n
    return out


def by_rows(raw, H, kind):
    rb = len(raw) // H
    return [segment(raw[y * rb:(y + 1) * rb], kind) for y in range(H)]


def zlib_rows(raw, H, flush):
    """One raw-deflate compressor over the rows, flushed with `flush` behind every row -> one piece per row."""
    z, rb = zlib.compressobj(6, zlib.DEFLATED, -15), len(raw) // H
    return [z.compress(raw[y * rb:(y + 1) * rb]) + z.flush(flush) for y in range(H)]


def _grey(seed, H, W):
    return PC._arbitrary(seed, 1, H, W)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (file bytes, image uint8 [C,H,W] or None when the file is refused, route word, status word)."""
    from egogaussian_amd import png
    out = {}

    def add(name, img, pieces, route, status=DC.OK, size=None):
        C, H, W = img.shape
        w, h = size or (W, H)
        out[name] = (file_of(w, h, C, pieces), img if status == DC.OK else None, route, status)

    # segments of 0, 1, 2, 3 and 5 bytes: starts at 0, 1, 3, 4, 4, 7, 12, 14, 17 (every residue mod 4); bytes 0, 1-2 and 3 are three segments in one
    # 32-bit word, the middle one strictly inside it
    tiny = _grey(11, 2, 10)
    raw = rows_of(tiny)
    lengths = [1, 2, 1, 0, 3, 5, 2, 3, 5]
    assert sum(lengths) == 22 == len(raw)
    for shift, kinds in enumerate([("stored", "fixed", "dynamic"), ("fixed", "dynamic", "stored"), ("dynamic", "stored", "fixed")]):
        add(f"tiny-{shift}", tiny, [HEADER] + by_lengths(raw, lengths, kinds) + [FINAL + adler(raw)], SEGMENTS)
    add("tiny-header-with-blocks", tiny, [HEADER + b"".join(by_lengths(raw, lengths)[:2])] + by_lengths(raw, lengths)[2:] + [FINAL + adler(raw)], SEGMENTS)

    # stored, fixed and dynamic blocks in one file, several blocks per segment, empty chunks between the segments
    img = PC.cases()["67x5x3"]
    raw = rows_of(img)
    mixed = by_rows(raw, 5, "mixed")
    add("mixed-blocks", img, [HEADER] + mixed + [FINAL + adler(raw)], SEGMENTS)
    add("empty-chunks", img, [HEADER, b""] + [p for s in mixed for p in (s, b"", b"")] + [FINAL + adler(raw), b"", b""], SEGMENTS)
    add("empty-chunk-first", img, [b"", HEADER] + mixed + [FINAL + adler(raw)], HEADER_SPLIT)
    add("header-split", img, [HEADER[:1], HEADER[1:]] + mixed + [FINAL + adler(raw)], HEADER_SPLIT)
    add("adler-in-its-own-chunk", img, [HEADER] + mixed + [FINAL, adler(raw)], TRAILER)
    add("final-block-not-last", img, [HEADER] + mixed[:2] + [FINAL + adler(raw)] + mixed[2:], TRAILER, DC.ADLER)
    add("chunk-behind-the-final-block", img, [HEADER] + mixed + [FINAL + adler(raw), b"\x00"], TRAILER, DC.BEHIND)
    add("no-final-block", img, [HEADER] + mixed, TRAILER, DC.TRUNCATED)
    add("cut-inside-a-block", img, [HEADER, mixed[0][:40], mixed[0][40:]] + mixed[1:] + [FINAL + adler(raw)], BLOCK_END)
    add("wrong-adler", img, [HEADER] + mixed + [FINAL + adler(raw + b"x")], ADLER, DC.ADLER)
    add("a-row-too-many", img, [HEADER] + mixed + [FINAL + adler(raw)], SUM, DC.TOO_MANY, size=(67, 4))
    add("a-row-too-few", img, [HEADER] + mixed + [FINAL + adler(raw)], SUM, DC.TOO_FEW, size=(67, 6))
    add("block-type-3", img, [HEADER] + mixed[:3] + [b"\x06"] + mixed[3:] + [FINAL + adler(raw)], INFLATE, DC.BLOCK_TYPE)
    add("zlib-header", img, [b"\x77\x9c"] + mixed + [FINAL + adler(raw)], INFLATE, DC.ZLIB_HEADER)
    f = bytearray(file_of(67, 5, 3, [HEADER] + mixed + [FINAL + adler(raw)]))
    at = -1
    for _ in range(3):                                                # the third IDAT chunk: the CRC behind its payload
        at = f.index(b"IDAT", at + 1)
    f[at + 4 + len(mixed[1])] ^= 0x10
    out["bad-chunk-crc"] = (bytes(f), None, CRC, DC.IDAT_CRC | (2 << 8))

    # zlib's own shapes: a full flush per row is segmentable (header and first blocks share chunk 0); a sync flush keeps the window, and rows
    # that repeat are matches into the segment before
    rep = np.ascontiguousarray(np.broadcast_to(_grey(12, 1, 40), (1, 6, 40)))
    raw = rows_of(rep, 0)
    for name, flush, route in (("zlib-full-flush", zlib.Z_FULL_FLUSH, SEGMENTS), ("zlib-sync-flush", zlib.Z_SYNC_FLUSH, DISTANCE)):
        pieces = zlib_rows(raw, 6, flush)
        add(name, rep, [HEADER + pieces[0]] + pieces[1:] + [FINAL + adler(raw)], route)
    for k in (1, 2, 3):
        add(f"statement-rows{k}", img, _idat(png.encode_statement(img, segment_rows=k)), SEGMENTS)

    # a distance of exactly the bytes the segment has produced, and one more (the byte before the segment: the serial route's to accept)
    edge = _grey(13, 4, 15).copy()
    r = bytearray(rows_of(edge, 0))
    r[19], r[20], r[21] = r[15], 0, r[17]                              # bytes 19 .. 21 repeat bytes 15 .. 17 (the last byte of row 0, row 1's filter byte, ...)
    r[24:32] = r[16:24]                                               # and the second half of row 1 its first
    edge = DC._grey_from_raw(bytes(r), 15)
    raw = bytes(r)
    rows = by_rows(raw, 4, "fixed")
    at_produced = segment(None, list(raw[16:24]) + [(8, 8)])
    one_before = segment(None, list(raw[16:19]) + [(3, 4)] + list(raw[22:32]))
    add("distance-equals-produced", edge, [HEADER, rows[0], at_produced] + rows[2:] + [FINAL + adler(raw)], SEGMENTS)
    add("distance-one-before-the-segment", edge, [HEADER, rows[0], one_before] + rows[2:] + [FINAL + adler(raw)], DISTANCE)

    # the cap: rows of exactly SEGMENT_MAX bytes, and of one more
    for name, W, route in (("segment-at-the-cap", SEGMENT_MAX - 1, SEGMENTS), ("segment-over-the-cap", SEGMENT_MAX, CAP)):
        big = _grey(14, 2, W)
        raw = rows_of(big)
        add(name, big, [HEADER] + zlib_rows(raw, 2, zlib.Z_FULL_FLUSH) + [FINAL + adler(raw)], route)

    # sizes, in the device encoder's segmentation (png.encode_statement, one row or one 4096-byte piece per segment)
    sizes = {n: PC.cases()[n] for n in ("1x1x1", "1x1x3", "1x7x1", "7x1x3", "67x5x3", "130x3x1")}
    sizes["300x70x3"] = PC._arbitrary(15, 3, 70, 300)
    sizes["1400x3x3"] = PC._arbitrary(16, 3, 3, 1400)
    for n, im in sizes.items():
        add("size-" + n, im, _idat(png.encode_statement(im)), SEGMENTS)
    for v in out.values():
        if v[1] is not None:
            v[1].setflags(write=False)
    return out


def _idat(data):
    from egogaussian_amd import png
    return [data[o:o + n] for o, n in png.parse(data)[3]]


def size_images():
    """The images of the size cases: what the device encoder is given in the GPU test."""
    return {k[5:]: v[1] for k, v in cases().items() if k.startswith("size-")}


def chunk_table(data):
    """A file -> (expect, [(length, CRC flag)], stream): what the host program reads."""
    from egogaussian_amd import png
    W, H, C, idat = png.parse(data)
    table = []
    for o, n in idat:
        stored = struct.unpack(">I", data[o + n:o + n + 4])[0]
        table.append((n, int(stored != (zlib.crc32(data[o - 4:o + n]) & 0xFFFFFFFF))))
    return H * (1 + W * C), table, b"".join(data[o:o + n] for o, n in idat)
