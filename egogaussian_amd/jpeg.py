"""Baseline JPEG files read on the device: the mirror of the read half of png.py.

    parse        the host's share, O(marker segments): SOI .. the SOS header; no entropy-coded byte is touched
    decode       the strict host reader, integer numpy / Python written from the standard and libjpeg's documented arithmetic: the STATEMENT
                 the kernels answer to (csrc/jpeg_decode.hip), status words included.  Not a call into any library.
    plan         the descriptor and table arrays of egs_jpeg_decode for a batch
    JpegReader   file bytes -> device uint8 [h, w, C]; DeviceFileReader's contract (file_reader.py)

The arithmetic, in the order decode() applies it (libjpeg-turbo's default path, which Pillow uses: tests/golden/jpeg_files.npz):
  Huffman decode with the DC predictors reset at every restart; dequantise; the `islow` inverse DCT (CONST_BITS 13, PASS1_BITS 2: column
  pass descaled by 11 into a workspace, row pass descaled by 18, + 128, SATURATING clamp to 0 .. 255); chroma planes cropped to
  ceil(W h / hmax) x ceil(H v / vmax) and upsampled by the triangle filter with replicated edges (a plane of one or two columns is
  replicated instead, as libjpeg does); fixed-point YCbCr -> RGB.

The range rule.  One 1-D pass of the inverse DCT is, per output, a linear form of its eight inputs whose coefficients (scaled by 2^13) have an
absolute sum of at most PASS_ABS_SUM = 61 214 -- and so has every intermediate of the factorisation (idct_forms() lists them).  With inputs
in int16 the magnitude stays below 32 768 * 61 214 + 2^17 < 2^31: int32 cannot overflow.  So a file is refused when a dequantised
coefficient lies outside int16 (status 8) or a value of the column pass's workspace does (status 9); inside those bounds the int32 kernels,
this statement in Python ints and libjpeg-turbo's C and SIMD paths are one function up to the final clamp.  Beyond +-512 after the
descale libjpeg's C path wraps through a masked table where its SIMD path saturates; the statement saturates and claims nothing about
Pillow there.  Genuine encoder output stays below +-2 200.
"""
import struct

import numpy as np

from . import lib as _lib
from . import _hip
from .file_reader import DeviceFileReader, _up

MAX_SIDE = 32767
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)
STATUS = {1: "a marker inside the entropy-coded data", 2: "a restart marker out of sequence, or not one per restart interval",
          3: "no EOI marker behind the entropy-coded data", 4: "bits no Huffman code owns", 5: "a coefficient index beyond 63",
          6: "a restart interval ends before its MCUs are done", 7: "a restart interval has bytes left over",
          8: "a dequantised coefficient outside int16 (the range rule)", 9: "a workspace value of the inverse DCT outside int16 (the range rule)"}
PASS_ABS_SUM = 61214
_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)", 0xC5: "SOF5 (differential sequential)",
              0xC6: "SOF6 (differential progressive)", 0xC7: "SOF7 (differential lossless)", 0xC9: "SOF9 (arithmetic sequential)",
              0xCA: "SOF10 (arithmetic progressive)", 0xCB: "SOF11 (arithmetic lossless)", 0xCD: "SOF13 (differential arithmetic sequential)",
              0xCE: "SOF14 (differential arithmetic progressive)", 0xCF: "SOF15 (differential arithmetic lossless)"}
# egs_jpeg_file, egs_jpeg_tables (include/egs_raster.h)
_FILE = np.dtype([("width", "<i4"), ("height", "<i4"), ("channels", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("restart_interval", "<i4"),
                  ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("interval_begin", "<u4"), ("n_intervals", "<u4"), ("entropy_begin", "<u4"),
                  ("entropy_bytes", "<u4"), ("tq", "u1", (4,)), ("td", "u1", (4,)), ("ta", "u1", (4,)), ("reserved", "<u4"),
                  ("file_offset", "<u8"), ("file_bytes", "<u8"), ("coef_offset", "<u8"), ("plane_offset", "<u8"), ("out_offset", "<u8")])
_HUFF = np.dtype([("counts", "u1", (16,)), ("values", "u1", (256,))])
_TABLES = np.dtype([("quant", "u1", (4, 64)), ("dc", _HUFF, (4,)), ("ac", _HUFF, (4,))])
assert _FILE.itemsize == 104 and _TABLES.itemsize == 2432


def status_text(word):
    """What a status word of egs_jpeg_decode says."""
    word = int(word)
    if word == 0:
        return "ok"
    text = STATUS.get(word & 255, f"status {word}")
    return f"{text} (restart interval {word >> 8})" if 4 <= (word & 255) <= 7 else text


class StatusError(ValueError):
    """decode(): the file is one the device refuses, with this status word."""

    def __init__(self, status):
        super().__init__(f"jpeg.decode: {status_text(status)} (status {status})")
        self.status = status


# ---- the host's share --------------------------------------------------------------------------------------------------------------------
def parse(file_bytes):
    """The marker segments from SOI up to and including the SOS header: DQT, DHT, SOF0, DRI, APP0 "JFIF", APP14 "Adobe"; other APPn and COM
    are skipped.  -> dict(W, H, C, hs, vs: the luma sampling (chroma is 1 x 1), quant: uint8 [4, 64] in natural order, dc / ac: [(counts
    uint8 [16], values uint8 [256]) or None] * 4, tq / td / ta: the table index per component, restart_interval, entropy_begin).
    ValueError, naming the marker or field, for everything this path does not read."""
    from .ingest import _ADVICE
    data = bytes(file_bytes) if not isinstance(file_bytes, (bytes, bytearray)) else file_bytes
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("jpeg.parse: no SOI marker")
    quant, dc, ac = [None] * 4, [None] * 4, [None] * 4
    frame, ri, jfif, adobe = None, 0, False, None
    pos = 2
    while True:
        if pos + 4 > n:
            raise ValueError(f"jpeg.parse: the file ends at byte {pos}, before an SOS marker")
        if data[pos] != 0xFF:
            raise ValueError(f"jpeg.parse: byte {pos} is not a marker")
        m = data[pos + 1]
        if m == 0xFF:                                                   # fill byte in front of a marker
            pos += 1
            continue
        if m == 0xD9 or 0xD0 <= m <= 0xD7 or m == 0x01 or m == 0xD8 or m == 0x00:
            raise ValueError(f"jpeg.parse: marker FF {m:02X} at byte {pos}, before an SOS marker")
        length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if length < 2 or pos + 2 + length > n:
            raise ValueError(f"jpeg.parse: segment FF {m:02X} at byte {pos} runs past the end of the file")
        seg = data[pos + 4:pos + 2 + length]
        if m in _SOF_NAMES or m == 0xC8:
            raise ValueError(f"jpeg.parse: {_SOF_NAMES.get(m, 'JPG (reserved)')}: this path reads baseline (SOF0) files; decode it on the host, "
                             f"{_ADVICE}")
        if m == 0xCC:
            raise ValueError(f"jpeg.parse: DAC (arithmetic coding conditioning): this path reads Huffman-coded baseline files; {_ADVICE}")
        if m == 0xDB:                                                   # DQT
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    raise ValueError(f"jpeg.parse: DQT table {tq} has 16-bit entries (Pq = {pq}): baseline tables are 8-bit; {_ADVICE}")
                if tq > 3 or at + 65 > len(seg):
                    raise ValueError(f"jpeg.parse: DQT at byte {pos}: table index {tq} or a table that leaves its segment")
                t = np.frombuffer(seg[at + 1:at + 65], dtype=np.uint8)
                if not t.all():
                    raise ValueError(f"jpeg.parse: DQT table {tq} has a zero entry")
                nat = np.zeros(64, dtype=np.uint8)
                nat[ZIGZAG] = t
                quant[tq] = nat
                at += 65
        elif m == 0xC4:                                                 # DHT
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise ValueError(f"jpeg.parse: DHT at byte {pos}: a table that leaves its segment")
                tc, th = seg[at] >> 4, seg[at] & 15
                counts = np.frombuffer(seg[at + 1:at + 17], dtype=np.uint8)
                total = int(counts.sum())
                if tc > 1 or th > 3:
                    raise ValueError(f"jpeg.parse: DHT at byte {pos}: class {tc}, index {th}")
                if total > 256 or at + 17 + total > len(seg):
                    raise ValueError(f"jpeg.parse: DHT table {tc}/{th} has {total} symbols: more than 256, or more than its segment holds")
                code, over = 0, False
                for length_ in range(1, 17):
                    code += int(counts[length_ - 1])
                    if code > (1 << length_):
                        over = True
                    code <<= 1
                if over:
                    raise ValueError(f"jpeg.parse: DHT table {tc}/{th}: the counts over-subscribe the code space")
                values = np.zeros(256, dtype=np.uint8)
                values[:total] = np.frombuffer(seg[at + 17:at + 17 + total], dtype=np.uint8)
                if tc == 0 and total and int(values[:total].max()) > 15:
                    raise ValueError(f"jpeg.parse: DHT table 0/{th}: a DC symbol above 15")
                (dc if tc == 0 else ac)[th] = (counts.copy(), values)
                at += 17 + total
        elif m == 0xC0:                                                 # SOF0
            if frame is not None:
                raise ValueError(f"jpeg.parse: a second SOF0 at byte {pos}")
            if len(seg) < 6:
                raise ValueError(f"jpeg.parse: SOF0 at byte {pos} is shorter than its fixed fields")
            prec, H, W, C = struct.unpack(">BHHB", seg[:6])
            if prec != 8:
                raise ValueError(f"jpeg.parse: SOF0 sample precision {prec}: this path reads 8-bit samples; {_ADVICE}")
            if not 1 <= H <= MAX_SIDE:
                raise ValueError(f"jpeg.parse: SOF0 height {H} is outside 1 .. {MAX_SIDE}")
            if not 1 <= W <= MAX_SIDE:
                raise ValueError(f"jpeg.parse: SOF0 width {W} is outside 1 .. {MAX_SIDE}")
            if C not in (1, 3):
                raise ValueError(f"jpeg.parse: SOF0 has {C} components (CMYK / YCCK and two-component files are not read here); {_ADVICE}")
            if len(seg) != 6 + 3 * C:
                raise ValueError(f"jpeg.parse: SOF0 at byte {pos}: {len(seg)} bytes for {C} components")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(C)]      # id, h, v, tq
            frame = (W, H, C, comps)
        elif m == 0xDD:                                                 # DRI
            if len(seg) != 2:
                raise ValueError(f"jpeg.parse: DRI at byte {pos} is {len(seg)} bytes")
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xE0 and seg[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:                                                 # SOS
            if frame is None:
                raise ValueError(f"jpeg.parse: SOS at byte {pos} before SOF0")
            W, H, C, comps = frame
            if not len(seg) or len(seg) != 4 + 2 * seg[0]:
                raise ValueError(f"jpeg.parse: SOS at byte {pos}: {len(seg)} bytes for {seg[0] if len(seg) else 0} components")
            ns = seg[0]
            sel = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
            ss, se, a = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
            if ns != C or [s[0] for s in sel] != [c[0] for c in comps] or (ss, se, a) != (0, 63, 0):
                raise ValueError(f"jpeg.parse: SOS at byte {pos} holds {ns} of {C} components with Ss {ss}, Se {se}, Ah/Al {a}: this path reads "
                                 f"one scan of all components in frame order (no multi-scan file); {_ADVICE}")
            sampling = [(c[1], c[2]) for c in comps]
            ok = sampling == [(1, 1)] if C == 1 else (sampling[0] in ((1, 1), (2, 1), (2, 2)) and sampling[1:] == [(1, 1), (1, 1)])
            if not ok:
                raise ValueError(f"jpeg.parse: SOF0 sampling factors {sampling}: this path reads luma 1x1, 2x1 or 2x2 with 1x1 chroma; {_ADVICE}")
            if C == 3:
                ids = [c[0] for c in comps]
                if not (jfif or adobe == 1 or (adobe is None and ids == [1, 2, 3])):
                    why = f"Adobe transform {adobe}" if adobe is not None else f"component ids {ids} with neither a JFIF nor an Adobe marker"
                    raise ValueError(f"jpeg.parse: {why}: the three components are not marked as YCbCr; {_ADVICE}")
            tq, td, ta = [c[3] for c in comps], [s[1] for s in sel], [s[2] for s in sel]
            for c in range(C):
                if tq[c] > 3 or quant[tq[c]] is None:
                    raise ValueError(f"jpeg.parse: component {c} refers to DQT table {tq[c]}, which is missing")
                if td[c] > 3 or dc[td[c]] is None:
                    raise ValueError(f"jpeg.parse: component {c} refers to DC DHT table {td[c]}, which is missing")
                if ta[c] > 3 or ac[ta[c]] is None:
                    raise ValueError(f"jpeg.parse: component {c} refers to AC DHT table {ta[c]}, which is missing")
            q = np.stack([t if t is not None else np.zeros(64, dtype=np.uint8) for t in quant])
            return dict(W=W, H=H, C=C, hs=sampling[0][0], vs=sampling[0][1], quant=q, dc=list(dc), ac=list(ac), tq=tq, td=td, ta=ta,
                        restart_interval=ri, entropy_begin=pos + 2 + length)
        pos += 2 + length


def geometry(p):
    """-> (mcus_x, mcus_y, blocks per MCU, n_intervals) of a parsed file."""
    mx, my = -(-p["W"] // (8 * p["hs"])), -(-p["H"] // (8 * p["vs"]))
    bpm = p["hs"] * p["vs"] + 2 if p["C"] == 3 else 1
    ri = p["restart_interval"]
    return mx, my, bpm, (-(-(mx * my) // ri) if ri else 1)


# ---- the statement -----------------------------------------------------------------------------------------------------------------------
def scan_intervals(data, begin, n_intervals):
    """The entropy-coded bytes from `begin`: FF 00 is a stuffed FF, FF D0 .. D7 starts the next restart interval behind it (its number is the
    interval's index mod 8), FF D9 ends the data.  -> [(start, end)] * n_intervals, or StatusError 1 / 2 / 3 for the first failure in byte
    order."""
    out, start, i, n = [], begin, begin, len(data)
    while True:
        i = data.find(b"\xff", i)
        if i < 0 or i + 1 >= n:
            raise StatusError(3)
        m = data[i + 1]
        if m == 0:
            i += 2
        elif 0xD0 <= m <= 0xD7:
            if m - 0xD0 != len(out) % 8:
                raise StatusError(2)
            out.append((start, i))
            start = i = i + 2
        elif m == 0xD9:
            out.append((start, i))
            if len(out) != n_intervals:
                raise StatusError(2)
            return out
        else:
            raise StatusError(1)


def _codebook(counts, values):
    """-> (maxcode [17] with -1 for an empty length, valptr [17], mincode [17]) of the canonical code."""
    maxcode, valptr, mincode = [-1] * 18, [0] * 18, [0] * 18
    code = k = 0
    for length in range(1, 17):
        valptr[length], mincode[length] = k, code
        k += int(counts[length - 1])
        code += int(counts[length - 1])
        maxcode[length] = code - 1 if counts[length - 1] else -1
        code <<= 1
    return maxcode, valptr, mincode


class _Bits:
    """The bits of one restart interval, stuffed bytes undone."""

    def __init__(self, data, start, end):
        self.b = bytes(data[start:end]).replace(b"\xff\x00", b"\xff")
        self.pos, self.n = 0, 8 * len(self.b)

    def bit(self):
        if self.pos >= self.n:
            return None
        v = (self.b[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return v


def _symbol(bits, book, values, k):
    """One Huffman symbol by the canonical-code walk: status 6 when the interval's bits run out first, 4 when 16 bits match no code."""
    maxcode, valptr, mincode = book
    code = 0
    for length in range(1, 17):
        b = bits.bit()
        if b is None:
            raise StatusError(6 | k << 8)
        code = code << 1 | b
        if code <= maxcode[length]:
            return int(values[valptr[length] + code - mincode[length]])
    raise StatusError(4 | k << 8)


def _receive(bits, s, k):
    v = 0
    for _ in range(s):
        b = bits.bit()
        if b is None:
            raise StatusError(6 | k << 8)
        v = v << 1 | b
    return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def entropy_decode(data, p, reset=True):
    """-> int16 [blocks, 64]: the dequantised coefficients in natural order, the blocks in MCU order (the luma blocks of an MCU row by row,
    then Cb, Cr).  StatusError 1 .. 8.  reset=False (no DC reset at a restart) is a deliberately wrong statement for the tests."""
    mx, my, bpm, n_int = geometry(p)
    intervals = scan_intervals(data, p["entropy_begin"], n_int)
    comp_of = [0] * (bpm - 2) + [1, 2] if p["C"] == 3 else [0]
    books_dc = [None if t is None else _codebook(*t) for t in p["dc"]]
    books_ac = [None if t is None else _codebook(*t) for t in p["ac"]]
    quant = p["quant"].astype(np.int64)
    coef = np.zeros((mx * my * bpm, 64), dtype=np.int16)
    per = p["restart_interval"] or mx * my
    for k, (start, end) in enumerate(intervals):
        bits = _Bits(data, start, end)
        pred = [0, 0, 0] if reset or k == 0 else pred
        for mcu in range(k * per, min((k + 1) * per, mx * my)):
            for j in range(bpm):
                c = comp_of[j]
                q = quant[p["tq"][c]]
                s = _symbol(bits, books_dc[p["td"][c]], p["dc"][p["td"][c]][1], k)
                if s:
                    pred[c] += _receive(bits, s, k)
                v = pred[c] * int(q[0])
                if not -32768 <= pred[c] <= 32767 or not -32768 <= v <= 32767:
                    raise StatusError(8)
                block = coef[mcu * bpm + j]
                block[0] = v
                at = 1
                while at < 64:
                    rs = _symbol(bits, books_ac[p["ta"][c]], p["ac"][p["ta"][c]][1], k)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        at += 16
                        if at > 63:                                      # a run of zeros must be followed by a coefficient
                            raise StatusError(5 | k << 8)
                        continue
                    at += r
                    if at > 63:
                        raise StatusError(5 | k << 8)
                    v = _receive(bits, s, k) * int(q[ZIGZAG[at]])
                    if not -32768 <= v <= 32767:
                        raise StatusError(8)
                    block[ZIGZAG[at]] = v
                    at += 1
        if (bits.n - bits.pos) >= 8:
            raise StatusError(7 | k << 8)
    return coef


def idct_pass(v, shift, log=None):
    """One 1-D pass of the `islow` inverse DCT on the eight values v[0 .. 8) (Python ints, or numpy int32 / int64 arrays: the same
    expression tree either way) -> eight values descaled by `shift`.  log, a list, receives every intermediate."""
    keep = (lambda x: (log.append(x), x)[1]) if log is not None else (lambda x: x)
    z2, z3 = v[2], v[6]
    z1 = keep((z2 + z3) * 4433)
    tmp2 = keep(z1 + z3 * -15137)
    tmp3 = keep(z1 + z2 * 6270)
    tmp0 = keep((v[0] + v[4]) * 8192)
    tmp1 = keep((v[0] - v[4]) * 8192)
    tmp10, tmp13, tmp11, tmp12 = keep(tmp0 + tmp3), keep(tmp0 - tmp3), keep(tmp1 + tmp2), keep(tmp1 - tmp2)
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = keep((z3 + z4) * 9633)
    t0, t1, t2, t3 = keep(t0 * 2446), keep(t1 * 16819), keep(t2 * 25172), keep(t3 * 12299)
    z1, z2, z3, z4 = keep(z1 * -7373), keep(z2 * -20995), keep(z3 * -16069), keep(z4 * -3196)
    z3, z4 = keep(z3 + z5), keep(z4 + z5)
    t0, t1, t2, t3 = keep(t0 + keep(z1 + z3)), keep(t1 + keep(z2 + z4)), keep(t2 + keep(z2 + z3)), keep(t3 + keep(z1 + z4))
    half = 1 << (shift - 1)
    outs = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return [keep(o + half) >> shift for o in outs]


def idct_forms():
    """Every intermediate and output of idct_pass (before the descale) as a linear form of the eight inputs -> int array [n, 8].  The largest
    absolute row sum is PASS_ABS_SUM."""
    rows = []
    for k in range(8):
        log = []
        idct_pass([1 if j == k else 0 for j in range(8)], 1, log)
        zero = []
        idct_pass([0] * 8, 1, zero)
        rows.append([a - b for a, b in zip(log, zero)])                 # (the rounding constant is not part of the form)
    return np.array(rows, dtype=np.int64).T


def idct_blocks(coef, dtype=np.int64, rows_first=False):
    """coef int16 [n, 64] -> uint8 samples [n, 8, 8]: column pass (descaled by 11) into the workspace, whose values must lie in int16
    (StatusError 9), row pass (descaled by 18), + 128, saturating clamp.  dtype=np.int32 is the arithmetic of the kernel.  rows_first is a
    deliberately wrong statement for the tests."""
    c = coef.reshape(-1, 8, 8).astype(dtype)
    with np.errstate(over="ignore"):
        if rows_first:
            ws = np.stack(idct_pass([c[:, :, k] for k in range(8)], 11), axis=2)
            out = np.stack(idct_pass([ws[:, k, :] for k in range(8)], 18), axis=1)
        else:
            ws = np.stack(idct_pass([c[:, k, :] for k in range(8)], 11), axis=1)
            if ws.size and (int(ws.min()) < -32768 or int(ws.max()) > 32767):
                raise StatusError(9)
            out = np.stack(idct_pass([ws[:, :, k] for k in range(8)], 18), axis=2)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes_of(samples, p):
    """samples uint8 [blocks, 8, 8] in MCU order -> the component planes, each padded to whole MCUs."""
    mx, my, bpm, _ = geometry(p)
    hs, vs = p["hs"], p["vs"]
    s = samples.reshape(my, mx, bpm, 8, 8)
    luma = s[:, :, :hs * vs].reshape(my, mx, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
    if p["C"] == 1:
        return [luma]
    return [luma] + [s[:, :, hs * vs + c].transpose(0, 2, 1, 3).reshape(my * 8, mx * 8) for c in range(2)]


def upsample(plane, p, nearest=False, swap_rounding=False, padded=False):
    """A chroma plane (padded) -> int32 [H, W]: cropped to ceil(W / hs) x ceil(H / vs), then libjpeg's "fancy" upsampling -- h2v1:
    (3 a + prev + 1) >> 2 and (3 a + next + 2) >> 2, the first and last output columns copied; h2v2: s = 3 near + far down the rows, then
    (3 s + prev + 8) >> 4 and (3 s + next + 7) >> 4 with (4 s + 8) >> 4 and (4 s + 7) >> 4 at the two edges; rows and columns outside the
    cropped plane repeat its edge.  A cropped plane of at most two columns is replicated (libjpeg's own condition).  nearest,
    swap_rounding and padded (the MCU-padded width in place of the cropped one) are deliberately wrong statements for the tests."""
    W, H, hs, vs = p["W"], p["H"], p["hs"], p["vs"]
    cw, ch = plane.shape[1] if padded else -(-W // hs), -(-H // vs)
    a = plane[:ch, :cw].astype(np.int32)
    if hs == 1:
        return a[:H, :W]
    if cw <= 2 or nearest:
        return np.repeat(np.repeat(a, vs, axis=0), 2, axis=1)[:H, :W]
    if vs == 2:
        up, down = np.vstack([a[:1], a[:-1]]), np.vstack([a[1:], a[-1:]])
        s = np.empty((2 * ch, cw), dtype=np.int32)
        s[0::2], s[1::2] = 3 * a + up, 3 * a + down
        (r0, r1), shift = ((7, 8) if swap_rounding else (8, 7)), 4
    else:
        s, (r0, r1), shift = a, ((2, 1) if swap_rounding else (1, 2)), 2
    prev, nxt = np.hstack([s[:, :1], s[:, :-1]]), np.hstack([s[:, 1:], s[:, -1:]])
    out = np.empty((s.shape[0], 2 * cw), dtype=np.int32)
    out[:, 0::2], out[:, 1::2] = (3 * s + prev + r0) >> shift, (3 * s + nxt + r1) >> shift
    if vs == 1:                                                         # (h2v2's edge expressions are the general ones with prev = next = s)
        out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out[:H, :W]


def colour(y, cb, cr, half=32768):
    """Fixed-point YCbCr -> RGB uint8 [H, W, 3].  half=0 is a deliberately wrong statement for the tests."""
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + half) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(file_bytes, wrong=None):
    """A baseline JPEG file -> uint8 [h, w, C] (C = 1 or 3), the strict host reader.  ValueError for a file parse() refuses; StatusError (a
    ValueError) with the device's status word for a file the kernels refuse.  wrong: for the tests, one of WRONG -- a statement that differs
    from this one in that single point."""
    if wrong is not None and wrong not in WRONG:
        raise ValueError(f"jpeg.decode: wrong is one of {WRONG}")
    data = bytes(file_bytes)
    p = parse(data)
    coef = entropy_decode(data, p, reset=wrong != "no DC reset at a restart")
    planes = planes_of(idct_blocks(coef, rows_first=wrong == "the row pass before the column pass"), p)
    W, H = p["W"], p["H"]
    if p["C"] == 1:
        return np.ascontiguousarray(planes[0][:H, :W, None])
    kw = dict(nearest=wrong == "nearest-neighbour chroma", swap_rounding=wrong == "the rounding constants swapped",
              padded=wrong == "the MCU-padded width for the last-column rule")
    return colour(planes[0][:H, :W], upsample(planes[1], p, **kw), upsample(planes[2], p, **kw), half=0 if wrong == ">> 16 without the half" else 32768)


WRONG = ("nearest-neighbour chroma", "the rounding constants swapped", "the MCU-padded width for the last-column rule",
         "the row pass before the column pass", ">> 16 without the half", "no DC reset at a restart")


# ---- the device --------------------------------------------------------------------------------------------------------------------------
def plan(parsed, out_gap=0):
    """parsed: [parse(file) with "nbytes": the file's length] -> dict(desc, tables: the two arrays of egs_jpeg_decode with files, coefficients,
    planes and outputs packed in order -- files, coefficients and planes at multiples of 16, outputs at multiples of 256 with `out_gap` bytes
    between them --, n_intervals, files_bytes, coef_bytes, plane_bytes, out_bytes: the totals)."""
    desc = np.zeros(len(parsed), dtype=_FILE)
    tables = np.zeros(len(parsed), dtype=_TABLES)
    fo = co = po = oo = k = 0
    for i, p in enumerate(parsed):
        nbytes = int(p["nbytes"])
        if nbytes >= 1 << 31:
            raise ValueError(f"jpeg: file {i} has {nbytes} bytes; the limit is 2 GiB")
        mx, my, bpm, n_int = geometry(p)
        pad = lambda v: list(v) + [0] * (4 - len(v))
        desc[i] = (p["W"], p["H"], p["C"], p["hs"], p["vs"], p["restart_interval"], mx, my, k, n_int, p["entropy_begin"],
                   nbytes - p["entropy_begin"], pad(p["tq"]), pad(p["td"]), pad(p["ta"]), 0, fo, nbytes, co, po, oo)
        tables[i]["quant"] = p["quant"]
        for name in ("dc", "ac"):
            for t, tab in enumerate(p[name]):
                if tab is not None:
                    tables[i][name][t]["counts"], tables[i][name][t]["values"] = tab
        k += n_int
        fo += _up(nbytes, 16)
        co += _up(mx * my * bpm * 128, 16)
        po += _up(mx * my * bpm * 64, 16)
        oo += _up(p["H"] * p["W"] * p["C"] + out_gap, 256)
    return dict(desc=desc, tables=tables, n_intervals=k, files_bytes=fo, coef_bytes=co, plane_bytes=po, out_bytes=oo)


class JpegReader(DeviceFileReader):
    """Baseline JPEG files -> device uint8 [h, w, C] tensors: DeviceFileReader's contract (file_reader.py: the buffers, the batches, one
    upload and one read of the status words per batch, the guard bytes).  Per batch the host walks the marker segments (parse) and the
    device runs four launches."""
    NAME, FORMAT, HOST_READER = "JpegReader", "JPEG", "jpeg.decode"
    status_text = staticmethod(status_text)

    @staticmethod
    def _parse_one(blob):
        return dict(parse(blob), nbytes=len(blob))

    @staticmethod
    def _shape(entry):
        return entry["W"], entry["H"], entry["C"]

    _plan = staticmethod(plan)

    def _second_table(self, p):
        return p["tables"], p["n_intervals"]

    def _scratch_need(self, lib, n, p):
        return int(lib.egs_jpeg_decode_scratch_bytes(n, p["n_intervals"], p["coef_bytes"], p["plane_bytes"]))

    def _reserve_scratch(self, max_file_bytes, max_pixels):
        return self.batch * (9 * (max_pixels + 2 * MAX_SIDE) + 4096)

    def _status_allocation(self):
        return 4 * self.batch

    def _launch(self, lib, call, n, status):
        _lib.check(lib.egs_jpeg_decode(*call, _hip.stream_of(self.device)))


def decode_device(file_bytes, device="cuda"):
    """One file (bytes or a path) -> device uint8 [h, w, C], by the kernels.  (A reader of many files keeps a JpegReader.)"""
    return JpegReader(device, batch=1).read([file_bytes])[0].clone()
