"""Builders shared by the JPEG tests (tests/test_jpeg_cpu.py, tests/test_gpu_jpeg.py): the golden Pillow files, a tiny baseline WRITER for
tests only (fixed tables, a given coefficient array in, file bytes out) to craft what Pillow cannot write, malformed() -- entropy-coded data
the device refuses, with the status word -- and refusals() -- headers parse() refuses, with the words its message must hold.
Everything is seeded, built once and left unchanged."""
import functools
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


@functools.lru_cache(maxsize=None)
def golden():
    """name -> (file bytes, uint8 [h, w, C] as Pillow decodes them) of tests/golden/jpeg_files.npz."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_files.npz"))
    return {k[:-5]: (z[k].tobytes(), z[k[:-5] + ".pixels"]) for k in sorted(z.files) if k.endswith(".file")}


# ---- the writer's fixed tables: neither is complete, so there are bits no code owns ----------------------------------------------------------------
# DC: the 16 categories in 5 bits each (codes 00000 .. 01111).  AC: eight common symbols in 4 bits (0000 .. 0111), the other 248 in 10 bits
# (1000000000 ..): short codes for the look-up, long ones for the canonical walk.
DC_COUNTS = [0, 0, 0, 0, 16] + [0] * 11
DC_VALUES = list(range(16))
_AC_SHORT = [0x00, 0xF0, 0x01, 0x02, 0x03, 0x11, 0x12, 0x21]
AC_COUNTS = [0, 0, 0, 8, 0, 0, 0, 0, 0, 248] + [0] * 6
AC_VALUES = _AC_SHORT + [v for v in range(256) if v not in _AC_SHORT]


def _codes(counts, values):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODE, AC_CODE = _codes(DC_COUNTS, DC_VALUES), _codes(AC_COUNTS, AC_VALUES)


class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, length):
        self.acc = self.acc << length | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)                 # pad with ones
        done, self.out = bytes(self.out), bytearray()
        return done


def _magnitude(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def encode_block(w, block, pred):
    """One block of 64 quantised coefficients in natural order -> its symbols; returns the new DC predictor."""
    dc = int(block[0])
    s, bits = _magnitude(dc - pred)
    w.put(*DC_CODE[s])
    if s:
        w.put(bits, s)
    run = 0
    zz = [int(block[ZIGZAG[k]]) for k in range(64)]
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            w.put(*AC_CODE[0xF0])
            run -= 16
        s, bits = _magnitude(zz[k])
        w.put(*AC_CODE[run << 4 | s])
        w.put(bits, s)
        run = 0
    if last < 63:
        w.put(*AC_CODE[0x00])
    return dc


def segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def header(W, H, C=3, hs=2, vs=2, quant=1, restart=0, jfif=True, ids=(1, 2, 3)):
    """The segments in front of the entropy-coded data as a list of (marker, payload) the tests may edit; quant: one value for all 64 entries."""
    segs = []
    if jfif:
        segs.append((0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"))
    segs.append((0xDB, bytes([0]) + bytes([quant] * 64)))
    comps = [(ids[0], hs << 4 | vs, 0), (ids[1], 0x11, 0), (ids[2], 0x11, 0)][:C]
    segs.append((0xC0, struct.pack(">BHHB", 8, H, W, C) + b"".join(bytes(c) for c in comps)))
    segs.append((0xC4, bytes([0x00]) + bytes(DC_COUNTS) + bytes(DC_VALUES) + bytes([0x10]) + bytes(AC_COUNTS) + bytes(AC_VALUES)))
    if restart:
        segs.append((0xDD, struct.pack(">H", restart)))
    segs.append((0xDA, bytes([C]) + b"".join(bytes([c[0], 0x00]) for c in comps) + bytes([0, 63, 0])))
    return segs


def entropy(blocks, bpm, C, hs=2, vs=2, restart=0):
    """blocks: int [n, 64] quantised coefficients, natural order, MCU order -> [interval bytes]."""
    comp_of = [0] * (bpm - 2) + [1, 2] if C == 3 else [0]
    n_mcu = len(blocks) // bpm
    per = restart or n_mcu
    out = []
    for m0 in range(0, n_mcu, per):
        w, pred = _BitWriter(), [0, 0, 0]
        for m in range(m0, min(n_mcu, m0 + per)):
            for j in range(bpm):
                pred[comp_of[j]] = encode_block(w, blocks[m * bpm + j], pred[comp_of[j]])
        out.append(w.flush())
    return out


def assemble(segs, intervals, eoi=True):
    data = b"\xff\xd8" + b"".join(segment(m, p) for m, p in segs)
    for k, iv in enumerate(intervals):
        data += (bytes([0xFF, 0xD0 + (k - 1) % 8]) if k else b"") + iv
    return data + (b"\xff\xd9" if eoi else b"")


def geometry(W, H, C, hs, vs):
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return mx, my, (hs * vs + 2 if C == 3 else 1)


def write(blocks, W, H, C=3, hs=2, vs=2, quant=1, restart=0):
    """The writer: quantised coefficients [mcus * blocks per MCU, 64] -> a baseline file."""
    bpm = geometry(W, H, C, hs, vs)[2]
    return assemble(header(W, H, C, hs, vs, quant, restart), entropy(blocks, bpm, C, hs, vs, restart))


def coefficients(seed, W, H, C=3, hs=2, vs=2, amplitude=40):
    """Seeded quantised coefficients: a DC level per block, a few low frequencies, one high one (a run of more than 16 zeros)."""
    rng = np.random.default_rng(seed)
    mx, my, bpm = geometry(W, H, C, hs, vs)
    b = np.zeros((mx * my * bpm, 64), dtype=np.int64)
    b[:, 0] = rng.integers(-amplitude, amplitude, len(b))
    for k in (1, 8, 9, 2, 16):
        b[:, k] = rng.integers(-amplitude // 4, amplitude // 4 + 1, len(b))
    b[::2, 62] = rng.integers(1, 4, len(b[::2]))
    b[1::3, 63] = -1
    return b


@functools.lru_cache(maxsize=None)
def written():
    """name -> (file bytes, the dequantised coefficients, (W, H, C, hs, vs)): what the writer makes of seeded coefficients, for the round trip."""
    out = {}
    for name, (W, H, C, hs, vs, q, ri) in {"w-420": (21, 19, 3, 2, 2, 3, 0), "w-422-ri1": (21, 19, 3, 2, 1, 2, 1), "w-444-ri2": (9, 17, 3, 1, 1, 5, 2),
                                           "w-L-ri3": (30, 9, 1, 1, 1, 4, 3)}.items():
        b = coefficients(len(out), W, H, C, hs, vs)
        out[name] = (write(b, W, H, C, hs, vs, q, ri), b * q, (W, H, C, hs, vs))
    return out


def _flat(W, H, dc, ac=None, **kw):
    """A 4:2:0 file whose every block has the DC value `dc` (and coefficient 1 = ac)."""
    mx, my, bpm = geometry(W, H, 3, 2, 2)
    b = np.zeros((mx * my * bpm, 64), dtype=np.int64)
    b[:, 0] = dc
    if ac is not None:
        b[:, 1] = ac
    return write(b, W, H, **kw)


@functools.lru_cache(maxsize=None)
def malformed():
    """name -> (file bytes, the status word the device and jpeg.decode give).  Every file passes parse()."""
    out = {}
    W, H = 21, 19                                                       # 2 x 2 MCUs of 6 blocks
    blocks = coefficients(7, W, H)
    segs, segs_ri = header(W, H), header(W, H, restart=1)
    iv, iv_ri = entropy(blocks, 6, 3), entropy(blocks, 6, 3, restart=1)
    good = assemble(segs, iv)
    at = len(good) - 2 - len(iv[0])                                      # the first entropy-coded byte
    out["a marker inside the data"] = (good[:at + 5] + b"\xff\xc4" + good[at + 5:], 1)
    out["a fill byte inside the data"] = (good[:at + 5] + b"\xff\xff" + good[at + 5:], 1)
    bad = bytearray(assemble(segs_ri, iv_ri))
    k = bad.index(b"\xff\xd1")
    bad[k + 1] = 0xD3
    out["a restart marker out of sequence"] = (bytes(bad), 2)
    out["fewer restart markers than intervals"] = (assemble(header(W, H, restart=1), entropy(blocks, 6, 3, restart=2)), 2)
    out["more restart markers than intervals"] = (assemble(header(W, H, restart=2), entropy(blocks, 6, 3, restart=1)), 2)
    out["no EOI"] = (assemble(segs, iv, eoi=False), 3)
    out["the file ends on FF"] = (assemble(segs, iv, eoi=False) + b"\xff", 3)
    out["bits no code owns"] = (good[:at] + b"\xfe\xfe" + good[at + 2:], 4)
    ri = assemble(segs_ri, iv_ri)
    k = ri.index(b"\xff\xd1") + 2                                         # the first byte of interval 2
    out["bits no code owns in interval 2"] = (ri[:k] + b"\xfe\xfe" + ri[k + 2:], 4 | 2 << 8)
    w = _BitWriter()                                                    # a block whose runs pass coefficient 63
    w.put(*DC_CODE[0])
    for _ in range(4):
        w.put(*AC_CODE[0xF1])
        w.put(1, 1)
    out["a coefficient index beyond 63"] = (assemble(segs, [w.flush() + iv[0]]), 5)
    w.put(*DC_CODE[0])
    for _ in range(4):
        w.put(*AC_CODE[0xF0])
    out["zero runs beyond 63"] = (assemble(segs, [w.flush() + iv[0]]), 5)
    out["an interval ends early"] = (assemble(segs, [iv[0][:-1]]), 6)
    out["interval 1 ends early"] = (assemble(segs_ri, [iv_ri[0], iv_ri[1][:-1]] + iv_ri[2:]), 6 | 1 << 8)
    out["an interval is empty"] = (assemble(segs_ri, iv_ri[:3] + [b""]), 6 | 3 << 8)
    out["bytes left over"] = (assemble(segs, [iv[0] + b"\x55"]), 7)
    out["bytes left over in interval 3"] = (assemble(segs_ri, iv_ri[:3] + [iv_ri[3] + b"\xff\x00"]), 7 | 3 << 8)
    out["a DC coefficient outside int16"] = (_flat(W, H, 200, quant=255), 8)
    out["an AC coefficient outside int16"] = (_flat(W, H, 1, ac=-129, quant=255), 8)
    climb = np.zeros((24, 64), dtype=np.int64)
    climb[[k for k in range(24) if k % 6 < 4], 0] = 40000                 # the luma blocks: differences the code can carry (20 000 twice,
    climb[0, 0] = 20000                                                 # then none), a sum it must not
    out["a DC predictor outside int16"] = (write(climb, W, H), 8)
    out["a workspace value outside int16"] = (_flat(W, H, 128, quant=255), 9)      # 32 640 is in range; the column pass gives 4 x that
    return out


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (file bytes, words the message of parse() must hold)."""
    W, H = 21, 19
    blocks = coefficients(9, W, H)
    iv = entropy(blocks, 6, 3)

    def edit(marker, fn, **kw):
        segs = header(W, H, **kw)
        return assemble([(m, fn(p) if m == marker else p) for m, p in segs], iv)

    def swap(marker, new, **kw):
        return assemble([(new if m == marker else m, p) for m, p in header(W, H, **kw)], iv)

    def drop(marker, **kw):
        return assemble([(m, p) for m, p in header(W, H, **kw) if m != marker], iv)

    def sof(**f):
        def fn(p):
            prec, h, w, c = struct.unpack(">BHHB", p[:6])
            comps = [list(p[6 + 3 * k:9 + 3 * k]) for k in range(c)]
            prec, h, w = f.get("prec", prec), f.get("h", h), f.get("w", w)
            for k, v in f.get("sampling", {}).items():
                comps[k][1] = v
            for k, v in f.get("ids", {}).items():
                comps[k][0] = v
            for k, v in f.get("tq", {}).items():
                comps[k][2] = v
            comps = comps[:f.get("c", c)] + [[9, 0x11, 0]] * max(0, f.get("c", c) - c)
            return struct.pack(">BHHB", prec, h, w, len(comps)) + b"".join(bytes(x) for x in comps)
        return fn

    good = assemble(header(W, H), iv)
    out = {"no SOI": (b"\x89PNG" + good[4:], "no SOI"),
           "a segment past the end of the file": (good[:40], "runs past the end"),
           "SOF1": (swap(0xC0, 0xC1), "SOF1"), "SOF2": (swap(0xC0, 0xC2), r"SOF2 \(progressive\)"), "SOF3": (swap(0xC0, 0xC3), "SOF3"),
           "SOF9": (swap(0xC0, 0xC9), "SOF9"), "SOF10": (swap(0xC0, 0xCA), "SOF10"), "SOF15": (swap(0xC0, 0xCF), "SOF15"),
           "12-bit samples": (edit(0xC0, sof(prec=12)), "precision 12"),
           "16-bit quantisation table": (edit(0xDB, lambda p: bytes([0x10]) + bytes(128)), "Pq = 1"),
           "missing DQT": (edit(0xC0, sof(tq={1: 2})), "DQT table 2, which is missing"),
           "missing DC table": (edit(0xDA, lambda p: p[:2] + b"\x10" + p[3:]), "DC DHT table 1, which is missing"),
           "missing AC table": (edit(0xDA, lambda p: p[:4] + b"\x03" + p[5:]), "AC DHT table 3, which is missing"),
           "no DHT at all": (drop(0xC4), "DHT table 0, which is missing"),
           "DHT over-subscribed": (edit(0xC4, lambda p: p[:1] + bytes([3]) + p[2:]), "over-subscribe"),
           "DHT of more than 256 symbols": (edit(0xC4, lambda p: bytes([0x00]) + bytes([0] * 8 + [255, 2] + [0] * 6) + bytes(257)), "257 symbols"),
           "DC symbol above 15": (edit(0xC4, lambda p: p[:17] + bytes([16]) + p[18:]), "DC symbol above 15"),
           "height 0": (edit(0xC0, sof(h=0)), "height 0"), "width 0": (edit(0xC0, sof(w=0)), "width 0"),
           "width above MAX_SIDE": (edit(0xC0, sof(w=40000)), "width 40000"), "height above MAX_SIDE": (edit(0xC0, sof(h=32768)), "height 32768"),
           "two components": (edit(0xC0, sof(c=2)), "2 components"), "four components": (edit(0xC0, sof(c=4)), "4 components"),
           "a scan of one component": (edit(0xDA, lambda p: b"\x01" + p[1:3] + p[-3:]), "1 of 3 components"),
           "components out of frame order": (edit(0xDA, lambda p: p[:1] + p[3:5] + p[1:3] + p[5:]), "frame order"),
           "Ss not 0": (edit(0xDA, lambda p: p[:-3] + b"\x01\x3f\x00"), "Ss 1"), "Se not 63": (edit(0xDA, lambda p: p[:-3] + b"\x00\x05\x00"), "Se 5"),
           "successive approximation": (edit(0xDA, lambda p: p[:-1] + b"\x10"), "Ah/Al 16"),
           "luma 1x2": (edit(0xC0, sof(sampling={0: 0x12})), r"sampling factors \[\(1, 2\)"),
           "luma 4x1": (edit(0xC0, sof(sampling={0: 0x41})), r"sampling factors \[\(4, 1\)"),
           "chroma 2x1": (edit(0xC0, sof(sampling={1: 0x21})), r"sampling factors \[\(2, 2\), \(2, 1\)"),
           "one component at 2x2": (assemble([(m, sof(sampling={0: 0x22})(p) if m == 0xC0 else p) for m, p in header(W, H, C=1, hs=1, vs=1)], iv),
                                    r"sampling factors \[\(2, 2\)\]"),
           "Adobe transform 0 without JFIF": (assemble([(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")] + header(W, H, jfif=False), iv), "Adobe transform 0"),
           "no marker and ids R G B": (assemble(header(W, H, jfif=False, ids=(82, 71, 66)), iv), r"component ids \[82, 71, 66\]")}
    return out
