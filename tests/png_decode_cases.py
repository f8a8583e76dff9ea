"""Files shared by the PNG decoder tests (tests/test_png_decode_cpu.py, tests/test_gpu_png_decode.py): seeded, built once, left unchanged.

Every file is built from a known image -- png_cases.cases() and the additions below -- so the expected pixels are the input and nothing
depends on Pillow.  Streams come from stdlib zlib over levels, strategies and window sizes; what zlib cannot produce (a distance of 32768,
a lone distance code, none, stored blocks of LEN 0 and 65535, a block header across an IDAT boundary) is assembled by BitWriter from a
token list.  describe() is a plain-loop inflater written from RFC 1951 that reports what a stream contains, so that a test can assert
that the corpus reaches the paths it is meant to reach.  malformed() holds one small file per status code of csrc/png_inflate.h."""
import functools
import heapq
import struct
import zlib

import numpy as np

from tests import png_cases as PC

SIGNATURE = b"\x89PNG\r\n\x1a\n"
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# status codes of csrc/png_inflate.h
(OK, IDAT_CRC, ZLIB_HEADER, BLOCK_TYPE, STORED_LEN, CODE_SET, REPEAT, NO_END, SYMBOL, DISTANCE, TRUNCATED, TOO_MANY, TOO_FEW, ADLER, BEHIND,
 FILTER) = range(16)


# ---- the container ------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


ANCILLARY = [chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)),
             chunk(b"tEXt", b"Comment\x00a test file"), chunk(b"tIME", struct.pack(">HBBBBB", 2024, 2, 29, 12, 0, 0))]


def make_file(W, H, C, stream, cuts=(), before=(), behind=(), empty=False):
    """A PNG file around `stream`: IDAT chunks cut at the byte offsets `cuts`, with empty IDATs in between when `empty`, the chunks
    `before` ahead of the first IDAT and `behind` ahead of IEND."""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < len(stream))) + [len(stream)]
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0))] + list(before)
    if empty:
        out.append(chunk(b"IDAT", b""))
    for lo, hi in zip(edges[:-1], edges[1:]):
        out.append(chunk(b"IDAT", stream[lo:hi]))
        if empty:
            out.append(chunk(b"IDAT", b""))
    return b"".join(out + list(behind) + [chunk(b"IEND", b"")])


def filter_with(img, types):
    """uint8 [C,H,W] filtered with the given filter type per row -> uint8 [H, 1 + W*C]."""
    C, H, W = img.shape
    x = img.transpose(1, 2, 0).reshape(H, W * C).astype(np.int64)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :-C]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255
    t = np.asarray(types, dtype=np.int64)
    rows = cand[t, np.arange(H)]
    return np.concatenate([t[:, None], rows], 1).astype(np.uint8)


def filtered(img, mode):
    """mode: 0 .. 4 forced on every row, 'cycle' (row y gets y % 5), 'own' (the project's filter_rows choice)."""
    H = img.shape[1]
    if mode == "own":
        return _own_filter(img)
    return filter_with(img, [y % 5 for y in range(H)] if mode == "cycle" else [mode] * H)


def _own_filter(img):
    """The project's rule (minimum sum of min(v, 256 - v), ties to the lowest type) by filter_with -- the vectorised filter_reference."""
    H = img.shape[1]
    cands = np.stack([filter_with(img, [f] * H)[:, 1:].astype(np.int64) for f in range(5)])
    score = np.minimum(cands, 256 - cands).sum(2)
    return filter_with(img, score.argmin(0))


# ---- a bit writer and blocks from token lists ------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.bits, self.n, self.out = 0, 0, bytearray()

    def put(self, value, count):                       # LSB first (header fields, extra bits)
        self.bits |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.bits & 255)
            self.bits >>= 8
            self.n -= 8

    def code(self, code, length):                      # a Huffman code: MSB first
        self.put(int(format(code, f"0{length}b")[::-1], 2) if length else 0, length)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def raw(self, data):
        self.align()
        self.out += data


def canonical(lens):
    """RFC 1951 3.2.2: code lengths -> codes (whatever the set: an over-subscribed one gives codes nobody will read)."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


def huffman_lengths(counts, n):
    """Huffman code lengths of symbols 0 .. n-1 with the given counts (a dict); a lone symbol gets a partner so that the code is complete."""
    used = sorted(s for s, c in counts.items() if c)
    lens = [0] * n
    if len(used) == 1:
        lens[used[0]] = 1
        lens[0 if used[0] else 1] = 1
        return lens
    heap = [(counts[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        c1, k1, m1 = heapq.heappop(heap)
        c2, k2, m2 = heapq.heappop(heap)
        for s in m1 + m2:
            lens[s] += 1
        heapq.heappush(heap, (c1 + c2, min(k1, k2), m1 + m2))
    assert max(lens) <= 15
    return lens


def len_symbol(length):
    s = max(i for i in range(29) if LBASE[i] <= length) if length < 258 else 28
    return 257 + s, LEXT[s], length - LBASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, DEXT[s], dist - DBASE[s]


def put_tokens(bw, tokens, litlens, distlens, end=True):
    """tokens: ints (literals), (length, distance) pairs, or ('lit', symbol) / ('dist', symbol) for a raw symbol without extra bits."""
    lc, dc = canonical(litlens), canonical(distlens)
    for t in tokens:
        if isinstance(t, int):
            bw.code(lc[t], litlens[t])
        elif t[0] == "lit":
            bw.code(lc[t[1]], litlens[t[1]])
        elif t[0] == "dist":
            bw.code(dc[t[1]], distlens[t[1]])
        else:
            s, nb, v = len_symbol(t[0])
            bw.code(lc[s], litlens[s])
            bw.put(v, nb)
            s, nb, v = dist_symbol(t[1])
            bw.code(dc[s], distlens[s])
            bw.put(v, nb)
    if end:
        bw.code(lc[256], litlens[256])


def stored_block(bw, data, final=False, nlen=None):
    bw.put(1 if final else 0, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    bw.out += data


def fixed_block(bw, tokens, final=False, end=True):
    bw.put(1 if final else 0, 1)
    bw.put(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST, end)


def dynamic_block(bw, tokens, final=False, litlens=None, distlens=None, hdist=None, cl_lens=None, length_syms=None, end=True):
    """A dynamic block.  Left to itself it takes Huffman lengths from the tokens and writes every length as a plain symbol 0 .. 15 under a
    Huffman code-length code.  litlens / distlens (lists), cl_lens (19) and length_syms ([(symbol, extra value)]) override each part."""
    if litlens is None or distlens is None:
        lcount, dcount = {256: 1}, {}
        for t in tokens:
            if isinstance(t, int):
                lcount[t] = lcount.get(t, 0) + 1
            else:
                s = len_symbol(t[0])[0]
                lcount[s] = lcount.get(s, 0) + 1
                s = dist_symbol(t[1])[0]
                dcount[s] = dcount.get(s, 0) + 1
        litlens = huffman_lengths(lcount, 286) if litlens is None else litlens
        if distlens is None:
            distlens = huffman_lengths(dcount, 30) if dcount else [0] * 30
    hlit = max(257, max(i for i, l in enumerate(litlens) if l) + 1)
    if hdist is None:
        hdist = max([1] + [i + 1 for i, l in enumerate(distlens) if l])
    seq = list(litlens[:hlit]) + list(distlens[:hdist])
    if length_syms is None:
        length_syms = [(l, 0) for l in seq]
    if cl_lens is None:
        cc = {}
        for s, _ in length_syms:
            cc[s] = cc.get(s, 0) + 1
        cl_lens = huffman_lengths(cc, 19)
        assert max(cl_lens) <= 7
    bw.put(1 if final else 0, 1)
    bw.put(2, 2)
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(15, 4)
    for s in ORDER:
        bw.put(cl_lens[s], 3)
    cc = canonical(cl_lens)
    for s, v in length_syms:
        bw.code(cc[s], cl_lens[s])
        bw.put(v, {16: 2, 17: 3, 18: 7}.get(s, 0))
    put_tokens(bw, tokens, list(litlens) + [0] * (288 - len(litlens)), list(distlens) + [0] * (32 - len(distlens)), end)


def zlib_wrap(deflate, data, cmf=0x78, flg=None, adler=None):
    if flg is None:
        flg = (31 - (cmf * 256) % 31) % 31
    return bytes([cmf, flg]) + bytes(deflate) + struct.pack(">I", zlib.adler32(bytes(data)) & 0xFFFFFFFF if adler is None else adler)


# ---- what a stream contains: a plain-loop inflater from RFC 1951 ----------------------------------------------------------------------------
def describe(stream):
    """-> dict(kinds=set of block types, blocks, max_lit_code, max_dist_code, max_match, max_dist, overlap (a match longer than its distance),
    dist1_overlap, lone_dist (a dynamic block with one distance code of length 1), no_dist (with none), stored_lens (set), out (bytes))."""
    data, pos = bytes(stream), 16                       # bit position; the 2-byte header is not examined here
    info = dict(kinds=set(), blocks=0, max_lit_code=0, max_dist_code=0, max_match=0, max_dist=0, overlap=False, dist1_overlap=False,
                lone_dist=False, no_dist=False, stored_lens=set(), block_starts=[])
    out = bytearray()

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((data[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def table(lens):
        return {(l, c): s for s, (l, c) in enumerate(zip(lens, canonical(lens))) if l}

    def symbol(tab):
        nonlocal pos
        code = 0
        for l in range(1, 16):
            code = (code << 1) | ((data[pos >> 3] >> (pos & 7)) & 1)
            pos += 1
            s = tab.get((l, code))
            if s is not None:
                return s, l
        raise ValueError("no code owns these bits")

    while True:
        info["block_starts"].append(pos)
        final, kind = bits(1), bits(2)
        info["kinds"].add(kind)
        info["blocks"] += 1
        if kind == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            assert n ^ nn == 0xFFFF
            info["stored_lens"].add(n)
            out += data[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        else:
            if kind == 1:
                lt, dt = table(FIXED_LIT), table(FIXED_DIST)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[ORDER[i]] = bits(3)
                ct, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s, _ = symbol(ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    elif s == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                assert len(lens) == hlit + hdist
                dl = lens[hlit:]
                info["lone_dist"] |= sorted(l for l in dl if l) == [1]
                info["no_dist"] |= not any(dl)
                lt, dt = table(lens[:hlit]), table(dl)
            while True:
                s, l = symbol(lt)
                info["max_lit_code"] = max(info["max_lit_code"], l)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                length = LBASE[s - 257] + bits(LEXT[s - 257])
                d, l = symbol(dt)
                info["max_dist_code"] = max(info["max_dist_code"], l)
                dist = DBASE[d] + bits(DEXT[d])
                assert dist <= len(out)
                info["max_match"] = max(info["max_match"], length)
                info["max_dist"] = max(info["max_dist"], dist)
                info["overlap"] |= length > dist
                info["dist1_overlap"] |= dist == 1 and length > 1
                start = len(out) - dist
                if dist >= length:
                    out += out[start:start + length]
                else:
                    for k in range(length):
                        out.append(out[start + k])
        if final:
            break
    info["out"] = bytes(out)
    return info


# ---- the good corpus --------------------------------------------------------------------------------------------------------------------------
SETTINGS = [("l0", 0, zlib.Z_DEFAULT_STRATEGY, 15), ("l1", 1, zlib.Z_DEFAULT_STRATEGY, 15), ("l6", 6, zlib.Z_DEFAULT_STRATEGY, 15),
            ("l9", 9, zlib.Z_DEFAULT_STRATEGY, 15), ("fixed", 6, zlib.Z_FIXED, 15), ("rle", 6, zlib.Z_RLE, 15),
            ("huff", 6, zlib.Z_HUFFMAN_ONLY, 15), ("filtered", 6, zlib.Z_FILTERED, 15), ("w9", 6, zlib.Z_DEFAULT_STRATEGY, 9)]
FILTER_MODES = [0, 1, 2, 3, 4, "cycle", "own"]
SMALL = ["1x1x", "1x7x", "7x1x", "67x5x", "130x3x", "zeros64x", "full64x"]


def deflate(raw, setting):
    _, level, strategy, wbits = setting
    z = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return z.compress(bytes(raw)) + z.flush()


def _chunking(stream, k):
    """The k-th way of cutting a stream into IDAT chunks and surrounding it."""
    k %= 5
    if k == 0:
        return dict()
    if k == 1:
        return dict(cuts=range(7, len(stream), 7))
    if k == 2:
        return dict(cuts=range(8191, len(stream), 8191))
    if k == 3:
        return dict(cuts=range(7, len(stream), 7), empty=True)
    return dict(before=ANCILLARY[:3], behind=ANCILLARY[3:], cuts=(len(stream) // 2,))


def fibonacci_image():
    """Grey 561 x 216 whose 121 392 stream bytes (filter 0) have the first 24 Fibonacci numbers as byte counts, shuffled: any length-limited
    Huffman coder must give 15-bit codes."""
    rng = np.random.default_rng(77)
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    H, RB = 216, 561
    assert sum(fib) == H * (RB + 1)
    counts = [int(c) for c in rng.permutation(fib)]
    big = counts.index(max(counts))
    counts[0], counts[big] = counts[big], counts[0]                  # byte 0 holds the 216 filter bytes
    counts[0] -= H
    body = rng.permutation(np.repeat(np.arange(24, dtype=np.uint8), counts))
    return body.reshape(1, H, RB)


def _grey_from_raw(raw, RB):
    """raw: stream bytes of filter-0 rows of 1 + RB bytes -> uint8 [1,H,RB]."""
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(-1, RB + 1)
    assert not rows[:, 0].any()
    return rows[:, 1:].copy()[None]


def _hand_streams():
    """name -> (W, H, C, zlib stream, image [C,H,W], extra cuts): what stdlib zlib cannot produce."""
    out = {}
    rng = np.random.default_rng(91)

    def raw_rows(H, RB):
        r = rng.integers(0, 256, (H, RB + 1), dtype=np.uint8)
        r[:, 0] = 0
        return r

    # a match of 258 at distance exactly 32768: rows of 256 stream bytes, row 128 starts with a copy of the stream's first 258 bytes
    r = raw_rows(130, 255).reshape(-1)
    r[32768:32768 + 258] = r[:258]
    raw = r.tobytes()
    bw = BitWriter()
    stored_block(bw, raw[:32768])
    fixed_block(bw, [(258, 32768)] + list(raw[32768 + 258:33100]))
    dynamic_block(bw, list(raw[33100:]), final=True)
    bw.align()
    out["dist32768"] = (255, 130, 1, zlib_wrap(bw.out, raw), _grey_from_raw(raw, 255), ())

    # one distance code of length 1 (distance symbol 3, an incomplete set zlib accepts), and none at all
    r = raw_rows(6, 19).reshape(-1)
    r[36] = 0                                                        # a match of 20 at distance 4 over row 2: byte 40, a filter byte, copies byte 36
    for k in range(20):
        r[40 + k] = r[36 + k]
    raw = r.tobytes()
    assert raw[40:60] == raw[36:56]
    bw = BitWriter()
    dl = [0] * 30
    dl[3] = 1
    dynamic_block(bw, list(raw[:40]) + [(20, 4)] + list(raw[60:]), final=True, distlens=dl)
    bw.align()
    out["lone_distance_code"] = (19, 6, 1, zlib_wrap(bw.out, raw), _grey_from_raw(raw, 19), ())
    bw = BitWriter()
    dynamic_block(bw, list(raw), final=True)
    bw.align()
    out["no_distance_code"] = (19, 6, 1, zlib_wrap(bw.out, raw), _grey_from_raw(raw, 19), ())

    # stored blocks of LEN 65535 and LEN 0, then more
    raw = raw_rows(260, 255).tobytes()
    bw = BitWriter()
    stored_block(bw, raw[:65535])
    stored_block(bw, b"")
    fixed_block(bw, list(raw[65535:65600]))
    stored_block(bw, raw[65600:], final=True)
    out["stored_0_and_65535"] = (255, 260, 1, zlib_wrap(bw.out, raw), _grey_from_raw(raw, 255), ())

    # a dynamic block's header across an IDAT boundary: the cut falls inside its first 17 bits
    raw = raw_rows(4, 30).tobytes()
    bw = BitWriter()
    fixed_block(bw, list(raw[:50]))
    at = bw.bitpos
    dynamic_block(bw, list(raw[50:]), final=True)
    bw.align()
    cut = 2 + at // 8 + 1                                             # the zlib header's 2 bytes; the byte behind the one the block starts in
    assert at % 8 and (at + 17) // 8 >= at // 8 + 1
    out["header_across_idat"] = (30, 4, 1, zlib_wrap(bw.out, raw), _grey_from_raw(raw, 30), (cut,))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> (file bytes, image uint8 [C,H,W], zlib stream)."""
    out = {}
    cases = PC.cases()
    for C in (1, 3):
        for i, stem in enumerate(SMALL):
            img = cases[stem + str(C)]
            H, W = img.shape[1:]
            for j, mode in enumerate(FILTER_MODES):
                raw = filtered(img, mode).tobytes()
                for k in ((i + j) % 9, (i + j + 4) % 9):
                    stream = deflate(raw, SETTINGS[k])
                    how = _chunking(stream, i + 2 * j + k + C)
                    out[f"{stem}{C}-f{mode}-{SETTINGS[k][0]}-c{(i + 2 * j + k + C) % 5}"] = (make_file(W, H, C, stream, **how), img, stream)
    large = [("noise256x3", "own", 0, 2), ("ramp256x3", "own", 3, 0), ("dither256x3", 4, 7, 2), ("half_plane512", 1, 5, 0),
             ("long22000x2x3", "cycle", 1, 2), ("dither1200x4x3", 3, 6, 4), ("half_plane512", 2, 2, 4), ("zeros64x3", 0, 2, 0)]
    for name, mode, k, how in large:
        img = cases[name]
        C, H, W = img.shape
        stream = deflate(filtered(img, mode).tobytes(), SETTINGS[k])
        out[f"{name}-f{mode}-{SETTINGS[k][0]}-c{how}"] = (make_file(W, H, C, stream, **_chunking(stream, how)), img, stream)
    fib = fibonacci_image()
    raw = filtered(fib, 0).tobytes()
    for k in (6, 2):
        stream = deflate(raw, SETTINGS[k])
        out[f"fibonacci-{SETTINGS[k][0]}"] = (make_file(561, 216, 1, stream, cuts=range(8191, len(stream), 8191)), fib, stream)
    for name, (W, H, C, stream, img, cuts) in _hand_streams().items():
        out["hand-" + name] = (make_file(W, H, C, stream, cuts=cuts), img, stream)
    for name, (f, img, stream) in list(out.items()):                   # every file of at most 100 stream bytes again, in 1-byte IDAT chunks
        if len(stream) <= 100:
            C, H, W = img.shape
            out[name + "-bytes"] = (make_file(W, H, C, stream, cuts=range(1, len(stream))), img, stream)
    for f, img, s in out.values():
        img.setflags(write=False)
    return out


def expected_raw(name):
    """The filtered data the stream of corpus()[name] must inflate to, by stdlib zlib (the arbiter)."""
    return zlib.decompress(corpus()[name][2])


# ---- the malformed corpus -----------------------------------------------------------------------------------------------------------------------
def arbiter(stream, expect):
    """zlib's verdict: the bytes when zlib ends at eof with no error and no unused data and gives `expect` bytes, else None."""
    z = zlib.decompressobj(15)
    try:
        raw = z.decompress(bytes(stream))
    except zlib.error:
        return None
    if not z.eof or z.unused_data or len(raw) != expect:
        return None
    return raw


@functools.lru_cache(maxsize=None)
def malformed():
    """name -> (file bytes, status, zlib stream or None, expected inflated length): one small file per status code, a few for the codes with
    several causes.  The image is 19 x 6 grey (120 stream bytes) unless the case is about sizes."""
    rng = np.random.default_rng(5)
    W, H = 19, 6
    rows = rng.integers(0, 4, (H, W + 1), dtype=np.uint8) * 60
    rows[:, 0] = 0
    raw = rows.tobytes()
    n = len(raw)
    good = zlib.compress(raw, 6)
    out = {}

    def add(name, status, stream, expect=n, w=W, h=H, **how):
        out[name] = (make_file(w, h, 1, bytes(stream), **how), status, bytes(stream), expect)

    # container level: the CRC of the second IDAT chunk
    f = bytearray(make_file(W, H, 1, good, cuts=(10, 20)))
    second = f.index(b"IDAT", f.index(b"IDAT") + 4)
    f[second + 4 + 10] ^= 0x40                                        # the first byte of its CRC
    out["idat_crc"] = (bytes(f), IDAT_CRC | (1 << 8), None, n)
    body = good[2:-4]
    add("zlib_cm", ZLIB_HEADER, zlib_wrap(body, raw, cmf=0x77))
    add("zlib_cinfo", ZLIB_HEADER, zlib_wrap(body, raw, cmf=0x88))
    add("zlib_fcheck", ZLIB_HEADER, zlib_wrap(body, raw, flg=0x02))
    add("zlib_fdict", ZLIB_HEADER, zlib_wrap(body, raw, flg=0x20 + (31 - (0x78 * 256 + 0x20) % 31) % 31))

    def hand(build):
        bw = BitWriter()
        build(bw)
        bw.align()
        return zlib_wrap(bw.out, raw)

    add("block_type_3", BLOCK_TYPE, hand(lambda bw: (bw.put(1, 1), bw.put(3, 2))))
    add("stored_nlen", STORED_LEN, hand(lambda bw: stored_block(bw, raw, final=True, nlen=0x1234)))
    toks = list(raw)
    cl_over = [3] * 19                                               # 19 codes of 3 bits: over-subscribed
    add("code_length_code_oversubscribed", CODE_SET, hand(lambda bw: dynamic_block(bw, toks, final=True, cl_lens=cl_over)))
    cl_inc = [0] * 19
    cl_inc[0] = cl_inc[8] = 2                                        # two codes of 2 bits: incomplete
    add("code_length_code_incomplete", CODE_SET,
        hand(lambda bw: dynamic_block(bw, [], final=True, cl_lens=cl_inc, litlens=[8] * 257, distlens=[0] * 30)))
    add("literal_set_oversubscribed", CODE_SET, hand(lambda bw: dynamic_block(bw, [], final=True, litlens=[7] * 257, distlens=[0] * 30, end=False)))
    dl = [0] * 30
    dl[0] = dl[1] = 2
    add("distance_set_incomplete", CODE_SET, hand(lambda bw: dynamic_block(bw, toks, final=True, distlens=dl, litlens=_lit_lengths(toks))))
    cl = [0] * 19
    cl[16] = cl[8] = 1
    add("repeat_without_previous", REPEAT,
        hand(lambda bw: dynamic_block(bw, [], final=True, cl_lens=cl, litlens=[8] * 257, distlens=[0] * 30, length_syms=[(16, 0)] * 90, end=False)))
    cl2 = [0] * 19
    cl2[18] = cl2[8] = 1
    add("repeat_past_the_end", REPEAT,
        hand(lambda bw: dynamic_block(bw, [], final=True, cl_lens=cl2, litlens=[8] * 257, distlens=[0] * 30,
                                      length_syms=[(8, 0)] * 200 + [(18, 127)], end=False)))
    no_end = [8] * 256 + [0]
    add("no_end_of_block", NO_END, hand(lambda bw: dynamic_block(bw, [], final=True, litlens=no_end + [0] * 28 + [8], distlens=[0] * 30, end=False)))
    add("literal_symbol_286", SYMBOL, hand(lambda bw: fixed_block(bw, toks[:5] + [("lit", 286)], final=True)))
    add("distance_symbol_30", SYMBOL, hand(lambda bw: fixed_block(bw, toks[:5] + [("lit", 257), ("dist", 30)], final=True)))
    add("hlit_declares_287", SYMBOL, hand(lambda bw: dynamic_block(bw, [], final=True, litlens=[9] * 287, distlens=[0] * 30, end=False)))
    add("distance_before_start", DISTANCE, hand(lambda bw: fixed_block(bw, toks[:5] + [(3, 6)] + toks[8:], final=True)))
    add("truncated_in_block", TRUNCATED, good[:len(good) - 9])
    add("truncated_in_adler", TRUNCATED, good[:len(good) - 2])
    add("too_many", TOO_MANY, good, expect=(W + 1) * (H - 1), h=H - 1)
    add("too_few", TOO_FEW, good, expect=(W + 1) * (H + 1), h=H + 1)
    add("adler", ADLER, good[:-1] + bytes([good[-1] ^ 1]))
    add("bytes_behind", BEHIND, good + b"\x00")
    bad = bytearray(raw)
    bad[3 * (W + 1)] = 5
    out["filter_type_5"] = (make_file(W, H, 1, zlib.compress(bytes(bad), 6)), FILTER, None, n)
    return out


def _lit_lengths(tokens):
    c = {256: 1}
    for t in tokens:
        c[t] = c.get(t, 0) + 1
    return huffman_lengths(c, 286)
