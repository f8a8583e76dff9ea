"""8-bit PNG files from device tensors and back: the write side of the files frame ingest reads, and (at the end of the module) their read side.

Every stage of the reference that produces images ends in 8-bit PNG files: render_results (its trainers/eval_metric.py:95-126) writes render,
ground truth and 1 - hand mask for every frame, and the end of each static phase (trainers/train_static.py:183-197) one predicted mask per
static frame.  The sweeps here already hand those bytes back on the device (EvalPass `images`, MaskPass `masks`); this module turns them into
file bytes there (csrc/png.hip, include/egs_raster.h egs_png_encode) so that the host only copies and writes.

    filter_rows       the filtered stream of an image, in torch integer ops on any device: the DEFINITION the kernel answers to, byte for byte
    encode_statement  a valid file from filter_rows and stdlib zlib, one full flush per segment: the host statement of the container and the
                      yardstick for sizes (and the CPU route: the kernel has none)
    decode            a minimal strict reader (stdlib zlib and struct): signature, chunk order, every CRC, the IHDR fields, the inflated
                      length, filter bytes <= 4; unfilters and returns the array.  The tests use it: nothing depends on Pillow
    encode            device uint8 [F,C,H,W] or [F,H,W] -> (buf uint8 [F, bound], sizes int32 [F]) by the kernel
    PngWriter         owns buf, scratch and pinned staging; save(images, paths) encodes batch by batch, reads each batch's sizes once, copies
                      the used prefix of each slot and writes the files from a small thread pool

    parse             the host's share of READING a file, O(chunks): signature, chunk walk, the small chunks' CRCs, IHDR -> (W, H, C, IDAT table)
    PngReader         file bytes -> device uint8 [h,w,C] by the kernels (csrc/png_decode.hip, csrc/png_inflate.h: CRC, inflate, unfilter and
                      every check of the stream on the device, one status word per file); decode_device for a single file

The file: signature, IHDR (bit depth 8, colour type 0 or 2, no interlace), IDAT ..., IEND.  The IDAT payloads together are one zlib stream
of the filtered data -- H rows of a filter-type byte and the W C filtered bytes of the interleaved row.  The filter type is libpng's
minimum-sum heuristic stated exactly: filters 0 .. 4 on the raw neighbours (0 where they do not exist), score = sum of min(v, 256 - v), the
lowest score wins, ties go to the lowest type.  The stream is compressed in independent segments (one per row; a row of more than
SEGMENT_BYTES stream bytes in pieces of SEGMENT_BYTES), each ending on a byte boundary and each an IDAT chunk of its own.
"""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import lib as _lib
from . import _hip
from .file_reader import DeviceFileReader, _up

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SEGMENT_BYTES = 4096          # csrc/png.hip PNG_SEG
FIXED_BYTES = 77              # signature 8, IHDR 25, zlib header chunk 14, final block + Adler-32 chunk 18, IEND 12
SEGMENT_EXTRA = 17            # chunk framing 12 + a stored block's header 5
MAX_SIDE = 32767
MAX_THREADS = 16


def _chw(image_u8):
    """uint8 [H,W] or [C,H,W], C in {1, 3} (torch or numpy) -> tensor [C,H,W]."""
    t = image_u8 if torch.is_tensor(image_u8) else torch.from_numpy(np.array(image_u8))                # (a copy: read-only arrays are welcome)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[0] not in (1, 3) or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"png: an image is uint8 [H,W] or [C,H,W] with C = 1 or 3 and sides >= 1; got {t.dtype} {tuple(t.shape)}")
    return t


def filter_rows(image_u8):
    """The filtered data of `image_u8` (uint8 [H,W] or [C,H,W], any device) -> uint8 [H, 1 + W*C]: per row the filter type, then the
    filtered bytes of the interleaved row, the type chosen by the rule in the module docstring."""
    t = _chw(image_u8)
    C, H, W = t.shape
    x = t.permute(1, 2, 0).reshape(H, W * C).to(torch.int32)
    a, b, c = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :-C]
    p = a + b - c
    pa, pb, pc = (p - a).abs(), (p - b).abs(), (p - c).abs()
    paeth = torch.where((pa <= pb) & (pa <= pc), a, torch.where(pb <= pc, b, c))
    cand = torch.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255                    # [5, H, W*C]
    score = torch.minimum(cand, 256 - cand).sum(2, dtype=torch.int64)                            # [5, H]
    best = score.min(0).values
    choice = torch.full((H,), 4, dtype=torch.int64, device=x.device)
    for f in (3, 2, 1, 0):
        choice = torch.where(score[f] == best, torch.full_like(choice, f), choice)
    rows = cand.gather(0, choice.view(1, H, 1).expand(1, H, W * C))[0]
    return torch.cat([choice.view(H, 1).to(torch.int32), rows], 1).to(torch.uint8)


def segments(height, row_bytes, segment_rows=1):
    """[(begin, end)] byte ranges of the filtered stream (rows of 1 + row_bytes): groups of `segment_rows` rows, a group longer than
    segment_rows * SEGMENT_BYTES cut into pieces of that size.  segment_rows = 1 is the kernel's segmentation."""
    rb, cut, out = row_bytes + 1, int(segment_rows) * SEGMENT_BYTES, []
    if segment_rows < 1:
        raise ValueError("png.segments: segment_rows >= 1")
    for y in range(0, height, segment_rows):
        lo, hi = y * rb, min(height, y + segment_rows) * rb
        out += [(s, min(hi, s + cut)) for s in range(lo, hi, cut)]
    return out


def bound(W, H, C):
    """Capacity of one image's slot (include/egs_raster.h egs_png_bound): the fixed chunks, the filtered data, and per segment the chunk
    framing and a stored block's header."""
    return FIXED_BYTES + H * (W * C + 1) + SEGMENT_EXTRA * H * -(-(W * C + 1) // SEGMENT_BYTES)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_statement(image_u8, segment_rows=1):
    """A valid PNG file (bytes) of `image_u8` built from filter_rows and zlib at its default level: one Z_FULL_FLUSH, and one IDAT chunk,
    per segment -- zlib restricted to the independence the kernel's workgroups have -- then the final block and the Adler-32 in a last
    IDAT chunk."""
    t = _chw(image_u8)
    C, H, W = t.shape
    stream = filter_rows(t).cpu().numpy().tobytes()
    z = zlib.compressobj(6, zlib.DEFLATED, 15)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0))]
    for lo, hi in segments(H, W * C, segment_rows):
        out.append(_chunk(b"IDAT", z.compress(stream[lo:hi]) + z.flush(zlib.Z_FULL_FLUSH)))
    out += [_chunk(b"IDAT", z.flush(zlib.Z_FINISH)), _chunk(b"IEND", b"")]
    return b"".join(out)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def inflate(file_bytes):
    """The checks of decode() up to the filtered data -> (W, H, C, filtered uint8 [H, 1 + W*C])."""
    data = bytes(file_bytes)
    if data[:8] != SIGNATURE:
        raise ValueError("png.decode: no PNG signature")
    pos, kinds, idat, ihdr = 8, [], [], None
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("png.decode: a truncated chunk header")
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise ValueError(f"png.decode: chunk {kind!r} runs past the end of the file")
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"png.decode: wrong CRC-32 in chunk {kind!r} at byte {pos}")
        kinds.append(kind)
        if kind == b"IHDR":
            ihdr = body
        elif kind == b"IDAT":
            idat.append(body)
        pos += 12 + n
        if kind == b"IEND":
            break
    if pos != len(data):
        raise ValueError("png.decode: bytes behind IEND")
    if len(kinds) < 3 or kinds[0] != b"IHDR" or kinds[-1] != b"IEND" or any(k != b"IDAT" for k in kinds[1:-1]):
        raise ValueError(f"png.decode: the chunks must be IHDR, IDAT ..., IEND; got {kinds[:4]} ... {kinds[-2:]}")
    if len(ihdr) != 13:
        raise ValueError("png.decode: IHDR is 13 bytes")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ihdr)
    if depth != 8 or colour not in (0, 2) or comp or filt or lace or W < 1 or H < 1:
        raise ValueError(f"png.decode: IHDR {(W, H, depth, colour, comp, filt, lace)} is not an 8-bit grey or RGB image without interlace")
    C = 3 if colour == 2 else 1
    z = zlib.decompressobj(15)
    try:
        raw = z.decompress(b"".join(idat))
    except zlib.error as e:                                              # (a wrong Adler-32 arrives here)
        raise ValueError(f"png.decode: {e}") from None
    if not z.eof:
        raise ValueError("png.decode: the zlib stream is truncated")
    if z.unused_data:
        raise ValueError("png.decode: bytes behind the zlib stream")
    if len(raw) != H * (1 + W * C):
        raise ValueError(f"png.decode: {len(raw)} inflated bytes, the image needs {H * (1 + W * C)}")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + W * C)
    if int(rows[:, 0].max()) > 4:
        raise ValueError(f"png.decode: filter type {int(rows[:, 0].max())}")
    return W, H, C, rows


def decode(file_bytes):
    """Strict reader of the files this module writes -> numpy uint8 [H,W] (colour type 0) or [3,H,W] (colour type 2).  ValueError for a
    wrong signature, chunk order, CRC-32, IHDR field, a truncated or overlong stream, a wrong Adler-32, a filter type above 4."""
    W, H, C, rows = inflate(file_bytes)
    out = np.zeros((H, W * C), dtype=np.uint8)
    prev = np.zeros(W * C, dtype=np.int64)
    for y in range(H):
        f, r = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if f == 0:
            cur = r
        elif f == 1:
            cur = np.cumsum(r.reshape(W, C), axis=0).reshape(-1) & 255
        elif f == 2:
            cur = (r + prev) & 255
        else:
            line, up, res = [0] * (W * C), prev.tolist(), r.tolist()
            for j in range(W * C):
                a = line[j - C] if j >= C else 0
                if f == 3:
                    pred = (a + up[j]) >> 1
                else:
                    pred = _paeth(a, up[j], up[j - C] if j >= C else 0)
                line[j] = (res[j] + pred) & 255
            cur = np.asarray(line, dtype=np.int64)
        out[y] = cur
        prev = cur
    img = out.reshape(H, W, C).transpose(2, 0, 1)
    return np.ascontiguousarray(img[0] if C == 1 else img)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def _device_images(images_u8, who):
    """uint8 [F,C,H,W] or [F,H,W] on a HIP device -> (tensor whose rows are dense, F, C, H, W, image_stride, plane_stride)."""
    t = images_u8
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{who}: images are on {getattr(t, 'device', 'the host')}: the PNG encoder has no CPU path "
                           "(png.encode_statement is the host statement)")
    if t.dim() == 3:
        t = t.unsqueeze(1)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] not in (1, 3) or t.shape[0] < 1:
        raise ValueError(f"{who}: images are uint8 [F,C,H,W] with C = 1 or 3, or [F,H,W]; got {t.dtype} {tuple(images_u8.shape)}")
    F, C, H, W = t.shape
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{who}: sides of 1 .. {MAX_SIDE}; got {W}x{H}")
    dense = t.stride(3) == 1 and t.stride(2) == W and (C == 1 or t.stride(1) >= H * W) and (F == 1 or t.stride(0) >= (C - 1) * t.stride(1) + H * W)
    if not dense:
        t = t.contiguous()
    return t, F, C, H, W, t.stride(0), t.stride(1)


def scratch_bytes(F, W, H, C):
    return int(_lib.load().egs_png_scratch_bytes(F, W, H, C))


def _launch(F, W, H, C, src_ptr, image_stride, plane_stride, out, sizes, scratch, dev):
    """out: uint8 [>= F, stride] rows; sizes: int32 [>= F]; both on dev.  Enqueues; nothing is read back."""
    with _hip.device_ctx(dev):
        _lib.check(_lib.load().egs_png_encode(F, W, H, C, src_ptr, int(image_stride), int(plane_stride), out.data_ptr(), out.stride(0),
                                              sizes.data_ptr(), scratch.data_ptr(), _hip.stream_of(dev)))


def encode(images_u8, out=None, sizes=None, scratch=None):
    """images_u8: uint8 [F,C,H,W] (C = 1 or 3) or [F,H,W] on a HIP device -> (buf uint8 [F, bound], sizes int32 [F]) on that device:
    buf[i, :sizes[i]] is image i's file.  Three launches, no synchronisation, nothing read back; with out / sizes / scratch given
    (buf of rows >= bound(W, H, C), int32 [F], uint8 [scratch_bytes(F, W, H, C)]) no allocation either: can be captured."""
    t, F, C, H, W, image_stride, plane_stride = _device_images(images_u8, "png.encode")
    dev = t.device
    cap = bound(W, H, C)
    if cap >= 1 << 31:
        raise ValueError(f"png.encode: a {W}x{H}x{C} file may exceed 2 GiB")
    if out is None:
        out = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    if sizes is None:
        sizes = torch.empty(F, dtype=torch.int32, device=dev)
    if scratch is None:
        scratch = torch.empty(scratch_bytes(F, W, H, C), dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] < F or out.shape[1] < cap or out.stride(1) != 1 or out.device != dev:
        raise ValueError(f"png.encode: out is uint8 [>= {F}, >= {cap}] on {dev}")
    if sizes.dtype != torch.int32 or sizes.numel() < F or not sizes.is_contiguous() or sizes.device != dev:
        raise ValueError(f"png.encode: sizes is a contiguous int32 [>= {F}] on {dev}")
    if scratch.dtype != torch.uint8 or scratch.numel() < scratch_bytes(F, W, H, C) or not scratch.is_contiguous() or scratch.device != dev:
        raise ValueError(f"png.encode: scratch is a contiguous uint8 [>= {scratch_bytes(F, W, H, C)}] on {dev}")
    _launch(F, W, H, C, t.data_ptr(), image_stride, plane_stride, out, sizes, scratch, dev)
    return out[:F], sizes[:F]


def _write(path, view):
    with open(path, "wb") as fh:
        fh.write(view)


class PngWriter:
    """Files of H x W images of C channels from a HIP device: owns the encoder's output slots and scratch for `batch` images and a pinned
    staging buffer of the same size.  The pool has `threads` workers (at most 16, never sized from the machine's CPU count)."""

    def __init__(self, H, W, C, device, batch=32, threads=8):
        self.H, self.W, self.C, self.batch = int(H), int(W), int(C), int(batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PngWriter: the PNG encoder has no CPU path (device {self.device}); png.encode_statement is the host statement")
        if self.C not in (1, 3) or self.batch < 1 or not (1 <= self.H <= MAX_SIDE) or not (1 <= self.W <= MAX_SIDE):
            raise ValueError("PngWriter: C = 1 or 3, batch >= 1, sides of 1 .. 32767")
        self.bound = bound(self.W, self.H, self.C)
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.buf = torch.empty((self.batch, self.bound), dtype=torch.uint8, device=self.device)
        self.sizes = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        self.scratch = torch.empty(scratch_bytes(self.batch, self.W, self.H, self.C), dtype=torch.uint8, device=self.device)
        self.staging = torch.empty((self.batch, self.bound), dtype=torch.uint8).pin_memory()
        self.host_reads = 0                                              # reads of `sizes` (one per batch)

    def save(self, images_u8, paths):
        """images_u8: uint8 [F,C,H,W] or [F,H,W] on the writer's device; paths: F file names.  Per batch: one encode, ONE read of the batch's
        sizes, one copy per image of the used prefix of its slot into pinned memory, then the files are written by the pool.
        -> the F file sizes (list of int)."""
        t, F, C, H, W, image_stride, plane_stride = _device_images(images_u8, "PngWriter.save")
        paths = [str(p) for p in paths]
        if (C, H, W) != (self.C, self.H, self.W) or t.device != self.device or len(paths) != F:
            raise ValueError(f"PngWriter.save: {F} images of {C}x{H}x{W} on {t.device} and {len(paths)} paths; the writer is for "
                             f"{self.C}x{self.H}x{self.W} on {self.device}, one path per image")
        written = []
        host = self.staging.numpy()
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            for lo in range(0, F, self.batch):
                n = min(self.batch, F - lo)
                _launch(n, W, H, C, t.data_ptr() + lo * image_stride, image_stride, plane_stride, self.buf, self.sizes, self.scratch, self.device)
                sz = self.sizes[:n].cpu().tolist()
                self.host_reads += 1
                for i in range(n):
                    self.staging[i, :sz[i]].copy_(self.buf[i, :sz[i]], non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
                list(pool.map(_write, paths[lo:lo + n], [memoryview(host[i])[:sz[i]] for i in range(n)]))      # (done before staging is reused)
                written += sz
        return written


# ---- the read side: file bytes go up as they are, the device inflates, checks and unfilters them (csrc/png_decode.hip) ------------------------
STATUS = {1: "wrong CRC-32 in an IDAT chunk", 2: "zlib header (CM, CINFO, FCHECK or FDICT)", 3: "block type 3", 4: "a stored block's LEN / NLEN",
          5: "a code-length code or a set of code lengths over-subscribed or incomplete", 6: "a repeat code with no previous length or past HLIT + HDIST",
          7: "no end-of-block code", 8: "literal/length symbol 286 / 287, distance symbol 30 / 31, or bits no code owns",
          9: "a distance reaching before the start of the output", 10: "the stream ends inside a block", 11: "more inflated bytes than H (1 + W C)",
          12: "fewer inflated bytes than H (1 + W C)", 13: "wrong Adler-32", 14: "bytes behind the zlib stream", 15: "a filter type above 4"}
_FILE = np.dtype([("width", "<i4"), ("height", "<i4"), ("channels", "<i4"), ("n_idat", "<i4"), ("idat_begin", "<u4"), ("stream_bytes", "<u4"),
                  ("file_offset", "<u8"), ("file_bytes", "<u8"), ("stream_offset", "<u8"), ("inflate_offset", "<u8"), ("out_offset", "<u8")])      # egs_png_file
_IDAT = np.dtype([("file", "<u4"), ("src", "<u4"), ("length", "<u4"), ("dst", "<u4")])                                                             # egs_png_idat
_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")
# egs_png_decode_ex: the flags, and the route words with EGS_PNG_SEGMENTS (1: the file's IDAT chunks were inflated as independent segments, a
# wave each; else 0 | reason << 8: why the serial wave inflated it)
SEGMENTS = 1
SEGMENT_MAX = 8192
ROUTE_SEGMENTS = 1
ROUTE_REASON = {0: "the segmented route was not asked for", 1: "chunk 0 is shorter than the zlib header", 2: "a chunk does not end on a block end",
                3: "a distance before the start of its segment", 4: f"a segment of more than {SEGMENT_MAX} bytes",
                5: "the final block or the Adler-32 is not at the end of the last non-empty chunk", 6: "the segments' lengths do not sum to H (1 + W C)",
                7: "the combined Adler-32", 8: "an inflate error inside a segment", 9: "an IDAT chunk's CRC-32"}


def route_text(word):
    """What a route word of egs_png_decode_ex says."""
    word = int(word)
    return "segments" if word == ROUTE_SEGMENTS else "serial: " + ROUTE_REASON.get(word >> 8, f"route {word}")


def status_text(word):
    """What a status word of egs_png_decode says."""
    word = int(word)
    if word == 0:
        return "ok"
    text = STATUS.get(word & 255, f"status {word}")
    return f"{text} (IDAT chunk {word >> 8})" if (word & 255) == 1 else text


def parse(file_bytes):
    """The host's share of reading a PNG file, O(number of chunks): signature, the chunk walk (lengths inside the file, IHDR first and 13
    bytes, IDAT chunks consecutive, IEND last and nothing behind it, no unknown critical chunk), the CRC-32 of IHDR, PLTE and IEND, the IHDR
    fields.  No IDAT byte is touched: their CRCs, the zlib stream and the filter types are the device's (png.PngReader).
    -> (W, H, C, [(offset, length)] of the IDAT payloads).  ValueError for every refusal; the modes frame ingest does not take (palette,
    alpha, 1 / 2 / 4 / 16 bits, interlace) name the field and carry ingest's advice."""
    from .ingest import _ADVICE
    data = file_bytes if isinstance(file_bytes, (bytes, bytearray, memoryview)) else bytes(file_bytes)
    n = len(data)
    if bytes(data[:8]) != SIGNATURE:
        raise ValueError("png.parse: no PNG signature")
    pos, idat, ihdr, state, ended = 8, [], None, 0, False               # state 0: before the IDATs, 1: inside, 2: behind
    while pos < n:
        if pos + 12 > n:
            raise ValueError(f"png.parse: a truncated chunk header at byte {pos}")
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + length > n:
            raise ValueError(f"png.parse: chunk {kind!r} at byte {pos} runs past the end of the file")
        if (ihdr is None) != (kind == b"IHDR"):
            raise ValueError(f"png.parse: IHDR must be the first chunk and the only one of its kind; chunk {kind!r} at byte {pos}")
        if kind in (b"IHDR", b"PLTE", b"IEND"):
            if struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])[0] != (zlib.crc32(data[pos + 4:pos + 8 + length]) & 0xFFFFFFFF):
                raise ValueError(f"png.parse: wrong CRC-32 in chunk {kind!r} at byte {pos}")
        if kind == b"IHDR":
            if length != 13:
                raise ValueError(f"png.parse: IHDR is 13 bytes, not {length}")
            ihdr = struct.unpack(">IIBBBBB", data[pos + 8:pos + 21])
        elif kind == b"IDAT":
            if state == 2:
                raise ValueError(f"png.parse: the IDAT chunks must be consecutive; another one at byte {pos}")
            state = 1
            idat.append((pos + 8, length))
        else:
            if kind not in _CRITICAL and not (kind[0] & 0x20):
                raise ValueError(f"png.parse: unknown critical chunk {kind!r} at byte {pos}")
            if state == 1:
                state = 2
        pos += 12 + length
        if kind == b"IEND":
            if length:
                raise ValueError("png.parse: IEND carries data")
            ended = True
            break
    if not ended:
        raise ValueError("png.parse: the file ends without an IEND chunk")
    if pos != n:
        raise ValueError("png.parse: bytes behind IEND")
    if not idat:
        raise ValueError("png.parse: no IDAT chunk")
    W, H, depth, colour, comp, filt, lace = ihdr
    if not 1 <= W <= MAX_SIDE:
        raise ValueError(f"png.parse: IHDR width {W} is outside 1 .. {MAX_SIDE}")
    if not 1 <= H <= MAX_SIDE:
        raise ValueError(f"png.parse: IHDR height {H} is outside 1 .. {MAX_SIDE}")
    if depth != 8:
        raise ValueError(f"png.parse: IHDR bit depth {depth}: this path reads 8-bit samples, Pillow resizes the other depths differently; {_ADVICE}")
    if colour not in (0, 2):
        raise ValueError(f"png.parse: IHDR colour type {colour} (palette or alpha): this path reads grey and RGB; {_ADVICE}")
    if comp:
        raise ValueError(f"png.parse: IHDR compression method {comp}")
    if filt:
        raise ValueError(f"png.parse: IHDR filter method {filt}")
    if lace:
        raise ValueError(f"png.parse: IHDR interlace method {lace}: interlaced files are not read here; {_ADVICE}")
    return W, H, 3 if colour == 2 else 1, idat


def plan(parsed, out_gap=0):
    """parsed: [(W, H, C, idat, file length)] -> dict(desc, idat: the two tables of egs_png_decode with files, streams, inflated data and outputs
    packed in order -- files at multiples of 16, outputs at multiples of 256 with `out_gap` bytes between them --, files_bytes, stream_bytes,
    inflate_bytes, out_bytes: the totals)."""
    desc = np.zeros(len(parsed), dtype=_FILE)
    idat = np.zeros(sum(len(p[3]) for p in parsed), dtype=_IDAT)
    fo = so = io = oo = k = 0
    for i, (W, H, C, chunks, nbytes) in enumerate(parsed):
        stream = sum(n for _, n in chunks)
        if nbytes >= 1 << 32 or stream >= 1 << 31:
            raise ValueError(f"png: file {i} has {nbytes} bytes, {stream} of them in IDAT chunks; the limit is 2 GiB")
        desc[i] = (W, H, C, len(chunks), k, stream, fo, nbytes, so, io, oo)
        at = 0
        for off, n in chunks:
            idat[k] = (i, off, n, at)
            at += n
            k += 1
        fo += _up(nbytes, 16)
        so += _up(stream, 16)
        io += _up(H * (1 + W * C), 16)
        oo += _up(H * W * C + out_gap, 256)
    return dict(desc=desc, idat=idat, files_bytes=fo, stream_bytes=so, inflate_bytes=io, out_bytes=oo)


class PngReader(DeviceFileReader):
    """8-bit PNG files -> device uint8 [h, w, C] tensors: the mirror of PngWriter, and DeviceFileReader's contract (file_reader.py: the
    buffers, the batches, one upload and one read of the status words per batch, the guard bytes).  Per batch the host walks the chunks
    (parse) and the device runs three launches.  segments=True asks for the segmented route (egs_png_decode_ex with EGS_PNG_SEGMENTS: a file
    whose IDAT chunks are independent deflate segments -- the device encoder's files, zlib with a full flush per chunk -- is inflated by one
    wave per chunk, every other file by the serial wave as before; statuses and pixels are the same either way); last_route then holds the
    route word per file of the last read() (route_text), read with the status words in the same one read."""
    NAME, FORMAT, HOST_READER = "PngReader", "PNG", "png.decode"
    status_text = staticmethod(status_text)

    def __init__(self, device, batch=32, max_file_bytes=0, max_pixels=0, guard=0, segments=False):
        self.flags = SEGMENTS if segments else 0
        self.last_route, self.last_route_ptr = [], None                 # with segments=True: the route word per file (else zeros)
        super().__init__(device, batch, max_file_bytes, max_pixels, guard)

    @staticmethod
    def _parse_one(blob):
        return parse(blob) + (len(blob),)

    @staticmethod
    def _shape(entry):
        return entry[:3]

    _plan = staticmethod(plan)

    def _second_table(self, p):
        return p["idat"], len(p["idat"])

    def _scratch_need(self, lib, n, p):
        n_idat = len(p["idat"])
        return int(lib.egs_png_decode_scratch_bytes_ex(n_idat, p["stream_bytes"], p["inflate_bytes"], self.flags) if self.flags else
                   lib.egs_png_decode_scratch_bytes(n_idat, p["stream_bytes"], p["inflate_bytes"]))

    def _reserve_scratch(self, max_file_bytes, max_pixels):
        return self.batch * (_up(max_file_bytes, 16) + _up(3 * max_pixels + MAX_SIDE, 16)) + 4096

    def _status_allocation(self):
        return 8 * self.batch                                           # the status words, then (segments) the route words: one read

    def _status_bytes(self, n):
        return 8 * n if self.flags & SEGMENTS else 4 * n

    def _launch(self, lib, call, n, status):
        self.last_route_ptr = status.data_ptr() + 4 * n if self.flags & SEGMENTS else None
        if self.flags:
            _lib.check(lib.egs_png_decode_ex(*call, _hip.stream_of(self.device), 7, self.flags, self.last_route_ptr))
        else:
            _lib.check(lib.egs_png_decode(*call, _hip.stream_of(self.device)))

    def _after_words(self, words, lo, n):
        routes = [r & 0xFFFFFFFF for r in words[n:]] if self.flags & SEGMENTS else [0] * n
        self.last_route = (self.last_route if lo else []) + routes
        return words[:n]


def decode_device(file_bytes, device="cuda", segments=False):
    """One file (bytes or a path) -> device uint8 [h, w, C], by the kernels; segments as PngReader takes it.  (A reader of many files
    keeps a PngReader.)"""
    return PngReader(device, batch=1, segments=segments).read([file_bytes])[0].clone()
