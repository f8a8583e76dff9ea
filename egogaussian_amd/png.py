"""8-bit PNG files from device tensors: the write side of the files frame ingest reads.

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
