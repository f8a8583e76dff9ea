"""The 8-bit frame store: a dataset resident on the device in its native precision, decoded by index inside the captured step.

The reference's images come from 8-bit files (its utils/general_utils.py:22-39: uint8 -> float / 255) and its masks are binarised to {0, 1}
(binarize_mask, :41-60), so a packed float32 frame (graph.pack_frame / pack_label_frame) says in 16 - 20 bytes per pixel what 3 bytes and
one or two bits hold.  A FrameStore keeps F frames of one image size and one frame layout as

    img    uint8 [F, image_stride]            the image bytes in the CHW order of `gt` (pre-multiplied by the object mask for object_loss)
    bits   int32 [F, n_planes, plane_words]   one bit per pixel and plane: gate, then obj_mask; pixel p is bit p % 32 of word p // 32
    small  float32 [F, small_floats]          the camera block, accum_R, accum_T and the pose_rows word (int32 bits), untouched

(strides: include/egs_raster.h egs_frame_store_layout) and turns them back into packed frames two ways: `frame(i)`, written in torch on
whatever device the store is on -- the DEFINITION of decoding, bit for bit what pack_frame gives for the original inputs -- and `decode`, the
HIP kernel (csrc/frames.hip, egs_frame_decode), which writes S frames in one launch from a device-side ring of indices and advances the
ring's cursor on the device, so that a captured step (graph.GraphedTrainStep(frame_store=)) needs no frame copy and no host work per replay.

Exactness.  An image value is byte / 255.0 by true division -- `lut` below, computed once on the host -- never byte * (1 / 255): the
product differs from the quotient at 126 of the 256 codes.  put() takes uint8 images, or float32 images whose every value is exactly such a
quotient; anything else is a ValueError unless quantize=True.  Masks and gates are exactly 0 or 1.
"""
import torch

from . import lib as _lib
from . import _hip
from .graph import frame_layout, frame_views, pack_camera, pose_word

LAYOUT_OPTIONS = ("dynamic", "motion", "gated", "object_loss", "label_phase", "pose_rows")
DEFAULT_RING_CAPACITY = 4096


def byte_table():
    """float32[256] on the host: code -> code / 255.0, the quotient itself."""
    return torch.arange(256, dtype=torch.uint8).float() / 255.0


def layout_flags(dynamic=False, motion=False, gated=False, object_loss=False, label_phase=False, pose_rows=False):
    """The EGS_FRAME_* word of a layout."""
    return (_lib.FRAME_DYNAMIC * bool(dynamic) | _lib.FRAME_MOTION * bool(motion) | _lib.FRAME_GATED * bool(gated)
            | _lib.FRAME_OBJECT_LOSS * bool(object_loss) | _lib.FRAME_LABEL_PHASE * bool(label_phase) | _lib.FRAME_POSE_ROWS * bool(pose_rows))


def _check_indices(indices, n_frames, what):
    idx = [int(i) for i in indices]
    for i in idx:
        if i < 0 or i >= n_frames:
            raise IndexError(f"{what}: frame index {i} outside [0, {n_frames})")
    return idx


class FrameRing:
    """A ring of frame indices and its two control words, cursor and length, on the device: ONE int32 tensor [2 + capacity] -- `ctl` its
    first two words, `ring` the rest -- so that the host sets a schedule with one small copy.  The decode reads row k's frame at
    ring[(ctl[0] + k) % ctl[1]] and then advances ctl[0] by the rows it wrote, on the device."""

    def __init__(self, capacity, n_frames, device):
        self.capacity, self.n_frames = int(capacity), int(n_frames)
        if self.capacity < 1:
            raise ValueError("FrameRing: capacity >= 1")
        self._words = torch.zeros(2 + self.capacity, dtype=torch.int32, device=device)
        self._words[1] = 1
        self.ctl, self.ring = self._words[0:2], self._words[2:]

    def set(self, indices):
        """Writes `indices` to ring[0:K] and ctl = {0, K}.  A host sequence (or an int) is range-checked here (IndexError) and travels as one
        copy; an int32 device tensor is copied as it is -- the kernel clamps what is out of range and counts it in the store's status."""
        if torch.is_tensor(indices) and indices.device.type != "cpu":
            if indices.dtype != torch.int32 or indices.dim() != 1:
                raise ValueError("FrameRing.set: a device tensor of indices is 1-D int32")
            k = int(indices.numel())
            self._fits(k)
            self.ring[:k].copy_(indices, non_blocking=True)
            self.ctl.copy_(torch.tensor([0, k], dtype=torch.int32), non_blocking=True)
            return k
        if isinstance(indices, int):
            indices = [indices]
        idx = _check_indices(indices.tolist() if torch.is_tensor(indices) else indices, self.n_frames, "FrameRing.set")
        self._fits(len(idx))
        self._words[:2 + len(idx)].copy_(torch.tensor([0, len(idx)] + idx, dtype=torch.int32), non_blocking=True)
        return len(idx)

    def _fits(self, k):
        if k < 1 or k > self.capacity:
            raise ValueError(f"FrameRing.set: {k} indices do not fit a ring of capacity {self.capacity} (at least one is needed)")


def _plane(t, name, H, W, device):
    """A mask or gate as a flat bool tensor; its values must be exactly 0 or 1."""
    t = t.detach().to(device)
    if t.numel() != H * W:
        raise ValueError(f"{name}: one value per pixel, [H,W] or [1,H,W] with H, W = {H}, {W}; got {tuple(t.shape)}")
    t = t.reshape(-1)
    if t.dtype == torch.bool:
        return t
    one = t == 1
    if not bool((one | (t == 0)).all()):
        raise ValueError(f"{name}: every value must be exactly 0 or 1 (binarise it first)")
    return one


def _pack_bits(b, words):
    """flat bool [n] -> int32 [words]: element p is bit p % 32 of word p // 32; the bits beyond n are 0."""
    full = torch.zeros(words * 32, dtype=torch.int64, device=b.device)
    full[:b.numel()] = b.to(torch.int64)
    full = full.view(words, 32)
    low = (full[:, :31] << torch.arange(31, dtype=torch.int64, device=b.device)).sum(1)
    return (low - (full[:, 31] << 31)).to(torch.int32)                 # bit 31 is the sign: the value stays inside int32


def _unpack_bits(w, n):
    """int32 [words] -> float32 [n] of 0.0 / 1.0 (the inverse of _pack_bits)."""
    sh = torch.arange(32, dtype=torch.int32, device=w.device)
    return ((w.view(-1, 1) >> sh) & 1).reshape(-1)[:n].to(torch.float32)


class FrameStore:
    def __init__(self, H, W, n_frames, device="cpu", dynamic=False, motion=False, gated=False, object_loss=False, label_phase=False,
                 ring_capacity=DEFAULT_RING_CAPACITY, pose_rows=False):
        """F = n_frames frames of H x W in the layout graph.frame_layout gives for the same options (object_loss: any true value).  The
        arrays start as zeros: an unset frame decodes to a black image, a zero camera, closed gates.  `ring`, `ctl`: the store's own
        FrameRing (ring_capacity entries), what decode() walks unless it is given another; `status`: device int32[1], sticky, the number of
        frame indices the kernel ever had to clamp."""
        self.H, self.W, self.n_frames = int(H), int(W), int(n_frames)
        if self.H < 1 or self.W < 1 or self.n_frames < 1:
            raise ValueError("FrameStore: H, W and n_frames >= 1")
        self.layout = dict(dynamic=bool(dynamic), motion=bool(motion), gated=bool(gated), object_loss=bool(object_loss), label_phase=bool(label_phase))
        if self.layout["label_phase"] and (dynamic or motion or object_loss):
            raise ValueError("FrameStore(label_phase=True) goes with gated only: the label frame is camera[, gate], obj_mask")
        if self.layout["motion"] and not self.layout["dynamic"]:
            raise ValueError("FrameStore(motion=True) goes with dynamic=True, as GraphedTrainStep")
        if pose_rows:                                                   # (the key exists only in such a store's layout: every other layout is what it was)
            if not self.layout["motion"]:
                raise ValueError("FrameStore(pose_rows=True) goes with motion=True: the frame word of a pose sequence")
            self.layout["pose_rows"] = True
        self.device = torch.device(device)
        n_pix = self.H * self.W
        self.n_pix, self.n_img = n_pix, (0 if label_phase else 3 * n_pix)
        self.off, self.frame_floats = frame_layout(self.n_img, n_pix, **self.layout)
        self.flags = layout_flags(**self.layout)
        self.planes = [n for n in ("gate", "obj_mask") if n in self.off]
        self.image_stride = (self.n_img + 15) & ~15
        self.plane_words = (((n_pix + 31) >> 5) + 3) & ~3
        self.small_begin = self.off["cam"][0]
        self.small_floats = (max(self.off[n][1] for n in ("cam", "accum_R", "accum_T", "pose_rows") if n in self.off) - self.small_begin + 3) & ~3
        dev = self.device
        self.img = torch.zeros((self.n_frames, self.image_stride), dtype=torch.uint8, device=dev) if self.n_img else None
        self.bits = torch.zeros((self.n_frames, len(self.planes), self.plane_words), dtype=torch.int32, device=dev) if self.planes else None
        self.small = torch.zeros((self.n_frames, self.small_floats), dtype=torch.float32, device=dev)
        self.lut = byte_table().to(dev)
        self._ring = FrameRing(ring_capacity, self.n_frames, dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    ring = property(lambda self: self._ring.ring)
    ctl = property(lambda self: self._ring.ctl)

    def new_ring(self, capacity):
        """A further FrameRing over this store's frames (a captured step keeps its own, so that a sweep on the same store leaves its schedule alone)."""
        return FrameRing(capacity, self.n_frames, self.device)

    # ---- sizes ----------------------------------------------------------------------------------------------------------------------------
    @property
    def nbytes(self):
        """Bytes of the frames as stored: img + bits + small (the 1 KB table, the ring and the status word are not dataset)."""
        return sum(t.numel() * t.element_size() for t in (self.img, self.bits, self.small) if t is not None)

    @property
    def float_nbytes(self):
        """Bytes of the same frames as packed float32 tensors."""
        return self.n_frames * self.frame_floats * 4

    # ---- writing ----------------------------------------------------------------------------------------------------------------------------
    def _image_bytes(self, gt, quantize):
        gt = gt.detach().to(self.device)
        if gt.numel() != self.n_img:
            raise ValueError(f"FrameStore.put: gt is [3,{self.H},{self.W}]; got {tuple(gt.shape)}")
        gt = gt.reshape(-1)
        if gt.dtype == torch.uint8:
            return gt
        if gt.dtype != torch.float32:
            raise ValueError(f"FrameStore.put: gt is uint8 or float32, got {gt.dtype}")
        if not bool(torch.isfinite(gt).all()):
            raise ValueError("FrameStore.put: gt holds values that are not finite")
        q = torch.round(gt.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
        if not quantize and not torch.equal(self.lut[q.long()].view(torch.int32), gt.contiguous().view(torch.int32)):
            raise ValueError("FrameStore.put: gt holds values that are not k / 255 in float32 (an 8-bit image divided by 255.0); "
                             "pass quantize=True to round them to the nearest code")
        return q

    def _check_given(self, who, items):
        """The layout decides what must be given: everything it has, nothing it lacks.  items: (name, value, wanted) triples."""
        for name, given, wanted in items:
            if (given is not None) != wanted:
                raise ValueError(f"{who}: this store's layout {'needs' if wanted else 'has no'} {name} ({self.layout})")

    def _small_block(self, cam, accum_R=None, accum_T=None, pose_rows=None):
        """One frame's row of `small` on the store's device (put() and ingest.FrameIngest.put() write it the same way)."""
        dev = self.device
        block = torch.zeros(self.small_floats, dtype=torch.float32, device=dev)
        rel = lambda n: slice(self.off[n][0] - self.small_begin, self.off[n][1] - self.small_begin)
        packed = cam if torch.is_tensor(cam) else pack_camera(cam)
        if packed.numel() != 35:
            raise ValueError("FrameStore.put: cam is a camera or its packed float32[35] block")
        block[rel("cam")] = packed.detach().reshape(-1).to(dev, torch.float32)
        if accum_R is not None:
            block[rel("accum_R")] = accum_R.detach().reshape(-1).to(dev, torch.float32)
        if accum_T is not None:
            block[rel("accum_T")] = accum_T.detach().reshape(-1, 4)[:3].reshape(-1).to(dev, torch.float32)
        if pose_rows is not None:                                       # (fixed_row, train_row[, reload]), or the int32[4] word itself
            word = pose_rows.detach().reshape(-1).to(torch.int32) if torch.is_tensor(pose_rows) else pose_word(pose_rows)
            block[rel("pose_rows")].view(torch.int32).copy_(word)
        return block

    def put(self, i, cam, gt=None, accum_R=None, accum_T=None, gate=None, obj_mask=None, quantize=False, _premasked=False, pose_rows=None):
        """Stores frame i -- the arguments of graph.pack_frame / pack_label_frame, and frame(i) then equals what those return for them, bit
        for bit.  cam: a camera, or its packed float32[35] block.  gt: uint8 [3,H,W], or float32 with every value exactly k / 255 in float32
        (x == round(x * 255) / 255 bit for bit), else ValueError unless quantize=True (then round(clamp(x, 0, 1) * 255), ties to even, is
        stored).  gate, obj_mask: [H,W] or [1,H,W], exactly 0 or 1, else ValueError.  The layout decides what must be given: everything it
        has, nothing it lacks.  With object_loss the image is stored pre-multiplied by obj_mask, as pack_frame(obj_mask=) stores gt * obj_mask."""
        i = _check_indices([i], self.n_frames, "FrameStore.put")[0]
        lay = self.layout
        has_mask = lay["object_loss"] or lay["label_phase"]
        self._check_given("FrameStore.put", (("gt", gt, not lay["label_phase"]), ("accum_R", accum_R, lay["dynamic"]), ("accum_T", accum_T, lay["motion"]),
                                             ("gate", gate, lay["gated"]), ("obj_mask", obj_mask, has_mask), ("pose_rows", pose_rows, lay.get("pose_rows", False))))
        dev = self.device
        block = self._small_block(cam, accum_R, accum_T, pose_rows)
        planes = {}
        if gate is not None:
            planes["gate"] = _plane(gate, "gate", self.H, self.W, dev)
        if obj_mask is not None:
            planes["obj_mask"] = _plane(obj_mask, "obj_mask", self.H, self.W, dev)
        q = None
        if gt is not None:
            q = self._image_bytes(gt, quantize)
            if lay["object_loss"]:
                m = planes["obj_mask"].repeat(3)
                if _premasked and bool((q[~m] != 0).any()):
                    raise ValueError("FrameStore.from_packed: an object-loss frame holds image values outside its object mask "
                                     "(pack_frame(obj_mask=) stores gt * obj_mask)")
                q = q * m.to(torch.uint8)
        # everything is checked: now write
        self.small[i] = block
        if q is not None:
            self.img[i, :self.n_img] = q
        for p, name in enumerate(self.planes):
            self.bits[i, p] = _pack_bits(planes[name], self.plane_words)

    @classmethod
    def from_packed(cls, frames, H, W, device=None, ring_capacity=DEFAULT_RING_CAPACITY, **layout):
        """The inverse of graph.pack_frame / pack_label_frame: a store of the given layout holding `frames` (a list or an [F, frame] tensor of
        packed float32 frames), on their device unless `device` says otherwise.  A frame whose size is not the layout's, an image value that
        is not k / 255, a mask value that is not 0 or 1: ValueError."""
        n = frames.shape[0] if torch.is_tensor(frames) else len(frames)
        if n == 0:
            raise ValueError("FrameStore.from_packed: no frames")
        store = cls(H, W, n, frames[0].device if device is None else device, ring_capacity=ring_capacity, **layout)
        off = store.off
        for i in range(n):
            f = frames[i].detach().reshape(-1)
            if f.numel() != store.frame_floats or f.dtype != torch.float32:
                raise ValueError(f"FrameStore.from_packed: frame {i} has {f.numel()} {f.dtype} elements, the layout {store.layout} at "
                                 f"{W}x{H} has {store.frame_floats} float32")
            seg = lambda name: f[off[name][0]:off[name][1]] if name in off else None
            word = seg("pose_rows")
            store.put(i, seg("cam"), gt=seg("gt"), accum_R=seg("accum_R"), accum_T=seg("accum_T"), gate=seg("gate"), obj_mask=seg("obj_mask"),
                      _premasked=True, pose_rows=None if word is None else word.view(torch.int32))
        return store

    def set_pose_rows(self, i, rows):
        """Rewrites frame i's pose_rows word in place: rows = (fixed_row, train_row[, reload]) (a store with pose_rows=True)."""
        if "pose_rows" not in self.off:
            raise ValueError(f"FrameStore.set_pose_rows: this store's layout has no pose_rows ({self.layout})")
        i = _check_indices([i], self.n_frames, "FrameStore.set_pose_rows")[0]
        b = self.off["pose_rows"][0] - self.small_begin
        self.small[i, b:b + 4].view(torch.int32).copy_(pose_word(rows), non_blocking=True)

    # ---- reading: the definition --------------------------------------------------------------------------------------------------------------
    def frame(self, i):
        """Frame i as a packed float32 tensor, in torch, on the store's device: image value = lut[byte] (byte / 255.0), plane value = its bit
        as 0.0 / 1.0, the small block as stored, 0.0 between the segments."""
        i = _check_indices([i], self.n_frames, "FrameStore.frame")[0]
        f = torch.zeros(self.frame_floats, dtype=torch.float32, device=self.device)
        if self.n_img:
            f[:self.n_img] = self.lut[self.img[i, :self.n_img].long()]
        f[self.small_begin:self.small_begin + self.small_floats] = self.small[i]
        for p, name in enumerate(self.planes):
            f[self.off[name][0]:self.off[name][1]] = _unpack_bits(self.bits[i, p], self.n_pix)
        return f

    def frames(self, indices=None):
        """torch.stack of frame(i) over `indices` (default: all)."""
        return torch.stack([self.frame(i) for i in (range(self.n_frames) if indices is None else indices)])

    def parts(self, i):
        """Frame i as the named float32 tensors a step is captured on: dict(frame, cam[35], gt[3,H,W], accum_R[3,3], accum_T[3,4], gate[H,W],
        obj_mask[H,W]) -- views of frame(i), None where the layout has none."""
        f = self.frame(i)
        return dict(frame_views(f, self.off, self.H, self.W), frame=f)

    # ---- reading: the kernel --------------------------------------------------------------------------------------------------------------------
    def decode(self, out, indices=None, ring=None):
        """The HIP path (include/egs_raster.h egs_frame_decode): writes S = out.numel() / frame_floats complete packed frames into `out` -- a
        contiguous float32 device tensor or view, [S, frame_floats] or flat; 4-byte alignment is enough -- row k from frame
        ring[(ctl[0] + k) % ctl[1]], then advances ctl[0] by S on the device.  indices: an int, a sequence of S ints or an int32 device
        tensor of S entries written to the ring first (ctl = {0, S}; host values are range-checked: IndexError); None: the ring as it stands.
        ring: a FrameRing of this store (default: the store's own).  Does not synchronise; can be captured.  HIP tensors only."""
        if not (torch.is_tensor(out) and out.is_cuda) or self.device.type != "cuda":
            raise RuntimeError(f"FrameStore.decode: the store is on {self.device}, out on {getattr(out, 'device', None)}: the fused HIP decode "
                               "has no CPU path (frame(i) is the torch statement)")
        if out.device != self.small.device or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() % self.frame_floats or not out.numel():
            raise RuntimeError(f"FrameStore.decode: out is a contiguous float32 tensor of S x {self.frame_floats} elements on the store's device")
        S = out.numel() // self.frame_floats
        ring = self._ring if ring is None else ring
        if indices is not None:
            k = 1 if isinstance(indices, int) else int(indices.numel()) if torch.is_tensor(indices) else len(indices)
            if k != S:
                raise ValueError(f"FrameStore.decode: out holds {S} frames, indices names {k}")
            ring.set(indices)
        L = _lib.load()
        p = lambda t: None if t is None else t.data_ptr()
        dev = out.device
        with _hip.device_ctx(dev):
            _lib.check(L.egs_frame_decode(self.H, self.W, self.flags, self.n_frames, S, p(self.img), p(self.bits), p(self.small), p(self.lut),
                                          p(ring.ring), ring.capacity, p(ring.ctl), p(self.status), p(out), _hip.stream_of(dev)))
        return out

    def png(self, indices, what="gt"):
        """The stored image bytes of frames `indices` as PNG files, encoded where they lie (png.encode / include/egs_raster.h egs_png_encode):
        the bytes are planar uint8 already, the strides are the store's.  -> (buf uint8 [K, bound], sizes int32 [K]) on the store's device;
        buf[k, :sizes[k]] is the file of frame indices[k] (for an object_loss store: of the image times its object mask, what is stored).
        A run of consecutive indices is one call.  HIP stores only; nothing is read back."""
        from . import png as _png
        if what != "gt":
            raise ValueError(f"FrameStore.png: what = 'gt' (the image bytes); masks are bit planes here, got {what!r}")
        if self.img is None:
            raise ValueError(f"FrameStore.png: this store's layout has no image ({self.layout})")
        if self.device.type != "cuda":
            raise RuntimeError(f"FrameStore.png: the store is on {self.device}: the PNG encoder has no CPU path (png.encode_statement is the host statement)")
        idx = _check_indices([indices] if isinstance(indices, int) else indices, self.n_frames, "FrameStore.png")
        if not idx:
            raise ValueError("FrameStore.png: no frames")
        K, run = len(idx), 1
        buf = torch.empty((K, _png.bound(self.W, self.H, 3)), dtype=torch.uint8, device=self.device)
        sizes = torch.empty(K, dtype=torch.int32, device=self.device)
        scratch = torch.empty(_png.scratch_bytes(K, self.W, self.H, 3), dtype=torch.uint8, device=self.device)
        for k in range(0, K, 1):
            if k + 1 < K and idx[k + 1] == idx[k] + 1:
                run += 1
                continue
            k0 = k + 1 - run
            _png._launch(run, self.W, self.H, 3, self.img[idx[k0]].data_ptr(), self.image_stride, self.n_pix, buf[k0:], sizes[k0:], scratch, self.device)
            run = 1
        return buf, sizes

    def ok(self):
        """True while the kernel never had to clamp a frame index (reads the status word: synchronises)."""
        return int(self.status.item()) == 0
