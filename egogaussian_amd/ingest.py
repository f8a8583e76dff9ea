"""Frame ingest: the producer of the 8-bit frame store.

The reference builds every frame in loadCam (its utils/camera_utils.py:21-94): image, hand mask and object mask go through PIL.Image.resize
with the default filter -- bicubic, antialiased, on 8-bit data --, are divided by 255 (PILtoTorch, utils/general_utils.py:22-39) and the
masks collapse to {0, 1} (binarize_mask, :41-60).  This module states that path on bytes and runs it on the device:

    target_size      loadCam's size rule, its double arithmetic included
    resample_tables  the coefficients and bounds of one axis, numpy float64 -- an independent restatement, not a call into the library
    resize_u8        the resize in torch integer ops, on any device: the DEFINITION the kernel answers to
    binarize         binarize_mask on bytes
    FrameIngest      source-resolution uint8 arrays -> one frame's rows of a FrameStore, by the HIP kernel (csrc/ingest.hip,
                     egs_frame_ingest): one launch per source array, the horizontal result of a tile in LDS as bytes, no intermediate in
                     device memory, no read-back -- the same bits loadCam followed by FrameStore.put leaves in the store.

The resize (Pillow Resample.c, modes L and RGB, no box, no reducing gap): a horizontal pass when the width changes, then a vertical pass
when the height changes; the intermediate is 8-bit, rounded and clamped like the output; a pass whose size does not change is skipped.  A
pixel of a pass is clamp((2^21 + sum in[xmin + x] * kk[x]) >> 22, 0, 255) in int32 with an arithmetic shift.

Files: FrameIngest.put_files takes 8-bit grey or RGB PNG files and baseline JPEG files (paths or bytes, told apart by their first two
bytes) in place of arrays and decodes them on the device (egogaussian_amd/png.py PngReader, csrc/png_decode.hip; egogaussian_amd/jpeg.py
JpegReader, csrc/jpeg_decode.hip) in front of the same kernel; put() with host-decoded arrays is unchanged.  Progressive, multi-scan and
CMYK JPEG files, and the PNG modes Pillow resizes differently (palette, alpha, 16-bit, interlaced ones too), are decoded on the host and go
through put().
"""
import math

import numpy as np
import torch

from . import lib as _lib
from . import _hip
from .file_reader import load_files

PRECISION_BITS = 22
MAX_SCALE = 8               # per axis: ksize <= 33, what bounds the kernel's tile in LDS
MAX_SIDE = 32767
_ADVICE = "resize it with Pillow on the host and store the result with FrameStore.put()"


def target_size(orig_w, orig_h, resolution=-1, resolution_scale=1.0):
    """(W, H) loadCam gives a frame of orig_w x orig_h (utils/camera_utils.py:24-41).  The double arithmetic is part of the rule:
    int(1921 / (1921 / 1600)) need not be 1600."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))      # (half to even)
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def ksize_of(n_in, n_out):
    scale = n_in / n_out
    return int(math.ceil(2.0 * max(scale, 1.0))) * 2 + 1


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resample_tables(n_in, n_out):
    """-> (kk int32 [n_out, ksize], bounds int32 [n_out, 2] = (xmin, xmax)): Pillow's precompute_coeffs + normalize_coeffs_8bpc for the
    bicubic filter, in float64, every expression in the order the C evaluates it (the running sum of the weights in index order too)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resample_tables: sizes >= 1")
    scale = np.float64(n_in) / np.float64(n_out)
    filterscale = max(scale, np.float64(1.0))
    support = np.float64(2.0) * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    ss = np.float64(1.0) / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                # (int) truncates; the operands are > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < xmax[:, None]
    w = np.where(live, _bicubic(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for k in range(ksize):
        ww = ww + w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    fixed = np.where(w < 0, -0.5 + w * float(1 << PRECISION_BITS), 0.5 + w * float(1 << PRECISION_BITS))
    kk = np.trunc(fixed).astype(np.int32)
    return kk, np.stack([xmin, xmax], axis=1).astype(np.int32)


def _as_tensor(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _pass(src, n_out, axis):
    """One pass along `axis` (0 or 1) of an int32 [h, w, C] tensor of bytes -> int32 bytes again."""
    n_in = src.shape[axis]
    kk, bounds = resample_tables(n_in, n_out)
    kk_t = torch.from_numpy(kk).to(src.device)
    lo = torch.from_numpy(bounds[:, 0].astype(np.int64)).to(src.device)
    shape = [1, 1, 1]
    shape[axis] = n_out
    acc = torch.full([n_out if d == axis else s for d, s in enumerate(src.shape)], 1 << (PRECISION_BITS - 1), dtype=torch.int32, device=src.device)
    for k in range(kk.shape[1]):
        idx = (lo + k).clamp(max=n_in - 1)                                         # (beyond xmax the coefficient is 0)
        acc += src.index_select(axis, idx) * kk_t[:, k].view(shape)
    return (acc >> PRECISION_BITS).clamp(0, 255)                                  # (arithmetic shift)


def resize_u8(array_hwc, size):
    """PIL.Image.resize(size) of an 8-bit L or RGB image, in torch integer ops.  array_hwc: uint8 [h, w] or [h, w, C] (numpy or torch,
    any device); size = (W, H).  -> uint8 tensor of shape [H, W] or [H, W, C] on the input's device."""
    t = _as_tensor(array_hwc)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError(f"resize_u8: a uint8 array [h,w] or [h,w,C]; got {t.dtype} {tuple(t.shape)}")
    W, H = int(size[0]), int(size[1])
    if W < 1 or H < 1 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("resize_u8: sizes >= 1")
    flat = t.dim() == 2
    v = (t.unsqueeze(-1) if flat else t).to(torch.int32)
    if v.shape[1] != W:
        v = _pass(v, W, 1)
    if v.shape[0] != H:
        v = _pass(v, H, 0)
    v = v.to(torch.uint8)
    return v.squeeze(-1) if flat else v


def binarize(resized):
    """binarize_mask on the bytes of a resized mask: uint8 [H, W] or [H, W, C] -> bool [H, W], any channel > 0."""
    t = _as_tensor(resized)
    return t > 0 if t.dim() == 2 else (t > 0).any(dim=-1)


def _source(a, name, h, w, channels):
    """A source array as a contiguous uint8 tensor [h, w, C] (host or device), or the ValueError that says why this path does not take it."""
    mode = getattr(a, "mode", None)
    if isinstance(mode, str) and not torch.is_tensor(a):                          # a PIL image: its mode says what np.asarray would hide
        if mode in ("P", "PA", "1"):
            raise ValueError(f"FrameIngest.put: {name} is a palette or bilevel image (mode {mode}): Pillow resizes those with the nearest "
                             f"neighbour, which this path does not reproduce; {_ADVICE}")
        a = np.asarray(a)
    t = _as_tensor(a)
    if t.dtype == torch.bool:
        raise ValueError(f"FrameIngest.put: {name} is bilevel (bool): Pillow resizes mode 1 with the nearest neighbour, which this path does not "
                         f"reproduce; {_ADVICE}")
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() == 3 and t.shape[2] == 4:
        raise ValueError(f"FrameIngest.put: {name} has 4 channels: Pillow premultiplies alpha before it resamples, which this path does not "
                         f"reproduce; {_ADVICE}")
    if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape[:2]) != (h, w) or t.shape[2] not in channels:
        want = " or ".join(f"[{h},{w},{c}]" for c in channels) + (f" or [{h},{w}]" if 1 in channels else "")
        raise ValueError(f"FrameIngest.put: {name} is uint8 {want} at the source resolution; got {t.dtype} {tuple(t.shape)}; {_ADVICE}")
    return t.contiguous()


def _parse_file(blob):
    """-> (the file's reader class, told by its first two bytes (FF D8: JPEG); its entry of that reader's `parsed`)."""
    if bytes(blob[:2]) == b"\xff\xd8":
        from .jpeg import JpegReader as kind
    else:
        from .png import PngReader as kind
    return kind, kind._parse_one(blob)


class FrameIngest:
    """Fills the rows of `store` (a FrameStore on a HIP device) from source-resolution 8-bit arrays of src_hw = (h, w).  Owns the device
    tables of (h -> store.H) and (w -> store.W), one pinned staging buffer and one device buffer per plane group."""

    def __init__(self, store, src_hw):
        h, w = int(src_hw[0]), int(src_hw[1])
        if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE or store.H > MAX_SIDE or store.W > MAX_SIDE or h > MAX_SCALE * store.H or w > MAX_SCALE * store.W:
            raise ValueError(f"FrameIngest: source {w}x{h} -> {store.W}x{store.H} is outside the supported range (sides 1 .. {MAX_SIDE}, at most "
                             f"{MAX_SCALE}x down per axis); {_ADVICE}")
        if store.device.type != "cuda":
            raise ValueError(f"FrameIngest: the store is on {store.device}; the ingest kernel writes a store on a HIP device ({_ADVICE}; "
                             "resize_u8 and binarize are the torch statement)")
        self.store, self.h, self.w = store, h, w
        dev = store.device
        self._tables = []
        for n_in, n_out in ((w, store.W), (h, store.H)):
            if n_in == n_out:
                self._tables += [None, None]
            else:
                kk, bounds = resample_tables(n_in, n_out)
                self._tables += [torch.from_numpy(kk).to(dev), torch.from_numpy(bounds).to(dev)]
        # one slot per plane group: a host array is copied into its pinned slot and uploaded from there; the slot's event says when the
        # upload has read it (waited for before the slot is written again: a wait for an upload, never a read of the device)
        self._pinned = torch.empty((3, h * w * 3), dtype=torch.uint8).pin_memory()
        self._device = torch.empty((3, h * w * 3), dtype=torch.uint8, device=dev)
        self._uploaded = [None, None, None]
        from . import png as _png
        self._reader = _png.PngReader(dev, batch=3)                    # put_files: its buffers are allocated by the first decode
        self._jpeg_reader = None                                        # put_files: created by the first JPEG file

    source = staticmethod(_source)      # (array, name, h, w, channels) -> uint8 [h,w,C] tensor, or the refusal

    def _upload(self, slot, t):
        if t.is_cuda:
            if t.device != self.store.device:
                raise ValueError(f"FrameIngest.put: a source on {t.device}, the store on {self.store.device}")
            return t
        n = t.numel()
        dst = self._device[slot, :n]
        if t.is_pinned():
            dst.copy_(t.view(-1), non_blocking=True)
            return dst
        if self._uploaded[slot] is not None:
            self._uploaded[slot].synchronize()
        self._pinned[slot, :n].copy_(t.view(-1))
        dst.copy_(self._pinned[slot, :n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.store.device))
        self._uploaded[slot] = ev
        return dst

    def put(self, i, cam, image=None, hand_mask=None, obj_mask=None, accum_R=None, accum_T=None, pose_rows=None):
        """Stores frame i from what loadCam starts with: image uint8 [h,w,3], hand_mask and obj_mask uint8 [h,w], [h,w,1] or [h,w,3], host
        (numpy, torch, pinned or not) or device arrays at the source resolution; cam, accum_R, accum_T, pose_rows as FrameStore.put takes
        them.  The layout decides what must be given: everything it has, nothing it lacks (hand_mask fills the gate as 1 - hand_mask).
        Uploads are non_blocking and nothing is read back."""
        from .frames import _check_indices
        st = self.store
        i = _check_indices([i], st.n_frames, "FrameIngest.put")[0]
        lay = st.layout
        st._check_given("FrameIngest.put", (("image", image, not lay["label_phase"]), ("accum_R", accum_R, lay["dynamic"]),
                                            ("accum_T", accum_T, lay["motion"]), ("hand_mask", hand_mask, lay["gated"]),
                                            ("obj_mask", obj_mask, lay["object_loss"] or lay["label_phase"]),
                                            ("pose_rows", pose_rows, lay.get("pose_rows", False))))
        groups = []                                                               # launch order: object mask, hand mask, image (which reads the object plane)
        if obj_mask is not None:
            groups.append((_lib.INGEST_OBJ_MASK, 0, _source(obj_mask, "obj_mask", self.h, self.w, (1, 3))))
        if hand_mask is not None:
            groups.append((_lib.INGEST_HAND_MASK, 1, _source(hand_mask, "hand_mask", self.h, self.w, (1, 3))))
        if image is not None:
            groups.append((_lib.INGEST_IMAGE, 2, _source(image, "image", self.h, self.w, (3,))))
        block = st._small_block(cam, accum_R, accum_T, pose_rows)
        # everything is checked: now write
        st.small[i] = block
        for plane, slot, t in groups:
            self._launch(i, plane, slot, t)

    def put_files(self, i, cam, image=None, hand_mask=None, obj_mask=None, accum_R=None, accum_T=None, pose_rows=None, segments=False):
        """put() with 8-bit PNG files or baseline JPEG files -- paths or bytes, each told by its first two bytes (FF D8: JPEG; a call may
        mix them, a JPEG image with PNG masks being the usual dataset) -- in place of the arrays.  The sizes and channel counts are checked
        from the headers against src_hw before any device work (png.parse, jpeg.parse; a mode this path does not take is refused there); the
        files are then uploaded as they are and decoded on the device on the store's stream, in front of the ingest launches.  Nothing is
        read back but each decoder's status words, once; a file the device refuses raises ValueError and the store is left as it was.  The
        store ends up bit-identical to put() with the decoded arrays.  segments=True decodes the PNG files with the segmented route
        (png.PngReader: a wave per IDAT chunk for the files that allow it, e.g. this project's own; the same store either way); it means
        nothing for JPEG."""
        from . import jpeg as _jpeg, png as _png
        self._reader.flags = (self._reader.flags & ~_png.SEGMENTS) | (_png.SEGMENTS if segments else 0)
        given = [(name, f) for name, f in (("obj_mask", obj_mask), ("hand_mask", hand_mask), ("image", image)) if f is not None]
        who = ", ".join(f"file {k} is {name}" for k, (name, _) in enumerate(given))
        try:                                                            # host only: the header walk of every file, the names' index the call's
            blobs, names, found = load_files([f for _, f in given], _parse_file)
        except ValueError as e:
            raise ValueError(f"FrameIngest.put_files: {e} ({who})") from None
        kinds, parsed = [kind for kind, _ in found], [p for _, p in found]
        for (name, _), p, kind in zip(given, parsed, kinds):
            W, H, C = kind._shape(p)
            if (H, W) != (self.h, self.w) or (name == "image" and C != 3):
                raise ValueError(f"FrameIngest.put_files: {name} is {W}x{H} with {C} channel(s); the source resolution is {self.w}x{self.h}"
                                 f"{' and an image has 3' if name == 'image' else ''}; {_ADVICE}")
        if _jpeg.JpegReader in kinds and self._jpeg_reader is None:
            self._jpeg_reader = _jpeg.JpegReader(self.store.device, batch=3)
        decoded = [None] * len(given)
        with _hip.device_ctx(self.store.device):
            for reader, kind in ((self._reader, _png.PngReader), (self._jpeg_reader, _jpeg.JpegReader)):
                idx = [k for k, c in enumerate(kinds) if c is kind]
                if not idx:
                    continue
                try:                                                    # (both decoders run before the first ingest launch)
                    part = reader.decode([blobs[k] for k in idx], [names[k] for k in idx], [parsed[k] for k in idx])
                except ValueError as e:
                    raise ValueError(f"FrameIngest.put_files: {e} ({who})") from None
                for k, t in zip(idx, part):
                    decoded[k] = t
        arrays = {name: t for (name, _), t in zip(given, decoded)}
        self.put(i, cam, image=arrays.get("image"), hand_mask=arrays.get("hand_mask"), obj_mask=arrays.get("obj_mask"), accum_R=accum_R,
                 accum_T=accum_T, pose_rows=pose_rows)

    def plane(self, i, which, array):
        """One plane group of frame i alone: which = "image", "hand_mask" or "obj_mask" (put() is the small block and up to three of these,
        object mask first: the image launch of an object_loss store reads the frame's object plane)."""
        from .frames import _check_indices
        i = _check_indices([i], self.store.n_frames, "FrameIngest.plane")[0]
        plane, slot, channels = {"obj_mask": (_lib.INGEST_OBJ_MASK, 0, (1, 3)), "hand_mask": (_lib.INGEST_HAND_MASK, 1, (1, 3)),
                                 "image": (_lib.INGEST_IMAGE, 2, (3,))}[which]
        self._launch(i, plane, slot, _source(array, which, self.h, self.w, channels))

    def _launch(self, i, plane, slot, t):
        st = self.store
        p = lambda x: None if x is None else x.data_ptr()
        dev = st.device
        with _hip.device_ctx(dev):
            src = self._upload(slot, t)
            _lib.check(_lib.load().egs_frame_ingest(st.H, st.W, st.flags, st.n_frames, i, plane, p(st.img), p(st.bits), p(src), self.h, self.w,
                                                    int(t.shape[2]), *[p(x) for x in self._tables], _hip.stream_of(dev)))
