"""The captured frame sweep that evaluate.EvalPass and masks.MaskPass share: per frame ONE device copy of a packed frame (or one decode
launch from a frames.FrameStore) into static buffers and ONE replay of a graph captured once under torch.no_grad() -- a forward followed by a
kernel that writes the frame's result row at a device-side cursor.  The host reads the rows once, after the last frame; a frame whose row
says the captured instance capacity clipped it is run again eagerly (the eager forward sizes its buffers itself): a sweep is never silently
clipped.

A pass supplies: `_what`, `_statement` (its name in messages, the torch statement of its definition), `_packed` (how its frames are packed),
`_replaced` (the decoded columns a re-render replaces), `_check_store(store)`, `_frame_layout(H, W, gated)`, `_set_static(views, H, W, dev)`,
`_body(rows, cursor, guard) -> (kept state, result)`, `_new_rows(n, dev)`, `_decode(rows)`, `_new_out(n, dev)` and `_bytes(result)` -- the
per-frame bytes (image or mask) copied into row i of what `_new_out` made, when it made anything.
"""
import numpy as np
import torch

from . import _C
from .frames import FrameStore
from .graph import _StaticCamera, capture_capacity, frame_views, record_graph, warm_up


class CapturedSweep:
    def __init__(self, pc, bg, graphed):
        self.pc, self.bg = pc, bg
        self.graphed = bool(graphed)
        self.graph = None
        self.guard = None
        self.capacity = 0
        self.host_reads = 0               # reads of result rows this object did (one per sweep; one more when frames were rendered again)
        self._key = None

    # ---- static inputs ------------------------------------------------------------------------------------------------------------
    def _make_static(self, cam, numel, dev):
        name = type(self).__name__
        H, W = int(cam.image_height), int(cam.image_width)
        for gated in (False, True):
            off, size = self._frame_layout(H, W, gated)
            if size == numel:
                break
        else:
            raise ValueError(f"{name}: a frame of {numel} floats is not {self._packed} of a {W}x{H} camera{self._options()}")
        self._frame = torch.zeros(size, device=dev, dtype=torch.float32)
        views = frame_views(self._frame, off, H, W)
        self._cam = _StaticCamera(cam, storage=views["cam"])
        self._set_static(views, H, W, dev)
        self._key = (numel, H, W, float(cam.FoVx), float(cam.FoVy), dev)
        self.graph = None

    def _options(self):
        return ""

    # ---- capture --------------------------------------------------------------------------------------------------------------------
    def _capture(self, first_frame, n_rows, capacity, capacity_margin):
        dev = self._frame.device
        self.guard = _C.StepGuard(dev)
        self._rows, self._cursor = self._new_rows(n_rows, dev)
        side = torch.cuda.Stream(device=dev)

        def first():                                                   # eager: sets the capacity hint, allocator pools, lazy state
            self._frame.copy_(first_frame)
            self._body(None, None, None)
        r_seen = warm_up([first], side, dev)
        self.capacity = capture_capacity(r_seen, capacity_margin, dev, capacity=capacity)
        self._model_version = getattr(self.pc, "model_version", 0)
        self.graph, self._captured = record_graph(lambda: self._body(self._rows, self._cursor, self.guard), side, dev)

    def recapture(self):
        """Forget the captured graph (after the model reallocated its arrays, or changed its active SH degree): the next run() captures again."""
        self.graph = None

    def _read_rows(self, rows):
        """THE device-to-host read of a sweep's results (tests wrap it to count)."""
        self.host_reads += 1
        return rows.cpu()

    # ---- the sweep ------------------------------------------------------------------------------------------------------------------
    def _sweep(self, frames, cam, capacity, capacity_margin):
        """run() of both passes -> (decoded columns of every frame, indices of the frames rendered again, what `_new_out` made, filled)."""
        name = type(self).__name__
        store = frames if isinstance(frames, FrameStore) else None
        if store is not None:
            self._check_store(store)
            if (store.H, store.W) != (int(cam.image_height), int(cam.image_width)):
                raise ValueError(f"{name}: the store's frames are {store.W}x{store.H}, the camera {cam.image_width}x{cam.image_height}")
            n, first = store.n_frames, store.frame(0)
            ring = store.new_ring(n)
            ring.set(range(n))                                          # the sweep's frames 0 .. n - 1: the decode walks them on the device
            load = lambda i: store.decode(self._frame, ring=ring)       # (called once per frame, in order)
            reload = lambda i: store.decode(self._frame, indices=[i])
        else:
            n = frames.shape[0] if torch.is_tensor(frames) else len(frames)
            if n == 0:
                raise ValueError(f"{name}.run: no frames")
            first = frames[0]
            load = reload = lambda i: self._frame.copy_(frames[i], non_blocking=True)      # the frame's every input: one copy
        if not first.is_cuda:
            raise RuntimeError(f"{name}: frames are on {first.device}: the {self._what} has no CPU path ({self._statement} is the torch statement)")
        dev = first.device
        key = (first.numel(), int(cam.image_height), int(cam.image_width), float(cam.FoVx), float(cam.FoVy), dev)
        if self._key != key:
            self._make_static(cam, first.numel(), dev)
        out = self._new_out(n, dev)
        if self.graphed:
            if self.graph is not None and getattr(self.pc, "model_version", 0) != self._model_version:
                raise RuntimeError(f"{name}: the model reallocated its arrays (CapacityGaussians.grow) after this pass was captured; "
                                   "the captured launches point at freed memory -- call recapture() first")
            if self.graph is None or self._rows.shape[0] < n or (capacity is not None and int(capacity) != self.capacity):
                self._capture(first, max(n, 64), capacity, capacity_margin)
            rows, cursor = self._rows, self._cursor
            rows.zero_(); cursor.zero_()
            src = None if out is None else self._bytes(self._captured[1])
            for i in range(n):
                load(i)
                self.graph.replay()
                if out is not None:
                    out[i].copy_(src, non_blocking=True)
        else:
            rows, cursor = self._new_rows(n, dev)
            self._eager(range(n), load, rows, cursor, out)
        fig = self._decode(self._read_rows(rows[:n]))
        again = [int(i) for i in np.nonzero(fig["clipped"])[0]]
        if again:
            rows2, cursor2 = self._new_rows(len(again), dev)
            self._eager(again, reload, rows2, cursor2, out)            # eager: the forward grows its buffers by itself
            fig2 = self._decode(self._read_rows(rows2))
            for k in self._replaced:
                fig[k][again] = fig2[k]
        return fig, again, out

    def _eager(self, indices, load, rows, cursor, out):
        for i in indices:
            load(i)
            _, res = self._body(rows, cursor, None)
            if out is not None:
                out[i].copy_(self._bytes(res), non_blocking=True)
