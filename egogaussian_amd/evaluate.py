"""The evaluation pass: per-frame PSNR and SSIM as the reference reports them, without leaving the device between frames.

The reference's eval_and_metric (its trainers/eval_metric.py:41-175) places the object by each frame's pose, renders it
(rot_cov=True, accum_R, which_object=1, no_grad), writes render, ground truth and 1 - hand mask to 8-bit PNGs, reads them back, multiplies
both images by the mask and averages ssim / psnr over the frames: its results.txt is defined on 8-bit images with the hand removed.  Here a
sweep is, per frame, ONE device copy of a packed frame (graph.pack_frame) into static buffers and ONE replay of a graph captured once under
torch.no_grad(): the render (colour only) followed by the metric kernel (fused.eval_metrics / include/egs_raster.h egs_eval_metrics), which
writes the frame's row -- squared 8-bit error, SSIM sum, the forward's overflow word -- at a device-side cursor.  The host reads the rows
once, after the last frame.  A frame whose row says the captured instance capacity clipped it is rendered again eagerly (the eager forward
sizes its buffers itself) and measured by the same kernel: an evaluation is never silently clipped.

LPIPS, the reference's third figure, is not covered: it needs VGG weights this package does not ship.
losses.eval_metrics is the torch statement of the per-frame definition.
"""
import numpy as np
import torch

from . import _C
from . import fused
from .frames import FrameStore
from .graph import _StaticCamera, begin_capture, end_capture, frame_layout
from .renderer import render
from .scene_synth import Pipe


def decode_rows(rows, n_elements):
    """rows: int64[F, 4] (include/egs_raster.h egs_eval_row), on any device -> dict of numpy arrays sse (int64), ssim_sum, ssim, psnr
    (float64), clipped (bool), instances (int64).  psnr = 10 log10(255^2 n / sse), inf where sse == 0; ssim = ssim_sum / n; n = C*H*W."""
    r = np.ascontiguousarray(rows.detach().cpu().numpy()).reshape(-1, fused.EVAL_ROW_WORDS)
    sse = r[:, 0].copy()
    ssim_sum = r[:, 1].copy().view(np.float64)
    with np.errstate(divide="ignore"):
        psnr = np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 * float(n_elements) / np.maximum(sse, 1).astype(np.float64)))
    return dict(sse=sse, ssim_sum=ssim_sum, ssim=ssim_sum / float(n_elements), psnr=psnr, clipped=r[:, 2] != 0, instances=r[:, 3].copy())


class EvalPass:
    def __init__(self, pc, bg, pipe=Pipe, dynamic=False, motion=False, which_object=1, graphed=True, keep_images=False):
        """dynamic / motion / which_object: as graph.GraphedTrainStep -- the render is called exactly as its captured step calls it
        (rot_cov=True, accum_R from the frame; with motion the object is placed by the frame's accum_T inside the rasterizer).
        graphed=False: the same calls, eagerly, frame by frame (no capture, no capacity to outgrow).
        keep_images: run() also returns the quantised renders, uint8[F,3,H,W] on the device -- what goes into the PNGs.
        A capacity.CapacityGaussians model is followed through its live row count like every render()."""
        if motion and not dynamic:
            raise ValueError("EvalPass(motion=True) goes with dynamic=True (the pose's rotation turns the covariances)")
        self.pc, self.bg, self.pipe = pc, bg, pipe
        self.dynamic, self.motion, self.which_object = bool(dynamic), bool(motion), which_object
        self.graphed, self.keep_images = bool(graphed), bool(keep_images)
        self.graph = None
        self.guard = None
        self.capacity = 0
        self.host_reads = 0               # reads of result rows this object did (one per sweep; one more when frames were rendered again)
        self._key = None

    # ---- static inputs ------------------------------------------------------------------------------------------------------------
    def _layout(self, cam, numel):
        H, W = int(cam.image_height), int(cam.image_width)
        for gated in (False, True):
            off, size = frame_layout(3 * H * W, H * W, self.dynamic, gated, self.motion)
            if size == numel:
                return off, size, gated, H, W
        raise ValueError(f"EvalPass: a frame of {numel} floats is not graph.pack_frame(cam, gt[, accum_R][, gate][, accum_T]) of a {W}x{H} camera "
                         f"with dynamic={self.dynamic}, motion={self.motion}")

    def _check_store(self, store, cam):
        lay = store.layout
        if lay["label_phase"] or lay["object_loss"] or lay["dynamic"] != self.dynamic or lay["motion"] != self.motion:
            raise ValueError(f"EvalPass: a store of layout {lay} does not hold graph.pack_frame(cam, gt[, accum_R][, gate][, accum_T]) frames "
                             f"with dynamic={self.dynamic}, motion={self.motion}")
        if (store.H, store.W) != (int(cam.image_height), int(cam.image_width)):
            raise ValueError(f"EvalPass: the store's frames are {store.W}x{store.H}, the camera {cam.image_width}x{cam.image_height}")

    def _make_static(self, cam, numel, dev):
        off, size, gated, H, W = self._layout(cam, numel)
        self._frame = torch.zeros(size, device=dev, dtype=torch.float32)
        fr = self._frame
        self._cam = _StaticCamera(cam, storage=fr[off["cam"][0]:off["cam"][1]])
        self._gt = fr[off["gt"][0]:off["gt"][1]].view(3, H, W)
        self._f = {"accum_R": fr[off["accum_R"][0]:off["accum_R"][1]].view(3, 3) if self.dynamic else None,
                   "accum_T": fr[off["accum_T"][0]:off["accum_T"][1]].view(3, 4) if self.motion else None}
        self._gate = fr[off["gate"][0]:off["gate"][1]].view(H, W) if gated else None
        self._shape = (3, H, W)
        self._key = (numel, H, W, float(cam.FoVx), float(cam.FoVy), dev)
        self.graph = None

    def _dynamic_kwargs(self):
        # exactly what GraphedTrainStep._dynamic_kwargs builds for a step without a trainable pose
        if not self.dynamic:
            return {}
        kw = dict(rot_cov=True, accum_R=self._f["accum_R"], which_object=self.which_object, during_training=False)
        if self.motion:
            from .motion import ComposedMotion
            kw["object_motion"] = ComposedMotion(self._f["accum_T"], self._f["accum_R"])
        return kw

    def _body(self, rows, cursor, guard):
        """One frame on the static inputs: the render, then the metric kernel writing at `cursor`."""
        with torch.no_grad():
            out = render(self._cam, self.pc, self.pipe, self.bg, color_only=True, **({"guard": guard} if guard is not None else {}),
                         **self._dynamic_kwargs())
            return out, fused.eval_metrics(out["render"], self._gt, keep=self._gate, rows=rows, cursor=cursor,
                                           overflow=None if guard is None else guard.overflow, out8=self.keep_images)

    # ---- capture --------------------------------------------------------------------------------------------------------------------
    def _capture(self, first_frame, n_rows, capacity, capacity_margin):
        dev = self._frame.device
        self.guard = _C.StepGuard(dev)
        self._rows, self._cursor = fused.eval_rows(n_rows, dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._frame.copy_(first_frame)
            self._body(None, None, None)                               # eager: sets the capacity hint, allocator pools, lazy state
            r_seen = _C.stats["num_rendered"]
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.capacity = max(int(r_seen * capacity_margin), _C.stats["capacity"]) if capacity is None else max(int(capacity), 1)
        _C.set_capacity_hint(self.capacity, dev)
        self._model_version = getattr(self.pc, "model_version", 0)
        self.graph = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            begin_capture(self.graph)
            try:
                self._captured = self._body(self._rows, self._cursor, self.guard)
            finally:
                end_capture(self.graph)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)

    def recapture(self):
        """Forget the captured graph (after the model reallocated its arrays, or changed its active SH degree): the next run() captures again."""
        self.graph = None

    def _read_rows(self, rows):
        """THE device-to-host read of a sweep's results (tests wrap it to count)."""
        self.host_reads += 1
        return rows.cpu()

    # ---- the sweep ------------------------------------------------------------------------------------------------------------------
    def run(self, frames, cam, capacity=None, capacity_margin=1.25):
        """frames: packed frames of graph.pack_frame(cam, gt, accum_R=, gate=keep, accum_T=) -- a list or an [F, frame] tensor; `gate` is
        keep = 1 - hand mask (frames packed without it keep every pixel) --, or a frames.FrameStore of that layout: every frame of it, each
        brought into the static buffers by one decode launch (from a ring set to 0 .. F - 1 before the sweep) instead of a copy.  cam: any camera of the sweep: the image size and field of view
        (a captured pass is specific to one, like a captured step).  capacity: the instance capacity to capture with, as is (default:
        capacity_margin x the first frame's count; frames that outgrow it are rendered again eagerly).
        -> dict(psnr, ssim: float64[F]; sse: int64[F]; mean_psnr, mean_ssim: the plain means; rerendered: indices of the frames rendered
        again; instances: int64[F], the captured forwards' instance counts (0 for eager frames)[; images: uint8[F,3,H,W] on the device])."""
        store = frames if isinstance(frames, FrameStore) else None
        if store is not None:
            self._check_store(store, cam)
            n, first = store.n_frames, store.frame(0)
            ring = store.new_ring(n)
            ring.set(range(n))                                          # the sweep's frames 0 .. n - 1: the decode walks them on the device
            load = lambda i: store.decode(self._frame, ring=ring)       # (called once per frame, in order)
            reload = lambda i: store.decode(self._frame, indices=[i])
        else:
            n = frames.shape[0] if torch.is_tensor(frames) else len(frames)
            if n == 0:
                raise ValueError("EvalPass.run: no frames")
            first = frames[0]
            load = reload = lambda i: self._frame.copy_(frames[i], non_blocking=True)      # the frame's every input: one copy
        if not first.is_cuda:
            raise RuntimeError(f"EvalPass: frames are on {first.device}: the evaluation pass has no CPU path (losses.eval_metrics is the torch statement)")
        dev = first.device
        key = (first.numel(), int(cam.image_height), int(cam.image_width), float(cam.FoVx), float(cam.FoVy), dev)
        if self._key != key:
            self._make_static(cam, first.numel(), dev)
        images = torch.empty((n,) + self._shape, dtype=torch.uint8, device=dev) if self.keep_images else None
        if self.graphed:
            if self.graph is not None and getattr(self.pc, "model_version", 0) != self._model_version:
                raise RuntimeError("EvalPass: the model reallocated its arrays (CapacityGaussians.grow) after this pass was captured; "
                                   "the captured launches point at freed memory -- call recapture() first")
            if self.graph is None or self._rows.shape[0] < n or (capacity is not None and int(capacity) != self.capacity):
                self._capture(first, max(n, 64), capacity, capacity_margin)
            rows, cursor = self._rows, self._cursor
            rows.zero_(); cursor.zero_()
            q = self._captured[1]["q_image"]
            for i in range(n):
                load(i)
                self.graph.replay()
                if images is not None:
                    images[i].copy_(q, non_blocking=True)
        else:
            rows, cursor = fused.eval_rows(n, dev)
            for i in range(n):
                load(i)
                _, res = self._body(rows, cursor, None)
                if images is not None:
                    images[i].copy_(res["q_image"], non_blocking=True)
        n_el = self._shape[0] * self._shape[1] * self._shape[2]
        fig = decode_rows(self._read_rows(rows[:n]), n_el)
        again = [int(i) for i in np.nonzero(fig["clipped"])[0]]
        if again:
            rows2, cursor2 = fused.eval_rows(len(again), dev)
            for i in again:
                reload(i)
                _, res = self._body(rows2, cursor2, None)                  # eager: the forward grows its buffers by itself
                if images is not None:
                    images[i].copy_(res["q_image"], non_blocking=True)
            fig2 = decode_rows(self._read_rows(rows2), n_el)
            for k in ("sse", "ssim_sum", "ssim", "psnr"):
                fig[k][again] = fig2[k]
        out = dict(psnr=fig["psnr"], ssim=fig["ssim"], sse=fig["sse"], mean_psnr=float(np.mean(fig["psnr"])), mean_ssim=float(np.mean(fig["ssim"])),
                   rerendered=again, instances=fig["instances"])
        if images is not None:
            out["images"] = images
        return out
