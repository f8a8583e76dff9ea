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

from . import fused
from .graph import dynamic_kwargs, frame_layout
from .renderer import render
from .scene_synth import Pipe
from .sweep import CapturedSweep


def decode_rows(rows, n_elements):
    """rows: int64[F, 4] (include/egs_raster.h egs_eval_row), on any device -> dict of numpy arrays sse (int64), ssim_sum, ssim, psnr
    (float64), clipped (bool), instances (int64).  psnr = 10 log10(255^2 n / sse), inf where sse == 0; ssim = ssim_sum / n; n = C*H*W."""
    r = np.ascontiguousarray(rows.detach().cpu().numpy()).reshape(-1, fused.EVAL_ROW_WORDS)
    sse = r[:, 0].copy()
    ssim_sum = r[:, 1].copy().view(np.float64)
    with np.errstate(divide="ignore"):
        psnr = np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 * float(n_elements) / np.maximum(sse, 1).astype(np.float64)))
    return dict(sse=sse, ssim_sum=ssim_sum, ssim=ssim_sum / float(n_elements), psnr=psnr, clipped=r[:, 2] != 0, instances=r[:, 3].copy())


class EvalPass(CapturedSweep):
    _what, _statement = "evaluation pass", "losses.eval_metrics"
    _packed = "graph.pack_frame(cam, gt[, accum_R][, gate][, accum_T])"
    _replaced = ("sse", "ssim_sum", "ssim", "psnr")

    def __init__(self, pc, bg, pipe=Pipe, dynamic=False, motion=False, which_object=1, graphed=True, keep_images=False):
        """dynamic / motion / which_object: as graph.GraphedTrainStep -- the render is called exactly as its captured step calls it
        (rot_cov=True, accum_R from the frame; with motion the object is placed by the frame's accum_T inside the rasterizer).
        graphed=False: the same calls, eagerly, frame by frame (no capture, no capacity to outgrow).
        keep_images: run() also returns the quantised renders, uint8[F,3,H,W] on the device -- what goes into the PNGs.
        A capacity.CapacityGaussians model is followed through its live row count like every render()."""
        if motion and not dynamic:
            raise ValueError("EvalPass(motion=True) goes with dynamic=True (the pose's rotation turns the covariances)")
        super().__init__(pc, bg, graphed)
        self.pipe, self.keep_images = pipe, bool(keep_images)
        self.dynamic, self.motion, self.which_object = bool(dynamic), bool(motion), which_object

    # ---- what the shared sweep asks for ----------------------------------------------------------------------------------------------
    def _options(self):
        return f" with dynamic={self.dynamic}, motion={self.motion}"

    def _frame_layout(self, H, W, gated):
        return frame_layout(3 * H * W, H * W, self.dynamic, gated, self.motion)

    def _check_store(self, store):
        lay = store.layout
        if lay["label_phase"] or lay["object_loss"] or lay.get("pose_rows") or lay["dynamic"] != self.dynamic or lay["motion"] != self.motion:
            raise ValueError(f"EvalPass: a store of layout {lay} does not hold {self._packed} frames{self._options()}")

    def _set_static(self, views, H, W, dev):
        self._f, self._gt, self._gate = views, views["gt"], views["gate"]
        self._shape = (3, H, W)

    def _body(self, rows, cursor, guard):
        """One frame on the static inputs: the render, then the metric kernel writing at `cursor`."""
        with torch.no_grad():
            out = render(self._cam, self.pc, self.pipe, self.bg, color_only=True, **({"guard": guard} if guard is not None else {}),
                         **(dynamic_kwargs(self._f, self.which_object) if self.dynamic else {}))
            return out, fused.eval_metrics(out["render"], self._gt, keep=self._gate, rows=rows, cursor=cursor,
                                           overflow=None if guard is None else guard.overflow, out8=self.keep_images)

    def _new_rows(self, n, dev):
        return fused.eval_rows(n, dev)

    def _decode(self, rows):
        return decode_rows(rows, self._shape[0] * self._shape[1] * self._shape[2])

    def _new_out(self, n, dev):
        return torch.empty((n,) + self._shape, dtype=torch.uint8, device=dev) if self.keep_images else None

    def _bytes(self, res):
        return res["q_image"]

    def run(self, frames, cam, capacity=None, capacity_margin=1.25):
        """frames: packed frames of graph.pack_frame(cam, gt, accum_R=, gate=keep, accum_T=) -- a list or an [F, frame] tensor; `gate` is
        keep = 1 - hand mask (frames packed without it keep every pixel) --, or a frames.FrameStore of that layout: every frame of it, each
        brought into the static buffers by one decode launch (from a ring set to 0 .. F - 1 before the sweep) instead of a copy.  cam: any camera of the sweep: the image size and field of view
        (a captured pass is specific to one, like a captured step).  capacity: the instance capacity to capture with, as is (default:
        capacity_margin x the first frame's count; frames that outgrow it are rendered again eagerly).
        -> dict(psnr, ssim: float64[F]; sse: int64[F]; mean_psnr, mean_ssim: the plain means; rerendered: indices of the frames rendered
        again; instances: int64[F], the captured forwards' instance counts (0 for eager frames)[; images: uint8[F,3,H,W] on the device])."""
        fig, again, images = self._sweep(frames, cam, capacity, capacity_margin)
        out = dict(psnr=fig["psnr"], ssim=fig["ssim"], sse=fig["sse"], mean_psnr=float(np.mean(fig["psnr"])), mean_ssim=float(np.mean(fig["ssim"])),
                   rerendered=again, instances=fig["instances"])
        if images is not None:
            out["images"] = images
        return out
