"""The evaluation pass: per-frame PSNR and SSIM as the reference reports them, without leaving the device between frames.

The reference's eval_and_metric (its trainers/eval_metric.py:41-175) places the object by each frame's pose, renders it
(rot_cov=True, accum_R, which_object=1, no_grad), writes render, ground truth and 1 - hand mask to 8-bit PNGs, reads them back, multiplies
both images by the mask and averages ssim / psnr over the frames: its results.txt is defined on 8-bit images with the hand removed.  Here a
sweep is, per frame, ONE device copy of a packed frame (graph.pack_frame) into static buffers and ONE replay of a graph captured once under
torch.no_grad(): the render (colour only) followed by the metric kernel (fused.eval_metrics / include/egs_raster.h egs_eval_metrics), which
writes the frame's row -- squared 8-bit error, SSIM sum, the forward's overflow word -- at a device-side cursor.  The host reads the rows
once, after the last frame.  A frame whose row says the captured instance capacity clipped it is rendered again eagerly (the eager forward
sizes its buffers itself) and measured by the same kernel: an evaluation is never silently clipped.

LPIPS, the reference's third figure, joins the same replay when the caller hands over the VGG weights (EvalPass(lpips=lpips.LPIPS(...));
this package ships none): the metric kernel's quantised images and the frame's gate go through csrc/lpips.hip inside the captured body, the
frame's six float64 figures land at a cursor of their own, and the sweep's one host read fetches both row arrays together.
losses.eval_metrics and lpips.lpips_vgg are the torch statements of the per-frame definitions.
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


def decode_lpips_rows(rows):
    """rows: float64[F, 6] (include/egs_raster.h egs_lpips_forward), on any device -> dict of numpy arrays lpips_taps [F,5], lpips [F]."""
    r = np.ascontiguousarray(rows.detach().cpu().numpy()).reshape(-1, fused.LPIPS_ROW_WORDS)
    return dict(lpips_taps=r[:, :5].copy(), lpips=r[:, 5].copy())


class EvalPass(CapturedSweep):
    _what, _statement = "evaluation pass", "losses.eval_metrics"
    _packed = "graph.pack_frame(cam, gt[, accum_R][, gate][, accum_T])"
    _replaced = ("sse", "ssim_sum", "ssim", "psnr")

    def __init__(self, pc, bg, pipe=Pipe, dynamic=False, motion=False, which_object=1, graphed=True, keep_images=False, lpips=None):
        """dynamic / motion / which_object: as graph.GraphedTrainStep -- the render is called exactly as its captured step calls it
        (rot_cov=True, accum_R from the frame; with motion the object is placed by the frame's accum_T inside the rasterizer).
        graphed=False: the same calls, eagerly, frame by frame (no capture, no capacity to outgrow).
        keep_images: run() also returns the quantised renders, uint8[F,3,H,W] on the device -- what goes into the PNGs.
        lpips: an lpips.LPIPS -- run() also returns the frames' LPIPS (of the quantised, gated images), computed inside the same body.
        A capacity.CapacityGaussians model is followed through its live row count like every render()."""
        if motion and not dynamic:
            raise ValueError("EvalPass(motion=True) goes with dynamic=True (the pose's rotation turns the covariances)")
        super().__init__(pc, bg, graphed)
        self.pipe, self.keep_images = pipe, bool(keep_images)
        self.dynamic, self.motion, self.which_object = bool(dynamic), bool(motion), which_object
        self.lpips = lpips
        if lpips is not None:
            self._replaced = EvalPass._replaced + ("lpips", "lpips_taps")

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
            res = fused.eval_metrics(out["render"], self._gt, keep=self._gate, rows=rows, cursor=cursor,
                                     overflow=None if guard is None else guard.overflow, out8=self.keep_images or self.lpips is not None)
            if self.lpips is not None:
                lp_rows, lp_cursor = (None, None) if rows is None else self._partner(rows)
                self.lpips(res["q_image"], res["q_gt"], keep=self._gate, rows=lp_rows, cursor=lp_cursor)
            return out, res

    def _new_rows(self, n, dev):
        rows, cursor = fused.eval_rows(n, dev)
        if self.lpips is not None:
            rows.lpips_partner = fused.lpips_rows(n, dev)                      # the row array carries its LPIPS (rows, cursor): one lifetime
        return rows, cursor

    @staticmethod
    def _partner(rows):
        """The LPIPS (rows, cursor) that _new_rows gave this row array (or the array `rows` is a slice of), else None."""
        return getattr(rows if rows._base is None else rows._base, "lpips_partner", None)

    def _read_rows(self, rows):
        """Still ONE read: the LPIPS rows travel as six more int64 words of each row."""
        lp = self._partner(rows)
        if lp is None:
            return super()._read_rows(rows)
        self.host_reads += 1
        return torch.cat([rows, lp[0][:rows.shape[0]].view(torch.int64)], 1).cpu()

    def _decode(self, rows):
        fig = decode_rows(rows[:, :fused.EVAL_ROW_WORDS].contiguous(), self._shape[0] * self._shape[1] * self._shape[2])
        if rows.shape[1] > fused.EVAL_ROW_WORDS:
            fig.update(decode_lpips_rows(rows[:, fused.EVAL_ROW_WORDS:].contiguous().view(torch.float64)))
        return fig

    def _new_out(self, n, dev):
        return torch.empty((n,) + self._shape, dtype=torch.uint8, device=dev) if self.keep_images else None

    def _bytes(self, res):
        return res["q_image"]

    def run(self, frames, cam, capacity=None, capacity_margin=1.25, save_renders=None):
        """frames: packed frames of graph.pack_frame(cam, gt, accum_R=, gate=keep, accum_T=) -- a list or an [F, frame] tensor; `gate` is
        keep = 1 - hand mask (frames packed without it keep every pixel) --, or a frames.FrameStore of that layout: every frame of it, each
        brought into the static buffers by one decode launch (from a ring set to 0 .. F - 1 before the sweep) instead of a copy.  cam: any camera of the sweep: the image size and field of view
        (a captured pass is specific to one, like a captured step).  capacity: the instance capacity to capture with, as is (default:
        capacity_margin x the first frame's count; frames that outgrow it are rendered again eagerly).
        -> dict(psnr, ssim: float64[F]; sse: int64[F]; mean_psnr, mean_ssim: the plain means; rerendered: indices of the frames rendered
        again; instances: int64[F], the captured forwards' instance counts (0 for eager frames)[; images: uint8[F,3,H,W] on the device]
        [; lpips: float64[F], lpips_taps: float64[F,5], mean_lpips -- with lpips=]).
        save_renders: F file names -- after the sweep the quantised renders are encoded on the device and written as 8-bit PNG files
        (png.PngWriter; needs keep_images=True; the result then also carries png_bytes, the file sizes).  The captured body is the same."""
        if save_renders is not None and not self.keep_images:
            raise ValueError("EvalPass.run(save_renders=) writes the quantised renders: construct the pass with keep_images=True")
        if self.lpips is not None and self.graph is not None:
            for t in self._partner(self._rows):                                # the captured rows' partner starts again at row 0, as they do
                t.zero_()
        fig, again, images = self._sweep(frames, cam, capacity, capacity_margin)
        out = dict(psnr=fig["psnr"], ssim=fig["ssim"], sse=fig["sse"], mean_psnr=float(np.mean(fig["psnr"])), mean_ssim=float(np.mean(fig["ssim"])),
                   rerendered=again, instances=fig["instances"])
        if images is not None:
            out["images"] = images
        if save_renders is not None:
            from .png import PngWriter
            F, C, H, W = images.shape
            out["png_bytes"] = PngWriter(H, W, C, images.device, batch=min(F, 32)).save(images, save_renders)
        if self.lpips is not None:
            out.update(lpips=fig["lpips"], lpips_taps=fig["lpips_taps"], mean_lpips=float(np.mean(fig["lpips"])))
        return out


def metrics_from_files(renders, gts, hands, lpips=None, device="cuda", batch=32, segments=False):
    """The device route of the reference's calculate_metric (its trainers/eval_metric.py:129-175): the figures of a directory of 8-bit PNG
    files -- renders[k], gts[k] (RGB) and hands[k] (1 or 3 channels, channel 0 is used; the file render_results wrote: 255 where the pixel
    counts) -- paths or bytes.  The files go up as they are and are decoded on the device (png.PngReader); keep = (hand byte / 255) >= 0.5,
    the images are byte / 255 as planar float tensors, and the same kernels as EvalPass measure them (fused.eval_metrics and, with
    lpips=lpips.LPIPS(...), csrc/lpips.hip) -- an EvalPass sweep that saved these files reports the same sse, ssim_sum and LPIPS rows.
    A hand file with a byte other than 0 / 255 raises ValueError: masks are binary by contract (include/egs_raster.h egs_eval_metrics).
    One read of the decoder's status words per batch of files, one of the hand check, one of the rows.  segments=True decodes with the
    segmented route (png.PngReader): the files EvalPass.run(save_renders=) wrote take it; the rows are the same either way.
    -> dict(ssim, psnr[, lpips]: float64[F]; sse: int64[F]; ssim_sum: float64[F]; rows: [(ssim, psnr[, lpips])] per file; means: the same
    tuple of plain means, in the reference's order SSIM, PSNR, LPIPS)."""
    from . import png as _png
    renders, gts, hands = list(renders), list(gts), list(hands)
    F = len(renders)
    if F < 1 or len(gts) != F or len(hands) != F:
        raise ValueError(f"metrics_from_files: {F} renders, {len(gts)} ground truths and {len(hands)} hand masks; one of each per frame, at least one")
    dev = torch.device(device)
    reader = _png.PngReader(dev, batch=batch, segments=segments)
    try:
        arrays = reader.read(renders + gts + hands)
    except ValueError as e:
        raise ValueError(f"metrics_from_files: {e} (files 0 .. {F - 1}: renders, then the ground truths, then the hand masks)") from None
    triples = []
    for k in range(F):
        r, g, h = arrays[k], arrays[F + k], arrays[2 * F + k]
        if r.shape[2] != 3 or r.shape != g.shape or h.shape[:2] != r.shape[:2]:
            raise ValueError(f"metrics_from_files: frame {k}: render {tuple(r.shape)}, ground truth {tuple(g.shape)}, hand mask {tuple(h.shape)}; "
                             "the images are [h,w,3] of one size and the mask has their size")
        triples.append((r, g, h[:, :, 0]))
    grey = torch.stack([((h != 0) & (h != 255)).any() for _, _, h in triples]).cpu().tolist()
    if any(grey):
        raise ValueError(f"metrics_from_files: hand mask(s) {[k for k, b in enumerate(grey) if b]} hold bytes other than 0 and 255: masks are binary "
                         "by contract")
    rows, cursor = fused.eval_rows(F, dev)
    lp_rows, lp_cursor = fused.lpips_rows(F, dev) if lpips is not None else (None, None)
    sizes = []
    with torch.no_grad():
        for r, g, h in triples:
            image, gt = r.permute(2, 0, 1).to(torch.float32) / 255, g.permute(2, 0, 1).to(torch.float32) / 255
            keep = (h.to(torch.float32) / 255 >= 0.5).to(torch.float32)
            res = fused.eval_metrics(image.contiguous(), gt.contiguous(), keep=keep, rows=rows, cursor=cursor, out8=lpips is not None)
            if lpips is not None:
                lpips(res["q_image"], res["q_gt"], keep=keep, rows=lp_rows, cursor=lp_cursor)
            sizes.append(image.numel())
    both = rows if lpips is None else torch.cat([rows, lp_rows.view(torch.int64)], 1)
    both = both.cpu()
    out = dict(sse=np.zeros(F, dtype=np.int64), ssim_sum=np.zeros(F), ssim=np.zeros(F), psnr=np.zeros(F))
    for k in range(F):
        fig = decode_rows(both[k:k + 1, :fused.EVAL_ROW_WORDS].contiguous(), sizes[k])
        for name in out:
            out[name][k] = fig[name][0]
    names = ["ssim", "psnr"]
    if lpips is not None:
        out.update(decode_lpips_rows(both[:, fused.EVAL_ROW_WORDS:].contiguous().view(torch.float64)))
        names.append("lpips")
    out["rows"] = [tuple(float(out[n][k]) for n in names) for k in range(F)]
    out["means"] = tuple(float(np.mean(out[n])) for n in names)
    return out
