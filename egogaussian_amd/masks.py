"""The mask hand-off between the static stage and the background stage: predicted object masks, the model split, the dilated gate.

At the end of each static phase the reference (its trainers/train_static.py:167-197) sets is_object from the trained labels, splits the model
into an object and a background PLY and, for every static frame, renders the label, thresholds its channel mean at 0.5 and stores the result
as an 8-bit image; train.py:80-90 then completes the dataset's object masks with those predictions, and the background stage
(trainers/train_static_bg.py:14-21, 81-99) gates its image gradient by 1 - dilate_5(hand mask | object mask).

Here a sweep is, per frame, ONE device copy of a packed label frame (graph.pack_label_frame: camera[, gate], object mask) into static buffers
and ONE replay of a graph captured once under torch.no_grad(): the scalar-colour label forward -- the call of GraphedTrainStep's label step --
followed by the mask kernel (fused.label_mask / include/egs_raster.h egs_label_mask), which writes the frame's mask bytes and, at a device-side
cursor, its row: the predicted / target / intersection / kept pixel counts and the forward's overflow word.  The mask is copied into a
uint8[F,H,W] device tensor; the host reads the rows once, after the last frame.  A frame whose row says the captured instance capacity
clipped it is rendered again eagerly.  The gate itself is fused.interaction_gate, which can write straight into the `gate` segment of a
graph.pack_frame frame.  losses.label_mask / losses.interaction_gate are the torch statements of both definitions.

`masks` stays on the device (0 / 255, what the PNG holds); run(save_masks=paths) also writes them as 8-bit PNG files, encoded on the device
(png.PngWriter).  Copying them into a dataset is the caller's.
"""
import copy

import numpy as np
import torch

from . import fused
from .graph import frame_layout
from .renderer import label_forward
from .sweep import CapturedSweep


def decode_rows(rows):
    """rows: int64[F, 6] (include/egs_raster.h egs_mask_row), on any device -> dict of numpy arrays predicted, target, intersection, kept,
    instances (int64), clipped (bool), iou (float64): intersection / (predicted + target - intersection), 1.0 where that union is 0."""
    r = np.ascontiguousarray(rows.detach().cpu().numpy()).reshape(-1, fused.MASK_ROW_WORDS)
    pred, tgt, inter = r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()
    union = pred + tgt - inter
    iou = np.where(union == 0, 1.0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64))
    return dict(predicted=pred, target=tgt, intersection=inter, kept=r[:, 3].copy(), clipped=r[:, 4] != 0, instances=r[:, 5].copy(), iou=iou)


class MaskPass(CapturedSweep):
    _what, _statement = "mask pass", "losses.label_mask"
    _packed = "graph.pack_label_frame(cam, obj_mask[, gate])"
    _replaced = ("predicted", "target", "intersection", "kept", "iou")

    def __init__(self, pc, bg, graphed=True, threshold=0.5):
        """pc: the model whose labels are rendered (a capacity.CapacityGaussians model is followed through its live row count); bg: the
        label render's background, float32[3].  graphed=False: the same calls, eagerly, frame by frame (no capture, no capacity to outgrow).
        threshold: a pixel is predicted object when the channel mean of its label render exceeds it (the reference: 0.5)."""
        super().__init__(pc, bg, graphed)
        self.threshold = float(threshold)

    # ---- what the shared sweep asks for ----------------------------------------------------------------------------------------------
    def _frame_layout(self, H, W, gated):
        return frame_layout(0, H * W, gated=gated, label_phase=True)

    def _check_store(self, store):
        if not store.layout["label_phase"]:
            raise ValueError(f"MaskPass: a store of layout {store.layout} does not hold graph.pack_label_frame frames (label_phase=True)")

    def _set_static(self, views, H, W, dev):
        self._target, self._gate = views["obj_mask"], views["gate"]
        self._mask8 = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        self._shape = (H, W)

    def _body(self, rows, cursor, guard):
        """One frame on the static inputs: the label forward of GraphedTrainStep's label step, then the mask kernel writing at `cursor`."""
        with torch.no_grad():
            _, color, _, geom, binning, img = label_forward(self._cam, self.pc, self.pc.get_label, self.bg, guard=guard)
            res = fused.label_mask(color, self.threshold, target=self._target, keep=self._gate, rows=rows, cursor=cursor,
                                   overflow=None if guard is None else guard.overflow, out=self._mask8)
        return (color, geom, binning, img), res

    def _new_rows(self, n, dev):
        return fused.mask_rows(n, dev)

    def _decode(self, rows):
        return decode_rows(rows)

    def _new_out(self, n, dev):
        return torch.empty((n,) + self._shape, dtype=torch.uint8, device=dev)

    def _bytes(self, res):
        return self._mask8

    def run(self, frames, cam, capacity=None, capacity_margin=1.25, save_masks=None):
        """frames: packed frames of graph.pack_label_frame(cam, obj_mask[, gate=keep]) -- a list or an [F, frame] tensor; `gate` is
        keep = 1 - hand mask (frames packed without it count every pixel), the object mask is the target the prediction is counted against --,
        or a frames.FrameStore(label_phase=True): every frame of it, each brought into the static buffers by one decode launch (from a ring
        set to 0 .. F - 1 before the sweep) instead of a copy.
        cam: any camera of the sweep: the image size and field of view (a captured pass is specific to one).  capacity: the instance
        capacity to capture with, as is (default: capacity_margin x the first frame's count; frames that outgrow it are rendered again eagerly).
        -> dict(masks: uint8[F,H,W] on the device, 255 where the label render's channel mean exceeds the threshold -- every pixel, gated or
        not; predicted, target, intersection, kept: int64[F], counted over the kept pixels; iou: float64[F] (1.0 where the union is empty);
        mean_iou; rerendered: indices of the frames rendered again; instances: int64[F], the captured forwards' instance counts (0 for eager
        frames)).
        save_masks: F file names -- after the sweep the masks are encoded on the device and written as 8-bit PNG files (png.PngWriter; the
        result then also carries png_bytes, the file sizes).  The captured body is the same."""
        fig, again, masks = self._sweep(frames, cam, capacity, capacity_margin)
        out = dict(masks=masks, predicted=fig["predicted"], target=fig["target"], intersection=fig["intersection"], kept=fig["kept"],
                   iou=fig["iou"], mean_iou=float(np.mean(fig["iou"])), rerendered=again, instances=fig["instances"])
        if save_masks is not None:
            from .png import PngWriter
            F, H, W = masks.shape
            out["png_bytes"] = PngWriter(H, W, 1, masks.device, batch=min(F, 32)).save(masks, save_masks)
        return out


def infer_is_object_from_label(g):
    """GaussianModel.infer_is_object_from_label (the reference, scene/gaussian_model.py:1116-1121): is_object = 1 where the trained label
    exceeds 0.5, else 0, int32 [N,1].  A capacity.CapacityGaussians model keeps its array and only its live rows are written."""
    with torch.no_grad():
        label = g.get_label.detach()
        n = getattr(g, "n_active", None)
        if n is None:
            g._is_object = (label > 0.5).to(torch.int32).reshape(-1, 1)
            return g._is_object
        if g._is_object.dtype != torch.int32:
            g._is_object = g._is_object.to(torch.int32)
        g._is_object[:n] = (label[:n] > 0.5).to(torch.int32).reshape(-1, 1)
    return g._is_object


def split_object_background(g):
    """-> (obj, bg): two copies of `g`, one pruned to the Gaussians with is_object == 1 and one to those with is_object == 0, as the
    reference does before it saves the two PLY files (trainers/train_static.py:172-178: deepcopy, prune_points) -- pruned by
    densify.prune_points(..., during_training=False), which builds new arrays and writes into none.  `g` is unchanged and shares no
    per-Gaussian array with the halves; they carry no optimizer, and a capacity-sized model's halves hold its live rows only, as plain
    models.  Both are ready for ply.save_ply."""
    from .densify import prune_points
    n = getattr(g, "n_active", None)
    is_obj = g.get_is_object.detach()[:n].flatten()
    halves = []
    with torch.no_grad():
        for drop in (is_obj != 1, is_obj != 0):
            h = copy.copy(g)                                             # the arrays are replaced below, never written
            h.optimizer = None
            h.__dict__.pop("_sel_cache", None)
            if n is not None:                                            # a plain model of the live rows: nothing beyond them belongs to it
                from .capacity import CapacityGaussians
                from .scene_synth import SynthGaussians
                if type(h) is CapacityGaussians:
                    h.__class__ = SynthGaussians
                for a in ("capacity", "n_active", "active_count"):
                    h.__dict__.pop(a, None)
            for a in _PER_GAUSSIAN:
                t = getattr(h, a, None)
                if torch.is_tensor(t):
                    setattr(h, a, t.detach()[:n])
            prune_points(h, drop, during_training=False)
            for a in _STATS:                                             # (prune_points leaves the training statistics to a training model)
                t = getattr(h, a, None)
                if torch.is_tensor(t):
                    setattr(h, a, t[~drop].clone())
            halves.append(h)
    return halves[0], halves[1]


_PER_GAUSSIAN = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_label", "_is_object", "_generation",
                 "max_radii2D", "xyz_gradient_accum", "denom")
_STATS = ("max_radii2D", "xyz_gradient_accum", "denom")
