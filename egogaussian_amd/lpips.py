"""LPIPS with the VGG-16 backbone: the third figure of the reference's evaluation (its trainers/eval_metric.py:129-175 reports
lpips(render * hand, gt * hand, net_type='vgg') next to SSIM and PSNR).

lpips_vgg is the torch statement of the definition -- any device, any float type --, as losses.py is for the loss kernels; LPIPS runs the
same definition by the HIP kernels of csrc/lpips.hip (include/egs_raster.h egs_lpips_forward), which evaluate.EvalPass(lpips=) puts into
its captured frame.  Weights are handed in by the caller (LPIPSWeights): this package ships none.

The definition is UNPINNED against the lpipsPyTorch package the reference imports: that package is not part of the reference's tree, so the
statement is written from the published definition (Zhang et al. 2018, the `lpips` network with `lin` heads), the same standing as the
rasterizer's oracle.  Two points a holder of the package should check against it:
  * the inputs are used as they are, in [0, 1]: the reference does not map them to [-1, 1] before the z-score;
  * the channel normalisation is f / (sqrt(sum_c f^2) + 1e-10): the eps is outside the root.
"""
import ctypes as C

import torch
import torch.nn.functional as F

MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10
# (Cin, Cout) of the 13 convolutions; the blocks; a 2x2 / stride 2 / floor max pool between blocks; a tap after each block's last ReLU
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
BLOCKS = (2, 2, 3, 3, 3)
TAP_CHANNELS = (64, 128, 256, 512, 512)
VGG_FEATURE_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # the convolutions of torchvision's vgg16().features
MIN_SIDE = 16                                                               # four pools: a smaller side leaves the last block no pixel


class LPIPSWeights:
    """13 (weight [Cout,Cin,3,3], bias [Cout]) pairs and five [C] linear-head vectors, float32, on `device` (the constructors: the CPU;
    to(device) gives a copy elsewhere, so that lpips_vgg on a device does not upload them per call)."""

    def __init__(self, convs, lins, device="cpu"):
        convs = [(w.detach().float().to(device).contiguous(), b.detach().float().to(device).contiguous()) for w, b in convs]
        lins = [l.detach().float().to(device).reshape(-1).contiguous() for l in lins]
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError(f"LPIPSWeights: 13 convolutions and 5 linear heads, not {len(convs)} and {len(lins)}")
        for k, ((w, b), (ci, co)) in enumerate(zip(convs, CONV_CHANNELS)):
            if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
                raise ValueError(f"LPIPSWeights: convolution {k} is {tuple(w.shape)} / {tuple(b.shape)}, not {(co, ci, 3, 3)} / {(co,)}")
        for k, (l, c) in enumerate(zip(lins, TAP_CHANNELS)):
            if l.numel() != c:
                raise ValueError(f"LPIPSWeights: linear head {k} holds {l.numel()} weights, not {c}")
        self.convs, self.lins = convs, lins

    def to(self, device):
        return LPIPSWeights(self.convs, self.lins, device)

    @classmethod
    def from_tensors(cls, conv_weights, conv_biases, lin_weights):
        return cls(list(zip(conv_weights, conv_biases)), list(lin_weights))

    @classmethod
    def from_state_dicts(cls, vgg_state, lin_state):
        """vgg_state: torchvision's vgg16 state dict, `features.{0,2,5,...,28}.{weight,bias}` (the classifier's entries are ignored).
        lin_state: the linear heads as [1,C,1,1] tensors under `lin{k}.model.1.weight` (the lpips package) or `{k}.1.weight`
        (lpipsPyTorch), k = 0 .. 4."""
        convs = []
        for i in VGG_FEATURE_INDICES:
            kw, kb = f"features.{i}.weight", f"features.{i}.bias"
            if kw not in vgg_state or kb not in vgg_state:
                raise KeyError(f"LPIPSWeights.from_state_dicts: no {kw} / {kb} among {sorted(vgg_state)}")
            convs.append((vgg_state[kw], vgg_state[kb]))
        lins = []
        for k in range(5):
            for key in (f"lin{k}.model.1.weight", f"{k}.1.weight"):
                if key in lin_state:
                    lins.append(lin_state[key])
                    break
            else:
                raise KeyError(f"LPIPSWeights.from_state_dicts: neither lin{k}.model.1.weight nor {k}.1.weight among {sorted(lin_state)}")
            if tuple(lins[-1].shape) != (1, TAP_CHANNELS[k], 1, 1):
                raise ValueError(f"LPIPSWeights.from_state_dicts: head {k} is {tuple(lins[-1].shape)}, not {(1, TAP_CHANNELS[k], 1, 1)}")
        return cls(convs, lins)

    @classmethod
    def random(cls, seed):
        """The tests' model: weights N(0, 2 / (9 Cin)), biases N(0, 0.05^2), linear weights U(0, 0.1) -- activations stay O(1) through all
        13 layers (taps 1.2e-2 .. 3e-4, sum ~ 2.3e-2 on independent random 8-bit images)."""
        g = torch.Generator().manual_seed(int(seed))
        convs = [(torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5, torch.randn(co, generator=g) * 0.05) for ci, co in CONV_CHANNELS]
        return cls(convs, [torch.rand(c, generator=g) * 0.1 for c in TAP_CHANNELS])


def vgg_taps(v, weights):
    """The five tap feature maps [C_k, H_k, W_k] of one image v [3,H,W] in [0,1] (same device and dtype as v)."""
    dev, dt = v.device, v.dtype
    f = ((v - torch.tensor(MEAN, device=dev, dtype=dt)[:, None, None]) / torch.tensor(STD, device=dev, dtype=dt)[:, None, None])[None]
    taps, layer = [], 0
    for k, n in enumerate(BLOCKS):
        if k:
            f = F.max_pool2d(f, 2, 2)                                      # floor
        for _ in range(n):
            w, b = weights.convs[layer]
            f = F.relu(F.conv2d(f, w.to(dev, dt), b.to(dev, dt), padding=1))      # zero padding, in z-scored space
            layer += 1
        taps.append(f[0])
    return taps


def lpips_vgg(x, y, weights):
    """x, y: [3,H,W] in [0,1] (used as they are), H, W >= 16; weights: LPIPSWeights -> (taps [5], lpips = their sum), in x's float type."""
    if x.dim() != 3 or x.shape[0] != 3 or x.shape != y.shape:
        raise ValueError("lpips_vgg: x and y are [3,H,W] tensors of one shape")
    if min(x.shape[1:]) < MIN_SIDE:
        raise ValueError(f"lpips_vgg: {x.shape[2]}x{x.shape[1]} is smaller than {MIN_SIDE} on a side: a pool would have no output")
    vals = []
    for fx, fy, l in zip(vgg_taps(x, weights), vgg_taps(y, weights), weights.lins):
        nx = fx / (fx.pow(2).sum(0, keepdim=True).sqrt() + EPS)            # eps outside the root
        ny = fy / (fy.pow(2).sum(0, keepdim=True).sqrt() + EPS)
        vals.append((l.to(x.device, x.dtype)[:, None, None] * (nx - ny).pow(2)).sum(0).mean())
    taps = torch.stack(vals)
    return taps, taps.sum()


# ---- the HIP path ---------------------------------------------------------------------------------------------------------------------
def pack_conv_weight(w):
    """[Cout,Cin,3,3] -> the kernels' K-major [9 Cin', Cout] (row (3 ky + kx) * Cin' + c), Cin' = Cin padded 3 -> 4 with zeros."""
    w = w.float()
    if w.shape[1] == 3:
        w = F.pad(w, (0, 0, 0, 0, 0, 1))
    return w.permute(2, 3, 1, 0).reshape(9 * w.shape[1], w.shape[0]).contiguous()


def conv3x3_relu_nhwc(x, packed_w, bias):
    """One layer by the HIP kernel (egs_conv3x3_relu_nhwc): x float32 [n,H,W,Cin] on the device -> relu(conv3x3(x) + bias) [n,H,W,Cout]."""
    from . import _hip, lib as _lib
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise RuntimeError("conv3x3_relu_nhwc: x is a contiguous float32 [n,H,W,Cin] tensor on a HIP device (lpips.vgg_taps is the torch statement)")
    n, H, W, cin = x.shape
    if packed_w.shape[0] != 9 * cin or not (packed_w.is_contiguous() and bias.is_contiguous() and packed_w.device == x.device == bias.device):
        raise RuntimeError("conv3x3_relu_nhwc: packed_w is pack_conv_weight's [9 Cin, Cout] on x's device")
    out = torch.empty((n, H, W, packed_w.shape[1]), dtype=torch.float32, device=x.device)
    with _hip.device_ctx(x.device):
        _lib.check(_lib.load().egs_conv3x3_relu_nhwc(n, H, W, cin, packed_w.shape[1], x.data_ptr(), packed_w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                     _hip.stream_of(x.device)))
    return out


class LPIPS:
    """lpips_vgg by the HIP kernels.  weights: LPIPSWeights, repacked once here and kept on `device`.  No fallback: a CPU tensor raises."""

    def __init__(self, weights, device):
        from . import lib as _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"LPIPS: {self.device} is no HIP device (lpips.lpips_vgg is the torch statement)")
        self._lib = _lib.load()
        self._w = [pack_conv_weight(w).to(self.device) for w, _ in weights.convs]
        self._b = [b.to(self.device) for _, b in weights.convs]
        self._l = [l.to(self.device) for l in weights.lins]
        self._struct = _lib.LpipsWeights()
        for i in range(13):
            self._struct.conv_w[i], self._struct.conv_b[i] = self._w[i].data_ptr(), self._b[i].data_ptr()
        for k in range(5):
            self._struct.lin[k] = self._l[k].data_ptr()
        self._workspaces, self._size = {}, None

    def workspace(self, H, W):
        """The workspace of an H x W pair: 412 H W floats -- 0.85 GB at 960 x 540 --, as all five tap maps stay in it.  One per size, and
        one that was handed out is never dropped while this object lives: a captured graph (evaluate.EvalPass) has its address in its
        launches, and a call at another size in between must not free it.  release_workspaces() is the explicit way to give them back."""
        ws = self._workspaces.get((H, W))
        if ws is None:
            n = int(self._lib.egs_lpips_workspace_bytes(H, W))
            if n == 0:
                raise ValueError(f"LPIPS: {W}x{H} is outside {MIN_SIDE} .. 8192 on a side")
            ws = self._workspaces[(H, W)] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return ws

    def release_workspaces(self):
        """Drop every workspace.  Only when no captured graph that ran this object will be replayed again (EvalPass.recapture() first)."""
        self._workspaces, self._size = {}, None

    def __call__(self, q_x, q_y, keep=None, rows=None, cursor=None):
        """q_x, q_y: uint8 [3,H,W] on the device -- fused.eval_metrics(out8=True)'s q_image / q_gt --, keep: float [H,W] or None (kept =
        keep >= 0.5; a removed pixel is 0 in both images, as the reference's `* hand`).  rows, cursor: fused.lpips_rows(capacity, device): the
        kernel writes row cursor[0] = (tap_1 .. tap_5, lpips) and advances the cursor on the device; None: a fresh one-row array.
        Does not synchronise.  -> dict(rows, cursor)."""
        from . import _hip, fused, lib as _lib
        for t, name in ((q_x, "q_x"), (q_y, "q_y")):
            if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[0] == 3 and t.is_contiguous() and t.device == self.device):
                raise RuntimeError(f"LPIPS: {name} is a contiguous uint8 [3,H,W] tensor on {self.device}")
        if q_x.shape != q_y.shape:
            raise RuntimeError("LPIPS: q_x and q_y have one shape")
        _, H, W = q_x.shape
        if min(H, W) < MIN_SIDE:
            raise ValueError(f"LPIPS: {W}x{H} is smaller than {MIN_SIDE} on a side: a pool would have no output")
        k = None
        if keep is not None:
            k = keep.detach()
            if not (k.device == self.device and k.dtype == torch.float32 and k.numel() == H * W and k.is_contiguous()):
                raise RuntimeError(f"LPIPS: keep is a contiguous float32 [H,W] tensor on {self.device}")
        if (rows is None) != (cursor is None):
            raise RuntimeError("LPIPS: rows and cursor go together (fused.lpips_rows)")
        if rows is None:
            rows, cursor = fused.lpips_rows(1, self.device)
        if not (rows.is_cuda and rows.dtype == torch.float64 and rows.dim() == 2 and rows.shape[1] == fused.LPIPS_ROW_WORDS and rows.is_contiguous()
                and rows.device == self.device and cursor.device == self.device and cursor.dtype == torch.int32 and cursor.numel() == 1):
            raise RuntimeError("LPIPS: rows is a contiguous float64[capacity, 6] tensor and cursor an int32[1] tensor on the images' device")
        ws = self.workspace(H, W)
        self._size = (H, W)
        with _hip.device_ctx(self.device):
            _lib.check(self._lib.egs_lpips_forward(H, W, q_x.data_ptr(), q_y.data_ptr(), None if k is None else k.data_ptr(), C.byref(self._struct),
                                                   ws.data_ptr(), rows.data_ptr(), int(rows.shape[0]), cursor.data_ptr(), _hip.stream_of(self.device)))
        return dict(rows=rows, cursor=cursor)

    def features(self, size=None):
        """The five tap maps as views into the workspace of `size` = (H, W): float32 [2, H_k, W_k, C_k] (image x, image y; channel-last) --
        what the last run at that size left.  Default: the size of the last call made through this object (the replay of a captured graph is
        no such call)."""
        size = self._size if size is None else (int(size[0]), int(size[1]))
        if size not in self._workspaces:
            raise RuntimeError("LPIPS.features: nothing has run yet" + ("" if size is None else f" at {size[1]}x{size[0]}"))
        H, W = size
        ws = self._workspaces[size]
        off = (C.c_int64 * 5)()
        from . import lib as _lib
        _lib.check(self._lib.egs_lpips_tap_offsets(H, W, off))
        out = []
        for k, c in enumerate(TAP_CHANNELS):
            h, w = H >> k, W >> k
            out.append(ws[off[k]: off[k] + 2 * h * w * c * 4].view(torch.float32).view(2, h, w, c))
        return out
