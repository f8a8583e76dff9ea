"""Image losses and PSNR of the reference's training step (PyTorch ops, run on whatever device the images are on).

l1_loss / l2_loss / ssim follow /root/reference/utils/loss_utils.py:57-107 (11x11 Gaussian window, sigma 1.5,
zero padding 5, C1 = 0.01^2, C2 = 0.03^2, per-channel depthwise); psnr follows /root/reference/utils/image_utils.py:14-19
(20 log10(1/sqrt(mse)) per image).  The window is applied as its two 1-D factors (the 2-D window is their outer
product), which is the same filter at a fifth of the work.
"""
import math

import torch
import torch.nn.functional as F


def l1_loss(a, b):
    return (a - b).abs().mean()


def l2_loss(a, b):
    return ((a - b) ** 2).mean()


def _gauss1d(size, sigma, device, dtype):
    g = torch.tensor([math.exp(-(x - size // 2) ** 2 / (2.0 * sigma ** 2)) for x in range(size)], device=device, dtype=dtype)
    return g / g.sum()


def _blur(x, g, C):
    k = g.numel()
    x = F.conv2d(x, g.view(1, 1, k, 1).expand(C, 1, k, 1), padding=(k // 2, 0), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, k).expand(C, 1, 1, k), padding=(0, k // 2), groups=C)


def ssim(img1, img2, window_size=11, size_average=True):
    squeeze = img1.dim() == 3
    if squeeze:
        img1, img2 = img1.unsqueeze(0), img2.unsqueeze(0)
    C = img1.shape[1]
    g = _gauss1d(window_size, 1.5, img1.device, img1.dtype)
    mu1, mu2 = _blur(img1, g, C), _blur(img2, g, C)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _blur(img1 * img1, g, C) - mu1_sq
    s2 = _blur(img2 * img2, g, C) - mu2_sq
    s12 = _blur(img1 * img2, g, C) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def training_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda) L1 + lambda (1 - SSIM), /root/reference/trainers/train_static.py:92-95, arguments/__init__.py:83."""
    return (1.0 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1.0 - ssim(image, gt))


def object_stage_loss(image, alpha, gt, obj_mask, lambda_dssim, lambda_image=1.0, lambda_l1_alpha=0.0, lambda_l2_alpha=0.5):
    """The loss of the stages that recover the object's motion (/root/reference/trainers/coarse_obj_pose.py:239-260,
    trainers/fine_obj.py:128-151):
        lambda_image * [(1 - lambda) L1 + lambda (1 - SSIM)](gt * obj_mask, image) + lambda_l1_alpha * L1(obj_mask, alpha)
            + lambda_l2_alpha * L2(obj_mask, alpha)
    `gt` is the frame as loaded: it is multiplied by the mask HERE.  alpha, obj_mask: [1,H,W] or [H,W].  The hand-mask hooks of the
    reference (grad * (1 - hand_mask) on the image and on alpha) are the caller's; fused.object_stage_loss takes them as grad_gate.
    The oracle of the HIP kernels behind fused.object_stage_loss, on any device and in any float type."""
    m = obj_mask.to(image.dtype)
    gtm = gt * m
    img = (1.0 - lambda_dssim) * l1_loss(gtm, image) + lambda_dssim * (1.0 - ssim(gtm, image))
    a = alpha.reshape(m.shape)
    return lambda_image * img + lambda_l1_alpha * l1_loss(m, a) + lambda_l2_alpha * l2_loss(m, a)


def label_bce_loss(render_label, obj_mask):
    """The label phase's loss (/root/reference/trainers/train_static.py:104-109): BCE-with-logits of the channel mean of the label render
    [3,H,W] against the object mask ([H,W] or [1,H,W]).  The reference's hand-mask hook (grad * (1 - hand_mask) on the mean) is the caller's;
    fused.label_bce_loss takes it as grad_gate.  The oracle of the HIP kernels behind fused.label_bce_loss, on any device and in any float type."""
    x = render_label.mean(0, keepdim=True)
    return torch.nn.functional.binary_cross_entropy_with_logits(x, obj_mask.to(x.dtype).reshape(x.shape))


def opacity_entropy(opacity, visibility):
    """The static stages' entropy regulariser, unweighted (/root/reference/trainers/train_static.py:97-102, trainers/train_static_bg.py:105-110,
    where it enters the loss with the factor 0.1): the mean over the visible Gaussians of the binary entropy of their activated opacity,
        -o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10),   o = opacity[visibility].
    opacity: get_opacity, [P,1] or [P]; visibility: the render's visibility_filter (bool[P]).  No visible Gaussian: NaN, as torch's mean() of
    an empty tensor.  The oracle of the HIP kernels behind fused.opacity_entropy and render(opacity_entropy=), on any device and in any float type."""
    vis = opacity[visibility]
    return (-vis * torch.log(vis + 1e-10) - (1 - vis) * torch.log(1 - vis + 1e-10)).mean()


def quantize8(x):
    """The 8-bit image a PNG of `x` holds: uint8(clamp(x * 255 + 0.5, 0, 255)), evaluated in float32 with truncation -- the conversion of
    torchvision.utils.save_image, which the reference's eval_and_metric writes its renders and ground truths with
    (the reference, trainers/eval_metric.py:41-175).  float32 whatever x's type is: the rule is defined there (on the 765 values around
    the boundaries (k + 0.5) / 255 it differs from exact round-half-up in 128).  Idempotent on k / 255; NaN -> 0.  Any device."""
    v = torch.nan_to_num(x.detach().to(torch.float32), nan=0.0, posinf=float("inf"), neginf=float("-inf"))
    return v.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def eval_metrics(image, gt, keep=None):
    """PSNR and SSIM of one frame as the reference's eval_and_metric reports them: on the 8-bit images, with the hand removed.
        u = kept ? quantize8(image) / 255 : 0,  v = kept ? quantize8(gt) / 255 : 0,  kept = keep >= 0.5  (keep = 1 - hand mask, [H,W]; None: all)
        sse = sum over kept pixels and channels of (quantize8(image) - quantize8(gt))^2      (an exact integer)
        psnr = 10 log10(255^2 * 3HW / sse): the mean counts gated pixels too, as the reference's does; inf when sse == 0
        ssim = mean over all 3HW entries of ssim()'s map of (u, v)
    The reference asserts its masks binary; a non-binary `keep` is outside the contract (it is thresholded here, multiplied there).
    image, gt: [C,H,W] in any float type on any device; the SSIM map is evaluated in that type.  -> dict(sse: int64 tensor, psnr, ssim: tensors of
    image's type).  The oracle of the HIP kernel behind fused.eval_metrics."""
    assert image.dim() == 3 and image.shape == gt.shape
    dt = image.dtype if image.dtype.is_floating_point else torch.float32
    qx, qy = quantize8(image).to(torch.int64), quantize8(gt).to(torch.int64)
    if keep is not None:
        kept = (keep.reshape(image.shape[-2], image.shape[-1]) >= 0.5).to(torch.int64)[None]
        qx, qy = qx * kept, qy * kept
    sse = ((qx - qy) ** 2).sum()
    n = image.numel()
    mse = sse.to(torch.float64) / (255.0 ** 2 * n)
    psnr_v = torch.where(sse == 0, torch.full_like(mse, float("inf")), -10.0 * torch.log10(mse.clamp_min(1e-300)))
    u, v = qx.to(dt) / 255, qy.to(dt) / 255
    return dict(sse=sse, psnr=psnr_v.to(dt), ssim=ssim(u, v))


def label_mask(render_label, threshold=0.5, target=None, keep=None):
    """The predicted object mask of one label render (the reference, trainers/train_static.py:187-188: mean over the channels, > 0.5, stored
    as an 8-bit image) and its counts against the dataset's mask:
        set = ((c0 + c1) + c2) / 3 > threshold      the channel mean in float32, added in this order; strict, so NaN is not set
        mask = set ? 255 : 0                        uint8 [H,W], every pixel: the stored mask ignores `keep`, as the reference's PNG does
        kept = keep >= 0.5 (None: every pixel);  predicted = #(kept & set), target = #(kept & target >= 0.5), intersection, kept = #kept
    render_label: [3,H,W]; target, keep: [H,W] or [1,H,W].  -> dict(mask: uint8[H,W]; predicted, target, intersection, kept: int64 tensors).
    The oracle of the HIP kernel behind fused.label_mask, on any device."""
    assert render_label.dim() == 3 and render_label.shape[0] == 3
    x = render_label.detach().to(torch.float32)
    H, W = x.shape[-2], x.shape[-1]
    mean = ((x[0] + x[1]) + x[2]) / 3
    on = mean > threshold
    kept = torch.ones_like(on) if keep is None else keep.reshape(H, W).to(torch.float32) >= 0.5
    tgt = torch.zeros_like(on) if target is None else target.reshape(H, W).to(torch.float32) >= 0.5
    count = lambda m: m.sum(dtype=torch.int64)
    return dict(mask=on.to(torch.uint8) * 255, predicted=count(kept & on), target=count(kept & tgt), intersection=count(kept & on & tgt), kept=count(kept))


def interaction_gate(hand_mask, obj_mask=None, dilate_size=None):
    """The gate of the background stage's image gradient (the reference, trainers/train_static_bg.py:14-21, 81-99):
        1 - dilate_k(hand_mask | obj_mask),   float32 [H,W]
    a pixel is set when either mask is non-zero there (torch.logical_or); it is gated (0) when any pixel of the k x k window around it, clipped
    to the image, is set -- a max-pool of the set indicator with stride 1 and padding k // 2 (padded entries never win).  k = dilate_size, odd;
    None: no dilation.  The oracle of the HIP kernel behind fused.interaction_gate, on any device."""
    a = hand_mask.detach()
    H, W = a.shape[-2], a.shape[-1]
    on = a.reshape(H, W) != 0
    if obj_mask is not None:
        on = torch.logical_or(on, obj_mask.detach().reshape(H, W) != 0)
    k = 1 if dilate_size is None else int(dilate_size)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"interaction_gate: dilate_size must be odd and positive, got {dilate_size}")
    on = on.to(torch.float32)
    if k > 1:
        on = torch.nn.functional.max_pool2d(on[None, None], kernel_size=k, stride=1, padding=k // 2)[0, 0]
    return 1.0 - on
