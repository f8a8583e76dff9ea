"""The evaluation figures' float64 anchor (include/egs_raster.h egs_eval_metrics; losses.eval_metrics; fused.eval_metrics): input builders,
the definition written out in numpy, deliberately wrong variants, and the checks the CPU and GPU tests share.

Definition, per frame (x, y float32[C,H,W]; keep float32[H,W] or None):
    q(v)  = uint8(clamp(v * 255 + 0.5, 0, 255))     evaluated in FLOAT32, one rounding per operation, truncating -- part of the definition:
                                                    on the 765 values around the boundaries (k + 0.5) / 255 it differs from exact
                                                    round-half-up in 128 (tests/test_eval_cpu.py)
    kept  = keep >= 0.5
    sse   = sum over kept pixels and channels of (q(x) - q(y))^2                         an exact integer: compared with ==
    psnr  = 10 log10(255^2 C H W / sse)                                                  the divisor counts gated pixels; inf for sse = 0
    ssim  = mean over all C H W entries of the SSIM map of (kept ? q(x) / 255 : 0, kept ? q(y) / 255 : 0)     everything from q on in float64

SSIM bar: |ssim - ssim64| <= 2e-6 = anchors.LOSS_VALUE_BAR.  With lambda = 1 the image loss's value is 1 - SSIM, and that bar is the one
the loss kernel's value is held to against float64 on the same strips, window and arithmetic; it transfers unchanged.  The float32 torch
statement has to stay under HALF of it (the yardstick, tests/test_eval_cpu.py)."""
import numpy as np
import torch

from tests import anchors

SSIM_BAR = anchors.LOSS_VALUE_BAR
SHAPES = anchors.LOSS_SHAPES                # the loss kernel's ladder around its 54 x 15 strip: the metric kernel walks the same strips
FAULTS = ("round_even", "mse_over_kept", "ssim_unmasked", "mask_one_image")


def inputs(C, H, W, seed=0):
    """anchors.loss_inputs stretched to [-0.1, 1.1] (both clamps of the quantiser are exercised), the gate as `keep` (binary, ~30 % gated)."""
    img, gt, gate = anchors.loss_inputs(C, H, W, seed)
    return (img * 1.2 - 0.1).float(), (gt * 1.2 - 0.1).float(), (gate >= 0.5).float()


def boundary_values():
    """float32[1280]: every k / 255; the 255 boundaries float32((k + 0.5) / 255) each with its two float32 neighbours; values below 0 and above 1."""
    f = np.float32
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(f)
    b = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(f)
    outside = np.array([-1e30, -3.0, -1.0, -1e-3, -1e-8, -0.0, 1.0 + 1e-3, 1.0019, 1.002, 1.5, 2.0, 255.0, 1e30], dtype=f)
    v = np.concatenate([exact, np.nextafter(b, f(-1)), b, np.nextafter(b, f(2)), outside]).astype(f)
    return np.concatenate([v, np.zeros(1280 - v.size, dtype=f)])


def boundary_frame(C=3, H=16, W=80):
    """The boundary values as an image pair [C,H,W] (x ascending, y the same values reversed): every one of them passes through the kernel's
    quantiser in both images."""
    v = boundary_values()
    n = C * H * W
    x = np.resize(v, n).reshape(C, H, W)
    y = np.resize(v[::-1], n).reshape(C, H, W)
    return torch.from_numpy(x.copy()), torch.from_numpy(y.copy())


def quantize_numpy(v, fault=None):
    """q(v) in numpy float32, operation by operation.  fault 'round_even': round-to-nearest-even of the exact product instead."""
    f = np.float32
    v = np.nan_to_num(np.asarray(v, dtype=f), nan=0.0, posinf=np.inf, neginf=-np.inf)
    if fault == "round_even":
        return np.clip(np.rint(v.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    t = (v * f(255.0)).astype(f)
    t = (t + f(0.5)).astype(f)
    return np.clip(t, f(0), f(255)).astype(np.uint8)


def ssim_map64(u, v):
    B = anchors.blur11
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = B(u), B(v)
    s1, s2, s12 = B(u * u) - mu1 * mu1, B(v * v) - mu2 * mu2, B(u * v) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def reference64(x, y, keep=None, fault=None):
    """The definition in numpy float64 -> dict(sse: int, psnr, ssim, ssim_sum: float, qx, qy: uint8 arrays).  fault: one of FAULTS."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    qx, qy = quantize_numpy(x, fault), quantize_numpy(y, fault)
    kept = np.ones(x.shape[1:], bool) if keep is None else (np.asarray(keep, np.float32).reshape(x.shape[1:]) >= 0.5)
    kx = kept if fault != "mask_one_image" else np.ones_like(kept)
    ix, iy = qx.astype(np.int64) * kx[None], qy.astype(np.int64) * kept[None]
    sse = int(((ix - iy) ** 2).sum())
    n = x.size if fault != "mse_over_kept" else max(int(kept.sum()) * x.shape[0], 1)
    psnr = float("inf") if sse == 0 else float(10.0 * np.log10(255.0 ** 2 * n / sse))
    if fault == "ssim_unmasked":
        u, v = qx.astype(np.float64) / 255.0, qy.astype(np.float64) / 255.0
    else:
        u, v = ix.astype(np.float64) / 255.0, iy.astype(np.float64) / 255.0
    m = ssim_map64(u, v)
    return dict(sse=sse, psnr=psnr, ssim=float(m.mean()), ssim_sum=float(m.sum()), qx=qx, qy=qy)


def check(sse, ssim, ref, frac=1.0, what=""):
    """sse EQUAL to the integer; |ssim - ssim64| <= frac * SSIM_BAR.  -> the SSIM distance."""
    assert int(sse) == ref["sse"], f"{what}: sse {int(sse)} != {ref['sse']}"
    d = abs(float(ssim) - ref["ssim"])
    assert d <= frac * SSIM_BAR, f"{what}: ssim {float(ssim)!r} is {d:.3e} from float64 {ref['ssim']!r} (bar {frac * SSIM_BAR:g})"
    return d


def psnr_of(sse, n):
    return float("inf") if int(sse) == 0 else float(10.0 * np.log10(255.0 ** 2 * n / int(sse)))
