"""CPU: the torch statement of the evaluation figures (losses.quantize8, losses.eval_metrics) against a real PNG round trip, against the
definition in numpy float64 (tests/eval_anchor.py), against deliberately wrong variants, and as the float32 yardstick of the SSIM bar."""
import io

import numpy as np
import pytest
import torch

from tests import eval_anchor as EA


def test_quantize8_is_the_float32_rule_and_survives_a_png_round_trip():
    """The bytes are those of the float32 expression v * 255 + 0.5, clamped, truncated (NOT exact round-half-up: 128 of the 765 boundary
    values say so); a PNG written from them by PIL and reopened holds the same bytes, and its / 255 values quantise to themselves."""
    from PIL import Image
    from egogaussian_amd.losses import quantize8
    v = EA.boundary_values()
    q = quantize8(torch.from_numpy(v))
    assert q.dtype == torch.uint8
    expect = torch.from_numpy(v).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()          # the statement itself, float32
    assert np.array_equal(q.numpy(), expect) and np.array_equal(EA.quantize_numpy(v), expect)
    # the 256 exact values survive; values outside [0, 1] clamp
    assert np.array_equal(q.numpy()[:256], np.arange(256, dtype=np.uint8))
    assert np.array_equal(quantize8(torch.tensor([-1.0, -1e-3, 1.0 + 1e-3, 2.0, float("nan"), float("inf"), -float("inf")])).numpy(),
                          np.array([0, 0, 255, 255, 0, 255, 0], dtype=np.uint8))
    # the boundary set: where the float32 rule and exact round-half-up part
    b = v[256:256 + 765]
    exact_half_up = np.clip(np.floor(b.astype(np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)      # (exact in float64: 24 + 8 bits)
    differ = int((expect[256:256 + 765] != exact_half_up).sum())
    print(f"float32 rule vs exact round-half-up on the boundary set: {differ} of 765 differ")
    assert differ == 128
    # a real PNG: write, reopen, / 255
    img = q.numpy()[:1280].reshape(16, 80)
    buf = io.BytesIO()
    Image.fromarray(img, mode="L").save(buf, format="PNG")
    back = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    again = quantize8(torch.from_numpy(back.astype(np.float32)) / 255)
    assert np.array_equal(again.numpy(), img), "q is not idempotent on k / 255"
    # any float type, same bytes (the rule is evaluated in float32)
    assert torch.equal(quantize8(torch.from_numpy(v).double()), q)


@pytest.mark.parametrize("shape", EA.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_metrics_against_the_definition_and_float32_yardstick(shape):
    """losses.eval_metrics in float64 IS the definition (sse equal, ssim to rounding); in float32 it stays under HALF of the SSIM bar."""
    from egogaussian_amd.losses import eval_metrics
    x, y, keep = EA.inputs(*shape)
    for k in (keep, None):
        ref = EA.reference64(x.numpy(), y.numpy(), None if k is None else k.numpy())
        r64 = eval_metrics(x.double(), y.double(), k)
        assert r64["sse"].dtype == torch.int64
        d64 = EA.check(r64["sse"], r64["ssim"], ref, frac=1e-6, what=f"float64 {shape}")
        assert abs(float(r64["psnr"]) - ref["psnr"]) <= 1e-9
        r32 = eval_metrics(x, y, k)
        d32 = EA.check(r32["sse"], r32["ssim"], ref, frac=0.5, what=f"float32 {shape}")
        assert abs(float(r32["psnr"]) - ref["psnr"]) <= 1e-4          # float32 result type: 10 log10 around 20 dB resolves 2e-6
        print(f"{shape} keep={'yes' if k is not None else 'no'}: sse {ref['sse']}, psnr {ref['psnr']:.4f}, ssim64 {ref['ssim']:.9f}, "
              f"|float64 - def| {d64:.1e}, |float32 - def| {d32:.1e} (bar {EA.SSIM_BAR:g})")


def test_special_frames():
    from egogaussian_amd.losses import eval_metrics
    x, y, keep = EA.inputs(3, 29, 107)
    r = eval_metrics(x, x.clone(), keep)
    assert int(r["sse"]) == 0 and float(r["psnr"]) == float("inf") and abs(float(r["ssim"]) - 1.0) <= EA.SSIM_BAR
    r = eval_metrics(x, y, torch.zeros_like(keep))                     # every pixel gated: both images are black
    assert int(r["sse"]) == 0 and float(r["psnr"]) == float("inf") and abs(float(r["ssim"]) - 1.0) <= EA.SSIM_BAR
    ref = EA.reference64(x.numpy(), y.numpy(), np.zeros(keep.shape, np.float32))
    assert ref["sse"] == 0 and ref["ssim"] == 1.0


@pytest.mark.parametrize("fault", EA.FAULTS)
def test_wrong_variants_are_told_apart(fault):
    """Each deliberately wrong variant of the definition misses the right one's figures by far more than the bars, on the test inputs
    (the boundary frame for the rounding rule: random images hold no ties)."""
    if fault == "round_even":
        x, y = EA.boundary_frame()
        x, y, keep = x.numpy(), y.numpy(), None
    else:
        x, y, keep = (t.numpy() for t in EA.inputs(3, 29, 107))
    good, bad = EA.reference64(x, y, keep), EA.reference64(x, y, keep, fault=fault)
    from egogaussian_amd.losses import eval_metrics
    got = eval_metrics(torch.from_numpy(x), torch.from_numpy(y), None if keep is None else torch.from_numpy(keep))
    EA.check(got["sse"], got["ssim"], good, frac=0.5, what="the right one")
    d_psnr = abs(bad["psnr"] - good["psnr"])
    print(f"{fault}: sse {bad['sse']} vs {good['sse']}, psnr {bad['psnr']:.4f} vs {good['psnr']:.4f}, ssim {bad['ssim']:.7f} vs {good['ssim']:.7f}")
    if fault == "round_even":
        assert not np.array_equal(bad["qx"], good["qx"]) and bad["sse"] != good["sse"]
    elif fault == "mse_over_kept":
        assert bad["sse"] == good["sse"] and d_psnr > 1.0              # ~30 % gated: 10 log10(1 / 0.7) = 1.5 dB
    elif fault == "ssim_unmasked":
        assert abs(bad["ssim"] - good["ssim"]) > 100 * EA.SSIM_BAR
    else:
        assert bad["sse"] != good["sse"] and abs(bad["ssim"] - good["ssim"]) > 100 * EA.SSIM_BAR
    if fault == "mse_over_kept":                                       # sse and ssim are the right ones; the PSNR is off by more than the project's 0.05 dB
        assert abs(float(got["psnr"]) - good["psnr"]) <= 1e-4 < 0.05 < abs(float(got["psnr"]) - bad["psnr"])
    else:
        with pytest.raises(AssertionError):
            EA.check(got["sse"], got["ssim"], bad, what="the wrong one")


def test_fused_route_refuses_cpu_tensors():
    from egogaussian_amd import fused
    x, y, keep = EA.inputs(1, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.eval_metrics(x, y, keep)


def test_c_abi_argument_errors_precede_device_work():
    from egogaussian_amd import lib
    L = lib.load()
    p = 4096                                                           # (fake non-null pointers are never dereferenced before the checks)
    assert L.egs_eval_metrics(2, 8, 8, p, p, None, None, p, None, None, p, 1, p, None) == -1       # channels not in {1, 3}
    assert L.egs_eval_metrics(3, 0, 8, p, p, None, None, p, None, None, p, 1, p, None) == -1
    assert L.egs_eval_metrics(3, 8, 0, p, p, None, None, p, None, None, p, 1, p, None) == -1
    assert L.egs_eval_metrics(3, 8, 8, None, p, None, None, p, None, None, p, 1, p, None) == -1
    assert L.egs_eval_metrics(3, 8, 8, p, p, None, None, p, None, None, p, 1, None, None) == -1    # no cursor
    assert L.egs_eval_metrics(1, 65536, 32768, p, p, None, None, p, None, None, p, 1, p, None) == -3
    assert L.egs_eval_metrics_partial_bytes(3, 31, 109) == 3 * 3 * 3 * 8 and L.egs_eval_metrics_partial_bytes(3, 0, 5) == 0
