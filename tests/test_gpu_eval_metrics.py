"""GPU: the metric kernel (csrc/eval_metrics.hip through fused.eval_metrics) against the definition (tests/eval_anchor.py) on the loss
kernel's ladder of shapes -- below the window, one strip, at / one under / one over one and two strips of 54 x 15."""
import functools

import numpy as np
import pytest
import torch

from tests import eval_anchor as EA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _case(shape, masked):
    """Inputs and the float64 reference of one shape, computed once and shared (read-only)."""
    x, y, keep = EA.inputs(*shape)
    keep = keep if masked else None
    return x, y, keep, EA.reference64(x.numpy(), y.numpy(), None if keep is None else keep.numpy())


def _run(x, y, keep, out8=False, rows=None, cursor=None, overflow=None):
    from egogaussian_amd import fused
    from egogaussian_amd.evaluate import decode_rows
    r = fused.eval_metrics(x.to(DEV), y.to(DEV), None if keep is None else keep.to(DEV), rows=rows, cursor=cursor, overflow=overflow, out8=out8)
    torch.cuda.synchronize()
    return r, decode_rows(r["rows"], x.numel())


@pytest.mark.parametrize("out8", (False, True), ids=("no_bytes", "bytes"))
@pytest.mark.parametrize("masked", (True, False), ids=("keep", "all_kept"))
@pytest.mark.parametrize("shape", EA.SHAPES, ids=IDS)
def test_kernel_against_the_definition(shape, masked, out8):
    x, y, keep, ref = _case(shape, masked)
    r, fig = _run(x, y, keep, out8)
    d = abs(float(fig["ssim"][0]) - ref["ssim"])
    print(f"{shape} keep={masked} out8={out8}: sse {int(fig['sse'][0])} ({ref['sse']}), |ssim - ssim64| {d:.2e} (bar {EA.SSIM_BAR:g}), psnr {fig['psnr'][0]:.5f} ({ref['psnr']:.5f})")
    EA.check(fig["sse"][0], fig["ssim"][0], ref, what=f"{shape}")
    assert abs(float(fig["psnr"][0]) - ref["psnr"]) <= 1e-9 and int(r["cursor"].item()) == 1
    assert not fig["clipped"][0] and int(fig["instances"][0]) == 0
    if out8:
        assert r["q_image"].dtype == torch.uint8 and tuple(r["q_image"].shape) == tuple(x.shape)
        assert np.array_equal(r["q_image"].cpu().numpy(), ref["qx"]) and np.array_equal(r["q_gt"].cpu().numpy(), ref["qy"])
    else:
        assert r["q_image"] is None and r["q_gt"] is None


def test_quantised_bytes_on_the_boundary_values():
    """Every k / 255, the 765 values around the boundaries, values outside [0, 1] and NaN: the bytes are losses.quantize8's."""
    from egogaussian_amd.losses import quantize8
    x, y = EA.boundary_frame()
    x[0, 0, 0] = float("nan")
    r, fig = _run(x, y, None, out8=True)
    assert torch.equal(r["q_image"].cpu(), quantize8(x)) and torch.equal(r["q_gt"].cpu(), quantize8(y))
    xq = torch.nan_to_num(x, nan=0.0)
    ref = EA.reference64(xq.numpy(), y.numpy(), None)
    EA.check(fig["sse"][0], fig["ssim"][0], ref, what="boundary frame")


def test_all_gated_and_identical_frames():
    x, y, keep, _ = _case((3, 29, 107), True)
    _, fig = _run(x, y, torch.zeros_like(keep))
    assert int(fig["sse"][0]) == 0 and fig["psnr"][0] == np.inf and abs(float(fig["ssim"][0]) - 1.0) <= EA.SSIM_BAR
    _, fig = _run(x, x.clone(), keep)
    assert int(fig["sse"][0]) == 0 and fig["psnr"][0] == np.inf and abs(float(fig["ssim"][0]) - 1.0) <= EA.SSIM_BAR


def test_rows_are_bit_identical_run_to_run_and_single_channel_masks_broadcast():
    x, y, keep, _ = _case((3, 29, 107), True)
    a, _ = _run(x, y, keep, out8=True)
    b, _ = _run(x, y, keep, out8=True)
    assert torch.equal(a["rows"], b["rows"]) and torch.equal(a["q_image"], b["q_image"])
    # a [1,H,W] keep is the same mask
    c, _ = _run(x, y, keep[None])
    assert torch.equal(a["rows"], c["rows"])


def test_cursor_rows_overflow_word_and_a_full_array():
    """The cursor advances by one per call; rows land where it points, carrying the overflow words; a full array is left untouched while the
    cursor still counts."""
    from egogaussian_amd import fused
    from egogaussian_amd.evaluate import decode_rows
    shapes = [(3, 16, 55), (3, 16, 55), (3, 16, 55)]
    rows, cursor = fused.eval_rows(2, DEV)
    word = torch.tensor([1, 12345], dtype=torch.int32, device=DEV)
    cases = [_case(s, m) for s, m in zip(shapes, (True, False, True))]
    _run(*cases[0][:3], rows=rows, cursor=cursor)
    assert int(cursor.item()) == 1 and torch.equal(rows[1], torch.zeros(4, dtype=torch.int64, device=DEV))
    _run(*cases[1][:3], rows=rows, cursor=cursor, overflow=word)
    assert int(cursor.item()) == 2
    full = rows.clone()
    fig = decode_rows(rows, 3 * 16 * 55)
    for k in (0, 1):
        EA.check(fig["sse"][k], fig["ssim"][k], cases[k][3], what=f"row {k}")
    assert list(fig["clipped"]) == [False, True] and list(fig["instances"]) == [0, 12345]
    _run(*cases[2][:3], rows=rows, cursor=cursor, overflow=word)          # the array is full
    assert int(cursor.item()) == 3 and torch.equal(rows, full)
    with pytest.raises(RuntimeError):
        fused.eval_metrics(cases[0][0].to(DEV), cases[0][1].to(DEV), rows=rows)      # rows without a cursor


def test_shape_errors_are_raised():
    from egogaussian_amd import fused
    with pytest.raises(RuntimeError):
        fused.eval_metrics(torch.zeros(2, 8, 8, device=DEV), torch.zeros(2, 8, 8, device=DEV))
    with pytest.raises(RuntimeError):
        fused.eval_metrics(torch.zeros(3, 8, 8, device=DEV), torch.zeros(3, 8, 8, device=DEV), keep=torch.zeros(4, 4, device=DEV))
