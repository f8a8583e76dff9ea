"""GPU: the image loss (loss.hip) against losses.training_loss evaluated in float64 on the CPU, with the same in float32 on the CPU as the
yardstick -- the launches that the loss gradient formed in the blend and the object-stage loss without alpha weights are each asserted
bit-identical to.  The shapes sit below the 11-tap window, at one strip (54 columns x 15 rows per wave), and at, one under and one over one
and two strips; lambda = 0.2 and 1, with and without a gradient gate.  Figures: profiles/anchor_parity.md."""
import pytest
import torch

from tests import anchors as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("C,H,W", A.LOSS_SHAPES)
def test_value_and_gradient_per_pixel_against_float64(C, H, W):
    from egogaussian_amd.fused import l1_ssim_loss
    img, gt, gate = A.loss_inputs(C, H, W)
    for lam in A.LOSS_LAMBDAS:
        for g8 in (None, gate):
            x = img.to(DEV).requires_grad_(True)
            l = l1_ssim_loss(x, gt.to(DEV), lam, grad_gate=None if g8 is None else g8.to(DEV))
            l.backward()
            ref64, ref32 = A.loss_reference(img, gt, lam, g8, torch.float64), A.loss_reference(img, gt, lam, g8, torch.float32)
            what = f"{(C, H, W)} lambda {lam} gate {g8 is not None}"
            value, grad = float(l.detach().cpu()), x.grad.cpu().numpy()
            e = abs(value - ref64[0])
            print(f"ANCHOR loss {what}: value {e:.1e} (torch float32 {abs(ref32[0] - ref64[0]):.1e})")
            fig = A.check_loss(value, grad, ref64, ref32, None if g8 is None else g8.numpy(), what=what)
            print(f"ANCHOR loss {what}: gradient max {fig['max'][0]:.2e} ({fig['max'][1]:.2e}), q99 {fig['q99'][0]:.2e} ({fig['q99'][1]:.2e}), "
                  f"strip seams {fig['seam'][0]:.2e} ({fig['seam'][1]:.2e}), border {fig['border'][0]:.2e} ({fig['border'][1]:.2e}), "
                  f"elsewhere {fig['interior'][0]:.2e} ({fig['interior'][1]:.2e})")
