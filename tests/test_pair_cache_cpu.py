"""CPU: the one-evaluation-for-two-calls protocol of patching.make_loss_functions (the trainers call l1_loss(x, gt) and then ssim(x, gt) on
the same pair; the first call evaluates fused.l1_and_ssim once and keeps the other half for the call that follows).  fused.l1_and_ssim is
replaced by a counting mirror on losses.l1_loss / losses.ssim and the HIP-image predicate by itself minus is_cuda, so what is tested is
when a kept half may be handed out -- never to another image, another ground truth, an edited tensor or another grad mode -- not the kernel
(tests/test_gpu_pair_loss.py)."""
import pytest
import torch

from egogaussian_amd import fused, losses, patching

SHAPE = (3, 12, 14)


@pytest.fixture
def pair(monkeypatch):
    """-> (l1, ssim, evals): the replacement functions over the mirror; evals lists what each evaluation returned."""
    evals = []

    def l1_and_ssim(a, b, raster_prologue=True):
        evals.append((losses.l1_loss(a, b), losses.ssim(a, b)))
        return evals[-1]

    monkeypatch.setattr(fused, "l1_and_ssim", l1_and_ssim)
    monkeypatch.setattr(patching, "_hip_image_pair", lambda a, b: (torch.is_tensor(a) and torch.is_tensor(b) and a.dim() == 3 and a.shape == b.shape
                                                                   and a.dtype == torch.float32 and b.dtype == torch.float32))
    l1, ss = patching.make_loss_functions(losses.l1_loss, losses.ssim)      # (the originals given, as install() gives the reference's)
    return l1, ss, evals


def _images(n=2, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(*SHAPE, generator=gen) for _ in range(n)]


def _same(v, ref):
    return torch.equal(v.detach(), ref.detach())


def test_l1_then_ssim_is_one_evaluation(pair):
    l1, ss, evals = pair
    a, b = _images()
    a.requires_grad_(True)
    v1, v2 = l1(a, b), ss(a, b)
    assert len(evals) == 1 and v1 is evals[0][0] and v2 is evals[0][1]
    assert _same(v1, losses.l1_loss(a, b)) and _same(v2, losses.ssim(a, b))
    v3 = ss(a, b)                                                     # the kept half is handed out once
    assert len(evals) == 2 and _same(v3, v2)


def test_ssim_then_l1_is_one_evaluation(pair):
    l1, ss, evals = pair
    a, b = _images()
    a.requires_grad_(True)
    v2, v1 = ss(a, b), l1(a, b)
    assert len(evals) == 1 and v1 is evals[0][0] and v2 is evals[0][1]
    assert _same(v1, losses.l1_loss(a, b)) and _same(v2, losses.ssim(a, b))


def test_another_ground_truth_is_evaluated_anew(pair):
    l1, ss, evals = pair
    a, b, c = _images(3)
    v1, v2 = l1(a, b), ss(a, c)
    assert len(evals) == 2
    assert _same(v1, losses.l1_loss(a, b)) and _same(v2, losses.ssim(a, c)) and not _same(v2, losses.ssim(a, b))


def test_another_image_is_evaluated_anew(pair):
    l1, ss, evals = pair
    a, b, c = _images(3)
    v1, v2 = l1(a, b), ss(c, b)
    assert len(evals) == 2 and _same(v2, losses.ssim(c, b)) and not _same(v2, losses.ssim(a, b))


def test_an_image_edited_in_place_is_evaluated_anew(pair):
    l1, ss, evals = pair
    leaf, b = _images()
    leaf.requires_grad_(True)
    a = leaf * 1.0                                                    # a non-leaf, as a render is
    v1 = l1(a, b)
    before = losses.ssim(a.detach().clone(), b)
    a.mul_(0.5)
    v2 = ss(a, b)
    assert len(evals) == 2
    assert _same(v2, losses.ssim(a.detach(), b)) and not _same(v2, before)


def test_a_ground_truth_edited_in_place_is_evaluated_anew(pair):
    l1, ss, evals = pair
    a, b, c = _images(3)
    l1(a, b)
    before = losses.ssim(a, b.clone())
    b.copy_(c)
    v2 = ss(a, b)
    assert len(evals) == 2
    assert _same(v2, losses.ssim(a, c)) and not _same(v2, before)


def test_the_second_of_two_l1_calls_is_the_one_ssim_pairs_with(pair):
    l1, ss, evals = pair
    a, b = _images()
    a.requires_grad_(True)
    l1(a, b)
    v1 = l1(a, b)
    v2 = ss(a, b)
    assert len(evals) == 2 and v1 is evals[1][0] and v2 is evals[1][1]


def test_a_half_kept_under_no_grad_is_not_handed_to_a_call_that_records(pair):
    """l1_loss(x, gt) under torch.no_grad() (logging, an evaluation pass) followed by ssim(x, gt) of a training iteration on the same tensors:
    a half without a grad_fn would drop the SSIM term from loss.backward() without a word."""
    l1, ss, evals = pair
    a, b = _images()
    a.requires_grad_(True)
    with torch.no_grad():
        v1 = l1(a, b)
    assert v1.grad_fn is None
    v2 = ss(a, b)
    assert v2.grad_fn is not None and len(evals) == 2
    v2.backward()
    a2 = a.detach().clone().requires_grad_(True)
    losses.ssim(a2, b).backward()
    assert torch.equal(a.grad, a2.grad) and float(a.grad.abs().max()) > 0
    # the other way round nothing is lost, whichever half is taken
    a.grad = None
    v1 = l1(a, b)
    with torch.no_grad():
        v2 = ss(a, b)
    assert _same(v2, losses.ssim(a, b))
    v1.backward()
    assert float(a.grad.abs().max()) > 0


def test_calls_the_kernel_does_not_cover_step_aside_and_leave_the_kept_half(pair):
    l1, ss, evals = pair
    a, b = _images()
    a.requires_grad_(True)
    n0 = dict(patching.calls)
    v1 = l1(a, b)
    per_image = ss(a, b, size_average=False)
    other_window = ss(a, b, 7)
    assert len(evals) == 1 and patching.calls["ssim_fallback"] == n0["ssim_fallback"] + 2 and patching.calls["ssim"] == n0["ssim"]
    assert _same(per_image, losses.ssim(a, b, 11, False)) and _same(other_window, losses.ssim(a, b, 7))
    assert not _same(other_window, losses.ssim(a, b))
    v2 = ss(a, b)                                                     # still the half of the first call
    assert len(evals) == 1 and v2 is evals[0][1] and v1 is evals[0][0]
    # a batched image is not covered either
    assert _same(l1(a[None], b[None]), losses.l1_loss(a, b)) and len(evals) == 1


def test_default_originals_take_the_window_and_the_averaging_flag():
    """make_loss_functions() without originals falls back to losses.py: what steps aside keeps its arguments."""
    l1, ss = patching.make_loss_functions()
    a, b = _images()
    assert _same(ss(a, b, size_average=False), losses.ssim(a, b, 11, False)) and ss(a, b, size_average=False).shape == (1,)
    assert _same(ss(a, b, 7), losses.ssim(a, b, 7)) and not _same(ss(a, b, 7), losses.ssim(a, b))
    assert _same(ss(a, b), losses.ssim(a, b)) and _same(l1(a, b), losses.l1_loss(a, b))
