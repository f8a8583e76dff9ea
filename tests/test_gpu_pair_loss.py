"""GPU: the two-value image loss -- fused.l1_and_ssim, what the reference's l1_loss(x, gt) and ssim(x, gt) become after install() -- against
losses.l1_loss / losses.ssim in float64 on the CPU, with the same in float32 on the CPU as the yardstick (tests/anchors.py, "two-value
loss").  It shares its forward with l1_ssim_loss; its own are k_l1_ssim_finish_pair, the upstream scalar of each term read on the device
(the kernel's (1 - SSIM) term carrying the weight -1), the gate argument of the C entry point, and the backward launch that carries the
rasterizer's backward prologue -- what a trainer iteration runs.  Shapes as tests/test_gpu_anchor_loss.py, with a block of exact ties.
Figures: profiles/anchor_parity.md."""
import functools

import numpy as np
import pytest
import torch

from tests import anchors as A
from tests.test_gpu_fused_adam import LEAVES, _groups, _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAINER_U = A.PAIR_UPSTREAMS[0]            # (0.8, -0.2): (1 - lambda) l1 + lambda (1 - ssim) at lambda = 0.2


@functools.lru_cache(maxsize=None)
def _refs(shape, u, gated=False):
    img, gt, gate = A.pair_inputs(*shape)
    g = gate if gated else None
    return A.pair_reference(img, gt, u, torch.float64, g), A.pair_reference(img, gt, u, torch.float32, g)


def _pair_on_device(shape, u=None, half=None):
    """u: (u0 l1 + u1 ssim).backward(); half: 'l1' | 'ssim' -- that value's backward() alone.  -> (l1, ssim, gradient) as numpy float32."""
    from egogaussian_amd.fused import l1_and_ssim
    img, gt, _ = A.pair_inputs(*shape)
    x = img.to(DEV).requires_grad_(True)
    l1v, ssv = l1_and_ssim(x, gt.to(DEV), raster_prologue=False)
    ({"l1": l1v, "ssim": ssv}[half] if half else u[0] * l1v + u[1] * ssv).backward()
    return l1v.detach().cpu().numpy(), ssv.detach().cpu().numpy(), x.grad.cpu().numpy()


@pytest.mark.parametrize("C,H,W", A.LOSS_SHAPES)
def test_values_and_gradient_per_pixel_against_float64(C, H, W):
    """Each upstream pair reaches the kernel as two device scalars that autograd produced."""
    for u in A.PAIR_UPSTREAMS:
        l1v, ssv, grad = _pair_on_device((C, H, W), u)
        ref64, ref32 = _refs((C, H, W), u)
        what = f"{(C, H, W)} u {u}"
        print(f"ANCHOR pair {what}: l1 {abs(float(l1v) - ref64[0]):.1e} (torch float32 {abs(ref32[0] - ref64[0]):.1e}), "
              f"ssim {abs(float(ssv) - ref64[1]):.1e} ({abs(ref32[1] - ref64[1]):.1e})")
        fig = A.check_pair((float(l1v), float(ssv)), grad, ref64, ref32, u, what=what)
        if u[1] != 0:
            print(f"ANCHOR pair {what}: gradient max {fig['max'][0]:.2e} ({fig['max'][1]:.2e}), q99 {fig['q99'][0]:.2e} ({fig['q99'][1]:.2e}), "
                  f"strip seams {fig['seam'][0]:.2e} ({fig['seam'][1]:.2e}), border {fig['border'][0]:.2e} ({fig['border'][1]:.2e}), "
                  f"elsewhere {fig['interior'][0]:.2e} ({fig['interior'][1]:.2e}), ties {fig['tie'][0]:.2e} ({fig['tie'][1]:.2e})")
        else:
            print(f"ANCHOR pair {what}: gradient u0 sign / n within {fig['l1_only'][0] / A.U:.2f} u of each element ({fig['l1_only'][1] / A.U:.2f} u), ties exactly zero")


@pytest.mark.parametrize("C,H,W", A.LOSS_SHAPES)
def test_one_half_alone_is_the_pair_with_the_other_upstream_zero(C, H, W):
    """l1.backward() alone and ssim.backward() alone (autograd hands None for the unused value): bit for bit the (1, 0) and (0, 1) gradients."""
    for half, u in (("l1", (1.0, 0.0)), ("ssim", (0.0, 1.0))):
        alone, both = _pair_on_device((C, H, W), half=half), _pair_on_device((C, H, W), u)
        assert all(A.same_bits(a, b) for a, b in zip(alone, both)), (half, (C, H, W))
        assert np.abs(alone[2]).max() > 0


@pytest.mark.parametrize("C,H,W", A.LOSS_SHAPES)
def test_trainer_upstreams_agree_with_the_one_value_kernel(C, H, W):
    """u = (0.8, -0.2) is l1_ssim_loss at lambda = 0.2: the gradient passes that loss's own check against training_loss in float64, and the
    value assembled from the pair is within the value bar of the one-value kernel's."""
    from egogaussian_amd.fused import l1_ssim_loss
    img, gt, _ = A.pair_inputs(C, H, W)
    l1v, ssv, grad = _pair_on_device((C, H, W), TRAINER_U)
    value = 0.8 * float(l1v) + 0.2 * (1.0 - float(ssv))
    ref64, ref32 = A.loss_reference(img, gt, 0.2, None, torch.float64), A.loss_reference(img, gt, 0.2, None, torch.float32)
    A.check_loss(value, grad, ref64, ref32, what=f"{(C, H, W)} pair at (0.8, -0.2) as l1_ssim_loss(0.2)")
    one = float(l1_ssim_loss(img.to(DEV), gt.to(DEV), 0.2))
    assert abs(value - one) <= A.LOSS_VALUE_BAR * max(1.0, abs(one)), (value, one)


def test_two_runs_give_identical_bits():
    a, b = _pair_on_device((3, 29, 107), TRAINER_U), _pair_on_device((3, 29, 107), TRAINER_U)
    assert all(A.same_bits(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("C,H,W", [(3, 16, 55), (1, 31, 109)])
def test_gate_of_the_c_entry_point(C, H, W):
    """egs_l1_ssim_pair_backward's gate (the Python wrapper never passes one): gated pixels exactly zero, every other bit-identical to the
    ungated call -- the gate is 0 / 1 and multiplied last --, and the gated gradient meets the float64 anchor."""
    from egogaussian_amd import _hip, lib
    L = lib.load()
    img, gt, gate = A.pair_inputs(C, H, W)
    x, y, g8 = img.to(DEV).contiguous(), gt.to(DEV).contiguous(), gate.to(DEV).contiguous()
    assert 0 < int((gate == 0).sum()) < H * W
    partial = torch.empty(L.egs_l1_ssim_partial_count(C, H, W), device=DEV)
    maps, vals = torch.empty((3, C, H, W), device=DEV), torch.empty(2, device=DEV)
    with _hip.device_ctx(x.device):
        s = _hip.stream_of(x.device)
        lib.check(L.egs_l1_ssim_pair_forward(C, H, W, x.data_ptr(), y.data_ptr(), partial.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(),
                                             maps[2].data_ptr(), vals[0:1].data_ptr(), vals[1:2].data_ptr(), s))
        for u in (TRAINER_U, (2.5, 0.0)):
            up = torch.tensor(u, device=DEV, dtype=torch.float32)
            out = []
            for g in (None, g8):
                dimg = torch.full_like(x, float("nan"))
                lib.check(L.egs_l1_ssim_pair_backward(C, H, W, x.data_ptr(), y.data_ptr(), up[0:1].data_ptr(), up[1:2].data_ptr(),
                                                      None if g is None else g.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(),
                                                      dimg.data_ptr(), None, s))
                out.append(dimg.cpu().numpy())
            plain, gated = out
            closed = np.broadcast_to(gate.numpy()[None] == 0, plain.shape)
            assert np.isfinite(plain).all() and np.isfinite(gated).all()
            assert not np.any(gated[closed] != 0), u
            assert A.same_bits(gated[~closed], plain[~closed]), u
            v = vals.cpu().numpy()
            ref64, ref32 = _refs((C, H, W), u, True)
            A.check_pair((float(v[0]), float(v[1])), gated, ref64, ref32, u, gate=gate.numpy(), what=f"{(C, H, W)} u {u} gated through the C ABI")
            ref64, ref32 = _refs((C, H, W), u)
            A.check_pair((float(v[0]), float(v[1])), plain, ref64, ref32, u, what=f"{(C, H, W)} u {u} through the C ABI")


# ---- the pair behind a render: the backward launch that carries the rasterizer's backward prologue ---------------------------------------
BAR = lambda a: 1e-5 * float(a.abs().max()) + 1e-9        # test_loss_backward_carrying_the_raster_prologue's: the order of the blend's float atomics


def _tiles_in_order(img_buf, H, W):
    """The tiles the tile-order words of a forward's image buffer name, sorted (as test_loss_backward_carrying_the_raster_prologue reads them)."""
    import ctypes
    from egogaussian_amd import _C
    lay = _C._lib.ImageLayout(); _C._lib.load().egs_get_image_layout(W, H, ctypes.byref(lay))
    words = img_buf[lay.tile_order:lay.tile_order + 4 * _C._lib.load().egs_order_words(W, H)].view(torch.int32).cpu().numpy().astype("uint32")
    return sorted(int(w & 0xffff) if (w & 0x01000000) else int(w) for w in words if w != 0xffffffff)


def _iteration(student, cam, gt, bg, loss_of, mask=None):
    """render -> loss_of(image, gt) -> backward.  A hook on the image sits between the two backwards: it records the gradient the loss
    handed over and whether the rasterizer's backward has been prepared by then (its node holds the scratch buffer the loss launch
    cleared: that backward then starts at its blend, rasterizer.backward_prologue_of), and applies the reference's hand mask when given.
    -> dict of gradients, 'prepared', 'tiles', 'values', 'nodes'."""
    from egogaussian_amd import _C
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import Pipe, SynthGaussians
    pc = SynthGaussians(student, device=DEV)
    out = render(cam, pc, Pipe, bg)
    img_buf, image = _C.stats["image_buffer"], out["render"]
    seen = {}

    def hook(g):
        seen["image"], seen["prepared"] = g.clone(), image.grad_fn.prologue_scratch is not None
        if mask is not None:
            seen["masked"] = g * (1 - mask)
            return seen["masked"]

    image.register_hook(hook)
    l1v, ssv = loss_of(image, gt)
    (0.8 * l1v + 0.2 * (1.0 - ssv)).backward()
    torch.cuda.synchronize()
    H, W = image.shape[1:]
    res = {a: getattr(pc, a).grad.clone() for a in LEAVES} | {"screen": out["viewspace_points"].grad.clone()} | seen
    return res | {"tiles": _tiles_in_order(img_buf, H, W), "values": (l1v.detach().clone(), ssv.detach().clone()), "nodes": (l1v.grad_fn, ssv.grad_fn)}


@functools.lru_cache(maxsize=None)
def _frame(H, W):
    return _scene(N=8000, H=H, W=W)


@pytest.mark.parametrize("H,W", [(96, 160), (70, 100)])
def test_pair_backward_carrying_the_raster_prologue(H, W):
    """What a trainer iteration runs after install(): l1_and_ssim on the rasterizer's output, whose backward launch also orders the tiles,
    clears the accumulator and does the optimizer's bookkeeping ((70, 100): tiles cut by both image edges).  Carried or not: the same image
    gradient bit for bit, every tile ordered exactly once, the same parameter gradients up to the order of the blend's float atomics --
    also with the reference's hand-mask hook between the two backwards, and with a fused optimizer taking its steps."""
    from egogaussian_amd.fused import l1_and_ssim
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import Pipe, SynthGaussians
    student, cams, gts, bg = _frame(H, W)
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    runs = {c: _iteration(student, cams[1], gts[1], bg, lambda x, y, c=c: l1_and_ssim(x, y, raster_prologue=c)) for c in (False, True)}
    assert runs[True]["prepared"] and not runs[False]["prepared"]
    assert runs[False]["tiles"] == runs[True]["tiles"] == list(range(nt))
    assert torch.equal(runs[False]["image"], runs[True]["image"]) and float(runs[True]["image"].abs().max()) > 0
    for k in LEAVES + ("screen",):
        a, b = runs[False][k], runs[True][k]
        assert float(a.abs().max()) > 0 and float((a - b).abs().max()) <= BAR(a), k
    # the hand mask of the reference's loop: grad * (1 - mask) between the two backwards
    mask = (torch.rand(1, H, W, generator=torch.Generator().manual_seed(5)) > 0.5).float().to(DEV)
    hooked = {c: _iteration(student, cams[1], gts[1], bg, lambda x, y, c=c: l1_and_ssim(x, y, raster_prologue=c), mask=mask) for c in (False, True)}
    assert hooked[True]["prepared"] and not hooked[False]["prepared"]
    assert hooked[False]["tiles"] == hooked[True]["tiles"] == list(range(nt))
    for c in (False, True):
        assert torch.equal(hooked[c]["image"], runs[False]["image"])
        assert torch.equal(hooked[c]["masked"], runs[False]["image"] * (1 - mask))
    for k in LEAVES + ("screen",):
        a, b = hooked[False][k], hooked[True][k]
        assert float(a.abs().max()) > 0 and float((a - b).abs().max()) <= BAR(a), k
    assert any(float((hooked[True][k] - runs[True][k]).abs().max()) > BAR(runs[True][k]) for k in LEAVES)      # (the mask did reach the rasterizer)
    # with a fused optimizer: its bookkeeping rides in the pair's backward launch; one step per iteration is counted and taken
    pc = SynthGaussians(student, device=DEV)
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    before = pc._xyz.detach().clone()
    for it in range(2):
        out = render(cams[it], pc, Pipe, bg, optimizer=opt)
        l1v, ssv = l1_and_ssim(out["render"], gts[it])
        (0.8 * l1v + 0.2 * (1.0 - ssv)).backward()
        opt.step()
    torch.cuda.synchronize()
    assert all(float(opt.state[getattr(pc, a)]["step"]) == 2.0 and getattr(pc, a).grad is None for a in LEAVES)
    assert not torch.equal(before, pc._xyz.detach())


def test_patched_loss_functions_on_a_render():
    """patching.make_loss_functions(): l1(img, gt) then ss(img, gt) on a rasterizer output are ONE autograd node, its backward launch carries
    the rasterizer's prologue, and values and gradients are those of the direct l1_and_ssim call."""
    from egogaussian_amd import patching
    from egogaussian_amd.fused import l1_and_ssim
    H, W = 96, 160
    student, cams, gts, bg = _frame(H, W)
    l1, ss = patching.make_loss_functions()
    n0 = dict(patching.calls)
    patched = _iteration(student, cams[1], gts[1], bg, lambda x, y: (l1(x, y), ss(x, y)))
    assert patching.calls["l1_loss"] == n0["l1_loss"] + 1 and patching.calls["ssim"] == n0["ssim"] + 1
    assert patched["nodes"][0] is not None and patched["nodes"][0] is patched["nodes"][1]
    assert patched["prepared"] and patched["tiles"] == list(range(((W + 15) // 16) * ((H + 15) // 16)))
    direct = _iteration(student, cams[1], gts[1], bg, l1_and_ssim)
    assert direct["prepared"]
    assert all(torch.equal(a, b) for a, b in zip(patched["values"], direct["values"]))
    assert torch.equal(patched["image"], direct["image"]) and float(direct["image"].abs().max()) > 0
    for k in LEAVES + ("screen",):
        a, b = direct[k], patched[k]
        assert float(a.abs().max()) > 0 and float((a - b).abs().max()) <= BAR(a), k
