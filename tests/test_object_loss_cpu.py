"""CPU: the object stages' loss -- the torch mirror against the reference's own value, the packed frame with an object mask, and the
additions to the C ABI (new symbols; every existing host struct keeps its size)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
load = lambda n: np.load(os.path.join(GOLD, n), allow_pickle=False)


def test_torch_mirror_reproduces_the_reference_loss():
    """losses.object_stage_loss on the captured render of the pose step (boundary_train.npz, written by the reference's own Python:
    trainers/fine_obj.py:136-149) gives the captured loss: 1e-6 relative."""
    from egogaussian_amd.losses import object_stage_loss
    g = load("boundary_train.npz")
    lam, l1a, l2a = [float(x) for x in g["pose_lambdas"]]
    T = lambda k: torch.tensor(g[k])
    for dtype in (torch.float32, torch.float64):
        v = object_stage_loss(T("pose_render").to(dtype), T("pose_alpha").to(dtype), T("pose_gt").to(dtype), T("pose_obj_mask").to(dtype), lam,
                              lambda_image=1.0, lambda_l1_alpha=l1a, lambda_l2_alpha=l2a)
        assert abs(float(v) - float(g["pose_loss"])) <= 1e-6 * abs(float(g["pose_loss"])), (dtype, float(v), float(g["pose_loss"]))
    # the terms are what they say: the mask multiplies gt, alpha is compared against the mask, the weights are the arguments
    from egogaussian_amd.losses import training_loss, l1_loss, l2_loss
    img, a, gt, m = T("pose_render").double(), T("pose_alpha").double(), T("pose_gt").double(), T("pose_obj_mask").double()
    want = 0.7 * training_loss(img, gt * m, lam) + 0.25 * l1_loss(m, a) + 0.125 * l2_loss(m, a)
    got = object_stage_loss(img, a[0], gt, m[0], lam, lambda_image=0.7, lambda_l1_alpha=0.25, lambda_l2_alpha=0.125)      # [H,W] alpha and mask
    assert abs(float(got) - float(want)) <= 1e-12
    assert float(object_stage_loss(img, a, gt, m, lam, 1.0, 0.0, 0.0)) == float(training_loss(img, gt * m, lam))


# frame_layout(3 * 37 * 53, 37 * 53, dynamic, gated, motion) of the commit before the obj_mask segment existed
OLD_LAYOUTS = {
    (False, False, False): ({"gt": (0, 5883), "cam": (5884, 5919)}, 5920),
    (False, False, True): ({"gt": (0, 5883), "cam": (5884, 5919), "accum_T": (5920, 5932)}, 5932),
    (False, True, False): ({"gt": (0, 5883), "cam": (5884, 5919), "gate": (5920, 7881)}, 7884),
    (False, True, True): ({"gt": (0, 5883), "cam": (5884, 5919), "accum_T": (5920, 5932), "gate": (5932, 7893)}, 7896),
    (True, False, False): ({"gt": (0, 5883), "cam": (5884, 5919), "accum_R": (5920, 5929)}, 5932),
    (True, False, True): ({"gt": (0, 5883), "cam": (5884, 5919), "accum_R": (5920, 5929), "accum_T": (5932, 5944)}, 5944),
    (True, True, False): ({"gt": (0, 5883), "cam": (5884, 5919), "accum_R": (5920, 5929), "gate": (5932, 7893)}, 7896),
    (True, True, True): ({"gt": (0, 5883), "cam": (5884, 5919), "accum_R": (5920, 5929), "accum_T": (5932, 5944), "gate": (5944, 7905)}, 7908),
}


def test_frame_layout_keeps_the_old_offsets_and_adds_an_aligned_mask_segment():
    from egogaussian_amd.graph import frame_layout
    H, W = 37, 53
    for dyn, gated, motion in itertools.product([False, True], repeat=3):
        old = OLD_LAYOUTS[(dyn, gated, motion)]
        assert frame_layout(3 * H * W, H * W, dyn, gated, motion) == old
        assert frame_layout(3 * H * W, H * W, dynamic=dyn, gated=gated, motion=motion, object_loss=False) == old
        off, size = frame_layout(3 * H * W, H * W, dyn, gated, motion, object_loss=True)
        b, e = off.pop("obj_mask")
        assert off == old[0]                                         # every other segment where it was
        assert b == old[1] and b % 4 == 0 and e - b == H * W and size == (e + 3) // 4 * 4 and size % 4 == 0


def test_pack_frame_stores_the_masked_image_and_the_mask():
    from egogaussian_amd.graph import frame_layout, pack_frame, pack_camera
    from egogaussian_amd.scene_synth import make_camera
    H, W = 37, 53
    gen = torch.Generator().manual_seed(3)
    cam = make_camera(7, H, W, device="cpu")
    gt = torch.rand(3, H, W, generator=gen)
    mask = (torch.rand(1, H, W, generator=gen) < 0.4).float()
    gate = torch.rand(H, W, generator=gen)
    R, Tm = torch.rand(3, 3, generator=gen), torch.rand(4, 4, generator=gen)
    f = pack_frame(cam, gt, R, gate, Tm, obj_mask=mask)
    off, size = frame_layout(3 * H * W, H * W, True, True, True, True)
    assert f.shape == (size,) and f.dtype == torch.float32
    seg = lambda k: f[off[k][0]:off[k][1]]
    assert torch.equal(seg("gt").view(3, H, W), gt * mask) and torch.equal(seg("obj_mask").view(H, W), mask[0])
    assert torch.equal(seg("gate").view(H, W), gate) and torch.equal(seg("accum_R").view(3, 3), R) and torch.equal(seg("accum_T").view(3, 4), Tm[:3])
    assert torch.equal(seg("cam"), pack_camera(cam))
    # without a mask: today's frame, bit for bit
    g = pack_frame(cam, gt, R, gate, Tm)
    off0, size0 = frame_layout(3 * H * W, H * W, True, True, True)
    assert g.shape == (size0,) and torch.equal(g[off0["gt"][0]:off0["gt"][1]].view(3, H, W), gt)
    assert torch.equal(g[off0["gt"][1]:], f[off["gt"][1]:size0])     # (everything behind the image is the same)


# sizeof of the host structs of include/egs_raster.h as they were before the object stages' loss (x86-64)
OLD_SIZES = {"egs_adam_leaf": 40, "egs_adam_sink": 272, "egs_object_rotation": 32, "egs_object_motion": 64, "egs_backward_prologue": 56, "egs_loss_grad": 88}


def test_library_exports_the_new_symbols_and_the_old_structs_keep_their_size():
    from egogaussian_amd import lib
    L = lib.load()
    for name in ("egs_object_loss_forward", "egs_object_loss_forward_ex", "egs_object_loss_backward_ex", "egs_backward_object_lossgrad"):
        assert hasattr(L, name) and name in lib.SIGNATURES, name
    assert L.egs_abi_version() == 6
    mirror = {"egs_adam_leaf": lib.AdamLeaf, "egs_adam_sink": lib.AdamSink, "egs_object_rotation": lib.ObjectRotation, "egs_object_motion": lib.ObjectMotion,
              "egs_backward_prologue": lib.BackwardPrologue, "egs_loss_grad": lib.LossGrad}
    for name, size in OLD_SIZES.items():
        assert C.sizeof(mirror[name]) == size, name
    assert C.sizeof(lib.ObjectLoss) == 48
    # argument errors precede device work
    assert L.egs_object_loss_forward(3, 8, 8, None, None, 0.2, None, None, None, None, None, None, None, None) == -1
    assert L.egs_object_loss_backward_ex(3, 8, 8, None, None, 0.2, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    # the header itself, through a C compiler where there is one: the binding's sizes are the header's
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        import tempfile
        names = list(OLD_SIZES) + ["egs_object_loss"]
        src = "#include <stdio.h>\n#include \"egs_raster.h\"\nint main(void) {" + \
            "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0; }\n"
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "s.c"), "w").write(src)
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
            out = dict(line.split() for line in subprocess.check_output([os.path.join(d, "s")]).decode().splitlines())
        assert {k: int(v) for k, v in out.items()} == dict(OLD_SIZES, egs_object_loss=48)
