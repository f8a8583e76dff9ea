"""CPU: the mask hand-off's C ABI (declared, bound, exported; argument errors before any device work), its torch statements
(losses.label_mask, losses.interaction_gate) against the numpy definitions of tests/mask_anchor.py and against the reference's conv2d line,
the row decoding of masks.MaskPass, and the refusal of CPU tensors.  Everything is integer-exact: every comparison is an equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mask_anchor as MA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_label_mask", "egs_label_mask_partial_bytes", "egs_interaction_gate")


def test_header_binding_and_library_agree_within_abi_6():
    from egogaussian_amd import lib
    L = lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egs_raster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", text))
    for n in NEW:
        assert n in declared and n in lib.SIGNATURES and hasattr(L, n), n
    assert declared == set(lib.SIGNATURES)
    assert L.egs_abi_version() == 6 and lib.ABI_VERSION == 6 and re.search(r"#define\s+EGS_ABI_VERSION\s+6\b", text)
    assert C.sizeof(lib.MaskRow) == 48 and [f[0] for f in lib.MaskRow._fields_] == ["predicted", "target", "intersection", "kept", "clipped", "instances"]
    assert "typedef struct egs_mask_row" in text
    from egogaussian_amd import fused
    assert fused.MASK_ROW_WORDS * 8 == C.sizeof(lib.MaskRow)


def test_interaction_gate_argument_errors_precede_device_work():
    from egogaussian_amd import lib
    L = lib.load()
    p = 4096                                                           # (fake non-null pointers are never dereferenced before the checks)
    for k in (0, 2, 4, 33, -1):
        assert L.egs_interaction_gate(8, 8, p, p, k, p, None) == -1, k
    assert L.egs_interaction_gate(8, 8, None, None, 3, p, None) == -1   # both inputs absent
    assert L.egs_interaction_gate(8, 8, p, p, 3, None, None) == -1      # no output
    assert L.egs_interaction_gate(0, 8, p, p, 3, p, None) == -1 and L.egs_interaction_gate(8, 0, p, p, 3, p, None) == -1
    assert L.egs_interaction_gate(-3, 8, p, None, 1, p, None) == -1 and L.egs_interaction_gate(8, -1, None, p, 1, p, None) == -1
    assert L.egs_interaction_gate(65536, 32768, p, None, 3, p, None) == -3


def test_label_mask_argument_errors_precede_device_work():
    from egogaussian_amd import lib
    L = lib.load()
    p = 4096
    assert L.egs_label_mask(8, 8, None, 0.5, None, None, None, p, None, p, 1, p, None) == -1     # no image
    assert L.egs_label_mask(8, 8, p, 0.5, None, None, None, None, None, p, 1, p, None) == -1     # no partial scratch
    assert L.egs_label_mask(8, 8, p, 0.5, None, None, None, p, None, p, 1, None, None) == -1     # no cursor
    assert L.egs_label_mask(8, 8, p, 0.5, None, None, None, p, None, None, 1, p, None) == -1     # no rows
    assert L.egs_label_mask(0, 8, p, 0.5, p, p, None, p, p, p, 1, p, None) == -1
    assert L.egs_label_mask(8, 0, p, 0.5, p, p, None, p, p, p, 1, p, None) == -1
    assert L.egs_label_mask(8, 8, p, 0.5, p, p, None, p, p, p, -1, p, None) == -1
    assert L.egs_label_mask(65536, 32768, p, 0.5, None, None, None, p, None, p, 1, p, None) == -3
    pb = L.egs_label_mask_partial_bytes
    assert pb(0, 5) == 0 and pb(5, 0) == 0 and pb(1, 1) == 16
    sizes = [pb(h, w) for h, w in ((1, 1), (5, 7), (37, 53), (48, 64), (70, 130), (540, 960), (1080, 1920))]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(s % 16 == 0 for s in sizes)
    assert pb(540, 960) >= (540 * 960 + 1023) // 1024 * 16


def _random_masks(H, W, density, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(H, W, generator=g) < density).float(), (torch.rand(H, W, generator=g) < density).float()


@pytest.mark.parametrize("shape", [(1, 1), (3, 40), (37, 53)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [1, 3, 5, 7, 31])
def test_torch_gate_equals_the_definition_and_the_reference_line(shape, k):
    from egogaussian_amd.losses import interaction_gate
    H, W = shape
    for density in (0.01, 0.3):
        a, b = _random_masks(H, W, density, seed=1000 * k + H + int(100 * density))
        if density == 0.01:
            a[H - 1, W - 1] = 1.0                                        # (a 1 % mask of a few pixels may be empty)
        for hand, obj in ((a, b), (a, None)):
            got = interaction_gate(hand, obj, k)
            assert got.dtype == torch.float32 and tuple(got.shape) == (H, W)
            want = MA.gate_np(hand.numpy(), None if obj is None else obj.numpy(), k)
            assert np.array_equal(got.numpy(), want), (shape, k, density)
            # the reference's own line: trainers/train_static_bg.py dilate_mask on logical_or(hand, obj)
            m = hand.bool() if obj is None else torch.logical_or(hand, obj)
            dil = torch.nn.functional.conv2d(m.int()[None].unsqueeze(0).float(), torch.ones(1, 1, k, k), padding=k // 2) > 0
            assert torch.equal(got, 1.0 - dil[0, 0].float()), (shape, k, density)
    assert torch.equal(interaction_gate(a[None], b[None], None), interaction_gate(a, b, 1))      # [1,H,W]; None means no dilation
    # logical_or's rule: NaN, negative and fractional values are set
    odd = torch.zeros(H, W); odd[0, 0] = float("nan")
    assert interaction_gate(odd, None, 1)[0, 0] == 0.0
    for v in (-1.0, 0.25, 2.0):
        odd[0, 0] = v
        assert interaction_gate(odd, None, k)[0, 0] == 0.0 and interaction_gate(torch.zeros(H, W), odd, k)[0, 0] == 0.0
    with pytest.raises(ValueError):
        interaction_gate(a, b, 4)


@pytest.mark.parametrize("thr", [0.5, -0.25])
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 53)], ids=lambda s: "x".join(map(str, s)))
def test_torch_label_mask_equals_the_definition(shape, thr):
    from egogaussian_amd.losses import label_mask
    H, W = shape
    img, spots = MA.special_label_image(H, W, thr, seed=H * W)
    rng = np.random.default_rng(5)
    target = (rng.random((H, W)) < 0.4).astype(np.float32)
    keep = (rng.random((H, W)) < 0.7).astype(np.float32)
    for t, k in ((target, keep), (target, None), (None, keep), (None, None)):
        want = MA.label_mask_np(img, thr, t, k)
        got = label_mask(torch.from_numpy(img), thr, None if t is None else torch.from_numpy(t)[None], None if k is None else torch.from_numpy(k))
        assert got["mask"].dtype == torch.uint8 and np.array_equal(got["mask"].numpy(), want["mask"])
        for name in ("predicted", "target", "intersection", "kept"):
            assert got[name].dtype == torch.int64 and int(got[name]) == want[name], (name, shape, thr)
    full = MA.label_mask_np(img, thr, target, keep)
    assert set(np.unique(full["mask"])) <= {0, 255} and full["kept"] == int(keep.sum()) and full["intersection"] <= min(full["predicted"], full["target"])
    expect = {"exact": 0, "next": 255, "nan": 0, "differ": 255}
    assert "exact" in spots
    for name, (y, x) in spots.items():
        assert full["mask"][y, x] == expect[name], (name, thr)
    if H * W > 1:
        assert {"exact", "next", "nan", "differ"} <= set(spots)
        # the stored mask ignores keep: gating everything changes the counts, not a byte
        none_kept = MA.label_mask_np(img, thr, target, np.zeros((H, W), np.float32))
        assert np.array_equal(none_kept["mask"], full["mask"]) and none_kept["predicted"] == none_kept["kept"] == 0


def test_row_decoding_and_iou():
    from egogaussian_amd.masks import decode_rows
    rows = torch.tensor([[10, 8, 6, 100, 0, 1234],
                         [0, 0, 0, 50, 0, 7],                          # empty union: IoU 1
                         [5, 0, 0, 50, 1, 99],                          # clipped
                         [3, 3, 3, 3, 0, 0]], dtype=torch.int64)
    d = decode_rows(rows)
    assert d["iou"].dtype == np.float64 and np.array_equal(d["iou"], np.array([6 / 12, 1.0, 0.0, 1.0]))
    assert np.array_equal(d["predicted"], [10, 0, 5, 3]) and np.array_equal(d["target"], [8, 0, 0, 3]) and np.array_equal(d["intersection"], [6, 0, 0, 3])
    assert np.array_equal(d["kept"], [100, 50, 50, 3]) and np.array_equal(d["clipped"], [False, False, True, False]) and np.array_equal(d["instances"], [1234, 7, 99, 0])
    assert all(d[k].dtype == np.int64 for k in ("predicted", "target", "intersection", "kept", "instances"))


def test_fused_routes_refuse_cpu_tensors():
    from egogaussian_amd import fused
    from egogaussian_amd.masks import MaskPass
    from egogaussian_amd.scene_synth import make_camera
    img = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.label_mask(img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.interaction_gate(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.interaction_gate(torch.zeros(1, 4, 4), torch.zeros(4, 4), 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MaskPass(None, torch.zeros(3)).run([torch.zeros(64)], make_camera(0, 4, 4))
    rows, cursor = fused.mask_rows(3, "cpu")
    assert tuple(rows.shape) == (3, 6) and rows.dtype == torch.int64 and cursor.dtype == torch.int32 and int(cursor) == 0
