"""CPU: the torch statement of LPIPS (egogaussian_amd/lpips.py lpips_vgg) against the independent numpy anchor (tests/lpips_anchor.py) in
float64, four wrong statements the comparison catches, the weight constructors and the size limit.  Random weights (LPIPSWeights.random):
no VGG weights are shipped."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_anchor as LA

# float64 on both sides (eps 1.1e-16), up to 4 608 products per output, 13 layers deep: rounding differences random-walk to the order of
# 1e-15 .. 1e-14.  The subtlest of the wrong statements below, the eps inside the root, moves a tap by ~1e-10 / |f|^2 ~ 1e-11.
BAR = 1e-13
SIZES = ((16, 16), (19, 35))            # 19 -> 9 -> 4 -> 2 -> 1 and 35 -> 17 -> 8 -> 4 -> 2: odd at several levels


@functools.lru_cache(maxsize=None)
def _weights():
    from egogaussian_amd.lpips import LPIPSWeights
    return LPIPSWeights.random(1)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """Independent random 8-bit images as float64 in [0,1], and the anchor's figures for them."""
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randint(0, 256, (3, H, W), generator=g).double() / 255
    y = torch.randint(0, 256, (3, H, W), generator=g).double() / 255
    taps, total = LA.lpips(x.numpy(), y.numpy(), *LA.numpy_weights(_weights()))
    return x, y, taps, total


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())


def _variant(x, y, weights, pad_zscore_of_zero=False, taps_late=False, ceil_pool=False, eps_inside=False):
    """The definition once more with four switches, each a plausible misreading.  All off: the statement itself (checked below)."""
    from egogaussian_amd import lpips as LP
    dt = x.dtype
    mean, std = torch.tensor(LP.MEAN, dtype=dt)[:, None, None], torch.tensor(LP.STD, dtype=dt)[:, None, None]

    def feats(v):
        first_pad = 1
        if pad_zscore_of_zero:                               # zeros around the IMAGE: the border then holds (0 - mean) / std
            v, first_pad = F.pad(v, (1, 1, 1, 1)), 0
        f = ((v - mean) / std)[None]
        out, layer = [], 0
        for k, n in enumerate(LP.BLOCKS):
            for j in range(n):
                w, b = weights.convs[layer]
                f = F.relu(F.conv2d(f, w.to(dt), b.to(dt), padding=first_pad if layer == 0 else 1))
                layer += 1
            if not taps_late:
                out.append(f[0])
            if k < 4:
                f = F.max_pool2d(f, 2, 2, ceil_mode=ceil_pool)
            if taps_late:                                    # the slice ends one module later: the tap sees the pooled map
                out.append(f[0])
        return out
    vals = []
    for fx, fy, l in zip(feats(x), feats(y), weights.lins):
        norm = (lambda f: (f.pow(2).sum(0, keepdim=True) + LP.EPS).sqrt()) if eps_inside else (lambda f: f.pow(2).sum(0, keepdim=True).sqrt() + LP.EPS)
        d = fx / norm(fx) - fy / norm(fy)
        vals.append((l.to(dt)[:, None, None] * d.pow(2)).sum(0).mean())
    return torch.stack(vals)


@pytest.mark.parametrize("H,W", SIZES)
def test_statement_equals_the_anchor(H, W):
    from egogaussian_amd.lpips import lpips_vgg, vgg_taps
    x, y, taps, total = _case(H, W)
    got_taps, got_total = lpips_vgg(x, y, _weights())
    print(f"{W}x{H}: taps {taps}, sum {total:.6e}; statement - anchor: taps {_rel(got_taps.numpy(), taps):.2e}, sum {abs(float(got_total) - total) / total:.2e}")
    assert got_taps.dtype == torch.float64 and tuple(got_taps.shape) == (5,)
    assert (taps > 0).all() and _rel(got_taps.numpy(), taps) <= BAR and abs(float(got_total) - total) <= BAR * total
    for k, (a, b) in enumerate(zip(vgg_taps(x, _weights()), LA.taps(x.numpy(), LA.numpy_weights(_weights())[0]))):
        assert tuple(a.shape) == b.shape == (LA_CHANNELS[k], H >> k, W >> k) and _rel(a.numpy(), b) <= BAR, k
    # the switchable copy with every switch off IS the statement
    assert torch.equal(_variant(x, y, _weights()), got_taps)


LA_CHANNELS = (64, 128, 256, 512, 512)


@pytest.mark.parametrize("wrong", ("pad_zscore_of_zero", "taps_late", "ceil_pool", "eps_inside"))
def test_wrong_statements_are_caught(wrong):
    """Each misreading moves a tap of the 19x35 case by more than ten times the bar the statement is held to."""
    x, y, taps, _ = _case(19, 35)
    got = _variant(x, y, _weights(), **{wrong: True}).numpy()
    per_tap = np.abs(got - taps) / taps
    print(f"{wrong}: relative tap differences {per_tap}")
    assert per_tap.max() > 10 * BAR


def test_identical_pair_is_exactly_zero():
    from egogaussian_amd.lpips import lpips_vgg
    x = _case(19, 35)[0]
    for dt in (torch.float64, torch.float32):
        taps, total = lpips_vgg(x.to(dt), x.to(dt).clone(), _weights())
        assert taps.dtype == dt and float(total) == 0.0 and (taps == 0).all()


def test_from_state_dicts_accepts_both_key_forms_and_refuses_others():
    from egogaussian_amd.lpips import LPIPSWeights, VGG_FEATURE_INDICES, lpips_vgg
    w = _weights()
    vgg = {}
    for i, (cw, cb) in zip(VGG_FEATURE_INDICES, w.convs):
        vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"] = cw, cb
    vgg["classifier.0.weight"] = torch.zeros(2, 2)                               # ignored
    forms = ({f"lin{k}.model.1.weight": l.reshape(1, -1, 1, 1) for k, l in enumerate(w.lins)},
             {f"{k}.1.weight": l.reshape(1, -1, 1, 1) for k, l in enumerate(w.lins)})
    x, y = _case(16, 16)[:2]
    want = lpips_vgg(x, y, w)[1]
    for lin in forms:
        got = LPIPSWeights.from_state_dicts(vgg, lin)
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got.convs, w.convs))
        assert all(torch.equal(a, b) for a, b in zip(got.lins, w.lins)) and torch.equal(lpips_vgg(x, y, got)[1], want)
    moved = w.to("cpu")
    assert moved is not w and all(torch.equal(a[0], b[0]) for a, b in zip(moved.convs, w.convs)) and torch.equal(lpips_vgg(x, y, moved)[1], want)
    t = LPIPSWeights.from_tensors([c[0] for c in w.convs], [c[1] for c in w.convs], w.lins)
    assert torch.equal(lpips_vgg(x, y, t)[1], want)
    with pytest.raises(KeyError, match=r"lin0\.weight"):                        # names the keys it found
        LPIPSWeights.from_state_dicts(vgg, {f"lin{k}.weight": l.reshape(1, -1, 1, 1) for k, l in enumerate(w.lins)})
    with pytest.raises(KeyError, match=r"features\.28"):
        LPIPSWeights.from_state_dicts({k: v for k, v in vgg.items() if not k.startswith("features.28.")}, forms[0])
    with pytest.raises(ValueError, match="head 2"):
        LPIPSWeights.from_state_dicts(vgg, dict(forms[0], **{"lin2.model.1.weight": w.lins[2].reshape(-1, 1, 1, 1)}))
    with pytest.raises(ValueError, match="convolution 3"):
        LPIPSWeights([c if k != 3 else (c[0][:, :64], c[1]) for k, c in enumerate(w.convs)], w.lins)


@pytest.mark.parametrize("H,W", ((15, 16), (16, 15), (8, 64)))
def test_small_images_are_refused(H, W):
    from egogaussian_amd.lpips import lpips_vgg
    with pytest.raises(ValueError, match="smaller than 16"):
        lpips_vgg(torch.zeros(3, H, W), torch.zeros(3, H, W), _weights())


def test_random_weights_keep_the_activations_of_order_one():
    """What makes LPIPSWeights.random a usable test model: no layer's features die out or blow up."""
    from egogaussian_amd.lpips import vgg_taps
    for k, f in enumerate(vgg_taps(_case(19, 35)[0], _weights())):
        rms = float(f.pow(2).mean().sqrt())
        assert 0.05 < rms < 20.0, (k, rms)


def test_packed_weight_order():
    """pack_conv_weight: row (3 ky + kx) * Cin' + c, column o; the first layer's fourth input row is zero."""
    from egogaussian_amd.lpips import pack_conv_weight
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3)
    p = pack_conv_weight(w)
    assert tuple(p.shape) == (36, 2) and p[(3 * 1 + 2) * 4 + 1, 1] == w[1, 1, 1, 2] and (p[3::4] == 0).all()
    w = torch.arange(2 * 16 * 9, dtype=torch.float32).reshape(2, 16, 3, 3)
    p = pack_conv_weight(w)
    assert tuple(p.shape) == (144, 2) and p[(3 * 2 + 0) * 16 + 5, 0] == w[0, 5, 2, 0]


def test_c_abi_sizes_and_argument_errors_precede_device_work():
    """include/egs_raster.h egs_lpips_*: host arithmetic and argument checks only (fake pointers are never dereferenced)."""
    import ctypes as C
    from egogaussian_amd import lib
    L = lib.load()
    ws = L.egs_lpips_workspace_bytes
    assert ws(15, 64) == 0 and ws(64, 15) == 0 and ws(9000, 64) == 0 and ws(16, 16) > 0 and ws(16, 16) % 256 == 0
    assert 411 * 540 * 960 * 4 <= ws(540, 960) <= 413 * 540 * 960 * 4             # all five tap maps stay: 412 H W floats less the pools' floors, 0.85 GB
    off = (C.c_int64 * 5)()
    assert L.egs_lpips_tap_offsets(19, 35, off) == 0 and L.egs_lpips_tap_offsets(8, 35, off) == -1 and L.egs_lpips_tap_offsets(19, 35, None) == -1
    sizes = [2 * (19 >> k) * (35 >> k) * c * 4 for k, c in enumerate((64, 128, 256, 512, 512))]
    assert all(o % 256 == 0 for o in off) and all(off[k] + sizes[k] <= off[k + 1] for k in range(4)) and off[4] + sizes[4] <= ws(19, 35)
    p, q = 4096, 4096 + 8
    wt = lib.LpipsWeights()
    fwd = lambda H=64, W=64, qx=p, qy=p, keep=None, w=wt, wsp=p, rows=p, cap=4, cur=p: L.egs_lpips_forward(
        H, W, qx, qy, keep, None if w is None else C.byref(w), wsp, rows, cap, cur, None)
    assert fwd() == -1                                                            # NULL weight arrays
    for i in range(13):
        wt.conv_w[i], wt.conv_b[i] = p, p
    for k in range(5):
        wt.lin[k] = p
    for kw in (dict(H=15), dict(W=8), dict(qx=None), dict(qy=None), dict(w=None), dict(wsp=None), dict(wsp=q), dict(rows=None), dict(cur=None), dict(cap=-1)):
        assert fwd(**kw) == -1, kw
    assert fwd(H=9000) == -3
    wt.conv_w[7] = q
    assert fwd() == -1
    conv = lambda n=2, H=5, W=7, cin=64, cout=64, i=p, w=p, b=p, o=8192: L.egs_conv3x3_relu_nhwc(n, H, W, cin, cout, i, w, b, o, None)
    for kw in (dict(n=0), dict(H=0), dict(W=0), dict(cin=3), dict(cin=8), dict(cin=24), dict(cout=32), dict(cout=96), dict(i=None), dict(w=None), dict(b=None),
               dict(o=None), dict(o=p), dict(i=q)):
        assert conv(**kw) == -1, kw
    assert conv(H=40000) == -3 and conv(cin=8192) == -3 and conv(n=70000) == -3
