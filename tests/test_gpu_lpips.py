"""GPU: LPIPS by the HIP kernels (egogaussian_amd/lpips.py LPIPS, csrc/lpips.hip) against the float64 torch statement on the CPU.

The yardstick of every comparison is the FLOAT32 torch statement's own distance from the float64 one on the same inputs (CPU):
  * tap feature maps: max-norm relative error <= 6 x the float32 statement's, per tap and case.  A CPU float32 run that accumulates K
    sequentially in chunks of 2 and 4, as an MFMA chain does, measured 1.6 - 3.1 x torch's blocked float32 (1.5e-6 against 4.9e-7 at worst);
    6 x leaves a factor of two over that, and a wrong lane map, halo or tap is off by orders of magnitude more;
  * the five tap values and their sum: relative error <= 6 x the LARGEST float32-statement distance over the whole case matrix (a scalar's
    per-case distance scatters from 1e-8 to 1e-6 and cannot serve as a yardstick);
  * a single layer: <= 6 x max(float32 F.conv2d's error, 2^-24) -- 2^-24 is the rounding of the one float32 store, below which a K = 36
    contraction's float32 error can fall by luck.
Random weights (LPIPSWeights.random(1)) and independent random 8-bit images: no VGG weights are shipped.  With EGS_LPIPS_PARITY_OUT=path the
figures of the case matrix are also written there as a table (profiles/lpips_parity.md is such a file)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((16, 16), (19, 35), (33, 47), (64, 64), (65, 130))
CASES = tuple((H, W, masked) for H, W in SIZES for masked in (False, True))
FACTOR = 6.0


@functools.lru_cache(maxsize=None)
def _weights():
    from egogaussian_amd.lpips import LPIPSWeights
    return LPIPSWeights.random(1)


@functools.lru_cache(maxsize=None)
def _net():
    from egogaussian_amd.lpips import LPIPS
    return LPIPS(_weights(), DEV)


def _inputs(H, W, masked):
    g = torch.Generator().manual_seed(1000 * H + 2 * W + int(masked))
    qx = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    qy = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    keep = (torch.rand(H, W, generator=g) >= 0.2).float() if masked else None          # binary, ~20 % of the pixels removed
    return qx, qy, keep


def _maxnorm(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@functools.lru_cache(maxsize=None)
def _case(H, W, masked):
    """One case, computed once: the float64 and float32 statements on the CPU, the HIP row and tap maps.  -> dict of figures."""
    from egogaussian_amd.lpips import lpips_vgg, vgg_taps
    qx, qy, keep = _inputs(H, W, masked)
    k64 = 1.0 if keep is None else keep.double()
    x64, y64 = qx.double() / 255 * k64, qy.double() / 255 * k64
    x32, y32 = (qx.float() / 255 * k64).float(), (qy.float() / 255 * k64).float()
    w = _weights()
    t64, s64 = lpips_vgg(x64, y64, w)
    t32, s32 = lpips_vgg(x32, y32, w)
    f64 = [vgg_taps(x64, w), vgg_taps(y64, w)]
    f32 = [vgg_taps(x32, w), vgg_taps(y32, w)]
    net = _net()
    res = net(qx.to(DEV), qy.to(DEV), keep=None if keep is None else keep.to(DEV))
    feats = [f.cpu() for f in net.features()]
    row = res["rows"].cpu().numpy()[0]
    assert int(res["cursor"].item()) == 1
    want = np.append(t64.numpy(), float(s64))
    got32 = np.append(t32.double().numpy(), float(s32))
    return dict(
        row=row, want=want,
        scalar_hip=np.abs(row - want) / np.abs(want), scalar_f32=np.abs(got32 - want) / np.abs(want),
        map_hip=[max(_maxnorm(feats[k][i].permute(2, 0, 1), f64[i][k]) for i in range(2)) for k in range(5)],
        map_f32=[max(_maxnorm(f32[i][k], f64[i][k]) for i in range(2)) for k in range(5)],
        shapes=[tuple(f.shape) for f in feats])


@functools.lru_cache(maxsize=None)
def _matrix():
    m = {c: _case(*c) for c in CASES}
    out = os.environ.get("EGS_LPIPS_PARITY_OUT")
    if out:
        yard = max(float(v["scalar_f32"].max()) for v in m.values())
        with open(out, "w") as fh:
            fh.write("# LPIPS: HIP kernels and the float32 torch statement (CPU) against the float64 torch statement\n\n"
                     "Written by tests/test_gpu_lpips.py (EGS_LPIPS_PARITY_OUT).  Random weights seed 1, independent random 8-bit images; "
                     "`keep` removes ~20 % of the pixels.\nMaps: max-norm relative error per tap (worse of the two images).  "
                     f"Scalars: largest relative error of the five taps and their sum.\n\nScalar yardstick (largest float32-statement distance of the matrix): {yard:.3e}; "
                     f"bar {FACTOR:g} x = {FACTOR * yard:.3e}\n\n| case | maps HIP | maps float32 statement | worst ratio | scalars HIP | scalars float32 |\n|---|---|---|---|---|---|\n")
            for (H, W, masked), v in m.items():
                fh.write(f"| {W}x{H}{' keep' if masked else ''} | {' '.join(f'{e:.2e}' for e in v['map_hip'])} | {' '.join(f'{e:.2e}' for e in v['map_f32'])} | "
                         f"{max(a / b for a, b in zip(v['map_hip'], v['map_f32'])):.2f} | {v['scalar_hip'].max():.2e} | {v['scalar_f32'].max():.2e} |\n")
    return m


@pytest.mark.parametrize("H,W,masked", CASES)
def test_tap_feature_maps(H, W, masked):
    v = _case(H, W, masked)
    print(f"{W}x{H} keep={masked}: maps HIP {['%.2e' % e for e in v['map_hip']]}, float32 statement {['%.2e' % e for e in v['map_f32']]}")
    assert v["shapes"] == [(2, H >> k, W >> k, c) for k, c in enumerate((64, 128, 256, 512, 512))]
    for k in range(5):
        assert v["map_f32"][k] > 0 and v["map_hip"][k] <= FACTOR * v["map_f32"][k], (k, v["map_hip"][k], v["map_f32"][k])


def test_tap_values_and_sum_over_the_case_matrix():
    m = _matrix()
    yard = max(float(v["scalar_f32"].max()) for v in m.values())
    for c, v in m.items():
        print(f"{c}: row {v['row']}, HIP rel err {v['scalar_hip'].max():.2e}, float32 statement {v['scalar_f32'].max():.2e}")
    print(f"yardstick {yard:.3e}, bar {FACTOR * yard:.3e}")
    assert 0 < yard < 1e-4                                                       # (a float32 distance, not a blunder of the statement's)
    for c, v in m.items():
        assert (v["want"] > 0).all() and v["scalar_hip"].max() <= FACTOR * yard, (c, v["scalar_hip"], yard)
        assert v["row"][5] == ((((v["row"][0] + v["row"][1]) + v["row"][2]) + v["row"][3]) + v["row"][4])      # the sum is formed in order


@pytest.mark.parametrize("cin,cout", ((4, 64), (64, 64), (512, 512)))
@pytest.mark.parametrize("H,W", ((16, 16), (5, 7), (1, 2)))
def test_single_layer_pins_the_lane_maps(cin, cout, H, W):
    """egs_conv3x3_relu_nhwc against F.conv2d in float64: ragged tiles, maps smaller than one tile, every output channel of every pixel."""
    from egogaussian_amd.lpips import conv3x3_relu_nhwc, pack_conv_weight
    g = torch.Generator().manual_seed(cin * 7 + cout + 100 * H + W)
    x = torch.randn(2, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.05
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    e32 = _maxnorm(F.relu(F.conv2d(x, w, b, padding=1)), want)
    packed = pack_conv_weight(w)
    assert tuple(packed.shape) == (9 * cin, cout)
    got = conv3x3_relu_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), packed.to(DEV), b.to(DEV)).cpu()
    err = _maxnorm(got.permute(0, 3, 1, 2), want)
    print(f"Cin {cin} Cout {cout} {W}x{H}: HIP {err:.2e}, float32 conv2d {e32:.2e}")
    assert tuple(got.shape) == (2, H, W, cout) and err <= FACTOR * max(e32, 2.0 ** -24)


def test_identical_pair_is_a_row_of_exact_zeros():
    qx, _, keep = _inputs(33, 47, True)
    net = _net()
    for k in (None, keep.to(DEV)):
        row = net(qx.to(DEV), qx.clone().to(DEV), keep=k)["rows"].cpu().numpy()[0]
        assert (row == 0).all() and not np.signbit(row).any(), row


def test_two_runs_give_identical_bits_and_a_full_array_is_left_alone():
    from egogaussian_amd import fused
    qx, qy, keep = _inputs(33, 47, True)
    net = _net()
    rows, cursor = fused.lpips_rows(2, DEV)
    args = (qx.to(DEV), qy.to(DEV), keep.to(DEV))
    net(*args, rows=rows, cursor=cursor)
    net(*args, rows=rows, cursor=cursor)
    r = rows.cpu().numpy()
    assert int(cursor.item()) == 2 and (r[0] > 0).all() and r[0].tobytes() == r[1].tobytes()
    assert r[0].tobytes() == _case(33, 47, True)["row"].tobytes()                 # ... and the bits of the earlier, separate call
    net(*args, rows=rows, cursor=cursor)                                          # the cursor stands at the capacity: nothing is written
    assert int(cursor.item()) == 3 and rows.cpu().numpy().tobytes() == r.tobytes()
    cursor.fill_(-1)
    net(*args, rows=rows, cursor=cursor)
    assert int(cursor.item()) == 0 and rows.cpu().numpy().tobytes() == r.tobytes()


def test_arguments_are_checked():
    from egogaussian_amd import fused
    net = _net()
    q = torch.zeros(3, 16, 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="smaller than 16"):
        net(q[:, :15].contiguous(), q[:, :15].contiguous())
    with pytest.raises(RuntimeError, match="uint8"):
        net(q.float(), q)
    with pytest.raises(RuntimeError, match="uint8"):
        net(q.cpu(), q.cpu())
    with pytest.raises(RuntimeError, match="go together"):
        net(q, q, rows=fused.lpips_rows(1, DEV)[0])
    with pytest.raises(RuntimeError, match="keep is a contiguous float32"):      # a gate on another device: its pointer never reaches the kernel
        net(q, q, keep=torch.ones(16, 16))


# ---- EvalPass(lpips=): the scene of tests/test_gpu_eval_pass.py -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweeps():
    from egogaussian_amd.evaluate import EvalPass
    from tests.test_gpu_eval_pass import _scene, _model
    s = _scene()
    out = {}
    for name, kw in (("graphed", dict(graphed=True, lpips=_net())), ("eager", dict(graphed=False, lpips=_net())), ("plain", dict(graphed=True))):
        ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1, keep_images=True, **kw)
        out[name] = (ev, ev.run(s["frames"], s["cams"][0]))
    return out


def test_eval_pass_graphed_eager_and_stand_alone_rows_are_the_same_bits():
    from egogaussian_amd.losses import quantize8
    from tests.test_gpu_eval_pass import _scene, F as N_FRAMES
    s, sw = _scene(), _sweeps()
    (ev_g, g), (ev_e, e) = sw["graphed"], sw["eager"]
    assert ev_g.host_reads == 1 and ev_e.host_reads == 1 and g["rerendered"] == [] and (g["instances"] > 0).all()
    assert g["lpips"].shape == (N_FRAMES,) and g["lpips_taps"].shape == (N_FRAMES, 5) and (g["lpips"] > 0).all()
    assert g["lpips"].tobytes() == e["lpips"].tobytes() and g["lpips_taps"].tobytes() == e["lpips_taps"].tobytes()
    assert g["mean_lpips"] == float(np.mean(g["lpips"])) and len(set(g["lpips"].tolist())) == N_FRAMES
    for k in range(N_FRAMES):
        row = _net()(g["images"][k].contiguous(), quantize8(s["gts"][k]).contiguous(), keep=s["keeps"][k])["rows"].cpu().numpy()[0]
        assert row[:5].tobytes() == g["lpips_taps"][k].tobytes() and row[5] == g["lpips"][k], k
    # a second sweep through the same captured graph starts again at row 0
    graph = ev_g.graph
    g2 = ev_g.run(s["frames"], s["cams"][0])
    assert ev_g.graph is graph and ev_g.host_reads == 2 and g2["lpips"].tobytes() == g["lpips"].tobytes()


def test_eval_pass_without_lpips_returns_what_it_returned():
    sw = _sweeps()
    g, p = sw["graphed"][1], sw["plain"][1]
    assert not any(k.startswith("lpips") or k == "mean_lpips" for k in p) and sorted(set(g) - set(p)) == ["lpips", "lpips_taps", "mean_lpips"]
    for k in ("sse", "ssim", "psnr", "instances"):
        assert g[k].tobytes() == p[k].tobytes(), k
    assert torch.equal(g["images"], p["images"]) and g["mean_psnr"] == p["mean_psnr"] and g["mean_ssim"] == p["mean_ssim"]


def test_eval_pass_clipped_frame_carries_the_eager_lpips_row():
    from egogaussian_amd.evaluate import EvalPass
    from tests.test_gpu_eval_pass import _scene, _model
    s, sw = _scene(), _sweeps()
    g, e = sw["graphed"][1], sw["eager"][1]
    order = np.argsort(g["instances"])
    top, second = int(g["instances"][order[-1]]), int(g["instances"][order[-2]])
    assert top > second + 1
    ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1, keep_images=True, lpips=_net())
    r = ev.run(s["frames"], s["cams"][0], capacity=(top + second) // 2)
    assert r["rerendered"] == [int(order[-1])] and ev.host_reads == 2
    assert r["lpips"].tobytes() == e["lpips"].tobytes() and r["lpips_taps"].tobytes() == e["lpips_taps"].tobytes()
    assert np.array_equal(r["sse"], e["sse"]) and torch.equal(r["images"], e["images"])


def test_shared_lpips_at_another_size_between_sweeps_leaves_the_captured_workspace_alone():
    """A captured pass has the workspace's address in its launches.  The same LPIPS object called at other sizes between two sweeps must
    neither free nor move it: the address stands, memory allocated in between is not written by the replay, the rows are the eager ones."""
    from egogaussian_amd.evaluate import EvalPass
    from tests.test_gpu_eval_pass import _scene, _model, H as SH, W as SW
    from egogaussian_amd.lpips import LPIPS
    s, e = _scene(), _sweeps()["eager"][1]
    net = LPIPS(_weights(), DEV)                                                  # its own object: no workspace from earlier tests
    ev = EvalPass(_model(), s["bg"], dynamic=True, motion=True, which_object=1, lpips=net)
    r1 = ev.run(s["frames"], s["cams"][0])
    graph, ws = ev.graph, net.workspace(SH, SW)
    at, size = ws.data_ptr(), ws.numel()
    for H, W in ((16, 16), (33, 47)):
        qx, qy, _ = _inputs(H, W, False)
        net(qx.to(DEV), qy.to(DEV))
    canary = torch.full((size // 4,), 7.0, device=DEV)                            # as large as the workspace: where a freed one would be handed out
    r2 = ev.run(s["frames"], s["cams"][0])
    torch.cuda.synchronize()
    assert ev.graph is graph and net.workspace(SH, SW).data_ptr() == at and len(net._workspaces) == 3
    assert bool((canary == 7.0).all())
    for r in (r1, r2):
        assert r["lpips"].tobytes() == e["lpips"].tobytes() and r["lpips_taps"].tobytes() == e["lpips_taps"].tobytes()
    assert [tuple(f.shape[1:3]) for f in net.features()] == [(33 >> k, 47 >> k) for k in range(5)]      # the last call through the object
    assert [tuple(f.shape[1:3]) for f in net.features((SH, SW))] == [(SH >> k, SW >> k) for k in range(5)] and net.features((SH, SW))[0].data_ptr() > at
    with pytest.raises(RuntimeError, match="nothing has run yet at 20x20"):
        net.features((20, 20))
