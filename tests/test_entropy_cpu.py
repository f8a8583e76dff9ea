"""CPU: the opacity-entropy regulariser -- the float64 anchor and its bars (tests/entropy_anchor.py) against the torch expression of
/root/reference/trainers/train_static.py:97-102 (the yardstick), the wrong variants the bars must refuse, losses.opacity_entropy,
GraphedTrainStep(entropy_reg=True) argument validation, and the C ABI additions (exported, mirrored in lib.py, argument errors before any
device work)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import entropy_anchor as EA

N, SEED, WEIGHT = 20011, 0, 0.1


@pytest.fixture(scope="module")
def yardstick():
    """torch's float32 autograd of the reference expression on the anchor's inputs, computed once."""
    x, vis = EA.inputs(N, SEED)
    xt = torch.tensor(x, requires_grad=True)
    o = torch.sigmoid(xt)
    v = o[torch.tensor(vis)]
    H = (-v * torch.log(v + 1e-10) - (1 - v) * torch.log(1 - v + 1e-10)).mean()
    (WEIGHT * H).backward()
    o32 = o.detach().numpy()
    return dict(x=x, vis=vis, o32=o32, value=float(H.detach()), grad=xt.grad.numpy().copy(), ref=EA.anchor(o32, vis, WEIGHT, 1.0, logit=True))


def test_inputs_cover_the_edges(yardstick):
    x, vis, o32 = yardstick["x"], yardstick["vis"], yardstick["o32"]
    assert x.shape == (N,) and 0.55 < vis.mean() < 0.65
    assert (o32 == 1).sum() >= 4 and (o32 == 0).sum() >= 1 and (o32 == 0.5).sum() >= 2       # saturated both ways, and the exact middle
    assert set(np.float32(EA.FIXED_LOGITS)) <= set(x)


def test_torch_float32_yardstick_sits_under_half_of_each_bar(yardstick):
    """The bars are not tuned to the code under test: float32 autograd of the reference's own expression must clear HALF of each."""
    ref = yardstick["ref"]
    g = yardstick["grad"]
    assert np.isfinite(g).all() and (g[~yardstick["vis"]] == 0).all()
    worst = EA.grad_excess(g, ref)
    print(f"\n  yardstick: worst gradient error {worst:.2f} x 2^-24 of the unit (bar {EA.GRAD_ULPS}); value off by {abs(yardstick['value'] - ref['value']):.2e}")
    assert worst <= 0.5 * EA.GRAD_ULPS
    assert EA.grad_ok(g, ref, factor=0.5) and EA.value_ok(yardstick["value"], ref, factor=0.5)


def test_subnormal_gradients_need_the_underflow_term_of_the_bar():
    """Every row visible: the row at logit -88 has a subnormal gradient (o = 6e-39).  torch's float32 autograd of the reference expression
    misses the purely relative bar THERE and nowhere else -- float32 resolves 2^-149 absolute down there -- and clears half of the bar with
    its one-quantum underflow term (tests/entropy_anchor.py, "Underflow")."""
    x, _ = EA.inputs(255, 3)
    vis = np.ones(255, bool)
    xt = torch.tensor(x, requires_grad=True)
    o = torch.sigmoid(xt)
    (0.25 * (-o * torch.log(o + 1e-10) - (1 - o) * torch.log(1 - o + 1e-10)).mean()).backward()
    ref = EA.anchor(o.detach().numpy(), vis, 0.25, 1.0, logit=True)
    g = xt.grad.numpy().astype(np.float64)
    sub = (np.abs(ref["grad"]) < 2.0 ** -126) & (ref["grad"] != 0)
    assert sub.sum() >= 1 and float(x[sub].max()) <= -87.0
    rel = np.zeros(255); m = ref["unit"] > 0
    rel[m] = np.abs(g - ref["grad"])[m] / (EA.U * ref["unit"][m])
    print(f"\n  all rows visible: worst relative error {rel[~sub].max():.2f} x 2^-24 on the normal rows, {rel[sub].max():.1f} x 2^-24 on the subnormal one(s)")
    assert rel[~sub].max() <= 0.5 * EA.GRAD_ULPS
    assert np.abs(g - ref["grad"])[sub].max() <= EA.TINY
    assert EA.grad_ok(g, ref, factor=0.5)
    assert EA.grad_excess(g, ref, tiny=0.0) == rel.max()


def test_anchor_is_finite_at_saturation_and_nan_without_visible_rows():
    o = np.float32([0.0, 1.0, 0.5, 1 - 2.0 ** -24, 2.0 ** -30])
    r = EA.anchor(o, np.ones(5, bool), 1.0, 1.0, logit=False)
    assert np.isfinite(r["grad"]).all() and np.isfinite(r["value"]) and r["grad"][2] == 0.0
    assert abs(r["grad"][0] - (-np.log(np.float64(np.float32(1e-10))) + 1.0) / 5) < 1e-12      # o = 0: (-ln(1e-10f) + 1 / 1) / n_vis
    r0 = EA.anchor(o, np.zeros(5, bool))
    assert np.isnan(r0["value"]) and (r0["grad"] == 0).all() and r0["n_vis"] == 0
    assert EA.value_ok(float("nan"), r0) and not EA.value_ok(0.0, r0)


def _variant(o32, vis, kind, weight=WEIGHT):
    o = o32.astype(np.float64)
    om = (np.float32(1) - o32).astype(np.float64)
    eps = 0.0 if kind == "no_eps" else 1e-10
    with np.errstate(all="ignore"):
        a, b = o + eps, om + eps
        dh = -np.log(a) - o / a + np.log(b) + om / b
        if kind == "pair_dropped":
            dh = -np.log(a) + np.log(b)
        n = len(o) if kind == "mean_over_all" else int(vis.sum())
        g = weight / n * dh * o * (1 - o)
    if kind == "sign":
        g = -g
    if kind != "invisible_rows":
        g = np.where(vis, g, 0.0)
    return g


@pytest.mark.parametrize("kind", ["mean_over_all", "pair_dropped", "sign", "invisible_rows", "no_eps"])
def test_the_check_refuses_wrong_variants(yardstick, kind):
    g = _variant(yardstick["o32"], yardstick["vis"], kind)
    assert not EA.grad_ok(g, yardstick["ref"]), kind
    if kind == "no_eps":
        assert not np.isfinite(g).all()                              # NaN at saturation: what the 1e-10 is there for


def test_the_check_accepts_the_exact_gradient(yardstick):
    ref = yardstick["ref"]
    assert EA.grad_ok(ref["grad"], ref, factor=1e-6) and EA.value_ok(ref["value"], ref, factor=0.0)
    assert not EA.value_ok(ref["value"] + 3e-5, ref)
    all_rows = EA.anchor(yardstick["o32"], np.ones(N, bool), WEIGHT)
    assert not EA.value_ok(all_rows["value"] * len(ref["grad"]) / ref["n_vis"], ref)             # a sum divided by the wrong count


def test_losses_opacity_entropy_is_the_reference_expression():
    from egogaussian_amd.losses import opacity_entropy
    x, vis = EA.inputs(4001, 3)
    o = torch.sigmoid(torch.tensor(x, dtype=torch.float64)).reshape(-1, 1).requires_grad_(True)
    m = torch.tensor(vis)
    got = opacity_entropy(o, m)
    v = o.detach().numpy().reshape(-1)[vis]
    with np.errstate(all="ignore"):
        want = float((-v * np.log(v + 1e-10) - (1 - v) * np.log(1 - v + 1e-10)).mean())
    assert abs(float(got.detach()) - want) <= 1e-13
    got.backward()
    od = o.detach().numpy().reshape(-1)
    dh = np.where(vis, (-np.log(od + 1e-10) - od / (od + 1e-10) + np.log(1 - od + 1e-10) + (1 - od) / (1 - od + 1e-10)) / vis.sum(), 0.0)
    assert np.abs(o.grad.numpy().reshape(-1) - dh).max() <= 1e-12 * np.abs(dh).max()
    assert torch.isnan(opacity_entropy(o.detach(), torch.zeros_like(m)))                       # torch's mean() of an empty tensor
    # float32, [P] and [P,1] alike
    o32 = torch.sigmoid(torch.tensor(x))
    assert float(opacity_entropy(o32, m)) == float(opacity_entropy(o32.reshape(-1, 1), m))


def test_graphed_step_argument_validation():
    """entropy_reg goes with the static image step only; it is refused before anything touches a device."""
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4, 3))
    opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": "xyz"}], capturable=True)
    bg = torch.zeros(3)

    class Pose:
        obj_translation = obj_rotation_6d = p
    for kw, name in ((dict(dynamic=True), "dynamic"), (dict(dynamic=True, motion=True), "dynamic"), (dict(motion=True), "motion"),
                     (dict(pose=Pose()), "pose"), (dict(object_loss=dict(lambda_image=1.0)), "object_loss"), (dict(label_phase=True), "label_phase")):
        with pytest.raises(ValueError, match=f"entropy_reg=True\\) does not go with {name}"):
            GraphedTrainStep(None, opt, bg, entropy_reg=True, **kw)
    for kw in (dict(gated=True), dict(densify_stats=True), dict(steps_per_replay=3), dict(double_buffer=True), dict(fuse_optimizer=False)):
        step = GraphedTrainStep(None, opt, bg, entropy_reg=True, **kw)
        assert step.entropy_reg and step.entropy_weight == 0.0 and step.entropy is None
        step.entropy_weight = 0.1                                    # a host value until the capture creates the device scalar
        assert step.entropy_weight == 0.1
    plain = GraphedTrainStep(None, opt, bg)
    assert not plain.entropy_reg
    with pytest.raises(ValueError, match="without entropy_reg"):
        plain.entropy_weight = 0.1


NEW_SYMBOLS = ("egs_opacity_entropy_scratch_bytes", "egs_opacity_entropy_forward", "egs_opacity_entropy_backward", "egs_backward_entropy_lossgrad")


def test_abi_additions_are_exported_mirrored_and_check_their_arguments():
    from egogaussian_amd import lib
    from tests.test_abi_cpu import _declared_symbols
    L = lib.load()
    declared = _declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(L, n) and n in lib.SIGNATURES, n
    # additions only: the entry point beside it keeps its signature, the ABI number stays
    assert len(lib.SIGNATURES["egs_backward_entropy_lossgrad"][1]) == len(lib.SIGNATURES["egs_backward_lossgrad"][1]) + 4
    assert L.egs_abi_version() == 6 == lib.ABI_VERSION
    assert [f[0] for f in lib.OpacityEntropy._fields_] == ["weight", "upstream", "scratch", "n_vis", "value"]
    assert C.sizeof(lib.OpacityEntropy) == 5 * C.sizeof(C.c_void_p)
    # one float32 sum and one count per 256 rows, 256-byte aligned
    sb = L.egs_opacity_entropy_scratch_bytes
    assert sb(0) == 0 and sb(1) == 256 and sb(256 * 32) == 256 and sb(256 * 32 + 1) == 512 and sb(70001) >= 274 * 8 and sb(70001) % 256 == 0
    # argument errors before any device work (fake non-null pointers are never dereferenced)
    p = C.c_void_p(4096)
    ent = lib.OpacityEntropy()
    assert L.egs_opacity_entropy_forward(-1, p, 0, p, None, None, C.byref(ent), None) == -1
    assert L.egs_opacity_entropy_forward(10, p, 0, p, None, None, None, None) == -1
    assert L.egs_opacity_entropy_forward(10, p, 0, p, None, None, C.byref(ent), None) == -1          # no n_vis word
    ent.n_vis = 4096
    assert L.egs_opacity_entropy_forward(10, p, 0, p, None, None, C.byref(ent), None) == -1          # no scratch
    ent.scratch = 4096
    assert L.egs_opacity_entropy_forward(10, None, 0, p, None, None, C.byref(ent), None) == -1
    assert L.egs_opacity_entropy_forward(10, p, 1, p, None, None, C.byref(ent), None) == -1          # only the opacity's activation flag
    assert L.egs_opacity_entropy_backward(10, p, 4, p, None, C.byref(ent), p, None) == -1            # no weight
    ent.weight = 4096
    assert L.egs_opacity_entropy_backward(10, p, 4, p, None, C.byref(ent), None, None) == -1
    assert L.egs_opacity_entropy_backward(0, None, 4, None, None, C.byref(ent), None, None) == 0
    args = lambda lg, e, gcol: (10, 0, 1, 0, p, p, p, None, None, p, 1.0, p, None, 0, p, p, p, 64, 64, 1.0, 1.0, p, p, None, p, lg, e, gcol, None, None,
                                p, p, p, p, None, p, None, p, p, None, None, None, None, None, 0, None, 0, p, None, 0)
    lg = lib.LossGrad()
    assert L.egs_backward_entropy_lossgrad(*args(None, None, p)) == -1                               # the struct is what the entry point is for
    assert L.egs_backward_entropy_lossgrad(*args(C.byref(lg), C.byref(ent), p)) == -2                # the blend forms the image gradient: no dL_dout_*
    bad = lib.OpacityEntropy(); bad.n_vis, bad.scratch = 4096, 4096
    assert L.egs_backward_entropy_lossgrad(*args(None, C.byref(bad), p)) == -1                       # no weight
    a8 = list(args(None, C.byref(ent), p)); a8[13] = 8                                               # EGS_ACT_OBJECT_MOTION
    assert L.egs_backward_entropy_lossgrad(*a8) == -2
