"""GPU: the launch geometry of the Adam steps taken inside other launches -- k_preprocess_backward<SINK> (csrc/preprocess.hip) and
sh16_adam_span / k_sh16_backward<SPLIT, SINK> (csrc/sh.hip): tails of 1 - 3 elements, tasks with nothing to do, leaves whose parameter or
moments are not 16-byte aligned, the live-row word at and around every edge, workgroups without a visible row.  tests/sink_cases.py
models which branch every task takes and tests/test_sink_cases_cpu.py asserts that the row counts used here reach every one of them.

Every comparison is torch.equal -- there is no tolerance to choose.  That is a statement about correctness and not only about agreement
because of a chain: the stand-alone kernel (adam.hip k_adam) is itself held to Adam in float64 by tests/test_gpu_anchor_adam.py, over its
own launch geometry as well; a fused step that leaves the same bits as that kernel fed the same gradient bits is therefore as close to
float64 as the anchor proves.  The gradients are the same bits in every run of one case because all of them run under the deterministic
backward (_C.deterministic_backward, tests/test_gpu_deterministic.py).

The optimizer state is seeded before the step as tests/test_gpu_anchor_adam.py::_one_step does (step count 6, exp_avg ~ 1e-3 N(0,1),
exp_avg_sq ~ 1e-6 U(0,1)): with non-zero moments every stepped element moves whatever its gradient, so a row that was skipped shows.
Every parameter and both its moments live between eight sentinel floats on either side: a tail that wrote past the last row shows too."""
import functools
import math
import types

import pytest
import torch

from tests import sink_cases as S
from tests.test_gpu_fused_adam import _groups

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 48, 64
FRAME = 5                                                              # make_camera(FRAME, ...): a few degrees off the world frame
SENTINEL, PAD = 7.0, 8
STEP0 = 6.0
LEAVES = {0: ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"),
          3: ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation", "_features_rest")}
SINK_ID = {"_xyz": 0, "_opacity": 1, "_scaling": 2, "_rotation": 3, "_features_dc": 4, "_features_rest": 5}      # EGS_SINK_*
SH_LAUNCH = ("_xyz", "_features_dc", "_features_rest")               # degree 3, split: stepped by the spherical-harmonics launch
KEYS = ("param", "exp_avg", "exp_avg_sq")


@pytest.fixture(autouse=True)
def _deterministic_backward():
    from egogaussian_amd import _C
    old = _C.deterministic_backward(True)
    yield
    _C.deterministic_backward(old)


@functools.lru_cache(maxsize=None)
def _case(P, degree, behind=False):
    """The student scene, camera, target image (rendered from the unperturbed scene) and seeded moments of one case; never modified.
    behind: rows 256 .. 511 lie behind the camera.  P = 515: the last row is a large opaque splat in the middle of the frame (its gradient
    is non-zero in every leaf -- the live-row tests need a row beyond the live count that would move if it were stepped)."""
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    scene = make_scene(P, H, W, 100 + P, sh_degree=degree)
    scene["log_scale"] += math.log(2.0)
    if P == 515:
        scene["xyz"][-1] = (0.1, -0.05, 4.0)
        scene["log_scale"][-1] = (math.log(0.2), math.log(0.1), math.log(0.15))
        scene["opacity_logit"][-1] = 1.0
    if behind:
        scene["xyz"][256:512, 2] = -5.0
    cam = make_camera(FRAME, H, W, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        target = render(cam, SynthGaussians(scene, device=DEV, sh_degree=degree, requires_grad=False), Pipe, bg)["render"].clone()
    student = perturb_student(scene)
    gen = torch.Generator().manual_seed(7000 + P)
    shapes = {"_xyz": (P, 3), "_features_dc": (P, 1, 3), "_opacity": (P, 1), "_scaling": (P, 3), "_rotation": (P, 4), "_features_rest": (P, 15, 3)}
    moments = {a: (1e-3 * torch.randn(shapes[a], generator=gen), 1e-6 * torch.rand(shapes[a], generator=gen)) for a in LEAVES[degree]}
    return student, cam, target, bg, moments


def _boxed(values, shift_bytes=0):
    """-> (buffer, view): `values` as a contiguous view that starts PAD floats + shift_bytes into a buffer of sentinels."""
    off = PAD + shift_bytes // 4
    n = values.numel()
    buf = torch.full((off + n + PAD,), SENTINEL, device=DEV)
    buf[off:off + n] = values.reshape(-1).to(DEV)
    view = buf[off:off + n].view(values.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == shift_bytes % 16
    return buf, view


def _run(P, degree, keep, active=None, shift=None, behind=False):
    """One forward, backward with the optimizer inside, and optimizer.step() of a fresh model.  keep: the sink also writes the owned
    leaves' gradients.  active: value of the live-row word (capacity P).  shift: (leaf, "param" | "exp_avg" | "exp_avg_sq", bytes) -- that
    one array starts so many bytes off a 16-byte boundary.  -> namespace(before, after: {leaf: {param, exp_avg, exp_avg_sq}}, step, grads,
    owned, radii)."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.optim import FusedAdam
    student, cam, target, bg, moments = _case(P, degree, behind)
    pc = SynthGaussians(student, device=DEV, sh_degree=degree)
    off = lambda a, key: shift[2] if shift is not None and shift[:2] == (a, key) else 0
    boxes, views = [], {}
    for a in LEAVES[degree]:
        vals = (getattr(pc, a).detach(),) + moments[a]
        views[a] = {}
        for key, val in zip(KEYS, vals):
            buf, view = _boxed(val, off(a, key))
            boxes.append((a, key, buf, view))
            views[a][key] = view
        setattr(pc, a, views[a]["param"].requires_grad_(True))
    if shift is not None:
        assert views[shift[0]][shift[1]].data_ptr() % 16 == shift[2] != 0
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    if active is not None:
        opt.active_rows = (torch.tensor([active], dtype=torch.int32, device=DEV), P)
    for a in LEAVES[degree]:
        opt.state[getattr(pc, a)] = {"step": torch.tensor(STEP0), "exp_avg": views[a]["exp_avg"], "exp_avg_sq": views[a]["exp_avg_sq"]}
    before = {a: {key: views[a][key].detach().clone() for key in KEYS} for a in LEAVES[degree]}
    real_make, made = opt.make_sink, []

    def making(**kw):
        sink = real_make(**kw)
        if sink is not None:
            sink.keep_grads = keep
        made.append(sink)
        return sink
    opt.make_sink = making
    out = render(cam, pc, Pipe, bg, optimizer=opt)
    l1_ssim_loss(out["render"], target, 0.2).backward()
    grads = {a: None if getattr(pc, a).grad is None else getattr(pc, a).grad.detach().clone() for a in LEAVES[degree]}
    opt.step()                                                        # steps what the backward left (never an owned leaf, keep or not)
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert len(made) == 1 and made[0] is not None
    for a, key, buf, view in boxes:
        o, n = view.storage_offset(), view.numel()
        assert bool((buf[:o] == SENTINEL).all()) and bool((buf[o + n:] == SENTINEL).all()), f"{a} {key}: the step wrote outside the array"
    after = {a: {key: views[a][key].detach().clone() for key in KEYS} for a in LEAVES[degree]}
    step = {a: float(opt.state[getattr(pc, a)]["step"]) for a in LEAVES[degree]}
    return types.SimpleNamespace(before=before, after=after, step=step, grads=grads, owned=set(made[0].owned), radii=out["radii"].clone())


def _twin(P, degree, res, active=None):
    """The stand-alone kernel on copies of what `res` started from, fed the gradients its backward wrote -> (after, step) as in _run."""
    from egogaussian_amd.optim import FusedAdam
    pc = types.SimpleNamespace(_features_rest=torch.empty(P, 0, 3, device=DEV))
    for a in LEAVES[degree]:
        p = res.before[a]["param"].clone().requires_grad_(True)
        p.grad = res.grads[a].clone()
        setattr(pc, a, p)
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    if active is not None:
        opt.active_rows = (torch.tensor([active], dtype=torch.int32, device=DEV), P)
    for a in LEAVES[degree]:
        opt.state[getattr(pc, a)] = {"step": torch.tensor(STEP0), "exp_avg": res.before[a]["exp_avg"].clone(), "exp_avg_sq": res.before[a]["exp_avg_sq"].clone()}
    opt.step()
    torch.cuda.synchronize()
    after = {a: {"param": getattr(pc, a).detach(), "exp_avg": opt.state[getattr(pc, a)]["exp_avg"], "exp_avg_sq": opt.state[getattr(pc, a)]["exp_avg_sq"]}
             for a in LEAVES[degree]}
    return after, {a: float(opt.state[getattr(pc, a)]["step"]) for a in LEAVES[degree]}


def _assert_same(got, want, leaves, what):
    for a in leaves:
        for key in KEYS:
            x, y = got[a][key], want[a][key]
            assert x.shape == y.shape and torch.equal(x, y), f"{what}: {a} {key} differs in {int((x != y).sum())} of {x.numel()} elements"


def _all_owned(degree):
    return {SINK_ID[a] for a in LEAVES[degree]}


def _rows_changed(res, a, key):
    """[P] bool: every element of the row differs from what it was before the step."""
    x, y = res.after[a][key], res.before[a][key]
    return (x != y).reshape(x.shape[0], -1).all(dim=1)


def _against_twin(P, degree, res, active=None, what=""):
    assert res.owned == _all_owned(degree)
    for a in LEAVES[degree]:
        assert res.grads[a] is not None, f"{a}: keep_grads writes the gradient as well"
        assert P < 255 or float(res.grads[a].abs().max()) > 0, f"{a}: an all-zero gradient"
    twin, twin_step = _twin(P, degree, res, active)
    _assert_same(res.after, twin, LEAVES[degree], f"{what}fused against stand-alone step")
    assert res.step == twin_step
    return twin_step


# ---- a. every row count ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("P", S.ROW_COUNTS)
def test_every_row_count_is_the_standalone_step_bit_for_bit(P, degree):
    """Degree 0: all five leaves are stepped by the preprocess backward; degree 3, split: features_dc, features_rest and the positions
    by the spherical-harmonics launch, the other three by the preprocess backward."""
    print("\n" + S.describe(P))
    res = _run(P, degree, keep=True)
    steps = _against_twin(P, degree, res)
    assert all(s == STEP0 + 1 for s in steps.values())
    for a in LEAVES[degree]:
        assert bool(_rows_changed(res, a, "exp_avg").all()), f"{a}: a row was not stepped (moments decay whatever the gradient)"
    plain = _run(P, degree, keep=False)                               # the default use: no gradient arrays at all
    assert plain.owned == _all_owned(degree) and all(g is None for g in plain.grads.values())
    _assert_same(plain.after, res.after, LEAVES[degree], "without gradient arrays against with them")
    assert plain.step == res.step
    if P >= 255:
        vis = res.radii > 0
        assert bool(vis.any()) and bool((~vis).any()), "the case is meant to hold culled and visible rows"
        for a in LEAVES[degree]:                                      # a culled row's gradient is exactly zero -- and it still took its step
            assert float(res.grads[a][~vis].abs().max()) == 0.0


# ---- b. live-row edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("active", S.LIVE_COUNTS)
def test_live_row_word_at_every_edge(active, degree):
    """optimizer.active_rows = (word, 515): rows at and beyond min(P, max(word, 0)) keep parameter and moments bit for bit although a
    gradient reached some of them; rows below it are all stepped.  The step count: the library counts the step whatever the word holds --
    egs_adam_tick (fused) and every workgroup of k_adam (stand-alone) advance state["step"] also when no row is live -- so for a word <= 0
    both runs end at the same count with nothing moved; the test asserts that they agree, not the value."""
    P = S.LIVE_P
    print("\n" + S.describe(P, active))
    res = _run(P, degree, keep=True, active=active)
    _against_twin(P, degree, res, active, what=f"active_rows {active}: ")
    live = S.live_rows(P, active)
    for a in LEAVES[degree]:
        for key in KEYS:
            assert torch.equal(res.after[a][key][live:], res.before[a][key][live:]), f"{a} {key}: a row at or beyond the live count was written"
        if live < P:
            assert float(res.grads[a][live:].abs().max()) > 0, f"{a}: the rows beyond the live count are meant to have a gradient"
        assert bool(_rows_changed(res, a, "exp_avg")[:live].all()), f"{a}: a live row was not stepped"


# ---- c. unaligned leaves --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _aligned(P, degree):
    return _run(P, degree, keep=False)


@pytest.mark.parametrize("P,degree,leaf", [(P, d, a) for P in S.UNALIGNED_P for d in (0, 3) for a in LEAVES[d]])
def test_unaligned_leaf_equals_the_aligned_run(P, degree, leaf):
    """The parameter, exp_avg and exp_avg_sq of one leaf in turn 4, 8 and 12 bytes off a 16-byte boundary.  A misaligned array of a leaf
    the preprocess backward steps sends its full tasks down the element-wise branch; misaligned moments of features_dc / features_rest
    at degree 3 send the whole span down it.  A misaligned features_dc / features_rest PARAMETER at degree 3 cannot be handed to the
    16-coefficient spherical-harmonics launch at all (it loads the rows as float4): by the library's conditions (include/egs_raster.h,
    egs_backward_adam: "any other colour layout: those three leaves cannot be fused") the two colour leaves and, because that launch is
    also the one that finishes their gradient, the positions are then left to optimizer.step() -- nothing else is -- and the state after
    step() must still be the aligned run's."""
    base = _aligned(P, degree)
    assert base.owned == _all_owned(degree)
    for key in KEYS:
        for nbytes in S.UNALIGNED_BYTES:
            res = _run(P, degree, keep=False, shift=(leaf, key, nbytes))
            what = f"{leaf} {key} {nbytes} bytes off"
            if degree == 3 and key == "param" and leaf in ("_features_dc", "_features_rest"):
                assert res.owned == _all_owned(degree) - {SINK_ID[a] for a in SH_LAUNCH}, what
            else:
                assert res.owned == _all_owned(degree), what
            for a in LEAVES[degree]:
                assert (res.grads[a] is None) == (SINK_ID[a] in res.owned), what
            _assert_same(res.after, base.after, LEAVES[degree], what + " against the aligned run")
            assert res.step == base.step, what


# ---- d. a workgroup without a visible row ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 3])
def test_workgroup_without_a_visible_row_still_steps(degree):
    """Rows 256 .. 511 behind the camera: workgroup 1 of the preprocess backward and blocks 4 .. 7 of the spherical-harmonics launch see
    no visible row.  Their rows take the dense step all the same, with a gradient of exactly zero."""
    P = S.LIVE_P
    res = _run(P, degree, keep=True, behind=True)
    assert not bool((res.radii[256:512] > 0).any()) and bool((res.radii[:256] > 0).any()) and bool((res.radii[512:] > 0).any())
    _against_twin(P, degree, res, what="rows 256..511 behind the camera: ")
    for a in LEAVES[degree]:
        assert float(res.grads[a][256:512].abs().max()) == 0.0, a
        assert bool(_rows_changed(res, a, "exp_avg").all()), f"{a}: a row was not stepped"
