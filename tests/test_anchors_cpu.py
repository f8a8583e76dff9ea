"""CPU: the anchor harness itself (tests/anchors.py) -- the float64 references against independent float64 forms, the float32 yardsticks
and the float32 emulation of Adam against the bars the GPU tests hold the kernels to, and deliberately wrong variants that every check has
to catch.  Runs no GPU code."""
import functools

import numpy as np
import pytest
import torch

from tests import anchors as A


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", sorted(A.ADAM_REGIMES))
def test_adam_emulation_stays_under_half_of_the_single_step_bars(regime):
    case = A.adam_case(regime)
    p, m, v = A.adam32(np.zeros(case["n"], np.float32), case["g"], case["m"], case["v"], case["step"], case["lr"])
    fig = A.check_adam_step(p, m, v, case, frac=0.5, what=regime)
    print(f"{regime}: emulation worst m {fig['m']:.2f}u (bar 4u), v {fig['v']:.2f}u (4u), p {fig['p']:.2f}u (16u)")
    z = (case["g"] == 0) & (case["m"] == 0) & (case["v"] == 0)
    assert A.same_bits(p[z], np.zeros(int(z.sum()), np.float32))


@pytest.mark.parametrize("fault,regime", [("no_bias_correction", "ordinary"), ("b2_for_one_minus_b2", "ordinary"), ("eps_in_sqrt", "small")])
def test_adam_single_step_check_catches_a_wrong_adam(fault, regime):
    case = A.adam_case(regime)
    p0 = np.zeros(case["n"], np.float32)
    A.check_adam_step(*A.adam32(p0, case["g"], case["m"], case["v"], case["step"], case["lr"]), case, what="unplanted")
    with pytest.raises(AssertionError):
        A.check_adam_step(*A.adam32(p0, case["g"], case["m"], case["v"], case["step"], case["lr"], fault=fault), case, what=fault)


def test_adam_distance_to_double_betas_is_the_derived_one():
    assert 1.28e-5 < A.ADAM_DOUBLE_BETA_DISTANCE < 1.30e-5
    case = A.adam_case("ordinary")
    _, _, v = A.adam32(np.zeros(case["n"], np.float32), case["g"], case["m"], case["v"], case["step"], case["lr"])
    d = A.adam_double_beta_check(v, case)
    print(f"exp_avg_sq vs Adam with double betas: {d:.3e} (derived bound {A.ADAM_DOUBLE_BETA_DISTANCE:.3e})")
    # ... and it IS that rounding, not slack in the check: a b2 two float32 steps further off is caught
    _, _, v_bad = A.adam32(np.zeros(case["n"], np.float32), case["g"], case["m"], case["v"], case["step"], case["lr"], betas=(0.9, 0.999 + 1e-7))
    with pytest.raises(AssertionError):
        A.adam_double_beta_check(v_bad, case)


@functools.lru_cache(maxsize=None)
def _trajectory(regime):
    inp = A.adam_trajectory_inputs(regime)
    ref = A.adam_trajectory64(inp)
    yard = A.adam_trajectory_stats(A.adam_trajectory_optimizer(inp, A.torch_adam32), ref, inp["sigma_g"])
    return inp, ref, yard


@pytest.mark.parametrize("regime", sorted(A.ADAM_REGIMES))
def test_adam_trajectory_emulation_against_torch_float32(regime):
    inp, ref, yard = _trajectory(regime)
    sub = A.adam_trajectory_stats(A.adam_trajectory_numpy32(inp), ref, inp["sigma_g"])
    print(f"{regime}: emulation (torch float32): " + A.check_adam_trajectory(sub, yard, what=regime))


@pytest.mark.parametrize("fault,regime", [("no_bias_correction", "first"), ("b2_for_one_minus_b2", "ordinary"), ("eps_in_sqrt", "small")])
def test_adam_trajectory_check_catches_a_wrong_adam(fault, regime):
    inp, ref, yard = _trajectory(regime)
    with pytest.raises(AssertionError):
        A.check_adam_trajectory(A.adam_trajectory_stats(A.adam_trajectory_numpy32(inp, fault=fault), ref, inp["sigma_g"]), yard, what=fault)


# ---- covariance producer ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cov(family, variant, dtype):
    return A.cov_eval(variant, A.cov_inputs(family), "torch", dtype=dtype, terms=dtype == torch.float64)


@pytest.mark.parametrize("family", A.COV_FAMILIES)
def test_covariance_float32_form_meets_the_value_bar(family):
    """The value bar is the float32 torch form's worst row over the families x ROW_Q_FACTOR: the form itself has to pass it with that room."""
    for variant in A.COV_VARIANTS:
        fig = A.check_cov_values(_cov(family, variant, torch.float32), _cov(family, variant, torch.float64), what=f"{family} {variant}")
        assert fig["cov"] <= A.COV_VALUE_BAR / 2.0, (family, variant, fig)
        print(f"{family} {variant}: float32 torch form, worst row {fig['cov']:.2e}" + (f", sigmoid {fig['sigmoid'] / A.U:.2f}u" if "sigmoid" in fig else ""))


@pytest.mark.parametrize("family", A.COV_FAMILIES)
def test_covariance_numpy_form_agrees_with_covariance_py_in_float64(family):
    inp = A.cov_inputs(family)
    for variant, mod in (("plain", 1.0), ("modifier", A.COV_MODIFIER)):
        ref = _cov(family, variant, torch.float64)
        cov, d_raw, d_quat = A.cov_numpy64(inp["raw"].numpy(), inp["quat"].numpy(), mod, inp["w"].numpy())
        rows = np.arange(inp["N"])
        assert A.row_errors(cov, ref["cov"], rows).max() < 1e-12
        assert A.row_errors(d_raw, ref["d_raw"], rows).max() < 1e-9 and A.row_errors(d_quat, ref["d_quat"], rows).max() < 1e-6
        sub = dict(cov=cov, d_raw=d_raw, d_quat=d_quat)
        A.check_cov_values(sub, ref | {"opacity": None}, what=family)
        A.check_cov_grad_rows(sub, _cov(family, variant, torch.float32), ref, what=family)


def test_covariance_checks_catch_a_wrong_covariance():
    inp = A.cov_inputs("bench")
    ref, yard = _cov("bench", "modifier", torch.float64), _cov("bench", "modifier", torch.float32)
    run = lambda fault: dict(zip(("cov", "d_raw", "d_quat"), A.cov_numpy64(inp["raw"].numpy(), inp["quat"].numpy(), A.COV_MODIFIER, inp["w"].numpy(), fault=fault)))
    good = run(None)
    A.check_cov_values(good, ref | {"opacity": None}); A.check_cov_grad_rows(good, yard, ref)
    with pytest.raises(AssertionError):
        A.check_cov_values(run("modifier_not_squared"), ref | {"opacity": None})
    with pytest.raises(AssertionError):
        A.check_cov_grad_rows(run("unsymmetrised_gradient"), yard, ref)
    A.check_cov_values(run("unsymmetrised_gradient"), ref | {"opacity": None})           # (that fault is in the backward only)


def test_covariance_dM_check():
    ref, yard = _cov("bench", "rot_matrix", torch.float64), _cov("bench", "rot_matrix", torch.float32)
    fig = A.check_cov_dM(yard, yard, ref)
    print(f"float32 torch form: dM within {fig['yard_in_u_terms']:.2f} u sum|terms| of float64")
    assert fig["yard_in_u_terms"] < 8.0          # the floor (8u sum|terms|) is above what the float32 form loses
    with pytest.raises(AssertionError):
        A.check_cov_dM(yard | {"dM": yard["dM"] * np.float32(1.001)}, yard, ref)


# ---- image loss -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", A.LOSS_SHAPES)
def test_loss_numpy_form_agrees_with_training_loss_in_float64(C, H, W):
    img, gt, gate = A.loss_inputs(C, H, W)
    for lam in A.LOSS_LAMBDAS:
        for gt_gate in (None, gate):
            ref64, ref32 = A.loss_reference(img, gt, lam, gt_gate, torch.float64), A.loss_reference(img, gt, lam, gt_gate, torch.float32)
            l, g = A.loss_numpy64(img.numpy(), gt.numpy(), lam, None if gt_gate is None else gt_gate.numpy())
            assert abs(l - ref64[0]) < 1e-12 and np.abs(g - ref64[1]).max() <= 1e-10 * np.abs(ref64[1]).max()
            fig = A.check_loss(l, g, ref64, ref32, gt_gate, what=f"{(C, H, W)} lambda {lam}")
            print(f"{(C, H, W)} lambda {lam} gate {gt_gate is not None}: float32 torch form value {fig['value_yard']:.1e}, gradient max {fig['max'][1]:.2e}, "
                  f"q99 {fig['q99'][1]:.2e}, seams {fig['seam'][1]:.2e}, border {fig['border'][1]:.2e}")


def test_loss_check_catches_a_dropped_tap_at_a_strip_seam():
    C, H, W = 1, 30, 108
    img, gt, _ = A.loss_inputs(C, H, W)
    for lam in A.LOSS_LAMBDAS:
        ref64, ref32 = A.loss_reference(img, gt, lam, None, torch.float64), A.loss_reference(img, gt, lam, None, torch.float32)
        A.check_loss(*A.loss_numpy64(img.numpy(), gt.numpy(), lam), ref64, ref32)
        for tap in (0, 4):                                            # the outermost tap (weight 1e-3) and one next to the centre
            with pytest.raises(AssertionError):
                A.check_loss(*A.loss_numpy64(img.numpy(), gt.numpy(), lam, drop=(54, tap)), ref64, ref32)


def test_loss_zones():
    seam, border = A.loss_zones(30, 108)
    assert seam[:, 49:59].all() and not seam[7, :49].any() and not seam[7, 59:].any()          # one vertical seam between columns 53 and 54
    assert seam[10:20].all() and not seam[:10, :49].any() and not seam[20:, :49].any()        # one horizontal seam between rows 14 and 15
    assert border[:5].all() and border[:, :5].all() and border[-5:].all() and border[:, -5:].all() and not border[5:-5, 5:-5].any()
    seam, border = A.loss_zones(1, 1)
    assert not seam.any() and border.all()


# ---- two-value loss ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(shape, u, dtype, gated=False, fault=None):
    img, gt, gate = A.pair_inputs(*shape)
    return A.pair_reference(img, gt, u, dtype, gate if gated else None, fault)


@pytest.mark.parametrize("C,H,W", A.LOSS_SHAPES)
def test_pair_float32_form_passes_the_pair_check(C, H, W):
    """The float32 CPU form is its own yardstick in the mixed rule (factor 1 <= 3); what this shows is that it meets the fixed bars -- 1e-4, and
    with SSIM switched off 2^-22 of each element and exact zeros on the ties -- with and without the gate."""
    gate = A.pair_inputs(C, H, W)[2].numpy()
    for u in A.PAIR_UPSTREAMS:
        for gated in (False, True):
            ref64, ref32 = _pair((C, H, W), u, torch.float64, gated), _pair((C, H, W), u, torch.float32, gated)
            fig = A.check_pair(ref32[:2], ref32[2], ref64, ref32, u, gate if gated else None, what=f"{(C, H, W)} u {u} gate {gated}")
            if u[1] != 0:
                print(f"{(C, H, W)} u {u} gate {gated}: float32 torch form values {fig['values_yard'][0]:.1e} {fig['values_yard'][1]:.1e}, gradient max {fig['max'][1]:.2e}, "
                      f"q99 {fig['q99'][1]:.2e}, seams {fig['seam'][1]:.2e}, border {fig['border'][1]:.2e}, ties {fig['tie'][1]:.2e}")
            else:
                print(f"{(C, H, W)} u {u} gate {gated}: float32 torch form, L1 term alone: {fig['l1_only'][1] / A.U:.2f} u of each element")


def test_pair_inputs_hold_the_tie_block():
    for C, H, W in A.LOSS_SHAPES:
        img, gt, _ = A.pair_inputs(C, H, W)
        tie = (img == gt).numpy()
        assert np.array_equal(tie, A.pair_tie_mask(C, H, W)) and bool(tie.any()) == (H >= 11 and W >= 11)      # (11 x 11 clips the block to 4 x 4)


def _fault_applies(fault, shape, u):
    """Whether the wrong form changes the float64 gradient at all -- found by evaluating it in float64."""
    return not np.array_equal(_pair(shape, u, torch.float64, False, fault)[2], _pair(shape, u, torch.float64)[2])


@pytest.mark.parametrize("fault", A.PAIR_FAULTS)
def test_pair_check_rejects_a_wrong_pair_gradient(fault):
    """Each wrong float32 form is refused at every shape and upstream pair at which the same wrong form, in float64, differs from the right
    float64 gradient.  That set is DERIVED (_fault_applies); what it has to come out as is stated here and compared: swapped upstreams change
    every pair of PAIR_UPSTREAMS (none has u0 == u1); a flipped SSIM sign those with u1 != 0; an SSIM upstream taken as 1 those with
    u1 != 1; sign(0) = +1 those with u0 != 0, at the shapes that have ties."""
    expected = {"upstreams_swapped": lambda s, u: u[0] != u[1], "ssim_sign_flipped": lambda s, u: u[1] != 0, "ssim_upstream_one": lambda s, u: u[1] != 1,
                "tie_sign_plus_one": lambda s, u: u[0] != 0 and s[1] >= 11 and s[2] >= 11}[fault]
    rejected = 0
    for shape in A.LOSS_SHAPES:
        for u in A.PAIR_UPSTREAMS:
            applies = _fault_applies(fault, shape, u)
            assert applies == expected(shape, u), (fault, shape, u)
            if not applies:
                continue
            ref64, ref32, wrong = _pair(shape, u, torch.float64), _pair(shape, u, torch.float32), _pair(shape, u, torch.float32, False, fault)
            with pytest.raises(AssertionError):
                A.check_pair(wrong[:2], wrong[2], ref64, ref32, u, what=f"{fault} {shape} {u}")
            d = np.abs(wrong[2] - ref64[2]).max() / np.abs(ref64[2]).max()
            print(f"{fault} {shape} u {u}: {d:.2e} of max|g64| away")
            rejected += 1
    assert rejected > 0
