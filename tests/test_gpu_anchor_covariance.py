"""GPU: the covariance producer (cov3d.hip) against covariance.py evaluated in float64 on the CPU, with the same functions in float32 on the
CPU as the yardstick -- the producer whose arithmetic (csrc/splat_geom.h) the preprocess's raw-parameter mode and the in-rasterizer object
rotation run too, and are each asserted equal to.  Values per row, gradients per row against the row's own magnitude, the dM reduction, block edges.  Figures: profiles/anchor_parity.md."""
import functools

import numpy as np
import pytest
import torch

from tests import anchors as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _ref(family, variant, dtype, N=4096):
    return A.cov_eval(variant, A.cov_inputs(family, N), "torch", dtype=dtype, terms=dtype == torch.float64)


@pytest.mark.parametrize("variant", A.COV_VARIANTS)
@pytest.mark.parametrize("family", A.COV_FAMILIES)
def test_values_and_gradient_rows_against_float64(family, variant):
    sub = A.cov_eval(variant, A.cov_inputs(family), "fused", device=DEV)
    ref, yard = _ref(family, variant, torch.float64), _ref(family, variant, torch.float32)
    what = f"{family} {variant}"
    fv = A.check_cov_values(sub, ref, what=what)
    yv = A.check_cov_values(yard, ref, what=what + " (float32 torch form)")
    print(f"ANCHOR cov values {what}: worst row {fv['cov']:.2e} (torch float32 {yv['cov']:.2e}; bar {A.COV_VALUE_BAR:g})"
          + (f", sigmoid {fv['sigmoid'] / A.U:.2f}u ({yv['sigmoid'] / A.U:.2f}u; bar 4u)" if "sigmoid" in fv else ""))
    fg = A.check_cov_grad_rows(sub, yard, ref, what=what)
    for name, f in fg.items():
        print(f"ANCHOR cov rows {what} {name}: q50 {f['q50'][0]:.2e} ({f['q50'][1]:.2e}), q90 {f['q90'][0]:.2e} ({f['q90'][1]:.2e}), rows > 1e-3 {f['tails'][0][0]} ({f['tails'][1][0]}), "
              f"> 1e-2 {f['tails'][0][1]} ({f['tails'][1][1]}), max {f['max'][0]:.2e} ({f['max'][1]:.2e})")
    if variant == "rot_matrix":
        fm = A.check_cov_dM(sub, yard, ref, what=what)
        print(f"ANCHOR cov dM {what}: {fm['dM_in_u_terms']:.2f} u sum|terms| (torch float32 {fm['yard_in_u_terms']:.2f}; floor 8)")


@functools.lru_cache(maxsize=None)
def _big(variant):
    return A.cov_eval(variant, A.cov_inputs("bench"), "fused", device=DEV)


@pytest.mark.parametrize("variant", ["opacity", "rot_matrix"])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_counts_at_the_block_edge(N, variant):
    """A row's result does not depend on how many rows there are: the first N rows alone must give, bit for bit, the rows the 4 096-row
    launch gives (which test_values_and_gradient_rows_against_float64 holds to float64) -- and are held to the value bar themselves.  The
    dM sum does depend on N and answers to float64."""
    inp = A.cov_head(A.cov_inputs("bench"), N)
    sub, big = A.cov_eval(variant, inp, "fused", device=DEV), _big(variant)
    ref = A.cov_eval(variant, inp, "torch", dtype=torch.float64, terms=True)
    A.check_cov_values(sub, ref, what=f"N = {N} {variant}")
    for name in ("cov", "opacity", "d_raw", "d_quat", "d_opac"):
        if sub[name] is not None:
            assert sub[name].shape[0] == N and A.same_bits(sub[name], big[name][:N]), f"N = {N} {variant}: {name} differs from the rows of the 4 096-row launch"
    if variant == "rot_matrix":
        fm = A.check_cov_dM(sub, A.cov_eval(variant, inp, "torch"), ref, what=f"N = {N}")
        print(f"ANCHOR cov dM N = {N}: {fm['dM_in_u_terms']:.2f} u sum|terms| (torch float32 {fm['yard_in_u_terms']:.2f}; floor 8)")


def test_dM_over_more_partial_sums_than_the_finish_kernel_has_threads():
    """N = 262 145: 1 025 workgroup partials, one more than k_cov3d_dm_finish's 1 024 threads take in their first pass."""
    inp = A.cov_inputs("bench", N=262145)
    sub = A.cov_eval("rot_matrix", inp, "fused", device=DEV)
    ref, yard = A.cov_eval("rot_matrix", inp, "torch", dtype=torch.float64, terms=True), A.cov_eval("rot_matrix", inp, "torch")
    fm = A.check_cov_dM(sub, yard, ref, what="N = 262145")
    print(f"ANCHOR cov dM N = 262145: {fm['dM_in_u_terms']:.2f} u sum|terms| (torch float32 {fm['yard_in_u_terms']:.2f}; floor 8)")
    A.check_cov_values(sub, ref, what="N = 262145")
    fg = A.check_cov_grad_rows(sub, yard, ref, what="N = 262145")
    # the last row sits alone in the last workgroup: the project's 1e-4 of its own magnitude, or 3 x the float32 torch form's distance
    last = np.array([262144])
    for name in ("d_raw", "d_quat"):
        assert A.row_errors(sub[name], ref[name], last)[0] <= max(1e-4, 3.0 * A.row_errors(yard[name], ref[name], last)[0]), name
        print(f"ANCHOR cov rows N = 262145 {name}: q50 {fg[name]['q50'][0]:.2e} ({fg[name]['q50'][1]:.2e}), q90 {fg[name]['q90'][0]:.2e} ({fg[name]['q90'][1]:.2e})")


@pytest.mark.parametrize("zero_selected", [False, True])
def test_row_zero_gradient_multiplier_of_the_duplicated_index(zero_selected):
    """The reference's [N,1]-index quirk (covariance.py): Gaussian 0 is rotated whenever any Gaussian is selected and receives its gradient
    once per selected Gaussian (once more if it is selected itself).  Three or four selected rows: a multiplier off by one is off by 20 % or
    more.  Row 0 against float64: within the project's 1e-4 of its own magnitude, or 3 x the float32 torch form's distance."""
    N = 64
    inp = A.cov_head(A.cov_inputs("bench"), N)
    io = torch.zeros(N, 1)
    io[[3, 17, 40]] = 1.0
    io[0] = 1.0 if zero_selected else 0.0
    for variant in ("selection", "rot_matrix"):
        sub = A.cov_eval(variant, inp, "fused", device=DEV, is_object=io)
        ref, yard = A.cov_eval(variant, inp, "torch", dtype=torch.float64, is_object=io, terms=True), A.cov_eval(variant, inp, "torch", is_object=io)
        # what the float64 reference does to row 0 is what the docstring says: the gradient of a plainly selected row 0, times the count
        io1 = io.reshape(-1).clone(); io1[0] = 1.0
        one_d = A.cov_eval(variant, inp, "torch", dtype=torch.float64, is_object=io1)
        mult = 5.0 if zero_selected else 3.0
        assert np.allclose(ref["d_raw"][0], mult * one_d["d_raw"][0], rtol=1e-9) and np.allclose(ref["d_quat"][0], mult * one_d["d_quat"][0], rtol=1e-9)
        A.check_cov_values(sub, ref, what=f"row-0 quirk {variant}")
        rows = np.arange(N)
        for name in ("d_raw", "d_quat"):
            e_s, e_y = A.row_errors(sub[name], ref[name], rows), A.row_errors(yard[name], ref[name], rows)
            assert (e_s <= np.maximum(1e-4, 3.0 * e_y)).all(), f"{variant} {name}: rows {np.nonzero(e_s > np.maximum(1e-4, 3.0 * e_y))[0].tolist()} (row 0: {e_s[0]:.2e}, float32 torch form {e_y[0]:.2e})"
            print(f"ANCHOR cov row-0 multiplier {variant} zero_selected={zero_selected} {name}: row 0 {e_s[0]:.2e} ({e_y[0]:.2e})")
        if variant == "rot_matrix":
            A.check_cov_dM(sub, yard, ref, what="row-0 quirk")
