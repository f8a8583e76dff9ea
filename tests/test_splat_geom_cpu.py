"""CPU: the per-Gaussian geometry of preprocess.hip and cov3d.hip (egogaussian_amd/csrc/splat_geom.h) -- the very header the kernels include,
compiled by the host compiler into a small program (tests/splat_geom_host.cpp).  Covariance, depth and conic bit for bit against the float32
oracle; the covariance chain, forward and backward, against float64 at the bars tests/test_gpu_anchor_covariance.py holds the kernel to."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import anchors as A
from tests.common import make_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("plain", "modifier", "selection", "rot_matrix")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("splat_geom") / "splat_geom_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "splat_geom_host.cpp"), "-o", exe])
    return exe


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _run(host, tmp_path, mode, arrays, n_out, *args):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]).tofile(src)
    subprocess.run([host, mode, src, dst] + [str(a) for a in args], check=True)
    out = np.fromfile(dst, dtype=np.float32)
    assert out.size == n_out
    return out


# ---- 1. bit identity with the float32 oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("modifier", [1.0, A.COV_MODIFIER])
def test_covariance_depth_and_conic_have_the_oracles_bits(host, tmp_path, modifier):
    """S(400, 48, 64) with scales and rotations given and no activation flag (no expf anywhere; sqrtf is not reached): on every visible row the
    header's six covariance entries, its camera-space depth, and the conic formed from its (a, b, c) by the oracle's three expressions in
    float32 are the oracle's, bit for bit."""
    from oracle.oracle import Oracle
    N, H, W = 400, 48, 64
    inp = make_inputs(N, H, W, seed=0, mode="col_sr")
    inp["scale_modifier"] = modifier
    st = Oracle(np.float32).forward(**inp, stop_after="preprocess")
    vis = st["radii"] > 0
    assert vis.sum() >= 100, f"only {int(vis.sum())} visible rows"
    out = _run(host, tmp_path, "project", [inp["means3D"].numpy(), inp["scales"].numpy(), inp["rotations"].numpy(), inp["viewmatrix"].numpy()], 10 * N,
               N, W, H, _bits(inp["tanfovx"]), _bits(inp["tanfovy"]), _bits(modifier))
    cov, depth, abc = out[:6 * N].reshape(N, 6), out[6 * N:7 * N], out[7 * N:].reshape(N, 3)
    a, b, c = abc[vis, 0], abc[vis, 1], abc[vis, 2]
    with np.errstate(all="ignore"):
        det = a * c - b * b                                           # float32 arrays: every operation rounds once, as the oracle's does
        det_inv = np.float32(1.0) / det
        conic = np.stack([c * det_inv, -b * det_inv, a * det_inv], axis=1)
    assert conic.dtype == np.float32
    print(f"modifier {modifier}: {int(vis.sum())} of {N} rows visible")
    assert A.same_bits(cov[vis], st["cov3D"][vis]), "covariance"
    assert A.same_bits(depth[vis], st["depths"][vis]), "depth"
    assert A.same_bits(conic, st["conic_opacity"][vis, :3]), "conic"


# ---- 2. the chain against float64, at the GPU test's bars ----------------------------------------------------------------------------
def _chain(host, tmp_path, variant, inp, is_object=None):
    """The variant through the header the way fused.py + k_cov3d_* run it -> the dict A.cov_eval gives."""
    from egogaussian_amd.fused import object_selection
    N = inp["N"]
    mod = A.COV_MODIFIER if variant == "modifier" else 1.0
    arrays, M, sel, mult = [inp["raw"].numpy(), inp["quat"].numpy(), inp["w"].numpy()], None, None, 1.0
    if variant in ("selection", "rot_matrix"):
        M = inp["A"].float()
        if variant == "rot_matrix":
            M = inp["Rt"].float() @ M
        sel, mult = object_selection(inp["is_object"] if is_object is None else is_object, 1, N)
        arrays += [M.numpy(), sel.numpy().astype(np.float32)]
    out = _run(host, tmp_path, "chain", arrays, 22 * N, N, 1, _bits(mod), _bits(float(mult)), int(M is not None), int(sel is not None))
    sub = dict(cov=out[:6 * N].reshape(N, 6), opacity=None, d_raw=out[6 * N:9 * N].reshape(N, 3), d_quat=out[9 * N:13 * N].reshape(N, 4), d_opac=None, dM=None)
    if variant == "rot_matrix":                                       # dL/dM: the rows' terms summed in float64; M = Rt A, so dL/dRt = dL/dM A^T
        dM = out[13 * N:].reshape(N, 3, 3).astype(np.float64).sum(0)
        sub["dM"] = (dM @ inp["A"].double().numpy().T).astype(np.float32)
    return sub


@functools.lru_cache(maxsize=None)
def _ref(family, variant, dtype):
    return A.cov_eval(variant, A.cov_inputs(family), "torch", dtype=dtype, terms=dtype == torch.float64)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("family", A.COV_FAMILIES)
def test_chain_values_and_gradient_rows_against_float64(host, tmp_path, family, variant):
    sub = _chain(host, tmp_path, variant, A.cov_inputs(family))
    ref, yard = _ref(family, variant, torch.float64), _ref(family, variant, torch.float32)
    what = f"{family} {variant}"
    fv = A.check_cov_values(sub, ref, what=what)
    fg = A.check_cov_grad_rows(sub, yard, ref, what=what)
    print(f"ANCHOR header cov values {what}: worst row {fv['cov']:.2e} (bar {A.COV_VALUE_BAR:g}); "
          + "; ".join(f"{n} q50 {f['q50'][0]:.2e} ({f['q50'][1]:.2e}) max {f['max'][0]:.2e} ({f['max'][1]:.2e})" for n, f in fg.items()))
    if variant == "rot_matrix":
        fm = A.check_cov_dM(sub, yard, ref, what=what)
        print(f"ANCHOR header cov dM {what}: {fm['dM_in_u_terms']:.2f} u sum|terms| (torch float32 {fm['yard_in_u_terms']:.2f}; floor 8)")


@pytest.mark.parametrize("zero_selected", [False, True])
def test_chain_row_zero_gradient_multiplier(host, tmp_path, zero_selected):
    """The reference's duplicated-index quirk as tests/test_gpu_anchor_covariance.py sets it up: N = 64, rows 3, 17, 40 selected, row 0 selected
    or not; every row within the project's 1e-4 of its own magnitude, or 3 x the float32 torch form's distance."""
    N = 64
    inp = A.cov_head(A.cov_inputs("bench"), N)
    io = torch.zeros(N, 1)
    io[[3, 17, 40]] = 1.0
    io[0] = 1.0 if zero_selected else 0.0
    for variant in ("selection", "rot_matrix"):
        sub = _chain(host, tmp_path, variant, inp, is_object=io)
        ref, yard = A.cov_eval(variant, inp, "torch", dtype=torch.float64, is_object=io, terms=True), A.cov_eval(variant, inp, "torch", is_object=io)
        A.check_cov_values(sub, ref, what=f"row-0 quirk {variant}")
        rows = np.arange(N)
        for name in ("d_raw", "d_quat"):
            e_s, e_y = A.row_errors(sub[name], ref[name], rows), A.row_errors(yard[name], ref[name], rows)
            assert (e_s <= np.maximum(1e-4, 3.0 * e_y)).all(), f"{variant} {name}: rows {np.nonzero(e_s > np.maximum(1e-4, 3.0 * e_y))[0].tolist()} (row 0: {e_s[0]:.2e}, float32 torch form {e_y[0]:.2e})"
            print(f"ANCHOR header cov row-0 multiplier {variant} zero_selected={zero_selected} {name}: row 0 {e_s[0]:.2e} ({e_y[0]:.2e})")
        if variant == "rot_matrix":
            A.check_cov_dM(sub, yard, ref, what="row-0 quirk")
