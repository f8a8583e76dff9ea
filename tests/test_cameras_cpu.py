"""CPU: the checker pinned at the general cameras of tests/cameras.py before the GPU is compared with it.

  * the float64 C oracle against rasterize_torch autograd at every named camera, under the bars of tests/test_oracle_cpu.py;
  * proof that those cases discriminate: the autograd side fed a deliberately wrong camera (tanfovx / tanfovy exchanged, the scale
    modifier dropped, the roll dropped, the camera centre at the origin) must fail that comparison by four decades;
  * the float32 oracle against the float64 oracle on the inputs of the GPU cases: how many pixels the two disagree on and how far apart
    they are there -- the room the flip rule's caps have left before the HIP path is looked at;
  * the fuzz harness's stream of draws without its --cameras switch is what it was.
"""
import hashlib

import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from tests.cameras import CAMERAS, CAMERA_CASES, CPU_CAMERA_CASES, ANISOTROPIC, IN_CLOUD, case_id, build_camera, population, assert_population, fuzz_draw, fuzz_inputs
from tests.common import (make_inputs, seeded_grads, rel_err, state_disagreement_pixels, gaussians_contributing_to, NEAR_SHARE, ROW_EXCLUDED_CAP)
from tests.test_oracle_cpu import _run_both

PAIRS = [("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacities"), ("dL_dsh", "shs"), ("dL_dcolors_precomp", "colors_precomp"),
         ("dL_dscale", "scales"), ("dL_drot", "rotations"), ("dL_dcov3D", "cov3D_precomp")]
IMAGE_SHARE = 2e-2           # the default `share=` of tests/common.py check_images_isolating_flips


def _grad_distances(g, dd, m2d):
    """Per gradient array: max-norm relative distance of the oracle's (g) from autograd's (leaves of dd, m2d)."""
    out = {gname: rel_err(g[gname].reshape(dd[leaf].shape), dd[leaf].grad.numpy()) for gname, leaf in PAIRS if leaf in dd}
    out["dL_dmean2D"] = rel_err(g["dL_dmean2D"], m2d.grad.numpy())
    return out


@pytest.mark.parametrize("case", CPU_CAMERA_CASES, ids=case_id)
def test_c_oracle_matches_autograd_fp64_at_general_cameras(case):
    cam, N, H, W, seed, deg, mode, smul = case
    d = make_inputs(N, H, W, seed, deg, mode, scale_mul=smul, camera=cam)
    assert d["scale_modifier"] == CAMERAS[cam]["scale_modifier"] and float(d["campos"].norm()) > 5.0
    assert float(d["viewmatrix"][:3, :3].abs().min()) > 1e-3, "the view matrix is meant to have no zero entry"
    dd, m2d, (col, radii, dep, alp, aux), st, g = _run_both(d, np.float64, torch.float64)
    assert_population(cam, population(st, d))
    assert np.array_equal(st["radii"], radii.numpy())
    assert np.array_equal(st["keys"], aux["keys"]) and np.array_equal(st["point_list"], aux["point_list"].astype(np.uint32))
    assert np.array_equal(st["n_contrib"], aux["n_contrib"].numpy().astype(np.uint32))
    for a, b in ((st["color"], col), (st["depth"], dep), (st["alpha"], alp)):
        assert rel_err(a, b.detach().numpy()) < 1e-12
    for name, e in _grad_distances(g, dd, m2d).items():
        assert e < 1e-10, (name, e)


# ---- the cases discriminate -----------------------------------------------------------------------------------------------------------
def _exchange_tanfov(d, cam, H, W):
    return dict(d, tanfovx=d["tanfovy"], tanfovy=d["tanfovx"])


def _drop_modifier(d, cam, H, W):
    return dict(d, scale_modifier=1.0)


def _drop_roll(d, cam, H, W):
    c = build_camera(cam, H, W, roll=0.0)[0]
    return dict(d, viewmatrix=c.world_view_transform.clone(), projmatrix=c.full_proj_transform.clone(), campos=c.camera_center.clone())


def _campos_at_origin(d, cam, H, W):
    return dict(d, campos=torch.zeros(3))


MUTATIONS = {  # name -> (mutation, the cameras that claim the property, the mode it is read in)
    "tanfovx and tanfovy exchanged": (_exchange_tanfov, ANISOTROPIC, "sh_sr"),
    "scale_modifier replaced by 1": (_drop_modifier, [c for c in CAMERAS if CAMERAS[c]["scale_modifier"] != 1.0], "col_sr"),
    "roll dropped from the view matrix": (_drop_roll, list(CAMERAS), "col_sr"),
    "campos at the origin": (_campos_at_origin, list(CAMERAS), "sh_sr"),
}
_TRUE = {}


def _true_side(cam, mode):
    """The float64 oracle's gradients of the unmutated frame (computed once per camera and mode, never modified)."""
    if (cam, mode) not in _TRUE:
        N, H, W = (2500 if cam in IN_CLOUD else 400), 40, 56
        d = make_inputs(N, H, W, 90, 2 if mode == "sh_sr" else 0, mode, scale_mul=4.0, camera=cam)
        dd, m2d, outs, st, g = _run_both(d, np.float64, torch.float64)
        assert_population(cam, population(st, d))
        assert max(_grad_distances(g, dd, m2d).values()) < 1e-10            # the unmutated comparison passes
        _TRUE[(cam, mode)] = (d, H, W, g)
    return _TRUE[(cam, mode)]


@pytest.mark.parametrize("name,cam", [(n, c) for n, (_, cams, _) in MUTATIONS.items() for c in cams], ids=lambda v: str(v).replace(" ", "_"))
def test_a_wrong_camera_on_the_autograd_side_is_detected(name, cam):
    """The comparison of the test above with autograd fed the mutated inputs: at least one gradient must be off by more than 1e-6 of its
    array's maximum, four decades over the 1e-10 bar -- at every camera that claims the property, else the camera is no test of it."""
    mutate, _, mode = MUTATIONS[name]
    d, H, W, g = _true_side(cam, mode)
    dd, m2d, _, _, _ = _run_both(mutate(d, cam, H, W), np.float64, torch.float64)
    dist = _grad_distances(g, dd, m2d)
    assert max(dist.values()) > 1e-6, (name, cam, dist)


# ---- room under the flip rule's caps, with the reference alone ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CAMERA_CASES, ids=case_id)
def test_float32_oracle_leaves_the_flip_caps_room_at_general_cameras(case):
    """The inputs of the GPU cases through the float32 and the float64 oracle.  Where the two take different branches
    (state_disagreement_pixels) the float32 result may be a threshold-level contribution away; the GPU tests grant the HIP path
    `share` = 2e-2 on such pixels (check_images_isolating_flips) and NEAR_SHARE = 2e-3 on the gradient rows of their contributors, and
    check_grad_rows_vs_float64 excludes those contributors up to ROW_EXCLUDED_CAP of the visible rows.  The inputs are chosen so that
    the reference alone uses less than half of each: asserted, and the counts printed (profiles/camera_parity.md records them)."""
    cam, N, H, W, seed, deg, mode, smul = case
    d = make_inputs(N, H, W, seed, deg, mode, scale_mul=smul, camera=cam)
    grads = seeded_grads(H, W, seed + 10)
    o32, o64 = Oracle(np.float32, nthreads=8), Oracle(np.float64, nthreads=8)
    st32 = o32.forward(**d)
    st64 = o64.forward(**{k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()})
    pop = population(st32, d)
    assert_population(cam, pop)
    assert np.array_equal(st32["radii"], st64["radii"])
    g32, g64 = o32.backward(st32, *grads), o64.backward(st64, *[x.double() for x in grads])
    dis = state_disagreement_pixels(st32, st64)
    ids = gaussians_contributing_to(st32, dis, 0)
    rep = []
    for name in ("color", "depth", "alpha"):
        a, b = np.asarray(st32[name], dtype=np.float64), np.asarray(st64[name], dtype=np.float64)
        err = np.abs(a - b).max(0) / (np.abs(b).max() + 1e-30)
        e_dis, e_rest = float(err[dis].max()) if dis.any() else 0.0, float(np.where(dis, 0.0, err).max())
        rep.append(f"{name} {e_rest:.1e} ({e_dis:.1e})")
        assert e_dis < 0.5 * IMAGE_SHARE, (name, e_dis)
    mask = np.zeros(N, dtype=bool); mask[ids] = True
    for name, a64 in g64.items():
        if a64 is None or name in ("dL_dconic", "dL_ddepth", "dL_dcolors_precomp"):
            continue
        a, b = np.asarray(g32[name], dtype=np.float64).reshape(N, -1), np.asarray(a64, dtype=np.float64).reshape(N, -1)
        err = np.abs(a - b).max(1) / (np.abs(b).max() + 1e-30)
        e_dis, e_rest = float(err[mask].max()) if mask.any() else 0.0, float(err[~mask].max())
        rep.append(f"{name} {e_rest:.1e} ({e_dis:.1e})")
        assert e_dis < 0.5 * NEAR_SHARE, (name, e_dis)
    assert ids.size <= 0.5 * ROW_EXCLUDED_CAP * pop["visible"], (ids.size, pop)
    print(f"\nROOM | {case_id(case)} | culled {pop['culled']} near {pop['near']} visible {pop['visible']} R {pop['R']} | disagreeing pixels {int(dis.sum())} of {H * W}, "
          f"their contributors {ids.size} | float32 from float64, max-norm, away from (on) them: " + "; ".join(rep))


# ---- the fuzz harness's plain stream --------------------------------------------------------------------------------------------------
def _inputs_hash(d):
    h = hashlib.sha256()
    for k in sorted(d):
        v = d[k]
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes() if torch.is_tensor(v) else repr(v).encode())
    return h.hexdigest()[:16]


# (N, H, W, mode, degree, active degree, scale multiplier, frame, culling, split SH, hash of the input dictionary) of draws 0, 1, 2,
# computed with the harness as it stood before it learnt about general cameras
RECORDED_DRAWS = {
    9001: [(63, 188, 400, "col_cov", 0, 0, 4.0, 54, False, False, "7f0a80166b707e97"), (1023, 122, 248, "sh_sr", 2, 0, 4.0, 115, True, True, "2c25a0680fbb331f"),
           (2, 286, 228, "sh_cov", 0, 0, 1.0, 44, True, False, "d454911200bc2df3")],
    424242: [(300, 142, 409, "sh_cov", 1, 0, 4.0, 72, False, True, "a631567723ec22e0"), (1, 39, 52, "col_cov", 0, 0, 8.0, 40, False, False, "b71e83451d47167c"),
             (7000, 269, 19, "col_sr", 0, 0, 0.5, 92, False, False, "2c73fe54e90ee70a")],
}


@pytest.mark.parametrize("seed", sorted(RECORDED_DRAWS))
def test_fuzz_stream_without_the_camera_switch_is_unchanged(seed):
    rng = np.random.default_rng(seed)
    for want in RECORDED_DRAWS[seed]:
        c = fuzz_draw(rng)
        got = (c["N"], c["H"], c["W"], c["mode"], c["deg"], c["active"], c["smul"], c["frame"], c["cull"], c["split"], _inputs_hash(fuzz_inputs(c)))
        assert got == want


def test_fuzz_stream_with_general_cameras_leaves_the_orbit():
    rng = np.random.default_rng(5)
    mods, pushed = set(), 0
    for _ in range(12):
        c = fuzz_draw(rng, cameras="general")
        c.update(N=64, H=24, W=40)
        d = fuzz_inputs(c)
        mods.add(d["scale_modifier"]); pushed += c["camera"]["push"] > 0
        assert float(d["viewmatrix"][:3, :3].abs().min()) > 0 and torch.isfinite(d["projmatrix"]).all()
        V = d["viewmatrix"].double()[:3, :3]
        assert float((V @ V.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert len(mods) > 1 and 0 < pushed < 12
