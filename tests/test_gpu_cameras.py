"""GPU parity at general cameras: the harness of tests/test_gpu_parity.py -- same bars, same flip rule, same row rule -- on frames
whose camera is rolled, turned, far from the world origin, anisotropic (fx != fy) or inside the cloud, with a scale modifier other than
1 (tests/cameras.py; tests/test_cameras_cpu.py pins the oracle at these cameras against float64 autograd first).  Every case states
what it must contain (cameras.assert_population) and asserts it on the oracle's state before anything is compared."""
import numpy as np
import pytest
import torch

from tests.cameras import CAMERAS, CAMERA_CASES, IN_CLOUD, case_id, population, assert_population, scene_in_world
from tests.common import make_inputs, seeded_grads, tile_culling, outlier_fraction
from tests import test_gpu_parity as P

pytestmark = pytest.mark.gpu

WIDE, WIDE_IN_CLOUD = "wide_rolled_far", "wide_rolled_far_in_cloud"          # cameras (a) and (d)


@pytest.fixture(autouse=True)
def _reference_lists():
    """As in tests/test_gpu_parity.py: tile culling off unless a test turns it on."""
    with tile_culling(False):
        yield


def _inputs(case):
    cam, N, H, W, seed, deg, mode, smul = case
    d = make_inputs(N, H, W, seed, deg, mode, scale_mul=smul, camera=cam)
    assert d["scale_modifier"] == CAMERAS[cam]["scale_modifier"]
    return d


def _stated_population(case, d, st):
    pop = population(st, d)
    assert_population(case[0], pop)
    return pop


@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "tile-culling"])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=case_id)
def test_forward_and_backward_parity_at_general_cameras(case, cull):
    cam, N, H, W, seed, deg, mode, smul = case
    d = _inputs(case)
    pop = _stated_population(case, d, P.oracle_forward(d)[1])
    rec = {}
    st, gb, out, hb = P.check_forward_and_backward_parity(d, cull, seed + 10, mode, record=rec)
    rows = "; ".join(f"{k} q50 {v['q50'][0]:.1e} ({v['q50'][1]:.1e}) q90 {v['q90'][0]:.1e} ({v['q90'][1]:.1e}) over 1e-3 {v['tails'][1e-3][0]} ({v['tails'][1e-3][1]})"
                     for k, v in rec["rows"].items())
    print(f"\nCAMERA_PARITY | {case_id(case)} culling {'on' if cull else 'off'} | culled {pop['culled']} near {pop['near']} visible {pop['visible']} R {pop['R']} | "
          f"flipped pixels {rec['flips']}, rows set aside {rec['set_aside']} | {rec['images']} | {rows}")
    if cam in IN_CLOUD:
        # the near plane inside a parity case: a row the oracle culls has radius 0, no tile, and an exactly zero row in every array the
        # backward writes (the helper compared the visible rows; check_grad_rows_vs_float64 the culled rows of the arrays it was given)
        gone = st["radii"] == 0
        assert gone.sum() >= 0.2 * N
        from egogaussian_amd import _C
        assert int(out[4].cpu().numpy()[gone].max()) == 0
        assert int(_C.geom_views(out[5], N)["offsets"].cpu().numpy().view(np.uint32)[gone].max()) == 0
        for k, t in enumerate(hb):
            if t.numel():
                assert float(t.reshape(N, -1)[torch.from_numpy(gone).to(t.device)].abs().max()) == 0.0, f"gradient array {k}: a culled row is not exactly zero"


@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "culled-lists"])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=case_id)
def test_fused_count_and_sort_in_blend_change_nothing_at_general_cameras(case, cull):
    """The rules of test_fused_count_pass_changes_nothing and test_sort_inside_the_forward_blend_changes_nothing: bit for bit."""
    d = _inputs(case)
    _stated_population(case, d, P.oracle_forward(d)[1])
    P.fused_count_pass_changes_nothing(d, make_inputs(900, 48, 80, case[4] + 1, 0, "rgb_sr"), cull)
    P.sort_inside_the_forward_blend_changes_nothing(d, cull)


@pytest.mark.parametrize("case", CAMERA_CASES, ids=case_id)
def test_tile_culling_changes_no_output_bit_at_general_cameras(case):
    d = _inputs(case)
    _stated_population(case, d, P.oracle_forward(d)[1])
    P.tile_culling_changes_no_output_bit(d, case[4] + 3)


@pytest.mark.parametrize("case", [c for c in CAMERA_CASES if c[0] in IN_CLOUD and c[5] in (0, 3)], ids=case_id)
def test_near_plane_inside_the_cloud(case):
    """mark_visible against the oracle's on positions of which a third sit behind the near plane, and the size-independent invariants
    of test_image_invariants_at_full_size: alpha = 1 - final_T, colour(bg) - colour(0) = final_T * bg, sum(tiles_touched) = R, the
    lists strictly increasing in (tile, depth, index), permutation invariance."""
    from egogaussian_amd import _C
    from oracle.oracle import Oracle
    dev = P._dev()
    cam, N, H, W, seed, deg, mode, smul = case
    d = _inputs(case)
    o, st = P.oracle_forward(d)
    _stated_population(case, d, st)
    vis = _C.mark_visible(d["means3D"].to(dev), d["viewmatrix"].to(dev), d["projmatrix"].to(dev)).cpu().numpy()
    want = Oracle(np.float32).mark_visible(d["means3D"], d["viewmatrix"])
    assert np.array_equal(vis, want) and 0.2 * N <= int((~want).sum()) < N
    g, out = P.hip_forward(d, dev)
    R, color, depth, alpha, radii, geom, binning, img = out
    assert R == st["R"] and np.array_equal(radii.cpu().numpy(), st["radii"])
    iv = _C.image_views(img, W, H); bv = _C.binning_views(binning, N, R, W, H, _C.stats["capacity"]); gv = _C.geom_views(geom, N)
    assert abs(float((alpha[0] + iv["final_T"] - 1).abs().max())) < 1e-4
    rng = iv["ranges"].cpu().numpy().view(np.uint32); pl = bv["point_list"].cpu().numpy().view(np.uint32)
    tile_of = np.repeat(np.arange(rng.shape[0], dtype=np.uint64), (rng[:, 1] - rng[:, 0]).astype(np.int64))
    keys = (tile_of << np.uint64(52)) | (gv["rec"].cpu().numpy()[pl, 9].view(np.uint32).astype(np.uint64) << np.uint64(20)) | pl
    assert len(keys) == R and np.all(keys[1:] > keys[:-1])
    assert int(gv["offsets"].sum()) == R
    d0 = dict(d); d0["bg"] = torch.zeros(3)
    _, out0 = P.hip_forward(d0, dev)
    assert float(((color - out0[1]) - iv["final_T"][None] * d["bg"].to(dev).view(3, 1, 1)).abs().max()) < 1e-5
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
    dp = {k: (v[perm] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N else v) for k, v in d.items()}
    _, outp = P.hip_forward(dp, dev)
    assert torch.equal(outp[4].cpu(), radii.cpu()[perm])
    assert outlier_fraction(outp[1].cpu().numpy(), color.cpu().numpy(), 1e-5) < 1e-4


@pytest.mark.parametrize("colour_mode", ["sh", "col"])
@pytest.mark.parametrize("where", ["orbit-modifier-1.7", WIDE, WIDE_IN_CLOUD])
def test_raw_parameter_mode_at_a_scale_modifier(where, colour_mode):
    """test_raw_parameter_mode_matches_activated_inputs with its bars at modifier 1.7: on the orbit with only the modifier changed, at
    camera (a), and at (a) inside the cloud -- the log-scale gradient chained through the modifier in the preprocess backward."""
    mode = "sh_sr" if colour_mode == "sh" else "col_sr"
    if where == "orbit-modifier-1.7":
        d = make_inputs(3000, 64, 96, 13, 0, mode, scale_mul=2.5)
        d["scale_modifier"] = 1.7
    else:
        d = make_inputs(3000, 64, 96, 13, 0, mode, scale_mul=2.5, camera=where)
    assert d["scale_modifier"] == 1.7
    P.raw_parameter_mode_matches_activated_inputs(d, colour_mode)


# ---- object rotation, motion and the fused optimizer at a scale modifier other than 1 ------------------------------------------------
@pytest.mark.parametrize("camera", [WIDE, WIDE_IN_CLOUD])
def test_object_rotation_inside_the_rasterizer_at_a_scale_modifier(camera):
    """tests/test_gpu_fused.py test_object_rotation_inside_the_rasterizer_matches_the_covariance_path, its comparison and its bars, at
    modifier 1.7: the rasterizer's own object-rotated covariance (and its dM path, which reuses the modified scales) against the
    rotated producer's."""
    from tests.test_gpu_fused import object_rotation_inside_the_rasterizer_matches_the_covariance_path
    assert CAMERAS[camera]["scale_modifier"] == 1.7
    object_rotation_inside_the_rasterizer_matches_the_covariance_path(camera)


@pytest.mark.parametrize("camera", [WIDE, WIDE_IN_CLOUD])
def test_motion_position_and_pose_gradients_at_a_scale_modifier(camera):
    """tests/test_gpu_motion.py test_position_and_pose_gradients (four stored coefficients: the generic spherical-harmonics kernels
    finish the position gradient), its references and its bounds, at modifier 1.7 with the pose expressed in the camera's world."""
    from tests.test_gpu_motion import position_and_pose_gradients
    assert CAMERAS[camera]["scale_modifier"] == 1.7
    position_and_pose_gradients("sh1", camera)


def test_fused_adam_step_with_culled_rows_in_every_block():
    """tests/test_gpu_fused_adam.py test_fused_step_is_the_standalone_step_bit_for_bit under camera (d): rows culled at the near plane
    sit in the same 256-row blocks as rows that are stepped.  Bit for bit, as there."""
    from tests.test_gpu_fused_adam import fused_step_is_the_standalone_step_bit_for_bit
    radii = fused_step_is_the_standalone_step_bit_for_bit(0, WIDE_IN_CLOUD).cpu().numpy()
    assert (radii == 0).mean() >= 0.2 and (radii > 0).sum() >= 100
    n_blocks = radii.size // 256
    mixed = [(radii[b * 256:(b + 1) * 256] == 0).any() and (radii[b * 256:(b + 1) * 256] > 0).any() for b in range(n_blocks)]
    assert all(mixed), "every 256-row block is meant to hold culled and stepped rows"


# ---- render()'s routes to a covariance at scaling_modifier = 1.7 ---------------------------------------------------------------------
LEAVES = ("_xyz", "_scaling", "_rotation", "_opacity")


def _render_route(route, scene, cam, mod, weights, rot=None):
    """One render of a SynthGaussians model through the named route, and the gradients of the four leaves the routes differ in."""
    from egogaussian_amd.scene_synth import SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    dev = P._dev()
    pc = SynthGaussians(scene, device=dev, sh_degree=1, fused=(route != "torch"))
    if route in ("producer", "rotated-producer"):
        pc.get_raw_parameters = lambda: None               # the fused producers: get_covariance_and_opacity / get_rotated_covariance_and_opacity
        pc.rotate_in_rasterizer = False
    kw = {}
    if rot is not None:
        R, is_obj = rot
        pc._is_object = is_obj
        kw = dict(rot_cov=True, accum_R=R, which_object=1, during_training=False)
    out = render(cam, pc, Pipe, torch.tensor([0.1, 0.2, 0.3], device=dev), scaling_modifier=mod, **kw)
    wc, wd, wa = weights
    ((out["render"] * wc).sum() + (out["depth"] * wd).sum() + (out["alpha"] * wa).sum()).backward()
    torch.cuda.synchronize()
    res = dict(image=out["render"].detach().cpu().numpy(), depth=out["depth"].detach().cpu().numpy(), alpha=out["alpha"].detach().cpu().numpy(),
               radii=out["radii"].cpu().numpy())
    res.update({a: getattr(pc, a).grad.cpu().numpy() for a in LEAVES})
    return res, pc


def _rel(x, y):
    return float(np.abs(x - y).max() / (np.abs(x).max() + 1e-30))


def test_render_routes_agree_at_scaling_modifier_1_7():
    """One model under camera (a), scaling_modifier = 1.7, through the torch covariance (get_covariance), the fused producer
    (get_covariance_and_opacity) and the raw-parameter route -- the modifier is applied by torch, by the producer, by the rasterizer.
    Pairwise: the bars of test_raw_parameter_mode_matches_activated_inputs (activations in torch against activations in the kernel);
    producer against raw also the bars of tests/test_gpu_provenance.py (the two routes of one library).  The raw route's image against
    the float32 oracle called with the unmodified scales and scale_modifier = 1.7.  With rot_cov: the rotated producer against
    get_raw_parameters_rotated, the bars of the object-rotation test."""
    from oracle.oracle import Oracle
    dev = P._dev()
    N, H, W = 3000, 64, 96
    scene, cam, mod = scene_in_world(WIDE, N, H, W, seed=7, sh_degree=1, device=dev, scale_mul=3.0)
    assert mod == 1.7
    weights = [t.to(dev) for t in seeded_grads(H, W, 21)]
    res = {r: _render_route(r, scene, cam, mod, weights)[0] for r in ("torch", "producer", "raw")}
    assert int((res["raw"]["radii"] > 0).sum()) > 1000
    for a, b in (("torch", "producer"), ("torch", "raw"), ("producer", "raw")):
        x, y = res[a], res[b]
        assert float((x["radii"] != y["radii"]).mean()) < 1e-3, (a, b)
        for k in ("image", "depth", "alpha"):
            assert outlier_fraction(y[k], x[k], P.TOL) <= 1e-4, (a, b, k)
        for k in LEAVES:
            assert outlier_fraction(y[k], x[k], 2e-4) <= 2e-4, (a, b, k)
            assert _rel(x[k], y[k]) < 5e-3, (a, b, k)
    x, y = res["producer"], res["raw"]
    assert np.array_equal(x["radii"], y["radii"])
    assert _rel(x["image"], y["image"]) < 1e-5 and _rel(x["depth"], y["depth"]) < 1e-5
    for k in LEAVES:
        assert _rel(x[k], y[k]) < 1e-4, k
    # the oracle: activated inputs, the scales NOT pre-multiplied, the modifier as the call scalar
    pc = _render_route("raw", scene, cam, mod, weights)[1]
    with torch.no_grad():
        st = Oracle(np.float32, nthreads=8).forward(
            means3D=pc.get_xyz, opacities=pc.get_opacity, shs=pc.get_features, scales=pc.get_scaling * 1, rotations=pc.get_rotation, scale_modifier=1.7,
            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center, bg=[0.1, 0.2, 0.3], image_height=H,
            image_width=W, tanfovx=float(np.tan(cam.FoVx / 2)), tanfovy=float(np.tan(cam.FoVy / 2)), sh_degree=1)
    assert float((res["raw"]["radii"] != st["radii"]).mean()) < 1e-3
    assert outlier_fraction(res["raw"]["image"], st["color"], P.TOL) <= 1e-4
    # rot_cov
    th = 0.7
    R = torch.tensor([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th) * 0.9, -0.3], [0.1, 0.3, 0.95]], dtype=torch.float32, device=dev)
    is_obj = (torch.rand(N, 1, generator=torch.Generator().manual_seed(4)) < 0.3).float().to(dev)
    is_obj[0, 0] = 0.0
    a = _render_route("rotated-producer", scene, cam, mod, weights, rot=(R, is_obj))[0]
    b = _render_route("raw-rotated", scene, cam, mod, weights, rot=(R, is_obj))[0]
    assert np.array_equal(a["radii"], b["radii"]) and not np.array_equal(a["radii"], res["raw"]["radii"])
    for k in ("image", "depth", "alpha"):
        assert np.array_equal(a[k], b[k]), k
    for k in LEAVES:
        assert float(np.abs(a[k] - b[k]).max()) <= 2e-5 * float(np.abs(a[k]).max()) + 1e-9, k


def test_provenance_substitution_keys_on_the_scale_modifier():
    """A covariance tagged with modifier 1.7 and rendered with settings modifier 1.7 is replaced by the raw parameters and matches the
    untagged route; the same tensor rendered with settings modifier 1.0 is rendered as given (provenance.substitute)."""
    import egogaussian_amd
    from egogaussian_amd import provenance
    from egogaussian_amd.rasterizer import GaussianRasterizer
    from egogaussian_amd.renderer import get_raster_settings
    from tests.test_adapter import RefShaped
    dev = P._dev()
    N, H, W = 3000, 64, 96
    scene, cam, mod = scene_in_world(WIDE, N, H, W, seed=8, sh_degree=0, device=dev, scale_mul=3.0)
    bg = torch.zeros(3, device=dev)
    outs = {}
    for tagged in (False, True):
        m = RefShaped(scene, device=dev); m.training_setup(); egogaussian_amd.attach(m, provenance=tagged)
        z = torch.zeros_like(m._xyz)
        for settings_mod in (1.7, 1.0):
            n0 = provenance.substitutions
            rast = GaussianRasterizer(get_raster_settings(cam, m, bg, settings_mod))
            img, radii = rast(means3D=m.get_xyz, means2D=z, opacities=m.get_opacity, shs=m.get_features, cov3D_precomp=m.get_covariance(1.7))[:2]
            assert provenance.substitutions == n0 + (1 if tagged and settings_mod == 1.7 else 0), (tagged, settings_mod)
            outs[(tagged, settings_mod)] = (img.detach().cpu().numpy(), radii.cpu().numpy())
    for settings_mod in (1.7, 1.0):
        (ia, ra), (ib, rb) = outs[(False, settings_mod)], outs[(True, settings_mod)]
        assert np.array_equal(ra, rb) and int((ra > 0).sum()) > 1000
        assert _rel(ia, ib) < 1e-5, settings_mod
    assert np.array_equal(outs[(True, 1.0)][0], outs[(False, 1.0)][0])        # not substituted: the very same call
