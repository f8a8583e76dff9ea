"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs.

Bars (BASELINE.json north_star): tile / sort indices bit-exact; RGB / depth / alpha and gradients within
1e-4 relative fp32.  Two fp32 effects are handled explicitly rather than by loosening the bar:
  * exp() on the GPU (v_exp_f32) and in glibc differ in the last ulp, so a (pixel, splat) pair whose alpha sits
    within ~1e-6 relative of the 1/255 or 1e-4 thresholds can be kept on one side and skipped on the other.
    Such pixels are DETECTED (off by more than 2e-6 of the image maximum) and must be PROVEN flips: the float64
    re-walk of the pixel's chain has to show a threshold-adjacent pair (tests/common.py flip_cause), otherwise the
    test fails; every other pixel of every image is held to 1e-4 (max-norm relative: of the plane's maximum), the
    proven flips to one threshold-level contribution, and only the Gaussians that CONTRIBUTE to a flipped pixel's chain
    (kept or threshold-adjacent entries of its float64 re-walk, tests/common.py gaussians_contributing_to: a fraction of
    the pixel's tile list) are set aside from the gradient bar -- held to 2e-3 instead, and capped in number.
  * gradient sums are accumulated in a different order (wave reductions + atomics).
The max-norm bar divides by the array's largest entry and says nothing about rows decades below it; the backward tests
therefore also measure every gradient row against its own magnitude, with the float64 oracle as the reference and the
float32 oracle's distance to it as the yardstick (tests/common.py check_grad_rows_vs_float64).
"""
import math

import numpy as np
import pytest
import torch

from tests.common import (make_inputs, seeded_grads, rel_err, outlier_fraction, tile_culling, fused_count, sort_in_blend, check_culled_lists, flip_pixels,
                          check_grads_isolating_flips, check_images_isolating_flips, check_grad_rows_vs_float64, gaussians_contributing_to)

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def hip_forward(d, dev, debug=False):
    from egogaussian_amd import _C
    g = _to(d, dev)
    e = torch.empty(0, device=dev)
    out = _C.rasterize_gaussians(g["bg"], g["means3D"], g.get("colors_precomp", e), g["opacities"], g.get("scales", e),
                                 g.get("rotations", e), g["scale_modifier"], g.get("cov3D_precomp", e), g["viewmatrix"],
                                 g["projmatrix"], g["tanfovx"], g["tanfovy"], g["image_height"], g["image_width"],
                                 g.get("shs", e), g["sh_degree"], g["campos"], False, debug)
    return g, out


def hip_backward(g, out, grads, dev, debug=False):
    from egogaussian_amd import _C
    R, color, depth, alpha, radii, geom, binning, img = out
    e = torch.empty(0, device=dev)
    gc, gd, ga = [x.to(dev) for x in grads]
    return _C.rasterize_gaussians_backward(g["bg"], g["means3D"], radii, g.get("colors_precomp", e), g.get("scales", e),
                                           g.get("rotations", e), g["scale_modifier"], g.get("cov3D_precomp", e),
                                           g["viewmatrix"], g["projmatrix"], g["tanfovx"], g["tanfovy"], gc, gd, ga,
                                           g.get("shs", e), g["sh_degree"], g["campos"], geom, R, binning, img, alpha, debug)


def oracle_forward(d, nthreads=8):
    from oracle.oracle import Oracle
    o = Oracle(np.float32, nthreads=nthreads)
    return o, o.forward(**d)


class pinned_capacity:
    """Run a block with the capacity hint of the current device set to `value`; the previous hint comes back afterwards.  Which sort
    instantiation and which launch site a frame gets is decided from the capacity, and the hint of a process otherwise only grows with
    the tests that ran before: a test that claims a path pins the capacity and asks the library which plan its call got (sort_plan_of)."""

    def __init__(self, value):
        self.value = int(value)

    def __enter__(self):
        from egogaussian_amd import _C
        self.key = torch.cuda.current_device()
        self.had, self.old = self.key in _C._capacity_hint, _C._capacity_hint.get(self.key)
        _C.set_capacity_hint(self.value)
        return self

    def __exit__(self, *exc):
        from egogaussian_amd import _C
        if self.had:
            _C._capacity_hint[self.key] = self.old
        else:
            _C._capacity_hint.pop(self.key, None)


def sort_plan_of(N, W, H, want_capacity, retries_before, debug=0):
    """The sort plan of the forward that has just run (SORT_* bits), after checking that it ran against the pinned capacity without a retry."""
    from egogaussian_amd import _C
    assert _C.stats["retries"] == retries_before, "the pinned capacity was too small: the forward was retried"
    assert _C.stats["capacity"] == want_capacity, (_C.stats["capacity"], want_capacity)
    return _C.sort_plan(N, W, H, _C.stats["capacity"], debug=debug)


def sort_regimes_of(st, capacity):
    """{(instantiation, regime): number of tiles} of an oracle state under the plan of `capacity` (tests/sort_regimes.py, the CPU model)."""
    import collections
    from tests import sort_regimes as sr
    return collections.Counter((i.inst, i.regime) for i in sr.regime_of_tiles(st, capacity, 0).values())


def float64_oracle(d, grads, nthreads=8):
    """The same frame and upstream gradients through the oracle in float64 -> (state, gradients)."""
    from oracle.oracle import Oracle
    o64 = Oracle(np.float64, nthreads=nthreads)
    st64 = o64.forward(**{k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()})
    return st64, o64.backward(st64, *[x.double() for x in grads])


def check_rows(d, grads, names, hb, st, gb, near, what, record=None):
    """Every gradient row of the HIP backward against its own magnitude (float64 oracle; yardstick: the float32 oracle `st`, `gb`)."""
    st64, g64 = float64_oracle(d, grads)
    return check_grad_rows_vs_float64(names, hb, st, gb, st64, g64, near, what=what, record=record)


CASES = [
    # N, H, W, seed, deg, mode, scale_mul
    (3000, 64, 64, 0, 0, "sh_cov", 1.0),       # BASELINE config 1 shape (training call)
    (3000, 70, 100, 1, 0, "sh_cov", 4.0),      # ragged image (not a multiple of 16), long lists, saturation
    (2000, 96, 128, 2, 3, "sh_cov", 2.0),      # SH degree 3
    (2000, 96, 128, 3, 0, "col_sr", 2.0),      # label call: colours + scale/rotation
    (2000, 50, 37, 4, 2, "sh_sr", 3.0),
    (2000, 64, 80, 5, 0, "col_cov", 3.0),
    (20000, 270, 480, 6, 0, "sh_cov", 2.0),
    (2000, 50, 37, 7, 1, "sh_sr", 3.0),        # SH degree 1: M = 4 under the per-row check
]


@pytest.fixture(autouse=True)
def _reference_lists():
    """Unless a test says otherwise the library keeps every instance of the reference's rectangles (tile culling off), so
    that its internal lists can be compared bit for bit with the oracle's; `cull=True` cases and the dedicated tests
    below run the default (culling on)."""
    with tile_culling(False):
        yield


@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "tile-culling"])
@pytest.mark.parametrize("N,H,W,seed,deg,mode,smul", CASES)
def test_forward_and_backward_parity(N, H, W, seed, deg, mode, smul, cull):
    check_forward_and_backward_parity(make_inputs(N, H, W, seed, deg, mode, scale_mul=smul), cull, seed + 10, mode)


def check_forward_and_backward_parity(d, cull, grad_seed, mode, record=None):
    """One frame (a make_inputs dictionary) through the HIP path and the oracle: integer stages bit for bit, images and gradients under
    the bars of this file.  record: a dict that receives the figures (flipped pixels, image distances, the row figures).
    -> (oracle state, oracle gradients, HIP forward outputs, HIP gradients)."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W, deg = int(d["means3D"].shape[0]), d["image_height"], d["image_width"], d["sh_degree"]
    o, st = oracle_forward(d)
    with tile_culling(cull):
        g, out = hip_forward(d, dev, debug=True)
    R, color, depth, alpha, radii, geom, binning, img = out
    torch.cuda.synchronize()

    # ---- integer stages: bit-exact -------------------------------------------------------------------
    assert R == st["R"], f"R {R} vs oracle {st['R']}"
    assert np.array_equal(radii.cpu().numpy(), st["radii"])
    gv = _C.geom_views(geom, N)
    vis = st["radii"] > 0
    assert np.array_equal(gv["offsets"].cpu().numpy().view(np.uint32), st["tiles_touched"])
    rec = gv["rec"].cpu().numpy()        # (x, y, qa, qb | qc, opacity, r, g | b, depth, bbox_x, bbox_y), egs_common.h
    assert np.array_equal(rec[vis, 0:2].view(np.uint32), st["xy"][vis].view(np.uint32)), "pixel centres not bit-exact"
    assert np.array_equal(rec[vis, 9].view(np.uint32), st["depths"][vis].view(np.uint32)), "depth not bit-exact"
    LOG2E = np.float32(1.4426950408889634)
    con = st["conic_opacity"][vis]
    q_expect = np.stack([np.float32(-0.5) * LOG2E * con[:, 0], -LOG2E * con[:, 1], np.float32(-0.5) * LOG2E * con[:, 2]], 1)
    assert np.array_equal(rec[vis][:, [2, 3, 4]].view(np.uint32), q_expect.astype(np.float32).view(np.uint32)), "conic not bit-exact"
    assert np.array_equal(rec[vis, 5].view(np.uint32), con[:, 3].view(np.uint32))
    rgb_hip = np.stack([rec[:, 6], rec[:, 7], rec[:, 8]], 1)
    assert rel_err(rgb_hip[vis], st["rgb"][vis]) < 1e-6
    rect = gv["rect"].cpu().numpy().view(np.uint32)
    rects_hip = np.stack([rect[:, 0] & 0xffff, rect[:, 1] & 0xffff, rect[:, 0] >> 16, rect[:, 1] >> 16], 1).astype(np.int32)
    assert np.array_equal(rects_hip[vis], st["rects"][vis])
    bv = _C.binning_views(binning, N, R, W, H, _C.stats["capacity"])
    assert bv["key_bits"] == st["key_bits"]
    iv = _C.image_views(img, W, H)
    pl = bv["point_list"].cpu().numpy().view(np.uint32)
    rng = iv["ranges"].cpu().numpy().view(np.uint32)
    nc_hip = iv["n_contrib"].cpu().numpy().view(np.uint32)
    if not cull:
        assert np.array_equal(pl, st["point_list"]), "sorted instance list not bit-exact"
        # rebuild the canonical 64-bit keys (tile << 32 | depth bits) from the HIP state and compare with the oracle's
        tile_of = np.repeat(np.arange(rng.shape[0], dtype=np.uint64), (rng[:, 1] - rng[:, 0]).astype(np.int64))
        keys_hip = (tile_of << np.uint64(32)) | rec[pl, 9].view(np.uint32).astype(np.uint64)
        assert np.array_equal(keys_hip, st["keys"]), "sorted keys not bit-exact"
        assert np.array_equal(rng, st["ranges"])
        nc_eq = (nc_hip == st["n_contrib"]).mean()
    else:
        kept, dropped = check_culled_lists(st, rng, pl, H, W)
        print(f"\n   tile culling: {kept} of {kept + dropped} instances kept")
        # the last contributor of every pixel is the same splat, at a (possibly) earlier position of the shorter list
        ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
        t = ty * ((W + 15) // 16) + tx
        has_o, has_h = st["n_contrib"] > 0, nc_hip > 0
        id_o = st["point_list"][np.where(has_o, st["ranges"][t, 0].astype(np.int64) + st["n_contrib"] - 1, 0)]
        id_h = pl[np.where(has_h, rng[t, 0].astype(np.int64) + nc_hip - 1, 0)]
        nc_eq = ((has_o == has_h) & (~has_o | (id_o == id_h))).mean()

    # ---- images ----------------------------------------------------------------------------------------
    e_c, e_d, e_a = (rel_err(color.cpu().numpy(), st["color"]), rel_err(depth.cpu().numpy(), st["depth"]),
                     rel_err(alpha.cpu().numpy(), st["alpha"]))
    f_c = outlier_fraction(color.cpu().numpy(), st["color"], TOL)
    print(f"\n[{N}@{W}x{H} {mode} deg{deg}] R={R} n_contrib equal {nc_eq:.6f}; max rel err colour {e_c:.2e} depth {e_d:.2e} "
          f"alpha {e_a:.2e}; colour outliers>{TOL:g}: {f_c:.2e}")
    assert nc_eq > 0.9995
    # threshold flips (tests/common.py): found with a threshold far below the bar and PROVEN (a threshold-adjacent pair in the float64 chain
    # of the pixel, else flip_pixels fails); every other pixel of every plane within 1e-4 of the plane's maximum
    flip_px = flip_pixels(color.cpu().numpy(), iv["final_T"].cpu().numpy(), st, None if cull else nc_hip)
    img_rep = check_images_isolating_flips((("color", color.cpu().numpy(), st["color"]), ("depth", depth.cpu().numpy(), st["depth"]),
                                            ("alpha", alpha.cpu().numpy(), st["alpha"]), ("final_T", iv["final_T"].cpu().numpy(), st["final_T"])),
                                           st, flip_px, TOL, what=f"[{N}@{W}x{H} {mode}]")
    print("   images: " + img_rep + f"; flipped pixels {int(flip_px.sum())}")

    # ---- gradients -------------------------------------------------------------------------------------
    grads = seeded_grads(H, W, grad_seed)
    hb = hip_backward(g, out, grads, dev, debug=True)
    torch.cuda.synchronize()
    gb = o.backward(st, *grads)
    names = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"]
    # every Gaussian that contributes to no (proven) flipped pixel is held to 1e-4 of the array's maximum ...
    near = []
    rep, _, _ = check_grads_isolating_flips(names, hb, gb, st, flip_px, TOL, what=f"[{N}@{W}x{H} {mode}]", near_out=near)
    print("   grads: " + rep)
    # ... and every row to its own magnitude
    rows = {}
    print("   " + check_rows(d, grads, names, hb, st, gb, near[0], f"[{N}@{W}x{H} {mode}]", record=rows))
    if record is not None:
        record.update(R=R, flips=int(flip_px.sum()), images=img_rep, set_aside=int(near[0].size), rows=rows)
    return st, gb, out, hb


@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "tile-culling"])
@pytest.mark.parametrize("mode", ["sh_cov", "sh_sr"])
def test_cold_rows_under_a_hot_window(mode, cull):
    """The scale of every gradient array swamped on purpose: the upstream gradients are multiplied by 1e3 inside one 32x32 window that
    straddles four tiles, so that the splats under it own the array maxima and (asserted on the oracle's gradients) at least 90 % of
    the visible rows of every array sit below 1e-3 of the maximum -- where a max-norm bar of 1e-4 accepts a row that is 10 % wrong.
    Both measures: the max-norm bar with the contributors of the proven flips set aside, and every row against its own magnitude."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 20000, 270, 480
    d = make_inputs(N, H, W, 6, 0, mode, scale_mul=2.0)
    grads = [x.clone() for x in seeded_grads(H, W, 16)]
    for x in grads:
        x[:, 120:152, 120:152] *= 1e3
    o, st = oracle_forward(d)
    gb = o.backward(st, *grads)
    names = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"]
    vis = st["radii"] > 0
    for name in names:
        if gb.get(name) is not None:
            mag = np.abs(np.asarray(gb[name], dtype=np.float64).reshape(N, -1)).max(1)
            cold = float((mag[vis] < 1e-3 * mag.max()).mean())
            assert cold >= 0.9, f"{name}: only {cold:.3f} of the visible rows are below 1e-3 of the array maximum"
    with tile_culling(cull):
        g, out = hip_forward(d, dev)
        hb = hip_backward(g, out, grads, dev)
    torch.cuda.synchronize()
    assert out[0] == st["R"] and np.array_equal(out[4].cpu().numpy(), st["radii"])
    iv = _C.image_views(out[7], W, H)
    flip_px = flip_pixels(out[1].cpu().numpy(), iv["final_T"].cpu().numpy(), st, None if cull else iv["n_contrib"].cpu().numpy().view(np.uint32))
    what = f"[hot window, {mode}, culling {'on' if cull else 'off'}]"
    near = []
    rep, _, _ = check_grads_isolating_flips(names, hb, gb, st, flip_px, TOL, what=what, near_out=near)
    print("\n   grads: " + rep)
    print("   " + check_rows(d, grads, names, hb, st, gb, near[0], what))


@pytest.mark.parametrize("N,H,W,seed,mode,smul", [(20000, 270, 480, 6, "sh_cov", 2.0), (3000, 70, 100, 1, "col_sr", 4.0),
                                                   (500000, 540, 960, 0, "sh_cov", 1.0)])
def test_tile_culling_changes_no_output_bit(N, H, W, seed, mode, smul):
    """Dropping the instances whose tile the splat cannot reach (the default) must leave colour, depth, alpha, final
    transmittance and radii bit-identical to the run that keeps the reference's full rectangles, and the gradients equal
    up to the order of the floating-point accumulation; the lists must shrink, stay sorted, and keep `num_rendered`."""
    tile_culling_changes_no_output_bit(make_inputs(N, H, W, seed, 0, mode, scale_mul=smul), seed + 3)


def tile_culling_changes_no_output_bit(d, grad_seed):
    """The body of the test above for one frame (a make_inputs dictionary)."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = int(d["means3D"].shape[0]), d["image_height"], d["image_width"]
    grads = seeded_grads(H, W, grad_seed)
    res = {}
    for cull in (False, True):
        with tile_culling(cull):
            g, out = hip_forward(d, dev)
            hb = hip_backward(g, out, grads, dev)
        iv = _C.image_views(out[7], W, H); bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"])
        rng = iv["ranges"].cpu().numpy().view(np.uint32).astype(np.int64)
        n_list = int((rng[:, 1] - rng[:, 0]).sum())
        res[cull] = dict(R=out[0], img=[t.clone() for t in out[1:5]] + [iv["final_T"].clone()], grads=[t.clone() for t in hb],
                         n_list=n_list, rng=rng, pl=bv["point_list"].cpu().numpy().view(np.uint32)[:n_list].copy(),
                         depth=_C.geom_views(out[5], N)["rec"].cpu().numpy()[:, 9].view(np.uint32).copy())
    a, b = res[False], res[True]
    assert a["R"] == b["R"] and a["n_list"] == a["R"] and b["n_list"] < a["R"]
    print(f"\n[{N}@{W}x{H}] instances {a['n_list']} -> {b['n_list']} ({b['n_list'] / a['n_list']:.3f})")
    for x, y in zip(a["img"], b["img"]):
        assert torch.equal(x, y), "tile culling changed an output value"
    for x, y in zip(a["grads"], b["grads"]):
        if x.numel():
            assert rel_err(y.cpu().numpy(), x.cpu().numpy()) < 1e-5
    tile_of = np.repeat(np.arange(len(b["rng"]), dtype=np.uint64), b["rng"][:, 1] - b["rng"][:, 0])
    keys = (tile_of << np.uint64(52)) | (b["depth"][b["pl"]].astype(np.uint64) << np.uint64(20)) | b["pl"]
    assert np.all(keys[1:] > keys[:-1])                              # strictly increasing in (tile, depth, index)
    key_a = np.repeat(np.arange(len(a["rng"]), dtype=np.int64), a["rng"][:, 1] - a["rng"][:, 0]) * (1 << 32) + a["pl"]
    key_b = tile_of.astype(np.int64) * (1 << 32) + b["pl"]
    assert np.array_equal(key_a[np.isin(key_a, key_b)], key_b)      # an ordered sub-list of the full list


@pytest.mark.parametrize("N,H,W,seed,mode,smul", [(20000, 270, 480, 5, "sh_cov", 2.0), (3001, 67, 131, 2, "rgb_sr", 1.0), (70000, 540, 960, 9, "sh_sr", 1.0),
                                                  (1200, 33, 47, 1, "sh_cov", 6.0)])
@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "culled-lists"])
def test_fused_count_pass_changes_nothing(N, H, W, seed, mode, smul, cull):
    """ABI 5: with a placement buffer the count pass of the tile bucketing runs inside the preprocess launch (k_preprocess_count).  Every
    array the chain leaves -- radii, records, rectangles, per-block counts, the scanned table's tile starts, ranges, the sorted lists, the
    images -- must equal, bit for bit, what the separate k_preprocess + k_bin_count launches produce; twice in a row (the second frame
    finds the chunk sums the first one's chain cleared), and after a frame of ANOTHER size on the same stream in between."""
    fused_count_pass_changes_nothing(make_inputs(N, H, W, seed, 0, mode, scale_mul=smul), make_inputs(900, 48, 80, seed + 1, 0, "rgb_sr"), cull)


def fused_count_pass_changes_nothing(d, other, cull):
    """The body of the test above for one frame `d` and a frame of another size `other` (make_inputs dictionaries)."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = int(d["means3D"].shape[0]), d["image_height"], d["image_width"]
    res = {}
    with tile_culling(cull):
        hip_forward(d, dev)                                          # establishes the capacity: the fused path needs capacity > 0
        for fused in (False, True, True):
            with fused_count(fused):
                if fused:
                    hip_forward(other, dev)
                g, out = hip_forward(d, dev)
            iv = _C.image_views(out[7], W, H); bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"]); gv = _C.geom_views(out[5], N)
            rng = iv["ranges"].cpu().numpy().view(np.uint32).astype(np.int64)
            n_list = int((rng[:, 1] - rng[:, 0]).sum())
            cur = dict(R=out[0], planes=[t.clone() for t in out[1:5]] + [iv["final_T"].clone(), iv["n_contrib"].clone()], rng=rng,
                       pl=bv["point_list"].cpu().numpy().view(np.uint32)[:n_list].copy(),
                       geom=[gv["offsets"].clone(), gv["visible"].clone()] + [gv[k][gv["visible"]].clone() for k in ("rec", "rect", "clamped")])   # (rows of culled Gaussians are not written)
            if not fused:
                res = cur
                continue
            assert cur["R"] == res["R"] and np.array_equal(cur["rng"], res["rng"]) and np.array_equal(cur["pl"], res["pl"]), "fused count pass changed the lists"
            for x, y in zip(cur["planes"] + cur["geom"], res["planes"] + res["geom"]):
                assert torch.equal(x, y), "fused count pass changed an output"


@pytest.mark.parametrize("N,H,W,seed,mode,smul", [(20000, 270, 480, 5, "sh_cov", 2.0), (3001, 67, 131, 2, "rgb_sr", 1.0), (70000, 540, 960, 9, "sh_sr", 1.0),
                                                  (1200, 33, 47, 1, "sh_cov", 6.0), (9000, 64, 64, 3, "rgb_sr", 8.0)])
@pytest.mark.parametrize("cull", [False, True], ids=["reference-lists", "culled-lists"])
def test_sort_inside_the_forward_blend_changes_nothing(N, H, W, seed, mode, smul, cull):
    """The forward blend's workgroups sort their tile's bucket themselves (render_fwd.hip SORT; no k_tile_sort launch): ranges, lists and every
    output plane must equal, bit for bit, what the separate sort launch produces -- including tiles beyond the register path's 1 792 entries
    (the last case: 9 000 splats x 8 on 16 tiles) and the chain that clears the fused count pass's chunk sums."""
    res = sort_inside_the_forward_blend_changes_nothing(make_inputs(N, H, W, seed, 0, mode, scale_mul=smul), cull)
    if smul == 8.0:
        assert res["longest"] > 1792, "this case is meant to take the slab path"


def sort_inside_the_forward_blend_changes_nothing(d, cull):
    """The body of the test above for one frame (a make_inputs dictionary).  -> the figures of the run with the separate sort launch."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = int(d["means3D"].shape[0]), d["image_height"], d["image_width"]
    res = {}
    with tile_culling(cull):
        R = hip_forward(d, dev)[1][0]
        n_tiles = ((W + 15) // 16) * ((H + 15) // 16)
        assert 0 < R <= 2048 * n_tiles, "this frame can never be sorted inside the blend: its instance count needs the second instantiation"
        for inside in (False, True, True):
            with sort_in_blend(inside), pinned_capacity(R):
                retries = _C.stats["retries"]
                g, out = hip_forward(d, dev)
                plan = sort_plan_of(N, W, H, R, retries)
            assert plan == (_C.SORT_IN_BLEND if inside else 0), f"plan {plan:#x} with sort_in_blend({inside}): the two launch sites are not the ones being compared"
            iv = _C.image_views(out[7], W, H); bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"])
            rng = iv["ranges"].cpu().numpy().view(np.uint32).astype(np.int64)
            n_list = int((rng[:, 1] - rng[:, 0]).sum())
            cur = dict(R=out[0], planes=[t.clone() for t in out[1:5]] + [iv["final_T"].clone(), iv["n_contrib"].clone()], rng=rng,
                       pl=bv["point_list"].cpu().numpy().view(np.uint32)[:n_list].copy(), longest=int((rng[:, 1] - rng[:, 0]).max()))
            if not inside:
                res = cur
                continue
            assert cur["R"] == res["R"] and np.array_equal(cur["rng"], res["rng"]) and np.array_equal(cur["pl"], res["pl"]), "sort inside the blend changed the lists"
            for x, y in zip(cur["planes"], res["planes"]):
                assert torch.equal(x, y), "sort inside the blend changed an output"
    return res


def _init_placement(t, W, H, dev):
    from egogaussian_amd import lib, _hip
    lib.check(lib.load().egs_placement_init(t.data_ptr(), int(W), int(H), _hip.stream_of(dev)))


def test_placement_buffer_first_seen_dirty():
    """A placement buffer may hold anything in its cost and tile-order words, but its sums region must be zero when a forward starts:
    the OWNER clears it once with egs_placement_init (include/egs_raster.h; ABI 6: the library keeps no record of buffers and never
    clears behind the caller's back).  Hand over a buffer full of 0xAB, initialised, through the C ABI path the Python layer uses and
    compare with the regular one."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 6000, 135, 240
    d = make_inputs(N, H, W, 4, 0, "sh_cov")
    hip_forward(d, dev)
    g, ref = hip_forward(d, dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = [k for k in _C._placement if k[0] == idx and k[1] == W and k[2] == H]
    assert key, "no placement buffer for this size"
    saved = _C._placement[key[0]]
    try:
        dirty = torch.full_like(saved, 0xAB)                          # a different address, dirty everywhere
        _init_placement(dirty, W, H, dev)                             # ... the owner's one call: only the sums region is cleared
        assert int((dirty == 0xAB).sum()) > 0 and int((dirty == 0).sum()) > 0
        _C._placement[key[0]] = dirty
        g, out = hip_forward(d, dev)
        g, out2 = hip_forward(d, dev)
    finally:
        _C._placement[key[0]] = saved
    for o in (out, out2):
        assert o[0] == ref[0]
        for x, y in zip(o[1:5], ref[1:5]):
            assert torch.equal(x, y)


def test_one_placement_buffer_two_image_sizes():
    """A C caller may hand ONE placement allocation to forwards of different sizes: the sums region sits behind a size-dependent number of
    cost words, so the owner calls egs_placement_init again whenever it changes the size it uses the buffer for (the contract of ABI 6;
    through ABI 5 a process-wide registry of addresses did this behind the caller's back)."""
    from egogaussian_amd import _C
    dev = _dev()
    sizes = [(6000, 135, 240, 4), (9000, 270, 480, 7)]
    ins = [make_inputs(N, H, W, seed, 0, "sh_cov") for N, H, W, seed in sizes]
    refs = []
    for d in ins:
        hip_forward(d, dev)
        refs.append(hip_forward(d, dev)[1])
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    keys = [[k for k in _C._placement if k[0] == idx and k[1] == W and k[2] == H][0] for _, H, W, _ in sizes]
    saved = [_C._placement[k] for k in keys]
    shared = torch.full((max(t.numel() for t in saved),), 0x5C, device=dev, dtype=torch.uint8)
    try:
        for k in keys:
            _C._placement[k] = shared
        for rnd in range(3):
            for (N, H, W, _), d, ref in zip(sizes, ins, refs):
                _init_placement(shared, W, H, dev)                    # the size changes: the owner re-initialises
                out = hip_forward(d, dev)[1]
                assert out[0] == ref[0] and all(torch.equal(x, y) for x, y in zip(out[1:5], ref[1:5])), f"round {rnd}"
    finally:
        for k, t in zip(keys, saved):
            _C._placement[k] = t


@pytest.mark.parametrize("H,W", [(2160, 3840), (2304, 4096)], ids=["32400-tiles", "36864-tiles"])
def test_4k_image_tile_counters_fill_the_lds(H, W):
    """3840x2160 = 32400 tiles: the per-tile counters of the bucketing kernels take 127 KiB of the 160 KiB LDS (one
    workgroup per CU) and a bucketing round stages 8 groups of 64 Gaussians instead of 16; 4096x2304 = 36864 tiles is the
    largest image the ABI accepts (144 KiB of counters, 4 groups per round).  Lists and image vs the oracle, with the
    reference's rectangles and with tile culling."""
    from egogaussian_amd import _C
    dev = _dev()
    N = 3000
    d = make_inputs(N, H, W, 11, 0, "sh_cov", scale_mul=6.0)
    o, st = oracle_forward(d)
    for cull in (False, True):
        with tile_culling(cull):
            g, out = hip_forward(d, dev)
        bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"]); iv = _C.image_views(out[7], W, H)
        assert out[0] == st["R"] and st["R"] > N
        pl, rng = bv["point_list"].cpu().numpy().view(np.uint32), iv["ranges"].cpu().numpy().view(np.uint32)
        if cull:
            kept, dropped = check_culled_lists(st, rng, pl, H, W)
            assert dropped > 0
        else:
            assert np.array_equal(pl, st["point_list"]) and np.array_equal(rng, st["ranges"])
        assert outlier_fraction(out[1].cpu().numpy(), st["color"], TOL) <= 1e-4


def test_empty_and_culled_inputs():
    from egogaussian_amd import _C
    dev = _dev()
    d = make_inputs(100, 48, 64, 0, 0, "sh_cov")
    # all behind the camera
    d2 = dict(d); d2["means3D"] = d["means3D"].clone(); d2["means3D"][:, 2] = -5.0
    g, out = hip_forward(d2, dev)
    R, color, depth, alpha, radii = out[:5]
    assert R == 0 and int(radii.abs().sum()) == 0
    bgimg = d["bg"].view(3, 1, 1).expand(3, 48, 64)
    assert torch.equal(color.cpu(), bgimg) and float(alpha.abs().sum()) == 0 and float(depth.abs().sum()) == 0
    hb = hip_backward(g, out, seeded_grads(48, 64), dev)
    assert all(float(t.abs().sum()) == 0 for t in hb if t.numel())
    # P == 0
    d0 = {k: (v[:0] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == 100 else v) for k, v in d.items()}
    g, out = hip_forward(d0, dev)
    assert out[0] == 0 and torch.equal(out[1].cpu(), bgimg) and out[4].numel() == 0
    hb = hip_backward(g, out, seeded_grads(48, 64), dev)
    assert hb[0].shape == (0, 3)


def test_capacity_guess_paths_agree():
    """The speculative one-call forward (capacity guess large enough), the retry path (guess too small) and the first
    call (no guess) must produce identical results."""
    from egogaussian_amd import _C
    dev = _dev()
    d = make_inputs(4000, 96, 128, 8, 0, "sh_cov", scale_mul=3.0)
    key = torch.cuda.current_device()
    outs = []
    for hint in (0, 10, 10_000_000):                       # no guess / too small (retry) / ample
        _C._capacity_hint[key] = hint
        before = _C.stats["retries"]
        g, out = hip_forward(d, dev)
        assert (_C.stats["retries"] > before) == (hint < out[0])
        bv = _C.binning_views(out[6], 4000, out[0], 128, 96, _C.stats["capacity"])
        outs.append((out[0], out[1].clone(), out[2].clone(), out[3].clone(), bv["point_list"].clone()))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and all(torch.equal(a, b) for a, b in zip(o[1:], outs[0][1:]))
    assert _C._capacity_hint[key] >= outs[0][0]


def test_deferred_count_check_agrees_and_finds_a_clipped_frame():
    """The eager forward WITHOUT the host wait for the instance count (a StepGuard(deferred=True): enqueued against the capacity hint,
    checked at the next forward): with room its outputs are those of the synchronous path bit for bit; with too little room the
    frame is clipped, which the following call finds -- the overflow is counted, the hint is raised, and that call's outputs are
    the synchronous path's again.  /root/reference/trainers/train_static.py:67-138 is the loop this serves."""
    from egogaussian_amd import _C
    dev = _dev()
    d = make_inputs(4000, 96, 128, 8, 0, "sh_cov", scale_mul=3.0)
    key = torch.cuda.current_device()
    _C._capacity_hint[key] = 0
    g, ref = hip_forward(d, dev)                                   # synchronous: establishes the capacity
    R = ref[0]
    bv = _C.binning_views(ref[6], 4000, R, 128, 96, _C.stats["capacity"])
    ref_list = bv["point_list"].clone()

    def deferred_forward(guard):
        gg = _to(d, dev)
        e = torch.empty(0, device=dev)
        return _C.rasterize_gaussians(gg["bg"], gg["means3D"], e, gg["opacities"], e, e, 1.0, gg["cov3D_precomp"], gg["viewmatrix"],
                                      gg["projmatrix"], gg["tanfovx"], gg["tanfovy"], 96, 128, gg["shs"], 0, gg["campos"], False, False, guard=guard)
    guard = _C.StepGuard(dev, deferred=True)
    out = deferred_forward(guard)
    assert out[0] == _C.stats["capacity"] >= R                     # the layout size, as under graph capture
    assert all(torch.equal(a, b) for a, b in zip(out[1:5], ref[1:5]))
    assert torch.equal(_C.binning_views(out[6], 4000, R, 128, 96, _C.stats["capacity"])["point_list"], ref_list)
    assert guard.check() and guard.last_R == R and guard.frames == 1 and int(guard.overflow[0].item()) == 0
    # too little room: the frame is clipped (and would be voided: the overflow word is set), the NEXT call knows
    _C._capacity_hint[key] = 1000
    guard2 = _C.StepGuard(dev, deferred=True)
    deferred_forward(guard2)
    torch.cuda.synchronize()
    assert int(guard2.overflow[0].item()) == 1 and guard2.overflows == 0        # clipped on the device, not yet seen by the host
    out = deferred_forward(guard2)
    assert guard2.overflows == 1 and _C.stats["capacity"] >= R and _C._capacity_hint[key] >= R
    assert all(torch.equal(a, b) for a, b in zip(out[1:5], ref[1:5]))
    assert guard2.check() is False and guard2.last_R == R and int(guard2.overflow[0].item()) == 0


def test_depth_ties_keep_index_order():
    """All Gaussians at the same depth: every tile list must come out in Gaussian-index order (oracle: stable sort)."""
    from egogaussian_amd import _C
    from egogaussian_amd.scene_synth import make_camera
    dev = _dev()
    d = make_inputs(3000, 64, 64, 5, 0, "col_sr", scale_mul=6.0)
    d["means3D"][:, 2] = 5.0
    cam = make_camera(0, 64, 64)
    d.update(viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)
    o, st = oracle_forward(d)
    assert set(sort_regimes_of(st, st["R"])) == {(4, "equal")}, "every tile is meant to take the index-digit passes of the four-wave instantiation"
    with pinned_capacity(st["R"]):
        retries = _C.stats["retries"]
        g, out = hip_forward(d, dev)
        assert sort_plan_of(3000, 64, 64, st["R"], retries) == _C.SORT_IN_BLEND
    bv = _C.binning_views(out[6], 3000, out[0], 64, 64, _C.stats["capacity"])
    assert out[0] == st["R"] and st["R"] > 3000
    assert np.array_equal(bv["point_list"].cpu().numpy().view(np.uint32), st["point_list"])
    assert rel_err(out[1].cpu().numpy(), st["color"]) < 1e-5


@pytest.mark.parametrize("layout", ["two-surfaces", "pile-with-ties", "one-outlier"])
def test_clustered_depths_take_the_sorts_fallback_and_still_match(layout):
    """The per-tile sort first spreads a tile's instances over 512 buckets by the top bits of (depth - tile minimum) and orders
    each bucket by direct comparison; depths piled up in a sliver of the range overflow a bucket and send the tile to the
    digit-by-digit passes.  Lists must stay bit-exact either way: two thin surfaces, a pile with exact depth ties in it, and
    a single far outlier that stretches the range (so that everything else lands in one bucket)."""
    from egogaussian_amd import _C
    from egogaussian_amd.scene_synth import make_camera
    dev = _dev()
    N, H, W = 6000, 64, 96
    d = make_inputs(N, H, W, 8, 0, "col_sr", scale_mul=5.0)
    gen = torch.Generator().manual_seed(3)
    z = d["means3D"][:, 2]
    if layout == "two-surfaces":
        z[:] = torch.where(torch.rand(N, generator=gen) < 0.5, 3.0, 7.0) + 1e-4 * torch.randn(N, generator=gen)
    elif layout == "pile-with-ties":
        z[:] = 5.0 + 1e-5 * torch.randint(0, 40, (N,), generator=gen).float()     # 40 distinct depths, hundreds of ties each
        z[::50] = 2.0 + 6.0 * torch.rand(len(z[::50]), generator=gen)
    else:
        z[:] = 4.0 + 1e-3 * torch.rand(N, generator=gen)
        z[0] = 9.5; d["means3D"][0, :2] = 0.0; d["scales"][0] = 3.0                 # one huge far splat over the whole image
    cam = make_camera(0, H, W)
    d.update(viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)
    o, st = oracle_forward(d)
    regimes = sort_regimes_of(st, st["R"])
    assert set(regimes) == {(4, "digits+ties")}, f"every tile is meant to take the digit-by-digit passes of the four-wave instantiation: {dict(regimes)}"
    with pinned_capacity(st["R"]):
        retries = _C.stats["retries"]
        g, out = hip_forward(d, dev)
        assert sort_plan_of(N, W, H, st["R"], retries) == _C.SORT_IN_BLEND
    bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"])
    assert out[0] == st["R"] and st["R"] > 2 * N
    assert np.array_equal(bv["point_list"].cpu().numpy().view(np.uint32), st["point_list"])
    assert outlier_fraction(out[1].cpu().numpy(), st["color"], TOL) <= 1e-4


@pytest.mark.parametrize("layout", ["uniform", "one-dense-tile", "dense-and-tied"])
def test_tiles_beyond_the_register_capacity_are_sorted_in_depth_slabs(layout):
    """Tile lists longer than the in-register capacity (1792 / 4096 keys) go through the depth-slab path: histogram into linear depth
    buckets, runs of buckets with at most the capacity gathered into LDS and ranked one after another.  `uniform`: every tile of a
    small image holds ~8 k instances (the second instantiation's slabs); `one-dense-tile`: a cluster of 12 k splats inside one tile of
    an otherwise light image -- few instances per tile on average, so only the first instantiation is launched and ITS slab path takes
    the tile; `dense-and-tied`: the same with a quarter of the cluster at one depth (ties settled by the index inside a slab, a pile
    too big for a bucket falls through to the digit-by-digit passes).  Lists and image against the oracle."""
    from egogaussian_amd import _C
    dev = _dev()
    if layout == "uniform":
        N, H, W = 24000, 64, 64
        d = make_inputs(N, H, W, 21, 0, "sh_cov", scale_mul=8.0)
    else:
        N, H, W = 16000, 128, 160
        d = make_inputs(N, H, W, 22, 0, "sh_cov", scale_mul=0.5)
        g = torch.Generator().manual_seed(9)
        m3 = d["means3D"]
        k = 12000
        m3[:k, 0] = 0.02 * torch.randn(k, generator=g); m3[:k, 1] = 0.02 * torch.randn(k, generator=g)     # a cluster on the optical axis: one tile
        m3[:k, 2] = 3.0 + 4.0 * torch.rand(k, generator=g)
        if layout == "dense-and-tied":
            m3[:3000, 2] = 4.5
    o, st = oracle_forward(d)
    lens = (st["ranges"][:, 1] - st["ranges"][:, 0])
    assert lens.max() > 4096 and (layout == "uniform") == (lens.mean() > 2048), (int(lens.max()), float(lens.mean()))
    # the path the layout names, from the CPU model of the dispatch under the pinned capacity, and the plan the library reports for the call
    regimes = sort_regimes_of(st, st["R"])
    want = {"uniform": (8, "slabs"), "one-dense-tile": (4, "slabs"), "dense-and-tied": (4, "global")}[layout]
    assert regimes[want] >= 1 and {i for i, _ in regimes} == ({8} if layout == "uniform" else {4}), dict(regimes)
    with pinned_capacity(st["R"]):
        retries = _C.stats["retries"]
        g_, out = hip_forward(d, dev)
        assert sort_plan_of(N, W, H, st["R"], retries) == (_C.SORT_SECOND_INSTANTIATION if layout == "uniform" else _C.SORT_IN_BLEND)
    bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"]); iv = _C.image_views(out[7], W, H)
    assert out[0] == st["R"]
    assert np.array_equal(iv["ranges"].cpu().numpy().view(np.uint32), st["ranges"])
    assert np.array_equal(bv["point_list"].cpu().numpy().view(np.uint32), st["point_list"]), f"longest list {int(lens.max())}"
    assert outlier_fraction(out[1].cpu().numpy(), st["color"], TOL) <= 1e-4


@pytest.mark.parametrize("layout", ["every-tile", "one-tile"])
def test_tiles_just_over_the_small_sorts_register_capacity(layout):
    """The four-wave instantiation of the per-tile sort holds 1 792 pairs in registers (eight workgroups per CU); lists of 1 793 ... 2 048
    used to fit it.  `every-tile`: lists of 1 200 ... 3 300, 2 090 on average, so both instantiations are launched and the eight-wave one takes the
    tiles beyond 1 792; `one-tile`: a cluster of ~1 900 splats in one tile of a light image -- only the four-wave instantiation is
    launched and that tile goes through its depth slabs.  Lists and image against the oracle."""
    from egogaussian_amd import _C
    dev = _dev()
    if layout == "every-tile":
        N, H, W = 11800, 64, 64
        d = make_inputs(N, H, W, 23, 0, "sh_cov", scale_mul=8.0)
    else:
        N, H, W = 6000, 128, 160
        d = make_inputs(N, H, W, 24, 0, "sh_cov", scale_mul=0.5)
        g = torch.Generator().manual_seed(11)
        m3 = d["means3D"]
        k = 1900
        m3[:k, 0] = 0.01 * torch.randn(k, generator=g); m3[:k, 1] = 0.01 * torch.randn(k, generator=g)
        m3[:k, 2] = 3.0 + 4.0 * torch.rand(k, generator=g)
    o, st = oracle_forward(d)
    lens = (st["ranges"][:, 1] - st["ranges"][:, 0])
    assert ((lens > 1792) & (lens <= 2048)).any(), sorted(lens.tolist())[-8:]
    assert (layout == "every-tile") == (lens.mean() > 2048), float(lens.mean())      # > 2048 on average: both instantiations are launched
    from tests import sort_regimes as sr
    just_over = [i for i in sr.regime_of_tiles(st, st["R"], 0).values() if 1792 < i.n <= 2048]
    want = (8, "one-pass") if layout == "every-tile" else (4, "slabs")
    assert just_over and all((i.inst, i.regime) == want for i in just_over), just_over
    with pinned_capacity(st["R"]):
        retries = _C.stats["retries"]
        g_, out = hip_forward(d, dev)
        assert sort_plan_of(N, W, H, st["R"], retries) == (_C.SORT_SECOND_INSTANTIATION if layout == "every-tile" else _C.SORT_IN_BLEND)
    bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"]); iv = _C.image_views(out[7], W, H)
    assert out[0] == st["R"]
    assert np.array_equal(iv["ranges"].cpu().numpy().view(np.uint32), st["ranges"])
    assert np.array_equal(bv["point_list"].cpu().numpy().view(np.uint32), st["point_list"]), f"longest list {int(lens.max())}"
    assert outlier_fraction(out[1].cpu().numpy(), st["color"], TOL) <= 1e-4


def test_ready_to_pin_harness_runs_against_the_hip_path(tmp_path):
    """tools/compare_upstream_npz.py end to end: reference outputs written by one backend (here the oracle, standing in for a holder
    of the CUDA build), compared with the HIP path through the drop-in module: radii, images, gradients (the lists are compared by the tests above)."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "compare_upstream_npz.py")
    r = subprocess.run([sys.executable, tool, "produce", "--backend", "oracle", "--cases", "A,E,F", "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    r = subprocess.run([sys.executable, tool, "compare", "--ref", str(tmp_path), "--backend", "hip", "--cases", "A,E,F"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.count("PASS") == 3, r.stdout + r.stderr[-1500:]


def test_ballot_rank_fallback_sorts_identically():
    """The per-tile sort has two rankers (LDS-atomic, verified on the device at first use; ballot-based fallback).  A ranker is only called
    by the digit passes: the generic scene (every tile sorted in one pass of buckets and comparisons) shows that the flag changes nothing
    there; the second scene holds tiles with all depths equal, with a pile of distinct depths and with a pile of tied depths
    (tests/sort_regimes.py), where the ranker this test names does the sorting."""
    from egogaussian_amd import _C, lib
    from tests import sort_regimes as sr
    dev = _dev()
    sc, st_r = sr.oracle_state("solo-registers")
    assert sr.reach(sc, st_r, "blend", ballot=True) >= {f"4-solo/blend/{r}" for r in ("equal", "digits", "digits+ties")}      # (outside the model's guard band)
    d = make_inputs(6000, 96, 128, 9, 0, "sh_cov", scale_mul=3.0)
    for d, st in ((d, oracle_forward(d)[1]), (sc.d, st_r)):
        N, H, W = int(st["P"]), d["image_height"], d["image_width"]
        res = []
        for force in (0, 1):
            old = _C.force_ballot_rank(force)                            # (the default of calls that do not say: EGS_CALL_BALLOT_RANK in their flags word)
            try:
                with pinned_capacity(st["R"]):
                    retries = _C.stats["retries"]
                    g, out = hip_forward(d, dev)
                    assert sort_plan_of(N, W, H, st["R"], retries) == _C.SORT_IN_BLEND | (_C.SORT_BALLOT_RANK if force else 0)
            finally:
                _C.force_ballot_rank(old)
            bv = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"])
            res.append(bv["point_list"].cpu().numpy().view(np.uint32)[:st["R"]].copy())
        assert np.array_equal(res[0], st["point_list"]) and np.array_equal(res[1], st["point_list"])


def test_mark_visible_matches_oracle():
    from egogaussian_amd import _C
    from oracle.oracle import Oracle
    dev = _dev()
    d = make_inputs(5000, 64, 64, 3)
    d["means3D"][::3, 2] -= 8.0
    vis = _C.mark_visible(d["means3D"].to(dev), d["viewmatrix"].to(dev), d["projmatrix"].to(dev))
    assert np.array_equal(vis.cpu().numpy(), Oracle(np.float32).mark_visible(d["means3D"], d["viewmatrix"]))


def test_autograd_surface_reaches_all_parameters():
    """render() through the drop-in module: gradients reach xyz, features, scaling, rotation, opacity (mode 1) and
    label (mode 2), as probed for the reference in SURVEY.md appendix A."""
    from egogaussian_amd.scene_synth import make_scene, make_camera, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render, get_render_label
    dev = _dev()
    H, W = 64, 64
    sc = make_scene(1000, H, W, 0); sc["log_scale"] += math.log(3.0)
    pc = SynthGaussians(sc, device=dev)
    cam = make_camera(0, H, W, device=dev)
    bg = torch.zeros(3, device=dev)
    out = render(cam, pc, Pipe, bg)
    assert out["render"].shape == (3, H, W) and out["depth"].shape == (1, H, W) and out["alpha"].shape == (1, H, W)
    assert out["radii"].dtype == torch.int32 and out["visibility_filter"].dtype == torch.bool
    assert torch.equal(out["visibility_filter"], out["radii"] > 0) and 0 < int(out["visibility_filter"].sum()) < 1000
    (out["render"].sum() + out["alpha"].sum()).backward()
    for p in (pc._xyz, pc._features_dc, pc._scaling, pc._rotation, pc._opacity):
        assert p.grad is not None and float(p.grad.abs().sum()) > 0
    assert out["viewspace_points"].grad is not None and float(out["viewspace_points"].grad[:, 2].abs().sum()) == 0
    lab = get_render_label(cam, pc, bg)
    lab.mean().backward()
    assert float(pc._label.grad.abs().sum()) > 0


def test_image_invariants_at_full_size():
    """Size-independent properties at BASELINE config B/C shape (100k @ 960x540): alpha = 1 - final_T,
    colour(bg) - colour(0) = final_T * bg, sum(tiles_touched) = R, keys sorted, permutation invariance."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 100000, 540, 960
    d = make_inputs(N, H, W, 0, 0, "sh_cov")
    g, out = hip_forward(d, dev)
    R, color, depth, alpha, radii, geom, binning, img = out
    iv = _C.image_views(img, W, H); bv = _C.binning_views(binning, N, R, W, H, _C.stats["capacity"]); gv = _C.geom_views(geom, N)
    assert abs(float((alpha[0] + iv["final_T"] - 1).abs().max())) < 1e-4
    rng = iv["ranges"].cpu().numpy().view(np.uint32); pl = bv["point_list"].cpu().numpy().view(np.uint32)
    tile_of = np.repeat(np.arange(rng.shape[0], dtype=np.uint64), (rng[:, 1] - rng[:, 0]).astype(np.int64))
    keys = (tile_of << np.uint64(52)) | (gv["rec"].cpu().numpy()[pl, 9].view(np.uint32).astype(np.uint64) << np.uint64(20)) | pl
    assert len(keys) == R and np.all(keys[1:] > keys[:-1])          # strictly increasing in (tile, depth, index)
    assert int(gv["offsets"].sum()) == R
    d0 = dict(d); d0["bg"] = torch.zeros(3)
    _, out0 = hip_forward(d0, dev)
    diff = color - out0[1]
    expect = iv["final_T"][None] * d["bg"].to(dev).view(3, 1, 1)
    assert float((diff - expect).abs().max()) < 1e-5
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
    dp = {k: (v[perm] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N else v) for k, v in d.items()}
    _, outp = hip_forward(dp, dev)
    assert outlier_fraction(outp[1].cpu().numpy(), color.cpu().numpy(), 1e-5) < 1e-4


def test_backward_properties_at_full_size():
    """Size-independent properties of the backward at BASELINE config C shape (500k @ 960x540, the benched workload), where the oracle
    is too slow to be the checker of every run: the forward is bit-for-bit repeatable (images AND lists); zero upstream gradients give
    exactly zero gradients; the backward is linear in the upstream gradients (it is a vector-Jacobian product) up to the order of its
    floating-point sums; the colour gradient of a Gaussian no pixel blends is zero."""
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 500000, 540, 960
    d = make_inputs(N, H, W, 0, 0, "sh_cov")
    g, out = hip_forward(d, dev)
    keep = [t.clone() for t in out[1:5]]
    pl = _C.binning_views(out[6], N, out[0], W, H, _C.stats["capacity"])["point_list"].clone()
    g2, out2 = hip_forward(d, dev)
    for a, b in zip(keep, out2[1:5]):
        assert torch.equal(a, b), "two forwards of the same inputs differ"
    assert out2[0] == out[0] and torch.equal(pl, _C.binning_views(out2[6], N, out2[0], W, H, _C.stats["capacity"])["point_list"])
    ga, gb = seeded_grads(H, W, 5), seeded_grads(H, W, 6)
    zero = [torch.zeros_like(x) for x in ga]
    for t in hip_backward(g2, out2, zero, dev):
        assert t.numel() == 0 or float(t.abs().max()) == 0.0, "zero upstream gradients must give zero gradients"
    ra = [t.clone() for t in hip_backward(g2, out2, ga, dev)]
    rb = [t.clone() for t in hip_backward(g2, out2, gb, dev)]
    mix = [2.0 * x - 0.5 * y for x, y in zip(ga, gb)]
    rm = hip_backward(g2, out2, mix, dev)
    for k, (m, a, b) in enumerate(zip(rm, ra, rb)):
        if m.numel():
            want = (2.0 * a.double() - 0.5 * b.double()).cpu().numpy()
            assert rel_err(m.double().cpu().numpy(), want) < 2e-5, f"gradient {k} is not linear in the upstream gradients"
    radii = out2[4]
    dcol = ra[1] if ra[1].numel() else None                          # dL/dcolors (colours precomputed) -- empty in the SH mode
    dsh = ra[5]
    if dsh.numel():
        assert float(dsh[radii == 0].abs().max()) == 0.0, "a culled Gaussian received a colour gradient"
    if dcol is not None:
        assert float(dcol[radii == 0].abs().max()) == 0.0


def test_config_D_1M_gaussians_1080p_depth_alpha_gradcheck():
    """BASELINE.json config 5 shape: 1 M Gaussians, 1920x1080, seeded upstream gradients on colour, depth and alpha;
    every output and gradient against the oracle (OpenMP over tiles on the host cores)."""
    import os
    from egogaussian_amd import _C
    dev = _dev()
    N, H, W = 1_000_000, 1080, 1920
    d = make_inputs(N, H, W, 0, 0, "sh_cov", frame=7, bg=(0.0, 0.0, 0.0))
    o, st = oracle_forward(d, nthreads=min(64, os.cpu_count() or 8))
    g, out = hip_forward(d, dev)
    R, color, depth, alpha, radii, geom, binning, img = out
    assert R == st["R"] and R > 5_000_000
    assert np.array_equal(radii.cpu().numpy(), st["radii"])
    bv = _C.binning_views(binning, N, R, W, H, _C.stats["capacity"])
    assert np.array_equal(bv["point_list"].cpu().numpy().view(np.uint32), st["point_list"])
    iv = _C.image_views(img, W, H)
    assert np.array_equal(iv["ranges"].cpu().numpy().view(np.uint32), st["ranges"])
    flip_px = flip_pixels(color.cpu().numpy(), iv["final_T"].cpu().numpy(), st, iv["n_contrib"].cpu().numpy().view(np.uint32))
    print("  D images: " + check_images_isolating_flips((("color", color.cpu().numpy(), st["color"]), ("depth", depth.cpu().numpy(), st["depth"]),
                                                         ("alpha", alpha.cpu().numpy(), st["alpha"])), st, flip_px, TOL, what="config D"))
    grads = seeded_grads(H, W, 99)
    hb = hip_backward(g, out, grads, dev)
    gb = o.backward(st, *grads)
    rep, _, _ = check_grads_isolating_flips(["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh"], hb, gb, st, flip_px, TOL, what="config D")
    print("  D: " + rep)


def test_training_psnr_matches_oracle_training():
    """The product chain on the GPU (fused cov3D, HIP rasterizer, fused loss, FusedAdam) and the oracle chain on the CPU
    (torch cov3D, differentiable torch rasterizer, torch loss, torch Adam) trained for the same seeded steps end within
    0.05 dB of each other (BASELINE.json: PSNR within 0.05 dB of the reference path)."""
    import random
    from egogaussian_amd.scene_synth import make_scene, make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    from egogaussian_amd.fused import l1_ssim_loss
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.losses import training_loss, psnr
    from oracle.raster_torch import rasterize_torch
    dev = _dev()
    N, H, W, K = 400, 48, 64, 12
    teacher = make_scene(N, H, W, seed=3); teacher["log_scale"] += math.log(4.0)
    student = perturb_student(teacher)
    frames = [0, 40, 80, 120]
    lrs = dict(xyz=1.6e-3, f=2.5e-3, op=0.05, sc=5e-3, rot=1e-3)

    def groups(pc):
        return [{"params": [pc._xyz], "lr": lrs["xyz"]}, {"params": [pc._features_dc], "lr": lrs["f"]},
                {"params": [pc._opacity], "lr": lrs["op"]}, {"params": [pc._scaling], "lr": lrs["sc"]},
                {"params": [pc._rotation], "lr": lrs["rot"]}]

    def cpu_render(cam, pc, bg):
        col, _, _, _, _ = rasterize_torch(means3D=pc.get_xyz, opacities=pc.get_opacity, shs=pc.get_features,
                                          cov3D_precomp=pc.get_covariance(), viewmatrix=cam.world_view_transform,
                                          projmatrix=cam.full_proj_transform, campos=cam.camera_center, bg=bg, image_height=H,
                                          image_width=W, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2))
        return col

    results = {}
    for side in ("gpu", "cpu"):
        d = dev if side == "gpu" else "cpu"
        cams = [make_camera(k, H, W, device=d) for k in frames]
        bg = torch.zeros(3, device=d)
        with torch.no_grad():
            tpc = SynthGaussians(teacher, device=d, requires_grad=False)
            gts = [(render(c, tpc, Pipe, bg)["render"] if side == "gpu" else cpu_render(c, tpc, bg)).clone() for c in cams]
        pc = SynthGaussians(student, device=d)
        opt = FusedAdam(groups(pc), lr=0.0, eps=1e-15) if side == "gpu" else torch.optim.Adam(groups(pc), lr=0.0, eps=1e-15)
        rnd = random.Random(0)
        for it in range(K):
            k = rnd.randrange(len(cams))
            img = render(cams[k], pc, Pipe, bg)["render"] if side == "gpu" else cpu_render(cams[k], pc, bg)
            loss = l1_ssim_loss(img, gts[k], 0.2) if side == "gpu" else training_loss(img, gts[k], 0.2)
            loss.backward(); opt.step(); opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            ps = [psnr((render(c, pc, Pipe, bg)["render"] if side == "gpu" else cpu_render(c, pc, bg))[None], g[None]).item()
                  for c, g in zip(cams, gts)]
        results[side] = (float(np.mean(ps)), gts[0].cpu())
    print(f"\n  PSNR after {K} steps: gpu {results['gpu'][0]:.4f} dB, oracle chain {results['cpu'][0]:.4f} dB")
    assert rel_err(results["gpu"][1].numpy(), results["cpu"][1].numpy()) < 1e-4       # same ground truth on both sides
    assert abs(results["gpu"][0] - results["cpu"][0]) <= 0.05


def test_integration_md_ctypes_stub_runs_as_written():
    """The binding shown in INTEGRATION.md section 2 is executed verbatim (only the library path is substituted) and must give
    the same forward result as the package's own _C module."""
    import os, re
    from egogaussian_amd import lib
    dev = _dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    block = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "def rasterize_forward" in b]
    assert len(block) == 1
    lib.load()
    ns = {}
    exec(block[0].replace('"libegs_raster.so"', repr(lib.library_path())), ns)
    d = make_inputs(3000, 70, 100, 1, 0, "sh_cov", scale_mul=3.0)
    with tile_culling(True):
        g, out = hip_forward(d, dev)
        R, color, depth, alpha, radii, geom, binning, img = ns["rasterize_forward"](
            g["bg"], g["means3D"], g["opacities"], g["shs"], g["cov3D_precomp"], g["viewmatrix"], g["projmatrix"], g["campos"],
            g["tanfovx"], g["tanfovy"], 70, 100, 0)
    torch.cuda.synchronize()
    assert R == out[0] and torch.equal(color, out[1]) and torch.equal(depth, out[2]) and torch.equal(alpha, out[3]) and torch.equal(radii, out[4])


def test_degenerate_inputs_terminate_and_stay_bounded():
    """NaN / inf positions, zero and huge scales, opacity 0 and 1: the launch chain must terminate with a bounded instance count
    (every rectangle is clamped to the tile grid) and leave the pixels no degenerate splat reaches finite; forward and backward."""
    dev = _dev()
    N, H, W = 4000, 64, 96
    d = make_inputs(N, H, W, 21, 0, "sh_sr", scale_mul=2.0)
    m = d["means3D"]
    m[0] = float("nan"); m[1, 0] = float("inf"); m[2, 2] = float("-inf"); m[3] = 0.0
    d["scales"][10:20] = 0.0; d["scales"][20:24] = 1e6; d["scales"][24] = float("nan")
    d["opacities"][30:40] = 0.0; d["opacities"][40:50] = 1.0
    d["rotations"][50:55] = 0.0                                        # zero quaternion
    for cull in (False, True):
        with tile_culling(cull):
            g, out = hip_forward(d, dev)
            hb = hip_backward(g, out, seeded_grads(H, W, 4), dev)
        torch.cuda.synchronize()
        n_tiles = ((H + 15) // 16) * ((W + 15) // 16)
        assert 0 < out[0] <= N * n_tiles
        assert int((out[4] < 0).sum()) == 0                              # radii stay non-negative
        finite = torch.isfinite(out[1]).all(dim=0)
        assert float(finite.float().mean()) > 0.2                        # the NaN / giant splats poison only the pixels they cover
        assert all(t.shape[0] == N for t in hb if t.numel())


@pytest.mark.parametrize("colour_mode", ["sh", "col"])
def test_raw_parameter_mode_matches_activated_inputs(colour_mode):
    """EGS_ACT_*: log-scales, unnormalised quaternions and opacity logits activated inside the preprocess kernel must give
    the images of the call with torch-activated inputs, and gradients that are those of the activated call chained through
    exp / normalize / sigmoid by autograd."""
    raw_parameter_mode_matches_activated_inputs(make_inputs(5000, 96, 128, 13, 0, "sh_sr" if colour_mode == "sh" else "col_sr", scale_mul=2.5), colour_mode)


def raw_parameter_mode_matches_activated_inputs(d, colour_mode):
    """The body of the test above for one frame (a make_inputs dictionary in a *_sr mode; its scale_modifier is the call's)."""
    from egogaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    dev = _dev()
    N, H, W = int(d["means3D"].shape[0]), d["image_height"], d["image_width"]
    g = _to(d, dev)
    gen = torch.Generator().manual_seed(0)
    raw_s = torch.log(g["scales"]).detach()
    raw_q = (g["rotations"] * (0.5 + 2.0 * torch.rand(N, 1, generator=gen).to(dev))).detach()        # any positive multiple of a unit quaternion
    raw_o = torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)).detach()
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=g["tanfovx"], tanfovy=g["tanfovy"], bg=g["bg"],
                                       scale_modifier=g["scale_modifier"], viewmatrix=g["viewmatrix"], projmatrix=g["projmatrix"],
                                       sh_degree=g["sh_degree"], campos=g["campos"], prefiltered=False, debug=False)
    grads = [t.to(dev) for t in seeded_grads(H, W, 3)]
    res = []
    for raw in (False, True):
        s, q, o = [t.clone().requires_grad_(True) for t in (raw_s, raw_q, raw_o)]
        xyz = g["means3D"].clone().requires_grad_(True)
        kw = dict(shs=g["shs"]) if colour_mode == "sh" else dict(colors_precomp=g["colors_precomp"])
        if raw:
            out = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=o, scales=s, rotations=q, raw_parameters=True, **kw)
        else:
            out = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=torch.sigmoid(o), scales=torch.exp(s),
                                         rotations=torch.nn.functional.normalize(q), **kw)
        color, radii, depth, alpha = out
        ((color * grads[0]).sum() + (depth * grads[1]).sum() + (alpha * grads[2]).sum()).backward()
        res.append((color.detach(), depth.detach(), alpha.detach(), radii, xyz.grad, s.grad, q.grad, o.grad))
    a, b = res
    assert float((a[3] != b[3]).float().mean()) < 1e-3                   # radii: the activations differ in the last ulp at most
    for k, name in ((0, "colour"), (1, "depth"), (2, "alpha")):
        assert outlier_fraction(b[k].cpu().numpy(), a[k].cpu().numpy(), TOL) <= 1e-4, name
    for k, name in ((4, "d/dxyz"), (5, "d/dlog-scale"), (6, "d/dquat"), (7, "d/dlogit")):
        assert outlier_fraction(b[k].cpu().numpy(), a[k].cpu().numpy(), 2e-4) <= 2e-4, name
        assert rel_err(b[k].cpu().numpy(), a[k].cpu().numpy()) < 5e-3, name
    with pytest.raises(Exception, match="raw_parameters"):
        GaussianRasterizer(rs)(means3D=g["means3D"], means2D=g["means3D"], opacities=raw_o, cov3D_precomp=torch.zeros(N, 6, device=dev),
                               raw_parameters=True, **kw)


@pytest.mark.parametrize("active,M", [(0, 16), (1, 16), (2, 9), (3, 16), (1, 4)])
def test_split_spherical_harmonics_match_the_concatenated_call(active, M):
    """shs=(features_dc, features_rest) -- the two tensors the reference's model stores -- must give the bits of shs=torch.cat(...)
    (same kernels, other addressing) with the gradient arriving already split (equal up to the order of the blend's float atomics); coefficients above the active degree get zeros.
    Also with a base address that is not 16-byte aligned (scalar path of the row transposition) and against the oracle's dL/dSH."""
    from egogaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    dev = _dev()
    N, H, W = 5003, 96, 128                                            # not a multiple of 64: ragged last wave
    deg_full = {4: 1, 9: 2, 16: 3}[M]
    d = make_inputs(N, H, W, 21, deg_full, "sh_cov", scale_mul=2.5)
    d["sh_degree"] = active
    g = _to(d, dev)
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=g["tanfovx"], tanfovy=g["tanfovy"], bg=g["bg"],
                                       scale_modifier=g["scale_modifier"], viewmatrix=g["viewmatrix"], projmatrix=g["projmatrix"],
                                       sh_degree=active, campos=g["campos"], prefiltered=False, debug=False)
    grads = [t.to(dev) for t in seeded_grads(H, W, 5)]
    res = {}
    for how in ("cat", "split", "split-unaligned"):
        xyz = g["means3D"].clone().requires_grad_(True)
        if how == "split-unaligned":
            store = torch.zeros(N * (M - 1) * 3 + 1, device=dev)
            store[1:] = g["shs"][:, 1:].reshape(-1)
            rest = store[1:].view(N, M - 1, 3).detach().requires_grad_(True)
            assert rest.data_ptr() % 16 == 4
        else:
            rest = g["shs"][:, 1:].clone().requires_grad_(True)
        dc = g["shs"][:, :1].clone().requires_grad_(True)
        shs = torch.cat((dc, rest), dim=1) if how == "cat" else (dc, rest)
        color, radii, depth, alpha = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=g["opacities"], shs=shs,
                                                            cov3D_precomp=g["cov3D_precomp"])
        ((color * grads[0]).sum() + (depth * grads[1]).sum() + (alpha * grads[2]).sum()).backward()
        res[how] = (color.detach(), radii, xyz.grad, dc.grad, rest.grad)
    ref = res["cat"]
    for how in ("split", "split-unaligned"):
        for k, name in enumerate(("colour", "radii")):
            assert torch.equal(res[how][k], ref[k]), f"{how}: {name} differs from the concatenated call"
        for k, name in ((2, "d/dxyz"), (3, "d/dfeatures_dc"), (4, "d/dfeatures_rest")):       # (the blend backward sums with float atomics)
            assert res[how][k].shape == ref[k].shape
            assert outlier_fraction(res[how][k].cpu().numpy(), ref[k].cpu().numpy(), 1e-4) <= 1e-4, f"{how}: {name}"
            assert torch.equal(res[how][k] == 0, ref[k] == 0), f"{how}: {name} zero pattern"
    n_active = (active + 1) ** 2
    assert float(ref[4][:, n_active - 1:].abs().max()) == 0.0 if n_active < M else True
    assert float(ref[4][:, :max(n_active - 1, 0)].abs().sum()) > 0 or active == 0
    assert float(ref[3].abs().sum()) > 0
    # the oracle on the same inputs
    o, st = oracle_forward(d)
    gb = o.backward(st, *seeded_grads(H, W, 5))
    full = torch.cat((ref[3], ref[4]), dim=1).cpu().numpy()
    assert outlier_fraction(full, gb["dL_dsh"].reshape(full.shape), TOL) <= 2e-4
    assert outlier_fraction(ref[2].cpu().numpy(), gb["dL_dmeans3D"], TOL) <= 2e-4
    assert outlier_fraction(ref[0].cpu().numpy(), st["color"], TOL) <= 1e-4


def test_indefinite_covariances_are_never_culled():
    """A user-supplied cov3D_precomp that is not positive semi-definite gives an indefinite 2D conic (the reference only rejects
    det == 0): its falloff has no maximum at the clamped edge optimum the ellipse-vs-block test computes, so such a splat must be
    kept everywhere.  Tile culling on and off must still agree bit for bit, and both with the oracle."""
    dev = _dev()
    N, H, W = 3000, 96, 128
    d = make_inputs(N, H, W, 17, 0, "col_cov", scale_mul=3.0)
    cov = d["cov3D_precomp"]
    cov[3::11, 1] = 4.0 * cov[3::11, 0]                # |xy| > sqrt(xx yy): det < 0, trace > 0 (the radius stays a number)
    cov[::7, 4] = -3.0 * cov[::7, 3]                   # same in the yz block
    o, st = oracle_forward(d)
    res = {}
    for cull in (False, True):
        with tile_culling(cull):
            g, out = hip_forward(d, dev)
            hb = hip_backward(g, out, seeded_grads(H, W, 2), dev)
        res[cull] = ([t.clone() for t in out[1:5]], [t.clone() for t in hb])
    assert out[0] == st["R"] and np.array_equal(res[True][0][3].cpu().numpy(), st["radii"])
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b), "tile culling changed an output for an indefinite conic"
    finite = np.isfinite(st["color"]).all(0)
    assert finite.mean() > 0.5
    hipc = res[True][0][0].cpu().numpy()
    assert outlier_fraction(hipc[:, finite], st["color"][:, finite], TOL) <= 1e-3


def test_hip_is_as_close_to_float64_as_the_float32_oracle():
    """Accuracy rather than agreement: the same frame through the oracle in float64 is the yardstick; the HIP path (its own
    summation orders, v_exp_f32, float atomics) must sit as close to it as the float32 oracle does (which follows the published
    order of operations), for the images and for every gradient."""
    from oracle.oracle import Oracle
    dev = _dev()
    N, H, W = 8000, 160, 256
    d = make_inputs(N, H, W, 31, 2, "sh_cov", scale_mul=2.0)
    grads = seeded_grads(H, W, 12)
    o32, st32 = oracle_forward(d)
    d64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}
    o64 = Oracle(np.float64, nthreads=8)
    st64 = o64.forward(**d64)
    g32, g64 = o32.backward(st32, *grads), o64.backward(st64, *[g.double() for g in grads])
    with tile_culling(True):
        g, out = hip_forward(d, dev)
        hb = hip_backward(g, out, grads, dev)
    names = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh"]
    # every row against its own magnitude (the figures below are relative to the array's maximum); set aside: the contributors of the
    # pixels where the HIP path and the float32 oracle took different branches (proven), and of those where the two oracles did
    from egogaussian_amd import _C
    flip_px = flip_pixels(out[1].cpu().numpy(), _C.image_views(out[7], W, H)["final_T"].cpu().numpy(), st32)
    print("\n" + check_grad_rows_vs_float64(names, hb, st32, g32, st64, g64, gaussians_contributing_to(st32, flip_px, 0), what=f"[{N}@{W}x{H}]"))
    rows = [("colour", out[1].cpu().numpy(), st32["color"], st64["color"]), ("depth", out[2].cpu().numpy(), st32["depth"], st64["depth"]),
            ("alpha", out[3].cpu().numpy(), st32["alpha"], st64["alpha"])]
    rows += [(n, h.cpu().numpy().reshape(g64[n].shape), g32[n], g64[n]) for n, h in zip(names, hb)]
    # (pixels where float32 and float64 disagree on a 1/255 or 1e-4 threshold are set aside by the median-free measure below:
    #  the comparison is on the fraction of entries farther than 1e-5 relative from the float64 value)
    print()
    for name, hip, a32, a64 in rows:
        f_hip, f_32 = outlier_fraction(hip, a64, 1e-5), outlier_fraction(a32, a64, 1e-5)
        e_hip, e_32 = rel_err(hip, a64), rel_err(a32, a64)
        print(f"  {name:12s} vs float64: HIP max rel {e_hip:.1e} (entries off by > 1e-5: {f_hip:.1e});  float32 oracle {e_32:.1e} ({f_32:.1e})")
        assert f_hip <= 2.0 * f_32 + 1e-4, name
        assert e_hip <= 3.0 * e_32 + 2e-5, name
