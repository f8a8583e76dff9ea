"""Shared input builders and comparison helpers for the tests (CPU tensors; tests move them as needed)."""
import math

import numpy as np
import torch

from egogaussian_amd.scene_synth import make_scene, make_camera
from tests.cameras import CAMERAS, IN_CLOUD, population, assert_population      # noqa: F401  (re-exported: the general cameras)


def make_inputs(N, H, W, seed=0, sh_degree=0, mode="sh_cov", frame=3, scale_mul=1.0, bg=(0.1, 0.2, 0.3), dtype=torch.float32,
                opacity_shift=0.0, camera=None):
    """Activated rasterizer inputs for S(N,H,W,seed).
    camera: None -> frame `frame` of the orbit (scene_synth.make_camera), scale_modifier 1; a name of tests/cameras.py CAMERAS (or a
            dict of a camera's fields) -> that camera's pose, intrinsics and scale_modifier, the scene's positions re-oriented and
            shifted into its world (`frame` is not read).  In the *_cov modes the modifier goes into the covariance, as the renderer
            puts it there: the rasterizer does not read scale_modifier when it is handed cov3D_precomp.
    mode: 'sh_cov'  -> shs + cov3D_precomp   (training call, /root/reference/gaussian_renderer/__init__.py:90-98)
          'col_sr'  -> colors_precomp + scales/rotations (label call, render_helper.py:61-63)
          'sh_sr'   -> shs + scales/rotations
          'col_cov' -> colors_precomp + cov3D_precomp"""
    sc = make_scene(N, H, W, seed, sh_degree=sh_degree)
    mod = 1.0
    if camera is None:
        cam = make_camera(frame, H, W)
    else:
        from tests.cameras import build_camera, world_positions
        cam, Q, shift, mod = build_camera(camera, H, W)
        sc["xyz"] = world_positions(sc["xyz"], Q, shift)
    t = lambda a: torch.tensor(a, dtype=dtype)
    scales = torch.exp(t(sc["log_scale"])) * scale_mul
    quat = t(sc["quat"])
    d = dict(means3D=t(sc["xyz"]), opacities=torch.sigmoid(t(sc["opacity_logit"]) + opacity_shift),
             viewmatrix=cam.world_view_transform.to(dtype), projmatrix=cam.full_proj_transform.to(dtype),
             campos=cam.camera_center.to(dtype), bg=torch.tensor(bg, dtype=dtype), image_height=H, image_width=W,
             tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2), sh_degree=sh_degree, scale_modifier=mod)
    if mode in ("sh_cov", "sh_sr"):
        d["shs"] = t(sc["features"])
    else:
        rng = np.random.default_rng(seed + 77)
        d["colors_precomp"] = t(rng.uniform(0, 1, (N, 3)).astype(np.float32))
    if mode in ("sh_cov", "col_cov"):
        from egogaussian_amd.covariance import covariance_from_scaling_rotation
        d["cov3D_precomp"] = covariance_from_scaling_rotation(scales, mod, quat).contiguous()
    else:
        d["scales"], d["rotations"] = scales, quat
    return d


def seeded_grads(H, W, seed=5, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(3, H, W, generator=g, dtype=dtype), torch.rand(1, H, W, generator=g, dtype=dtype),
            torch.rand(1, H, W, generator=g, dtype=dtype))


def rel_err(a, b):
    """max |a-b| relative to max |b| (the 'relative fp32' figure of BASELINE.json's north_star)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def outlier_fraction(a, b, rtol):
    """fraction of elements with |a-b| > rtol * max|b|."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) > rtol * (np.abs(b).max() + 1e-30)).mean())


import contextlib


@contextlib.contextmanager
def tile_culling(on):
    """Run a block with the library's tile culling forced on / off (off: internal lists = the reference algorithm's)."""
    from egogaussian_amd import _C
    old = _C.set_tile_culling(on)
    try:
        yield
    finally:
        _C.set_tile_culling(old)


@contextlib.contextmanager
def sort_in_blend(on):
    """Run a block with the per-tile sort inside the forward blend's launch (on, the default) or as launches of its own."""
    from egogaussian_amd import _C
    old = _C.set_sort_in_blend(on)
    try:
        yield
    finally:
        _C.set_sort_in_blend(old)


@contextlib.contextmanager
def fused_count(on):
    """Run a block with the count pass of the bucketing inside the preprocess launch (on, the default with a placement buffer) or as its own launch."""
    from egogaussian_amd import _C
    old = _C.set_fused_count(on)
    try:
        yield
    finally:
        _C.set_fused_count(old)


def check_culled_lists(st, ranges_hip, point_list_hip, H, W):
    """With tile culling on, every tile's list must be the oracle's list with some entries removed (same order), and every
    removed (tile, splat) instance must be one the reference skips at all 256 pixels: alpha < 1/255 or power > 0
    (evaluated here in float64 from the oracle's conic / opacity / centre).  Returns (kept, dropped) instance counts."""
    import numpy as np
    ro, po = st["ranges"].astype(np.int64), st["point_list"]
    rh = ranges_hip.astype(np.int64)
    n_o, n_h = ro[:, 1] - ro[:, 0], rh[:, 1] - rh[:, 0]
    assert np.all(n_h <= n_o)
    assert int(n_h.sum()) == len(point_list_hip[:int(n_h.sum())])
    tile_o = np.repeat(np.arange(len(ro)), n_o)
    tile_h = np.repeat(np.arange(len(rh)), n_h)
    # the HIP ranges are compact and in tile order, like the oracle's
    assert np.array_equal(rh[n_h > 0, 0], (np.cumsum(n_h) - n_h)[n_h > 0])
    key_o = tile_o.astype(np.int64) * (1 << 32) + po.astype(np.int64)          # (tile, splat) is unique
    key_h = tile_h.astype(np.int64) * (1 << 32) + point_list_hip[:len(tile_h)].astype(np.int64)
    kept = np.isin(key_o, key_h)
    assert kept.sum() == len(key_h) and np.array_equal(key_o[kept], key_h), "culled list is not an ordered sub-list of the reference list"
    drop_t, drop_g = tile_o[~kept], po[~kept]
    gx = (W + 15) // 16
    co, xy = st["conic_opacity"].astype(np.float64), st["xy"].astype(np.float64)
    worst = 0.0
    for lo in range(0, len(drop_t), 200000):
        t, g = drop_t[lo:lo + 200000], drop_g[lo:lo + 200000]
        px = (t % gx)[:, None] * 16 + np.arange(16)[None, :]                     # [n,16]
        py = (t // gx)[:, None] * 16 + np.arange(16)[None, :]
        dx = xy[g, 0][:, None, None] - px[:, None, :]                            # [n,1,16]
        dy = xy[g, 1][:, None, None] - py[:, :, None]                            # [n,16,1]
        power = -0.5 * (co[g, 0][:, None, None] * dx * dx + co[g, 2][:, None, None] * dy * dy) - co[g, 1][:, None, None] * dx * dy
        alpha = np.minimum(0.99, co[g, 3][:, None, None] * np.exp(np.minimum(power, 0.0)))
        alpha = np.where((power > 0) | (px[:, None, :] >= W) | (py[:, :, None] >= H), 0.0, alpha)
        worst = max(worst, float(alpha.max()) if alpha.size else 0.0)
    assert worst < (1.0 / 255.0) * (1 + 1e-5), f"a culled instance reaches alpha {worst} >= 1/255 somewhere in its tile"
    return int(kept.sum()), int((~kept).sum())


class OracleRasterize(torch.autograd.Function):
    """The C oracle (forward + analytic backward) as a CPU autograd op, so that an oracle-side TRAINING chain (torch covariance ->
    oracle rasterizer -> torch loss -> torch Adam) can run for hundreds of steps in seconds.  Test infrastructure only.
    Inputs: means3D [N,3], opacities [N,1], shs [N,M,3], cov3D [N,6] (float32 CPU tensors) + a dict of camera / image constants."""

    @staticmethod
    def forward(ctx, means3D, opacities, shs, cov3D, const):
        from oracle.oracle import Oracle
        o = Oracle(np.float32, nthreads=const.get("nthreads", 8))
        st = o.forward(means3D=means3D, opacities=opacities, shs=shs, cov3D_precomp=cov3D, viewmatrix=const["viewmatrix"],
                       projmatrix=const["projmatrix"], campos=const["campos"], bg=const["bg"], image_height=const["H"], image_width=const["W"],
                       tanfovx=const["tanfovx"], tanfovy=const["tanfovy"], sh_degree=const.get("sh_degree", 0))
        ctx.o, ctx.st, ctx.shapes = o, st, (means3D.shape, opacities.shape, shs.shape, cov3D.shape)
        OracleRasterize.last_radii = torch.from_numpy(st["radii"].copy())          # what a trainer reads besides the image (densification)
        return torch.from_numpy(np.ascontiguousarray(st["color"], dtype=np.float32))

    @staticmethod
    def backward(ctx, g_color):
        gb = ctx.o.backward(ctx.st, g_color.contiguous(), None, None)
        OracleRasterize.last_mean2D_grad = torch.from_numpy(np.ascontiguousarray(gb["dL_dmean2D"], dtype=np.float32))   # = viewspace_points.grad
        t = lambda a, s: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(s)
        return (t(gb["dL_dmeans3D"], ctx.shapes[0]), t(gb["dL_dopacity"], ctx.shapes[1]), t(gb["dL_dsh"], ctx.shapes[2]),
                t(gb["dL_dcov3D"], ctx.shapes[3]), None)


def quantize_8bit(img):
    """What a rendered image goes through before the reference's metrics read it back: torchvision.utils.save_image to PNG
    (/root/reference/trainers/eval_metric.py:113-120) = round(255 x) clamped to [0, 255], then / 255 on load."""
    return torch.floor(img * 255.0 + 0.5).clamp(0, 255) / 255.0


# ---- threshold flips: isolate the damage instead of loosening the bar --------------------------------------------------------------
# v_exp_f32 and glibc expf differ in the last place, so a (pixel, splat) pair whose alpha sits within float32 arithmetic's reach of 1/255
# (or whose transmittance sits at 1e-4) is kept on one side and skipped on the other.  Such a pair changes ITS pixel, hence the gradients of
# the splats that contribute to that pixel's chain -- and nothing else.  The parity tests therefore (1) find the pixels that differ by more
# than a detection level far below the parity bar, (2) make every one of them PROVE why (pixel_account below: the float64 re-walk of the
# pixel's chain either bounds what two float32 evaluations of that chain can differ by -- the pixel is then ordinary float noise and stays
# under the 1e-4 bar like every other pixel -- or holds a threshold-adjacent pair -- a flip; anything else fails the test), (3) collect the
# CONTRIBUTORS of the flipped pixels' chains (gaussians_contributing_to: the kept and the threshold-adjacent entries of the same float64
# walk, up to the point where both sides must have stopped -- a few per cent of the pixel's tile list, which is what was set aside through
# round 6), and (4) hold every other Gaussian's gradients and every other pixel to the north star's 1e-4; the few affected rows are bounded
# by a flipped pair's share (2e-3), and how many rows may be set aside at all is capped (check_grads_isolating_flips).  Max-norm bars say
# nothing about rows decades below the array's maximum: check_grad_rows_vs_float64 measures every row against ITS OWN magnitude.
FLIP_DETECT = 2e-6

ALPHA_WINDOW = 1e-5          # least relative half-width around 1/255 in which a pair's alpha may be kept on one side and skipped on the other
T_WINDOW = 1e-9              # least absolute half-width around the 1e-4 transmittance stop (relative 1e-5)
POWER_WINDOW = 1e-6          # least |power| below which the `power > 0` skip may go either way
EPS32 = 2.0 ** -24           # float32 unit roundoff
K_ARITH = 8.0                # roundings that separate two float32 evaluations of one exponent: ~4 per side (dx, dy, three products, two sums;
                             # this library also rounds the conic once more when it pre-scales it by log2 e), each relative to the LARGEST
                             # term of -(A dx^2 + C dy^2) / 2 - B dx dy, not to the sum: for a splat centred hundreds of pixels away the
                             # terms are in the hundreds and the exponent they cancel to is ~ -5


def walk_chain(st, y, x):
    """The float64 re-walk of pixel (y, x)'s chain that pixel_account and gaussians_contributing_to share: per list entry of the pixel's
    tile the exponent, its arithmetic reach r, alpha, whether the entry is kept (power <= 0, alpha >= 1/255), whether it is
    threshold-adjacent (near_a / near_p / near_T), T' after it and that T's accumulated relative error; `end`: the number of entries
    up to and including the one at which BOTH sides must have stopped (`stopped`: whether there is such an entry).  None: empty list."""
    W = st["W"]
    gx = (W + 15) // 16
    t = (y // 16) * gx + x // 16
    ids = st["point_list"][int(st["ranges"][t, 0]):int(st["ranges"][t, 1])].astype(np.int64)
    if ids.size == 0:
        return None
    co = st["conic_opacity"][ids].astype(np.float64)
    dx = st["xy"][ids, 0].astype(np.float64) - float(x)
    dy = st["xy"][ids, 1].astype(np.float64) - float(y)
    ta, tb, tc = 0.5 * co[:, 0] * dx * dx, co[:, 1] * dx * dy, 0.5 * co[:, 2] * dy * dy
    power = -(ta + tc) - tb
    r = K_ARITH * EPS32 * (np.abs(ta) + np.abs(tb) + np.abs(tc) + 1.0)              # per pair: |d power| = |d alpha| / alpha
    alpha = np.minimum(0.99, co[:, 3] * np.exp(np.minimum(power, 50.0)))
    near_p = np.abs(power) <= np.maximum(POWER_WINDOW, r)
    near_a = (power <= np.maximum(POWER_WINDOW, r)) & (np.abs(alpha * 255.0 - 1.0) <= np.maximum(ALPHA_WINDOW, r))
    keep = (power <= 0.0) & (alpha >= 1.0 / 255.0)
    Tp = np.cumprod(np.where(keep, 1.0 - alpha, 1.0))                 # T' after entry j if it is kept
    relT = np.cumsum(np.where(keep, (alpha * r + EPS32) / (1.0 - alpha), 0.0))      # relative error of T' after entry j
    win_T = np.maximum(T_WINDOW, 1e-4 * relT)
    near_T = keep & (np.abs(Tp - 1e-4) <= win_T)
    stop = np.nonzero(keep & (Tp < 1e-4 - win_T))[0]                   # the first entry at which BOTH sides must have stopped
    end = int(stop[0]) + 1 if stop.size else ids.size
    return dict(ids=ids, power=power, r=r, alpha=alpha, keep=keep, near_a=near_a, near_p=near_p, near_T=near_T, Tp=Tp, relT=relT, end=end,
                stopped=bool(stop.size))


def pixel_account(st, y, x):
    """The chain of pixel (y, x) re-walked in FLOAT64 from the oracle's per-Gaussian state (pixel centres, conics, opacities, colours: the
    values both sides share bit for bit; oracle/raster_oracle.c egso_render_forward is the loop).  ->
      cause   : a description of the first pair, at or before the point where both sides must have stopped, at which two float32
                evaluations may take different branches -- alpha within the pair's own arithmetic error (at least ALPHA_WINDOW, relative)
                of 1/255, exponent within it of 0, T' = T (1 - alpha) within the accumulated error (at least T_WINDOW) of 1e-4 -- or None;
      noise_c : what two float32 evaluations that take the SAME branches can differ by in the pixel's colour (absolute, any channel),
      noise_T : ... and in its final transmittance.
    The error model: an exponent is off by at most K_ARITH * EPS32 * (|A dx^2| / 2 + |C dy^2| / 2 + |B dx dy| + 1) =: r_j (absolute, hence
    relative in alpha); T_j by the sum of alpha_k r_k / (1 - alpha_k) over the kept pairs in front; a contribution c alpha T by its
    relative errors added.  Worst case, first order: a pixel that is off by MORE than this with no adjacent pair is a wrong result."""
    w = walk_chain(st, y, x)
    if w is None:
        return None, 0.0, 0.0
    ids, power, r, alpha, keep, Tp, relT, end = w["ids"], w["power"], w["r"], w["alpha"], w["keep"], w["Tp"], w["relT"], w["end"]
    cause = None
    for name, m in (("alpha", w["near_a"]), ("T'", w["near_T"]), ("power", w["near_p"])):
        j = np.nonzero(m[:end])[0]
        if j.size:
            j = int(j[0])
            cause = (f"{name} threshold: list entry {j} (Gaussian {int(ids[j])}) alpha*255 = {alpha[j] * 255.0:.9f}, power = {power[j]:.3e}, T' = {Tp[j]:.6e}, "
                     f"arithmetic reach {r[j]:.1e}, accumulated in T {relT[j]:.1e}")
            break
    # noise of a chain that takes the same branches on both sides (entries before the stop only)
    n = end if not w["stopped"] else end - 1                           # the stopping entry itself does not contribute
    k = keep[:n]
    T_before = np.concatenate([[1.0], Tp[:-1]])[:n]
    relT_before = np.concatenate([[0.0], relT[:-1]])[:n]
    cmax = np.abs(st["rgb"][ids[:n]].astype(np.float64)).max(1) if "rgb" in st else np.ones(n)
    noise_c = float(np.sum(np.where(k, cmax * alpha[:n] * T_before * (r[:n] + relT_before + 2 * EPS32), 0.0)))
    T_fin = float(Tp[n - 1]) if n else 1.0
    rel_fin = float(relT[n - 1]) if n else 0.0
    noise_c += float(np.abs(st["bg"]).max()) * T_fin * rel_fin if "bg" in st else 0.0
    return cause, noise_c, T_fin * rel_fin


def flip_cause(st, y, x):
    """The threshold-adjacent pair of pixel (y, x), or None (see pixel_account)."""
    return pixel_account(st, y, x)[0]


def flip_pixels(color_hip, final_T_hip, st, n_contrib_hip=None, justify=True, report=None):
    """bool[H,W]: pixels whose colour, final transmittance or (reference lists only) contributor count differ from the oracle's because a
    (pixel, splat) pair went the other way at one of the compositing loop's three thresholds -- PROVEN per pixel.  Every pixel that is off
    by more than FLIP_DETECT is put through pixel_account(): it is a flip when its float64 chain holds a threshold-adjacent pair; it is
    float noise (NOT in the returned mask: it answers to the 1e-4 bar like every other pixel, and relaxes no Gaussian's bound) when it has
    no such pair but is off by no more than what two float32 evaluations of that chain can differ by; otherwise the call fails: a pixel
    that is off with neither is a wrong blend, whatever the fraction ('the flip rule excuses without proving cause').
    report: a dict that receives the counts (detected, flips, noise) and the largest noise bound used."""
    c = np.asarray(color_hip, dtype=np.float64); T = np.asarray(final_T_hip, dtype=np.float64)
    cscale = max(float(np.abs(st["color"]).max()), 1e-30)
    dc = np.abs(c - st["color"]).max(0); dT = np.abs(T - st["final_T"])
    px = (dc > FLIP_DETECT * cscale) | (dT > FLIP_DETECT)
    if n_contrib_hip is not None:
        dn = np.asarray(n_contrib_hip) != st["n_contrib"]
        px = px | dn
    if not justify or not px.any():
        if report is not None:
            report.update(detected=int(px.sum()), flips=int(px.sum()), noise=0, max_noise_bound=0.0)
        return px
    flips = np.zeros_like(px)
    bad, n_noise, worst_bound = [], 0, 0.0
    for y, x in np.argwhere(px):
        cause, noise_c, noise_T = pixel_account(st, int(y), int(x))
        if cause is not None:
            flips[y, x] = True
        elif (n_contrib_hip is None or not dn[y, x]) and dc[y, x] <= FLIP_DETECT * cscale + noise_c and dT[y, x] <= FLIP_DETECT + noise_T:
            n_noise += 1
            worst_bound = max(worst_bound, noise_c / cscale, noise_T)
        else:
            bad.append((int(y), int(x), float(dc[y, x]), float(dT[y, x]), f"float32 reach of this chain: colour {noise_c:.2e}, T {noise_T:.2e}"))
    if report is not None:
        report.update(detected=int(px.sum()), flips=int(flips.sum()), noise=n_noise, max_noise_bound=worst_bound)
    assert not bad, (f"{len(bad)} of {int(px.sum())} pixels differ from the oracle by more than the detection level ({FLIP_DETECT:g} of the image maximum) AND by more than "
                     f"two float32 evaluations of their chain can, with NO threshold-adjacent pair in the float64 chain -- neither flips nor float noise: "
                     f"(y, x, colour diff, final_T diff, reach) {bad[:8]}")
    return flips


def check_images_isolating_flips(images, st, flip_px, tol=1e-4, share=2e-2, what=""):
    """The image-sized outputs ((name, hip array, oracle array) triples) against the oracle: every pixel that is not a (justified) flipped
    pixel within `tol` of the plane's maximum -- asserted, no fraction is excused --, the flipped ones within one threshold-level
    contribution (`share`).  -> report string."""
    rep = []
    for name, hip, ora in images:
        h = np.asarray(hip, dtype=np.float64).reshape(-1, *flip_px.shape); o = np.asarray(ora, dtype=np.float64).reshape(h.shape)
        scale = float(np.abs(o).max()) + 1e-30
        err = np.abs(h - o).max(0) / scale
        e_far = float(np.where(flip_px, 0.0, err).max()) if err.size else 0.0
        e_near = float(err[flip_px].max()) if flip_px.any() else 0.0
        assert e_far < tol, f"{what} {name}: max rel err {e_far} at pixel {np.unravel_index(int(np.argmax(np.where(flip_px, 0.0, err))), err.shape)} away from every flipped pixel"
        assert e_near < share, f"{what} {name}: max rel err {e_near} on a flipped pixel"
        rep.append(f"{name} {e_far:.1e}" + (f" (flipped pixels {e_near:.1e})" if flip_px.any() else ""))
    return "; ".join(rep)


def _grow(px_mask, halo):
    """(ys, xs) of the mask's pixels and of every pixel within `halo` of one (clipped to the image, each pixel once)."""
    H, W = px_mask.shape
    ys, xs = np.nonzero(px_mask)
    if halo and ys.size:
        dy, dx = np.meshgrid(np.arange(-halo, halo + 1), np.arange(-halo, halo + 1), indexing="ij")
        ys = np.clip(ys[:, None] + dy.reshape(1, -1), 0, H - 1).reshape(-1)
        xs = np.clip(xs[:, None] + dx.reshape(1, -1), 0, W - 1).reshape(-1)
        flat = np.unique(ys * W + xs)
        ys, xs = flat // W, flat % W
    return ys, xs


def gaussians_in_flipped_tiles(st, flip_px, halo=0):
    """ids of the Gaussians in the oracle's lists of the tiles that hold a flipped pixel: the set that was excused through round 6.  Kept
    for the printed ratio and the cap of check_grads_isolating_flips only; what IS set aside is gaussians_contributing_to.  halo: as there."""
    W = flip_px.shape[1]
    gx = (W + 15) // 16
    ys, xs = _grow(flip_px, halo)
    tiles = np.unique((ys // 16) * gx + xs // 16)
    if tiles.size == 0:
        return np.zeros(0, dtype=np.int64)
    rng, pl = st["ranges"], st["point_list"]
    return np.unique(np.concatenate([pl[int(rng[t, 0]):int(rng[t, 1])] for t in tiles]).astype(np.int64))


def gaussians_contributing_to(st, px_mask, halo=0):
    """ids of the Gaussians whose gradients a change in the chains of the mask's pixels can reach: per pixel the float64 re-walk of
    pixel_account (walk_chain), and of it the entries up to the point where BOTH sides must have stopped that are kept (power <= 0,
    alpha >= 1/255) or threshold-adjacent (near_a / near_p / near_T: kept on one side only).  An entry of the tile's list that is
    neither contributes nothing to this pixel on either side, so nothing that happens in this pixel can move its gradients.
    halo: pixels around a pixel of the mask that count too -- when the upstream image gradient comes from a loss with a window (SSIM,
    11x11, forward and backward: 10), a flipped pixel changes the upstream gradient of its neighbours."""
    out = []
    for y, x in zip(*_grow(px_mask, halo)):
        w = walk_chain(st, int(y), int(x))
        if w is None:
            continue
        e = w["end"]
        m = (w["keep"] | w["near_a"] | w["near_p"] | w["near_T"])[:e]
        out.append(w["ids"][:e][m])
    return np.unique(np.concatenate(out)) if out else np.zeros(0, dtype=np.int64)


ARBITER_MIN_RADIUS = 36      # px: splats from this size on sum >= 4 000 pixel terms per gradient entry (tests/fuzz_parity.py uses the same size)
NEAR_SHARE = 2e-3            # bound on a row set aside next to a proven flip: 3.2 x the worst such row on record (6.2e-4, profiles/r6_parity_log.txt:98)
SET_ASIDE_OF_TILE_LISTS = 0.5    # cap: rows set aside / rows the tile-list rule would have set aside (CPU-measured: 0.05-0.07 at config C size, 0.18-0.48 at 20000@480x270)
SET_ASIDE_OF_MODEL = 0.01        # cap, models of 100 000 Gaussians and more: rows set aside / N (CPU-measured: 0.51 % at config C size with halo 10)


class FarRowOverBar(AssertionError):
    """check_grads_isolating_flips: a row that contributes to no flipped pixel missed the bar (the one failure a caller may put to the
    float64 oracle; a set-aside row over its share and a cap on the set-aside count are plain AssertionErrors)."""


def check_grads_isolating_flips(names, hip_grads, oracle_grads, st, flip_px, tol=1e-4, share=NEAR_SHARE, what="", halo=0, far_frac=0.0, far_cap=3.0, over_rows=None,
                                near_out=None, arbiter=None):
    """Every gradient array (one row per Gaussian) against the oracle: rows of Gaussians that contribute to no flipped pixel's chain
    within `tol` of the array's maximum (the north star's bar, asserted; "relative" is max-norm relative: |hip - oracle| over the largest
    |oracle| entry of the array), the contributors of the flipped pixels (gaussians_contributing_to) within `share`.  How many rows may be
    set aside is a condition of the test, not a measurement: at most half of what the tile-list rule of rounds 5-6 set aside for the
    same pixels and halo, and at most 1 % of a model of 100 000 Gaussians or more.
    -> (report string, worst unaffected error, number of Gaussians set aside).
    over_rows: a dict that receives, per array name, the rows far from every flip that sit between tol and far_cap x tol (the caller then
    has to account for each of them: tests/test_gpu_bench_mode.py does so with repeated runs and the float64 oracle).
    near_out: a list that receives the ids that were set aside (for check_grad_rows_vs_float64).
    arbiter: a callable -> the float64 oracle's gradients of the same frame (called only when needed).  The tile-list rule set aside, by
    accident, every splat that fills the screen (it is in every tile's list); the contributor rule does not, and on such a row -- half
    a million signed pixel terms -- the FLOAT32 ORACLE's own sum moves by 1-4e-4 of the array's maximum with the order its threads
    reach the tiles in (trained scene, Gaussian 119933, radius 3 565 px, dL/dmeans3D z: float64 62.859, this library 62.864, float32
    oracle 61.43 / 61.48 / 61.67 / 60.49 with 1 / 8 / 64 / 8 threads).  A row that the tile-list rule held to 5e-2 and that misses the
    bar against the float32 oracle is therefore put to the float64 one, by the rule of tests/test_gpu_offscreen.py: within `tol` of the
    float64 value, or within twice the float32 oracle's own distance from it -- else it fails as before.  The row itself has to be of that
    kind: a radius of ARBITER_MIN_RADIUS px or more (>= 4 000 pixel terms, the size from which tests/fuzz_parity.py grants a float32 sum
    its order noise); and so that no row is held to less than it was, it also has to be one the tile-list rule had set aside.  No
    other row is arbitrated.  An arbitrated row counts in the returned `worst` with its distance from the FLOAT64 oracle."""
    near = gaussians_contributing_to(st, flip_px, halo)
    in_tiles = gaussians_in_flipped_tiles(st, flip_px, halo)
    if near_out is not None:
        near_out.append(near)
    counts = f"flipped pixels {int(flip_px.sum())}, Gaussians set aside (contributors / tile lists) {near.size} / {in_tiles.size}"
    assert near.size <= SET_ASIDE_OF_TILE_LISTS * in_tiles.size, f"{what}: {counts}: more than {SET_ASIDE_OF_TILE_LISTS:g} of the tile lists' Gaussians set aside"
    n_model = int(st["P"]) if "P" in st else int(np.asarray(st["radii"]).shape[0])
    if n_model >= 100_000:
        assert near.size <= SET_ASIDE_OF_MODEL * n_model, f"{what}: {counts}: more than {SET_ASIDE_OF_MODEL:.0%} of the model's {n_model} Gaussians set aside"
    rep, worst = [], 0.0
    for name, h in zip(names, hip_grads):
        ora = oracle_grads.get(name) if isinstance(oracle_grads, dict) else None
        if ora is None or h is None or (hasattr(h, "numel") and h.numel() == 0):
            continue
        hh = (h.detach().cpu().numpy() if hasattr(h, "detach") else np.asarray(h)).reshape(ora.shape).astype(np.float64)
        oo = np.asarray(ora, dtype=np.float64)
        scale = float(np.abs(oo).max()) + 1e-30
        row_err = np.abs(hh - oo).reshape(oo.shape[0], -1).max(1) / scale
        mask = np.zeros(oo.shape[0], dtype=bool); mask[near[near < oo.shape[0]]] = True
        e_far = float(row_err[~mask].max()) if (~mask).any() else 0.0
        e_near = float(row_err[mask].max()) if mask.any() else 0.0
        rep.append(f"{name} {e_far:.1e}" + (f" (near flips {e_near:.1e})" if mask.any() else ""))
        # Rows away from every proven flip: the bar itself, no fraction excused (far_frac = 0).  (Through round 5 one row in 100 000 was let
        # through up to 3 x the bar as "fp32 accumulation order"; round 6 traced every such row of the benched-mode test to an L1 sign tie --
        # a threshold of the LOSS, now found and proven like the compositing loop's own -- and the suite has used the allowance nowhere since.
        # A caller that passes far_frac > 0 gets the rows back in `over_rows` and has to account for each.)
        far_err = np.where(mask, 0.0, row_err)
        cand = np.zeros(0, dtype=np.int64)
        if arbiter is not None:
            cand = np.nonzero((far_err >= tol) & (np.asarray(st["radii"])[:oo.shape[0]] >= ARBITER_MIN_RADIUS) & np.isin(np.arange(oo.shape[0]), in_tiles))[0]
        if cand.size:
            g64 = arbiter()
            a64 = np.asarray(g64[name], dtype=np.float64).reshape(oo.shape)
            e64 = np.abs(hh - a64).reshape(oo.shape[0], -1).max(1)[cand] / scale
            e_o = np.abs(oo - a64).reshape(oo.shape[0], -1).max(1)[cand] / scale
            ok = e64 <= np.maximum(tol, 2.0 * e_o)
            rep[-1] += " [" + "; ".join(f"row {int(i)} (radius {int(st['radii'][i])}) {row_err[i]:.1e} from the float32 oracle, which is {b:.1e} from the float64 one; this row "
                                        f"{a:.1e} from it{'' if k else ': NOT ACCOUNTED FOR'}" for i, a, b, k in zip(cand, e64, e_o, ok)) + "]"
            far_err[cand[ok]] = 0.0
            e_far = float(far_err.max())
            worst = max(worst, float(e64[ok].max()) if ok.any() else 0.0)      # (an accounted row stands with its distance from the float64 oracle)
        worst = max(worst, e_far)
        n_over = int((far_err >= tol).sum())
        if n_over > int(far_frac * oo.shape[0]) or (n_over and float(far_err.max()) >= far_cap * tol):
            i = int(np.argmax(far_err))
            raise FarRowOverBar(f"{what} {name}: max rel err {e_far} on Gaussian {i} (hip {hh[i].ravel()[:4]}, oracle {oo[i].ravel()[:4]}, array max {scale:.3e}), "
                                 f"a contributor to no flipped pixel ({int(flip_px.sum())} flipped pixels at {np.argwhere(flip_px)[:12].tolist()}, {near.size} Gaussians contribute to them; "
                                 f"radius {int(st['radii'][i])}, centre {st['xy'][i].tolist()}); {n_over} rows over {tol:g}")
        if n_over:
            rep[-1] += f" [{n_over} row(s) of {oo.shape[0]} between {tol:g} and {far_cap * tol:g}: to be accounted for by the caller]"
            if over_rows is not None:
                over_rows[name] = np.nonzero(far_err >= tol)[0]
        if not e_near < share:
            i = int(np.argmax(np.where(mask, row_err, -1.0)))
            causes = [f"pixel ({int(y)}, {int(x)}): {flip_cause(st, int(y), int(x))}" for y, x in np.argwhere(flip_px)[:6]]
            raise AssertionError(f"{what} {name}: max rel err {e_near} (bound {share:g}) on Gaussian {i}, a contributor to a flipped pixel's chain (hip {hh[i].ravel()[:4]}, "
                                 f"oracle {oo[i].ravel()[:4]}, array max {scale:.3e}; radius {int(st['radii'][i])}, centre {st['xy'][i].tolist()}); " + "; ".join(causes))
    return "; ".join(rep) + "; " + counts, worst, int(near.size)


# ---- every row against its OWN magnitude, float64 as the reference ------------------------------------------------------------------
ROW_TAUS = (1e-3, 1e-2)      # tail thresholds of the per-row relative error
ROW_Q_FACTOR = 3.0           # subject quantiles <= 3 x the float32 oracle's (the factor test_hip_is_as_close_to_float64_as_the_float32_oracle uses for max-norm)
ROW_TAIL_FACTOR = 2.0        # subject tail counts <= 2 x the float32 oracle's (that test's factor for its outlier fractions) ...
ROW_TAIL_SLACK = 3           # ... + 3 rows: one ill-conditioned (cancelling) row must not fail an array whose baseline is zero
ROW_EXCLUDED_CAP = 0.02      # excluded rows / visible rows


def state_disagreement_pixels(st32, st64):
    """bool[H,W]: pixels where the float32 and the float64 oracle took different branches -- n_contrib differs, or final_T is off by
    more than 10 x FLIP_DETECT.  Their contributors' float64 gradients are those of ANOTHER chain, hence no yardstick for a float32 path."""
    return (np.asarray(st32["n_contrib"]) != np.asarray(st64["n_contrib"])) | \
           (np.abs(np.asarray(st32["final_T"], dtype=np.float64) - np.asarray(st64["final_T"], dtype=np.float64)) > 10.0 * FLIP_DETECT)


def row_errors(a, ref64, rows):
    """e_i = max_c |a[i,c] - ref64[i,c]| / max_c |ref64[i,c]| for the given rows (ref64 rows must not be all zero)."""
    n = ref64.shape[0]
    a = np.asarray(a, dtype=np.float64).reshape(n, -1)[rows]; b = np.asarray(ref64, dtype=np.float64).reshape(n, -1)[rows]
    return np.abs(a - b).max(1) / np.abs(b).max(1)


def row_rule(e_s, evals):
    """The state-free core of check_grad_rows_vs_float64 (tests/anchors.py holds kernels without a rasterizer state to it): the per-row
    errors of the subject (e_s) against those of one or more float32 yardstick evaluations (evals, same rows, same float64 reference).
    -> (subject q50/q90, yardstick q50/q90, subject tail counts, yardstick tail counts, the list of violated conditions):
      * q50 and q90: subject <= ROW_Q_FACTOR x yardstick (the larger of the evaluations);
      * for tau in ROW_TAUS: #{e > tau}: subject <= ROW_TAIL_FACTOR x yardstick + ROW_TAIL_SLACK rows."""
    q_s = np.quantile(e_s, [0.5, 0.9])
    q_o = np.max([np.quantile(e, [0.5, 0.9]) for e in evals], axis=0)
    c_s = [int((e_s > tau).sum()) for tau in ROW_TAUS]
    c_o = [max(int((e > tau).sum()) for e in evals) for tau in ROW_TAUS]
    bad = []
    for q, a, b in (("q50", q_s[0], q_o[0]), ("q90", q_s[1], q_o[1])):
        if not a <= ROW_Q_FACTOR * b:
            bad.append(f"{q} {a:.2e} > {ROW_Q_FACTOR:g} x {b:.2e}")
    for tau, cs, co in zip(ROW_TAUS, c_s, c_o):
        if cs > ROW_TAIL_FACTOR * co + ROW_TAIL_SLACK:
            bad.append(f"{cs} rows over {tau:g} > {ROW_TAIL_FACTOR:g} x {co} + {ROW_TAIL_SLACK}")
    return q_s, q_o, c_s, c_o, bad


def check_grad_rows_vs_float64(names, subject_grads, st32, g32, st64, g64, near_ids, what="", g32_alt=None, record=None):
    """Max-norm bars divide by the largest entry of the array; a splatting backward has rows decades below it, which such a bar does
    not see.  Here every row answers to ITS OWN magnitude, with the float64 oracle as the reference and the float32 oracle's distance
    to it as the yardstick (never the subject's own numbers).
    Rows measured, per array: radii > 0, float64 row not all zero, not in `near_ids` (the caller's set-aside rows: contributors of the
    subject's proven flips) and not a contributor (gaussians_contributing_to, halo 0) to a pixel where the float32 and float64 oracle
    states disagree (state_disagreement_pixels).  e_i = max_c |subject[i,c] - g64[i,c]| / max_c |g64[i,c]|; the same for g32.  Asserted:
      * q50 and q90 of e_i: subject <= 3 x float32 oracle (a systematic small bias on every row);
      * for tau in (1e-3, 1e-2): #{e_i > tau}: subject <= 2 x float32 oracle + 3 rows (rows that are plainly wrong, however cold);
      * rows with radii == 0 equal the oracle's (zero);
      * the excluded rows are at most 2 % of the visible rows.
    g32_alt: a dict name -> list of further float32-oracle evaluations of the same gradients in another summation order; the yardstick's
    counts and quantiles are then the larger of the evaluations per array (said in the report).
    record: a dict that receives the figures per array.  -> report string; on failure the ten worst rows and a per-decade table."""
    N = int(st32["P"])
    radii = np.asarray(st32["radii"])
    vis = radii > 0
    dis_px = state_disagreement_pixels(st32, st64)
    dis_ids = gaussians_contributing_to(st32, dis_px, 0)
    excl = np.zeros(N, dtype=bool)
    excl[np.asarray(near_ids, dtype=np.int64)] = True
    excl[dis_ids] = True
    n_vis, n_excl = int(vis.sum()), int((excl & vis).sum())
    head = (f"{what} rows vs float64: {n_vis} visible, {n_excl} excluded ({int(np.asarray(near_ids).size)} near the subject's flips, {dis_ids.size} contributors of the "
            f"{int(dis_px.sum())} pixels where the float32 and float64 oracles disagree)")
    fails, rep = [], [head]
    if n_excl > ROW_EXCLUDED_CAP * n_vis:
        fails.append(f"{n_excl} of {n_vis} visible rows excluded: more than {ROW_EXCLUDED_CAP:.0%}")
    for name, sg in zip(names, subject_grads):
        a64 = g64.get(name) if isinstance(g64, dict) else None
        if a64 is None or sg is None or (hasattr(sg, "numel") and sg.numel() == 0):
            continue
        a64 = np.asarray(a64, dtype=np.float64).reshape(N, -1)
        ss = (sg.detach().cpu().numpy() if hasattr(sg, "detach") else np.asarray(sg)).astype(np.float64).reshape(N, -1)
        o32 = np.asarray(g32[name], dtype=np.float64).reshape(N, -1)
        if not np.array_equal(ss[~vis], o32[~vis]) or np.abs(o32[~vis]).sum() != 0.0:
            j = np.nonzero(~vis)[0][np.nonzero((ss[~vis] != o32[~vis]).any(1))[0][:5]]
            fails.append(f"{name}: rows of culled Gaussians (radii == 0) differ from the oracle's zeros, e.g. rows {j.tolist()}")
        mag = np.abs(a64).max(1)
        rows = np.nonzero(vis & (mag > 0) & ~excl)[0]
        if rows.size == 0:
            continue
        e_s = row_errors(ss, a64, rows)
        evals = [row_errors(o32, a64, rows)] + [row_errors(alt, a64, rows) for alt in (g32_alt or {}).get(name, [])]
        q_s, q_o, c_s, c_o, bad = row_rule(e_s, evals)
        if record is not None:
            record[name] = dict(rows=int(rows.size), q50=(float(q_s[0]), float(q_o[0])), q90=(float(q_s[1]), float(q_o[1])),
                                tails={tau: (cs, co) for tau, cs, co in zip(ROW_TAUS, c_s, c_o)}, excluded=n_excl, visible=n_vis)
        rep.append(f"   {name:12s} {rows.size:6d} rows: q50 {q_s[0]:.1e} (oracle32 {q_o[0]:.1e}), q90 {q_s[1]:.1e} ({q_o[1]:.1e}), "
                   + ", ".join(f"rows > {tau:g}: {cs} ({co})" for tau, cs, co in zip(ROW_TAUS, c_s, c_o))
                   + (f"  [oracle32: the larger of {len(evals)} summation orders]" if len(evals) > 1 else ""))
        if bad:
            amax = float(mag.max())
            e_o = evals[0]
            worst = np.argsort(-e_s)[:10]
            lines = [f"      row {int(rows[k])}: magnitude 1e{int(np.floor(np.log10(mag[rows[k]] / amax)))} of the array max, radius {int(radii[rows[k]])}, "
                     f"centre ({float(st32['xy'][rows[k], 0]):.1f}, {float(st32['xy'][rows[k], 1]):.1f}), e subject {e_s[k]:.2e}, e oracle32 {e_o[k]:.2e}" for k in worst]
            dec = np.floor(np.log10(mag[rows] / amax)).astype(int)
            table = [f"      1e{d:+d}: {int((dec == d).sum())} rows, subject median {np.median(e_s[dec == d]):.1e} max {e_s[dec == d].max():.1e} over 1e-3 {int((e_s[dec == d] > 1e-3).sum())}; "
                     f"oracle32 median {np.median(e_o[dec == d]):.1e} max {e_o[dec == d].max():.1e} over 1e-3 {int((e_o[dec == d] > 1e-3).sum())}" for d in sorted(set(dec.tolist()), reverse=True)]
            fails.append(f"{name}: " + "; ".join(bad) + "\n    ten worst rows:\n" + "\n".join(lines) + "\n    per decade of row magnitude / array max:\n" + "\n".join(table))
    assert not fails, head + "\n  " + "\n  ".join(fails)
    return "\n".join(rep)
