"""Scenes for tests/test_gpu_backward_lines.py: a handful of Gaussians that are ALL on screen, so that the accumulator line of Gaussian 1
(the first whose address differs between a 12-float and a 16-float stride) is written and read.  CPU tensors, as tests/common.py."""
import functools

import torch

from tests.common import make_inputs, seeded_grads


def small_scene(P, H, W, seed, sigma=(2.0, 4.0), opacity=(0.3, 0.9)):
    """make_inputs(..., 'col_sr') with the positions replaced: P points spread over the middle of the view frustum, 4 to 6 units in front of the
    camera, sigma about 2-4 pixels -- every splat overlaps several 8x8 quadrants, several of them share quadrants."""
    d = make_inputs(P, H, W, seed, 0, "col_sr")
    gen = torch.Generator().manual_seed(1000 + seed)
    z = 4.0 + 2.0 * torch.rand(P, generator=gen)
    u = 1.4 * torch.rand(P, 2, generator=gen) - 0.7
    pv = torch.stack([u[:, 0] * z * d["tanfovx"], u[:, 1] * z * d["tanfovy"], z, torch.ones(P)], 1)
    d["means3D"] = (pv @ torch.linalg.inv(d["viewmatrix"]))[:, :3].contiguous()          # (row vectors: p_view = [p, 1] @ viewmatrix)
    focal = W / (2.0 * d["tanfovx"])
    d["scales"] = ((sigma[0] + (sigma[1] - sigma[0]) * torch.rand(P, 3, generator=gen)) * (z / focal)[:, None]).contiguous()
    d["opacities"] = (opacity[0] + (opacity[1] - opacity[0]) * torch.rand(P, 1, generator=gen)).reshape(d["opacities"].shape)
    return d


def hot_scene():
    """256 x 256 pixels = 256 tiles; Gaussian 2 of five fills the screen (its alpha >= 1/255 box covers every tile: EGS_HOT_MIN_TILES),
    the other four are small.  -> (inputs, index of the large one)"""
    H = W = 256
    d = small_scene(5, H, W, 7)
    big = 2
    pv = torch.tensor([[0.0, 0.0, 5.0, 1.0]])
    d["means3D"][big] = (pv @ torch.linalg.inv(d["viewmatrix"]))[0, :3]
    d["scales"][big] = 10.0
    d["opacities"][big] = 0.5
    return d, big


NAMES = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"]


def run_small_scene(d, grad_seed, colour_only=False, what=""):
    """One frame of a few Gaussians through the library (GPU) and the oracles, held to the bars of tests/test_gpu_parity.py that do not need a
    population of rows: instance count and radii equal, threshold flips proven (flip_pixels), the image planes and every gradient row within TOL
    of the array's maximum -- against the float32 oracle AND against the float64 one.
    colour_only: the colour gradient alone (MODE 1 of the backward blend; the oracles get zero planes for depth and alpha: the same function).
    The per-row rule of tests/common.py (check_grad_rows_vs_float64) compares QUANTILES of the rows' errors with the float32 oracle's; on a
    scene of one or three rows a quantile is a single rounding draw (seen: 2.5e-7 against 4.0e-8 on the one row of dL_dscale, four ulps against
    a lucky half) and the rule says nothing.  This function therefore returns the per-row errors of the rows that rule measures
    ({array: (subject, float32 oracle)}, same row selection), and pooled_row_rule applies the rule to the rows of all scenes of a module together.
    -> dict(st, gb, g, out, hb, rows)."""
    import numpy as np
    from egogaussian_amd import _C
    from tests.common import (tile_culling, flip_pixels, check_images_isolating_flips, check_grads_isolating_flips, state_disagreement_pixels,
                              gaussians_contributing_to, row_errors)
    from tests.test_gpu_parity import hip_forward, hip_backward, oracle_forward, float64_oracle, _dev, TOL
    dev = _dev()
    N, H, W = int(d["means3D"].shape[0]), d["image_height"], d["image_width"]
    gc, gd, ga = seeded_grads(H, W, grad_seed)
    o_grads = (gc, torch.zeros_like(gd), torch.zeros_like(ga)) if colour_only else (gc, gd, ga)
    h_grads = (gc, torch.empty(0), torch.empty(0)) if colour_only else (gc, gd, ga)
    o, st = oracle_forward(d)
    gb = o.backward(st, *o_grads)
    with tile_culling(False):
        g, out = hip_forward(d, dev)
        hb = hip_backward(g, out, h_grads, dev)
    torch.cuda.synchronize()
    assert out[0] == st["R"] and np.array_equal(out[4].cpu().numpy(), st["radii"])
    iv = _C.image_views(out[7], W, H)
    flip_px = flip_pixels(out[1].cpu().numpy(), iv["final_T"].cpu().numpy(), st, iv["n_contrib"].cpu().numpy().view(np.uint32))
    check_images_isolating_flips((("color", out[1].cpu().numpy(), st["color"]), ("depth", out[2].cpu().numpy(), st["depth"]),
                                  ("alpha", out[3].cpu().numpy(), st["alpha"])), st, flip_px, TOL, what=what)
    near = []
    rep32 = check_grads_isolating_flips(NAMES, hb, gb, st, flip_px, TOL, what=what + " / float32", near_out=near)[0]
    st64, g64 = float64_oracle(d, o_grads)
    rep64 = check_grads_isolating_flips(NAMES, hb, g64, st, flip_px, TOL, what=what + " / float64")[0]
    print(f"\n   {what} vs float32 oracle: {rep32}\n   {what} vs float64 oracle: {rep64}")
    vis = np.asarray(st["radii"]) > 0
    excl = np.zeros(N, dtype=bool)
    excl[np.asarray(near[0], dtype=np.int64)] = True
    excl[gaussians_contributing_to(st, state_disagreement_pixels(st, st64), 0)] = True
    rows = {}
    for name, sg in zip(NAMES, hb):
        a64 = g64.get(name)
        if a64 is None or sg is None or sg.numel() == 0:
            continue
        a64 = np.asarray(a64, dtype=np.float64).reshape(N, -1)
        ss, o32 = sg.detach().cpu().numpy().astype(np.float64).reshape(N, -1), np.asarray(gb[name], dtype=np.float64).reshape(N, -1)
        assert np.array_equal(ss[~vis], o32[~vis]), f"{what} {name}: rows of culled Gaussians"
        sel = np.nonzero(vis & (np.abs(a64).max(1) > 0) & ~excl)[0]
        rows[name] = (row_errors(ss, a64, sel), row_errors(o32, a64, sel))
    return dict(st=st, gb=gb, g=g, out=out, hb=hb, rows=rows)


def pooled_row_rule(runs, what):
    """tests/common.py row_rule (q50 and q90 within 3 x the float32 oracle's, tail counts within 2 x + 3 rows) on every array's rows of all `runs`
    (run_small_scene results) together.  -> report string."""
    import numpy as np
    from tests.common import row_rule, ROW_TAUS
    rep, fails = [], []
    for name in NAMES:
        parts = [r["rows"][name] for r in runs if name in r["rows"]]
        if not parts:
            continue
        e_s, e_o = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        q_s, q_o, c_s, c_o, bad = row_rule(e_s, [e_o])
        rep.append(f"   {name:12s} {e_s.size:5d} rows: q50 {q_s[0]:.1e} (oracle32 {q_o[0]:.1e}), q90 {q_s[1]:.1e} ({q_o[1]:.1e}), max {e_s.max():.1e} ({e_o.max():.1e}), "
                   + ", ".join(f"rows > {tau:g}: {cs} ({co})" for tau, cs, co in zip(ROW_TAUS, c_s, c_o)))
        if bad:
            fails.append(f"{name}: " + "; ".join(bad))
    assert not fails, what + "\n  " + "\n  ".join(fails) + "\n" + "\n".join(rep)
    return what + " rows vs float64, pooled:\n" + "\n".join(rep)


LINE_CASES = [(1, 32, 32), (3, 32, 32), (5, 32, 32), (257, 48, 48)]


@functools.lru_cache(maxsize=None)
def line_case(P):
    """(inputs, upstream gradients on colour, depth and alpha) of the case with P Gaussians; built once, not to be modified"""
    H, W = {p: (h, w) for p, h, w in LINE_CASES}[P]
    return small_scene(P, H, W, P), seeded_grads(H, W, P + 10)


@functools.lru_cache(maxsize=None)
def line_run(P):
    """run_small_scene of line_case(P) with its upstream gradients (colour, depth and alpha); run once"""
    return run_small_scene(line_case(P)[0], P + 10, what=f"[{P} Gaussians]")


@functools.lru_cache(maxsize=None)
def hot_run():
    return run_small_scene(hot_scene()[0], 17, what="[hot]")
