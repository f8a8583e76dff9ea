"""GPU: the eight-row reduction of the backward blend (csrc/render_bwd.hip red_write_rows8: MODE 1 = seven rows + one folded pair, MODE 2 = six rows +
two folded pairs), on images of one tile where every lane of every quadrant-wave carries a term.

  * one Gaussian over all 256 pixels of a 16 x 16 image, a different upstream gradient per pixel: each quadrant-wave's FIRST visit is its only one --
    the visit whose first row went astray when the wait state behind the write of M0 was missing;
  * two and 65 Gaussians on the same image: a second visit in a batch of 64, and a second batch;
  * 13 x 11 pixels: partly filled quadrants, whose lanes outside the image must add zero.

Both blends are held to the oracles by tests/backward_line_scenes.py run_small_scene (proven flips, every row within TOL of the array's maximum
against the float32 and the float64 oracle) and, all cases together, to the per-row rule of tests/common.py: MODE 2 with upstream gradients on
colour, depth and alpha -- all ten sums reach a gradient: the five moments dL/dmean2D and dL/dcov3D (scales, rotations), slot 5 dL/dopacity, 6-8
dL/dcolors, 9 dL/dmeans3D through the depth -- and MODE 1 with the colour gradient alone (nine sums)."""
import functools

import pytest

from tests.backward_line_scenes import small_scene, run_small_scene, pooled_row_rule

pytestmark = pytest.mark.gpu

CASES = {   # P, H, W, sigma in pixels, opacity
    "one-gaussian-every-pixel": (1, 16, 16, (11.0, 13.0), (0.7, 0.9)),
    "two-gaussians": (2, 16, 16, (11.0, 13.0), (0.4, 0.6)),
    "65-gaussians-two-batches": (65, 16, 16, (11.0, 13.0), (0.02, 0.04)),
    "13x11-partly-filled-quadrants": (3, 11, 13, (9.0, 11.0), (0.4, 0.6)),
}


@functools.lru_cache(maxsize=None)
def _run(case, colour_only):
    P, H, W, sigma, opacity = CASES[case]
    return run_small_scene(small_scene(P, H, W, 40 + P, sigma=sigma, opacity=opacity), 50 + P, colour_only=colour_only,
                           what=f"[{case}, {'colour only' if colour_only else 'colour, depth, alpha'}]")


@pytest.mark.parametrize("colour_only", [False, True], ids=["MODE 2", "MODE 1"])
@pytest.mark.parametrize("case", list(CASES))
def test_sums_of_a_single_tile(case, colour_only):
    P = CASES[case][0]
    r = _run(case, colour_only)
    st = r["st"]
    assert int((st["radii"] > 0).sum()) == P
    if P == 1:
        assert int(st["n_contrib"].min()) == 1, "the one Gaussian is meant to reach all 256 pixels"
    if P == 65:
        assert int(st["n_contrib"].max()) > 64, "a pixel is meant to blend more than one batch of 64"
    assert all(float(t.abs().max()) > 0 for t in r["hb"][:4])


def test_every_row_against_its_own_magnitude():
    """The per-row rule over the rows of the four cases in both modes (142 rows per array)."""
    print("\n" + pooled_row_rule([_run(c, m) for c in CASES for m in (False, True)], "eight-row reduction"))
