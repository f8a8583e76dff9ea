"""GPU: the per-tile sort in every regime of its dispatch, with both rankers, at both launch sites and in both instantiations.

Each case is one small frame built by tests/sort_regimes.py so that chosen tiles take chosen code paths of csrc/tile_sort.h.  The capacity
hint is PINNED per case -- which instantiation and which launch site a frame gets depends on it, and the hint of a process otherwise only
grows with the tests that ran before -- and the library is asked which plan the call got (egs_forward_sort_plan).  The sorted lists are
held bit for bit to the oracle's; for a sort inside the forward blend the colour plane is held to it as well: that sort feeds the blend of
the same workgroup, so a list that is written correctly but read stale shows only in the image."""
import numpy as np
import pytest
import torch

from tests import sort_regimes as sr
from tests.common import outlier_fraction
from tests.test_gpu_parity import hip_forward, pinned_capacity, TOL

pytestmark = pytest.mark.gpu

CASES = [(name, site, ballot) for name in sr.BUILDERS for site in sr.sites_of(name) for ballot in (False, True)]


@pytest.mark.parametrize("name,site,ballot", CASES, ids=[f"{n}-{s}-{'ballot' if b else 'atomic'}" for n, s, b in CASES])
def test_sort_regime(name, site, ballot):
    from egogaussian_amd import _C
    dev = torch.device("cuda:0")
    sc, st = sr.oracle_state(name)
    H, W, P, R = sc.d["image_height"], sc.d["image_width"], int(st["P"]), int(st["R"])
    cap, flags = sr.capacity_for(sc, st), sr.flags_for(site, ballot)
    cells = sr.reach(sc, st, site, ballot)                             # the targeted tiles are in the named cells, outside the guard band
    infos = sr.regime_of_tiles(st, cap, flags)
    assert cells and all(infos[t].regime == regime for t, (regime, n) in sc.targets.items())
    retries = _C.stats["retries"]
    with pinned_capacity(cap):
        g, out = hip_forward(sc.d, dev, debug=flags)
        torch.cuda.synchronize()
        assert _C.stats["retries"] == retries, "the pinned capacity was too small: another path ran"
        assert _C.stats["capacity"] == cap
        plan = _C.sort_plan(P, W, H, _C.stats["capacity"], debug=flags)
    assert plan == sr.expected_plan(sc, site, ballot), f"plan {plan:#x}: not the launch site / instantiations / ranker this case is built for"
    iv = _C.image_views(out[7], W, H); bv = _C.binning_views(out[6], P, R, W, H, cap)
    assert out[0] == R
    assert np.array_equal(iv["ranges"].cpu().numpy().view(np.uint32), st["ranges"])
    got, want = bv["point_list"].cpu().numpy().view(np.uint32)[:R], st["point_list"][:R]
    if not np.array_equal(got, want):
        bad = [(t, tuple(infos[t])[1:]) for t, (b, e) in enumerate(st["ranges"].astype(np.int64)) if e > b and not np.array_equal(got[b:e], want[b:e])]
        raise AssertionError(f"sorted lists differ from the oracle's in tiles (tile, instantiation, regime, n, largest bucket, depth passes, index passes, ties): {bad}")
    if site == "blend":
        assert outlier_fraction(out[1].cpu().numpy(), st["color"], TOL) <= 1e-4
