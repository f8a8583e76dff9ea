"""GPU: the tile bucketing in every regime of its slot walk and its table scan, at both sites of the count pass.

Each case is one small frame built by tests/bucket_regimes.py so that the bucketing kernels (csrc/bin_walk.h, binning.hip, the fused count
pass of preprocess.hip) take chosen code paths: strides, padding workgroups and the tail of the table scan; the slot decode at every
rectangle width; the owner map and the binary search in one walk; the block deal; more than one round with and without the owner map; the
chunk prefix on both sides of its threshold; the box cut of the culling walk.  The capacity is PINNED per case and the library is asked
which geometry the call got (egs_forward_bin_geometry): it has to be the one the case is built for.

Held per case: the instance count, the tile ranges, the sorted lists and the rebuilt 64-bit keys bit for bit against the oracle; the
scanned [tile][workgroup] count table and its total against the numpy table of tests/bucket_regimes.py; with tile culling the lists are an
ordered sub-list of the oracle's whose missing entries are provably invisible (tests/common.py check_culled_lists), and the table is held
to the lists the frame left.  Every case runs with the count pass inside the preprocess launch and as a launch of its own wherever the
geometry allows the former, and both must leave the same table bits.

Sizes: those of the issue's table, each confirmed by the getter.  One case is added: `decode` (30 x 17 tiles) enumerates every width and row
boundary of its image, but with a correctly rounded reciprocal none of its first guesses needs the decode's repair lines; `decode-wide`
(61 x 3 tiles, widths 31 .. 61) holds the four smallest widths -- 41, 47, 55, 61 -- at which even that reciprocal leaves a row boundary
one row short (tests/bucket_regimes.py decode_model)."""
import numpy as np
import pytest
import torch

from tests import bucket_regimes as br
from tests.common import check_culled_lists
from tests.test_gpu_parity import hip_forward, pinned_capacity

pytestmark = pytest.mark.gpu


def _cases():
    out = []
    for name in br.BUILDERS:
        culls = (False,) if name in ("decode", "decode-wide", "long-group") else (True,) if name == "box-cut" else (False, True)
        out += [(name, cull) for cull in culls]
    return out


CASES = _cases()


def _frame(sc, st, cull, fused, dev):
    """one forward at the pinned capacity -> (R, ranges, point_list, depth words, scanned table, total)"""
    from egogaussian_amd import _C
    P, W, H, R = int(st["P"]), int(st["W"]), int(st["H"]), int(st["R"])
    flags = br.flags_for(cull, fused)
    geo = _C.bin_geometry(P, W, H, debug=flags)
    assert geo == br.geometry_of(st, cull), "the library's geometry is not the model's"
    for k, v in sc.expect.get(int(cull), {}).items():
        assert geo[k] == v, f"{sc.name}: the call got {k} = {geo[k]}, the case is built for {v}: {geo}"
    assert _C.forward_fuses_count(P, W, H, debug=flags) == bool(fused and geo["can_fuse"])
    retries = _C.stats["retries"]
    with pinned_capacity(R):
        g, out = hip_forward(sc.d, dev, debug=flags)
        torch.cuda.synchronize()
        assert _C.stats["retries"] == retries and _C.stats["capacity"] == R, "the pinned capacity was not the one the frame ran against"
        total = int(_C.stats["total_view"].cpu()[0])
    iv, bv = _C.image_views(out[7], W, H), _C.binning_views(out[6], P, R, W, H, R)
    assert bv["bin_blocks"] == geo["nblocks"]
    ranges = iv["ranges"].cpu().numpy().view(np.uint32)
    pl = bv["point_list"].cpu().numpy().view(np.uint32)[:R]
    depth = _C.geom_views(out[5], P)["rec"][:, 9].contiguous().cpu().numpy().view(np.uint32)
    table = bv["table"].cpu().numpy().view(np.uint32)                       # the [:, :nblocks] view: the only host copy of the table
    return out[0], ranges, pl, depth, table, total, geo


@pytest.mark.parametrize("name,cull", CASES, ids=[f"{n}-{'culled' if c else 'reference'}-lists" for n, c in CASES])
def test_bucket_regime(name, cull):
    dev = torch.device("cuda:0")
    sc, st = br.oracle_state(name)
    assert cull in br.culls_of(sc)
    cells = br.reach(sc, st)                                                # the oracle's rectangles are the structure the case names
    assert cells
    H, W, P, R = int(st["H"]), int(st["W"]), int(st["P"]), int(st["R"])
    want_ranges, want_pl, want_keys = np.asarray(st["ranges"]), np.asarray(st["point_list"]), np.asarray(st["keys"])
    vis = np.asarray(st["tiles_touched"]) > 0
    sites = (True, False) if br.geometry_of(st, cull)["can_fuse"] else (False,)
    tables = {}
    for fused in sites:
        what = f"{name}, culling {'on' if cull else 'off'}, count pass {'fused' if fused else 'separate'}"
        got_R, ranges, pl, depth, table, total, geo = _frame(sc, st, cull, fused, dev)
        assert got_R == R, what
        assert np.array_equal(depth[vis], np.asarray(st["depths"], dtype=np.float32).view(np.uint32)[vis]), what
        n = ranges[:, 1].astype(np.int64) - ranges[:, 0]
        if not cull:
            assert np.array_equal(ranges, want_ranges), f"{what}: tile ranges differ from the oracle's"
            if not np.array_equal(pl, want_pl):
                own = br.owner_of(st, True, geo)
                bad = np.nonzero(pl != want_pl)[0]
                t = int(np.searchsorted(want_ranges[:, 1].astype(np.int64), bad[0], side="right"))
                i = int(want_pl[bad[0]])
                raise AssertionError(f"{what}: {bad.size} of {R} list entries differ, first in tile {t}: Gaussian {i} expected (workgroup {own['workgroup'][i]}, "
                                     f"round {own['round'][i]}, group {own['group_in_round'][i]}, lane {own['lane'][i]}, span start {own['span'][i]}), got {int(pl[bad[0]])}")
            keys = (np.repeat(np.arange(len(n), dtype=np.uint64), n) << np.uint64(32)) | depth[pl].astype(np.uint64)
            assert np.array_equal(keys, want_keys), f"{what}: rebuilt (tile, depth) keys differ"
            want_table, want_total = br.table_reference(st, geo)
        else:
            kept, dropped = check_culled_lists(st, ranges, pl, H, W)
            assert kept == int(n.sum()) and kept + dropped == R
            if name == "box-cut":
                assert dropped > 0, what
                lists = pl[:kept]
                i = int(sc.info["faint"])
                assert not np.any(lists == i), f"{what}: the faint splat (empty alpha box) kept {int((lists == i).sum())} of its {int(st['tiles_touched'][i])} instances"
                for key in ("elongated", "clipped"):
                    i = int(sc.info[key])
                    k = int((lists == i).sum())
                    assert 0 < k < int(st["tiles_touched"][i]), f"{what}: the {key} splat kept {k} of {int(st['tiles_touched'][i])} instances"
            want_table, want_total = br.table_reference(st, geo, lists=(ranges, pl))
        try:
            br.check_table(table, total, want_table, want_total, geo)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
        tables[fused] = table
        print(f"{what}: R {R}, listed {int(n.sum())}, geometry {geo}")
    if len(tables) == 2:
        assert np.array_equal(tables[True], tables[False]), f"{name}: the fused and the separate count pass leave different tables"
