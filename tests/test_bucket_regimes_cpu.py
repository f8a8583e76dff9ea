"""CPU: the model of the tile bucketing's launch geometry (tests/bucket_regimes.py) against the library's egs_forward_bin_geometry, every
scene builder against the cells it names, the union of the builders against CELLS, the numpy count table against the oracle's ranges, and
the check the GPU tests use against deliberately wrong tables.  No device."""
import numpy as np
import pytest

from tests import bucket_regimes as br

K = br.K


def _getter(P, W, H, cull):
    from egogaussian_amd import _C
    return _C.bin_geometry(P, W, H, debug=br.flags_for(cull, True))


def test_constants_are_the_sources():
    assert (K["threads"], K["map_slots"], K["round_words"], K["target_blocks"], K["prefix_min"], K["max_tiles"]) == (1024, 4096, (4, 32, 8, 256), 512, 4096, 36864)
    assert (K["lds"], K["half_lds"], K["chunk"], K["min_stride"], K["groups"], K["prefix_threads"]) == (160 * 1024, 80 * 1024, 2048, 4, 8, 1024)
    assert br.ORDER_LDS == 12880 and br.WAVES == 16


def test_geometry_by_hand():
    """the sizes the issue's table of cases was worked out for"""
    g = br.geometry_model
    pick = lambda q, *names: tuple(q[n] for n in names)
    assert pick(g(1, 48, 48, 1), "n_tiles", "nblocks", "stride", "n_chunks", "gpr", "rounds") == (9, 1, 4, 1, 16, 1)
    assert [g(P, 48, 48, 1)["nblocks"] for P in br.TINY_P] == [1, 1, 1, 1, 1, 1, 2, 2, 4, 5, 9]
    assert [g(P, 48, 48, 1)["stride"] for P in br.TINY_P] == [4, 4, 4, 4, 4, 4, 4, 4, 4, 8, 16]
    assert pick(g(2100, 480, 270, 1), "n_tiles", "stride", "n_chunks") == (510, 16, 4)
    assert pick(g(131300, 64, 64, 0), "nblocks", "stride", "groups_per_block", "rounds", "can_fuse") == (257, 512, 8, 1, 1)
    assert pick(g(524800, 64, 64, 1), "nblocks", "gpr", "groups_per_block", "rounds", "use_map", "can_fuse") == (410, 16, 20, 2, 1, 0)
    assert pick(g(65700, 2048, 2048, 1), "n_tiles", "n_chunks", "prefixed") == (16384, 4096, 1)
    assert pick(g(65700, 2048, 2032, 1), "n_tiles", "n_chunks", "prefixed") == (16256, 4064, 0)
    assert pick(g(131300, 4096, 2304, 1), "n_chunks", "gpr", "rounds", "use_map", "cull", "prefixed", "can_fuse") == (9216, 4, 2, 0, 1, 1, 0)
    assert pick(g(131300, 4096, 2304, 0), "n_chunks", "gpr", "rounds", "use_map", "cull", "can_fuse") == (9216, 8, 1, 0, 0, 1)
    assert g(0, 64, 64, 1) == dict(dict.fromkeys(br.GEOMETRY_FIELDS, 0), n_tiles=16, gx=4)


def _image_with_tiles(n):
    """(W, H) of an accepted image of exactly n tiles (sides of at most 2 047 tiles), or None"""
    for gx in range(min(n, 2047), 0, -1):
        if n % gx == 0:
            return (16 * gx, 16 * (n // gx)) if n // gx <= 2047 else None
    return None


def _nearest_image(n, step):
    while _image_with_tiles(n) is None:
        n += step
    return _image_with_tiles(n)


def test_model_equals_the_library():
    """geometry_model against egs_forward_bin_geometry over a grid that holds both sides of every threshold.  What depends on the image is
    decided by the tile count alone: the model is swept over every count the ABI accepts, and at each count where gpr, use_map or the
    culling change the grid takes the nearest image on either side (a count that no accepted image has -- a prime beyond 2 047 -- gives way
    to its neighbour).  What depends on the model size changes at the sizes listed."""
    sizes = [(48, 48), (64, 80), (480, 270), (64, 64), (960, 540), (1920, 1080), (2048, 2032), (2048, 2048), (3840, 2160), (4096, 2304), (47, 33)]
    change = []
    for cull in (0, 1):
        prev = None
        for n in range(1, K["max_tiles"] + 1):
            q = br.geometry_model(1000, 16 * n, 16, cull)                   # (the model does not mind the side; the library is asked about real images)
            cur = (q["gpr"], q["use_map"], q["cull"])
            if prev is not None and cur != prev:
                change.append((cull, n, prev, cur))
                sizes += [_nearest_image(n - 1, -1), _nearest_image(n, 1)]
            prev = cur
    # with culling 16 -> 8 groups (half the LDS), the map lost, 8 -> 4; without it 16 -> 8, the map lost (16 again), 16 -> 8
    assert [c[:2] for c in change] == sorted(c[:2] for c in change) and len(change) >= 6, change
    assert {c[3][0] for c in change} >= {4, 8, 16} and {c[3][1] for c in change} == {0, 1} and all(c[3][2] == c[0] for c in change)
    # the prefix pass: 4096 chunks of 2048 / stride rows
    sizes += [(2048, 2032), (2048, 2048), (16 * 1023, 16 * 16), (16 * 1024, 16 * 16), (16 * 2047, 16 * 16)]
    Ps = [1, 63, 64, 65, 255, 256, 257, 300, 512, 513, 1000, 1024, 1025, 2048, 2049, 2100, 4096, 4097, 32768, 32769, 65536, 65537, 65700, 131072, 131073, 131300, 262144, 262145, 393216, 393217,
          524288, 524289, 524800, 1000000, 2000000, 4100000]
    n = 0
    for W, H in sorted(set(sizes)):
        for P in Ps:
            for cull in (0, 1):
                assert _getter(P, W, H, cull) == br.geometry_model(P, W, H, cull), (P, W, H, cull)
                n += 1
    assert n == len(set(sizes)) * len(Ps) * 2
    seen = {k: set() for k in ("gpr", "use_map", "prefixed", "stride", "rounds", "can_fuse")}
    for W, H in sorted(set(sizes)):
        for P in Ps:
            for cull in (0, 1):
                q = br.geometry_model(P, W, H, cull)
                for k in seen:
                    seen[k].add(q[k])
    assert seen["gpr"] >= {4, 8, 16} and seen["use_map"] == {0, 1} and seen["prefixed"] == {0, 1} and seen["can_fuse"] == {0, 1}
    assert seen["stride"] >= {4, 8, 16, 512} and seen["rounds"] >= {1, 2, 4}
    assert _getter(0, 64, 64, 1) == br.geometry_model(0, 64, 64, 1)
    # argument errors
    from egogaussian_amd import lib
    import ctypes as C
    q = lib.BinGeometry()
    L = lib.load()
    assert L.egs_forward_bin_geometry(10, 64, 64, 0, None) == -1 and L.egs_forward_bin_geometry(-1, 64, 64, 0, C.byref(q)) == -1
    assert L.egs_forward_bin_geometry(10, 0, 64, 0, C.byref(q)) == -1 and L.egs_forward_bin_geometry(10, 8192, 8192, 0, C.byref(q)) == -3


def test_culling_is_never_given_up_for_lack_of_lds():
    """egs_bin_geometry turns the culling off when even four groups per round do not fit beside the per-tile counters.  At every image the
    ABI accepts (at most EGS_MAX_TILES tiles) that branch is unreachable: asked for culling, the geometry culls.  The first tile count at
    which it would not lies above the limit -- raising the limit past it fails here."""
    for n in (1, 2040, 8160, 21000, 28000, 32400, K["max_tiles"] - 1, K["max_tiles"]):
        rows = (n + 255) // 256
        W, H = (4096, 16 * rows) if n > 2047 else (16 * n, 16)
        q = br.geometry_model(100000, W, H, 1)
        assert q["cull"] == 1 and q["gpr"] >= 4, (n, q)
    # the counters are the only term that grows: the smallest culling round (four groups, no map) fits up to this many tiles
    last = (K["lds"] - br.round_words(4, True, False) * 4) // 4
    assert last == 37856 and K["max_tiles"] <= last
    assert _getter(100000, 4096, 2304, 1)["cull"] == 1


_reached = {}


@pytest.mark.parametrize("name", list(br.BUILDERS))
def test_builder_reaches_the_cells_it_names(name):
    sc, st = br.oracle_state(name)
    cells = br.reach(sc, st)                                                # (raises when the oracle's rectangles are not the structure built for)
    assert cells and set(sc.cells) <= cells
    _reached[name] = cells
    for cull in br.culls_of(sc):
        q = _getter(int(st["P"]), int(st["W"]), int(st["H"]), cull)
        assert q == br.geometry_of(st, cull)
        assert all(q[k] == v for k, v in sc.expect.get(int(cull), {}).items()), (name, cull, q)
    print(name, "R", st["R"], sorted(cells)[:6])


def test_the_builders_cover_the_cells():
    reached = set()
    for name in br.BUILDERS:
        if name not in _reached:                                            # (this test run alone)
            _reached[name] = br.reach(*br.oracle_state(name))
        reached |= _reached[name]
    missing = [c for c in br.CELLS if c not in reached]
    assert not missing, f"cells no builder reaches: {missing}"
    assert reached == set(br.CELLS)


@pytest.mark.parametrize("name", ["tiny-1025-48x48", "tiny-2100-480x270", "tiny-300-64x80", "decode", "decode-wide", "long-group", "block-deal", "two-rounds-mapped", "prefix-on",
                                  "prefix-off", "box-cut"])
def test_table_reference_agrees_with_the_oracles_lists(name):
    """row starts of the scanned table = the starts of the oracle's tile ranges, its total = R; the same table from the oracle's sorted
    lists instead of its rectangles"""
    sc, st = br.oracle_state(name)
    geo = br.geometry_of(st, False)
    table, total = br.table_reference(st, geo)
    ranges = np.asarray(st["ranges"]).astype(np.int64)
    n = ranges[:, 1] - ranges[:, 0]
    assert total == int(st["R"]) == int(n.sum())
    assert np.array_equal(table[n > 0, 0], ranges[n > 0, 0])
    assert np.array_equal(table[:, 0].astype(np.int64), np.cumsum(n) - n)
    assert np.all(np.diff(table.astype(np.int64).ravel()) >= 0)
    t2, tot2 = br.table_reference(st, geo, lists=(st["ranges"], st["point_list"]))
    br.check_table(t2, tot2, table, total, geo)
    own = br.owner_of(st, True, geo)
    assert int(own["slots"].sum()) == total


@pytest.mark.parametrize("name,variant", [("two-rounds-mapped", "skip-second-round"), ("tiny-1025-48x48", "count-unused-columns"), ("block-deal", "count-unused-columns"),
                                          ("prefix-on", "drop-chunk-carry"), ("prefix-off", "drop-chunk-carry"), ("tiny-2100-480x270", "drop-chunk-carry"),
                                          ("block-deal", "no-interleave"), ("two-rounds-mapped", "no-interleave"), ("tiny-300-48x48", "count-unused-columns")])
def test_wrong_tables_are_caught(name, variant):
    """what a kernel with one of four defects would leave is refused by the check the GPU tests apply"""
    sc, st = br.oracle_state(name)
    geo = br.geometry_of(st, False)
    table, total = br.table_reference(st, geo)
    br.check_table(table.copy(), total, table, total, geo)
    wrong, wtotal = br.table_reference(st, geo, variant=variant)
    with pytest.raises(AssertionError, match="scanned count table"):
        br.check_table(wrong, wtotal, table, total, geo)
    if variant == "drop-chunk-carry" and geo["prefixed"]:
        # ... and the defect is the carry BETWEEN iterations: the first 1024 chunks are right
        first = K["prefix_threads"] * K["chunk"] // geo["stride"]
        assert np.array_equal(wrong[:first], table[:first]) and not np.array_equal(wrong[first:], table[first:])


def test_slot_decode_needs_no_more_than_its_two_repair_lines():
    """The walk turns a slot's offset kk inside a rectangle of width wd into (row, col) with a float32 reciprocal and repairs a first guess
    that is off by one.  Over every width an accepted image can have (a side of at most 32 767 px: 2 048 tiles) and every offset a
    rectangle of that width can hold (at most EGS_MAX_TILES tiles), with the reciprocal correctly rounded and one step to either side of it
    (the hardware's is good to one), the repaired decode is divmod(kk, wd).  The repair is needed: a first guess can be one row short (at a
    row boundary, kk = m * wd, with a reciprocal rounded down).  It is never one row long at these sizes -- that takes m * wd beyond 2^23."""
    short = long_ = 0
    for wd in range(1, 2049):
        kk = np.arange(wd * (K["max_tiles"] // wd), dtype=np.int64)
        for ulps in (-1, 0, 1):
            row, col, low, high = br.decode_model(kk, wd, ulps)
            assert np.array_equal(row, kk // wd) and np.array_equal(col, kk % wd), (wd, ulps)
            assert np.all(kk[high] % wd == 0), "a first guess that is a row short sits on a row boundary"
            short += int(high.sum()); long_ += int(low.sum())
    assert short > 0 and long_ == 0
    # the 30 x 17 image of the `decode` case holds every row boundary of every width: with a reciprocal one step low all of them take the repair
    for wd in range(1, 31):
        got = np.nonzero(br.decode_model(np.arange(17 * wd), wd, -1)[3])[0]
        assert got.size >= 15 and np.all(got % wd == 0), (wd, got)
