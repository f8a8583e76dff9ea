"""CPU: the model of the per-tile sort's dispatch (tests/sort_regimes.py) on hand-written depth words, every scene builder against the
cell it names (inside the guard band), the union of the builders against MATRIX, and the model's launch-plan arithmetic against the
library's egs_forward_sort_plan.  No device."""
import numpy as np
import pytest

from tests import sort_regimes as sr

K, S, B = sr.K, sr.K["small_cap"], sr.K["big_cap"]
Z5, Z9 = 0x40A00000, 0x41100000          # 5.0f, 9.0f


def _spread(n, step):
    """n depth words `step` ulps apart from 5.0 up, inside the binade [4, 8) where a float is linear in its bit pattern"""
    assert n * step < 0x600000
    return (Z5 + np.arange(n, dtype=np.uint64) * step).astype(np.uint32)


def test_constants_are_the_sources():
    assert (S, B, K["bucket_max"], K["slab_bucket_max"], K["dbits"], K["solo_per_tile"]) == (1792, 4096, 96, 512, 9, 2048)


def test_each_arm_of_the_table_from_literal_bit_patterns():
    c = sr.classify
    assert c([Z5] * 5, 4) == ("equal", 5, 0, True) and c([Z5], 4) == ("equal", 1, 0, False)
    assert c([0x40400000, Z5, Z9], 4) == ("one-pass", 1, 3, False)
    pile = lambda m: list(range(Z5, Z5 + m)) + [Z9]                 # m consecutive floats from 5.0 (bucket 0) and 9.0 (the last bucket)
    assert c(pile(200), 4) == ("digits", 200, 3, False)
    assert c(pile(200) + [Z5 + 7], 4) == ("digits+ties", 201, 3, True)
    assert c(_spread(S + 1, 2048), 4)[0] == "slabs" and c(_spread(B + 1, 1024), 8)[0] == "slabs"
    assert c([Z5] * (S + 1), 4) == ("global", S + 1, 0, True) and c([Z5] * (B + 1), 8) == ("global", B + 1, 0, True)
    # the eight-wave instantiation has 1024 buckets: a pile that shares a bucket of the 512 is apart in the 1024
    two = [Z5] * 60 + [Z5 + 0x1800] * 60 + [Z5 + 0x400000]         # 0x1800 ulps up: a bucket is 0x2000 ulps wide (512 buckets) / 0x1000 (1024)
    assert c(two, 4)[:2] == ("digits+ties", 120) and c(two, 8)[:2] == ("one-pass", 60)


def test_list_length_on_both_sides_of_each_cap():
    c = sr.classify
    assert c([Z5] * S, 4)[0] == "equal" and c([Z5] * (S + 1), 4)[0] == "global"
    assert c([Z5] * B, 8)[0] == "equal" and c([Z5] * (B + 1), 8)[0] == "global"
    assert c(_spread(S, 2048), 4)[0] == "one-pass" and c(_spread(S + 1, 2048), 4)[0] == "slabs"
    assert c(_spread(B, 1024), 8)[0] == "one-pass" and c(_spread(B + 1, 1024), 8)[0] == "slabs"
    # the same list on the other instantiation: 1 793 entries fit the eight-wave registers
    assert c(_spread(S + 1, 2048), 8)[0] == "one-pass"


def test_bucket_count_on_both_sides_of_each_limit():
    c = sr.classify
    lim = K["bucket_max"]
    for m, want in ((lim, "one-pass"), (lim + 1, "digits")):
        r = c(list(range(Z5, Z5 + m)) + [Z9], 4)
        assert (r[0], r[1]) == (want, m)
    assert c([Z5] * lim + [Z9], 4)[0] == "one-pass" and c([Z5] * (lim + 1) + [Z9], 4)[0] == "digits+ties"
    # slabs: a pile of p at the smallest depth (bucket 0, alone: the spread starts sixteen steps up, a bucket is under four) plus a spread
    slim = K["slab_bucket_max"]
    for inst, n, step in ((4, S + 600, 2048), (8, B + 600, 1024)):
        for p, want in ((slim, "slabs"), (slim + 1, "global")):
            bits = np.concatenate([np.full(p, Z5, np.uint32), _spread(n - p + 16, step)[16:]])
            r = c(bits, inst)
            assert bits.size == n and (r[0], r[1]) == (want, p), (inst, p, r)


@pytest.mark.parametrize("e,passes", [(9, 1), (18, 2), (27, 3)])
def test_depth_span_around_each_digit_boundary(e, passes):
    """a span of 2^e - 1 ulps fits `passes` nine-bit digits; 2^e and 2^e + 1 need one more"""
    for span, want in ((2 ** e - 1, passes), (2 ** e, passes + 1), (2 ** e + 1, passes + 1)):
        assert sr.classify([Z5, Z5 + span], 4)[2] == want
        assert sr.classify([Z5] * 200 + [Z5 + span], 4)[2] == want
    assert sr.classify([0x3E800000, 0x46EA6000], 4)[2] == 4         # 0.25 beside 30 000


def test_index_passes():
    assert [sr.index_passes_of(P) for P in (1, 2, 300, 512, 513, 3000, 262144, 262145, 262400)] == [0, 1, 1, 1, 2, 2, 2, 3, 3]


def test_regime_of_tiles_reads_keys_ranges_and_the_plan():
    """a made-up oracle state of three tiles: which instantiation takes a tile follows the capacity"""
    d = [np.full(10, Z5, np.uint32), _spread(S + 1, 2048), np.concatenate([np.arange(Z5, Z5 + 300), [Z9]]).astype(np.uint32)]
    keys = np.concatenate([(np.uint64(t + 1) << np.uint64(32)) | x.astype(np.uint64) for t, x in enumerate(d)])       # (tile << 32 | depth word)
    ends = np.cumsum([x.size for x in d])
    ranges = np.array([[0, 0]] + [[e - x.size, e] for e, x in zip(ends, d)], dtype=np.uint32)       # tile 0 is empty
    st = dict(keys=keys, ranges=ranges, P=3000, R=int(ends[-1]))
    solo = sr.regime_of_tiles(st, 2048 * 4, 0)
    both = sr.regime_of_tiles(st, 2048 * 4 + 1, 0)
    assert sorted(solo) == [1, 2, 3]
    assert solo[1] == sr.Tile(1, 4, "equal", 10, 10, 0, 2, True) and both[1] == solo[1]
    assert (solo[2].inst, solo[2].regime) == (4, "slabs") and (both[2].inst, both[2].regime) == (8, "one-pass")
    assert solo[3][:5] == (3, 4, "digits", 301, 300) and both[3] == solo[3]


def test_guard_band_refuses_the_middle():
    T = lambda regime, n, mb, dp=3: sr.Tile(0, 4, regime, n, mb, dp, 2, False)
    sr.check_guard_band(T("one-pass", 400, 48), "one-pass"); sr.check_guard_band(T("digits", 400, 192), "digits")
    sr.check_guard_band(T("slabs", 2000, 256), "slabs"); sr.check_guard_band(T("global", 2000, 1024), "global")
    sr.check_guard_band(T("global", 2000, 2000, 0), "global"); sr.check_guard_band(T("equal", 400, 400, 0), "equal")
    for info, intended in ((T("one-pass", 400, 49), "one-pass"), (T("digits", 400, 191), "digits"), (T("slabs", 2000, 257), "slabs"),
                           (T("global", 2000, 1023), "global"), (T("digits", 400, 300), "digits+ties")):
        with pytest.raises(AssertionError):
            sr.check_guard_band(info, intended)


_reached = {}


@pytest.mark.parametrize("name", list(sr.BUILDERS))
def test_builder_reaches_the_cells_it_names(name):
    sc, st = sr.oracle_state(name)
    infos = sr.regime_of_tiles(st, sr.capacity_for(sc, st), sr.flags_for("own", False))
    for site in sr.sites_of(name):
        for ballot in (False, True):
            cells = sr.reach(sc, st, site, ballot)                   # (raises when a targeted tile is not in its cell, or inside the guard band)
            assert cells, name
            _reached.setdefault(name, set()).update(cells)
            # ... and under the library's own answer for the pinned capacity the plan is the one the case names
            from egogaussian_amd import lib
            plan = lib.load().egs_forward_sort_plan(int(st["P"]), sr.capacity_for(sc, st), sc.d["image_width"], sc.d["image_height"], sr.flags_for(site, ballot))
            assert plan == sr.expected_plan(sc, site, ballot), (name, site, ballot, plan)
    print(name, "R", st["R"], {t: tuple(i)[1:] for t, i in infos.items()})


def test_the_builders_cover_the_matrix():
    assert len(set(sr.MATRIX)) == len(sr.MATRIX), "a cell is listed twice"
    reached = set()
    for name in sr.BUILDERS:
        if name not in _reached:                                      # (this test run alone)
            sc, st = sr.oracle_state(name)
            _reached[name] = set().union(*[sr.reach(sc, st, site) for site in sr.sites_of(name)])
        reached |= _reached[name]
    missing = [c for c in sr.MATRIX if c not in reached]
    assert not missing, f"MATRIX cells no builder reaches: {missing}"
    assert reached == set(sr.MATRIX)
    print(f"{len(sr.MATRIX)} cells reached by {len(sr.BUILDERS)} builders")


def test_plan_arithmetic_matches_the_library():
    from egogaussian_amd import lib
    L = lib.load()
    assert (sr.SORT_IN_BLEND, sr.SORT_SECOND_INSTANTIATION, sr.SORT_BALLOT_RANK) == (lib.SORT_IN_BLEND, lib.SORT_SECOND_INSTANTIATION, lib.SORT_BALLOT_RANK)
    assert (sr.CALL_SYNC, sr.CALL_KEEP_ALL_INSTANCES, sr.CALL_SEPARATE_COUNT, sr.CALL_SEPARATE_SORT, sr.CALL_BALLOT_RANK) == \
        (lib.CALL_SYNC, lib.CALL_KEEP_ALL_INSTANCES, lib.CALL_SEPARATE_COUNT, lib.CALL_SEPARATE_SORT, lib.CALL_BALLOT_RANK)
    n = 0
    for W, H in ((16, 16), (32, 32), (64, 64), (47, 33), (128, 96), (200, 160), (960, 540), (1920, 1080)):
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        for cap in (0, 1, tiles, 2048 * tiles - 1, 2048 * tiles, 2048 * tiles + 1, 4096 * tiles, 2 ** 31 - 1):
            for flags in range(32):
                for P in (0, 1, 300, 500000):
                    assert L.egs_forward_sort_plan(P, cap, W, H, flags) == sr.plan_model(P, cap, tiles, flags), (P, cap, W, H, flags)
                    n += 1
    assert n == 8 * 8 * 32 * 4
