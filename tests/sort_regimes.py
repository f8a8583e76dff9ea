"""A CPU model of the per-tile sort's dispatch (egogaussian_amd/csrc/tile_sort.h, binning.hip egs_sort_plan) and scene builders that put
chosen tiles of a small frame into chosen regimes.  Test infrastructure: nothing here runs on a device.

The sort takes one of six code paths per tile (cap = TS_SMALL_CAP / 4096, NB = 512 / 1024 linear depth buckets for the four- / eight-wave
instantiation):
    equal        n <= cap, all depths equal                                  index-digit passes only                     [ranker]
    one-pass     n <= cap, no bucket over TS_BUCKET_MAX                      bucket and compare
    digits       n <= cap, a bucket over TS_BUCKET_MAX, no two equal depths  packed-counter depth passes                 [ranker]
    digits+ties  the same, with equal depths                                 index passes, then the depth passes again   [ranker]
    slabs        n > cap, no bucket over TS_SLAB_BUCKET_MAX                  depth slabs through LDS
    global       n > cap, a bucket over TS_SLAB_BUCKET_MAX or all equal      global-memory ping-pong                     [ranker]
Which instantiation a tile gets is decided on the host: `solo` = capacity <= 2048 x tiles -- the four-wave instantiation takes every tile
(and may run inside the forward blend); otherwise it takes n <= TS_SMALL_CAP and the eight-wave one the rest.  Every constant is read from
the sources, so a changed constant moves the model with it.

GUARD BAND (a condition on the builders, not a tolerance): the model evaluates the kernel's bucket function in numpy float32, operation by
operation (the library is built with -ffp-contract=off), but it does not have to be bit-exact to be right: a builder's targeted tile
counts as an intended one-pass / slabs tile only when its largest bucket is at most HALF the limit, and as an intended fallback only when
it is at least TWICE the limit (or all depths are equal); anything in between raises.  List lengths are exact: each splat's rectangle lies
in one tile, which is asserted from the oracle's tiles_touched.

LENGTHS THE CODE CANNOT COMBINE WITH A REGIME.  A list of one entry has dmax == dmin: it is `equal`, never one-pass.  A fallback needs a
bucket of more than TS_BUCKET_MAX (96; 192 inside the guard band) entries, so lists of 63 / 64 / 65 cannot be digits+ties; the ranker
regime they can reach is `equal`, and that is what MATRIX asks of them."""
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL_SYNC, CALL_KEEP_ALL_INSTANCES, CALL_SEPARATE_COUNT, CALL_SEPARATE_SORT, CALL_BALLOT_RANK = 1, 2, 4, 8, 16
SORT_IN_BLEND, SORT_SECOND_INSTANTIATION, SORT_BALLOT_RANK = 1, 2, 4
REGIMES = ("equal", "one-pass", "digits", "digits+ties", "slabs", "global")
RANKER_REGIMES = ("equal", "digits", "digits+ties", "global")       # the regimes that call wave_digit_rank


def read_constants():
    """The sort's constants, by regex from the sources (as tests/test_abi_cpu.py reads the header)."""
    src = lambda *p: open(os.path.join(ROOT, "egogaussian_amd", "csrc", *p)).read()
    ts, bn = src("tile_sort.h"), src("binning.hip")
    one = lambda pat, text: int(re.search(pat, text).group(1))
    c = dict(small_cap=one(r"#define\s+TS_SMALL_CAP\s+(\d+)", ts), bucket_max=one(r"#define\s+TS_BUCKET_MAX\s+(\d+)u", ts),
             slab_bucket_max=one(r"#define\s+TS_SLAB_BUCKET_MAX\s+(\d+)u", ts), dbits=one(r"#define\s+TS_DBITS\s+(\d+)", ts),
             big_cap=one(r"k_tile_sort<true,\s*8,\s*(\d+),\s*TS_SMALL_CAP \+ 1u>", bn), solo_per_tile=one(r"<=\s*(\d+)ull\s*\*\s*\(uint64_t\)n_tiles", bn))
    assert one(r"k_tile_sort<false,\s*8,\s*(\d+),", bn) == c["big_cap"] and re.search(r"k_tile_sort<true,\s*4,\s*TS_SMALL_CAP,\s*0u>", bn)
    assert re.search(r"constexpr int TS_NB = TS_WAVES \* 128;", ts), "the model's bucket count is TS_WAVES * 128"
    return c


K = read_constants()
CAP = {4: K["small_cap"], 8: K["big_cap"]}
NB = {4: 4 * 128, 8: 8 * 128}

Tile = namedtuple("Tile", "tile inst regime n max_bucket depth_passes index_passes ties")


def plan_model(P, capacity, n_tiles, flags):
    """binning.hip egs_sort_plan, in Python: SORT_* bits."""
    if P <= 0 or capacity <= 0 or n_tiles <= 0:
        return 0
    solo = capacity <= K["solo_per_tile"] * n_tiles
    return ((SORT_IN_BLEND if solo and not flags & (CALL_SEPARATE_SORT | CALL_SYNC) else 0) | (0 if solo else SORT_SECOND_INSTANTIATION)
            | (SORT_BALLOT_RANK if flags & CALL_BALLOT_RANK else 0))


def index_passes_of(P):
    """ceil(bits(P - 1) / TS_DBITS), as egs_launch_binning counts them."""
    return (max(int(P) - 1, 0).bit_length() + K["dbits"] - 1) // K["dbits"]


def bucket_counts(bits, nb):
    """The histogram of tile_sort.h's bucket(): floor((z - zmin) * (NB / (zmax - zmin))) clamped to [0, NB - 1], float32 step by step."""
    z = np.asarray(bits, dtype=np.uint32).view(np.float32)
    zmin, zmax = z.min(), z.max()
    zscale = np.float32(nb) / np.float32(zmax - zmin)
    f = (z - zmin).astype(np.float32) * zscale
    b = np.minimum(np.maximum(f, np.float32(0)), np.float32(nb - 1)).astype(np.uint32)
    return np.bincount(b, minlength=nb)


def classify(bits, inst):
    """One tile's depth words (uint32 bit patterns of positive floats, any order) on the `inst`-wave instantiation
    -> (regime, largest bucket, depth passes, has ties)."""
    bits = np.asarray(bits, dtype=np.uint32)
    n = int(bits.size)
    assert n > 0 and inst in (4, 8)
    dmin, dmax = int(bits.min()), int(bits.max())
    depth_passes = ((dmax - dmin).bit_length() + K["dbits"] - 1) // K["dbits"]
    ties = bool(np.unique(bits).size < n)
    if dmax == dmin:
        return ("equal" if n <= CAP[inst] else "global"), n, 0, ties
    mb = int(bucket_counts(bits, NB[inst]).max())
    if n <= CAP[inst]:
        return ("one-pass" if mb <= K["bucket_max"] else "digits+ties" if ties else "digits"), mb, depth_passes, ties
    return ("slabs" if mb <= K["slab_bucket_max"] else "global"), mb, depth_passes, ties


def regime_of_tiles(st, capacity, flags):
    """Per non-empty tile of an oracle state (Oracle.forward(..., stop_after="binning") or a full forward): a Tile record -- which
    instantiation sorts it under the plan of (capacity, flags), the regime it takes there, its length, largest bucket, depth passes,
    index passes and whether two entries share a depth."""
    ranges = np.asarray(st["ranges"]).astype(np.int64)
    plan = plan_model(int(st["P"]), int(capacity), len(ranges), int(flags))
    ip = index_passes_of(st["P"])
    out = {}
    for t, (b, e) in enumerate(ranges):
        n = int(e - b)
        if n == 0:
            continue
        inst = 8 if (plan & SORT_SECOND_INSTANTIATION) and n > K["small_cap"] else 4
        bits = (np.asarray(st["keys"][b:e]) & np.uint64(0xffffffff)).astype(np.uint32)
        regime, mb, dp, ties = classify(bits, inst)
        out[t] = Tile(t, inst, regime, n, mb, dp, ip, ties)
    return out


def check_guard_band(info, intended):
    """Raise unless `info` (a Tile) is in regime `intended` with its largest bucket outside the band around the limit."""
    if info.regime != intended:
        raise AssertionError(f"tile {info.tile}: built for {intended}, the model says {info}")
    limit = K["bucket_max"] if info.n <= CAP[info.inst] else K["slab_bucket_max"]
    if intended in ("one-pass", "slabs"):
        ok = 2 * info.max_bucket <= limit
    elif intended == "equal":
        ok = info.depth_passes == 0
    else:
        ok = info.max_bucket >= 2 * limit or info.depth_passes == 0
    if not ok:
        raise AssertionError(f"tile {info.tile}: largest bucket {info.max_bucket} is inside the guard band of the limit {limit} ({intended}): {info}")


# ---- the cells that must be reached ------------------------------------------------------------------------------------------------
def _matrix():
    m = []
    for site in ("own", "blend"):
        m += [f"4-solo/{site}/{r}" for r in REGIMES]
    m += [f"4-beside-8/own/{r}" for r in ("equal", "one-pass", "digits", "digits+ties")]
    m += [f"8/own/{r}" for r in REGIMES]
    m += ["len/4/1/equal"]
    for n in (63, 64, 65):
        m += [f"len/4/{n}/one-pass", f"len/4/{n}/equal"]
    for n in (255, 256, 257, K["small_cap"] - 1, K["small_cap"]):
        m += [f"len/4/{n}/one-pass", f"len/4/{n}/digits+ties"]
    for n in (K["small_cap"] + 1, K["big_cap"] - 1, K["big_cap"]):
        m += [f"len/8/{n}/one-pass", f"len/8/{n}/digits+ties"]
    m += [f"len/4/{K['small_cap'] + 1}/slabs", f"len/8/{K['big_cap'] + 1}/slabs"]
    m += [f"depth-passes/{k}" for k in (1, 2, 3, 4)]
    m += [f"index-passes/{k}/{r}" for k in (1, 2, 3) for r in ("equal", "digits+ties")]
    return m


MATRIX = _matrix()


def cells_of(infos, solo, site):
    """The MATRIX cells a set of targeted Tile records reaches when launched at `site` ("own" / "blend")."""
    cells = set()
    for i in infos:
        where = "4-solo" if solo else "4-beside-8" if i.inst == 4 else "8"
        cells.add(f"{where}/{site}/{i.regime}")
        cells.add(f"len/{i.inst}/{i.n}/{i.regime}")
        if i.regime == "digits+ties":
            cells.add(f"depth-passes/{i.depth_passes}")
        if i.regime in ("equal", "digits+ties"):
            cells.add(f"index-passes/{i.index_passes}/{i.regime}")
    return cells & set(MATRIX)


# ---- depth recipes: float32 depths of one tile's cluster -----------------------------------------------------------------------------
def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _b32(z):
    return int(np.asarray([z], dtype=np.float32).view(np.uint32)[0])


def z_equal(n, rng, z=5.0):
    return np.full(n, z, np.float32)


def z_uniform(n, rng, lo=3.0, hi=7.0):
    return rng.uniform(lo, hi, n).astype(np.float32)


def z_pile(n, rng, values=None, base=5.0, outlier=9.0, outliers=1, step=1):
    """n - outliers depths piled on consecutive float32 values from `base` up (distinct when values is None, else drawn from that many:
    ties), plus far outlier(s) that stretch the range so the pile shares the first bucket."""
    m = n - outliers
    k = rng.permutation(m) if values is None else rng.integers(0, values, m)
    pile = _f32(np.uint32(_b32(base)) + (k * step).astype(np.uint32))
    return np.concatenate([pile, np.full(outliers, outlier, np.float32)])[rng.permutation(n)]


def z_pile_ulps(n, rng, span_ulps, values=2, base=5.0):
    """A tied pile on `values` neighbouring float32 values and two entries further up, the last `span_ulps` above the base."""
    k = rng.integers(0, values, n - 2)
    b = np.uint32(_b32(base))
    return _f32(np.concatenate([b + k.astype(np.uint32), [b + np.uint32(span_ulps // 2 + 1), b + np.uint32(span_ulps)]]).astype(np.uint32))[rng.permutation(n)]


def z_slab_pile(n, rng, pile, z=4.5):
    """n depths uniform over [3, 7] with `pile` of them at one depth (a bucket no slab can take)."""
    out = z_uniform(n, rng)
    out[:pile] = z
    return out[rng.permutation(n)]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
Scene = namedtuple("Scene", "name d targets solo")        # targets: {tile: intended regime}


def make_scene(name, H, W, clusters, solo, seed, P=None, split_rows=None):
    """Identity camera (depth = z), col_sr inputs, one cluster per targeted tile at the tile's centre: clusters = [(tile, depths)].
    Every splat is far smaller than a pixel, so its rectangle (the 0.3 px^2 blur's radius of 2) lies inside the tile.  All splats of a
    tile share one centre, half a pixel from the four pixels around it: those get alpha = 0.43 x opacity in [0.0087, 0.043], every other
    pixel less than 0.0016 -- nothing sits near the 1/255 threshold, so the colour plane does not depend on the last bit of exp().
    P / split_rows: pad the model to P rows with Gaussians behind the camera; the visible rows are then the first and the last
    `split_rows` rows (clusters are dealt over both halves, so a tile's list mixes low and high indices)."""
    from egogaussian_amd.scene_synth import make_camera
    rng = np.random.default_rng(seed)
    cam = make_camera(0, H, W)
    tanx, tany = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    fx, fy = W / (2 * tanx), H / (2 * tany)
    gx = (W + 15) // 16
    zs, xs, ys = [], [], []
    for tile, z in clusters:
        z = np.asarray(z, dtype=np.float32)
        cx, cy = (tile % gx) * 16 + 7.5, (tile // gx) * 16 + 7.5
        zs.append(z); xs.append((cx - (W - 1) / 2) * z.astype(np.float64) / fx); ys.append((cy - (H - 1) / 2) * z.astype(np.float64) / fy)
    z, x, y = np.concatenate(zs), np.concatenate(xs), np.concatenate(ys)
    n_vis = z.size
    order = rng.permutation(n_vis)                                  # a tile's entries are spread over the whole index range
    xyz = np.stack([x, y, z.astype(np.float64)], 1)[order]
    N = n_vis if P is None else int(P)
    means = np.zeros((N, 3), np.float32); means[:, 2] = -1.0        # padding: behind the camera, culled by both sides
    if P is None:
        rows = np.arange(n_vis)
    else:
        assert n_vis <= 2 * split_rows < N
        rows = np.concatenate([np.arange((n_vis + 1) // 2), np.arange(N - n_vis // 2, N)])
    means[rows] = xyz.astype(np.float32)
    means[rows, 2] = z[order]                                         # the depth words exactly as the recipe made them
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32)
    quat = np.zeros((N, 4), np.float32); quat[:, 0] = 1.0
    d = dict(means3D=t(means), opacities=t(rng.uniform(0.02, 0.1, (N, 1))), colors_precomp=t(rng.uniform(0, 1, (N, 3))),
             scales=t(np.full((N, 3), 1e-3, np.float32)), rotations=t(quat), viewmatrix=cam.world_view_transform.float(),
             projmatrix=cam.full_proj_transform.float(), campos=cam.camera_center.float(), bg=torch.tensor([0.1, 0.2, 0.3]),
             image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, sh_degree=0, scale_modifier=1.0)
    return Scene(name, d, {tile: None for tile, _ in clusters}, solo)


def _scene(name, H, W, spec, solo, seed, **kw):
    """spec = [(tile, intended regime, n, recipe, recipe kwargs)]"""
    rng = np.random.default_rng(seed + 1000)
    sc = make_scene(name, H, W, [(tile, recipe(n, rng, **rk)) for tile, _, n, recipe, rk in spec], solo, seed, **kw)
    return sc._replace(targets={tile: (regime, n) for tile, regime, n, _, _ in spec})


def _registers(n):          # the four register regimes on tiles 0, 5, 10, 15
    return [(0, "equal", n, z_equal, {}), (5, "one-pass", n, z_uniform, {}), (10, "digits", n, z_pile, {}), (15, "digits+ties", n, z_pile, dict(values=40))]


S, B = K["small_cap"], K["big_cap"]
# name -> (H, W, [(tile, intended regime, n, depth recipe, recipe kwargs)], solo, seed[, make_scene kwargs])
SPECS = {
    # ---- the four-wave instantiation alone (solo): own launch or inside the blend
    "solo-registers": (64, 64, _registers(400), True, 1),
    "solo-oversize": (64, 64, [(1, "slabs", S + 1, z_uniform, {}), (6, "global", 2400, z_slab_pile, dict(pile=1100)),
                                                             (11, "global", S + 8, z_equal, {})], True, 2),
    "lengths-one-pass": (64, 64, [(0, "equal", 1, z_equal, {})] + [
        (t, "one-pass", n, z_uniform, {}) for t, n in zip((1, 2, 3, 5, 6, 7, 9, 10), (63, 64, 65, 255, 256, 257, S - 1, S))], True, 3),
    "lengths-fallback": (64, 64, [(t, "equal", n, z_equal, {}) for t, n in zip((1, 2, 3), (63, 64, 65))] + [
        (t, "digits+ties", n, z_pile, dict(values=40)) for t, n in zip((5, 6, 7, 9, 10), (255, 256, 257, S - 1, S))], True, 4),
    # depth passes 1..4: the pile-to-outlier span under 2^9, 2^18, 2^27 ulps and above (z = 30 000 beside z = 0.25)
    "depth-passes": (64, 64, [
        (0, "digits+ties", 500, z_pile_ulps, dict(span_ulps=500)), (5, "digits+ties", 400, z_pile, dict(values=40, outlier=_f32([_b32(5.0) + (1 << 17)])[0])),
        (10, "digits+ties", 400, z_pile, dict(values=40, outlier=7.0)),
        (15, "digits+ties", 400, z_pile, dict(values=40, base=30000.0, outlier=0.25, step=5))], True, 5),
    # index passes 1 and 3 (2: every other scene): P <= 512, and P = 262 400 with the visible rows at both ends of the index range
    "index-pass-1": (32, 32, [(0, "equal", 90, z_equal, {}), (3, "digits+ties", 210, z_pile, dict(values=10))], True, 6),
    "index-pass-3": (32, 32, [(0, "equal", 300, z_equal, {}), (3, "digits+ties", 300, z_pile, dict(values=10))], True, 7,
                     dict(P=262400, split_rows=300)),
    # ---- both instantiations launched (capacity > 2048 x tiles): the four-wave one beside the eight-wave one
    "eight-lo": (64, 64, [(0, "equal", 400, z_equal, {}), (5, "one-pass", 400, z_uniform, {}),
                                                    (10, "one-pass", S + 1, z_uniform, {}), (15, "digits+ties", S + 1, z_pile, dict(values=40))], False, 8),
    "eight-hi-1": (64, 64, [(0, "digits", 400, z_pile, {}), (5, "digits+ties", 400, z_pile, dict(values=40)),
                                                        (10, "one-pass", B - 1, z_uniform, {}), (15, "digits+ties", B - 1, z_pile, dict(values=40))], False, 9),
    "eight-hi": (64, 64, [(10, "one-pass", B, z_uniform, {}), (15, "digits+ties", B, z_pile, dict(values=40))], False, 10),
    "eight-equal-digits": (64, 64, [(10, "equal", 3000, z_equal, {}), (15, "digits", 3000, z_pile, {})], False, 11),
    "eight-oversize": (64, 64, [(10, "slabs", B + 1, z_uniform, {}), (15, "global", B + 104, z_slab_pile, dict(pile=1100))], False, 12),
}


BUILDERS = {name: (lambda name=name: _scene(name, *SPECS[name][:5], **(SPECS[name][5] if len(SPECS[name]) > 5 else {}))) for name in SPECS}


def sites_of(name):
    """The launch sites a scene can be sorted at: a solo frame in launches of its own or inside the blend, the other kind in its own launches only."""
    return ("own", "blend") if SPECS[name][3] else ("own",)


def capacity_for(scene, st):
    """The capacity to pin so that the scene's `solo` holds: R itself for a solo frame; for the other kind the larger of R and one more
    than the solo rule's limit."""
    n_tiles, R = len(st["ranges"]), int(st["R"])
    if scene.solo:
        assert 0 < R <= K["solo_per_tile"] * n_tiles, (R, n_tiles)
        return R
    return max(R, K["solo_per_tile"] * n_tiles + 1)


def flags_for(site, ballot):
    return CALL_KEEP_ALL_INSTANCES | (CALL_SEPARATE_SORT if site == "own" else 0) | (CALL_BALLOT_RANK if ballot else 0)


def expected_plan(scene, site, ballot):
    return (SORT_IN_BLEND if site == "blend" else 0) | (0 if scene.solo else SORT_SECOND_INSTANTIATION) | (SORT_BALLOT_RANK if ballot else 0)


_oracle_cache = {}


def oracle_state(name):
    """(scene, full float32 oracle forward of it), computed once per process and shared; callers must not modify it."""
    if name not in _oracle_cache:
        from oracle.oracle import Oracle
        sc = BUILDERS[name]()
        _oracle_cache[name] = (sc, Oracle(np.float32, nthreads=8).forward(**sc.d))
    return _oracle_cache[name]


def reach(scene, st, site, ballot=False):
    """Check the scene against the oracle state (every rectangle in one tile, the targeted tiles' lengths exact, each in its intended
    regime outside the guard band, no list beyond the targeted tiles) -> the MATRIX cells it reaches at `site`."""
    assert int(np.asarray(st["tiles_touched"]).max()) == 1, "a splat's rectangle leaves its tile"
    infos = regime_of_tiles(st, capacity_for(scene, st), flags_for(site, ballot))
    assert set(infos) == set(scene.targets), (sorted(infos), sorted(scene.targets))
    for tile, (regime, n) in scene.targets.items():
        assert infos[tile].n == n, f"{scene.name}: tile {tile} holds {infos[tile].n} entries, built for {n}"
        check_guard_band(infos[tile], regime)
    return cells_of(infos.values(), scene.solo, site)
