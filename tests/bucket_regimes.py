"""A CPU model of the tile bucketing's launch geometry and count table (egogaussian_amd/csrc/bin_walk.h, binning.hip, the fused count pass
of preprocess.hip) and scene builders that put one small frame into each regime of the slot walk and the table scan.  Test infrastructure:
nothing here runs on a device, and nothing is taken from the library -- the constants are read from the sources by regex, the rectangles
come from the oracle (Oracle.forward(..., stop_after="binning")), and a builder asserts from the oracle's `rects` and `tiles_touched` that
the structure it intends is the one it got.

The bucketing in the model's words.  The Gaussians are cut into BLOCKS of 256 consecutive ones (four GROUPS of 64); block B belongs to
WORKGROUP B % nblocks and is its DEAL B // nblocks; the workgroup numbers its groups l = 4 * deal + (group inside the block) and takes them
`gpr` at a time: ROUND l // gpr.  A group's instances are SLOTS 0 .. sum(tiles_touched) - 1 in Gaussian order, walked 64 at a time; a slot
finds its Gaussian through the owner map (slots below BIN_MAP_SLOTS of a workgroup that has room for the map) or by binary search.  Every
workgroup leaves one column of the [tile][stride] count table; the table is scanned in chunks of 2048 entries, whose sums the count pass
accumulated; from EGS_CHUNK_PREFIX_MIN chunks on a one-workgroup kernel turns the chunk sums into prefixes first, 1024 chunks per
iteration with a carry between iterations."""
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL_SYNC, CALL_KEEP_ALL_INSTANCES, CALL_SEPARATE_COUNT = 1, 2, 4
TILE = 16
GEOMETRY_FIELDS = ("n_tiles", "gx", "nblocks", "stride", "n_chunks", "gpr", "cull", "use_map", "groups_per_block", "rounds", "prefixed", "can_fuse", "lds")


def read_constants():
    """The bucketing's constants, by regex from the sources (as tests/sort_regimes.py reads the sort's)."""
    src = lambda *p: open(os.path.join(ROOT, "egogaussian_amd", "csrc", *p)).read()
    bw, bn, ec, pp, bp = src("bin_walk.h"), src("binning.hip"), src("egs_common.h"), src("preprocess.hip"), src("backward_prologue.h")
    one = lambda pat, text: int(re.search(pat, text).group(1))
    m = re.search(r"return \(size_t\)gpr \* 64 \* (\d+) \+ (\d+) \+ \(cull \? \(size_t\)gpr \* 64 \* (\d+) : 0\) \+ \(map \? \(size_t\)gpr \* (\d+) : 0\);", bw)
    assert m, "bin_round_words is not the expression the model reads"
    c = dict(threads=one(r"#define\s+EGS_BIN_THREADS\s+(\d+)", ec), map_slots=one(r"#define\s+BIN_MAP_SLOTS\s+(\d+)", bw),
             round_words=tuple(int(x) for x in m.groups()), target_blocks=one(r"#define\s+EGS_BIN_TARGET_BLOCKS\s+(\d+)", bn),
             prefix_min=one(r"#define\s+EGS_CHUNK_PREFIX_MIN\s+(\d+)", bn), max_tiles=one(r"#define\s+EGS_MAX_TILES\s+(\d+)", ec),
             lds=1024 * one(r"room = (\d+) \* 1024 - counters", bn), half_lds=1024 * one(r"sizeof\(uint32_t\) > (\d+) \* 1024 &&", bn),
             chunk=one(r"const size_t rpc = (\d+) / stride", ec), min_stride=one(r"uint32_t s = (\d+); while \(s < bin_blocks\) s <<= 1", ec),
             groups=one(r"#define\s+EGS_BIN_GROUPS\s+(\d+)", ec), prefix_threads=one(r"__launch_bounds__\((\d+)\) void k_chunk_prefix", bn),
             order_levels=one(r"#define\s+ORDER_LEVELS\s+(\d+)", bp), order_balance=one(r"#define\s+ORDER_BALANCE_MAX\s+(\d+)", bp))
    assert c["chunk"] == one(r"#define\s+EGS_SCAN_THREADS\s+(\d+)", ec) * one(r"#define\s+EGS_SCAN_ITEMS\s+(\d+)", ec), "a scan chunk is one scan workgroup's share"
    assert one(r"for \(uint32_t k0 = 0; k0 < n_chunks; k0 \+= (\d+)\)", bn) == c["prefix_threads"]
    assert re.search(r"while \(gpr > 4 && !fits\(gpr, true\)\) gpr >>= 1;", bn) and re.search(r"if \(!cull\) while \(gpr > 1 && !fits\(gpr, false\)\) gpr >>= 1;", bn)
    assert re.search(r"return q\.gpr >= 4 && q\.gpr % 4 == 0 && q\.lds >= sizeof\(EgsOrderLds\);", pp)
    assert re.search(r"uint32_t level_base\[ORDER_LEVELS\], level_fill\[ORDER_LEVELS\], wsum\[16\], wmax;\s*uint4 quad_cost\[ORDER_BALANCE_MAX\];[^\n]*\s*uint16_t sorted_tile\[ORDER_BALANCE_MAX\];", bp)
    assert re.search(r"return 4u \* \(bid \+ nblocks \* \(l >> 2\)\) \+ \(l & 3u\);", bw), "the block deal is B = bid + nblocks * (l / 4)"
    return c


K = read_constants()
WAVES = K["threads"] // 64
align16 = lambda x: (x + 15) & ~15
ORDER_LDS = align16(align16(4 * (2 * K["order_levels"] + 16 + 1)) + 16 * K["order_balance"] + 2 * K["order_balance"])     # sizeof(EgsOrderLds)


def round_words(gpr, cull, use_map):
    """bin_walk.h bin_round_words: LDS words of a round of `gpr` groups behind the per-tile counters."""
    a, b, c, d = K["round_words"]
    return gpr * 64 * a + b + (gpr * 64 * c if cull else 0) + (gpr * d if use_map else 0)


def geometry_model(P, W, H, cull):
    """binning.hip egs_bin_geometry, bin_walk.h bin_groups_per_block, preprocess.hip egs_can_fuse_count (without its environment switch) and the
    prefix rule of egs_launch_binning, in Python -> a dict of GEOMETRY_FIELDS (what egs_forward_bin_geometry returns)."""
    gx = (W + TILE - 1) // TILE
    n_tiles = gx * ((H + TILE - 1) // TILE)
    q = dict.fromkeys(GEOMETRY_FIELDS, 0)
    q.update(n_tiles=n_tiles, gx=gx)
    if P <= 0:
        return q
    k = (P + 256 * K["target_blocks"] - 1) // (256 * K["target_blocks"])
    gpb = 256 * max(k, 1)
    nblocks = (P + gpb - 1) // gpb
    counters = ((n_tiles + 3) & ~3) * 4
    room = K["lds"] - counters
    cull = 1 if cull else 0
    use_map = round_words(WAVES, cull, True) * 4 <= room
    fits = lambda g, c: round_words(g, c, use_map) * 4 <= room
    gpr = WAVES
    if cull:
        while gpr > 4 and not fits(gpr, True):
            gpr >>= 1
        if not fits(gpr, True):
            cull, gpr = 0, WAVES
    if not cull:
        while gpr > 1 and not fits(gpr, False):
            gpr >>= 1
    if gpr == WAVES and counters + round_words(gpr, cull, use_map) * 4 > K["half_lds"] and counters + round_words(gpr // 2, cull, use_map) * 4 <= K["half_lds"]:
        gpr //= 2
    lds = counters + round_words(gpr, cull, use_map) * 4
    stride = K["min_stride"]
    while stride < nblocks:
        stride <<= 1
    rpc = K["chunk"] // stride
    n_chunks = (n_tiles + rpc - 1) // rpc
    blocks256 = (P + 255) // 256
    per_block = 4 * ((blocks256 + nblocks - 1) // nblocks)
    q.update(nblocks=nblocks, stride=stride, n_chunks=n_chunks, gpr=gpr, cull=cull, use_map=int(use_map), groups_per_block=per_block,
             rounds=(per_block + gpr - 1) // gpr, prefixed=int(n_chunks >= K["prefix_min"]), lds=lds,
             can_fuse=int(per_block <= gpr and gpr >= 4 and gpr % 4 == 0 and lds >= ORDER_LDS))
    return q


def geometry_of(st, cull):
    return geometry_model(int(st["P"]), int(st["W"]), int(st["H"]), cull)


def owner_of(st, cull_off, geo=None):
    """Which Gaussian belongs to which 256-block, workgroup, deal, local group, round, group of the round and lane (arrays of P entries).
    Culling off: also `slots` [ceil(P / 64)], each 64-Gaussian group's slot total, and `span` [P], a Gaussian's first slot inside its group
    (the walk's slots are then the reference's rectangles: the oracle's tiles_touched)."""
    P = int(st["P"])
    geo = geo or geometry_of(st, not cull_off)
    i = np.arange(P, dtype=np.int64)
    blk = i >> 8
    wg, deal = blk % geo["nblocks"], blk // geo["nblocks"]
    l = 4 * deal + ((i >> 6) & 3)
    own = dict(block=blk, workgroup=wg, deal=deal, local_group=l, round=l // geo["gpr"], group_in_round=l % geo["gpr"], lane=i & 63, group=i >> 6)
    if cull_off:
        tt = np.asarray(st["tiles_touched"]).astype(np.int64)
        own["slots"] = np.bincount(i >> 6, weights=tt, minlength=(P + 63) // 64).astype(np.int64)
        incl = np.cumsum(tt)
        first = np.repeat((incl - tt)[::64], 64)[:P]                       # the scan's value at the group's first Gaussian
        own["span"] = incl - tt - first
    return own


def instances_of_rects(st):
    """(tile, Gaussian) of every instance of the oracle's rectangles, in Gaussian order, row-major inside a rectangle."""
    rects = np.asarray(st["rects"]).astype(np.int64)
    tt = np.asarray(st["tiles_touched"]).astype(np.int64)
    assert np.array_equal(tt, (rects[:, 2] - rects[:, 0]) * (rects[:, 3] - rects[:, 1]))
    ids = np.repeat(np.arange(len(tt), dtype=np.int64), tt)
    off = np.arange(ids.size, dtype=np.int64) - np.repeat(np.cumsum(tt) - tt, tt)
    wd = (rects[:, 2] - rects[:, 0])[ids]
    gx = (int(st["W"]) + TILE - 1) // TILE
    return (rects[ids, 1] + off // wd) * gx + rects[ids, 0] + off % wd, ids


VARIANTS = ("skip-second-round", "count-unused-columns", "drop-chunk-carry", "no-interleave")


def table_reference(st, geo, lists=None, variant=None):
    """The exclusive-scanned [tile][workgroup] count table in numpy -> (table uint32 [n_tiles, nblocks], total).
    Instances: the oracle's rectangles (culling off), or -- lists = (ranges [n_tiles, 2], point_list) -- the entries of a culled frame's own
    lists, which tests/common.py check_culled_lists holds to the oracle separately.  Column = the Gaussian's workgroup under the block deal.
    variant: one of VARIANTS, a deliberately WRONG table (what a kernel with that defect would leave), for the tests of the check itself."""
    assert variant is None or variant in VARIANTS
    n_tiles, nblocks, stride = geo["n_tiles"], geo["nblocks"], geo["stride"]
    own = owner_of(st, False, geo)
    if lists is None:
        tile, ids = instances_of_rects(st)
    else:
        ranges, pl = np.asarray(lists[0]).astype(np.int64), np.asarray(lists[1]).astype(np.int64)
        n = ranges[:, 1] - ranges[:, 0]
        tile, ids = np.repeat(np.arange(n_tiles, dtype=np.int64), n), pl[:int(n.sum())]
    wg = own["workgroup"][ids]
    if variant == "no-interleave":                                          # consecutive blocks to one workgroup
        wg = own["block"][ids] // (geo["groups_per_block"] // 4)
    if variant == "skip-second-round":
        keep = own["round"][ids] == 0
        tile, wg = tile[keep], wg[keep]
    raw = np.zeros(n_tiles * stride, np.uint32)                             # the table as the count pass leaves it: [tile][stride]
    np.add.at(raw, tile * stride + wg, 1)
    if variant == "count-unused-columns":                                   # columns >= nblocks hold whatever the buffer held
        raw.reshape(n_tiles, stride)[:, nblocks:] = 1
    scanned = np.cumsum(raw, dtype=np.uint32) - raw
    if variant == "drop-chunk-carry":
        # the chunk prefix restarts: every k_chunk_prefix iteration (a prefixed table), at every chunk (the others)
        span = K["chunk"] * (K["prefix_threads"] if geo["prefixed"] else 1)
        first = (np.arange(raw.size, dtype=np.int64) // span) * span
        scanned = scanned - scanned[first]
    return scanned.reshape(n_tiles, stride)[:, :nblocks], int(raw.sum(dtype=np.uint64))


def check_table(got, got_total, want, want_total, geo=None):
    """The check the GPU tests hold the scanned table to: every (tile, workgroup) entry and the total, bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.int32:
        got = got.view(np.uint32)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (got.shape, want.shape, got.dtype)
    if int(got_total) == int(want_total) and np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    where = ""
    if len(bad):
        t, b = (int(x) for x in bad[0])
        where = f", first at tile {t} (chunk {t * geo['stride'] // K['chunk']})" if geo else f", first at tile {t}"
        where += f", workgroup {b}: {int(got[t, b])}, expected {int(want[t, b])}"
    raise AssertionError(f"scanned count table: {len(bad)} of {got.size} entries differ{where}; total {int(got_total)}, expected {int(want_total)}")


def decode_model(kk, wd, rcp_ulps=0):
    """bin_walk.h bin_walk_round's slot decode in numpy float32, operation by operation: row = (uint32)((float)kk * rcp(wd)), col = kk - row * wd,
    then the two repair lines.  rcp_ulps: the reciprocal moved that many float32 steps from the correctly rounded one (the hardware's
    reciprocal is good to one).  -> (row, col, the slots whose first guess had col < 0, the slots whose first guess had col >= wd)"""
    assert re.search(r"uint32_t row = \(uint32_t\)\(\(float\)kk \* __builtin_amdgcn_rcpf\(\(float\)wd\)\);", open(os.path.join(ROOT, "egogaussian_amd", "csrc", "bin_walk.h")).read())
    kk = np.asarray(kk, dtype=np.int64)
    rcp = np.float32(1.0) / np.float32(wd)
    for _ in range(abs(rcp_ulps)):
        rcp = np.nextafter(rcp, np.float32(np.inf if rcp_ulps > 0 else 0.0), dtype=np.float32)
    row = (kk.astype(np.float32) * rcp).astype(np.int64)
    col = kk - row * wd
    low, high = col < 0, col >= wd
    row, col = np.where(low, row - 1, row), np.where(low, col + wd, col)
    high = col >= wd
    row, col = np.where(high, row + 1, row), np.where(high, col - wd, col)
    return row, col, low, high


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
Scene = namedtuple("Scene", "name d cells expect info")       # cells: what reach() must find; expect: {cull: geometry fields the case is built for}


def _camera(H, W):
    from egogaussian_amd.scene_synth import make_camera
    cam = make_camera(0, H, W)                                              # frame 0: the view matrix is the identity, depth = z
    tanx, tany = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    return cam, tanx, tany, W / (2 * tanx), H / (2 * tany)


def make_scene(name, H, W, P, rows, px, py, radius=None, z=None, opacity=0.5, cov=None, seed=0, cells=(), expect=None, info=None):
    """col_cov inputs of P Gaussians, of which `rows` are in front of the identity camera with their centres at pixel (px, py) and depth z
    (default: seeded uniform in [3, 7]); every other row lies behind the camera.  radius (per row; None: 2, the 0.3 px^2 blur's): an isotropic
    covariance sized so that the projected 3-sigma radius comes out as that integer (aimed half a pixel below it: the oracle rounds up);
    cov: {position in rows: 3x3 world covariance} replaces it.  What the rectangles then ARE is the oracle's business (reach())."""
    rng = np.random.default_rng(seed)
    cam, tanx, tany, fx, fy = _camera(H, W)
    rows = np.asarray(rows, dtype=np.int64)
    n = rows.size
    assert n == np.unique(rows).size and (n == 0 or (rows.min() >= 0 and rows.max() < P))
    px, py = np.broadcast_to(np.asarray(px, np.float64), n), np.broadcast_to(np.asarray(py, np.float64), n)
    z = rng.uniform(3.0, 7.0, n) if z is None else np.broadcast_to(np.asarray(z, np.float64), n)
    x, y = (px - (W - 1) / 2) * z / fx, (py - (H - 1) / 2) * z / fy
    s2 = np.full(n, 1e-6)
    if radius is not None:
        r = np.broadcast_to(np.asarray(radius, np.float64), n)
        u, v = np.clip(x / z, -1.3 * tanx, 1.3 * tanx), np.clip(y / z, -1.3 * tany, 1.3 * tany)
        a, b = fx / z, fy / z
        m00, m01, m11 = a * a * (1 + u * u), a * b * u * v, b * b * (1 + v * v)
        lam = 0.5 * (m00 + m11) + np.sqrt(0.25 * (m00 - m11) ** 2 + m01 ** 2)
        s2 = np.where(r > 2, (((r - 0.5) / 3) ** 2 - 0.3) / lam, s2)
    means = np.zeros((P, 3), np.float32); means[:, 2] = -1.0
    means[rows] = np.stack([x, y, z], 1).astype(np.float32)
    c6 = np.zeros((P, 6), np.float32); c6[:, [0, 3, 5]] = 1e-6
    c6[rows] = (s2[:, None] * np.array([1, 0, 0, 1, 0, 1.0])[None, :]).astype(np.float32)
    for k, S in (cov or {}).items():
        c6[rows[k]] = np.asarray(S, np.float64)[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(np.float32)
    op = np.full((P, 1), 0.5, np.float32)
    op[rows, 0] = np.broadcast_to(np.asarray(opacity, np.float32), n)
    col = np.random.default_rng(seed + 1).uniform(0, 1, (P, 3)).astype(np.float32)
    t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_, dtype=np.float32))
    d = dict(means3D=t(means), opacities=t(op), colors_precomp=t(col), cov3D_precomp=t(c6), viewmatrix=cam.world_view_transform.float(),
             projmatrix=cam.full_proj_transform.float(), campos=cam.camera_center.float(), bg=torch.tensor([0.1, 0.2, 0.3]),
             image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, sh_degree=0, scale_modifier=1.0)
    return Scene(name, d, tuple(cells), expect or {}, dict(info or {}, rows=rows))


def _scatter(rng, n, H, W, rmax):
    """n splats anywhere on the image, radii 2 .. rmax"""
    return rng.uniform(0, W, n), rng.uniform(0, H, n), rng.integers(2, rmax + 1, n).astype(np.float64)


# -- tiny tables: every Gaussian on screen
TINY_P = (1, 63, 64, 65, 255, 256, 257, 300, 1000, 1025, 2100)
TINY_SIZES = ((48, 48), (80, 64), (270, 480))                               # (H, W): 9, 20 and 510 tiles


def _tiny(P, H, W):
    rng = np.random.default_rng(1000 * P + W)
    px, py, r = _scatter(rng, P, H, W, 24)
    geo = geometry_model(P, W, H, True)
    cells = [f"table/stride-{geo['stride']}", f"table/nblocks-{geo['nblocks']}", f"table/chunks-{geo['n_chunks']}"]
    cells += ["table/padding-workgroups"] if geo["nblocks"] % 8 else []
    cells += ["table/unused-columns"] if geo["nblocks"] < geo["stride"] else []
    cells += ["table/tail-not-whole"] if (geo["n_tiles"] * geo["stride"]) % 8 else []
    cells += ["table/partial-last-group"] if P % 64 else []
    cells += ["table/partial-last-block"] if P % 256 else []
    return make_scene(f"tiny-{P}-{W}x{H}", H, W, P, np.arange(P), px, py, r, seed=P + W, cells=cells,
                      expect={c: dict(rounds=1, use_map=1, gpr=WAVES, prefixed=0, can_fuse=1) for c in (0, 1)})


# -- decode: one Gaussian per rectangle width at full height, anchored at the left and at the right edge of a 30 x 17 image
def _decode():
    H, W, R = 270, 480, 260                                                # (2 R >= the image's width: the far side of every rectangle is clamped)
    wd = np.arange(1, 31)
    px = np.concatenate([16 * wd - 7 - R, 16 * (30 - wd) + 8 + R]).astype(np.float64)      # x1 = wd: px + R = 16 wd - 7; x0 = 30 - wd: px - R = 16 x0 + 8
    cells = [f"decode/{side}/wd-{k}" for side in ("left", "right") for k in wd]
    return make_scene("decode", H, W, 60, np.arange(60), px, 134.5, float(R), cells=cells + ["walk/map-and-search"],
                      expect={0: dict(use_map=1, rounds=1, nblocks=1)}, info=dict(cull=(0,)))


# -- decode, wide: widths 31 .. 61 on a 61 x 3 image.  From width 41 on there are widths whose CORRECTLY ROUNDED float32 reciprocal, times the
#    offset of a row boundary, falls short of the row (41 * (1 / 41) = 0.99999994): the first guess is a row short and the repair line runs
WIDE = tuple(range(31, 62))


def _decode_wide():
    H, W, R = 48, 976, 500
    wd = np.array(WIDE)
    return make_scene("decode-wide", H, W, len(WIDE), np.arange(len(WIDE)), (16 * wd - 7 - R).astype(np.float64), 23.5, float(R),
                      cells=[f"decode/wide/wd-{k}" for k in WIDE] + ["decode/first-guess-a-row-short", "walk/map-and-search"],
                      expect={0: dict(use_map=1, rounds=1, nblocks=1)}, info=dict(cull=(0,)))


# -- long group: 64 consecutive Gaussians of >= 65 tiles each (a group of more than BIN_MAP_SLOTS slots) and a group of a single 510-tile
#    Gaussian among empty lanes
def _long_group():
    H, W = 270, 480
    rng = np.random.default_rng(5)
    rows = np.concatenate([np.arange(64), [128 + 17]])
    px = np.concatenate([rng.uniform(100, 380, 64), [240.0]])
    py = np.concatenate([rng.uniform(90, 180, 64), [134.5]])
    r = np.concatenate([rng.integers(70, 120, 64), [400]]).astype(np.float64)
    return make_scene("long-group", H, W, 256, rows, px, py, r, seed=5, cells=("walk/map-and-search", "walk/span-straddles-the-map", "walk/lone-span"),
                      expect={0: dict(use_map=1, rounds=1, nblocks=1)}, info=dict(cull=(0,)))


# -- block deal: a workgroup of two 256-blocks, the second one dealt nblocks further on
def _block_deal():
    H, W, P = 64, 64, 131300
    rows = np.concatenate([np.arange(256), 256 * 257 + np.arange(256), [P - 1]])
    rng = np.random.default_rng(6)
    px, py, r = _scatter(rng, rows.size, H, W, 12)
    g = dict(nblocks=257, stride=512, groups_per_block=8, rounds=1, use_map=1)
    return make_scene("block-deal", H, W, P, rows, px, py, r, seed=6, cells=("deal/second-deal-block", "deal/tail-block", "table/stride-512", "table/nblocks-257",
                                                                              "table/padding-workgroups", "table/unused-columns"), expect={0: g, 1: g})


# -- two rounds with the owner map: 20 groups per workgroup in rounds of 16 + 4
def _two_rounds_mapped():
    H, W, P = 64, 64, 524800
    nb = 410
    rows = [np.arange(256) + 256 * B for B in (0, 3 * nb, 4 * nb)]                                   # workgroup 0: both rounds full of work
    for b in (7, 200, 409):                                                                           # three more: a few rows of every deal
        rows += [256 * (b + nb * deal) + np.array([0, 63, 64, 130, 255]) for deal in range(5)]
    rows = np.unique(np.concatenate(rows + [[P - 1]]))
    rng = np.random.default_rng(7)
    px, py, r = _scatter(rng, rows.size, H, W, 12)
    g = dict(nblocks=nb, stride=512, gpr=16, groups_per_block=20, rounds=2, use_map=1, can_fuse=0)
    return make_scene("two-rounds-mapped", H, W, P, rows, px, py, r, seed=7, cells=("rounds/two", "rounds/last-round-partly-filled", "rounds/row-P-1-in-the-last-round",
                                                                                    "rounds/second-round-over-a-used-block"), expect={0: g, 1: g})


def _big_rows(rng, P, nblocks, n):
    """n rows spread over the model, with rows of both deals of workgroups 0 and 5, and row P - 1"""
    rows = [rng.integers(0, P, n), np.arange(40), 256 * nblocks + np.arange(40), 256 * 5 + np.arange(0, 256, 9)]
    if P > 256 * (nblocks + 5):
        rows.append(256 * (nblocks + 5) + np.arange(0, 256, 7))
    rows = np.unique(np.concatenate(rows + [[P - 1]]))
    return rows[rows < P]


def _on_tiles(rng, rows, H, W, chunk_tiles):
    """centres: the first splats at the centres of the tiles named (one tile each), the rest anywhere with radii up to 24"""
    gx = (W + 15) // 16
    px, py, r = _scatter(rng, rows.size, H, W, 24)
    k = len(chunk_tiles)
    t = np.asarray(chunk_tiles)
    px[:k], py[:k], r[:k] = (t % gx) * 16 + 7.5, (t // gx) * 16 + 7.5, 2
    return px, py, r


# -- prefix threshold: the same model on 4096 chunks (prefix pass) and 4064 (none)
def _prefix(H):
    W, P = 2048, 65700
    geo = geometry_model(P, W, H, True)
    rpc = K["chunk"] // geo["stride"]
    chunks = sorted({0, 1023, 1024, geo["n_chunks"] - 1})
    rng = np.random.default_rng(8)
    rows = _big_rows(rng, P, 257, 2000)
    px, py, r = _on_tiles(rng, rows, H, W, [c * rpc + 1 for c in chunks])
    on = geo["n_chunks"] >= K["prefix_min"]
    g = dict(nblocks=257, stride=512, n_chunks=geo["n_chunks"], prefixed=int(on), rounds=1, use_map=1)
    return make_scene(f"prefix-{'on' if on else 'off'}", H, W, P, rows, px, py, r, seed=8, cells=(f"prefix/{'on' if on else 'off'}", "prefix/chunks-0-1023-1024-last") +
                      (("prefix/carry-across-iterations",) if on else ()), expect={0: g, 1: g}, info=dict(chunks=chunks))


# -- the largest image: no room for the owner map; two rounds of four groups with culling, one round of eight without
def _no_map():
    H, W, P = 2304, 4096, 131300
    geo = geometry_model(P, W, H, True)
    rpc = K["chunk"] // geo["stride"]
    chunks = sorted({0, 1023, 1024, 2048, 8191, 8192, geo["n_chunks"] - 1})
    rng = np.random.default_rng(9)
    rows = _big_rows(rng, P, 257, 3000)
    px, py, r = _on_tiles(rng, rows, H, W, [c * rpc + 2 for c in chunks])
    base = dict(nblocks=257, stride=512, n_chunks=9216, prefixed=1, use_map=0, groups_per_block=8)
    return make_scene("no-map", H, W, P, rows, px, py, r, seed=9, cells=("rounds/two-search-only", "rounds/one-search-only", "prefix/on", "prefix/nine-iterations",
                                                                         "deal/second-deal-block", "deal/tail-block"),
                      expect={1: dict(base, gpr=4, rounds=2, cull=1, can_fuse=0), 0: dict(base, gpr=8, rounds=1, cull=0)}, info=dict(chunks=chunks))


# -- box cut: what the culling walk's set-up does to a rectangle before any slot is dealt
def _box_cut():
    H, W = 270, 480
    c, s = math.cos(math.radians(45)), math.sin(math.radians(45))
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    z = 5.0
    fx = _camera(H, W)[3]
    long_, short_ = 40 * z / fx, 1.5 * z / fx                                # 40 px and 1.5 px standard deviations on the image
    elong = Rz @ np.diag([long_ ** 2, short_ ** 2, short_ ** 2]) @ Rz.T
    rng = np.random.default_rng(10)
    px, py, r = _scatter(rng, 40, H, W, 30)
    px[:3], py[:3], r[:3] = (240, 240, -40), (134.5, 134.5, 134.5), (100, 2, 90)
    op = np.full(40, 0.6); op[:3] = (0.003, 0.9, 0.02)
    return make_scene("box-cut", H, W, 300, np.arange(40) * 7, px, py, r, z=z, opacity=op, cov={1: elong}, seed=10,
                      cells=("cut/empty-box", "cut/ellipse-corners", "cut/clipped-box"), expect={1: dict(cull=1, use_map=1, rounds=1)}, info=dict(cull=(1,), faint=0, elongated=7, clipped=14))


BUILDERS = {f"tiny-{P}-{W}x{H}": (lambda P=P, H=H, W=W: _tiny(P, H, W)) for H, W in TINY_SIZES for P in TINY_P}
BUILDERS.update({"decode": _decode, "decode-wide": _decode_wide, "long-group": _long_group, "block-deal": _block_deal, "two-rounds-mapped": _two_rounds_mapped,
                 "prefix-on": lambda: _prefix(2048), "prefix-off": lambda: _prefix(2032), "no-map": _no_map, "box-cut": _box_cut})

CELLS = sorted(set(
    [f"table/stride-{s}" for s in (4, 8, 16, 512)] + [f"table/nblocks-{n}" for n in (1, 2, 4, 5, 9, 257)] + ["table/chunks-1", "table/chunks-2", "table/chunks-4"] +
    ["table/padding-workgroups", "table/unused-columns", "table/tail-not-whole", "table/partial-last-group", "table/partial-last-block"] +
    [f"decode/{side}/wd-{k}" for side in ("left", "right") for k in range(1, 31)] +
    [f"decode/wide/wd-{k}" for k in WIDE] + ["decode/first-guess-a-row-short"] +
    ["walk/map-and-search", "walk/span-straddles-the-map", "walk/lone-span", "deal/second-deal-block", "deal/tail-block"] +
    ["rounds/two", "rounds/last-round-partly-filled", "rounds/row-P-1-in-the-last-round", "rounds/second-round-over-a-used-block", "rounds/two-search-only", "rounds/one-search-only"] +
    ["prefix/on", "prefix/off", "prefix/chunks-0-1023-1024-last", "prefix/carry-across-iterations", "prefix/nine-iterations"] +
    ["cut/empty-box", "cut/ellipse-corners", "cut/clipped-box"]))


def culls_of(scene):
    """the culling settings a scene is run with (True: tile culling on)"""
    return tuple(bool(c) for c in scene.info.get("cull", (0, 1)))


_oracle_cache = {}


def oracle_state(name):
    """(scene, float32 oracle state up to the sorted lists), computed once per process and shared; callers must not modify it."""
    if name not in _oracle_cache:
        from oracle.oracle import Oracle
        sc = BUILDERS[name]()
        _oracle_cache[name] = (sc, Oracle(np.float32, nthreads=8).forward(stop_after="binning", **sc.d))
    return _oracle_cache[name]


def max_alpha_per_tile(st, i):
    """float64: the largest alpha Gaussian i reaches on any pixel of each tile of its rectangle -> ([rows, cols] array, rect)"""
    x0, y0, x1, y1 = (int(v) for v in st["rects"][i])
    W, H = int(st["W"]), int(st["H"])
    xs, ys = np.arange(x0 * 16, min(x1 * 16, W)), np.arange(y0 * 16, min(y1 * 16, H))
    a, b, c, o = (float(v) for v in st["conic_opacity"][i])
    dx, dy = float(st["xy"][i, 0]) - xs[None, :], float(st["xy"][i, 1]) - ys[:, None]
    power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
    alpha = np.where(power > 0, 0.0, np.minimum(0.99, o * np.exp(np.minimum(power, 0.0))))
    out = np.zeros((y1 - y0, x1 - x0))
    for ty in range(y1 - y0):
        for tx in range(x1 - x0):
            blk = alpha[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
            out[ty, tx] = blk.max() if blk.size else 0.0
    return out, (x0, y0, x1, y1)


def reach(scene, st):
    """The cells a scene PROVABLY reaches, from the oracle state and the model of the geometry alone (every claim is an assertion on the
    oracle's rects / tiles_touched / ranges; a builder that misses its structure fails here) -> set of CELLS."""
    P, W, H = int(st["P"]), int(st["W"]), int(st["H"])
    rects, tt = np.asarray(st["rects"]).astype(np.int64), np.asarray(st["tiles_touched"]).astype(np.int64)
    vis = tt > 0
    rows = scene.info["rows"]
    assert np.array_equal(np.nonzero(vis)[0], rows), f"{scene.name}: the rows on screen are not the rows built ({int(vis.sum())} of {rows.size})"
    cells = set()
    name = scene.name
    geos = {c: geometry_of(st, c) for c in culls_of(scene)}
    for c, g in geos.items():
        for k, v in scene.expect.get(int(c), {}).items():
            assert g[k] == v, f"{name}: the model's geometry has {k} = {g[k]}, the case is built for {v} (culling {'on' if c else 'off'})"
    g = next(iter(geos.values()))
    own = owner_of(st, True, geos.get(False) or g)
    n_entries = g["n_tiles"] * g["stride"]
    if name.startswith("tiny-"):
        cells |= {f"table/stride-{g['stride']}", f"table/nblocks-{g['nblocks']}", f"table/chunks-{g['n_chunks']}"}
        assert g["n_chunks"] == (n_entries + K["chunk"] - 1) // K["chunk"]
        if g["nblocks"] % 8:
            cells.add("table/padding-workgroups")
        if g["nblocks"] < g["stride"]:
            cells.add("table/unused-columns")
        if n_entries % 8:                                                    # the last thread's eight entries straddle the end of the table
            assert n_entries % 4 == 0
            cells.add("table/tail-not-whole")
        if P % 64 and vis[P - 1]:
            cells.add("table/partial-last-group")
        if P % 256 and vis[P - 1]:
            cells.add("table/partial-last-block")
        assert np.unique(own["workgroup"][vis]).size == g["nblocks"], "a workgroup without work"
    if name == "decode":
        for k in range(30):
            assert tuple(rects[k]) == (0, 0, k + 1, 17), (k, rects[k])
            assert tuple(rects[30 + k]) == (30 - (k + 1), 0, 30, 17), (k, rects[30 + k])
            cells |= {f"decode/left/wd-{k + 1}", f"decode/right/wd-{k + 1}"}
    if name == "decode-wide":
        short = []
        for k, w in enumerate(WIDE):
            assert tuple(rects[k]) == (0, 0, w, 3), (w, rects[k])
            cells.add(f"decode/wide/wd-{w}")
            short += [(w, int(kk)) for kk in np.nonzero(decode_model(np.arange(3 * w), w)[3])[0]]
        assert {w for w, _ in short} >= {41, 47, 55, 61} and all(kk % w == 0 for w, kk in short), short
        cells.add("decode/first-guess-a-row-short")                          # (with a correctly rounded reciprocal; the hardware's is within one step of it)
    if name in ("decode", "decode-wide", "long-group"):
        grp = int(np.argmax(own["slots"]))
        assert g["use_map"] and own["slots"][grp] > K["map_slots"] + 64
        cells.add("walk/map-and-search")                                     # units on both sides of slot BIN_MAP_SLOTS in one group
    if name == "long-group":
        assert np.all(tt[:64] >= 65) and own["slots"][0] >= 65 * 64
        sp, e = own["span"][:64], own["span"][:64] + tt[:64]
        assert np.any((sp < K["map_slots"]) & (e > K["map_slots"])) and np.any(sp > K["map_slots"])
        cells.add("walk/span-straddles-the-map")
        assert tt[145] == 510 and tt[128:192].sum() == 510 and g["n_tiles"] == 510
        cells.add("walk/lone-span")
    if name in ("block-deal", "no-map"):
        assert g["groups_per_block"] == 8 and np.any(vis & (own["deal"] == 1)) and np.any(vis & (own["deal"] == 0))
        both = np.intersect1d(own["workgroup"][vis & (own["deal"] == 0)], own["workgroup"][vis & (own["deal"] == 1)])
        assert both.size, "no workgroup with work in both of its blocks"
        cells.add("deal/second-deal-block")
        assert vis[P - 1] and P % 256 and own["deal"][P - 1] == 1
        cells.add("deal/tail-block")
    if name == "block-deal":
        assert g["stride"] == 512 and g["nblocks"] == 257 and vis[:256].all() and vis[256 * 257:256 * 258].all()
        cells |= {"table/stride-512", "table/nblocks-257", "table/padding-workgroups", "table/unused-columns"}
    if name == "two-rounds-mapped":
        for c, gg in geos.items():
            assert (gg["rounds"], gg["gpr"], gg["groups_per_block"], gg["use_map"]) == (2, 16, 20, 1)
        per_wg = {int(b): set(own["round"][vis & (own["workgroup"] == b)].tolist()) for b in (0, 7, 200, 409)}
        assert all(v == {0, 1} for v in per_wg.values()), per_wg
        cells.add("rounds/two")
        assert g["groups_per_block"] % g["gpr"] == 4
        cells.add("rounds/last-round-partly-filled")
        assert vis[P - 1] and own["round"][P - 1] == 1 and own["workgroup"][P - 1] == 409
        cells.add("rounds/row-P-1-in-the-last-round")
        r0 = vis & (own["workgroup"] == 0) & (own["round"] == 0)
        assert set(own["group_in_round"][r0].tolist()) >= {0, 1, 2, 3} and np.any(vis & (own["workgroup"] == 0) & (own["round"] == 1))
        cells.add("rounds/second-round-over-a-used-block")                   # groups 0..3 of round 1 are parked where round 0's were
    if name.startswith("prefix-") or name == "no-map":
        tile, _ = instances_of_rects(st)
        rpc = K["chunk"] // g["stride"]
        have = set(np.unique(tile // rpc).tolist())
        assert set(scene.info["chunks"]) <= have, (scene.info["chunks"], sorted(have)[:8])
        assert {0, 1023, 1024, g["n_chunks"] - 1} <= have
        cells.add("prefix/chunks-0-1023-1024-last" if name != "no-map" else "prefix/on")
        cells.add("prefix/on" if g["prefixed"] else "prefix/off")
        if g["prefixed"]:
            assert g["n_chunks"] > K["prefix_threads"] and min(have) < K["prefix_threads"] <= max(have)
            if name != "no-map":
                cells.add("prefix/carry-across-iterations")
    if name == "no-map":
        assert (g["n_chunks"] + K["prefix_threads"] - 1) // K["prefix_threads"] == 9 and {2048, 8191, 8192} <= have
        cells.add("prefix/nine-iterations")
        gc, gk = geos[True], geos[False]
        assert (gc["cull"], gc["use_map"], gc["gpr"], gc["rounds"]) == (1, 0, 4, 2) and (gk["use_map"], gk["gpr"], gk["rounds"]) == (0, 8, 1)
        oc = owner_of(st, False, gc)
        both = [b for b in (0, 5) if set(oc["round"][vis & (oc["workgroup"] == b)].tolist()) == {0, 1}]
        assert both == [0, 5]
        assert tt.max() > 1                                                  # spans of more than one slot under the search
        cells |= {"rounds/two-search-only", "rounds/one-search-only"}
    if name == "box-cut":
        i = scene.info["faint"]
        assert tt[i] >= 100 and float(st["conic_opacity"][i, 3]) < 1.0 / 255.0
        cells.add("cut/empty-box")
        i = scene.info["elongated"]
        ma, _ = max_alpha_per_tile(st, i)
        dead = ma < 0.9 / 255.0
        assert tt[i] >= 36 and dead[0, 0] and dead[-1, -1] and (~dead).sum() >= 6 and dead.sum() >= tt[i] // 3, (tt[i], dead.sum())
        cells.add("cut/ellipse-corners")
        i = scene.info["clipped"]
        ma, (x0, y0, x1, y1) = max_alpha_per_tile(st, i)
        live_cols = np.nonzero((ma >= 1.0 / 255.0).any(0))[0]
        assert x0 == 0 and x1 >= 3 and live_cols.size and live_cols.max() < x1 - 1 - x0 and float(st["xy"][i, 0]) < 0, (x0, x1, live_cols)
        cells.add("cut/clipped-box")                                         # the box ends inside the rectangle on the right, at the image's edge on the left
    assert cells <= set(CELLS), sorted(cells - set(CELLS))
    missing = set(scene.cells) - cells
    assert not missing, f"{name}: built for {sorted(missing)}, not reached"
    return cells


def flags_for(cull, fused):
    return (0 if cull else CALL_KEEP_ALL_INSTANCES) | (0 if fused else CALL_SEPARATE_COUNT)
