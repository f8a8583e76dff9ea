"""The model-bookkeeping kernels -- the shared u32 scan (binning.hip egs_launch_scan_u32), the densify / prune plan, the gathers and the
split-children kernel (densify.hip), the 3-NN statistic (knn.hip) -- held to plain references.  Input builders, NumPy references (float64
where values are involved), deliberately wrong variants and the checks themselves; tests/test_gpu_bookkeeping.py hands the checks the
kernels' output, tests/test_bookkeeping_cpu.py hands them the references' own output and the wrong variants.  No bar in here comes from a
kernel's output: the integer checks are exact, the two value checks carry their derivation."""
import os

import numpy as np
import torch

from tests.common import row_errors, row_rule

U = 2.0 ** -24                                  # float32 unit roundoff
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32w(x):
    """A Python float as the C ABI carries it: rounded to float32, widened back."""
    return float(F32(x))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


# =========================================================== A. scan + compaction ===========================================================
SCAN_EPB, SCAN_SPINE_MAX = 2048, 4096           # egs_common.h EGS_SCAN_EPB, binning.hip EGS_SCAN_SPINE_MAX
SENT_SRC, SENT_KIND, SENT_RANK = -7, 0xEE, -9   # what the plan's output arrays hold before the call
PRUNE_SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 6143)
PRUNE_PATTERNS = ("none", "all", "first", "last", "block_last", "block_density")
LARGE_SIZES = (4096 * 2048, 4096 * 2048 + 1, 4096 * 2048 + 3 * 2048 + 5)
LARGE_PATTERNS = ("all", "last", "block_density")
LATTICE_SIZES = (2049, 4097, 4096 * 2048 + 2049)
DENSITY_PERIOD, DENSITY_STEP, SPREAD = 2039, 37, 1021         # a prime below 2048; a step coprime to it; an odd number (a permutation of a block)


def scan_regime(n):
    """Which kernels egs_launch_scan_u32 launches for n elements, from its branch conditions."""
    if n <= SCAN_EPB:
        return "single"
    return "reduce+apply_sum" if (n + SCAN_EPB - 1) // SCAN_EPB <= SCAN_SPINE_MAX else "recursive"


def block_density(b):
    """Rows kept in (full) block b under 'block_density': 1 + 37 b mod 2039.  Blocks fewer than 2039 apart never have equal sums -- all
    blocks of every size up to 2039 * 2048; beyond that no pattern can do it (2049 possible sums), and equal sums are 2039 blocks apart."""
    return 1 + (b * DENSITY_STEP) % DENSITY_PERIOD


def keep_mask(i, P, pattern):
    """bool keep[i] for the row indices i (a NumPy array or a torch tensor of int64: the large masks are built on the device)."""
    b, j = i // SCAN_EPB, i % SCAN_EPB
    if pattern == "none":
        return i < 0
    if pattern == "all":
        return i >= 0
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == P - 1
    if pattern == "block_last":
        return j == SCAN_EPB - 1
    if pattern == "block_density":
        return (j * SPREAD) % SCAN_EPB < block_density(b)
    raise ValueError(pattern)


def prune_flags(keep):
    """k_mask_flags: (keep_orig, keep_clone, keep_child, is_split) of a prune plan."""
    z = np.zeros(keep.shape[0], bool)
    return np.stack([np.asarray(keep, bool), z, z, z])


def plan_reference(flags):
    """The plan as its definition states it: [kept originals | kept clones | first children | second children], each ascending in the source
    index; split_rank = rank among the split sources, -1 elsewhere; totals = (originals, clones, children, split sources)."""
    o, c, k = (np.flatnonzero(flags[a]) for a in range(3))
    src = np.concatenate([o, c, k, k]).astype(np.int32)
    kind = np.concatenate([np.full(o.size, 0), np.full(c.size, 1), np.full(k.size, 2), np.full(k.size, 3)]).astype(np.uint8)
    s = np.asarray(flags[3], bool)
    rank = np.where(s, np.cumsum(s) - 1, -1).astype(np.int32)
    return dict(totals=(int(o.size), int(c.size), int(k.size), int(s.sum())), src=src, kind=kind, split_rank=rank)


SCAN_FAULTS = ("carry_dropped_level1", "carry_dropped_level2", "spine_scanned_inclusively", "total_before_last_element")
PLAN_FAULTS = SCAN_FAULTS + ("second_children_offset_by_n_split",)


def scan_model(a, fault=None, depth=0):
    """Exclusive scan and total of a, composed the way egs_launch_scan_u32 composes them: blocks of 2048; at most 4096 blocks: every block adds
    up the sums before it; more: the block sums are scanned by the same routine (level 2) and added as carries.  fault: one of SCAN_FAULTS,
    the deliberately wrong variants (the carry of block 1 dropped at level 1 / in the scan of the spine; every carry including its own block;
    the total read one element early)."""
    a = np.asarray(a, np.int64)
    n = a.size
    if n <= SCAN_EPB:
        ex = np.cumsum(a) - a
    else:
        nb = (n + SCAN_EPB - 1) // SCAN_EPB
        blocks = np.zeros(nb * SCAN_EPB, np.int64)
        blocks[:n] = a
        blocks = blocks.reshape(nb, SCAN_EPB)
        sums = blocks.sum(1)
        if nb <= SCAN_SPINE_MAX:
            carry = np.cumsum(sums) - sums
        else:
            carry, _ = scan_model(sums, fault, depth + 1)
        if (fault == "carry_dropped_level1" and depth == 0) or (fault == "carry_dropped_level2" and depth == 1):
            carry = carry.copy(); carry[1] = 0
        if fault == "spine_scanned_inclusively" and depth == 0:
            carry = carry + sums
        ex = (np.cumsum(blocks, 1) - blocks + carry[:, None]).reshape(-1)[:n]
    total = int(ex[n - 1]) + (0 if fault == "total_before_last_element" and depth == 0 else int(a[n - 1]))
    return ex, total


def plan_model(flags, fault=None):
    """k_densify_emit over four scan_model scans, into arrays that hold the sentinels: what the device produces, with the planted fault.
    (A write that a fault sends past the arrays' 3 P rows is dropped.)"""
    P = flags.shape[1]
    offs, tot = zip(*(scan_model(flags[k], fault) for k in range(4)))
    nO, nC, nK, nS = tot
    src, kind = np.full(3 * P, SENT_SRC, np.int32), np.full(3 * P, SENT_KIND, np.uint8)

    def put(pos, rows, code):
        ok = (pos >= 0) & (pos < 3 * P)
        src[pos[ok]] = rows[ok]; kind[pos[ok]] = code
    i = np.flatnonzero(flags[0]); put(offs[0][i], i, 0)
    i = np.flatnonzero(flags[1]); put(nO + offs[1][i], i, 1)
    i = np.flatnonzero(flags[2]); p = nO + nC + offs[2][i]
    put(p, i, 2); put(p + (nS if fault == "second_children_offset_by_n_split" else nK), i, 3)
    rank = np.where(flags[3], offs[3], -1).astype(np.int32)
    return dict(totals=tuple(int(t) for t in tot), src=src, kind=kind, split_rank=rank)


def check_plan(got, want, what=""):
    """Exact: totals; src and kind of the n_new planned rows; split_rank of every source; and src / kind beyond n_new still the sentinels.
    got: totals, src [3P], kind [3P], split_rank [P] (NumPy), the arrays having held SENT_SRC / SENT_KIND before the call."""
    tot = tuple(int(t) for t in got["totals"])
    assert tot == want["totals"], f"{what}: totals {tot}, expected {want['totals']}"
    n = tot[0] + tot[1] + 2 * tot[2]
    for name in ("src", "kind"):
        g, w = np.asarray(got[name]), want[name]
        if not np.array_equal(g[:n], w):
            k = int(np.flatnonzero(g[:n] != w)[0])
            raise AssertionError(f"{what}: {name}[{k}] = {g[k]}, expected {w[k]} ({int((g[:n] != w).sum())} of {n} rows differ)")
        sent = SENT_SRC if name == "src" else SENT_KIND
        assert bool((g[n:] == sent).all()), f"{what}: {name} written beyond n_new = {n} (first at {n + int(np.flatnonzero(g[n:] != sent)[0])})"
    g, w = np.asarray(got["split_rank"]), want["split_rank"]
    if not np.array_equal(g, w):
        k = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"{what}: split_rank[{k}] = {g[k]}, expected {w[k]} ({int((g != w).sum())} differ)")


# ---- the densify plan on a lattice ---------------------------------------------------------------------------------------------------------
# No float evaluation can put a lattice point on the wrong side of a threshold: exp(-6) = 0.0025 < dense_extent = 0.04 < exp(-3) = 0.050 <
# exp(-0.7) / 1.6 = 0.31 < big_extent = 0.4 < exp(-0.7) = 0.50 < 1 / 1.6 = 0.625 < 1; sigmoid(-4) = 0.018 < min_opacity = 0.05 < 0.5; gradient
# means 0, 1e-4 < max_grad = 3e-4 < 1e-3, inf; radii 0, 10 < 20 < 30.
LATTICE_KW = dict(max_grad=3e-4, min_opacity=0.05, extent=4.0, max_screen_size=20.0, percent_dense=0.01)
LATTICE_CURR_GEN, LATTICE_OBJECT = 1, 1


def lattice_combos():
    """Every (clone, split, curr_gen given, prune_prev_gen, which_object given) the entry point accepts: prune_prev_gen off needs curr_gen."""
    return [(c, s, g, p, o) for c in (True, False) for s in (True, False) for g in (True, False) for p in (True, False) for o in (True, False)
            if p or g]


def combo_kw(combo):
    c, s, g, p, o = combo
    return dict(LATTICE_KW, clone=c, split=s, curr_gen=LATTICE_CURR_GEN if g else None, prune_prev_gen=p, which_object=LATTICE_OBJECT if o else None)


def lattice_inputs(P, seed=0):
    rng = np.random.default_rng(1000 + seed + P % 9973)
    pick = lambda vals, size, p=None: np.asarray(vals, F32)[rng.choice(len(vals), size=size, p=p)]
    denom = pick([0.0, 1.0, 2.0, 4.0], P, [0.1, 0.3, 0.3, 0.3])
    mean = pick([0.0, 1e-4, 1e-3], P)
    accum = np.where(denom > 0, mean * denom, pick([0.0, 1e-3], P)).astype(F32)          # a power-of-two denom: the quotient is `mean` again
    return dict(accum=accum, denom=denom, scaling=pick([-6.0, -3.0, -0.7, 0.0], (P, 3), [0.4, 0.3, 0.15, 0.15]), opacity=pick([-4.0, 0.0, 4.0], P),
                max_radii=pick([0.0, 10.0, 30.0], P), generation=rng.integers(0, 3, P).astype(np.int32), is_object=rng.integers(0, 2, P).astype(np.int32))


def thresholds(kw):
    """(dense_extent, big_extent) as the C entry forms them: float32 products of the float32 arguments."""
    return float(F32(kw["percent_dense"]) * F32(kw["extent"])), float(F32(0.1) * F32(kw["extent"]))


RULE_FAULTS = ("clone_grad_strict", "split_grad_strict", "clone_extent_strict", "split_extent_non_strict", "opacity_non_strict",
               "screen_size_non_strict", "big_extent_non_strict", "child_rule_on_parent_scale", "stats_reset_ignored")


def rule_flags(inp, kw, fault=None):
    """The rule table of densify_and_clone / densify_and_split / the final prune (oracle/densify_torch.py) in float64 NumPy on the float32
    inputs -> bool [4, P]: keep_orig, keep_clone, keep_child, is_split.  fault: one of RULE_FAULTS -- one comparison flipped between strict and
    non-strict, the children tested with the parent's scale, or the statistics reset forgotten."""
    d = lambda a: np.asarray(a, np.float64)
    cmp = lambda a, op, b, name: ({">=": a > b, ">": a >= b, "<=": a < b, "<": a <= b} if fault == name else
                                  {">=": a >= b, ">": a > b, "<=": a <= b, "<": a < b})[op]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = d(inp["accum"]) / d(inp["denom"])
    g[np.isnan(g)] = 0.0
    smax = np.exp(d(inp["scaling"])).max(1)
    dense, big = thresholds(kw)
    max_grad, min_opacity, mss = f32w(kw["max_grad"]), f32w(kw["min_opacity"]), f32w(kw["max_screen_size"] or 0.0)
    P = g.shape[0]
    obj = np.ones(P, bool) if kw["which_object"] is None else inp["is_object"] == kw["which_object"]
    C = cmp(np.abs(g), ">=", max_grad, "clone_grad_strict") & cmp(smax, "<=", dense, "clone_extent_strict") & obj & bool(kw["clone"])
    S = cmp(g, ">=", max_grad, "split_grad_strict") & cmp(smax, ">", dense, "split_extent_non_strict") & obj & bool(kw["split"])
    faint = cmp(1.0 / (1.0 + np.exp(-d(inp["opacity"]))), "<", min_opacity, "opacity_non_strict")
    use = mss > 0
    reset = (kw["clone"] or kw["split"]) and fault != "stats_reset_ignored"
    big_vs = cmp(d(inp["max_radii"]), ">", mss, "screen_size_non_strict") & use & (not reset)
    big_ws = cmp(smax, ">", big, "big_extent_non_strict") & use
    big_child = cmp(smax if fault == "child_rule_on_parent_scale" else smax / 1.6, ">", big, "big_extent_non_strict") & use
    gen, cur = inp["generation"], kw["curr_gen"]
    gen_orig = np.ones(P, bool) if kw["prune_prev_gen"] else gen == cur
    gen_clone = np.ones(P, bool) if kw["prune_prev_gen"] else (np.full(P, cur) if cur is not None else gen) == cur
    return np.stack([~S & ~((faint | big_vs | big_ws) & gen_orig), C & ~((faint | big_ws) & gen_clone), S & ~((faint | big_child) & gen_orig), S])


def restatement_state(inp):
    """The inputs as a state of oracle/densify_torch.py that lets the plan be read back from the result: label = the row's index, Adam moments
    1 (new rows get 0), positions 0 and identity rotations (a child lands at exp(scaling) z)."""
    P = inp["accum"].shape[0]
    t = lambda a: torch.tensor(np.ascontiguousarray(a))
    st = dict(xyz=torch.zeros(P, 3), f_dc=t(np.arange(3 * P, dtype=F32).reshape(P, 1, 3) % 251), f_rest=torch.full((P, 1, 3), 0.25),
              opacity=t(inp["opacity"].reshape(P, 1)), scaling=t(inp["scaling"]), rotation=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1),
              label=t(np.arange(P, dtype=F32).reshape(P, 1)))
    for k in list(st):
        st[k + "_exp_avg"] = torch.ones_like(st[k]); st[k + "_exp_avg_sq"] = torch.full_like(st[k], 2.0)
    st.update(generation=t(inp["generation"].reshape(P, 1)), is_object=t(inp["is_object"].reshape(P, 1)),
              xyz_gradient_accum=t(inp["accum"].reshape(P, 1)), denom=t(inp["denom"].reshape(P, 1)), max_radii2D=t(inp["max_radii"]))
    return st


def rank_draws(rows):
    """z for restatement_state: row r of the first children is +(r + 1) on every axis, of the second children -(r + 1)."""
    n = rows // 2
    r = torch.arange(1, n + 1, dtype=torch.float32)
    return torch.cat([r, -r])[:, None].repeat(1, 3)


def decode_plan(st_out, inp):
    """(src, kind, rank of the child rows) read from a densified restatement_state: src from the label; originals are the rows that still carry
    Adam moments; clones kept their source's raw scale, children did not; a first child lies on the + side, a second on the - side, at
    (split rank + 1) scales from its parent."""
    n = lambda a: a.detach().cpu().numpy()
    src = np.rint(n(st_out["label"])[:, 0]).astype(np.int32)
    orig = n(st_out["label_exp_avg"])[:, 0] != 0
    scal, x = n(st_out["scaling"]), n(st_out["xyz"])[:, 0].astype(np.float64)
    same = (bits(scal) == bits(inp["scaling"][src])).all(1)
    kind = np.where(orig, 0, np.where(same, 1, np.where(x > 0, 2, 3))).astype(np.uint8)
    rank = np.rint(np.abs(x) / np.exp(inp["scaling"][src, 0].astype(np.float64))).astype(np.int64) - 1
    return src, kind, np.where(kind >= 2, rank, -1)


def restatement_run(inp, kw):
    """oracle/densify_torch.densify_and_prune on restatement_state(inp) with rank_draws -> the state it leaves."""
    from oracle import densify_torch as D
    return D.densify_and_prune(restatement_state(inp), z=rank_draws, **kw)


def restatement_plan(inp, kw):
    """oracle/densify_torch.densify_and_prune on the inputs -> (src, kind, child ranks, generation, is_object) of the rows it leaves."""
    out = restatement_run(inp, kw)
    src, kind, rank = decode_plan(out, inp)
    return src, kind, rank, out["generation"].numpy()[:, 0], out["is_object"].numpy()[:, 0]


def check_reference_against_restatement(inp, kw, what=""):
    """The NumPy rule table + plan_reference against oracle/densify_torch.py, row for row: source, kind, the children's split rank, and the
    tags a gather with the clone value produces."""
    ref = plan_reference(rule_flags(inp, kw))
    src, kind, rank, gen, obj = restatement_plan(inp, kw)
    assert np.array_equal(src, ref["src"]) and np.array_equal(kind, ref["kind"]), f"{what}: rows differ ({src.size} vs {ref['src'].size})"
    child = kind >= 2
    assert np.array_equal(rank[child], ref["split_rank"][src[child]]), f"{what}: split ranks differ"
    want_gen = inp["generation"][src] if kw["curr_gen"] is None else np.where(kind == 1, kw["curr_gen"], inp["generation"][src])
    assert np.array_equal(gen, want_gen) and np.array_equal(obj, inp["is_object"][src]), f"{what}: tags differ"
    return ref


def gather_inputs(P, D, seed=0):
    """float32 rows with the values a copy must not touch among them: -0, inf, NaN, a denormal."""
    rng = np.random.default_rng(77 + D + seed)
    a = rng.normal(size=(P, D)).astype(F32)
    flat = a.reshape(-1)
    flat[::97] = F32(-0.0); flat[5::389] = F32(np.inf); flat[7::401] = F32(np.nan); flat[11::211] = F32(1e-41)
    return a


def check_gather_f32(out, n_new, D, table, plan, zero_new, sentinel, what=""):
    """out (flat, longer than n_new D, pre-filled with `sentinel`): bit equality with table[src]; zero_new: +0 for every row that is not a
    kept original; nothing beyond n_new D written."""
    want = table[plan["src"]].copy()
    if zero_new:
        want[plan["kind"] != 0] = 0.0
    got = np.asarray(out)
    assert np.array_equal(bits(got[:n_new * D]), bits(want).reshape(-1)), f"{what}: {int((bits(got[:n_new * D]) != bits(want).reshape(-1)).sum())} elements differ"
    assert np.array_equal(bits(got[n_new * D:]), np.full(got.size - n_new * D, bits([sentinel])[0], np.uint32)), f"{what}: written beyond n_new D"


# ========================================================= B. rule edges of k_densify_flags =========================================================
EDGE_P = 257
MAX_GRAD = 2.0 ** -12
EDGE_SCENARIOS = {
    # dense_extent = 1 = exp(0), big_extent = 0.4; screen-size rules off
    "dense_eq": dict(percent_dense=0.25, extent=4.0, max_grad=MAX_GRAD, min_opacity=0.5, max_screen_size=None, clone=True, split=True,
                     curr_gen=None, prune_prev_gen=True, which_object=None),
    # dense_extent = the float32 below 1: exp(0) is the next float up from the threshold
    "dense_below": dict(percent_dense=float(F32(1.0) - F32(2.0 ** -24)), extent=1.0, max_grad=MAX_GRAD, min_opacity=0.5, max_screen_size=None,
                        clone=True, split=True, curr_gen=None, prune_prev_gen=True, which_object=None),
    # big_extent = 1 = exp(0), dense_extent = 2^-7 * 10; no clone or split step: the statistics are live
    "screen_only": dict(percent_dense=2.0 ** -7, extent=10.0, max_grad=MAX_GRAD, min_opacity=0.5, max_screen_size=20.0, clone=False, split=False,
                        curr_gen=None, prune_prev_gen=True, which_object=None),
    "screen_after_clone": dict(percent_dense=2.0 ** -7, extent=10.0, max_grad=MAX_GRAD, min_opacity=0.5, max_screen_size=20.0, clone=True,
                               split=False, curr_gen=None, prune_prev_gen=True, which_object=None),
    "big_split": dict(percent_dense=2.0 ** -7, extent=10.0, max_grad=MAX_GRAD, min_opacity=0.5, max_screen_size=20.0, clone=True, split=True,
                      curr_gen=None, prune_prev_gen=True, which_object=None),
    "generation": dict(percent_dense=0.25, extent=4.0, max_grad=MAX_GRAD, min_opacity=0.5, max_screen_size=None, clone=True, split=True,
                       curr_gen=1, prune_prev_gen=False, which_object=None),
}
HI = 2.0 ** -10                                   # a gradient mean well over max_grad
# name: (row, accum, denom, raw scale on axis 0 (the other axes -3), raw opacity, max_radii, generation)
EDGE_ROWS = {
    "grad_eq_small": (3, 2.0 ** -11, 2.0, -3.0, 3.0, 0.0, 0),
    "grad_below_small": (4, float(np.nextafter(F32(MAX_GRAD), F32(0))), 1.0, -3.0, 3.0, 0.0, 0),
    "grad_eq_large": (255, 2.0 ** -11, 2.0, 1.0, 3.0, 0.0, 0),
    "grad_below_large": (256, float(np.nextafter(F32(MAX_GRAD), F32(0))), 1.0, 1.0, 3.0, 0.0, 0),
    "scale_on_threshold": (17, HI, 1.0, 0.0, 3.0, 0.0, 0),
    "scale_on_threshold_quiet": (18, 0.0, 1.0, 0.0, 3.0, 0.0, 0),
    "opacity_eq": (30, 0.0, 1.0, -3.0, 0.0, 0.0, 0),
    "opacity_below": (31, 0.0, 1.0, -3.0, -3.0, 0.0, 0),
    "radii_eq": (40, 0.0, 1.0, -3.0, 3.0, 20.0, 0),
    "radii_above": (41, 0.0, 1.0, -3.0, 3.0, 30.0, 0),
    "parent_over_children_under": (50, HI, 1.0, float(np.log(1.5)), 3.0, 0.0, 0),
    "children_over": (51, HI, 1.0, float(np.log(4.0)), 3.0, 0.0, 0),
    "split_after_pruned_children": (52, HI, 1.0, float(np.log(1.5)), 3.0, 0.0, 0),
    "zero_over_zero": (60, 0.0, 0.0, -3.0, 3.0, 0.0, 0),
    "x_over_zero_small": (61, 2.0 ** -20, 0.0, -3.0, 3.0, 0.0, 0),
    "x_over_zero_large": (62, 2.0 ** -20, 0.0, 1.0, 3.0, 0.0, 0),
    "negative_mean_small": (70, -HI, 1.0, -3.0, 3.0, 0.0, 0),
    "negative_mean_large": (71, -HI, 1.0, 1.0, 3.0, 0.0, 0),
    "faint_other_generation_cloned": (80, HI, 1.0, -3.0, -3.0, 0.0, 0),
    "faint_current_generation": (81, 0.0, 1.0, -3.0, -3.0, 0.0, 1),
}
# What the reference's rules give each named row, as the kinds that survive ("0" itself, "1" a clone, "23" both children), per scenario
EDGE_EXPECT = {
    "dense_eq": {"grad_eq_small": "01", "grad_below_small": "0", "grad_eq_large": "23", "grad_below_large": "0", "scale_on_threshold": "01",
                 "scale_on_threshold_quiet": "0", "opacity_eq": "0", "opacity_below": "", "zero_over_zero": "0", "x_over_zero_small": "01",
                 "x_over_zero_large": "23", "negative_mean_small": "01", "negative_mean_large": "0", "radii_above": "0"},
    "dense_below": {"scale_on_threshold": "23", "scale_on_threshold_quiet": "0", "grad_eq_small": "01"},
    "screen_only": {"radii_eq": "0", "radii_above": "", "scale_on_threshold": "0", "scale_on_threshold_quiet": "0", "parent_over_children_under": "",
                    "opacity_eq": "0"},
    "screen_after_clone": {"radii_eq": "0", "radii_above": "0", "scale_on_threshold_quiet": "0", "grad_eq_small": "01"},
    "big_split": {"scale_on_threshold_quiet": "0", "parent_over_children_under": "23", "children_over": "", "split_after_pruned_children": "23",
                  "radii_above": "0", "grad_eq_large": ""},
    "generation": {"faint_other_generation_cloned": "0", "faint_current_generation": "", "opacity_below": "0", "grad_eq_small": "01"},
}


def edge_model():
    """257 rows (two 256-thread blocks of k_densify_flags): filler rows well clear of every threshold of every scenario -- half of them
    clone or split, so that a wrong decision shifts every later row of the plan -- and the named rows of EDGE_ROWS.  Asserted here, in
    float32: every equality row is exactly on its threshold, and the thresholds are what both the C entry (float32 product) and the
    restatement (double product, compared against float32 tensors) take them to be."""
    rng = np.random.default_rng(5)
    P = EDGE_P
    pick = lambda vals, size: np.asarray(vals, F32)[rng.integers(0, len(vals), size)]
    inp = dict(accum=pick([0.0, HI], P), denom=np.ones(P, F32), scaling=np.full((P, 3), -3.0, F32), opacity=pick([3.0, 3.0, -3.0], P),
               max_radii=pick([0.0, 30.0], P), generation=rng.integers(0, 3, P).astype(np.int32), is_object=np.zeros(P, np.int32))
    inp["scaling"][:, 0] = pick([-3.0, 1.0], P)
    for name, (row, accum, denom, s0, op, radii, gen) in EDGE_ROWS.items():
        inp["accum"][row], inp["denom"][row], inp["opacity"][row], inp["max_radii"][row], inp["generation"][row] = accum, denom, op, radii, gen
        inp["scaling"][row] = (s0, -3.0, -3.0)
        assert float(inp["accum"][row]) == accum, name                      # the row's numbers are float32 numbers
    f = lambda name: EDGE_ROWS[name][0]
    one = F32(1.0)
    assert np.exp(inp["scaling"][f("scale_on_threshold")]).max() == one and F32(1.0) / (F32(1.0) + np.exp(-inp["opacity"][f("opacity_eq")])) == F32(0.5)
    assert inp["accum"][f("grad_eq_small")] / inp["denom"][f("grad_eq_small")] == F32(MAX_GRAD) == inp["accum"][f("grad_eq_large")] / inp["denom"][f("grad_eq_large")]
    below = inp["accum"][f("grad_below_small")] / inp["denom"][f("grad_below_small")]
    assert below < F32(MAX_GRAD) and np.nextafter(below, one) == F32(MAX_GRAD)
    assert inp["max_radii"][f("radii_eq")] == F32(EDGE_SCENARIOS["screen_only"]["max_screen_size"])
    for name, kw in EDGE_SCENARIOS.items():
        dense, big = thresholds(kw)
        assert F32(kw["percent_dense"] * kw["extent"]) == F32(dense) and F32(0.1 * kw["extent"]) == F32(big), name
        for v in ("max_grad", "min_opacity", "percent_dense", "extent"):
            assert f32w(kw[v]) == kw[v], (name, v)                         # exactly representable: no side rounds them differently
    assert thresholds(EDGE_SCENARIOS["dense_eq"])[0] == 1.0 and thresholds(EDGE_SCENARIOS["screen_only"])[1] == 1.0
    assert np.nextafter(F32(thresholds(EDGE_SCENARIOS["dense_below"])[0]), F32(2)) == one
    return inp


def edge_kwargs(name):
    """(percent_dense, the keyword arguments of densify_and_prune) of a scenario."""
    kw = dict(EDGE_SCENARIOS[name])
    return kw.pop("percent_dense"), kw


def outcome_of(src, kind, row):
    return "".join(str(k) for k in sorted(kind[src == row].tolist()))


def check_edge_outcome(src, kind, gen, want, scenario, what=""):
    """A densified edge model (decoded: decode_plan) against the restatement's, row for row, and the named rows against EDGE_EXPECT."""
    w_src, w_kind, _, w_gen, _ = want
    for name, exp in EDGE_EXPECT[scenario].items():
        got = outcome_of(src, kind, EDGE_ROWS[name][0])
        assert got == exp, f"{what} {scenario}: row '{name}' survives as '{got}', the reference's rules give '{exp}'"
    assert np.array_equal(src, w_src) and np.array_equal(kind, w_kind) and np.array_equal(gen, w_gen), f"{what} {scenario}: plans differ"


# ============================================================ C. split children ============================================================
SPLIT_ROWS, SPLIT_PARENTS = 5003, 6007
SPLIT_DISP_K, SPLIT_SCALE_K = 32.0, (5.0, 2.0)
SPLIT_FAULTS = ("rotation_transposed", "quaternion_not_normalised", "second_child_reads_first_draw")
SPLIT_SENTINEL = 12345.5


def trained_scale_range():
    """(min, max) of the raw scales of the trained scene the benchmark renders (bench_data/trained_scene.npz): what training produces."""
    s = np.load(os.path.join(ROOT, "bench_data", "trained_scene.npz"))["log_scale"]
    return float(s.min()), float(s.max())


def split_case(seed=0):
    """6007 Gaussians, 5003 of them split: quaternions of norm 10^[-3, 3] (one in ten within 1e-4 of an axis, some exactly on one), raw
    scales uniform over the trained scene's range, positions of magnitude 10^[-3, 3], draws out to +-5 with exact zeros (single entries
    and whole rows).  The new model: the 1004 unsplit rows (kind 0), the first children, the second children."""
    rng = np.random.default_rng(31 + seed)
    P, n = SPLIT_PARENTS, SPLIT_ROWS
    lo, hi = trained_scale_range()
    q = rng.normal(size=(P, 4))
    axis = rng.random(P) < 0.1
    q[axis] = 1e-4 * rng.normal(size=(int(axis.sum()), 4))
    q[axis, rng.integers(0, 4, int(axis.sum()))] = rng.choice([-1.0, 1.0], int(axis.sum()))
    q[::601] = np.eye(4)[rng.integers(0, 4, q[::601].shape[0])]
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, (P, 1))
    z = np.clip(rng.normal(size=(2 * n, 3)) * 1.5, -5.0, 5.0)
    z[rng.random((2 * n, 3)) < 0.05] = 0.0
    z[rng.random(2 * n) < 0.02] = 0.0
    z[::331] = rng.choice([-5.0, 5.0], z[::331].shape)
    split = np.zeros(P, bool); split[np.sort(rng.choice(P, n, replace=False))] = True
    s = np.flatnonzero(split)
    rest = np.flatnonzero(~split)
    case = dict(xyz=(rng.choice([-1.0, 1.0], (P, 3)) * 10.0 ** rng.uniform(-3, 3, (P, 3))).astype(F32), scaling=rng.uniform(lo, hi, (P, 3)).astype(F32),
                rotation=q.astype(F32), z=z.astype(F32), n_split=n, src=np.concatenate([rest, s, s]).astype(np.int32),
                kind=np.concatenate([np.zeros(rest.size), np.full(n, 2), np.full(n, 3)]).astype(np.uint8),
                split_rank=np.where(split, np.cumsum(split) - 1, -1).astype(np.int32))
    case["rows"] = case["src"].size
    return case


def split_eval(case, dtype, fault=None):
    """The header formula of k_split_children -- position = parent + R(q / |q|) (exp(raw) z), raw scale = log(exp(raw) / 1.6) -- in `dtype`
    NumPy (float64: the reference; float32, one rounding per operation: the yardstick) for the child rows
    -> (xyz_new, displacement, scaling_new), each [2 n_split, 3].  fault: one of SPLIT_FAULTS."""
    T = lambda a: np.asarray(a, dtype)
    child = case["kind"] >= 2
    s, k = case["src"][child], case["kind"][child].astype(np.int64)
    zrow = (0 if fault == "second_child_reads_first_draw" else (k - 2)) * case["n_split"] + case["split_rank"][s]
    sc = np.exp(T(case["scaling"])[s])
    v = sc * T(case["z"])[zrow]
    q = T(case["rotation"])[s]
    if fault != "quaternion_not_normalised":
        q = q * (dtype(1) / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))[:, None]
    r, x, y, w = q.T
    one, two = dtype(1), dtype(2)
    R = np.stack([one - two * (y * y + w * w), two * (x * y - r * w), two * (x * w + r * y),
                  two * (x * y + r * w), one - two * (x * x + w * w), two * (y * w - r * x),
                  two * (x * w - r * y), two * (y * w + r * x), one - two * (x * x + y * y)], 1).reshape(-1, 3, 3)
    if fault == "rotation_transposed":
        R = R.transpose(0, 2, 1)
    disp = (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]
    xyz = disp + T(case["xyz"])[s]
    return xyz, disp, np.log(sc / dtype(1.6))


def check_split(xyz_new, scaling_new, case, what=""):
    """xyz_new, scaling_new: [rows, 3] float32, pre-filled with SPLIT_SENTINEL, after the kernel (or a float32 evaluation) wrote the child rows.
      * rows of kind 0 are untouched;
      * a child whose draw is exactly zero sits on its parent, bit for bit;
      * every other child's displacement xyz_new - parent (not the sum: a parent at 1e3 must not hide a wrong displacement) and every
        child's scaling_new, against float64, by the project's row rule (tests/common.py row_rule) with the float32 NumPy evaluation as the
        yardstick -- all rows take part;
      * and every element against a worst-case bound, no row excused.  With u = 2^-24, exp and log good to 1 ulp (2u), v = exp(raw) z:
        |q|^-1 carries 4u (four non-negative squares, sqrt, divide), each unit component 5u, a product of two 11u; an off-diagonal entry
        2 (xy -+ rw), |xy| + |rw| <= 1/2, is off by <= 12u, a diagonal entry 1 - 2 (y^2 + w^2) by <= 25u; v by 3u of itself; the three
        products and two sums of a row add 3u sum|v_j|: the displacement is off by <= (25 + 3 + 3)u sum|v_j| < 32u sum|v_j|, and the sum
        with the parent adds u |xyz_new|.  scaling_new = log(exp(raw) / 1.6): the argument carries 2u + u (1.6 as a float) + u, the
        logarithm turns that into an absolute 4u and adds 2u of its own value: <= 5u + 2u |scaling_new|.
    -> figures."""
    x64, d64, s64 = split_eval(case, np.float64)
    x32, _, s32 = split_eval(case, F32)
    child = case["kind"] >= 2
    got_x, got_s = np.asarray(xyz_new, F32), np.asarray(scaling_new, F32)
    sent = bits(np.full((int((~child).sum()), 3), SPLIT_SENTINEL))
    assert np.array_equal(bits(got_x[~child]), sent) and np.array_equal(bits(got_s[~child]), sent), f"{what}: a row of kind 0 was written"
    parent = case["xyz"][case["src"][child]]
    zero = ~np.any(d64 != 0, axis=1)
    assert zero.sum() >= 20 and bool((np.abs(case["z"]).max(1) == 0).sum() >= 20)
    assert np.array_equal(bits(got_x[child][zero]), bits(parent[zero])), f"{what}: a child with a zero draw is not on its parent"
    gx, gs = got_x[child].astype(np.float64), got_s[child].astype(np.float64)
    p64 = parent.astype(np.float64)
    fig, fails = {}, []
    vsum = (np.exp(case["scaling"].astype(np.float64))[case["src"][child]] * np.abs(_draw_rows(case))).sum(1, keepdims=True)
    over = np.abs(gx - x64) - (SPLIT_DISP_K * U * vsum + U * np.abs(x64))
    fig["xyz_bound"] = float((np.abs(gx - x64) / (SPLIT_DISP_K * U * vsum + U * np.abs(x64) + 1e-300)).max())
    if (over > 0).any():
        fails.append(f"xyz_new: {int((over > 0).sum())} elements over 32u sum|v| + u|xyz| (worst {fig['xyz_bound']:.2f} of the bound, child row {int(np.argmax(over.max(1)))})")
    bar = SPLIT_SCALE_K[0] * U + SPLIT_SCALE_K[1] * U * np.abs(s64)
    fig["scaling_bound"] = float((np.abs(gs - s64) / bar).max())
    if (np.abs(gs - s64) > bar).any():
        fails.append(f"scaling_new: {int((np.abs(gs - s64) > bar).sum())} elements over 5u + 2u|value| (worst {fig['scaling_bound']:.2f} of the bound)")
    for name, sub, yard, ref, rows in (("displacement", gx - p64, x32.astype(np.float64) - p64, d64, np.flatnonzero(~zero)),
                                       ("scaling", gs, s32.astype(np.float64), s64, np.arange(s64.shape[0]))):
        e_s, e_y = row_errors(sub, ref, rows), row_errors(yard, ref, rows)
        q_s, q_o, c_s, c_o, bad = row_rule(e_s, [e_y])
        fig[name] = dict(rows=int(rows.size), q50=(float(q_s[0]), float(q_o[0])), q90=(float(q_s[1]), float(q_o[1])), tails=(tuple(c_s), tuple(c_o)),
                         max=(float(e_s.max()), float(e_y.max())))
        if bad:
            fails.append(f"{name}: " + "; ".join(bad))
    assert not fails, f"{what}: " + " | ".join(fails)
    return fig


def _draw_rows(case):
    child = case["kind"] >= 2
    s, k = case["src"][child], case["kind"][child].astype(np.int64)
    return case["z"].astype(np.float64)[(k - 2) * case["n_split"] + case["split_rank"][s]]


def split_outputs(case, dtype=F32, fault=None):
    """(xyz_new, scaling_new) [rows, 3] as the kernel leaves them, from split_eval: sentinels in the rows of kind 0."""
    x, _, s = split_eval(case, dtype, fault)
    child = case["kind"] >= 2
    out_x, out_s = (np.full((case["rows"], 3), SPLIT_SENTINEL, F32) for _ in range(2))
    out_x[child], out_s[child] = x.astype(F32), s.astype(F32)
    return out_x, out_s


# ================================================================ D. 3-NN ================================================================
KNN_SMALL_N = (1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 3966, 3967, 3968, 4100)     # the grid's scan has N/2 + 65 elements: 2048 at 3966, 2049 at 3968
KNN_ROW_N = 20000
KNN_ROW_BOUND = (1.0 + U) ** 8 - 1.0
KNN_CANDIDATES = 12


def knn_cloud(layout, N, seed=0):
    rng = np.random.default_rng(900 + seed + N)
    if layout == "normal":
        pts = rng.normal(size=(N, 3))
    elif layout == "clusters":                                      # five dense blobs far apart, as the grid test's layout of that name
        pts = rng.normal(size=(N, 3)) * 0.01 + rng.integers(0, 5, size=(N, 1)) * 10.0
    elif layout == "identical":
        pts = np.tile(np.array([[0.375, -2.5, 7.0]]), (N, 1))
    else:
        raise ValueError(layout)
    pts = pts.astype(F32)
    if layout != "identical" and N >= 1000:
        pts[[N // 7, N // 5, N // 3, N // 2, N - 1]] = pts[11]      # five coincident points: their answer is exactly zero
    return pts


def knn_reference(pts):
    """float64 on the float32 points, through an exact k-d tree -> (mean of the three smallest squared distances [N], the indices of the
    KNN_CANDIDATES nearest points of every point, itself among them).  Asserted: the last candidate is clearly farther than the third
    neighbour, so no float32 evaluation can prefer a point outside the candidates."""
    from scipy.spatial import cKDTree
    p = pts.astype(np.float64)
    d, idx = cKDTree(p).query(p, k=KNN_CANDIDATES + 1)
    assert bool((d[:, -1] > d[:, 3] * (1.0 + 1e-4)).all())
    d2 = ((p[:, None, :] - p[idx[:, :4]]) ** 2).sum(2)             # the squares summed directly (the tree's distances went through a sqrt)
    d2 = np.sort(d2, 1)
    assert bool((d2[:, 0] == 0).all())                              # the point itself (or a coincident one: the same number)
    return d2[:, 1:4].mean(1), idx


def knn_float32(pts, idx):
    """The kernel's expression in float32 NumPy over each point's candidates: float32 differences, fma(dz, dz, fma(dy, dy, dx dx)), the point
    itself left out by index, the three smallest, (b0 + b1 + b2) / 3."""
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)   # exact product, one rounding
    q = pts[:, None, :]
    d = pts[idx] - q
    dd = fma(d[..., 2], d[..., 2], fma(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
    dd = np.where(idx == np.arange(pts.shape[0])[:, None], F32(np.inf), dd)
    b = np.sort(dd, 1)[:, :3]
    return ((b[:, 0] + b[:, 1]) + b[:, 2]) / F32(3.0)


def check_knn_rows(got, want, what=""):
    """Every row relative to ITS OWN float64 answer: |got - want| <= ((1 + u)^8 - 1) want; rows whose answer is exactly 0 exactly 0.
    The count, u = 2^-24: each difference is one rounding of the exact difference of two float32 numbers (1 + e); dx dx is rounded once
    more: (1 + e)^3 on dx^2; the inner fma adds dy^2 (1 + e)^2 and rounds: (1 + e)^4 / (1 + e)^3; the outer fma adds dz^2 (1 + e)^2 and
    rounds: (1 + e)^5 / (1 + e)^4 / (1 + e)^3 on the three squares.  All terms are non-negative, so the computed distance is within
    (1 + u)^5 of the exact one, and so is each of the three smallest (an order statistic moves no further than the values do).
    b0 + b1, + b2, / 3.0f are three more roundings of non-negative numbers: (1 + u)^8 in all."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    assert zero.sum() >= 5 and bool((got[zero] == 0).all()), f"{what}: a row whose float64 answer is 0 is not 0"
    rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
    assert rel.max() <= KNN_ROW_BOUND, f"{what}: {int((rel > KNN_ROW_BOUND).sum())} rows over {KNN_ROW_BOUND / U:.2f}u of their own value (worst {rel.max() / U:.2f}u)"
    return float(rel.max() / U)
