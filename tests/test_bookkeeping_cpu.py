"""CPU: the bookkeeping harness itself (tests/bookkeeping_cases.py) -- every check is handed its reference's own output, which must pass,
and the deliberately wrong variants, each of which at least one case of the matrix the GPU tests run has to catch (the case is printed).
The lattice reference is pinned to oracle/densify_torch.py, the float32 yardsticks are held to the bars.  Runs no GPU code."""
import functools

import numpy as np
import pytest

from tests import bookkeeping_cases as B


def _caught(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ---- A. scan + compaction --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice(P, combo=None):
    inp = B.lattice_inputs(P)
    kw = B.combo_kw(combo or (True, True, True, True, False))
    return inp, kw, B.rule_flags(inp, kw)


def _matrix():
    """(name, flags) of every plan the GPU tests of section A run, smallest first (the generator stops where a fault is caught)."""
    for P in B.PRUNE_SIZES:
        for pat in B.PRUNE_PATTERNS:
            yield f"prune P={P} {pat}", lambda P=P, pat=pat: B.prune_flags(B.keep_mask(np.arange(P, dtype=np.int64), P, pat))
    for P in B.LATTICE_SIZES[:2]:
        yield f"densify lattice P={P}", lambda P=P: _lattice(P)[2]
    for P in B.LARGE_SIZES:
        for pat in B.LARGE_PATTERNS:
            yield f"prune P={P} {pat}", lambda P=P, pat=pat: B.prune_flags(B.keep_mask(np.arange(P, dtype=np.int64), P, pat))
    yield f"densify lattice P={B.LATTICE_SIZES[2]}", lambda: _lattice(B.LATTICE_SIZES[2])[2]


def test_every_scan_regime_is_in_the_matrix():
    regimes = {P: B.scan_regime(P) for P in B.PRUNE_SIZES + B.LARGE_SIZES + B.LATTICE_SIZES}
    print(regimes)
    assert set(regimes.values()) == {"single", "reduce+apply_sum", "recursive"}
    assert regimes[2048] == "single" and regimes[2049] == "reduce+apply_sum" and regimes[4096 * 2048] == "reduce+apply_sum"
    assert regimes[4096 * 2048 + 1] == "recursive" and regimes[B.LATTICE_SIZES[2]] == "recursive"
    # the first recursive size: a spine of 4097 entries, whose own scan has 3 blocks
    assert (4096 * 2048 + 1 + 2047) // 2048 == 4097 and (4097 + 2047) // 2048 == 3
    # 'block_density': no two of the first 2039 blocks have equal sums, and the level-2 blocks' sums differ as well
    d = B.block_density(np.arange(4100))
    assert len(set(d[:2039].tolist())) == 2039 and d.min() >= 1 and d.max() <= 2047
    assert d[:2048].sum() != d[2048:4096].sum()
    keep = B.keep_mask(np.arange(6143, dtype=np.int64), 6143, "block_density")
    assert [int(keep[b * 2048:(b + 1) * 2048].sum()) for b in range(2)] == d[:2].tolist()


@pytest.mark.parametrize("P", B.PRUNE_SIZES)
def test_prune_plan_model_equals_flatnonzero(P):
    for pat in B.PRUNE_PATTERNS:
        keep = B.keep_mask(np.arange(P, dtype=np.int64), P, pat)
        want = B.plan_reference(B.prune_flags(keep))
        assert np.array_equal(want["src"], np.flatnonzero(keep)) and not want["kind"].any() and (want["split_rank"] == -1).all()
        B.check_plan(B.plan_model(B.prune_flags(keep)), want, f"P={P} {pat}")


@pytest.mark.parametrize("fault", B.PLAN_FAULTS)
def test_plan_check_catches_a_wrong_scan(fault):
    """Each fault of the three-level scan model (and of the emit step) changes the plan of at least one case of the matrix."""
    for name, flags in _matrix():
        f = flags()
        if _caught(B.check_plan, B.plan_model(f, fault), B.plan_reference(f), name):
            print(f"{fault}: caught by '{name}' ({B.scan_regime(f.shape[1])})")
            if fault == "carry_dropped_level2":
                assert B.scan_regime(f.shape[1]) == "recursive"
            return
    raise AssertionError(f"{fault}: no case of the matrix sees it")


def test_large_plans_pass_the_unplanted_model():
    """The recursive composition itself (no fault) against flatnonzero, at the first recursive size."""
    P = B.LARGE_SIZES[1]
    f = B.prune_flags(B.keep_mask(np.arange(P, dtype=np.int64), P, "block_density"))
    B.check_plan(B.plan_model(f), B.plan_reference(f), f"P={P}")


def test_second_child_fault_needs_pruned_children():
    """n_child != n_split on the lattice: the planted offset fault is visible there."""
    _, _, flags = _lattice(2049)
    assert 0 < flags[2].sum() < flags[3].sum() and flags[1].sum() > 0


@pytest.mark.parametrize("combo", B.lattice_combos())
def test_lattice_reference_is_the_restatement(combo):
    """The NumPy rule table + plan at P = 4097 against oracle/densify_torch.py (what the reference-captured fixtures pin), for every
    combination of clone / split / curr_gen / prune_prev_gen / which_object."""
    inp, kw, flags = _lattice(4097, combo)
    ref = B.check_reference_against_restatement(inp, kw, str(combo))
    B.check_plan(B.plan_model(flags), ref, str(combo))
    if combo == (True, True, True, True, False):
        assert min(ref["totals"]) > 20 and ref["totals"][2] < ref["totals"][3]          # every kind present, some children pruned


@pytest.mark.parametrize("D", [1, 3, 4, 45])
def test_gather_check_against_its_own_reference(D):
    _, _, flags = _lattice(4097)
    plan = B.plan_reference(flags)
    table = B.gather_inputs(4097, D)
    n = plan["src"].size
    for zero_new in (False, True):
        out = np.full(n * D + 100, 3.25, np.float32)
        out[:n * D] = np.where((plan["kind"] != 0)[:, None] & zero_new, np.float32(0), table[plan["src"]]).reshape(-1)
        B.check_gather_f32(out, n, D, table, plan, zero_new, 3.25)
        bad = out.copy(); bad[n * D] = 0.0
        assert _caught(B.check_gather_f32, bad, n, D, table, plan, zero_new, 3.25)
    neg = out.copy(); neg[np.flatnonzero(np.repeat(plan["kind"] != 0, D))[0]] = -0.0          # -0 where +0 is required
    assert _caught(B.check_gather_f32, neg, n, D, table, plan, True, 3.25)


# ---- B. rule edges ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge(scenario):
    inp = B.edge_model()
    pd, kw = B.edge_kwargs(scenario)
    return inp, dict(kw, percent_dense=pd), B.restatement_plan(inp, dict(kw, percent_dense=pd))


@pytest.mark.parametrize("scenario", sorted(B.EDGE_SCENARIOS))
def test_edge_rows_do_what_the_reference_rules_say(scenario):
    """The restatement on the hand-built model: every named row survives as EDGE_EXPECT states, and the NumPy rule table agrees with the
    restatement on every row."""
    inp, kw, want = _edge(scenario)
    B.check_edge_outcome(want[0], want[1], want[3], want, scenario, "restatement")
    ref = B.plan_reference(B.rule_flags(inp, kw))
    assert np.array_equal(ref["src"], want[0]) and np.array_equal(ref["kind"], want[1])
    assert len(set(want[1].tolist())) >= (1 if not (kw["clone"] or kw["split"]) else 2)


@pytest.mark.parametrize("fault", B.RULE_FAULTS)
def test_edge_model_catches_a_wrong_rule(fault):
    """One comparison flipped, the child rule on the parent's scale, the statistics reset ignored: each changes what survives of at least
    one named row, in at least one scenario."""
    hits = []
    for scenario in sorted(B.EDGE_SCENARIOS):
        inp, kw, want = _edge(scenario)
        bad = B.plan_reference(B.rule_flags(inp, kw, fault))
        rows = [n for n, e in B.EDGE_EXPECT[scenario].items() if B.outcome_of(bad["src"], bad["kind"], B.EDGE_ROWS[n][0]) != e]
        if rows:
            assert _caught(B.check_edge_outcome, bad["src"], bad["kind"], want[3], want, scenario)
            hits.append((scenario, rows))
    print(f"{fault}: caught by {hits}")
    assert hits, f"{fault}: no named row changes"


# ---- C. split children -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _split():
    return B.split_case()


def test_split_inputs_are_what_they_claim():
    c = _split()
    lo, hi = B.trained_scale_range()
    n = np.linalg.norm(c["rotation"].astype(np.float64), axis=1)
    assert n.min() < 3e-3 and n.max() > 3e2 and c["scaling"].min() < lo + 0.1 and c["scaling"].max() > hi - 0.1
    assert np.abs(c["z"]).max() == 5.0 and (c["z"] == 0).mean() > 0.03
    a = np.abs(c["xyz"])
    assert a.min() < 2e-3 and a.max() > 5e2
    unit = np.abs(c["rotation"].astype(np.float64)) / n[:, None]
    assert ((unit.max(1) > 1 - 1e-6).sum() >= 100) and (unit.max(1) == 1).sum() >= 5          # near an axis, and exactly on one


def test_split_yardstick_sits_within_the_bars():
    c = _split()
    fig = B.check_split(*B.split_outputs(c), c, "float32 NumPy")
    print(fig)
    assert fig["xyz_bound"] <= 1.0 and fig["scaling_bound"] <= 1.0


@pytest.mark.parametrize("fault", B.SPLIT_FAULTS)
def test_split_check_catches_a_wrong_kernel(fault):
    c = _split()
    with pytest.raises(AssertionError) as e:
        B.check_split(*B.split_outputs(c, fault=fault), c, fault)
    print(f"{fault}: {str(e.value)[:300]}")


def test_split_check_catches_written_kind0_rows_and_moved_zero_draws():
    c = _split()
    x, s = B.split_outputs(c)
    bad = x.copy(); bad[0] = 0.0
    assert _caught(B.check_split, bad, s, c)
    child = np.flatnonzero(c["kind"] >= 2)
    zero_rows = child[np.abs(B._draw_rows(c)).max(1) == 0]
    bad = x.copy(); bad[zero_rows[0], 0] = np.nextafter(bad[zero_rows[0], 0], np.float32(np.inf))
    assert _caught(B.check_split, bad, s, c)


# ---- D. 3-NN -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _knn(layout):
    pts = B.knn_cloud(layout, B.KNN_ROW_N)
    want, idx = B.knn_reference(pts)
    return pts, want, idx


@pytest.mark.parametrize("layout", ["clusters", "normal"])
def test_knn_float32_evaluation_stays_inside_the_derived_bound(layout):
    pts, want, idx = _knn(layout)
    assert abs(B.KNN_ROW_BOUND / B.U - 8.0) < 1e-5
    worst = B.check_knn_rows(B.knn_float32(pts, idx), want, layout)
    print(f"{layout}: float32 NumPy worst row {worst:.2f}u (bound {B.KNN_ROW_BOUND / B.U:.2f}u); rows span {want[want > 0].min():.2e} .. {want.max():.2e}")
    # what a max-norm bar of 1e-5 max(want) allows the densest row, relative to its own value: far more than this bound
    loose = 1e-5 * want.max() / want[want > 0].min()
    print(f"  a bar of 1e-5 max allows the densest row {loose:.1e} of itself, this bound {B.KNN_ROW_BOUND:.1e}")
    assert loose > 100.0 * B.KNN_ROW_BOUND
    off = B.knn_float32(pts, idx) * np.float32(1.0 + 2e-6)
    assert _caught(B.check_knn_rows, off, want)
