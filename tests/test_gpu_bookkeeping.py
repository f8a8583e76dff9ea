"""GPU: the model-bookkeeping kernels against the references and checks of tests/bookkeeping_cases.py (tests/test_bookkeeping_cpu.py shows
that those inputs see the faults they are meant to see).
  A  the prune / densify plan = flags + four scans + compaction, at every regime and block edge of the shared u32 scan -- the recursive
     regime (more than 4096 * 2048 elements) included --, and the gathers that read the plan: exact;
  B  every selection rule of k_densify_flags with a row ON its threshold, through densify.densify_and_prune and through the in-place
     route of a capacity-sized model, against oracle/densify_torch.py: exact;
  C  k_split_children against its header formula in float64;
  D  the grid 3-NN search against the all-pairs kernel from 1 point up (same bits), and the all-pairs kernel row by row against float64."""
import functools

import numpy as np
import pytest
import torch

from tests import bookkeeping_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fresh_plan(P):
    """A _Plan whose output arrays hold the sentinels of tests/bookkeeping_cases.py."""
    from egogaussian_amd.densify import _Plan
    plan = _Plan(P, torch.device(DEV))
    plan.src.fill_(B.SENT_SRC); plan.kind.fill_(B.SENT_KIND); plan.split_rank.fill_(B.SENT_RANK)
    return plan


def _read(plan):
    torch.cuda.synchronize()
    return dict(totals=plan.totals.tolist(), src=plan.src.cpu().numpy(), kind=plan.kind.cpu().numpy(), split_rank=plan.split_rank.cpu().numpy())


def _prune_plan(keep):
    """egs_prune_plan for a bool keep tensor on the device -> the plan's arrays (NumPy)."""
    from egogaussian_amd import densify, lib
    L, P = lib.load(), keep.shape[0]
    plan = _fresh_plan(P)
    m = (~keep).contiguous().view(torch.uint8)
    p = densify._p
    with torch.cuda.device(DEV):
        lib.check(L.egs_prune_plan(P, p(m), p(plan.scratch), p(plan.src), p(plan.kind), p(plan.split_rank), p(plan.totals), densify._stream()))
    return _read(plan)


def _densify_plan(inp, kw, keep_plan=False):
    """egs_densify_plan on the lattice inputs -> the plan's arrays (NumPy) [, the _Plan itself, finished]."""
    from egogaussian_amd import densify, lib
    L, P = lib.load(), inp["accum"].shape[0]
    plan = _fresh_plan(P)
    t = {k: _dev(v) for k, v in inp.items()}
    p = densify._p
    with torch.cuda.device(DEV):
        lib.check(L.egs_densify_plan(
            P, p(t["accum"]), p(t["denom"]), p(t["scaling"]), p(t["opacity"]), p(t["max_radii"]), p(t["generation"]), p(t["is_object"]),
            float(kw["max_grad"]), float(kw["min_opacity"]), float(kw["percent_dense"]), float(kw["extent"]), float(kw["max_screen_size"] or 0.0),
            int(kw["clone"]), int(kw["split"]), int(kw["curr_gen"] is not None), int(kw["curr_gen"] or 0), int(kw["prune_prev_gen"]),
            int(kw["which_object"] is not None), int(kw["which_object"] or 0), p(plan.scratch), p(plan.src), p(plan.kind), p(plan.split_rank),
            p(plan.totals), densify._stream()))
    got = _read(plan)
    return (got, plan.finish()) if keep_plan else got


# ---- A. plan = scan + compaction --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", B.PRUNE_SIZES)
def test_prune_plan_at_every_block_and_regime_edge(P):
    """egs_prune_plan against np.flatnonzero: totals, src, kind, split_rank (-1 everywhere), and src / kind untouched beyond n_new.
    Scan kernels by P: <= 2048 k_scan_single; 2049 .. 6143 k_scan_reduce + k_scan_apply_sum (2 and 3 blocks)."""
    i = np.arange(P, dtype=np.int64)
    for pat in B.PRUNE_PATTERNS:
        keep = B.keep_mask(i, P, pat)
        got = _prune_plan(_dev(keep))
        assert (got["split_rank"] == -1).all()
        B.check_plan(got, B.plan_reference(B.prune_flags(keep)), f"P={P} {pat} ({B.scan_regime(P)})")


@pytest.mark.parametrize("P", B.LARGE_SIZES)
def test_prune_plan_around_the_recursive_threshold(P):
    """4096 * 2048 rows: the last size of k_scan_reduce + k_scan_apply_sum; one more: the first recursive size (k_scan_reduce, the spine of
    4097 sums scanned in place by k_scan_reduce + k_scan_apply_sum over 3 blocks with its scratch behind the spine, k_scan_apply); and a size
    with a spine of 4100.  The mask is built on the device, the reference by NumPy on the host."""
    assert B.scan_regime(P) == ("recursive" if P > 4096 * 2048 else "reduce+apply_sum")
    i_host, i_dev = np.arange(P, dtype=np.int64), torch.arange(P, dtype=torch.int64, device=DEV)
    for pat in B.LARGE_PATTERNS:
        got = _prune_plan(B.keep_mask(i_dev, P, pat))
        B.check_plan(got, B.plan_reference(B.prune_flags(B.keep_mask(i_host, P, pat))), f"P={P} {pat}")


@functools.lru_cache(maxsize=None)
def _lattice(P):
    return B.lattice_inputs(P)


@pytest.mark.parametrize("P", B.LATTICE_SIZES)
def test_densify_plan_on_the_lattice(P):
    """egs_densify_plan -- four scans on different data -- against the rule table written out in float64 NumPy (pinned to
    oracle/densify_torch.py by tests/test_bookkeeping_cpu.py): all four totals, [kept originals | kept clones | first children | second
    children] each ascending in the source, the kind codes, split_rank.  P = 4096 * 2048 + 2049 takes the recursive scan."""
    inp, kw = _lattice(P), B.combo_kw((True, True, True, True, False))
    want = B.plan_reference(B.rule_flags(inp, kw))
    assert min(want["totals"]) > 0 and want["totals"][2] < want["totals"][3]
    B.check_plan(_densify_plan(inp, kw), want, f"P={P} ({B.scan_regime(P)})")


@pytest.mark.parametrize("combo", B.lattice_combos(), ids=lambda c: "".join("ny"[int(v)] for v in c))
def test_densify_plan_every_switch(combo):
    """clone / split on and off, curr_gen given or not, prune_prev_gen on and off, which_object given or not, at P = 4097."""
    inp, kw = _lattice(4097), B.combo_kw(combo)
    B.check_plan(_densify_plan(inp, kw), B.plan_reference(B.rule_flags(inp, kw)), str(combo))


@functools.lru_cache(maxsize=None)
def _plan_4097():
    inp, kw = _lattice(4097), B.combo_kw((True, True, True, True, False))
    got, plan = _densify_plan(inp, kw, keep_plan=True)
    want = B.plan_reference(B.rule_flags(inp, kw))
    B.check_plan(got, want, "P=4097")
    return inp, plan, want


@pytest.mark.parametrize("D", [1, 3, 4, 45])
def test_gather_rows_are_bit_copies(D):
    """egs_gather_rows_f32 over the P = 4097 plan: the bits of table[src] (-0, inf, NaN and denormals among them); zero_new: exactly +0 in
    every row that is not a kept original; nothing written beyond n_new D."""
    from egogaussian_amd import densify, lib
    L = lib.load()
    _, plan, want = _plan_4097()
    n, table, p = plan.n_new, B.gather_inputs(4097, D), densify._p
    t = _dev(table)
    for zero_new in (0, 1):
        out = torch.full((n * D + 257,), 3.25, device=DEV)
        with torch.cuda.device(DEV):
            lib.check(L.egs_gather_rows_f32(n, D, p(plan.src), p(plan.kind), zero_new, p(t), p(out), densify._stream()))
        B.check_gather_f32(out.cpu().numpy(), n, D, table, want, bool(zero_new), 3.25, f"D={D} zero_new={zero_new}")


@pytest.mark.parametrize("clone_value", [None, 5])
def test_gather_i32_with_and_without_the_clone_value(clone_value):
    from egogaussian_amd import densify, lib
    L = lib.load()
    inp, plan, want = _plan_4097()
    n, p = plan.n_new, densify._p
    out, gen = torch.full((n + 257,), -77, dtype=torch.int32, device=DEV), _dev(inp["generation"])
    with torch.cuda.device(DEV):
        lib.check(L.egs_gather_i32(n, p(plan.src), p(plan.kind), int(clone_value is not None), clone_value or 0, p(gen), p(out), densify._stream()))
    got = out.cpu().numpy()
    ref = inp["generation"][want["src"]]
    if clone_value is not None:
        ref = np.where(want["kind"] == 1, clone_value, ref)
    assert (want["kind"] == 1).any() and np.array_equal(got[:n], ref) and (got[n:] == -77).all()


# ---- B. rule edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", sorted(B.EDGE_SCENARIOS))
def test_rule_edges_against_the_restatement(scenario):
    """The hand-built 257-row model (tests/bookkeeping_cases.py edge_model: a row exactly ON every threshold, one float off it, 0/0 and x/0,
    children on the other side of big_extent than their parent, a clone of another generation) through densify.densify_and_prune: the same
    rows survive, as the same kinds, in the same order as oracle/densify_torch.py leaves them; every array equal (positions and scales of
    the child rows, which section C holds, aside); and the in-place route of a capacity-sized model leaves the same live prefix."""
    from egogaussian_amd import densify
    from tests.test_gpu_densify import Model
    from tests.test_gpu_capacity import CapModel
    inp = B.edge_model()
    pd, kw = B.edge_kwargs(scenario)
    full = dict(kw, percent_dense=pd)
    want_state = B.restatement_run(inp, full)
    want = B.restatement_plan(inp, full)
    m = Model(B.restatement_state(inp), pd)
    n0, n1 = densify.densify_and_prune(m, z=B.rank_draws, **kw)
    got = m.state()
    assert n0 == B.EDGE_P and n1 == want[0].size == got["xyz"].shape[0]
    src, kind, _ = B.decode_plan(got, inp)
    B.check_edge_outcome(src, kind, got["generation"].numpy()[:, 0], want, scenario, "kernel")
    child = torch.from_numpy(kind >= 2)
    for k, v in want_state.items():
        a, b = got[k], v.to(got[k].dtype)
        if k in ("xyz", "scaling"):
            a, b = a[~child], b[~child]
        assert torch.equal(a, b), f"{scenario}: {k}"
    cm = CapModel(B.restatement_state(inp), 1024, pd)
    assert densify.densify_and_prune(cm, z=B.rank_draws, **kw) == (n0, n1) and cm.n_active == n1
    live = cm.live_state()
    for k, v in got.items():
        assert torch.equal(live[k], v), f"{scenario}: in place, {k}"


# ---- C. split children ----------------------------------------------------------------------------------------------------------------------
def test_split_children_against_float64():
    """egs_split_children on 5003 split Gaussians (quaternion norms 10^[-3, 3], near and on the axes, raw scales over the trained scene's
    range, parents at 10^[-3, 3], draws out to +-5 with exact zeros): check_split -- rows of kind 0 untouched, zero draws on the parent bit
    for bit, the displacement and the new raw scale against float64 by the row rule with the float32 NumPy form as the yardstick, and every
    element inside the derived worst-case bound."""
    from egogaussian_amd import densify, lib
    L = lib.load()
    c = B.split_case()
    p = densify._p
    x = torch.full((c["rows"], 3), B.SPLIT_SENTINEL, device=DEV)
    s = torch.full((c["rows"], 3), B.SPLIT_SENTINEL, device=DEV)
    t = {k: _dev(c[k]) for k in ("src", "kind", "split_rank", "z", "xyz", "scaling", "rotation")}
    with torch.cuda.device(DEV):
        lib.check(L.egs_split_children(c["rows"], p(t["src"]), p(t["kind"]), p(t["split_rank"]), c["n_split"], p(t["z"]), p(t["xyz"]), p(t["scaling"]),
                                       p(t["rotation"]), p(x), p(s), densify._stream()))
    fig = B.check_split(x.cpu().numpy(), s.cpu().numpy(), c, "k_split_children")
    print(f"\n  k_split_children: {fig}")


# ---- D. 3-NN --------------------------------------------------------------------------------------------------------------------------------
def test_knn_grid_equals_all_pairs_from_one_point_up():
    """method='grid' against method='pairs', same bits, on a normal cloud of N = 1 .. 4100 points: the grid's scan has N / 2 + 65 elements
    (k_scan_single up to N = 3967, two blocks from 3968), k_knn_grid_setup reduces 1 .. 17 partials."""
    from simple_knn._C import distCUDA2
    for N in B.KNN_SMALL_N:
        t = _dev(B.knn_cloud("normal", N))
        a, b = distCUDA2(t, method="pairs"), distCUDA2(t, method="grid")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"N={N}: {int((a != b).sum())} rows differ"
        assert bool(torch.isinf(a).all() and (a > 0).all()) if N < 4 else bool(torch.isfinite(a).all()), f"N={N}"


@pytest.mark.parametrize("N", B.KNN_SMALL_N)
def test_knn_of_identical_points(N):
    """N copies of one point (zero extent on every axis, all points in one cell): grid and all-pairs agree bit for bit; the answer is
    exactly 0 from 4 points up and +inf below.  (N = 3 is the case that found a defect: a point with two neighbours kept one FLT_MAX slot,
    (0 + 0) + FLT_MAX does not overflow, and both kernels returned the finite FLT_MAX / 3 = 1.134e38; knn.hip now tests the empty slot.)"""
    from simple_knn._C import distCUDA2
    t = _dev(B.knn_cloud("identical", N))
    a, b = distCUDA2(t, method="pairs"), distCUDA2(t, method="grid")
    print(f"\n  N={N}: pairs {a[:1].tolist()}, grid {b[:1].tolist()}")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"N={N}: grid and all-pairs differ"
    want = 0.0 if N >= 4 else float("inf")
    assert bool((a == want).all()) and bool((b == want).all()), f"N={N}: expected {want}, all-pairs gives {a[:3].tolist()}, grid {b[:3].tolist()}"


@functools.lru_cache(maxsize=None)
def _knn_reference(layout):
    pts = B.knn_cloud(layout, B.KNN_ROW_N)
    return pts, B.knn_reference(pts)[0]


@pytest.mark.parametrize("layout", ["clusters", "normal"])
def test_knn_all_pairs_row_by_row_against_float64(layout):
    """Every row of method='pairs' at N = 20 000 within (1 + u)^8 - 1 of ITS OWN float64 answer (check_knn_rows derives the count), rows whose
    answer is 0 exactly 0 -- on five dense blobs far apart, whose rows a bar relative to the array's maximum does not see, and on a normal
    cloud."""
    from simple_knn._C import distCUDA2
    pts, want = _knn_reference(layout)
    got = distCUDA2(_dev(pts), method="pairs").cpu().numpy()
    worst = B.check_knn_rows(got, want, layout)
    print(f"\n  {layout}: worst row {worst:.2f}u of its own value (bound {B.KNN_ROW_BOUND / B.U:.2f}u)")
