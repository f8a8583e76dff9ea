"""CPU: the device-sized densify / prune route's host-visible parts -- the four new entry points and their argument checks,
densify.apply_statement (the torch statement egs_densify_apply answers to) against oracle/densify_torch.py applied to the live
prefix, and CapacityGaussians.n_active as a property over a cached host int."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import densify_torch as D
from tests import bookkeeping_cases as B
from tests import device_densify_cases as K

NEW_SYMBOLS = ("egs_densify_plan_dev", "egs_prune_plan_dev", "egs_densify_apply_scratch_bytes", "egs_densify_apply")
EGS_ERR_ARG = -1


def test_library_exports_the_new_entry_points():
    """The four symbols exist in the built library and lib.py declares a signature for each."""
    from egogaussian_amd import lib
    raw = C.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in lib.SIGNATURES, name
        assert hasattr(raw, name), f"{name} is not exported by {lib.LIB_PATH}"
    L = lib.load()
    res, args = lib.SIGNATURES["egs_densify_apply"]
    assert res is C.c_int and len(args) == 16 and L.egs_densify_apply.argtypes == args
    assert len(lib.SIGNATURES["egs_densify_plan_dev"][1]) == 17 and len(lib.SIGNATURES["egs_prune_plan_dev"][1]) == 9
    assert C.sizeof(lib.DensifyRuleBlock) == 48 and C.sizeof(lib.DensifyArray) == 24


def test_apply_scratch_is_one_shadow_row_per_row_rewritten():
    """egs_densify_apply_scratch_bytes = capacity * sum(row_floats) * 4: exactly the bytes of the arrays the apply rewrites, nothing more."""
    from egogaussian_amd import lib
    L = lib.load()
    rows = [3, 3, 45, 1, 3, 4, 1] * 3 + [1, 1, 1] + [1, 1]           # config C's table: parameters, two moments each, statistics, tags (SH degree 3)
    arr = (C.c_int32 * len(rows))(*rows)
    assert L.egs_densify_apply_scratch_bytes(500000, len(rows), arr) == 500000 * sum(rows) * 4
    assert L.egs_densify_apply_scratch_bytes(0, len(rows), arr) == 0 and L.egs_densify_apply_scratch_bytes(10, 0, arr) == 0


def test_argument_errors_come_back_before_any_device_work():
    """Every refusal below is decided on the host: this test runs where there is no device at all."""
    from egogaussian_amd import lib
    L = lib.load()
    one = C.c_void_p(0x1000)                                         # never dereferenced: the checks come first
    table = (lib.DensifyArray * 3)(lib.DensifyArray(0x1000, 3, lib.DENSIFY_PARAM, 0, 0), lib.DensifyArray(0x1000, 3, lib.DENSIFY_PARAM, 0, 0),
                                    lib.DensifyArray(0x1000, 4, lib.DENSIFY_PARAM, 0, 0))

    def apply(capacity=8, n=3, tab=table, xyz=0, scaling=1, rotation=2, rules=one, z=one, status=one):
        return L.egs_densify_apply(capacity, one, one, one, one, one, rules, n, tab, xyz, scaling, rotation, z, one, status, None)
    assert apply(capacity=0) == EGS_ERR_ARG and apply(n=0) == EGS_ERR_ARG and apply(n=lib.DENSIFY_MAX_ARRAYS + 1) == EGS_ERR_ARG
    assert apply(status=None) == EGS_ERR_ARG and apply(z=None) == EGS_ERR_ARG          # a densify plan needs its draws
    assert apply(xyz=2) == EGS_ERR_ARG and apply(rotation=1) == EGS_ERR_ARG and apply(scaling=3) == EGS_ERR_ARG
    for bad in (lib.DensifyArray(0, 3, lib.DENSIFY_PARAM, 0, 0), lib.DensifyArray(0x1000, 0, lib.DENSIFY_PARAM, 0, 0),
                lib.DensifyArray(0x1000, 3, 4, 0, 0), lib.DensifyArray(0x1000, 3, lib.DENSIFY_PARAM, lib.DENSIFY_TAG_I32, 0),
                lib.DensifyArray(0x1000, 1, lib.DENSIFY_TAG, lib.DENSIFY_TAG_CLONE_GEN, 0)):
        tab = (lib.DensifyArray * 3)(bad, table[1], table[2])
        assert apply(tab=tab) == EGS_ERR_ARG
    assert L.egs_densify_plan_dev(0, *([one] * 8), 1, *([one] * 6), None) == EGS_ERR_ARG
    assert L.egs_densify_plan_dev(8, *([one] * 8), 1, None, *([one] * 5), None) == EGS_ERR_ARG          # no rule block
    assert L.egs_prune_plan_dev(8, one, None, *([one] * 5), None) == EGS_ERR_ARG


def test_rule_block_words():
    """The block DeviceDensify writes: float32 thresholds formed as egs_densify_plan forms them, the switches as int32 words."""
    from egogaussian_amd import densify
    w = densify._rule_words(0.01, 3e-4, 0.05, 4.0, 20.0, True, False, 3, False, None)
    f = w[:5].view(np.float32)
    dense, big = B.thresholds(dict(percent_dense=0.01, extent=4.0))
    assert w.dtype == np.int32 and w.shape == (12,)
    assert tuple(float(v) for v in f) == (B.f32w(3e-4), B.f32w(0.05), dense, big, 20.0)
    assert tuple(int(v) for v in w[5:]) == (1, 0, 1, 3, 0, 0, 0)
    assert float(densify._rule_words(0.01, 1.0, 0.1, 4.0, None, True, True, None, True, 2)[:5].view(np.float32)[4]) == 0.0
    with pytest.raises(NotImplementedError):
        densify._check_rules(split=True, split_prev_gen=False)
    with pytest.raises(ValueError):
        densify._check_rules(prune_prev_gen=False, curr_gen=None)


def _run_statement(before, plan, n_old, z, curr_gen, stats_reset, status=None):
    from egogaussian_amd import densify
    st = {k: v.clone() for k, v in before.items()}
    count = torch.tensor([n_old], dtype=torch.int32)
    status = torch.zeros(4, dtype=torch.int64) if status is None else status
    ok = densify.apply_statement(st, plan, count, status, z=z, curr_gen=curr_gen, stats_reset=stats_reset)
    return ok, st, int(count[0]), [int(v) for v in status]


def _densify_case(inp, kw, capacity, z, what, applications=None):
    """apply_statement on the padded state with the NumPy plan against the restatement on the live prefix; a plan that does not fit
    must leave everything as it was."""
    n_old = inp["accum"].shape[0]
    live = K.live_state(inp)
    before = K.pad_state(live, capacity)
    plan, n_new = K.reference_plan(inp, kw)
    stats_reset = bool(kw["clone"] or kw["split"])
    ok, after, count, status = _run_statement(before, plan, n_old, z, kw["curr_gen"], stats_reset)
    if n_new > capacity:
        assert not ok and count == n_old and status == [1, n_new, 0, 0], f"{what}: {status}"
        K.assert_states_equal(after, before, what + " (refused)")
        return n_new
    out = D.densify_and_prune(live, z=lambda rows: z[:rows], **kw)
    assert out["xyz"].shape[0] == n_new, f"{what}: the restatement leaves {out['xyz'].shape[0]} rows, the plan {n_new}"
    assert ok and count == n_new and status == [0, 0, 1, n_new], f"{what}: {status}"
    K.assert_states_equal(after, K.expected_after(before, n_old, out, stats_reset), what)
    return n_new


@pytest.mark.parametrize("n_live", K.LIVE_COUNTS)
def test_statement_matches_the_restatement_on_the_live_prefix(n_live):
    """Every rule set of bookkeeping_cases.py at this live count in a capacity of 4100; at 257 also on the edge model, whose named rows sit
    on the thresholds."""
    z = K.draws(K.CAPACITY)
    inp = K.live_inputs(n_live)
    accepted = refused = 0
    for name, kw in K.rule_sets():
        n_new = _densify_case(inp, kw, K.CAPACITY, z, f"{name} n={n_live}")
        accepted, refused = accepted + (n_new <= K.CAPACITY), refused + (n_new > K.CAPACITY)
    assert accepted > 0 and (refused > 0) == (n_live == K.CAPACITY)        # a full model that grows cannot fit; every smaller one here does
    if n_live == B.EDGE_P:
        edge = B.edge_model()
        for name in B.EDGE_SCENARIOS:
            _densify_case(edge, dict(B.EDGE_SCENARIOS[name]), K.CAPACITY, z, f"edge model {name}")


@pytest.mark.parametrize("n_live", K.LIVE_COUNTS)
@pytest.mark.parametrize("pattern", ["none", "all", "block_density", "last"])
def test_statement_prune_plan(n_live, pattern):
    """The prune plan: every array's kept rows in order, statistics gathered (not zeroed), tags zero on the vacated rows; 'none' prunes
    everything (n_new == 0), 'all' nothing."""
    inp = K.live_inputs(n_live)
    live = K.live_state(inp)
    before = K.pad_state(live, K.CAPACITY)
    keep = B.keep_mask(np.arange(n_live), n_live, pattern)
    plan, n_new = K.prune_plan(keep)
    ok, after, count, status = _run_statement(before, plan, n_live, None, None, False)
    kept = {k: v[torch.from_numpy(np.asarray(keep, bool))] for k, v in live.items()}
    assert ok and count == n_new == int(keep.sum()) and status == [0, 0, 1, n_new]
    K.assert_states_equal(after, K.expected_after(before, n_live, kept, False), f"prune {pattern} n={n_live}")
    if pattern == "none":
        assert n_new == 0 and float(after["generation"][:n_live].abs().sum()) == 0


def _growing_case():
    inp = K.live_inputs(2049)
    kw = dict(K.GROWING)
    plan, n_new = K.reference_plan(inp, kw)
    assert n_new > 2049
    return inp, kw, n_new


def test_statement_exact_fit_is_accepted_and_one_row_short_is_refused():
    """n_new == capacity: applied.  n_new == capacity + 1: every array, statistic and the count bit-identical to before, status advanced --
    and a second refusal counts on (sticky), while a later accepted apply leaves the refusal words alone."""
    from egogaussian_amd import densify
    inp, kw, n_new = _growing_case()
    assert _densify_case(inp, kw, n_new, K.draws(n_new), "exact fit") == n_new
    assert _densify_case(inp, kw, n_new - 1, K.draws(n_new - 1), "one row short") == n_new
    before = K.pad_state(K.live_state(inp), n_new - 1)
    plan, _ = K.reference_plan(inp, kw)
    status = torch.zeros(4, dtype=torch.int64)
    for expect in ([1, n_new, 0, 0], [2, n_new, 0, 0]):
        ok, after, count, st = _run_statement(before, plan, 2049, K.draws(n_new - 1), None, True, status)
        assert not ok and st == expect and count == 2049
        K.assert_states_equal(after, before, "refused twice")
    keep = np.ones(2049, bool); keep[5] = False
    ok, _, count, st = _run_statement(before, K.prune_plan(keep)[0], 2049, None, None, False, status)
    assert ok and count == 2048 and st == [2, n_new, 1, 2048]


@pytest.mark.parametrize("n_live", K.LIVE_COUNTS)
def test_statement_nothing_selected(n_live):
    """No row clones, splits or is pruned: the model, statistics included, is row for row what it was."""
    inp = K.live_inputs(n_live)
    assert _densify_case(inp, dict(K.NOTHING_SELECTED), K.CAPACITY, K.draws(K.CAPACITY), f"nothing selected n={n_live}") == n_live


def test_statement_everything_pruned_by_the_rules():
    """min_opacity above every opacity: n_new == 0, the tags of all former rows zero."""
    inp = K.live_inputs(257)
    kw = dict(K.NOTHING_SELECTED, min_opacity=2.0)
    assert _densify_case(inp, kw, K.CAPACITY, K.draws(K.CAPACITY), "everything pruned") == 0


class _Spy:
    def __init__(self, pc):
        self.calls, self.pc = 0, pc

    def __call__(self):
        self.calls += 1
        return int(self.pc.active_count.item())


def _cpu_model(n=100, capacity=260):
    from egogaussian_amd.capacity import CapacityGaussians
    from egogaussian_amd.scene_synth import make_scene
    pc = CapacityGaussians(make_scene(n, 32, 32, 0), capacity, device="cpu")
    spy = _Spy(pc)
    pc._read_active_count = spy
    return pc, spy


def test_n_active_never_reads_the_word_until_marked_stale():
    pc, spy = _cpu_model()
    assert pc.n_active == 100 and pc.live(pc._xyz).shape[0] == 100
    pc.set_active(180)
    assert pc.n_active == 180 and int(pc.active_count) == 180
    pc.n_active = 120                                               # plain assignment keeps working (what set_active does)
    assert pc.n_active == 120
    pc.grow(400)
    assert pc.n_active == 120 and spy.calls == 0
    with pytest.raises(ValueError):
        pc.set_active(401)


def test_stale_n_active_syncs_exactly_once():
    pc, spy = _cpu_model()
    pc.active_count.fill_(77)                                       # what the commit launch does on the device
    assert pc.n_active == 100 and spy.calls == 0                    # nobody said so: the cached int stands
    pc.mark_active_stale()
    assert spy.calls == 0                                           # marking reads nothing
    assert pc.n_active == 77 and pc.n_active == 77 and pc.live(pc._xyz).shape[0] == 77
    assert spy.calls == 1
    pc.mark_active_stale(); pc.set_active(50)                       # a host-side set makes the int fresh again
    assert pc.n_active == 50 and spy.calls == 1


def test_device_densify_refuses_a_plain_model_and_a_model_without_moments():
    from egogaussian_amd import densify
    from egogaussian_amd.scene_synth import SynthGaussians, make_scene
    plain = SynthGaussians(make_scene(10, 32, 32, 0), device="cpu")
    with pytest.raises(ValueError, match="densify_and_prune"):
        densify.DeviceDensify(plain)
    pc, _ = _cpu_model()
    with pytest.raises(ValueError, match="optimizer"):
        densify.DeviceDensify(pc)
