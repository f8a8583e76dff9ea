"""Cases shared by tests/test_device_densify_cpu.py (densify.apply_statement against oracle/densify_torch.py) and
tests/test_gpu_device_densify.py (densify.DeviceDensify against the host-driven densify_and_prune / prune_points): capacity-sized
states built from tests/bookkeeping_cases.py's generators, the rule sets of that file, and what a state must look like afterwards.
Nothing in here comes from the code under test."""
import numpy as np
import torch

from tests import bookkeeping_cases as B

CAPACITY = 4100
LIVE_COUNTS = (1, 257, 2049, 4100)        # one row; two 256-thread workgroups; one and two scan blocks of 2048 crossed
JUNK = 7                                  # what rows at and beyond the live count hold: not zeros, so a stray write or read shows
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
TAGS = ("generation", "is_object")


def rule_sets():
    """(name, keyword arguments incl. percent_dense) of every rule set of bookkeeping_cases.py: the 24 switch combinations on the lattice
    thresholds and the six edge scenarios."""
    out = [("lattice-" + "".join("01"[int(b)] for b in combo), B.combo_kw(combo)) for combo in B.lattice_combos()]
    out += [("edge-" + name, dict(kw)) for name, kw in B.EDGE_SCENARIOS.items()]
    return out


# No clone or split step, no opacity below 0, no size rule: every row stays where it is (and the statistics are not reset).
NOTHING_SELECTED = dict(max_grad=1.0, min_opacity=0.0, extent=4.0, max_screen_size=None, percent_dense=0.01, clone=False, split=False,
                        curr_gen=None, prune_prev_gen=True, which_object=None)


# Nothing is pruned (sigmoid(-4) = 0.018 > 0.01, no size rule) while every third row clones or splits: the model grows.
GROWING = dict(B.LATTICE_KW, max_screen_size=None, min_opacity=0.01, clone=True, split=True, curr_gen=2, prune_prev_gen=True, which_object=None)


def live_inputs(n_live, seed=0):
    """The lattice inputs with real geometry: positions, quaternions (unnormalised) and features that differ row by row."""
    return B.lattice_inputs(n_live, seed)


def live_state(inp, seed=0):
    """bookkeeping_cases.restatement_state with positions and rotations a split child's arithmetic can go wrong on, and moments that
    differ row by row."""
    st = B.restatement_state(inp)
    P = inp["accum"].shape[0]
    g = torch.Generator().manual_seed(4000 + seed + P)
    st["xyz"] = torch.randn(P, 3, generator=g) * 3.0
    st["rotation"] = torch.randn(P, 4, generator=g) * (0.5 + torch.rand(P, 1, generator=g) * 4.0)
    for k in B_PARAMS:
        st[k + "_exp_avg"] = torch.randn(st[k].shape, generator=g)
        st[k + "_exp_avg_sq"] = torch.rand(st[k].shape, generator=g)
    return st


B_PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "label")


def pad_state(st, capacity):
    """Every array of a live state with junk rows up to `capacity`."""
    n = st["xyz"].shape[0]
    pad = lambda t: torch.cat([t, torch.full((capacity - n,) + tuple(t.shape[1:]), JUNK, dtype=t.dtype)])
    return {k: pad(v) for k, v in st.items()}


def draws(capacity, seed=0):
    """z [2 capacity, 3]: the draws of every run; the first 2 n_split rows are what the host-sized routes are handed."""
    return torch.randn(2 * capacity, 3, generator=torch.Generator().manual_seed(77 + seed))


def reference_plan(inp, kw):
    """The plan of the live prefix from the NumPy rule table (bookkeeping_cases.rule_flags + plan_reference) and its new row count."""
    plan = B.plan_reference(B.rule_flags(inp, kw))
    t = plan["totals"]
    return plan, t[0] + t[1] + 2 * t[2]


def prune_plan(keep):
    plan = B.plan_reference(B.prune_flags(np.asarray(keep, bool)))
    return plan, plan["totals"][0]


def expected_after(before, n_old, new_live, stats_reset):
    """The capacity-sized state after an accepted apply, from the state before and the new live rows a host-sized reference produced:
    rows [0, n_new) are the new model; tags are zero on [n_new, n_old); the statistics are zero everywhere after a clone / split step;
    every other row is what it was."""
    out = {k: v.clone() for k, v in before.items()}
    n_new = new_live["xyz"].shape[0]
    for k, v in out.items():
        if k in STATS and stats_reset:
            v.zero_()
            continue
        v[:n_new] = new_live[k].to(v.dtype)
        if k in TAGS and n_new < n_old:
            v[n_new:n_old] = 0
    return out


def assert_states_equal(got, want, what=""):
    """torch.equal on every array (NaN-free by construction); names the first differing row."""
    assert set(got) == set(want), f"{what}: arrays {sorted(set(got) ^ set(want))}"
    for k in want:
        g, w = got[k].cpu(), want[k].cpu()
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {tuple(g.shape)} {g.dtype}, expected {tuple(w.shape)} {w.dtype}"
        if not torch.equal(g, w):
            rows = (g != w).reshape(g.shape[0], -1).any(1).nonzero().flatten()
            r = int(rows[0])
            raise AssertionError(f"{what}: {k} differs in {rows.numel()} rows, first row {r}: {g[r].flatten()[:4].tolist()} vs {w[r].flatten()[:4].tolist()}")
