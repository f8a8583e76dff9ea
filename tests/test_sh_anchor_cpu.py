"""CPU: the spherical-harmonics anchor itself (tests/sh_anchor.py) -- the table reaches every path of the dispatch rule, the float64
reference agrees with egogaussian_amd.sh.eval_sh and with autograd, the float32 yardstick stays under half of every bar, every deliberately
wrong variant fails a check, the clamp band is thin, and the direction term is not negligible in the cases that check it."""
import numpy as np
import pytest
import torch

from tests import sh_anchor as sa


def _cases():
    return [sa.get_case(k) for k in sa.table()]


def test_table_covers_the_axes():
    keys = sa.table()
    assert 100 <= len(keys) <= 150 and len(set(keys)) == len(keys)
    assert {k[0] for k in keys} == set(sa.PS)
    assert {(k[1], k[3]) for k in keys} == set(sa.M_ACTIVE)
    assert {k[2] for k in keys} == set(sa.LAYOUTS)
    assert {k[4] for k in keys} == set(sa.PATTERNS)
    whole_block_culled = [k for k in keys if k[4] == "block-1-empty"]
    assert whole_block_culled and all(k[0] >= 128 for k in whole_block_culled)


def test_table_reaches_every_cell_of_the_dispatch_rule():
    """{generic, sh16-CAT, sh16-SPLIT} x {vector, scalar / tail} x {forward, backward} x every active degree, and nvalid % 4 in {0,1,2,3} for SPLIT."""
    hit, residues, families = set(), set(), set()
    for case in _cases():
        family, cells = sa.expected_path(case)
        families.add(family)
        hit |= {(family, direction, loader, case.active) for direction, loader in cells}
        residues |= sa.split_tail_residues(case)
    want = {(f, d, l, a) for f in ("generic", "sh16-cat", "sh16-split") for d in ("forward", "backward") for l in ("vector", "tail") for a in range(4)}
    assert not want - hit, sorted(want - hit)
    assert residues == {0, 1, 2, 3}
    assert "inline" in families


def test_dispatch_mirror_on_known_cases():
    c = lambda P, M, layout, active, pattern: sa.sh_case(P, M, layout, active, pattern, 1)
    assert sa.expected_path(c(64, 16, "cat", 3, "all")) == ("sh16-cat", {("forward", "vector"), ("backward", "vector")})
    assert sa.expected_path(c(65, 16, "split", 0, "all")) == ("sh16-split", {("forward", "vector"), ("forward", "tail"), ("backward", "vector"), ("backward", "tail")})
    assert sa.expected_path(c(64, 16, "split-unaligned", 1, "all"))[0] == "generic"
    # 63 rows of 27 words: 1701 is odd -> the scalar loop; the forward of an all-culled model loads nothing
    assert sa.expected_path(c(63, 9, "cat", 2, "all")) == ("generic", {("forward", "tail"), ("backward", "tail")})
    assert sa.expected_path(c(64, 9, "cat", 2, "none")) == ("generic", {("backward", "vector")})
    assert sa.expected_path(c(4, 1, "cat", 0, "all")) == ("inline", set())


def test_cases_are_poisoned_and_what_they_claim():
    neg = tot = 0
    for case in _cases():
        nb = (case.active + 1) ** 2
        sh = case.shs.numpy()
        assert np.isnan(sh[~case.visible]).all() and np.isnan(sh[:, nb:]).all() and np.isfinite(sh[case.visible][:, :nb]).all()
        ref = sa.evaluate(case, np.float64)
        neg += int(ref.neg[case.visible].sum()); tot += 3 * int(case.visible.sum())
        d = (case.means3D - case.cam.campos).numpy()[case.visible]
        if case.P >= 24 and case.pattern == "all":
            assert ((d == 0).sum(1) == 2).any() and ((d == 0).sum(1) == 1).any(), "rows on a coordinate axis and in a coordinate plane"
            assert (1.0 / np.linalg.norm(d, axis=1)).max() > 1.5, "rows close to the camera"
    assert 0.25 < neg / tot < 0.5, neg / tot                            # a third or so of the channels is clamped


@pytest.mark.parametrize("key", [(191, 16, "cat", 3, "all"), (130, 9, "cat", 2, "all"), (67, 4, "cat", 1, "random-half"), (65, 16, "cat", 0, "all")], ids=sa.case_id)
def test_reference_matches_eval_sh_and_autograd(key):
    from egogaussian_amd.sh import eval_sh
    case = sa.sh_case(*key, seed=3)
    vis = torch.from_numpy(case.visible)
    nb = (case.active + 1) ** 2
    ref = sa.evaluate(case, np.float64)
    g, _ = sa.synthetic_upstream(case)
    bw = sa.backward(case, ref, g, ref.neg)
    p = case.means3D[vis].double().requires_grad_(True)
    sh = case.shs[vis][:, :nb].double().requires_grad_(True)
    d = p - case.cam.campos.double()
    v = eval_sh(case.active, sh.transpose(1, 2), d / d.norm(dim=1, keepdim=True)) + 0.5
    assert np.abs(v.detach().numpy() - ref.v[case.visible]).max() <= 1e-13 * ref.unit.max()
    gz = torch.from_numpy(np.where(ref.neg, 0.0, g.astype(np.float64)))[vis]
    (torch.clamp_min(v, 0.0) * torch.from_numpy(g.astype(np.float64))[vis]).sum().backward()
    assert np.abs(sh.grad.numpy() - bw.dsh[case.visible][:, :nb]).max() <= 1e-13 * max(bw.unit.max(), 1e-300)
    assert float(bw.dsh[:, nb:].max(initial=0.0)) == 0.0
    scale = np.abs(bw.t).max() if case.active else 1.0
    p_grad = np.zeros_like(bw.t[case.visible]) if p.grad is None else p.grad.numpy()      # (degree 0 does not see the direction)
    assert np.abs(p_grad - bw.t[case.visible]).max() <= 1e-12 * scale
    assert (np.abs(bw.t).max() > 0) == (case.active > 0) and gz.abs().sum() > 0


def test_yardstick_stays_under_half_of_every_bar():
    for case in _cases():
        r = sa.yardstick_ratios(case)
        bar = sa.bars(case)
        for q in ("color", "dsh", "pos"):
            assert r[q] <= 0.5 * bar[q], (case.id, q, r[q], bar[q])
        assert not r["zeros"], (case.id, r["zeros"])
    for active in range(4):
        ty = sa.table_yardstick(active)
        print(f"active degree {active}: yardstick ratios (u) colour {ty['color']:.2f}  dL/dSH {ty['dsh']:.2f}  direction term {ty['pos']:.2f}")
        assert all(0 < ty[q] < 64 for q in ("color", "dsh")), ty       # a float32 evaluation of a few dozen operations, not a cancellation
        # degree 0 has no direction term: b + 0 is b, and the bar is equality.  Above it the tangent projection g - d (d . g) cancels where g is
        # nearly along d, and the unit u (|a| + |b| + |t64|) does not know |g|: hundreds of u in the worst row, still 1e-4 of the term
        assert (0 < ty["pos"] < 4096) if active else ty["pos"] == 0, ty


def test_the_yardstick_passes_and_every_wrong_variant_fails():
    caught = {v: [] for v in sa.VARIANTS}
    for case in _cases():
        g, b = sa.synthetic_upstream(case)
        fails, _ = sa.verdict(case, sa.variant_result(case, None, g, b), g, b)
        assert not fails, (case.id, fails)
        for v in sa.VARIANTS:
            fails, _ = sa.verdict(case, sa.variant_result(case, v, g, b), g, b)
            if fails:
                caught[v].append(case.id)
    for v, ids in caught.items():
        print(f"{v}: fails {len(ids)} of {len(sa.table())} cases")
        assert ids, f"no check notices the variant {v}"


def test_clamp_band_is_thin():
    """Channels whose |v64| lies inside the colour bar may carry either clamp bit: at most 1 % of the visible channels."""
    inside = tot = 0
    for case in _cases():
        ref = sa.evaluate(case, np.float64)
        vis = case.visible
        inside += int((np.abs(ref.v[vis]) <= sa.bars(case)["color"] * sa.U * ref.unit[vis]).sum())
        tot += 3 * int(vis.sum())
    assert inside <= sa.BAND_CAP * tot, (inside, tot)


def test_direction_term_is_not_negligible_next_to_the_projection_term():
    """Float64 oracle on the cases of the position check (active degree > 0): in at least half of the visible rows |t| >= 2^-10 |dL/dmeans3D|."""
    from oracle.oracle import Oracle
    from tests.common import seeded_grads
    o = Oracle(np.float64)
    grads = [x.double() for x in seeded_grads(sa.H, sa.W, 5)]
    big = tot = 0
    for case in _cases():
        if case.active == 0 or not case.visible.any():
            continue
        st = o.forward(**{k: (v.double() if torch.is_tensor(v) else v) for k, v in sa.oracle_inputs(case).items()})
        assert np.array_equal(st["radii"] > 0, case.visible), case.id
        gb = o.backward(st, *grads)
        ref = sa.evaluate(case, np.float64)
        assert np.array_equal(st["clamped"].astype(bool), ref.neg) or sa.clamp_mismatches(case, st["clamped"].astype(bool), ref, 1.0)[0] == 0
        t = sa.backward(case, ref, gb["dL_dcolor"].astype(np.float32), ref.neg).t
        tn, dn = np.linalg.norm(t[case.visible], axis=1), np.linalg.norm(gb["dL_dmeans3D"][case.visible], axis=1)
        big += int((tn >= 2.0 ** -10 * dn).sum()); tot += int(case.visible.sum())
    print(f"direction term >= 2^-10 of dL/dmeans3D in {big} of {tot} visible rows")
    assert 2 * big >= tot
