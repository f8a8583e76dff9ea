"""GPU: stage 4 on the device (csrc/pose_seq.hip egs_pose_interpolate, PoseSequence.interpolated) -- the kernel against the float64 mirror
under the bar of tests/interpolation_cases.py (per entry max(3 x the float32 mirror's largest distance from float64 on the case, 2 float32
ulps of max(1, |entry|))), its exact properties, the table against the reference's recorded run, and the evaluation pass as the consumer."""
import functools

import numpy as np
import pytest
import torch

from tests import interpolation_cases as ic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("small_n2", "n3", "n5", "n16", "n32", "translation_n5", "identity_n3")      # n = 2 (the minimum) .. 32 (the maximum)
FILL = 7.0
ERR_RANGE = -3


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.int32 if t.element_size() == 4 else torch.uint8).cpu()


def _launch(transforms, words, K_new, iters=1500, lr=0.01):
    """egs_pose_interpolate on an old table holding `transforms` (float32 [4,4] each, row i = transform i) and a new table of K_new rows
    filled with FILL -> (return code, rel [K_new,12], valid [K_new], residual [G]) on the host."""
    from egogaussian_amd import lib, _hip
    from egogaussian_amd.poses import PoseSequence
    old, new = PoseSequence(range(len(transforms)), DEV), PoseSequence(range(K_new), DEV)
    old.rel.copy_(torch.stack([T[:3].reshape(12) for T in transforms])); old.valid.fill_(1)
    new.rel.fill_(FILL)
    w = torch.tensor(words, dtype=torch.int32).reshape(-1, 3).to(DEV)
    res = torch.full((w.shape[0],), FILL, device=DEV)
    status = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    dev = torch.device(DEV)
    with _hip.device_ctx(dev):
        code = lib.load().egs_pose_interpolate(old.struct(), new.struct(), w.data_ptr(), w.shape[0], iters, lr, res.data_ptr(), status.data_ptr(),
                                               _hip.stream_of(dev))
    torch.cuda.synchronize()
    assert int(status) == (1 if code == ERR_RANGE else 0)
    return code, new.rel.cpu(), new.valid.cpu(), res.cpu()


def _inputs():
    return [ic.case_inputs(name) for name in CASES]


def _mixed_words():
    words, first = [], 1                                             # (row 0 and the last row belong to no gap)
    for i, (_, n) in enumerate(_inputs()):
        words.append((first, n, i)); first += n
    return words, first + 1


@functools.lru_cache(maxsize=None)
def _mixed():
    """ONE launch over all the cases' lengths (read-only afterwards)."""
    words, K = _mixed_words()
    return _launch([T for T, _ in _inputs()], words, K)


def test_kernel_against_the_float64_mirror():
    code, rel, valid, res = _mixed()
    assert code == 0
    words, K = _mixed_words()
    untouched = torch.full((12,), FILL)
    assert torch.equal(rel[0], untouched) and torch.equal(rel[K - 1], untouched) and valid.tolist() == [0] + [1] * (K - 2) + [0]
    fails = []
    for name, (first, n, _), (T, _), r in zip(CASES, words, _inputs(), res.tolist()):
        m = ic.mirrors(T, n)
        assert all(torch.equal(bits(rel[first + k]), bits(rel[first])) for k in range(n)), name
        x, xr = ic.row_excess(rel[first], m), ic.residual_excess(r, m)
        print(f"{name}: n = {n}, row / bar {x:.3f}, residual {r:.3e} (float64 mirror {m['res64']:.3e}, float32 mirror {m['res32']:.3e}) / bar {xr:.3f}")
        if not (x <= 1.0 and xr <= 1.0):
            fails.append((name, x, xr))
        if name.startswith("identity"):
            assert torch.equal(bits(rel[first]), bits(torch.eye(4)[:3].reshape(12))) and r == 0.0
    assert not fails, fails


def test_a_gaps_rows_do_not_depend_on_the_launch():
    """Bit-identical alone (at another place of another table), in the mixed launch, and on a second run of it."""
    code, rel, valid, res = _mixed()
    words, K = _mixed_words()
    code2, rel2, valid2, res2 = _launch([T for T, _ in _inputs()], words, K)
    assert code2 == 0 and torch.equal(bits(rel), bits(rel2)) and torch.equal(bits(res), bits(res2)) and torch.equal(valid, valid2)
    for name, (first, n, _), (T, _) in zip(CASES, words, _inputs()):
        c, r1, v1, s1 = _launch([T], [(0, n, 0)], n)
        assert c == 0 and v1.tolist() == [1] * n
        assert torch.equal(bits(r1), bits(rel[first:first + n])) and torch.equal(bits(s1), bits(res[CASES.index(name)])), name


def test_words_out_of_range_are_refused_and_nothing_is_written():
    Ts = [T for T, _ in _inputs()][:3]
    K = 12
    good = [(0, 2, 0), (2, 3, 1), (5, 5, 2)]
    big = 2 ** 31 - 1
    for bad in [(10, 1, 0), (0, 33, 0), (10, 0, 0), (10, -4, 0), (-1, 2, 0), (11, 2, 0), (K, 2, 0), (10, 2, -1), (10, 2, 3), (big, 2, 0), (10, big, 0),
                (10, 2, big), (-big - 1, 2, 0)]:
        for words in ([bad], good + [bad], [bad] + good):
            code, rel, valid, res = _launch(Ts, words, K)
            assert code == ERR_RANGE, (bad, code)
            assert bool((rel == FILL).all()) and bool((res == FILL).all()) and not bool(valid.any()), bad
    code, rel, valid, res = _launch(Ts, good + [(10, 2, 0)], K)       # the last two rows: inside
    assert code == 0 and valid.tolist() == [1] * K and torch.equal(bits(rel[10]), bits(rel[0]))


def _scenario_args():
    g = ic.golden()
    return [str(f) for f in g["run_frames"]], [tuple(str(x) for x in p) for p in g["run_phases"]]


def test_interpolated_table_against_the_recorded_run():
    from tests.test_pose_interpolation_cpu import _old_sequence, check_table_against_the_recording
    old = _old_sequence(DEV)
    before = {n: getattr(old, n).clone() for n in ("rel", "valid", "accum")}
    new = old.interpolated(*_scenario_args(), check=False)
    torch.cuda.synchronize()
    assert new.rel.is_cuda and new.gap_residual.is_cuda
    check_table_against_the_recording(old, new)
    for n, v in before.items():
        assert torch.equal(bits(v), bits(getattr(old, n))), n
    accum = new.accum.clone()
    new.accum.fill_(3.0)
    new.accumulate()                                                  # egs_pose_accumulate afresh
    torch.cuda.synchronize()
    assert torch.equal(bits(accum), bits(new.accum))
    again = old.interpolated(*_scenario_args(), check=False)
    assert all(torch.equal(bits(getattr(new, n)), bits(getattr(again, n))) for n in ("rel", "valid", "accum", "gap_residual"))


def test_check_names_a_gap_that_ended_off_and_keeps_quiet_otherwise(monkeypatch):
    import warnings
    from egogaussian_amd import poses
    T, n = ic.case_inputs("n3")
    old = poses.PoseSequence(["2", "5"], DEV)
    old.set("2", torch.zeros(3), torch.eye(3)); old.set("5", T[:3, 3], T[:3, :3])
    old.accumulate()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        new = old.interpolated(range(8), [(3, 5)])
    assert new.keys == ["2", "3", "4", "5"] and new.gaps == [(1, 3, 1)]
    real = poses._lib.load()

    class TwoSteps:                                                   # the library with this entry cut to two iterations: far from the mirror's end point
        def __getattr__(self, name):
            return getattr(real, name)

        def egs_pose_interpolate(self, a, b, w, G, iters, lr, res, status, stream):
            return real.egs_pose_interpolate(a, b, w, G, 2, lr, res, status, stream)
    monkeypatch.setattr(poses._lib, "load", lambda: TwoSteps())
    with pytest.warns(UserWarning, match="frames 3 .. 5"):
        old.interpolated(range(8), [(3, 5)])


def test_eval_pass_renders_a_held_out_frame_at_its_own_pose():
    """An object scene of the sizes tests/test_gpu_pose_sequence.py uses; keys 1, 2, 4 trained, frame 3 held out inside the phase (2, 4).  The
    evaluation pass at frame 3 with the new table's accumulated pose renders what the float64 mirror's pose composed by hand renders, and
    not what the previous key's pose -- all the old table could offer -- renders."""
    from tests.test_gpu_motion import _model, _pose
    from tests.test_gpu_object_loss import _frames
    from egogaussian_amd.evaluate import EvalPass
    from egogaussian_amd.graph import pack_frame
    from egogaussian_amd.poses import PoseSequence
    cams, _, bg, gt, _, gate = _frames()
    rel = {"1": _pose(0.4, (0.5, -0.3, 0.4)), "2": _pose(0.02, (0.01, -0.01, 0.005)), "4": _pose(0.25, (0.3, -0.2, 0.1))}
    old = PoseSequence(rel, DEV)
    for k, T in rel.items():
        old.set(k, T[:3, 3], T[:3, :3])
    old.accumulate()
    assert old.rows("3") == (1, -1)                                   # before: the pose of key 2
    new = old.interpolated(["1", "2", "3", "4"], [("2", "4")], check=False)
    assert new.keys == ["1", "2", "3", "4"] and new.gaps == [(2, 2, 2)] and new.rows("3") == (2, -1) and new.rows("4") == (3, -1)
    m = ic.mirrors(rel["4"], 2)
    M = torch.eye(4, dtype=torch.float64); M[:3] = m["row64"].reshape(3, 4)
    under = torch.eye(4, dtype=torch.float64); under[:3] = old.accum[1].double().cpu().reshape(3, 4)
    by_hand = (M @ under).float().to(DEV)
    own, previous = torch.eye(4, device=DEV), torch.eye(4, device=DEV)
    own[:3], previous[:3] = new.accum[2].reshape(3, 4), old.accum[1].reshape(3, 4)
    assert float((own - by_hand).abs().max()) <= 4 * float(np.finfo(np.float32).eps) * float(by_hand.abs().max())
    frames = [pack_frame(cams[2], gt, accum_R=T[:3, :3].contiguous(), gate=gate, accum_T=T) for T in (own, by_hand, previous)]
    ev = EvalPass(_model(0), bg, dynamic=True, motion=True, which_object=1, graphed=False, keep_images=True)
    img = ev.run(frames, cams[2])["images"].cpu().to(torch.int16)
    same, other = (img[0] - img[1]).abs(), (img[0] - img[2]).abs()
    print("own vs by hand: max", int(same.max()), "entries", int((same > 0).sum()), "| own vs previous key: max", int(other.max()), "entries", int((other > 0).sum()))
    # a pose that differs in the last place moves a colour by ~1e-7: at most a quantisation step, on next to no entries
    assert int(same.max()) <= 1 and int((same > 0).sum()) <= img[0].numel() // 1000
    assert int(other.max()) >= 32 and int((other > 0).sum()) >= img[0].numel() // 100
