"""GPU: the object pose sequence on the device (csrc/pose_seq.hip, egogaussian_amd/poses.py) -- the head and tail kernels alone against the
torch mirror in float64 with the float32 CPU mirror as the yardstick, their exact properties, and GraphedTrainStep(pose_sequence=): the
fine_obj pattern against the eager route with host bookkeeping, the coarse alternation in one captured step, a store-fed replay."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0                                   # x the float32 CPU mirror's distance from float64 on the same inputs (tests/anchors.py)
KS = (1, 2, 3, 64, 65, 300)
LR = (1e-3, 2e-3)


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.int32 if t.element_size() == 4 else torch.uint8).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def _rot(rng, amax=0.3):
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    a = rng.uniform(-amax, amax)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


@functools.lru_cache(maxsize=None)
def _table(K):
    """Seeded rel [K,12] (rotations up to 0.3 rad, translations up to 0.5), valid (row 1 invalid where K >= 3), a pose that is not
    orthonormal, Adam moments of a state in progress, per train_row a grad21.  float32 CPU tensors."""
    rng = np.random.default_rng(100 + K)
    rel = np.concatenate([np.stack([_rot(rng) for _ in range(K)]), rng.uniform(-0.5, 0.5, (K, 3, 1))], axis=2).reshape(K, 12)
    valid = np.ones(K, np.uint8)
    if K >= 3:
        valid[1] = 0
    pose = np.concatenate([rng.uniform(-0.5, 0.5, 3), (_rot(rng)[:, :2] + rng.normal(size=(3, 2)) * 0.05).reshape(6)])
    m = rng.normal(size=9) * 1e-2
    v = (np.abs(m) * rng.uniform(1.0, 10.0, 9)) ** 2
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    rows = sorted({0, K // 2, K - 1})
    return dict(rel=f(rel), valid=torch.tensor(valid), pose=f(pose), m=f(m), v=f(v), step=torch.tensor([6.0, 6.0]), rows=rows,
                grads={r: f(rng.normal(size=21)) for r in rows})


def _sequence(K, accumulate=True):
    from egogaussian_amd.poses import PoseSequence
    t = _table(K)
    seq = PoseSequence(range(10, 10 + K), DEV)
    seq.rel.copy_(t["rel"]); seq.valid.copy_(t["valid"]); seq.pose.copy_(t["pose"])
    seq.exp_avg.copy_(t["m"]); seq.exp_avg_sq.copy_(t["v"]); seq.step.copy_(t["step"])
    seq.set_lr(*LR)
    if accumulate:
        seq.accumulate()
    return seq


def _word(*w):
    return torch.tensor(list(w) + [0] * (4 - len(w)), dtype=torch.int32, device=DEV)


def _fixed_for(t, train_row):
    return next((i for i in range(train_row - 1, -1, -1) if int(t["valid"][i])), -1)


def _state(seq):
    return {n: getattr(seq, n).detach().clone() for n in ("rel", "valid", "accum", "pose", "exp_avg", "exp_avg_sq", "step")}


def _dist(x, ref64):
    """max |x - x64| over the array, in units of max |x64|."""
    ref64 = ref64.double().cpu()
    return float((x.double().cpu() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("K", KS)
def test_head_and_tail_against_float64(K):
    """A12, M9, dpose, the written rel row and accum: kernel vs the mirror in float64, the bar = 4 x the float32 CPU mirror's distance from
    float64 on the SAME inputs (the table as it lies on the device, the same pose, moments and grad21); per quantity the largest distance
    over the train rows (first, middle, last) is compared.  accum0: egs_pose_accumulate of the seeded table."""
    from egogaussian_amd import poses
    t = _table(K)
    fig = {}

    def note(name, kernel, yard32, ref64):
        k, y = fig.get(name, (0.0, 0.0))
        fig[name] = (max(k, _dist(kernel, ref64)), max(y, _dist(yard32, ref64)))

    seq = _sequence(K)
    note("accum0", seq.accum, poses.accumulate(t["rel"], t["valid"]), poses.accumulate(t["rel"].double(), t["valid"]))
    for train_row in t["rows"]:
        seq = _sequence(K)
        fixed = _fixed_for(t, train_row)
        accum0 = seq.accum.cpu()                                      # the head's and tail's input: the float32 table on the device
        A12, M9, dpose = torch.zeros(12, device=DEV), torch.zeros(9, device=DEV), torch.zeros(9, device=DEV)
        w = _word(fixed, train_row, 0)
        seq.head(w, A12, M9)
        seq.tail(w, t["grads"][train_row].to(DEV), dpose)
        torch.cuda.synchronize()
        for dtype, sink in ((torch.float64, "ref"), (torch.float32, "yard")):
            c = lambda x: x.to(dtype)
            A, M = poses.compose_from_rows(c(accum0), c(t["pose"]), fixed, train_row)
            out = poses.tail_step(c(accum0), c(t["rel"]), t["valid"], c(t["pose"]), c(t["m"]), c(t["v"]), c(t["step"]), c(torch.tensor(LR, dtype=torch.float32)),
                                  c(t["grads"][train_row]), fixed, train_row, betas=tuple(float(np.float32(b)) for b in poses.BETAS), eps=float(np.float32(poses.EPS)))
            if sink == "ref":
                ref = dict(A12=A.reshape(12), M9=M.reshape(9), dpose=out["dpose"], rel_row=out["rel"][train_row], accum=out["accum"][train_row:])
            else:
                yard = dict(A12=A.reshape(12), M9=M.reshape(9), dpose=out["dpose"], rel_row=out["rel"][train_row], accum=out["accum"][train_row:])
        got = dict(A12=A12, M9=M9, dpose=dpose, rel_row=seq.rel[train_row], accum=seq.accum[train_row:])
        for name in got:
            note(name, got[name], yard[name], ref[name])
        assert int(seq.valid[train_row]) == 1 and seq.step.tolist() == [7.0, 7.0]
    for name, (k, y) in fig.items():
        print(f"K={K} {name}: kernel {k:.3e} yardstick {y:.3e} bar {MARGIN * y:.3e}")
    if os.environ.get("EGS_POSE_PARITY_OUT"):                         # the rows of profiles/pose_sequence_parity.md
        with open(os.environ["EGS_POSE_PARITY_OUT"], "a") as fh:
            for name, (k, y) in fig.items():
                fh.write(f"| {K} | {name} | {k:.3e} | {y:.3e} | {MARGIN * y:.3e} |\n")
    fails = [f"{name}: {k:.3e} > {MARGIN:g} x {y:.3e}" for name, (k, y) in fig.items() if not k <= MARGIN * y]
    assert not fails, f"K={K}: " + "; ".join(fails)


@pytest.mark.parametrize("K", [1, 3, 65])
def test_a_fixed_pose_frame_is_bit_copies_and_leaves_the_state_alone(K):
    t = _table(K)
    seq = _sequence(K)
    before = _state(seq)
    A12, M9 = torch.full((12,), 7.0, device=DEV), torch.full((9,), 7.0, device=DEV)
    for fixed in sorted({-1, 0, K - 1}):
        w = _word(fixed, -1, 1)
        seq.head(w, A12, M9)
        seq.tail(w, t["grads"][0].to(DEV), None)
        torch.cuda.synchronize()
        row = seq.accum[fixed] if fixed >= 0 else torch.eye(4, device=DEV)[:3].reshape(12)
        assert same(A12, row) and same(M9, row.reshape(3, 4)[:, :3])
        for n, v in _state(seq).items():
            assert same(v, before[n]), (fixed, n)
    # rows outside the table mean "none" as well: nothing outside it is addressed
    seq.head(_word(K, K + 5, 1), A12, M9)
    seq.tail(_word(K, K + 5, 1), t["grads"][0].to(DEV), None)
    torch.cuda.synchronize()
    assert same(A12, torch.eye(4, device=DEV)[:3].reshape(12))
    for n, v in _state(seq).items():
        assert same(v, before[n]), n


@pytest.mark.parametrize("K", [3, 65, 300])
def test_tail_keeps_the_rows_below_and_equals_the_full_accumulation(K):
    """Rows below train_row of accum are bit-unchanged; the suffix the tail writes equals egs_pose_accumulate of the table it left; two runs
    give the same bits everywhere; an overflowed frame (skip word set) takes no step."""
    t = _table(K)
    for train_row in t["rows"]:
        runs = []
        for _ in range(2):
            seq = _sequence(K)
            before = _state(seq)
            A12, M9, dpose = torch.zeros(12, device=DEV), torch.zeros(9, device=DEV), torch.zeros(9, device=DEV)
            w = _word(_fixed_for(t, train_row), train_row, 0)
            seq.head(w, A12, M9)
            seq.tail(w, t["grads"][train_row].to(DEV), dpose, skip=torch.ones(2, dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            for n, v in _state(seq).items():
                assert same(v, before[n]), ("skip", n)
            seq.tail(w, t["grads"][train_row].to(DEV), dpose, skip=torch.zeros(2, dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            after = _state(seq)
            assert same(after["accum"][:train_row], before["accum"][:train_row])
            assert same(after["rel"][:train_row], before["rel"][:train_row]) and same(after["rel"][train_row + 1:], before["rel"][train_row + 1:])
            assert not same(after["pose"], before["pose"]) and not same(after["accum"][train_row:], before["accum"][train_row:])
            seq.accum.fill_(3.0)
            seq.accumulate()
            torch.cuda.synchronize()
            assert same(seq.accum, after["accum"]), "egs_pose_accumulate differs from the tail's suffix"
            runs.append(dict(after, A12=A12, M9=M9, dpose=dpose))
        for n in runs[0]:
            assert same(runs[0][n], runs[1][n]), n


def test_reload_makes_the_rows_pose_the_parameters():
    K = 3
    t = _table(K)
    seq = _sequence(K)
    A12, M9 = torch.zeros(12, device=DEV), torch.zeros(9, device=DEV)
    seq.head(_word(0, 2, 1), A12, M9)
    torch.cuda.synchronize()
    row = t["rel"][2].reshape(3, 4)
    assert same(seq.pose, torch.cat([row[:, 3], row[:, :2].reshape(6)]))
    from egogaussian_amd import poses
    A, _ = poses.compose_from_rows(seq.accum.cpu().double(), seq.pose.cpu().double(), 0, 2)
    assert _dist(A12, A.reshape(12)) <= 4 * float(np.finfo(np.float32).eps)


def test_the_tails_adam_is_the_capturable_adam_bit_for_bit():
    """Three consecutive tail calls; next to them egs_adam_step_capturable on a copy of the state, fed the tail's own dpose: parameter, both
    moments and the step counts agree bit for bit after every call."""
    from egogaussian_amd import lib, _hip, poses
    L = lib.load()
    K = 3
    t = _table(K)
    seq = _sequence(K)
    p, m, v = seq.pose.clone(), seq.exp_avg.clone(), seq.exp_avg_sq.clone()
    step, lr = seq.step.clone(), seq.lr.clone()
    counters = [torch.full((1,), int(s), dtype=torch.int32, device=DEV) for s in step.tolist()]
    dpose = torch.zeros(9, device=DEV)
    gen = torch.Generator().manual_seed(3)
    for call in range(3):
        w = _word(0, 2, 0)
        seq.tail(w, torch.randn(21, generator=gen).to(DEV), dpose)
        g = dpose.clone()
        parts = lambda x: [x[0:3], x[3:9]]
        arr = lambda ts: (C.c_void_p * 2)(*[x.data_ptr() for x in ts])
        NN = (C.c_int64 * 2)(3, 6)
        with _hip.device_ctx(torch.device(DEV)):
            lib.check(L.egs_adam_step_capturable(2, arr(parts(p)), arr(parts(g)), arr(parts(m)), arr(parts(v)), NN, arr([step[0:1], step[1:2]]),
                                                 arr([lr[0:1], lr[1:2]]), arr(counters), poses.BETAS[0], poses.BETAS[1], poses.EPS, None, None, None,
                                                 _hip.stream_of(torch.device(DEV))))
        torch.cuda.synchronize()
        assert same(seq.pose, p) and same(seq.exp_avg, m) and same(seq.exp_avg_sq, v) and same(seq.step, step), call
        assert seq.step.tolist() == [7.0 + call] * 2


# ---- the captured step ---------------------------------------------------------------------------------------------------------------
POSE_LR, K_STEPS = 1e-3, 4
KEYS4 = ("1", "2", "3", "4")


def _rel4():
    """Four relative poses: the first carries the object to where the scene of test_gpu_motion.py expects it, the others nudge it on."""
    from tests.test_gpu_motion import _pose
    Ts = [_pose(0.4, (0.5, -0.3, 0.4))] + [_pose(0.02 * k, (0.01 * k, -0.01, 0.005 * k)) for k in (1, 2, 3)]
    return [T[:3].clone() for T in Ts]


def _sequence4(lr=POSE_LR):
    from egogaussian_amd.poses import PoseSequence
    seq = PoseSequence(KEYS4, DEV)
    for k, T in zip(KEYS4, _rel4()):
        seq.set(k, T[:, 3], T[:, :3])
    seq.accumulate()
    seq.set_lr(lr, lr)
    return seq


def _step_with_sequence(pc, seq, lrs=True, **kw):
    from tests.test_gpu_motion import _groups
    from tests.test_gpu_object_loss import LAM, W_OBJ, _frames
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep
    cams, Ts, bg, gt, mask, gate = _frames()
    opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
    step = GraphedTrainStep(pc, opt, bg, LAM, dynamic=True, motion=True, gated=True, object_loss=W_OBJ, pose_sequence=seq, **kw)
    return step, opt


def test_graphed_step_over_dynamic_frames_against_the_eager_route_with_host_bookkeeping():
    """The fine_obj pattern: every frame trains its own row on top of the rows before it, reload = 1.  One warm-up step plus K = 4 replays
    over different dynamic frames with NO host work between them, against two runs of the parent's eager route doing the bookkeeping on the
    host (`.data` reload, write-back, re-accumulation with the mirror).  Bars: those of test_graphed_step_with_a_trainable_pose."""
    from tests.test_gpu_motion import _model, LEAVES, Move
    from tests.test_gpu_object_loss import _eager_step, _frames, _pose_groups
    from egogaussian_amd import poses
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import pack_frame
    cams, Ts, bg, gt, mask, gate = _frames()
    order = [0] + [k % 4 for k in range(1, K_STEPS + 1)]
    rows = lambda k: (k - 1, k, 1)                                    # every key is valid: the last valid key before frame k is k - 1
    pa, seq = _model(0), _sequence4()
    step, oa = _step_with_sequence(pa, seq)
    step.capture(cams[0], gt, warmup=1, gate=gate, obj_mask=mask, capacity_margin=2.0, pose_rows=rows(0))
    la = []
    later_changed = None
    for k in order[1:]:
        before = seq.accum.clone()
        la.append(float(step(pack_frame(cams[k], gt, gate=gate, obj_mask=mask, pose_rows=rows(k)))))
        if k == 1:                                                    # a dynamic step moved the accumulated pose of every later frame, with no host write
            torch.cuda.synchronize()
            later_changed = same(seq.accum[0], before[0]) and all(not same(seq.accum[j], before[j]) for j in (1, 2, 3))
            accum_after_1 = seq.accum.cpu().double()
        if k == 2:                                                    # ... and frame 2 was composed on top of it
            torch.cuda.synchronize()
            r2 = torch.tensor(_rel4()[2].numpy()).double()
            pose2 = torch.cat([r2[:, 3], r2[:, :2].reshape(6)])
            A, _ = poses.compose_from_rows(accum_after_1, pose2, 1, 2)
            assert float((step.accum_T.cpu().double() - A).abs().max()) <= 1e-5
    torch.cuda.synchronize()
    assert step.ok() and later_changed
    assert seq.step.tolist() == [K_STEPS + 1.0] * 2 and float(oa.state[pa._xyz]["step"]) == K_STEPS + 1
    table_a = (seq.rel.cpu(), seq.accum.cpu())
    runs = []
    for _ in range(2):
        pb, pose_b = _model(0), Move((0.0, 0.0, 0.0), [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]], DEV)
        ob = FusedAdam(_pose_groups(pb, pose_b), lr=0.0, eps=1e-15, capturable=True)
        rel = torch.stack([T.reshape(12) for T in _rel4()])
        valid = torch.ones(4, dtype=torch.uint8)
        lb = []
        for k in order:
            accum = poses.accumulate(rel, valid)                     # get_accum_T_seq / get_accum_R_seq on the host
            T = torch.eye(4)
            if k > 0:
                T[:3] = accum[k - 1].reshape(3, 4)
            row = rel[k].reshape(3, 4)
            pose_b.obj_translation.data.copy_(row[:, 3]); pose_b.obj_rotation_6d.data.copy_(row[:, :2])      # fine_obj.py:118-119
            lb.append(_eager_step(pb, ob, cams[k], T.to(DEV), bg, gt, mask, gate, pose=pose_b))
            with torch.no_grad():                                     # get_obj_trans_rot, stored under the frame's key
                rel[k] = torch.cat([Move.matrix(pose_b.obj_rotation_6d), pose_b.obj_translation[:, None]], dim=1).reshape(12).cpu()
        torch.cuda.synchronize()
        runs.append((rel, poses.accumulate(rel, valid), pb, lb))
    for name, a, b1, b2 in (("rel", table_a[0], runs[0][0], runs[1][0]), ("accum", table_a[1], runs[0][1], runs[1][1])):
        bound = 4 * (b1 - b2).abs() + 1e-4 * POSE_LR * K_STEPS
        print(name, "max |a - b1|", float((a - b1).abs().max()), "max |b1 - b2|", float((b1 - b2).abs().max()), "floor", 1e-4 * POSE_LR * K_STEPS)
        assert bool(((a - b1).abs() <= bound).all()), name
    assert float((table_a[0] - torch.stack([T.reshape(12) for T in _rel4()])).abs().max()) > 0
    lb = runs[0][3]
    print("losses", la, lb[1:])
    assert all(abs(u - v) <= 2e-3 * abs(u) for u, v in zip(lb[1:], la)), (lb, la)
    for a in ("_xyz",) + LEAVES:
        u, v = getattr(pa, a).detach(), getattr(runs[0][2], a).detach()
        print(a, float((u - v).abs().mean()), float(u.abs().mean()))
        assert float((u - v).abs().mean()) <= 2e-4 * float(u.abs().mean()) + 1e-7, a


def test_coarse_alternation_in_one_captured_step():
    """Replays alternating trainable-pose frames (train_row >= 0, reload = 0) and fixed-pose frames (train_row < 0) of ONE captured step."""
    from tests.test_gpu_motion import _model, LEAVES
    from tests.test_gpu_object_loss import _frames
    from egogaussian_amd.graph import pack_frame
    cams, Ts, bg, gt, mask, gate = _frames()
    pa, seq = _model(0), _sequence4()
    step, oa = _step_with_sequence(pa, seq)
    step.capture(cams[0], gt, warmup=1, gate=gate, obj_mask=mask, capacity_margin=2.0, pose_rows=(0, -1))
    leaves = ("_xyz",) + LEAVES
    pose_state = lambda: {n: getattr(seq, n).detach().clone() for n in ("pose", "exp_avg", "exp_avg_sq", "step")}
    model_state = lambda: {a: getattr(pa, a).detach().clone() for a in leaves}
    frame = lambda k, rows: pack_frame(cams[k], gt, gate=gate, obj_mask=mask, pose_rows=rows)
    assert seq.step.tolist() == [0.0, 0.0]                            # the warm-up frame had a fixed pose
    n_train = 0
    for k, rows in ((1, (0, 1, 0)), (2, (2, -1)), (3, (2, 3, 0)), (0, (0, -1)), (1, (0, 1, 0)), (2, (1, -1, 1))):
        p0, m0 = pose_state(), model_state()
        step(frame(k, rows))
        torch.cuda.synchronize()
        p1, m1 = pose_state(), model_state()
        assert not same(m1["_xyz"], m0["_xyz"]) and not same(m1["_opacity"], m0["_opacity"]), "the Gaussians step on every frame"
        if rows[1] < 0:
            for n in p0:
                assert same(p0[n], p1[n]), (k, n)
        else:
            n_train += 1
            assert not same(p0["pose"][:3], p1["pose"][:3]) and not same(p0["pose"][3:], p1["pose"][3:])
            assert p1["step"].tolist() == [float(n_train)] * 2
    assert step.ok() and float(oa.state[pa._xyz]["step"]) == 7.0
    for g in oa.param_groups:                                         # the stages' zero_gaussians_lr: the Gaussians freeze, the pose keeps moving
        g["lr"] = 0.0
    p0, m0 = pose_state(), model_state()
    step(frame(3, (2, 3, 0)))
    torch.cuda.synchronize()
    p1, m1 = pose_state(), model_state()
    assert all(same(m0[a], m1[a]) for a in leaves) and not same(p0["pose"], p1["pose"])
    seq.set_lr(0.0, 0.0)                                              # zero_pose_lr: the value freezes, the step count advances
    step(frame(1, (0, 1, 0)))
    torch.cuda.synchronize()
    p2 = pose_state()
    assert same(p1["pose"], p2["pose"]) and p2["step"].tolist() == [float(n_train + 2)] * 2


def _run_store_schedule(feed):
    """Six replays on the one-wave scene of tests/test_gpu_frames.py (a step there has no order of float atomics to vary), every frame with
    its own pose_rows word: from packed frames, or from a FrameStore holding the same frames."""
    from tests.test_gpu_frames import _grid_scene, W_OBJ
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.poses import PoseSequence
    from egogaussian_amd.scene_synth import SynthGaussians
    H, W = 48, 64
    s = _grid_scene(H, W)
    words = [(-1, 0, 1), (0, 1, 1), (1, -1), (1, 2, 0), (2, 3, 1), (3, -1)]
    store = FrameStore(H, W, 6, DEV, dynamic=True, motion=True, gated=True, object_loss=True, pose_rows=True)
    eye = torch.eye(4, device=DEV)
    for k in range(6):
        store.put(k, s["cam"], gt=s["gt8"][k], accum_R=eye[:3, :3], accum_T=eye[:3], gate=s["gates"][k], obj_mask=s["masks"][k], pose_rows=(-1, -1))
        store.set_pose_rows(k, words[k])
    floats = [store.frame(k) for k in range(6)]
    seq = PoseSequence(KEYS4, DEV)
    for i, k in enumerate(KEYS4):
        seq.set(k, torch.tensor([1e-4 * i, -1e-4, 0.0]), torch.eye(3))
    seq.accumulate()
    seq.set_lr(1e-5, 1e-5)
    pc = SynthGaussians(s["student"], device=DEV)
    pc._is_object = s["is_object"]
    opt = pc.training_setup(FusedAdam, capturable=True)
    kw = dict(dynamic=True, motion=True, gated=True, object_loss=W_OBJ, pose_sequence=seq)
    if feed == "packed":
        p = store.parts(0)
        step = GraphedTrainStep(pc, opt, s["bg"], 0.2, **kw).capture(s["cam"], p["gt"], warmup=1, capacity_margin=2.0, gate=p["gate"], obj_mask=p["obj_mask"],
                                                                    pose_rows=words[0])
    else:
        step = GraphedTrainStep(pc, opt, s["bg"], 0.2, frame_store=store, ring_capacity=16, **kw).capture(s["cam"], index=0, warmup=1, capacity_margin=2.0)
    for i in (1, 2, 3, 4, 5, 0):
        step(floats[i] if feed == "packed" else i)
    torch.cuda.synchronize()
    assert step.ok() and (feed == "packed" or step.store_ok())
    state = {n: getattr(seq, n).detach().clone() for n in ("rel", "valid", "accum", "pose", "exp_avg", "exp_avg_sq", "step")}
    for a in ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"):
        state[a] = getattr(pc, a).detach().clone()
    return state


def test_store_fed_replay_equals_the_packed_frame_replay():
    packed, again = _run_store_schedule("packed"), _run_store_schedule("packed")
    assert all(same(packed[n], again[n]) for n in packed), "two runs of the packed-frame step differ: the scene does not make the step deterministic"
    assert packed["step"].tolist() == [5.0, 5.0] and packed["valid"].tolist() == [1, 1, 1, 1]
    stored = _run_store_schedule("store")
    diff = [n for n in packed if not same(packed[n], stored[n])]
    assert not diff, diff


def test_misuse_is_refused():
    from tests.test_gpu_motion import _model, _groups
    from tests.test_gpu_object_loss import _pose_groups, _pose_module
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    bg = torch.zeros(3, device=DEV)
    pc, pose, seq = _model(0), _pose_module(), _sequence4()
    with pytest.raises(ValueError, match="pose="):
        GraphedTrainStep(pc, FusedAdam(_pose_groups(pc, pose), lr=0.0, eps=1e-15, capturable=True), bg, dynamic=True, motion=True, pose=pose, pose_sequence=seq)
    for kw in (dict(), dict(dynamic=True)):
        with pytest.raises(ValueError, match="motion=True"):
            GraphedTrainStep(pc, FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True), bg, pose_sequence=seq, **kw)
