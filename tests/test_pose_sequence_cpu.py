"""CPU: the torch mirror of the object pose sequence (egogaussian_amd/poses.py) against the fixture recorded from the reference's own
functions (tests/golden/pose_sequence.npz, recipe: tests/golden/make_golden_pose_sequence.py), against motion.ObjectMotion.compose() and
against float64 autograd; the frame rule; the frame layout's new segment; the C ABI's additions."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "pose_sequence.npz"))
KEYS = [str(k) for k in G["keys"]]
FRAMES = [str(f) for f in G["frames"]]
EPS32 = float(np.finfo(np.float32).eps)


def _sequence(variant, device="cpu"):
    from egogaussian_amd.poses import PoseSequence
    seq = PoseSequence(reversed(KEYS), device)                     # (any order: the constructor sorts)
    for k in KEYS:
        if bool(G[f"{variant}_has_{k}"]):
            seq.set(k, torch.tensor(G["t_" + k]), torch.tensor(G["R_" + k]))
    seq.accumulate()
    return seq


@pytest.mark.parametrize("variant", ["full", "gap"])
def test_accumulate_matches_the_reference_sequences(variant):
    """accumulate vs get_accum_T_seq / get_accum_R_seq: the same float32 products in the same order -- a few ulp of the entries' scale."""
    seq = _sequence(variant)
    assert seq.keys == KEYS
    aT, aR = seq.accum_T_seq(), seq.accum_R_seq()
    acc = seq.accum.reshape(-1, 3, 4)
    prev = torch.eye(4)[:3]
    for i, k in enumerate(KEYS):
        if not bool(G[f"{variant}_has_{k}"]):
            assert aT[k] is None and aR[k] is None and seq.export()[k] is None
            assert torch.equal(acc[i], prev), "an invalid row repeats its predecessor"
            continue
        T, R = torch.tensor(G[f"{variant}_accT_{k}"]), torch.tensor(G[f"{variant}_accR_{k}"])
        assert float((aT[k] - T).abs().max()) <= 8 * EPS32 * float(T.abs().max()), k
        assert float((aR[k] - R).abs().max()) <= 8 * EPS32, k
        assert torch.equal(aR[k], acc[i][:, :3]) and torch.equal(aT[k][:3], acc[i]) and torch.equal(aT[k][3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
        e = seq.export()[k]
        assert torch.equal(e["translation"], torch.tensor(G["t_" + k])) and torch.equal(e["rotation"], torch.tensor(G["R_" + k]))
        prev = acc[i]


def test_accumulate_suffix_continues_the_full_chain():
    from egogaussian_amd.poses import accumulate
    seq = _sequence("gap")
    full = accumulate(seq.rel, seq.valid)
    for start in (0, 1, 3, 6):
        broken = full.clone()
        broken[start:] = 7.0
        assert torch.equal(accumulate(seq.rel, seq.valid, start=start, accum=broken), full)
    assert torch.equal(accumulate(seq.rel, torch.zeros(7)), torch.eye(4)[:3].reshape(1, 12).expand(7, 12))


def test_rot6d_to_matrix_and_its_gradient():
    from egogaussian_amd.poses import rot6d_to_matrix
    for i in range(int(G["n_r6"])):
        r6 = torch.tensor(G[f"r6_{i}"], requires_grad=True)
        R = rot6d_to_matrix(r6)
        (R * torch.tensor(G[f"r6_w_{i}"])).sum().backward()
        assert float((R.detach() - torch.tensor(G[f"r6_R_{i}"])).abs().max()) <= 4 * EPS32, i
        g = torch.tensor(G[f"r6_grad_{i}"])
        assert float((r6.grad - g).abs().max()) <= 16 * EPS32 * max(1.0, float(g.abs().max())), i
        flat = rot6d_to_matrix(torch.tensor(G[f"r6_{i}"]).reshape(6))
        assert torch.equal(flat, R.detach())


def _reference_dicts(seq):
    return {k: v for k, v in seq.accum_T_seq().items() if v is not None}, {k: v for k, v in seq.accum_R_seq().items() if v is not None}


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("frame", FRAMES)
def test_rows_reproduce_the_recorded_triples_and_select_motion(frame, training):
    from egogaussian_amd.motion import select_motion
    seq = _sequence("full")
    fixed_row, train_row = seq.rows(frame, training)
    p = f"rule_{frame}_{int(training)}_"
    assert p + "error" not in G.files
    aT, aR = _reference_dicts(seq)
    sel = select_motion(aT, aR, frame, training, trainable=object() if training else None)
    acc = seq.accum.reshape(-1, 3, 4)
    if p + "fell_off" in G.files or not bool(G[p + "has_fixed"]):
        assert (fixed_row, train_row) == (-1, -1) and sel is None
        return
    assert sel is not None
    assert (train_row >= 0) == bool(G[p + "has_trainable"]) == (sel.trainable is not None)
    T = acc[fixed_row] if fixed_row >= 0 else torch.eye(4)[:3]
    assert float((T - torch.tensor(G[p + "fixed_T"])[:3]).abs().max()) <= 8 * EPS32 * float(T.abs().max())
    assert float((T[:, :3] - torch.tensor(G[p + "fixed_R"])).abs().max()) <= 8 * EPS32
    assert torch.equal(T, sel.fixed_T[:3]) and torch.equal(T[:, :3], sel.fixed_R)
    if training:
        assert KEYS[train_row] == next(k for k in KEYS if int(k) >= int(frame))


def test_rows_on_a_sequence_with_an_invalid_key():
    seq = _sequence("gap")
    gap = KEYS.index(str(G["none_key"]))
    assert seq.rows(KEYS[gap], True) == (gap - 1, gap)              # training: the last valid key strictly before the frame
    assert seq.rows(KEYS[gap + 1], True) == (gap - 1, gap + 1)      # ... which skips the invalid one
    assert seq.rows(str(int(KEYS[gap]) + 5), False) == (gap - 1, -1)
    with pytest.raises(ValueError, match="no pose yet"):
        seq.rows(KEYS[gap], False)
    seq.clear(KEYS[0])
    assert seq.rows(KEYS[0], True) == (-1, 0) and seq.rows(KEYS[1], True) == (-1, 1)
    with pytest.raises(KeyError):
        seq.set("00021", torch.zeros(3), torch.eye(3))
    with pytest.raises(ValueError):
        seq.word((0, 7))
    assert seq.word((2, 3), reload=True).tolist() == [2, 3, 1, 0]


class _Move:
    def __init__(self, pose):
        self.obj_translation, self.obj_rotation_6d = pose[0:3], pose[3:9].reshape(3, 2)

    def rot_L(self, L):
        from egogaussian_amd.poses import rot6d_to_matrix
        return rot6d_to_matrix(self.obj_rotation_6d) @ L


def _case(dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    seq = _sequence("gap")
    pose = torch.cat([torch.tensor(G["obj_translation"]), torch.tensor(G["obj_rotation_6d"]).reshape(6) + 0.05 * torch.randn(6, generator=gen)])
    return seq.accum.to(dtype), seq.rel.to(dtype), seq.valid, pose.to(dtype), torch.randn(21, generator=gen).to(dtype)


@pytest.mark.parametrize("fixed_row", [-1, 2])
def test_compose_from_rows_equals_object_motion_compose(fixed_row):
    from egogaussian_amd.motion import ObjectMotion
    from egogaussian_amd.poses import compose_from_rows
    accum, _, _, pose, _ = _case(torch.float32)
    T = torch.eye(4)
    if fixed_row >= 0:
        T[:3] = accum[fixed_row].reshape(3, 4)
    A12, M = compose_from_rows(accum, pose, fixed_row, 3)
    A12_ref, M_ref = ObjectMotion(T, _Move(pose)).compose("cpu")
    assert torch.equal(A12, A12_ref) and torch.equal(M, M_ref)
    A12, M = compose_from_rows(accum, pose, fixed_row, -1)          # a fixed-pose frame: the row and its block themselves
    assert torch.equal(A12, T[:3]) and torch.equal(M, T[:3, :3])


@pytest.mark.parametrize("fixed_row", [-1, 2])
def test_tail_step_gradients_equal_float64_autograd_through_compose(fixed_row):
    from egogaussian_amd.motion import ObjectMotion
    from egogaussian_amd.poses import pose_gradient, tail_step
    accum, rel, valid, pose, g21 = _case(torch.float64)
    T = torch.eye(4, dtype=torch.float64)
    if fixed_row >= 0:
        T[:3] = accum[fixed_row].reshape(3, 4)
    leaf = pose.clone().requires_grad_(True)
    A = ObjectMotion(T, _Move(leaf))
    Tl, Rl = A.fixed_T, A.fixed_R
    Rt = A.trainable.rot_L(torch.eye(3, dtype=torch.float64))       # (compose() itself works in float32: its expressions in float64)
    A12 = torch.cat([Rt @ Tl[:3, :3], (Rt @ Tl[:3, 3] + leaf[0:3])[:, None]], dim=1)
    ((A12.reshape(12) * g21[:12]).sum() + ((Rt @ Rl).reshape(9) * g21[12:]).sum()).backward()
    g = pose_gradient(accum, pose, g21, fixed_row)
    assert float((g - leaf.grad).abs().max()) <= 1e-13 * float(leaf.grad.abs().max())
    z = lambda n: torch.zeros(n, dtype=torch.float64)
    out = tail_step(accum, rel, valid, pose, z(9), z(9), z(2), torch.tensor([1e-3, 2e-3], dtype=torch.float64), g21, fixed_row, 3)
    assert torch.equal(out["dpose"], g) and out["step"].tolist() == [1.0, 1.0] and int(out["valid"][3]) == 1
    # the first Adam step moves every scalar by its learning rate against the gradient's sign
    want = pose - torch.cat([torch.full((3,), 1e-3, dtype=torch.float64), torch.full((6,), 2e-3, dtype=torch.float64)]) * torch.sign(g)
    assert float((out["pose"] - want).abs().max()) <= 1e-12
    assert torch.equal(out["accum"][:3], accum[:3]) and not torch.equal(out["accum"][3:], accum[3:])
    same = tail_step(accum, rel, valid, pose, z(9), z(9), z(2), z(2), g21, fixed_row, -1)
    assert same["dpose"] is None and all(same[k] is v for k, v in (("pose", pose), ("rel", rel), ("valid", valid), ("accum", accum)))


def test_frame_layout_keeps_every_other_offset():
    from egogaussian_amd.graph import frame_layout, frame_views, pack_frame, pose_word
    from egogaussian_amd.scene_synth import make_camera
    for H, W in ((7, 9), (96, 160), (540, 960)):
        for gated in (False, True):
            for obj in (False, True):
                a, size_a = frame_layout(3 * H * W, H * W, True, gated, True, obj)
                b, size_b = frame_layout(3 * H * W, H * W, True, gated, True, obj, pose_rows=True)
                assert b["pose_rows"] == (a["accum_T"][1], a["accum_T"][1] + 4) and size_b == size_a + 4
                for name, (lo, hi) in a.items():
                    shift = 4 if lo >= b["pose_rows"][0] else 0
                    assert b[name] == (lo + shift, hi + shift), name
                for name in ("gt", "cam", "accum_R", "accum_T"):
                    assert a[name] == b[name]
                assert "pose_rows" not in frame_layout(3 * H * W, H * W, True, gated, True, obj)[0]
    H, W = 7, 9
    cam = make_camera(3, H, W)
    f = pack_frame(cam, torch.rand(3, H, W), pose_rows=(2, 3, 1))
    off, _ = frame_layout(3 * H * W, H * W, True, False, True, pose_rows=True)
    v = frame_views(f, off, H, W)
    assert v["pose_rows"].dtype == torch.int32 and v["pose_rows"].tolist() == [2, 3, 1, 0]
    assert torch.equal(v["accum_R"], torch.eye(3)) and torch.equal(v["accum_T"], torch.eye(4)[:3])
    assert pose_word((-1, -1)).tolist() == [-1, -1, 0, 0]
    with pytest.raises(ValueError):
        pose_word((1,))


def test_frame_store_carries_the_word_untouched():
    from egogaussian_amd import lib
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.graph import pack_frame
    from egogaussian_amd.scene_synth import make_camera
    H, W = 7, 9
    cam = make_camera(3, H, W)
    gt = torch.randint(0, 256, (3, H, W), dtype=torch.uint8).float() / 255.0
    frames = [pack_frame(cam, gt, pose_rows=rows) for rows in ((-1, -1), (-1, 0, 1), (0, 1, 1))]
    store = FrameStore.from_packed(frames, H, W, dynamic=True, motion=True, pose_rows=True)
    for i, f in enumerate(frames):
        assert torch.equal(store.frame(i).view(torch.int32), f.view(torch.int32)), i
    store.set_pose_rows(1, (2, -1))
    assert store.parts(1)["pose_rows"].tolist() == [2, -1, 0, 0] and store.parts(2)["pose_rows"].tolist() == [0, 1, 1, 0]
    fl = lib.FrameLayout()
    assert lib.load().egs_frame_store_layout(H, W, store.flags, C.byref(fl)) == 0
    assert (fl.small_floats, fl.frame_floats) == (store.small_floats, store.frame_floats) and fl.small_floats == 64
    assert lib.load().egs_frame_store_layout(H, W, lib.FRAME_POSE_ROWS | lib.FRAME_DYNAMIC, C.byref(fl)) == -2
    with pytest.raises(ValueError):
        FrameStore(H, W, 1, dynamic=True, pose_rows=True)
    with pytest.raises(ValueError):
        FrameStore(H, W, 1, dynamic=True, motion=True).set_pose_rows(0, (0, 0))
    assert "pose_rows" not in FrameStore(H, W, 1, dynamic=True, motion=True).layout


def test_abi_additions_and_argument_errors():
    from egogaussian_amd import lib
    L = lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egs_raster.h")).read(), flags=re.S)
    for n in ("egs_pose_head", "egs_pose_tail", "egs_pose_accumulate"):
        assert re.search(r"\b%s\s*\(" % n, text) and n in lib.SIGNATURES and hasattr(L, n), n
    assert L.egs_abi_version() == 6 and re.search(r"#define\s+EGS_FRAME_POSE_ROWS\s+32\b", text)
    assert "pose_seq.hip" in open(os.path.join(ROOT, "egogaussian_amd", "csrc", "Makefile")).read()
    assert lib.built_source_hash() == lib.kernel_source_hash()
    p = 4096                                                           # (fake non-null pointers are never dereferenced before the checks)
    st = lib.PoseSequence()
    st.K = 3
    for name in ("rel", "valid", "accum", "pose", "exp_avg", "exp_avg_sq", "step", "lr"):
        setattr(st, name, p)
    assert L.egs_pose_head(None, p, p, p, None) == -1 and L.egs_pose_head(C.byref(st), None, p, p, None) == -1
    assert L.egs_pose_head(C.byref(st), p, None, p, None) == -1 and L.egs_pose_head(C.byref(st), p, p, None, None) == -1
    assert L.egs_pose_tail(C.byref(st), None, p, p, p, None) == -1 and L.egs_pose_tail(C.byref(st), p, None, p, p, None) == -1
    assert L.egs_pose_accumulate(None, None) == -1
    for name in ("rel", "valid", "accum", "pose", "exp_avg", "exp_avg_sq", "step", "lr"):
        setattr(st, name, None)
        assert L.egs_pose_accumulate(C.byref(st), None) == -1, name
        setattr(st, name, p)
    st.K = 0
    assert L.egs_pose_accumulate(C.byref(st), None) == -1


def test_kernels_have_no_cpu_path():
    seq = _sequence("full")
    with pytest.raises(RuntimeError, match="HIP devices only"):
        seq.head(torch.zeros(4, dtype=torch.int32), torch.zeros(12), torch.zeros(9))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        seq.tail(torch.zeros(4, dtype=torch.int32), torch.zeros(21))
