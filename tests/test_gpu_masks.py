"""GPU: the mask hand-off -- the two kernels (fused.interaction_gate, fused.label_mask) against the numpy definitions of tests/mask_anchor.py,
the captured sweep (egogaussian_amd/masks.py MaskPass) against the eager one and against the definition applied to the eager label render,
the model split, and a gated captured training step fed by the gate kernel.  Everything is integer-exact: every comparison is an equality."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import mask_anchor as MA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- 1. egs_interaction_gate --------------------------------------------------------------------------------------------------------------
GATE_SIZES = [(1, 1), (3, 5), (5, 64), (7, 65), (37, 53), (48, 64), (70, 130), (33, 200), (100, 200)]
GATE_KS = (1, 3, 5, 15, 31)


def _tile_rows(k):
    """Output rows of one wave of k_interaction_gate (masks.hip egs_interaction_gate): its tiles are 64 columns x this many rows."""
    r = k // 2
    return (1 if r <= 2 else 2 if r <= 4 else 3 if r <= 8 else 5) * 8 - 2 * r


def _gate(a, b, k, **kw):
    from egogaussian_amd import fused
    t = lambda m: None if m is None else torch.from_numpy(m).to(DEV)
    if a is None:                                                        # only the second input: through the C ABI's `b`
        from egogaussian_amd import lib, _hip
        bt = t(b)
        out = torch.empty(bt.shape, dtype=torch.float32, device=DEV)
        with _hip.device_ctx(bt.device):
            lib.check(lib.load().egs_interaction_gate(bt.shape[0], bt.shape[1], None, bt.data_ptr(), k, out.data_ptr(), _hip.stream_of(bt.device)))
        return out.cpu().numpy()
    return fused.interaction_gate(t(a), t(b), k, **kw).cpu().numpy()


def _singles(H, W, k):
    """Masks of isolated set pixels: the four corners; the middle of the last row and of the last column; both sides of the kernel's tile seams."""
    rows = _tile_rows(k)
    groups = [[(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)], [(H - 1, W // 2), (H // 2, W - 1)],
              [(rows - 1, 63), (rows, 64), (2 * rows - 1, 127), (2 * rows, 128)]]
    out = []
    for g in groups:
        m = np.zeros((H, W), np.float32)
        for y, x in g:
            if y < H and x < W:
                m[y, x] = 1.0
        if m.any():
            out.append(m)
    return out


@pytest.mark.parametrize("shape", GATE_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_interaction_gate_equals_the_definition(shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    assert (100, 200) in GATE_SIZES and 100 >= 3 * max(_tile_rows(k) for k in range(1, 32, 2)) and 200 >= 3 * 64      # three tiles each way at every k
    for k in GATE_KS:
        a = (rng.random((H, W)) < 0.01).astype(np.float32)
        b = (rng.random((H, W)) < 0.01).astype(np.float32)
        a[rng.integers(H), rng.integers(W)] = 1.0                        # (1 % of a few pixels may be none)
        b[rng.integers(H), rng.integers(W)] = 1.0
        cases = [("a", a, None), ("b", None, b), ("both", a, b)] + [(f"single{i}", m, None) for i, m in enumerate(_singles(H, W, k))]
        odd = np.zeros((H, W), np.float32)
        for i, v in enumerate((-1.0, 0.25, 2.0, float("nan"))):
            odd[(i * 7) % H, (i * 29) % W] = v
        cases += [("values", odd, None), ("values-b", np.zeros((H, W), np.float32), odd)]
        for name, x, y in cases:
            want = MA.gate_np(x, y, k)
            got = _gate(x, y, k)
            assert got.dtype == np.float32 and np.array_equal(got, want), (shape, k, name, int((got != want).sum()))
        zeros, ones = np.zeros((H, W), np.float32), np.ones((H, W), np.float32)
        assert np.array_equal(_gate(zeros, zeros, k), ones) and np.array_equal(_gate(zeros, None, k), ones)
        assert np.array_equal(_gate(ones, None, k), zeros) and np.array_equal(_gate(zeros, ones, k), zeros)


def test_interaction_gate_probes_at_the_window_edge():
    """A probe pixel exactly k // 2 away from a set pixel is gated, one further is not: horizontally, vertically and diagonally."""
    H, W, y, x = 70, 130, 33, 66
    a = np.zeros((H, W), np.float32); a[y, x] = 1.0
    for k in GATE_KS:
        r = k // 2
        got = _gate(a, None, k)
        assert np.array_equal(got, MA.gate_np(a, None, k))
        for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)):
            assert got[y + dy * r, x + dx * r] == 0.0, (k, dy, dx)
            assert got[y + dy * (r + 1), x + dx * (r + 1)] == 1.0, (k, dy, dx)
        assert int((got == 0).sum()) == k * k


def test_interaction_gate_writes_a_misaligned_view_and_nothing_around_it():
    """`out` is a view starting at an odd float offset of a larger tensor (the gate segment of a packed frame is such a view): the view holds
    the gate, the floats around it are unchanged; masks of other types and [1,H,W] shapes are converted first."""
    from egogaussian_amd import fused
    H, W, k = 37, 53, 5
    rng = np.random.default_rng(3)
    a, b = (rng.random((H, W)) < 0.02).astype(np.float32), (rng.random((H, W)) < 0.02).astype(np.float32)
    want = MA.gate_np(a, b, k)
    for lead in (1, 3):
        big = torch.full((lead + H * W + 9,), 7.0, device=DEV)
        view = big[lead:lead + H * W]
        assert view.data_ptr() % 16 != 0
        ret = fused.interaction_gate(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), k, out=view)
        assert ret is view
        host = big.cpu().numpy()
        assert np.array_equal(host[lead:lead + H * W].reshape(H, W), want)
        assert (host[:lead] == 7.0).all() and (host[lead + H * W:] == 7.0).all()
    as_bytes = fused.interaction_gate(torch.from_numpy((a * 255).astype(np.uint8)).to(DEV)[None], torch.from_numpy(b > 0).to(DEV), k)
    assert np.array_equal(as_bytes.cpu().numpy(), want)
    assert np.array_equal(fused.interaction_gate(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy(), MA.gate_np(a, b, 1))
    with pytest.raises(ValueError):
        fused.interaction_gate(torch.from_numpy(a).to(DEV), None, 4)
    with pytest.raises(RuntimeError):
        fused.interaction_gate(torch.from_numpy(a).to(DEV), None, 3, out=torch.empty(5, device=DEV))


# ---- 2. egs_label_mask -----------------------------------------------------------------------------------------------------------------------
def _rows_host(rows):
    return rows.cpu().numpy()


def _check_row(row, want, instances=(0, 0)):
    assert [int(v) for v in row] == [want["predicted"], want["target"], want["intersection"], want["kept"], instances[0], instances[1]], (list(map(int, row)), want)


@pytest.mark.parametrize("thr", [0.5, -0.25])
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 53), (48, 64), (70, 130)], ids=lambda s: "x".join(map(str, s)))
def test_label_mask_equals_the_definition(shape, thr):
    """Mask bytes and the four counts against label_mask_np of the same device image read back: with and without target / keep, without mask
    bytes, on aligned tensors (16-byte loads where H*W allows) and on views that start at odd offsets (4-byte loads, byte stores)."""
    from egogaussian_amd import fused
    H, W = shape
    img_h, spots = MA.special_label_image(H, W, thr, seed=H * W + 1)
    rng = np.random.default_rng(9)
    target_h = (rng.random((H, W)) < 0.4).astype(np.float32)
    keep_h = (rng.random((H, W)) < 0.7).astype(np.float32)
    if H * W > 1:
        assert {"exact", "next", "nan", "differ"} <= set(spots)

    def placed(host, lead, dtype=torch.float32):
        big = torch.zeros(lead + host.size + 5, dtype=dtype, device=DEV)
        big[lead:lead + host.size] = torch.from_numpy(host.reshape(-1)).to(DEV)
        return big[lead:lead + host.size].view(host.shape)

    for lead in (0, 1):                                                  # 0: fresh allocations; 1: every tensor one element into a larger one
        img = placed(img_h, lead)
        back = img.cpu().numpy()
        assert np.array_equal(back.view(np.int32), img_h.view(np.int32))
        for t_h, k_h in ((target_h, keep_h), (target_h, None), (None, keep_h), (None, None)):
            want = MA.label_mask_np(back, thr, t_h, k_h)
            t = None if t_h is None else placed(t_h, lead)
            k = None if k_h is None else placed(k_h, lead)[None]
            out = None
            if lead:
                store = torch.full((H * W + 8,), 9, dtype=torch.uint8, device=DEV)
                out = store[3:3 + H * W].view(H, W)
            res = fused.label_mask(img, thr, target=t, keep=k, out=out)
            assert np.array_equal(res["mask8"].cpu().numpy(), want["mask"]), (shape, thr, lead)
            if lead:
                s = store.cpu().numpy()
                assert (s[:3] == 9).all() and (s[3 + H * W:] == 9).all()
            assert int(res["cursor"]) == 1
            _check_row(_rows_host(res["rows"])[0], want)
            res2 = fused.label_mask(img, thr, target=t, keep=k, mask=False)          # mask8 = NULL: the counts alone
            assert res2["mask8"] is None
            _check_row(_rows_host(res2["rows"])[0], want)
    for name, (y, x) in spots.items():
        assert want["mask"][y, x] == {"exact": 0, "next": 255, "nan": 0, "differ": 255}[name], name


def test_label_mask_rows_cursor_overflow_word_and_determinism():
    """Two consecutive calls fill rows 0 and 1 and leave the cursor at 2; a full row array is left untouched while the cursor counts on; the
    overflow word travels in the row; two runs give identical rows."""
    from egogaussian_amd import fused
    H, W = 70, 130
    img_h, _ = MA.special_label_image(H, W, 0.5, seed=77)
    rng = np.random.default_rng(10)
    t_h, k_h = (rng.random((H, W)) < 0.5).astype(np.float32), (rng.random((H, W)) < 0.8).astype(np.float32)
    img, t, k = (torch.from_numpy(v).to(DEV) for v in (img_h, t_h, k_h))
    want0, want1 = MA.label_mask_np(img_h, 0.5, t_h, k_h), MA.label_mask_np(img_h, -0.25, t_h, None)
    overflow = torch.tensor([1, 4321], dtype=torch.int32, device=DEV)
    runs = []
    for _ in range(2):
        rows, cursor = fused.mask_rows(2, DEV)
        fused.label_mask(img, 0.5, target=t, keep=k, rows=rows, cursor=cursor)
        fused.label_mask(img, -0.25, target=t, rows=rows, cursor=cursor, overflow=overflow)
        assert int(cursor) == 2
        r = _rows_host(rows)
        _check_row(r[0], want0); _check_row(r[1], want1, instances=(1, 4321))
        before = r.copy()
        fused.label_mask(img, 0.5, rows=rows, cursor=cursor)                              # the array is full
        assert int(cursor) == 3 and np.array_equal(_rows_host(rows), before)
        runs.append(before)
    assert np.array_equal(runs[0], runs[1])
    assert want0["predicted"] != want1["predicted"] and 0 < want0["intersection"] < want0["predicted"]
    cursor.fill_(-1)
    fused.label_mask(img, 0.5, rows=rows, cursor=cursor)                                  # a negative cursor writes nothing either
    assert int(cursor) == 0 and np.array_equal(_rows_host(rows), runs[0])


# ---- 3. MaskPass ---------------------------------------------------------------------------------------------------------------------------
N, H, W, F = 2000, 48, 64, 6
FRAMES = (20, 60, 110, 160, 210, 280)


@functools.lru_cache(maxsize=None)
def _scene():
    """-> dict: scene, labels (+2 on the 30 % of the Gaussians with the smallest x, -2 elsewhere: a region of its own in every view), cameras,
    keeps (1 - a rectangular hand per frame), object masks, packed label frames."""
    from egogaussian_amd.scene_synth import make_scene, make_camera
    from egogaussian_amd.graph import pack_label_frame
    scene = make_scene(N, H, W, 3); scene["log_scale"] += math.log(3.0)
    x = scene["xyz"][:, 0]
    label = np.where(x < np.quantile(x, 0.3), 2.0, -2.0).astype(np.float32)[:, None]
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in FRAMES]
    gen = torch.Generator().manual_seed(11)
    keeps, objs = [], []
    for k in range(F):
        keep = torch.ones(H, W, device=DEV)
        y0, x0 = int(torch.randint(0, H - 22, (1,), generator=gen)), int(torch.randint(0, W - 30, (1,), generator=gen))
        keep[y0:y0 + 10 + 2 * k, x0:x0 + 12 + 3 * k] = 0.0                 # the hand: a rectangle of its own per frame
        obj = torch.zeros(H, W, device=DEV)
        obj[4 + k:30 + k, 0:20 + 2 * k] = 1.0                               # the dataset's object mask: a rectangle on the object's side
        keeps.append(keep); objs.append(obj)
    frames = [pack_label_frame(cams[k], objs[k], gate=keeps[k]) for k in range(F)]
    return dict(scene=scene, label=label, bg=bg, cams=cams, keeps=keeps, objs=objs, frames=frames)


def _model():
    from egogaussian_amd.scene_synth import SynthGaussians
    s = _scene()
    pc = SynthGaussians(s["scene"], device=DEV, requires_grad=False)
    pc._label = torch.from_numpy(s["label"]).to(DEV)
    return pc


def _pass(graphed, **kw):
    from egogaussian_amd.masks import MaskPass
    s = _scene()
    mp = MaskPass(_model(), s["bg"], graphed=graphed)
    return mp, mp.run(s["frames"], s["cams"][0], **kw)


@functools.lru_cache(maxsize=None)
def _sweeps():
    """(captured, eager, label_mask_np of the eager get_render_label(scalar=True) images read back) -- computed once, read-only."""
    from egogaussian_amd.renderer import get_render_label
    s = _scene()
    g = _pass(True)
    e = _pass(False)
    pc = _model()
    host = []
    with torch.no_grad():
        for k in range(F):
            img = get_render_label(s["cams"][k], pc, s["bg"], scalar=True).detach().cpu().numpy()
            host.append(MA.label_mask_np(img, 0.5, s["objs"][k].cpu().numpy(), s["keeps"][k].cpu().numpy()))
    torch.cuda.synchronize()
    return g, e, host


COUNTS = ("predicted", "target", "intersection", "kept")


def test_captured_sweep_equals_eager_sweep_and_the_definition():
    (mp_g, g), (mp_e, e), host = _sweeps()
    assert g["rerendered"] == [] and e["rerendered"] == [] and (g["instances"] > 0).all() and (e["instances"] == 0).all()
    assert g["masks"].dtype == torch.uint8 and tuple(g["masks"].shape) == (F, H, W) and g["masks"].is_cuda
    gm, em = g["masks"].cpu().numpy(), e["masks"].cpu().numpy()
    set_px = []
    for k in range(F):
        whole = int((host[k]["mask"] == 255).sum())
        set_px.append(whole)
        print(f"frame {k}: predicted {int(g['predicted'][k])} / {int(e['predicted'][k])} / {host[k]['predicted']}, target {int(g['target'][k])}, "
              f"intersection {int(g['intersection'][k])}, kept {int(g['kept'][k])}, iou {g['iou'][k]:.4f}, set pixels {whole} of {H * W}, "
              f"instances {int(g['instances'][k])}")
        assert np.array_equal(gm[k], em[k]) and np.array_equal(gm[k], host[k]["mask"]), k
        for name in COUNTS:
            assert int(g[name][k]) == int(e[name][k]) == host[k][name], (k, name)
        union = host[k]["predicted"] + host[k]["target"] - host[k]["intersection"]
        assert g["iou"][k] == e["iou"][k] == (host[k]["intersection"] / union if union else 1.0)
        # what keeps the comparison from being empty
        assert 0.05 * H * W <= whole <= 0.95 * H * W, (k, whole)
        assert host[k]["kept"] < H * W and 0 < host[k]["intersection"] < host[k]["predicted"]
    assert len(set(int(v) for v in g["predicted"])) == F, "the six frames are not distinct"
    assert all(g[name].dtype == np.int64 for name in COUNTS) and g["iou"].dtype == np.float64 and g["mean_iou"] == float(np.mean(g["iou"]))
    # the stored mask ignores keep: set pixels under the hand are in the mask and not in the count
    assert any(set_px[k] > host[k]["predicted"] for k in range(F))


def test_one_host_read_per_sweep():
    """Counted by wrapping the result read: one per sweep, of all F rows at once -- also on a second sweep through the same captured graph."""
    from egogaussian_amd.masks import MaskPass
    s = _scene()
    mp = MaskPass(_model(), s["bg"])
    calls, inner = [], mp._read_rows
    mp._read_rows = lambda rows: (calls.append(int(rows.shape[0])), inner(rows))[1]
    r1 = mp.run(s["frames"], s["cams"][0])
    graph = mp.graph
    assert calls == [F] and mp.host_reads == 1 and graph is not None
    r2 = mp.run(torch.stack(s["frames"]), s["cams"][0])
    assert calls == [F, F] and mp.host_reads == 2 and mp.graph is graph, (calls, mp.host_reads)      # no re-capture either
    assert all(np.array_equal(r1[k], r2[k]) for k in COUNTS) and torch.equal(r1["masks"], r2["masks"])


def test_overflowed_frame_is_flagged_rendered_again_and_matches_eager():
    """Captured with an instance capacity between the two largest frames' counts: exactly the largest frame is clipped on the device, comes
    back flagged, is rendered again eagerly and then carries the eager mask and counts."""
    (_, g), (_, e), _ = _sweeps()
    order = np.argsort(g["instances"])
    top, second = int(g["instances"][order[-1]]), int(g["instances"][order[-2]])
    assert top > second + 1, (top, second)
    mp, r = _pass(True, capacity=(top + second) // 2)
    print(f"instances {list(map(int, g['instances']))}, capacity {(top + second) // 2}, rendered again {r['rerendered']}")
    assert r["rerendered"] == [int(order[-1])] and mp.host_reads == 2
    assert all(np.array_equal(r[k], e[k]) for k in COUNTS) and np.array_equal(r["iou"], e["iou"])
    assert torch.equal(r["masks"], e["masks"])


def test_reallocated_model_is_refused_until_recapture():
    from egogaussian_amd.masks import MaskPass
    s = _scene()
    pc = _model()
    mp = MaskPass(pc, s["bg"])
    mp.run(s["frames"][:2], s["cams"][0])
    pc.model_version = getattr(pc, "model_version", 0) + 1                  # what CapacityGaussians.grow does after replacing the arrays
    with pytest.raises(RuntimeError, match="reallocated its arrays"):
        mp.run(s["frames"][:2], s["cams"][0])
    mp.recapture()
    assert mp.run(s["frames"][:2], s["cams"][0])["rerendered"] == []
    with pytest.raises(RuntimeError, match="no CPU path"):
        mp.run([f.cpu() for f in s["frames"][:2]], s["cams"][0])


# ---- 4. the model split -----------------------------------------------------------------------------------------------------------------------
ARRAYS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_label", "_generation", "_is_object")


def _labelled(capacity=None, n=300):
    from egogaussian_amd.scene_synth import make_scene, SynthGaussians
    from egogaussian_amd.capacity import CapacityGaussians
    scene = make_scene(n, 48, 64, 21)
    g = SynthGaussians(scene, device=DEV) if capacity is None else CapacityGaussians(scene, capacity, device=DEV)
    rows = g._label.shape[0]
    gen = torch.Generator().manual_seed(4)
    label = torch.rand(rows, 1, generator=gen) * 2 - 0.5                   # about a third above 0.5, also in the rows beyond the live count
    label[0, 0], label[1, 0] = 0.5, float(np.nextafter(np.float32(0.5), np.float32(1)))      # exactly 0.5 is background
    g._label = label.to(DEV).requires_grad_(True)
    g._generation = (torch.arange(rows, dtype=torch.int32) % 5).reshape(-1, 1).to(DEV)
    return g


def test_infer_is_object_from_label():
    from egogaussian_amd.masks import infer_is_object_from_label
    g = _labelled()
    got = infer_is_object_from_label(g)
    want = torch.where(g.get_label > 0.5, torch.ones_like(g.get_label, dtype=torch.int), torch.zeros_like(g.get_label, dtype=torch.int))
    assert got is g._is_object and got.dtype == torch.int32 and tuple(got.shape) == (300, 1) and torch.equal(got, want)
    assert int(got[0]) == 0 and int(got[1]) == 1 and 0 < int(got.sum()) < 300
    c = _labelled(capacity=512)
    c._is_object = torch.full((512, 1), 7, dtype=torch.int32, device=DEV)
    got = infer_is_object_from_label(c)
    want = torch.where(c.get_label[:300] > 0.5, 1, 0).to(torch.int32)
    assert got.dtype == torch.int32 and tuple(got.shape) == (512, 1) and torch.equal(got[:300], want)
    assert bool((got[300:] == 7).all()) and bool((c.get_label[300:] > 0.5).any()), "rows beyond the live count are untouched"
    f = _labelled(capacity=512)                                            # the float tags a fresh model carries become int32; dead rows keep their value
    assert f._is_object.dtype == torch.float32
    got = infer_is_object_from_label(f)
    assert got.dtype == torch.int32 and torch.equal(got[:300], want) and bool((got[300:] == 0).all())


@pytest.mark.parametrize("capacity", [None, 512], ids=["plain", "capacity"])
def test_split_object_background_and_ply_round_trip(capacity, tmp_path):
    from egogaussian_amd.masks import infer_is_object_from_label, split_object_background
    from egogaussian_amd.scene_synth import make_scene, SynthGaussians
    from egogaussian_amd import ply
    g = _labelled(capacity)
    infer_is_object_from_label(g)
    n = 300
    before = {a: getattr(g, a).detach().clone() for a in ARRAYS}
    obj, bgm = split_object_background(g)
    for a in ARRAYS:                                                       # the source model is unchanged
        assert torch.equal(getattr(g, a).detach(), before[a]) and getattr(g, a).shape == before[a].shape, a
    is_obj = before["_is_object"][:n].flatten()
    n_obj = int((is_obj == 1).sum())
    assert 0 < n_obj < n
    for half, sel in ((obj, is_obj == 1), (bgm, is_obj == 0)):
        for a in ARRAYS:
            got, want = getattr(half, a).detach(), before[a][:n][sel]
            assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.to(want.dtype), want), a
    assert obj._xyz.shape[0] == n_obj and bgm._xyz.shape[0] == n - n_obj
    assert bool((obj._is_object == 1).all()) and bool((bgm._is_object == 0).all())
    for name, half in (("obj", obj), ("bg", bgm)):
        path = os.path.join(str(tmp_path), f"{name}.ply")
        ply.save_ply(half, path)
        back = ply.load_ply(SynthGaussians(make_scene(1, 48, 64, 0), device=DEV), path, train_params=False, device=DEV)
        assert torch.equal(back._is_object, half._is_object.to(torch.int32)) and back._is_object.shape[0] == half._xyz.shape[0]
        assert torch.equal(back._xyz, half._xyz.detach()) and torch.equal(back._label, half._label.detach())
        assert torch.equal(back._generation, half._generation.to(torch.int32))


# ---- 5. end to end: a gated captured step fed by the gate kernel ----------------------------------------------------------------------------------
def test_gated_captured_step_with_the_kernels_gate_equals_the_uploaded_gate():
    """GraphedTrainStep(gated=True) replays on a pack_frame frame whose gate segment fused.interaction_gate(hand, predicted mask, 5, out=) wrote
    in place; its parameters and moments equal, bit for bit, those of the same step given the definition's gate (tests/mask_anchor.py gate_np,
    which returns the gate itself, 1 where the gradient passes) uploaded from the host.  On the one-wave scene of tests/test_gpu_entropy.py,
    where two runs of one step are bit-identical."""
    from egogaussian_amd import fused
    from egogaussian_amd.scene_synth import SynthGaussians
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.graph import GraphedTrainStep, pack_frame, frame_layout
    from tests.test_gpu_entropy import _one_wave_frames, _groups, _state, _differing
    student, cams, gts, bg = _one_wave_frames()
    cam, gt = cams[0], gts[0]
    Hh, Ww = gt.shape[-2:]
    hand = torch.zeros(Hh, Ww, device=DEV); hand[20:41, 30:62] = 1.0
    yy, xx = torch.meshgrid(torch.arange(Hh, device=DEV), torch.arange(Ww, device=DEV), indexing="ij")
    label_img = (3.0 - ((yy - 60.0) ** 2 + (xx - 90.0) ** 2).sqrt() / 6.0).expand(3, Hh, Ww).contiguous()       # a disc of radius 15 above 0.5
    predicted = fused.label_mask(label_img)["mask8"]
    assert predicted.dtype == torch.uint8 and 300 < int((predicted == 255).sum()) < 1200
    want_gate = MA.gate_np(hand.cpu().numpy(), predicted.cpu().numpy(), 5)
    assert 0.05 < float((want_gate == 0).mean()) < 0.5
    off, _ = frame_layout(gt.numel(), Hh * Ww, gated=True)
    ones = torch.ones(Hh, Ww, device=DEV)

    def run(how):
        pc = SynthGaussians(student, device=DEV)
        opt = FusedAdam(_groups(pc), lr=0.0, eps=1e-15, capturable=True)
        step = GraphedTrainStep(pc, opt, bg, 0.2, gated=True).capture(cam, gt, warmup=1, gate=ones)
        if how == "kernel":
            frame = pack_frame(cam, gt, gate=ones)
            seg = frame[off["gate"][0]:off["gate"][1]]
            fused.interaction_gate(hand, predicted, 5, out=seg)
            assert np.array_equal(seg.cpu().numpy().reshape(Hh, Ww), want_gate)
        elif how == "host":
            frame = pack_frame(cam, gt, gate=torch.from_numpy(want_gate).to(DEV))
        else:
            frame = pack_frame(cam, gt, gate=ones)
        for _ in range(2):
            step(frame)
        torch.cuda.synchronize()
        assert step.ok()
        return _state(pc, opt)

    kernel, host, kernel2, open_ = run("kernel"), run("host"), run("kernel"), run("ones")
    assert not _differing(kernel, kernel2), "two runs of one configuration differ: the scene does not make the step deterministic"
    assert not _differing(kernel, host), _differing(kernel, host)
    assert _differing(kernel, open_), "the gate gated nothing"
