"""GPU: frame ingest -- the kernel (egogaussian_amd/csrc/ingest.hip through ingest.FrameIngest) against the torch statement
ingest.resize_u8 / binarize on every case of tests/golden/ingest.npz and all three plane kinds; a store filled by FrameIngest.put from the
recorded SOURCES against a store filled by FrameStore.put from the recorded REFERENCE OUTPUTS, in six layouts; neighbouring frames, padding
and re-ingest; one run at the workload's shape.  The definition is integer arithmetic: every comparison is an equality of bits.  Neither the
reference nor Pillow is imported here."""
import numpy as np
import pytest
import torch

from tests.test_ingest_cpu import cases, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = golden()
CASES = cases(G)
IDS = [f"{h}x{w}-to-{W}x{H}" for _, (h, w), (W, H) in CASES]
LAYOUTS = {"plain": dict(),
           "gated": dict(gated=True),
           "dynamic-motion-gated": dict(dynamic=True, motion=True, gated=True),
           "object-loss": dict(dynamic=True, motion=True, gated=True, object_loss=True),
           "label-gated": dict(label_phase=True, gated=True),
           "pose-rows": dict(dynamic=True, motion=True, gated=True, pose_rows=True)}


def _chw(hwc):
    """uint8 [H, W, 3] -> the store's flat CHW bytes"""
    return torch.as_tensor(hwc).permute(2, 0, 1).reshape(-1)


def _words(bits, store):
    from egogaussian_amd.frames import _pack_bits
    return _pack_bits(bits.reshape(-1).to(DEV), store.plane_words)


# ---- 1. kernel against statement: every case, every plane kind --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_equals_the_statement(case):
    from egogaussian_amd import ingest
    from egogaussian_amd.frames import FrameStore
    k, (h, w), (W, H) = case
    image = FrameStore(H, W, 2, DEV, gated=True)                       # image without the object plane's product, and the gate
    label = FrameStore(H, W, 2, DEV, label_phase=True, gated=True)     # both planes
    ing_i, ing_l = ingest.FrameIngest(image, (h, w)), ingest.FrameIngest(label, (h, w))
    src = G[f"img_{k}"]
    ing_i.plane(1, "image", src)
    want = _chw(ingest.resize_u8(torch.from_numpy(src).to(DEV), (W, H)))
    assert torch.equal(image.img[1, :image.n_img], want), (k, "image", int((image.img[1, :image.n_img] != want).sum()))
    assert torch.equal(want.cpu(), _chw(G[f"img_out_{k}"])), "the statement on the device is not the reference's bytes"
    for name in ("mask_l", "mask_rgb"):
        m = G[f"{name}_{k}"]
        bits = ingest.binarize(ingest.resize_u8(torch.from_numpy(m).to(DEV), (W, H)))
        assert torch.equal(bits.cpu(), torch.from_numpy(G[f"{name}_bin_{k}"]).bool())
        ing_l.plane(1, "hand_mask", m)
        ing_l.plane(1, "obj_mask", m)
        gate, obj = label.bits[1, 0], label.bits[1, 1]
        assert torch.equal(gate, _words(~bits, label)), (k, name, "gate")
        assert torch.equal(obj, _words(bits, label)), (k, name, "obj_mask")
    assert not bool(image.img[0].any()) and not bool(label.bits[0].any()) and not bool(image.bits.any())      # frame 0 and the unused plane: untouched


# ---- 2. the same store as put() -----------------------------------------------------------------------------------------------------------------
def _frame_args(k, lay, seed):
    """-> (cam, FrameStore.put keywords from the reference's recorded outputs, FrameIngest.put keywords from the recorded sources)"""
    from egogaussian_amd.scene_synth import make_camera
    _, (h, w), (W, H) = CASES[k]
    g = torch.Generator().manual_seed(seed)
    cam = make_camera(seed % 300, H, W)
    put, ing = {}, {}
    if not lay.get("label_phase"):
        put["gt"] = torch.from_numpy(G[f"img_out_{k}"]).permute(2, 0, 1).contiguous()
        ing["image"] = G[f"img_{k}"]
    if lay.get("gated"):
        put["gate"] = 1.0 - torch.from_numpy(G[f"mask_l_bin_{k}"]).float()
        ing["hand_mask"] = G[f"mask_l_{k}"]
    if lay.get("object_loss") or lay.get("label_phase"):
        put["obj_mask"] = torch.from_numpy(G[f"mask_rgb_bin_{k}"]).float()
        ing["obj_mask"] = G[f"mask_rgb_{k}"]
    both = {}
    if lay.get("dynamic"):
        both["accum_R"] = torch.rand(3, 3, generator=g)
    if lay.get("motion"):
        both["accum_T"] = torch.rand(4, 4, generator=g)
    if lay.get("pose_rows"):
        both["pose_rows"] = (1, 2, 1)
    put.update(both), ing.update(both)
    return cam, put, ing


@pytest.mark.parametrize("k", [0, 1, 3], ids=[IDS[0], IDS[1], IDS[3]])
@pytest.mark.parametrize("layout", list(LAYOUTS), ids=list(LAYOUTS))
def test_same_store_as_put(layout, k):
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    lay = LAYOUTS[layout]
    _, (h, w), (W, H) = CASES[k]
    a, b = FrameStore(H, W, 2, DEV, **lay), FrameStore(H, W, 2, DEV, **lay)
    ing = FrameIngest(b, (h, w))
    for i in (1, 0):
        cam, put, src = _frame_args(k, lay, seed=10 * k + i)
        if i == 0:                                                     # the second frame from device arrays, the first from host arrays
            src = {n: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for n, v in src.items()}
        a.put(i, cam, **put)
        ing.put(i, cam, **src)
    for name in ("img", "bits", "small"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), (layout, k, name)
    assert torch.equal(a.frames().view(torch.int32), b.frames().view(torch.int32))
    out_a, out_b = torch.empty((2, a.frame_floats), device=DEV), torch.empty((2, b.frame_floats), device=DEV)
    a.decode(out_a, indices=[1, 0]); b.decode(out_b, indices=[1, 0])
    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)) and torch.equal(out_a.view(torch.int32), a.frames([1, 0]).view(torch.int32))


def test_put_asks_what_the_layout_has():
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    _, (h, w), (W, H) = CASES[1]
    store = FrameStore(H, W, 1, DEV, gated=True)
    ing = FrameIngest(store, (h, w))
    cam, _, src = _frame_args(1, dict(gated=True), 3)
    with pytest.raises(ValueError, match="FrameIngest.put: this store's layout needs hand_mask"):
        ing.put(0, cam, image=src["image"])
    with pytest.raises(ValueError, match="FrameIngest.put: this store's layout has no obj_mask"):
        ing.put(0, cam, obj_mask=src["hand_mask"], **src)
    with pytest.raises(ValueError, match="premultiplies alpha"):
        ing.put(0, cam, image=np.zeros((h, w, 4), np.uint8), hand_mask=src["hand_mask"])
    with pytest.raises(IndexError):
        ing.put(1, cam, **src)
    assert not bool(store.img.any()) and not bool(store.bits.any()) and not bool(store.small.any())      # a refused put writes nothing


# ---- 3. neighbouring frames, padding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4], ids=[IDS[1], IDS[4]])
def test_neighbouring_frames_and_padding_stay(k):
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    lay = LAYOUTS["object-loss"]
    _, (h, w), (W, H) = CASES[k]
    store = FrameStore(H, W, 3, DEV, **lay)
    assert store.image_stride > store.n_img or k != 1                  # 41 x 29: one padding byte, and 1189 % 32 != 0
    g = torch.Generator().manual_seed(5)
    for i in (0, 2):
        store.img[i] = torch.randint(0, 256, (store.image_stride,), generator=g, dtype=torch.uint8).to(DEV)
        store.bits[i] = torch.randint(-2**31, 2**31 - 1, tuple(store.bits[i].shape), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
        store.small[i] = torch.rand(store.small_floats, generator=g).to(DEV)
    before = [t.clone() for t in (store.img, store.bits, store.small)]
    cam, _, src = _frame_args(k, lay, 9)
    src["hand_mask"] = np.zeros_like(src["hand_mask"])                 # the gate is then all ones: every bit up to H W is set, none beyond
    FrameIngest(store, (h, w)).put(1, cam, **src)
    for t, was in zip((store.img, store.bits, store.small), before):
        assert torch.equal(t[0], was[0]) and torch.equal(t[2], was[2])
    assert not bool(store.img[1, store.n_img:].any())
    n = store.n_pix
    for p in range(2):
        words = store.bits[1, p].cpu().numpy().view(np.uint32)
        unpacked = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)
        assert not unpacked[n:].any(), p
        if p == 0:
            assert unpacked[:n].all()


# ---- 4. re-ingest ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 0], ids=[IDS[1], IDS[0]])
def test_reingest_leaves_nothing_behind(k):
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    lay = LAYOUTS["object-loss"]
    _, (h, w), (W, H) = CASES[k]
    used, fresh = FrameStore(H, W, 1, DEV, **lay), FrameStore(H, W, 1, DEV, **lay)
    cam, _, src = _frame_args(k, lay, 4)
    first = dict(src, image=np.full((h, w, 3), 255, np.uint8), hand_mask=np.zeros((h, w), np.uint8), obj_mask=np.full((h, w, 3), 255, np.uint8))
    ing = FrameIngest(used, (h, w))
    ing.put(0, cam, **first)
    assert bool((used.bits[0, 0] != 0).any()) and bool((used.bits[0, 1] != 0).any()) and bool((used.img[0, :used.n_img] == 255).all())
    ing.put(0, cam, **src)
    FrameIngest(fresh, (h, w)).put(0, cam, **src)
    for name in ("img", "bits", "small"):
        assert torch.equal(getattr(used, name), getattr(fresh, name)), name


# ---- 5. the workload's shape -------------------------------------------------------------------------------------------------------------------------
def test_workload_shape_1080p_to_1600x900():
    from egogaussian_amd import ingest
    from egogaussian_amd.frames import FrameStore
    h, w = 1080, 1920
    W, H = ingest.target_size(w, h)
    assert (W, H) == (1600, 900)
    g = torch.Generator().manual_seed(11)
    image = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    blocks = lambda c, p: (torch.rand((h // 8, w // 8, c), generator=g) < p).repeat_interleave(8, 0).repeat_interleave(8, 1)
    hand = (blocks(1, 0.3) * torch.randint(1, 256, (h, w, 1), generator=g, dtype=torch.uint8)).contiguous()
    obj = (blocks(3, 0.2) * torch.randint(1, 256, (h, w, 3), generator=g, dtype=torch.uint8)).contiguous()
    store = FrameStore(H, W, 2, DEV, gated=True, object_loss=True)
    from egogaussian_amd.scene_synth import make_camera
    ingest.FrameIngest(store, (h, w)).put(1, make_camera(0, H, W), image=image.pin_memory(), hand_mask=hand, obj_mask=obj.to(DEV))
    r_img = ingest.resize_u8(image.to(DEV), (W, H))
    b_hand = ingest.binarize(ingest.resize_u8(hand.to(DEV), (W, H)))
    b_obj = ingest.binarize(ingest.resize_u8(obj.to(DEV), (W, H)))
    assert 0.1 < float(b_hand.float().mean()) < 0.9 and 0.1 < float(b_obj.float().mean()) < 0.9
    assert torch.equal(store.bits[1, 0], _words(~b_hand, store)) and torch.equal(store.bits[1, 1], _words(b_obj, store))
    want = _chw(r_img * b_obj.unsqueeze(-1).to(torch.uint8))
    assert torch.equal(store.img[1, :store.n_img], want), int((store.img[1, :store.n_img] != want).sum())
    assert not bool(store.img[0].any()) and not bool(store.bits[0].any()) and not bool(store.img[1, store.n_img:].any())
