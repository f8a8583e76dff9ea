"""GPU: the 8-bit frame store -- the decode kernel (egogaussian_amd/csrc/frames.hip through frames.FrameStore.decode) against the torch
definition FrameStore.frame, both of its paths, the ring arithmetic and the clamping; a captured step fed from the store against its twin fed
packed float frames; the evaluation and mask sweeps on a store against the same sweeps on packed frames.  Every decoded value has one right
answer: every comparison is an equality of bits, and no frame or pixel is set aside."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_frames_cpu import LAYOUTS, bits_equal, frame_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 5
# (32,128): a whole number of vector runs; (70,130): several workgroups and a tail; the small ones: segments shorter than a run, H W % 4 != 0
SHAPES = [(1, 1), (3, 5), (5, 64), (7, 65), (37, 53), (48, 64), (32, 128), (70, 130)]
RINGS = {1: ([3], [0], [F - 1]), 3: ([3, 0, 4], [2, 2, 2], [0, F - 1, 0])}      # a permutation, a repeated index, first and last frame
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _store(layout, shape):
    """-> (store of F random frames on the device, its F frames by the torch definition, the packed frames pack_frame gives on the host)"""
    from egogaussian_amd.frames import FrameStore
    H, W = shape
    lay = LAYOUTS[layout]
    store = FrameStore(H, W, F, DEV, **lay)
    wants = []
    for i in range(F):
        cam, kw, want = frame_inputs(H, W, lay, seed=1000 * H + 10 * W + i)
        store.put(i, cam, **kw)
        wants.append(want)
    return store, store.frames(), torch.stack(wants)


def _out(store, S, lead):
    """S rows and one guard row of NaN; lead = 1: a view one float into a larger tensor, whose base is not 16-byte aligned."""
    big = torch.full((lead + (S + 1) * store.frame_floats + 3,), NAN, device=DEV)
    view = big[lead:lead + (S + 1) * store.frame_floats].view(S + 1, store.frame_floats)
    assert (view.data_ptr() % 16 == 0) == (lead == 0)
    return big, view


def _untouched(big, view, S, lead):
    n = view.shape[1]
    return bool(torch.isnan(view[S]).all()) and bool(torch.isnan(big[:lead]).all()) and bool(torch.isnan(big[lead + (S + 1) * n:]).all())


# ---- 1, 2. the decode equals the definition: aligned (16-byte loads and stores) and one float off (4-byte ones) -------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", list(LAYOUTS), ids=list(LAYOUTS))
def test_decode_equals_the_definition(layout, shape):
    store, definition, packed = _store(layout, shape)
    assert bits_equal(definition.cpu(), packed), "frame(i) on the device is not pack_frame of the inputs"
    for lead in (0, 1):
        for S, rings in RINGS.items():
            for ring in rings:
                big, view = _out(store, S, lead)
                ret = store.decode(view[:S], indices=ring)
                assert ret.data_ptr() == view.data_ptr()
                want = definition[ring]
                bad = int((view[:S].view(torch.int32) != want.view(torch.int32)).sum())
                assert bad == 0, (layout, shape, lead, S, ring, bad)
                assert _untouched(big, view, S, lead), (layout, shape, lead, S, ring)
    flat = torch.full((store.frame_floats,), NAN, device=DEV)                  # a flat tensor is one row; an int is one index
    store.decode(flat, indices=1)
    assert bits_equal(flat, definition[1])
    assert store.ok()


# ---- 3. all 256 codes, both paths -------------------------------------------------------------------------------------------------------------
def test_all_256_codes_decode_exactly_on_both_paths():
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.scene_synth import make_camera
    want = (torch.arange(256, dtype=torch.uint8).float() / 255.0).to(DEV)
    product = (torch.arange(256, dtype=torch.uint8).float() * torch.tensor(1.0 / 255.0)).to(DEV)
    assert int((product.view(torch.int32) != want.view(torch.int32)).sum()) == 126
    store = FrameStore(16, 16, 1, DEV)
    codes = torch.arange(256, dtype=torch.uint8).view(1, 16, 16)
    store.put(0, make_camera(0, 16, 16), gt=torch.cat([codes, codes.flip(2), codes.flip(1)]))
    for lead in (0, 1):
        big, view = _out(store, 1, lead)
        store.decode(view[:1], indices=[0])
        img = view[0, :768].view(3, 16, 16)
        assert bits_equal(img[0].reshape(-1), want) and bits_equal(img[1].flip(1).reshape(-1), want) and bits_equal(img[2].flip(0).reshape(-1), want), lead
        assert _untouched(big, view, 1, lead)


# ---- 4. the ring: consecutive decodes walk it on the device ------------------------------------------------------------------------------------
def test_ring_arithmetic():
    store, definition, _ = _store("dynamic-motion-gated", (37, 53))
    K, S = 6, 2
    ring = store.new_ring(8)
    order = [4, 1, 3, 0, 2, 1]
    assert ring.set(order) == K
    out = torch.full((S, store.frame_floats), NAN, device=DEV)
    cursors = [int(ring.ctl[0])]
    for call in range(4):                                                 # no host write in between
        store.decode(out, ring=ring)
        lo = (call * S) % K
        assert bits_equal(out, definition[order[lo:lo + S]]), call
        cursors.append(int(ring.ctl[0]))
    assert cursors == [0, 2, 4, 0, 2] and int(ring.ctl[1]) == K
    # a cursor that does not divide the ring: rows wrap inside one call
    ring.set([0, 1, 2])
    three = torch.full((2, store.frame_floats), NAN, device=DEV)
    got = []
    for _ in range(3):
        store.decode(three, ring=ring)
        got.append((int(ring.ctl[0]), three.clone()))
    assert [c for c, _ in got] == [2, 1, 0]
    assert bits_equal(got[0][1], definition[[0, 1]]) and bits_equal(got[1][1], definition[[2, 0]]) and bits_equal(got[2][1], definition[[1, 2]])
    assert store.ring.data_ptr() != ring.ring.data_ptr() and store.ok()


# ---- 5. indices out of range are clamped and counted ------------------------------------------------------------------------------------------
def test_out_of_range_indices_are_clamped_and_counted():
    """The kernel's defined behaviour for a ring the host did not check (a device tensor): index -1 decodes frame 0, index F frame F - 1,
    the sticky status word counts both, nothing outside the rows is written."""
    from egogaussian_amd.frames import FrameStore
    _, _, packed = _store("object-loss", (37, 53))
    store = FrameStore.from_packed(packed.to(DEV), 37, 53, **LAYOUTS["object-loss"])      # (its own status word)
    definition = store.frames()
    assert bits_equal(definition.cpu(), packed)
    for lead in (0, 1):
        big, view = _out(store, 2, lead)
        store.decode(view[:2], indices=torch.tensor([-1, F], dtype=torch.int32, device=DEV))
        assert bits_equal(view[:2], definition[[0, F - 1]]) and _untouched(big, view, 2, lead)
        assert int(store.status) == 2 * (lead + 1) and not store.ok()
    store.decode(view[:2], indices=[1, 2])                                # sticky: a good call leaves the count
    assert int(store.status) == 4 and bits_equal(view[:2], definition[[1, 2]])
    with pytest.raises(IndexError):
        store.decode(view[:2], indices=[0, F])
    with pytest.raises(ValueError):
        store.decode(view[:2], indices=[0, 1, 2])
    with pytest.raises(RuntimeError):
        store.decode(torch.empty(7, device=DEV))


# ---- 6. a captured step on the store equals the same step on packed float frames ---------------------------------------------------------------
N_TARGET = 2000
ORDER = (3, 0, 5, 1, 4, 2)                                               # six replays of one frame, three of two, in this order
W_OBJ = dict(lambda_image=0.7, lambda_l1_alpha=0.3, lambda_l2_alpha=0.2)
STATE = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_label")
STATS = ("max_radii2D", "xyz_gradient_accum", "denom")


@functools.lru_cache(maxsize=None)
def _grid_scene(H, W):
    """About 2 000 Gaussians of scene_synth.make_scene (seeded), re-seated as tests/test_gpu_entropy.py _one_wave_scene does: each on the
    centre of an 8x8 pixel quadrant with a footprint of 0.5 px, so that exactly one wave of the backward blend adds to its accumulator line
    and a step has no order of float atomics to vary -- two runs of one step are then bit-identical (asserted below), and equality between
    two differently fed steps is a statement about the feeding.  Six frames of one camera: images (the teacher's render plus noise, quantised
    to 8 bits once), gates, object masks and accumulated rotations of their own.
    -> dict(student, cam, bg, gt8[6], gates[6], masks[6], Rs[6], is_object)"""
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_scene, make_camera, SynthGaussians, Pipe
    seed = 5
    cam = make_camera(0, H, W, device=DEV)
    qy, qx = H // 8, W // 8
    per = max(1, round(N_TARGET / (qy * qx)))
    n = qy * qx * per
    sc = make_scene(n, H, W, seed)
    rng = np.random.default_rng(seed)
    z = rng.uniform(3.0, 8.0, n)
    px = np.tile(np.arange(qx) * 8 + 3.5, qy * per)
    py = np.tile(np.repeat(np.arange(qy) * 8 + 3.5, qx), per)
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    view = np.stack([((2 * px + 1) / W - 1) * tx * z, ((2 * py + 1) / H - 1) * ty * z, z, np.ones(n)], 1)
    sc["xyz"] = (view @ np.linalg.inv(cam.world_view_transform.cpu().double().numpy()))[:, :3].astype(np.float32)
    sc["log_scale"] = np.repeat(np.log(0.5 * z / (W / (2 * tx)))[:, None], 3, 1).astype(np.float32)
    student = {k: v.copy() for k, v in sc.items()}
    student["features"] += rng.normal(0, 0.2, student["features"].shape).astype(np.float32)
    student["opacity_logit"] += rng.normal(0, 0.5, student["opacity_logit"].shape).astype(np.float32)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        out = render(cam, SynthGaussians(sc, device=DEV, requires_grad=False), Pipe, bg)
    assert int((out["radii"] > 0).sum()) > 0.9 * n and int(out["radii"].max()) <= 3, "the scene is not the one-wave scene it is meant to be"
    gen = torch.Generator().manual_seed(seed)
    gt8, gates, masks, Rs = [], [], [], []
    for k in range(6):
        noisy = (out["render"].cpu() + 0.05 * torch.randn(3, H, W, generator=gen)).clamp(0, 1)
        gt8.append(torch.round(noisy * 255.0).to(torch.uint8).to(DEV))
        gates.append((torch.rand(H, W, generator=gen) < 0.85).float().to(DEV))
        m = torch.zeros(H, W); m[2 + k:H - 6 + k, 3 + 2 * k:W - 14 + 2 * k] = 1.0
        masks.append(m.to(DEV))
        a = 0.1 + 0.15 * k
        Rs.append(torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], device=DEV))
    is_object = (torch.rand(n, 1, generator=gen) < 0.5).float().to(DEV)
    return dict(student=student, cam=cam, bg=bg, gt8=gt8, gates=gates, masks=masks, Rs=Rs, is_object=is_object, n=n)


CONFIGS = {"static-gated": (dict(gated=True, densify_stats=True), dict(gated=True)),
           "object-loss": (dict(dynamic=True, motion=True, gated=True, object_loss=W_OBJ), dict(dynamic=True, motion=True, gated=True, object_loss=True)),
           "label-phase": (dict(label_phase=True, gated=True), dict(label_phase=True, gated=True))}


@functools.lru_cache(maxsize=None)
def _step_store(config, shape):
    from egogaussian_amd.frames import FrameStore
    H, W = shape
    s = _grid_scene(H, W)
    lay = CONFIGS[config][1]
    store = FrameStore(H, W, 6, DEV, **lay)
    eye34 = torch.eye(4, device=DEV)[:3]                                  # the object stays where the scene puts it (see _grid_scene)
    for k in range(6):
        if lay.get("label_phase"):
            store.put(k, s["cam"], gate=s["gates"][k], obj_mask=s["masks"][k])
        elif lay.get("object_loss"):
            store.put(k, s["cam"], gt=s["gt8"][k], accum_R=s["Rs"][k], accum_T=eye34, gate=s["gates"][k], obj_mask=s["masks"][k])
        else:
            store.put(k, s["cam"], gt=s["gt8"][k], gate=s["gates"][k])
    return store, [store.frame(k) for k in range(6)]                       # the float frames are built FROM the store: both sides see the same data


def _run_step(config, shape, S, feed):
    """feed: "packed" -- capture on frame 0's tensors, replay packed float frames; "store" -- capture(cam, index=0), step(indices);
    "schedule" -- set_schedule(ORDER) once, then bare step() calls.  -> every parameter, both moments, the step counts, loss_sum, the statistics."""
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.scene_synth import SynthGaussians
    H, W = shape
    s = _grid_scene(H, W)
    store, floats = _step_store(config, shape)
    pc = SynthGaussians(s["student"], device=DEV)
    pc._is_object = s["is_object"]
    with torch.no_grad():
        pc._label += (torch.randn(s["n"], 1, generator=torch.Generator().manual_seed(8)) * 0.5).to(DEV)
    opt = pc.training_setup(FusedAdam, capturable=True)
    for g in opt.param_groups:
        if g["name"] == "label":
            g["lr"] = 1e-2
    kw = dict(CONFIGS[config][0])
    parts = store.parts(0)
    if feed == "packed":
        step = GraphedTrainStep(pc, opt, s["bg"], 0.2, steps_per_replay=S, **kw)
        if kw.get("label_phase"):
            step.capture(s["cam"], obj_mask=parts["obj_mask"], gate=parts["gate"], warmup=1, capacity_margin=2.0)
        else:
            step.capture(s["cam"], parts["gt"], warmup=1, capacity_margin=2.0, accum_R=parts["accum_R"], gate=parts["gate"], accum_T=parts["accum_T"],
                         obj_mask=parts["obj_mask"])
    else:
        step = GraphedTrainStep(pc, opt, s["bg"], 0.2, steps_per_replay=S, frame_store=store, ring_capacity=16, **kw).capture(
            s["cam"], index=0, warmup=1, capacity_margin=2.0)
    if feed == "schedule":
        step.set_schedule(list(ORDER))
    for lo in range(0, 6, S):
        idx = list(ORDER[lo:lo + S])
        if feed == "packed":
            step(floats[idx[0]] if S == 1 else torch.stack([floats[i] for i in idx]))
        elif feed == "store":
            step(idx[0] if S == 1 and lo == 0 else idx)                  # an int, or a sequence
        else:
            step()
    torch.cuda.synchronize()
    assert step.ok()
    if feed != "packed":
        assert step.store_ok()
    state = {"loss_sum": step.loss_sum.detach().clone().reshape(1)}
    for a in STATE:
        p = getattr(pc, a)
        state[a] = p.detach().clone()
        for key in ("exp_avg", "exp_avg_sq", "step"):
            if p in opt.state and key in opt.state[p]:
                state[a + "." + key] = opt.state[p][key].detach().clone().reshape(-1).float()
    for a in STATS:
        state[a] = getattr(pc, a).detach().clone()
    return state


def _differing(a, b):
    assert set(a) == set(b)
    return {k: int((a[k].contiguous().view(torch.int32) != b[k].contiguous().view(torch.int32)).sum()) for k in a if not bits_equal(a[k].float(), b[k].float())}


@pytest.mark.parametrize("S", [1, 2], ids=["one-per-replay", "two-per-replay"])
@pytest.mark.parametrize("shape", [(48, 64), (37, 53)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("config", list(CONFIGS), ids=list(CONFIGS))
def test_step_on_the_store_equals_the_step_on_packed_frames(config, shape, S):
    packed = _run_step(config, shape, S, "packed")
    again = _run_step(config, shape, S, "packed")
    assert not _differing(packed, again), "two runs of the packed-frame step differ: the scene does not make the step deterministic"
    fresh = _grid_scene(*shape)["student"]
    moved = "_label" if config == "label-phase" else "_opacity"
    if moved == "_opacity":
        assert not torch.equal(packed[moved].cpu().reshape(-1), torch.tensor(fresh["opacity_logit"]).reshape(-1)), "nothing was trained"
    else:
        assert float(packed["_label.exp_avg"].abs().max()) > 0, "nothing was trained"
    assert float(packed[moved + ".step"][0]) == 7.0                       # one warm-up step and six replayed ones
    stored = _run_step(config, shape, S, "store")
    diff = _differing(packed, stored)
    assert not diff, (config, shape, S, "step(indices)", diff)
    scheduled = _run_step(config, shape, S, "schedule")
    diff = _differing(packed, scheduled)
    assert not diff, (config, shape, S, "set_schedule", diff)


def test_step_on_the_store_checks_its_indices_on_the_host():
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.optim import FusedAdam
    from egogaussian_amd.scene_synth import SynthGaussians, make_camera
    shape = (37, 53)
    s = _grid_scene(*shape)
    store, _ = _step_store("static-gated", shape)
    pc = SynthGaussians(s["student"], device=DEV)
    opt = pc.training_setup(FusedAdam, capturable=True)
    step = GraphedTrainStep(pc, opt, s["bg"], 0.2, gated=True, steps_per_replay=2, frame_store=store, ring_capacity=4)
    with pytest.raises(ValueError):
        step.capture(make_camera(0, 48, 64, device=DEV), index=0)         # another image size
    with pytest.raises(ValueError):
        step.capture(s["cam"], s["gt8"][0].float() / 255.0, index=0)       # the contents come from the store
    step.capture(s["cam"], index=2, warmup=1, capacity_margin=2.0)
    with pytest.raises(ValueError):
        step()                                                            # no indices yet
    for bad in ([0, 6], [-1, 0]):
        with pytest.raises(IndexError):
            step(bad)
        with pytest.raises(IndexError):
            step.set_schedule(bad)
    for bad in ([0], [0, 1, 2], 3):                                       # not S of them; an int for S = 2
        with pytest.raises(ValueError):
            step(bad)
    for bad in ([0, 1, 2], [0, 1, 2, 3, 4, 5], []):                       # not a multiple of S; beyond the ring's capacity; none
        with pytest.raises(ValueError):
            step.set_schedule(bad)
    step(torch.tensor([1, 3], dtype=torch.int32, device=DEV))             # a device tensor goes as it is
    step.set_schedule([0, 1, 2, 3])
    step(); step(); step()
    torch.cuda.synchronize()
    assert step.ok() and step.store_ok() and int(step._ring.ctl[0]) == 2 and int(step._ring.ctl[1]) == 4
    assert float(opt.state[pc._xyz]["step"]) == 1 + 2 * 4


# ---- 7. the evaluation and mask sweeps on a store --------------------------------------------------------------------------------------------
SWEEP_SHAPE, SWEEP_F = (37, 53), 5


@functools.lru_cache(maxsize=None)
def _sweep_scene():
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.renderer import render
    from egogaussian_amd.scene_synth import make_scene, make_camera, SynthGaussians, Pipe
    H, W = SWEEP_SHAPE
    scene = make_scene(2000, H, W, 3); scene["log_scale"] += math.log(3.0)
    x = scene["xyz"][:, 0]
    label = np.where(x < np.quantile(x, 0.3), 2.0, -2.0).astype(np.float32)[:, None]
    bg = torch.zeros(3, device=DEV)
    cams = [make_camera(k, H, W, device=DEV) for k in (20, 60, 110, 160, 210)]
    gen = torch.Generator().manual_seed(11)
    images = FrameStore(H, W, SWEEP_F, DEV, gated=True)
    labels = FrameStore(H, W, SWEEP_F, DEV, label_phase=True, gated=True)
    pc = SynthGaussians(scene, device=DEV, requires_grad=False)
    for k in range(SWEEP_F):
        keep = torch.ones(H, W, device=DEV); keep[3 + k:12 + 2 * k, 5 + k:20 + 3 * k] = 0.0
        obj = torch.zeros(H, W, device=DEV); obj[4 + k:25 + k, 0:18 + 2 * k] = 1.0
        with torch.no_grad():
            img = render(cams[k], pc, Pipe, bg)["render"].cpu()
        noisy = (img + 0.03 * torch.randn(3, H, W, generator=gen)).clamp(0, 1)
        images.put(k, cams[k], gt=noisy, gate=keep, quantize=True)
        labels.put(k, cams[k], gate=keep, obj_mask=obj)
    return dict(scene=scene, label=label, bg=bg, cams=cams, images=images, labels=labels)


def _sweep_model():
    from egogaussian_amd.scene_synth import SynthGaussians
    s = _sweep_scene()
    pc = SynthGaussians(s["scene"], device=DEV, requires_grad=False)
    pc._label = torch.from_numpy(s["label"]).to(DEV)
    return pc


def _f64_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_evaluation_sweep_on_a_store_equals_the_sweep_on_packed_frames(graphed):
    from egogaussian_amd.evaluate import EvalPass
    s = _sweep_scene()
    store = s["images"]
    packed = store.frames()
    res = {}
    for name, frames in (("packed", packed), ("store", store), ("list", [store.frame(i) for i in range(SWEEP_F)])):
        ep = EvalPass(_sweep_model(), s["bg"], graphed=graphed, keep_images=True)
        res[name] = ep.run(frames, s["cams"][0])
        assert ep.host_reads == 1 and res[name]["rerendered"] == []
    a = res["packed"]
    assert a["sse"].dtype == np.int64 and (a["sse"] > 0).all() and len(set(a["sse"].tolist())) == SWEEP_F
    for name in ("store", "list"):
        b = res[name]
        assert np.array_equal(a["sse"], b["sse"]) and np.array_equal(_f64_bits(a["ssim"]), _f64_bits(b["ssim"])), name
        assert np.array_equal(_f64_bits(a["psnr"]), _f64_bits(b["psnr"])) and np.array_equal(a["instances"], b["instances"])
        assert torch.equal(a["images"], b["images"])
    if graphed:                                                           # a capacity between the two largest frames: one frame is rendered again
        order = np.argsort(a["instances"])
        top, second = int(a["instances"][order[-1]]), int(a["instances"][order[-2]])
        assert top > second + 1, (top, second)
        small = {}
        for name, frames in (("packed", packed), ("store", store)):
            ep = EvalPass(_sweep_model(), s["bg"], keep_images=True)
            small[name] = ep.run(frames, s["cams"][0], capacity=(top + second) // 2)
            assert small[name]["rerendered"] == [int(order[-1])] and ep.host_reads == 2
        for r in small.values():
            assert np.array_equal(r["sse"], a["sse"]) and np.array_equal(_f64_bits(r["ssim"]), _f64_bits(a["ssim"])) and torch.equal(r["images"], a["images"])
    assert store.ok()


@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_mask_sweep_on_a_store_equals_the_sweep_on_packed_frames(graphed):
    from egogaussian_amd.masks import MaskPass
    s = _sweep_scene()
    store = s["labels"]
    packed = store.frames()
    counts = ("predicted", "target", "intersection", "kept")
    res = {}
    for name, frames in (("packed", packed), ("store", store)):
        mp = MaskPass(_sweep_model(), s["bg"], graphed=graphed)
        res[name] = mp.run(frames, s["cams"][0])
        assert mp.host_reads == 1 and res[name]["rerendered"] == []
    a, b = res["packed"], res["store"]
    assert all(np.array_equal(a[k], b[k]) for k in counts) and torch.equal(a["masks"], b["masks"]) and np.array_equal(a["instances"], b["instances"])
    assert (a["predicted"] > 0).all() and (a["kept"] < SWEEP_SHAPE[0] * SWEEP_SHAPE[1]).all() and (a["intersection"] > 0).all()
    assert len(set(a["predicted"].tolist())) == SWEEP_F, "the frames are not distinct"
    if graphed:
        order = np.argsort(a["instances"])
        top, second = int(a["instances"][order[-1]]), int(a["instances"][order[-2]])
        assert top > second + 1, (top, second)
        for frames in (packed, store):
            mp = MaskPass(_sweep_model(), s["bg"])
            r = mp.run(frames, s["cams"][0], capacity=(top + second) // 2)
            assert r["rerendered"] == [int(order[-1])] and mp.host_reads == 2
            assert all(np.array_equal(r[k], a[k]) for k in counts) and torch.equal(r["masks"], a["masks"])
    assert store.ok()
