"""GPU: densify.DeviceDensify (egs_densify_plan_dev / egs_prune_plan_dev / egs_densify_apply: plan and in-place apply with every count
on the device) against the host-driven densify.densify_and_prune / prune_points on an identical capacity-sized model -- torch.equal
over all `capacity` rows of every parameter, both moments of every group, the three statistics, both tags, and the count."""
import math

import numpy as np
import pytest
import torch

from tests import bookkeeping_cases as B
from tests import device_densify_cases as K
from tests.test_gpu_capacity import CapModel, _scene
from tests.test_gpu_densify import ATTR, DEV

pytestmark = pytest.mark.gpu


def _kw(kw):
    kw = dict(kw)
    return kw.pop("percent_dense"), kw


def _full(m):
    """Every array of the model over all capacity rows, and the device count."""
    st = m.state()
    st["active_count"] = m.active_count.cpu()
    return st


def _pair(live, capacity, percent_dense):
    return CapModel(live, capacity, percent_dense, "fused"), CapModel(live, capacity, percent_dense, "fused")


def _load(m, live, n_live):
    """New contents for the same arrays: the live state in rows [0, n_live), junk beyond."""
    padded = K.pad_state(live, m.capacity)
    with torch.no_grad():
        for k, a in ATTR.items():
            p = getattr(m, a)
            p.copy_(padded[k].to(DEV))
            m.optimizer.state[p]["exp_avg"].copy_(padded[k + "_exp_avg"].to(DEV))
            m.optimizer.state[p]["exp_avg_sq"].copy_(padded[k + "_exp_avg_sq"].to(DEV))
        m._generation.copy_(padded["generation"].to(DEV)); m._is_object.copy_(padded["is_object"].to(DEV))
        for k in K.STATS:
            getattr(m, k).copy_(padded[k].to(DEV))
    m.set_active(n_live)


def _densify_parity(inp, kw, capacity, z, what):
    from egogaussian_amd import densify
    pd, kw = _kw(kw)
    n_old = inp["accum"].shape[0]
    live = K.live_state(inp)
    host, dev = _pair(live, capacity, pd)
    before = _full(dev)
    _, n_new = K.reference_plan(inp, dict(kw, percent_dense=pd))
    dd = densify.DeviceDensify(dev, z=z)
    dd.enqueue(**kw)
    report = dd.check()
    if n_new > capacity:                                           # the host-driven call would grow(): here nothing may change
        assert report == dict(refusals=1, rows_needed=n_new, applications=0, n_new=0, refused_since_last_check=True), f"{what}: {report}"
        K.assert_states_equal(_full(dev), before, what + " (refused)")
        return n_new
    assert densify.densify_and_prune(host, z=lambda rows: z[:rows], **kw) == (n_old, n_new), what
    assert report == dict(refusals=0, rows_needed=0, applications=1, n_new=n_new, refused_since_last_check=False), f"{what}: {report}"
    K.assert_states_equal(_full(dev), _full(host), what)
    return n_new


@pytest.mark.parametrize("n_live", K.LIVE_COUNTS)
def test_enqueue_matches_host_driven_densify_and_prune(n_live):
    """Every rule set of bookkeeping_cases.py at live counts 1, 257 (two workgroups), 2049 and 4100 (one and two scan blocks crossed) in
    a capacity of 4100; at 257 also the edge model, whose named rows sit on the rule thresholds."""
    z = K.draws(K.CAPACITY).to(DEV)
    inp = K.live_inputs(n_live)
    fits = [_densify_parity(inp, kw, K.CAPACITY, z, f"{name} n={n_live}") <= K.CAPACITY for name, kw in K.rule_sets()]
    assert any(fits) and (not all(fits)) == (n_live == K.CAPACITY)
    if n_live == B.EDGE_P:
        edge = B.edge_model()
        for name, kw in B.EDGE_SCENARIOS.items():
            _densify_parity(edge, dict(kw), K.CAPACITY, z, f"edge model {name}")
    _densify_parity(inp, dict(K.NOTHING_SELECTED), K.CAPACITY, z, f"nothing selected n={n_live}")
    assert _densify_parity(inp, dict(K.NOTHING_SELECTED, min_opacity=2.0), K.CAPACITY, z, f"everything pruned n={n_live}") == 0


@pytest.mark.parametrize("n_live", K.LIVE_COUNTS)
def test_enqueue_prune_matches_host_driven_prune_points(n_live):
    """prune_points through egs_prune_plan_dev: nothing kept, everything kept, a block-dependent density, the last row only; the mask
    given over the capacity (junk True beyond the live count) and, for one pattern, over the live rows only."""
    from egogaussian_amd import densify
    inp = K.live_inputs(n_live)
    live = K.live_state(inp)
    for pattern in ("none", "all", "block_density", "last"):
        keep = B.keep_mask(np.arange(n_live), n_live, pattern)
        mask = torch.ones(K.CAPACITY, dtype=torch.bool)
        mask[:n_live] = torch.from_numpy(~np.asarray(keep, bool))
        host, dev = _pair(live, K.CAPACITY, 0.01)
        n_new = int(keep.sum())
        assert densify.prune_points(host, mask.to(DEV)) == (n_live, n_new)
        dd = densify.DeviceDensify(dev)
        dd.enqueue_prune(mask.to(DEV) if pattern != "block_density" else mask[:n_live].to(DEV))
        assert dd.check() == dict(refusals=0, rows_needed=0, applications=1, n_new=n_new, refused_since_last_check=False)
        K.assert_states_equal(_full(dev), _full(host), f"prune {pattern} n={n_live}")


def test_exact_fit_is_accepted():
    inp = K.live_inputs(2049)
    _, n_new = K.reference_plan(inp, dict(K.GROWING))
    assert n_new > 2049
    assert _densify_parity(inp, dict(K.GROWING), n_new, K.draws(n_new).to(DEV), "n_new == capacity") == n_new


def test_refusal_in_place_then_grow():
    """A capacity one row short of n_new: everything bit-identical to before, check() reports the refusal and the rows needed (once);
    after grow() the old object refuses to run, and a new one does what the host-driven call does."""
    from egogaussian_amd import densify
    from egogaussian_amd.capacity import CapacityGaussians
    n = 2049
    inp = K.live_inputs(n)
    pd, kw = _kw(K.GROWING)
    _, n_new = K.reference_plan(inp, dict(K.GROWING))
    live = K.live_state(inp)
    scene = dict(xyz=live["xyz"].numpy(), log_scale=live["scaling"].numpy(), quat=live["rotation"].numpy(), opacity_logit=live["opacity"].numpy(),
                 features=torch.cat([live["f_dc"], live["f_rest"]], 1).numpy())

    def model(capacity):
        pc = CapacityGaussians(scene, capacity, device=DEV)
        pc.training_setup(percent_dense=pd)
        with torch.no_grad():
            for k in ("xyz_gradient_accum", "denom", "max_radii2D", "generation", "is_object"):
                t = getattr(pc, k if k in K.STATS else "_" + k)
                t[:n] = live[k].to(DEV).to(t.dtype).view(t[:n].shape)
            g = torch.Generator().manual_seed(9)
            for grp in pc.optimizer.param_groups:
                p = grp["params"][0]
                pc.optimizer.state[p] = {"step": torch.tensor(2.0), "exp_avg": torch.randn(p.shape, generator=g).to(DEV),
                                         "exp_avg_sq": torch.rand(p.shape, generator=g).to(DEV)}
        return pc

    def full(pc):
        out = {k: getattr(pc, a).detach().clone() for k, a in ATTR.items()}
        for k, a in ATTR.items():
            st = pc.optimizer.state[getattr(pc, a)]
            out[k + "_exp_avg"], out[k + "_exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        out.update(generation=pc._generation.clone(), is_object=pc._is_object.clone(), active_count=pc.active_count.clone())
        out.update({k: getattr(pc, k).clone() for k in K.STATS})
        return out

    pc = model(n_new - 1)
    assert pc._is_object.dtype == torch.float32                   # the float tag of the models here is read as it is
    z = K.draws(n_new - 1).to(DEV)
    before = full(pc)
    dd = densify.DeviceDensify(pc, z=z)
    dd.enqueue(**kw)
    report = dd.check()
    assert report == dict(refusals=1, rows_needed=n_new, applications=0, n_new=0, refused_since_last_check=True), report
    assert dd.check()["refused_since_last_check"] is False and pc.n_active == n
    K.assert_states_equal(full(pc), before, "refused in place")
    pc.grow(n_new + 100)
    with pytest.raises(RuntimeError, match="new DeviceDensify"):
        dd.enqueue(**kw)
    z2 = torch.cat([z, torch.zeros(2 * (pc.capacity - (n_new - 1)), 3, device=DEV)])
    host = model(n_new - 1)
    host.grow(n_new + 100)
    assert densify.densify_and_prune(host, z=lambda rows: z2[:rows], **kw) == (n, n_new)
    dd = densify.DeviceDensify(pc, z=z2)
    dd.enqueue(**kw)
    assert dd.check() == dict(refusals=0, rows_needed=0, applications=1, n_new=n_new, refused_since_last_check=False)
    assert pc.n_active == n_new == host.n_active                   # the stale host int was fetched from the device word
    K.assert_states_equal(full(pc), full(host), "after grow()")
    for bad in (dict(split_prev_gen=False), dict(prune_prev_gen=False, curr_gen=None)):
        with pytest.raises((NotImplementedError, ValueError)):
            dd.enqueue(**dict(kw, **bad))
    assert dd.check()["applications"] == 1                          # argument errors enqueue nothing


def test_one_capture_serves_other_states_rules_and_counts():
    """Capture once (nothing runs), then replay on three states with different live counts and statistics; the third switches on the
    size threshold, which was off at capture, and another curr_gen.  Every replay equals the host-driven call on a copy of the state it
    started from, handed the draws the replay made (the object owns z: torch.randn is part of the graph)."""
    from egogaussian_amd import densify
    pd = 0.01
    states = [(257, dict(B.LATTICE_KW, max_screen_size=None, clone=True, split=True, curr_gen=None, prune_prev_gen=True, which_object=None)),
              (2049, dict(B.LATTICE_KW, max_screen_size=None, clone=True, split=True, curr_gen=1, prune_prev_gen=True, which_object=None)),
              (1500, dict(B.LATTICE_KW, max_screen_size=20.0, clone=True, split=True, curr_gen=2, prune_prev_gen=False, which_object=1))]
    first = K.live_state(K.live_inputs(states[0][0]))
    dev = CapModel(first, K.CAPACITY, pd, "fused")
    gen = torch.Generator(device=DEV).manual_seed(5)
    dd = densify.DeviceDensify(dev, generator=gen).capture()
    graph = dd.graph
    torch.cuda.synchronize()
    K.assert_states_equal(_full(dev), _full(CapModel(first, K.CAPACITY, pd, "fused")), "capture ran something")
    draws = []
    for i, (n_live, kw) in enumerate(states):
        inp = K.live_inputs(n_live, seed=i)
        live = K.live_state(inp, seed=i)
        _, rules = _kw(kw)
        _load(dev, live, n_live)
        host = CapModel(live, K.CAPACITY, pd, "fused")
        dd.replay(**rules)
        z = dd.z.clone()
        _, n_new = K.reference_plan(inp, kw)
        assert n_new <= K.CAPACITY and densify.densify_and_prune(host, z=lambda rows: z[:rows], **rules) == (n_live, n_new)
        K.assert_states_equal(_full(dev), _full(host), f"replay {i}")
        assert dd.graph is graph and dd.check()["applications"] == i + 1
        draws.append(z)
    assert not torch.equal(draws[0], draws[1]) and abs(float(draws[1].mean())) < 0.05 and abs(float(draws[1].std()) - 1) < 0.05


def _node_count(dd):
    """(nodes, kernel nodes) of the chain as hipGraph records it (the caller owns z: library launches only), asked of the HIP runtime
    the process has loaded: hipGraphGetNodes / hipGraphNodeGetType on the recorded graph."""
    import ctypes as C
    from egogaussian_amd.graph import begin_capture, end_capture
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    g = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        begin_capture(g)
        try:
            dd._chain()
        finally:
            end_capture(g)
    torch.cuda.current_stream().wait_stream(side)
    raw, n = C.c_void_p(g.raw_cuda_graph()), C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0 and n.value > 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(n)) == 0
    kernels = 0
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
        kernels += kind.value == 0                                   # hipGraphNodeTypeKernel
    return n.value, kernels


def test_launch_count_does_not_depend_on_the_table_or_the_plan():
    """The recorded chain has the same number of nodes for SH degree 0 (f_rest has no column and leaves the table: 23 arrays) and
    degree 3 (26 arrays, one of 45 floats per row), for a model of one live row and a full one: two apply launches whatever the table
    and the plan hold."""
    from egogaussian_amd import densify
    counts = {}
    for degree in (0, 3):
        for n_live in (1, 1000):
            inp = K.live_inputs(n_live)
            live = K.live_state(inp)
            M = (degree + 1) ** 2
            live["f_rest"] = torch.full((n_live, M - 1, 3), 0.25)
            live["f_rest_exp_avg"], live["f_rest_exp_avg_sq"] = torch.zeros_like(live["f_rest"]), torch.zeros_like(live["f_rest"])
            m = CapModel(live, 1000, 0.01, "fused")
            dd = densify.DeviceDensify(m, z=K.draws(1000).to(DEV))
            counts[(degree, n_live)] = _node_count(dd)
    torch.cuda.synchronize()
    assert len(set(counts.values())) == 1, counts
    total, kernels = next(iter(counts.values()))
    assert total == kernels >= 8, counts             # flags, four scans, emit, gather, commit: kernel launches and nothing else


def test_densify_inside_a_replayed_training_loop():
    """A captured training step (densify_stats=True) replays 20 times, DeviceDensify.replay densifies from the statistics those steps
    left, 20 more replays follow with no recapture().  The densified state equals the host-driven call on a copy of the snapshot; the next
    render sees the new count: radii zero at and beyond it, non-zero somewhere among the new rows."""
    from egogaussian_amd import densify
    from egogaussian_amd.capacity import CapacityGaussians
    from egogaussian_amd.graph import GraphedTrainStep
    from egogaussian_amd.scene_synth import make_camera, perturb_student, SynthGaussians, Pipe
    from egogaussian_amd.renderer import render
    H, W, n, cap = 64, 64, 2000, 8000
    teacher = _scene(n, H, W)
    student = perturb_student(teacher)
    cam, bg = make_camera(0, H, W, device=DEV), torch.zeros(3, device=DEV)
    with torch.no_grad():
        gt = render(cam, SynthGaussians(teacher, device=DEV, requires_grad=False), Pipe, bg)["render"].clone()
    pc = CapacityGaussians(student, cap, device=DEV)
    pc.training_setup(capturable=True)
    step = GraphedTrainStep(pc, pc.optimizer, bg, 0.2, densify_stats=True).capture(cam, gt, warmup=2, capacity_margin=4.0)
    for _ in range(20):
        step(cam, gt)
    dd = densify.DeviceDensify(pc).capture()
    torch.cuda.synchronize()
    arrays = {k: getattr(pc, a) for k, a in ATTR.items()}
    moments = {k: pc.optimizer.state[p] for k, p in arrays.items() if "exp_avg" in pc.optimizer.state.get(p, {})}
    assert {"xyz", "f_dc", "opacity", "scaling", "rotation"} <= set(moments)
    host = CapacityGaussians(student, cap, device=DEV)
    host.training_setup(capturable=True)
    with torch.no_grad():
        for k, a in ATTR.items():
            p = getattr(host, a)
            p.copy_(arrays[k])
            if k in moments:
                host.optimizer.state[p] = {"step": torch.tensor(20.0), "exp_avg": moments[k]["exp_avg"].clone(), "exp_avg_sq": moments[k]["exp_avg_sq"].clone()}
        for k in K.STATS + ("_generation", "_is_object"):
            getattr(host, k).copy_(getattr(pc, k))
    assert float(pc.denom[:n].sum()) > 0
    rules = dict(max_grad=5e-5, min_opacity=0.005, extent=10.0, max_screen_size=None)
    dd.replay(**rules)
    z = dd.z.clone()
    n0, n1 = densify.densify_and_prune(host, z=lambda rows: z[:rows], **rules)
    assert n0 == n and n1 != n and n1 <= cap and pc.n_active == n1 and dd.check()["refused_since_last_check"] is False
    for k, a in ATTR.items():
        assert torch.equal(getattr(pc, a).detach(), getattr(host, a).detach()), k
        if k in moments:
            for m in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(moments[k][m], host.optimizer.state[getattr(host, a)][m]), (k, m)
    for k in K.STATS + ("_generation", "_is_object", "active_count"):
        assert torch.equal(getattr(pc, k), getattr(host, k)), k
    graph0 = step.graph
    loss = step(cam, gt)
    torch.cuda.synchronize()
    radii, n_orig = step.radii, int(dd.totals[0])
    assert int(radii[n1:].abs().max()) == 0 and n_orig < n1
    assert int(radii[n_orig:n1].max()) > 0, "no clone or split child is visible"
    for _ in range(19):
        loss = step(cam, gt)
    torch.cuda.synchronize()
    assert step.ok() and step.recaptures == 0 and step.graph is graph0 and math.isfinite(float(loss))
