"""Densification bookkeeping on the device, with the reference's method names and
semantics so that a trainer can call these instead of the GaussianModel methods:

    reference (scene/gaussian_model.py)                        here
    -----------------------------------------------------     --------------------------------------------------------
    gaussians.max_radii2D[vis] = max(...)  (train_static:125)  add_densification_stats(gaussians, viewspace, vis, radii)
    gaussians.add_densification_stats(viewspace, vis)  :735        (one kernel for both; no index tensors)
    gaussians.densify_and_prune(...)                   :678     densify_and_prune(gaussians, ...)
    gaussians.prune_points(mask)                       :536     prune_points(gaussians, mask)
    gaussians.reset_opacity()                          :484     reset_opacity(gaussians)

`gaussians` is duck-typed: the reference's GaussianModel or egogaussian_amd.scene_synth.SynthGaussians -- anything with
`_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, _label` (parameters registered one per group, named
"xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "label", in `optimizer`), `_generation`, `_is_object`,
`xyz_gradient_accum`, `denom`, `max_radii2D`, `percent_dense`.  As in the reference every call leaves NEW nn.Parameter
objects in the model and in the optimizer, with the Adam moments carried over for surviving Gaussians and zero for new ones.

The selection rules and the element order are the reference's, evaluated by HIP kernels (csrc/densify.hip): one pass
computes, for every Gaussian, which of {itself, a clone, two split children} survive; scans turn that into a plan
(source index + kind per new Gaussian); one gather per array builds the new model.  The reference materialises ~40
intermediate masked copies and concatenations per call and synchronises with the host at every boolean index; here the
host reads four counters once.  HIP device tensors only (no CPU path; the CPU restatement is oracle/densify_torch.py, pinned
by a fixture captured from the reference).

A capacity-sized model (capacity.CapacityGaussians) can also be densified and pruned with that one host read gone: DeviceDensify
below plans over `capacity` rows with the live count read on the device and applies the plan in place in two launches, as a chain
a hipGraph can record; apply_statement states in torch ops what that apply does.  The host-driven calls stay as they are.
"""
import ctypes as C

import torch
from torch import nn

from . import lib as _lib
from . import _hip as _launch

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "label")
_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation", "label": "_label"}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return _launch.stream_of(torch.device("cuda", torch.cuda.current_device()))


def _hip(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the densification kernels have no CPU path")
    return t


def add_densification_stats(gaussians, viewspace_point_tensor, update_filter, radii=None):
    """xyz_gradient_accum[f] += |viewspace.grad[f, :2]|, denom[f] += 1 and, when `radii` is given, max_radii2D[f] =
    max(max_radii2D[f], radii[f]) for the visible Gaussians f -- in place, one kernel."""
    L = _lib.load()
    g = _hip(viewspace_point_tensor.grad, "viewspace_point_tensor.grad").float().contiguous()
    P = g.shape[0]
    vis = None
    if update_filter is not None:
        vis = update_filter if update_filter.dtype in (torch.bool, torch.uint8) else update_filter != 0
        vis = vis.contiguous().view(torch.uint8)
    r = None if radii is None else radii.to(torch.int32).contiguous()
    acc, den = gaussians.xyz_gradient_accum, gaussians.denom
    mr = gaussians.max_radii2D if radii is not None else None
    for t in (acc, den) + ((mr,) if mr is not None else ()):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("densification statistics must be contiguous float32 HIP tensors")
    with torch.cuda.device(g.device):
        _lib.check(L.egs_densify_stats(P, _p(g), _p(vis), _p(r), _p(acc), _p(den), _p(mr), _stream()))


class _Plan:
    """Device-side description of the new model: src[k], kind[k] for its k-th Gaussian."""

    def __init__(self, P, dev):
        L = _lib.load()
        self.P, self.dev = P, dev
        self.scratch = torch.empty(L.egs_densify_plan_scratch_bytes(P), dtype=torch.uint8, device=dev)
        self.src = torch.empty(3 * P, dtype=torch.int32, device=dev)
        self.kind = torch.empty(3 * P, dtype=torch.uint8, device=dev)
        self.split_rank = torch.empty(P, dtype=torch.int32, device=dev)
        self.totals = torch.zeros(4, dtype=torch.int64, device=dev)

    def finish(self):
        n_orig, n_clone, n_child, n_split = [int(v) for v in self.totals.tolist()]          # the one host read
        self.n_split, self.n_new = n_split, n_orig + n_clone + 2 * n_child
        self.counts = (n_orig, n_clone, n_child)
        return self

    def rows(self, t, zero_new=False):
        """New float array: row k = t[src[k]]; zero_new: zeros for every row that is not a kept original (Adam moments)."""
        L = _lib.load()
        src = t.detach().float().contiguous()
        D = int(src.numel() // max(src.shape[0], 1))
        out = torch.empty((self.n_new,) + tuple(src.shape[1:]), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(L.egs_gather_rows_f32(self.n_new, D, _p(self.src), _p(self.kind), int(zero_new), _p(src), _p(out), _stream()))
        return out

    def ints(self, t, clone_value=None):
        L = _lib.load()
        orig_dtype = t.dtype
        src = t.detach().to(torch.int32).contiguous()
        out = torch.empty((self.n_new,) + tuple(src.shape[1:]), dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(L.egs_gather_i32(self.n_new, _p(self.src), _p(self.kind), int(clone_value is not None),
                                        0 if clone_value is None else int(clone_value), _p(src.view(-1)), _p(out.view(-1)), _stream()))
        return out.to(orig_dtype)


def _apply_in_place(gaussians, plan, reset_stats, z=None, curr_gen=None):
    """Capacity-sized model (capacity.CapacityGaussians): the new model is gathered from the live prefix into temporaries and
    copied back INTO the same arrays; tensors, Parameter objects and optimizer state entries keep their identity and address.
    Returns False (nothing changed) when the new count does not fit the capacity -- the caller grows the model first."""
    L = _lib.load()
    n_old, n_new = gaussians.n_active, plan.n_new
    if n_new > gaussians.capacity:
        return False
    live = lambda t: t.detach()[:n_old]
    old = {k: live(getattr(gaussians, _ATTR[k])) for k in GROUPS}
    new = {k: plan.rows(old[k]) for k in GROUPS}
    if plan.n_split:
        with torch.cuda.device(plan.dev):
            _lib.check(L.egs_split_children(plan.n_new, _p(plan.src), _p(plan.kind), _p(plan.split_rank), plan.n_split, _p(z),
                                            _p(old["xyz"].float().contiguous()), _p(old["scaling"].float().contiguous()),
                                            _p(old["rotation"].float().contiguous()), _p(new["xyz"]), _p(new["scaling"]), _stream()))
    opt = getattr(gaussians, "optimizer", None)
    with torch.no_grad():
        if opt is not None:
            for group in opt.param_groups:
                name = group.get("name")
                if name not in new:
                    continue
                stored = opt.state.get(group["params"][0], None)
                if stored is not None and "exp_avg" in stored:
                    for key in ("exp_avg", "exp_avg_sq"):
                        stored[key][:n_new].copy_(plan.rows(stored[key][:n_old], zero_new=True))
        for k in GROUPS:
            getattr(gaussians, _ATTR[k]).detach()[:n_new].copy_(new[k])
        gaussians._generation[:n_new].copy_(plan.ints(gaussians._generation[:n_old], clone_value=curr_gen))
        gaussians._is_object[:n_new].copy_(plan.ints(gaussians._is_object[:n_old]))
        if n_new < n_old:                                       # vacated rows hold no Gaussian: their tags must not be counted by anyone
            gaussians._generation[n_new:n_old].zero_()
            gaussians._is_object[n_new:n_old].zero_()
        for name in ("xyz_gradient_accum", "denom", "max_radii2D"):
            t = getattr(gaussians, name)
            if reset_stats:
                t.zero_()
            else:
                t[:n_new].copy_(plan.rows(t[:n_old]))
    gaussians.set_active(n_new)
    return True


def _apply(gaussians, plan, reset_stats, z=None, curr_gen=None, during_training=True):
    L = _lib.load()
    old = {k: getattr(gaussians, _ATTR[k]) for k in GROUPS}
    new = {k: plan.rows(old[k]) for k in GROUPS}
    if plan.n_split:
        with torch.cuda.device(plan.dev):
            _lib.check(L.egs_split_children(plan.n_new, _p(plan.src), _p(plan.kind), _p(plan.split_rank), plan.n_split, _p(z),
                                            _p(old["xyz"].detach().float().contiguous()), _p(old["scaling"].detach().float().contiguous()),
                                            _p(old["rotation"].detach().float().contiguous()), _p(new["xyz"]), _p(new["scaling"]), _stream()))
    opt = getattr(gaussians, "optimizer", None) if during_training else None
    if opt is not None:
        for group in opt.param_groups:
            name = group.get("name")
            if name not in new:                              # object pose groups etc. are left alone (gaussian_model.py:515, :250)
                continue
            p_old = group["params"][0]
            stored = opt.state.get(p_old, None)
            p_new = nn.Parameter(new[name].requires_grad_(True))
            if stored is not None:
                stored["exp_avg"] = plan.rows(stored["exp_avg"], zero_new=True)
                stored["exp_avg_sq"] = plan.rows(stored["exp_avg_sq"], zero_new=True)
                del opt.state[p_old]
                opt.state[p_new] = stored
            group["params"][0] = p_new
            new[name] = p_new
    for k in GROUPS:
        v = new[k]
        if opt is None and during_training:
            v = nn.Parameter(v.requires_grad_(True))
        setattr(gaussians, _ATTR[k], v)
    gaussians._generation = plan.ints(gaussians._generation, clone_value=curr_gen)
    gaussians._is_object = plan.ints(gaussians._is_object)
    if during_training:
        if reset_stats:
            gaussians.xyz_gradient_accum = torch.zeros((plan.n_new, 1), device=plan.dev)
            gaussians.denom = torch.zeros((plan.n_new, 1), device=plan.dev)
            gaussians.max_radii2D = torch.zeros((plan.n_new,), device=plan.dev)
        else:
            gaussians.xyz_gradient_accum = plan.rows(gaussians.xyz_gradient_accum)
            gaussians.denom = plan.rows(gaussians.denom)
            gaussians.max_radii2D = plan.rows(gaussians.max_radii2D)


def densify_and_prune(gaussians, max_grad, min_opacity, extent, max_screen_size, clone=True, split=True, curr_gen=None,
                      prune_prev_gen=True, split_prev_gen=True, which_object=None, z=None, generator=None):
    """Same arguments as GaussianModel.densify_and_prune (:678).  `z` ([2 * n_split, 3] standard-normal draws, first children
    first -- or a callable rows -> such a tensor) makes the split deterministic; by default it is drawn here with `generator`.  Returns (n_before, n_after)."""
    if not split_prev_gen and split:
        raise NotImplementedError("split_prev_gen=False: the reference raises here (curr_gen lands in densify_and_split's N slot, "
                                  "gaussian_model.py:698 vs :588); there is no behaviour to reproduce")
    if not prune_prev_gen and curr_gen is None:
        raise ValueError("prune_prev_gen=False needs curr_gen")
    L = _lib.load()
    xyz = _hip(gaussians._xyz, "_xyz")
    in_place = getattr(gaussians, "capacity", None) is not None      # capacity.CapacityGaussians: plan on the live prefix, write back in place
    P, dev = (gaussians.n_active if in_place else xyz.shape[0]), xyz.device
    if P == 0:
        return 0, 0
    f = lambda t: t.detach()[:P].float().contiguous()
    i32 = lambda t: t.detach()[:P].to(torch.int32).contiguous()
    plan = _Plan(P, dev)
    mss = 0.0 if not max_screen_size else float(max_screen_size)
    with torch.cuda.device(dev):
        _lib.check(L.egs_densify_plan(
            P, _p(f(gaussians.xyz_gradient_accum)), _p(f(gaussians.denom)), _p(f(gaussians._scaling)), _p(f(gaussians._opacity)),
            _p(f(gaussians.max_radii2D)), _p(i32(gaussians._generation)), _p(i32(gaussians._is_object)), float(max_grad),
            float(min_opacity), float(gaussians.percent_dense), float(extent), mss, int(bool(clone)), int(bool(split)),
            int(curr_gen is not None), 0 if curr_gen is None else int(curr_gen), int(bool(prune_prev_gen)),
            int(which_object is not None), 0 if which_object is None else int(which_object), _p(plan.scratch), _p(plan.src),
            _p(plan.kind), _p(plan.split_rank), _p(plan.totals), _stream()))
    plan.finish()
    if plan.n_split:
        if z is None:
            z = torch.randn((2 * plan.n_split, 3), device=dev, generator=generator)
        elif callable(z):
            z = z(2 * plan.n_split).to(dev)                          # z(rows) -> [rows, 3]: the caller's draws, sized once the plan is known
        z = _hip(z, "z").float().contiguous()
        if tuple(z.shape) != (2 * plan.n_split, 3):
            raise ValueError(f"z must be [{2 * plan.n_split}, 3] (two children per split Gaussian), got {tuple(z.shape)}")
    if in_place:
        if not _apply_in_place(gaussians, plan, reset_stats=bool(clone or split), z=z, curr_gen=curr_gen):
            gaussians.grow(max(int(plan.n_new * 1.5), plan.n_new + 1024))        # new arrays: a captured step must be captured again
            if not _apply_in_place(gaussians, plan, reset_stats=bool(clone or split), z=z, curr_gen=curr_gen):
                raise RuntimeError(f"densify_and_prune: {plan.n_new} Gaussians do not fit the capacity {gaussians.capacity} after grow()")
        return P, plan.n_new
    _apply(gaussians, plan, reset_stats=bool(clone or split), z=z, curr_gen=curr_gen)
    return P, plan.n_new


def prune_points(gaussians, mask, during_training=True):
    """GaussianModel.prune_points (:536): drop the Gaussians where `mask` is True, carrying the optimizer moments along."""
    L = _lib.load()
    xyz = _hip(gaussians._xyz, "_xyz")
    in_place = getattr(gaussians, "capacity", None) is not None and during_training
    P, dev = (gaussians.n_active if in_place else xyz.shape[0]), xyz.device
    if P == 0:
        return 0, 0
    m = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0)[:P].contiguous().view(torch.uint8)
    plan = _Plan(P, dev)
    with torch.cuda.device(dev):
        _lib.check(L.egs_prune_plan(P, _p(m), _p(plan.scratch), _p(plan.src), _p(plan.kind), _p(plan.split_rank), _p(plan.totals), _stream()))
    plan.finish()
    if in_place:
        _apply_in_place(gaussians, plan, reset_stats=False)
        return P, plan.n_new
    _apply(gaussians, plan, reset_stats=False, during_training=during_training)
    return P, plan.n_new


_STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
_MOMENTS = ("exp_avg", "exp_avg_sq")


def _rule_words(percent_dense, max_grad, min_opacity, extent, max_screen_size, clone, split, curr_gen, prune_prev_gen, which_object):
    """The twelve words of egs_densify_rules_dev (int32 view).  The two thresholds are float32 products of the float32 arguments, as
    egs_densify_plan forms them."""
    import numpy as np
    f = np.float32
    w = np.zeros(12, np.int32)
    w[:5].view(np.float32)[:] = (f(max_grad), f(min_opacity), f(percent_dense) * f(extent), f(0.1) * f(extent),
                                 f(0.0 if not max_screen_size else max_screen_size))
    w[5:] = (int(bool(clone)), int(bool(split)), int(curr_gen is not None), 0 if curr_gen is None else int(curr_gen), int(bool(prune_prev_gen)),
             int(which_object is not None), 0 if which_object is None else int(which_object))
    return w


def _check_rules(split=True, curr_gen=None, prune_prev_gen=True, split_prev_gen=True, **_):
    if not split_prev_gen and split:
        raise NotImplementedError("split_prev_gen=False: the reference raises here (curr_gen lands in densify_and_split's N slot, "
                                  "gaussian_model.py:698 vs :588); there is no behaviour to reproduce")
    if not prune_prev_gen and curr_gen is None:
        raise ValueError("prune_prev_gen=False needs curr_gen")


def apply_statement(state, plan, active_count, status, z=None, curr_gen=None, stats_reset=False):
    """What egs_densify_apply does, in torch ops on any device: the statement the kernels answer to.

    state: name -> [capacity, ...] tensor, the names of oracle/densify_torch.py (the seven parameters, "<p>_exp_avg", "<p>_exp_avg_sq",
    "generation", "is_object", "xyz_gradient_accum", "denom", "max_radii2D"); rewritten IN PLACE.  plan: "src", "kind", "split_rank",
    "totals" (originals, clones, children per copy, split sources) as egs_densify_plan_dev leaves them for the live prefix.
    active_count: int tensor [1], in / out.  status: int tensor [4] (refusals, rows the latest refusal needed, applications, n_new of the
    latest application), in / out.  z: [2 * capacity, 3]; child c of split rank r reads row c * n_split + r.  curr_gen: the clones'
    generation, None = inherited.  stats_reset: a clone or split step ran (a prune plan: False).  -> True when applied."""
    t = lambda a: a if torch.is_tensor(a) else torch.as_tensor(a)
    capacity = state["xyz"].shape[0]
    dev = state["xyz"].device
    n_orig, n_clone, n_child, n_split = (int(v) for v in t(plan["totals"]).tolist()[:4])
    n_old, n_new = int(active_count[0]), n_orig + n_clone + 2 * n_child
    if n_new > capacity:                                            # refusal: no array, no statistic, no count
        status[0] += 1; status[1] = n_new
        return False
    status[2] += 1; status[3] = n_new
    if n_old == 0:
        return True
    src = t(plan["src"])[:n_new].to(dev, torch.int64)
    kind = t(plan["kind"])[:n_new].to(dev, torch.int64)
    old = {k: v[:n_old].clone() for k, v in state.items()}          # the shadow: every row is read before any is written
    new = {}
    for k, v in old.items():
        rows = v[src]
        if k.endswith("_exp_avg") or k.endswith("_exp_avg_sq"):
            rows[kind != 0] = 0
        elif k == "generation" and curr_gen is not None:
            rows[kind == 1] = curr_gen
        new[k] = rows
    child = kind >= 2
    if bool(child.any()):
        s = src[child]
        zrow = (kind[child] - 2) * n_split + t(plan["split_rank"]).to(dev, torch.int64)[s]
        scale = torch.exp(old["scaling"][s])
        q = old["rotation"][s]
        q = q / q.norm(dim=1, keepdim=True)
        r, x, y, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y),
                         2 * (x * y + r * w), 1 - 2 * (x * x + w * w), 2 * (y * w - r * x),
                         2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
        new["xyz"][child] = torch.bmm(R, (scale * z[zrow].to(dev)).unsqueeze(-1)).squeeze(-1) + old["xyz"][s]
        new["scaling"][child] = torch.log(scale / (0.8 * 2))
    for k, v in state.items():
        if k in _STATS and stats_reset:
            v.zero_()                                               # all `capacity` rows
            continue
        v[:n_new] = new[k]
        if k in ("generation", "is_object") and n_new < n_old:
            v[n_new:n_old] = 0                                      # vacated rows hold no Gaussian
    active_count[0] = n_new                                         # last
    return True


class DeviceDensify:
    """densify_and_prune / prune_points of a capacity-sized model (capacity.CapacityGaussians with an optimizer whose moments exist)
    with every count left on the device: plan (egs_densify_plan_dev / egs_prune_plan_dev) and in-place apply (egs_densify_apply) are
    enqueued on the current stream -- a fixed number of launches, no allocation, no host read -- and can be recorded once into a hipGraph
    of their own (capture / replay).  The rule values travel in a twelve-word device block written before every run, so one capture
    serves every rule set; what a capture bakes in is the addresses of the model's arrays and its capacity, which is why a changed
    address (CapacityGaussians.grow) is refused on every call and asks for a new object.  A densification that does not fit the capacity
    writes nothing and counts a refusal in `status`; check() reads it when the trainer synchronises anyway.

    z: the caller's [2 * capacity, 3] standard-normal draws (child c of split rank r reads row c * n_split + r); by default the object
    owns the buffer and refills it with torch.randn(..., out=) (`generator`) before every run."""

    def __init__(self, gaussians, z=None, generator=None):
        g = gaussians
        if getattr(g, "capacity", None) is None or getattr(g, "active_count", None) is None:
            raise ValueError("DeviceDensify needs a capacity-sized model (capacity.CapacityGaussians): a plain model's arrays change size, "
                             "which only the host-driven densify.densify_and_prune / densify.prune_points can do")
        if getattr(g, "optimizer", None) is None:
            raise ValueError("DeviceDensify needs the model's optimizer (training_setup) with its Adam moments allocated")
        L = _lib.load()
        self.gaussians, self.capacity, self.dev = g, int(g.capacity), g._xyz.device
        self.generator = generator
        entries = self._entries()
        if len(entries) > _lib.DENSIFY_MAX_ARRAYS:
            raise ValueError(f"{len(entries)} per-Gaussian arrays; egs_densify_apply takes {_lib.DENSIFY_MAX_ARRAYS}")
        self._names = [e[0] for e in entries]
        self._table = (_lib.DensifyArray * len(entries))()
        row_floats = (C.c_int32 * len(entries))()
        for i, (name, ten, role, flags) in enumerate(entries):
            want = torch.int32 if flags & _lib.DENSIFY_TAG_I32 else torch.float32
            if not (ten.is_cuda and ten.device == self.dev and ten.dtype == want and ten.is_contiguous() and ten.dim() >= 1 and ten.shape[0] == self.capacity
                    and ten.numel() > 0):
                raise ValueError(f"DeviceDensify: {name} must be a contiguous {want} tensor of {self.capacity} rows on {self.dev} "
                                 f"(got {tuple(ten.shape)} {ten.dtype} on {ten.device})")
            row_floats[i] = ten.numel() // self.capacity
            self._table[i] = _lib.DensifyArray(ten.data_ptr(), row_floats[i], role, flags, 0)
        self._addresses = self._current_addresses()
        self._index = {n: self._names.index(n) for n in ("xyz", "scaling", "rotation")}
        self._object_is_float = int(g._is_object.dtype == torch.float32)
        cap, dev = self.capacity, self.dev
        self.plan_scratch = torch.empty(L.egs_densify_plan_scratch_bytes(cap), dtype=torch.uint8, device=dev)
        self.src = torch.empty(3 * cap, dtype=torch.int32, device=dev)
        self.kind = torch.empty(3 * cap, dtype=torch.uint8, device=dev)
        self.split_rank = torch.empty(cap, dtype=torch.int32, device=dev)
        self.totals = torch.zeros(5, dtype=torch.int64, device=dev)
        self.scratch_bytes = int(L.egs_densify_apply_scratch_bytes(cap, len(entries), row_floats))
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=dev)
        self.rules = torch.zeros(12, dtype=torch.int32, device=dev)
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)         # four uint32 words
        self._owns_z = z is None
        if z is None:
            z = torch.zeros((2 * cap, 3), dtype=torch.float32, device=dev)
        elif not (z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and tuple(z.shape) == (2 * cap, 3)):
            raise ValueError(f"z must be a contiguous float32 [{2 * cap}, 3] tensor on the model's device (two draws per row of the capacity)")
        self.z = z
        self._mask = None
        self.graph = None
        self._refusals_seen = 0

    # ---- the array table -----------------------------------------------------------------------------------------------------------
    def _entries(self):
        """(name, tensor, role, flags) of every per-Gaussian array, in the table's order."""
        g, opt = self.gaussians, self.gaussians.optimizer
        out, moments = [], []
        by_name = {grp.get("name"): grp["params"][0] for grp in opt.param_groups}
        for k in GROUPS:
            p = getattr(g, _ATTR[k])
            if by_name.get(k) is not p:
                raise ValueError(f"DeviceDensify: the optimizer's group '{k}' does not hold the model's {_ATTR[k]}")
            st = opt.state.get(p, None)
            if p.numel() == 0:                                      # f_rest at SH degree 0: no column, nothing to move
                continue
            out.append((k, p.detach(), _lib.DENSIFY_PARAM, 0))
            if st is not None and all(m in st for m in _MOMENTS):   # (a group that never received a gradient has none: as densify_and_prune)
                moments += [(f"{k}_{m}", st[m], _lib.DENSIFY_MOMENT, 0) for m in _MOMENTS]
        if not moments:
            raise ValueError("DeviceDensify: the optimizer has no Adam moments yet (the first step creates them, at addresses this object "
                             "must know); step once, or capture the training step, before building it")
        out += moments
        out += [(n, getattr(g, n), _lib.DENSIFY_STAT, 0) for n in _STATS]
        out.append(("generation", g._generation, _lib.DENSIFY_TAG, _lib.DENSIFY_TAG_I32 | _lib.DENSIFY_TAG_CLONE_GEN))
        out.append(("is_object", g._is_object, _lib.DENSIFY_TAG, _lib.DENSIFY_TAG_I32 if g._is_object.dtype == torch.int32 else 0))
        return out

    def _current_addresses(self):
        g, opt = self.gaussians, self.gaussians.optimizer
        ptrs = []
        for k in GROUPS:
            p = getattr(g, _ATTR[k])
            st = opt.state.get(p, {})
            ptrs += [p.data_ptr()] + [st[m].data_ptr() if m in st else 0 for m in _MOMENTS]
        ptrs += [getattr(g, n).data_ptr() for n in _STATS + ("_generation", "_is_object", "active_count")]
        return (int(g.capacity),) + tuple(ptrs)

    def _check_addresses(self):
        if self._current_addresses() != self._addresses:
            raise RuntimeError("DeviceDensify: the model's arrays moved or its capacity changed since this object was built "
                               "(CapacityGaussians.grow, or a call that replaced a parameter); build a new DeviceDensify -- the table and any "
                               "captured chain point at the old arrays")

    # ---- the chain -------------------------------------------------------------------------------------------------------------------
    def _write_rules(self, max_grad, min_opacity, extent, max_screen_size, clone=True, split=True, curr_gen=None, prune_prev_gen=True,
                     split_prev_gen=True, which_object=None):
        w = _rule_words(self.gaussians.percent_dense, max_grad, min_opacity, extent, max_screen_size, clone, split, curr_gen, prune_prev_gen,
                        which_object)
        self.rules.copy_(torch.from_numpy(w).pin_memory(), non_blocking=True)                # the one small copy

    def _chain(self):
        """The launches of one densification, as they are enqueued or recorded: the draws, the plan, the apply."""
        L, g = _lib.load(), self.gaussians
        if self._owns_z:
            torch.randn(self.z.shape, generator=self.generator, out=self.z)
        _lib.check(L.egs_densify_plan_dev(
            self.capacity, _p(g.active_count), _p(g.xyz_gradient_accum), _p(g.denom), _p(g._scaling), _p(g._opacity), _p(g.max_radii2D),
            _p(g._generation), _p(g._is_object), self._object_is_float, _p(self.rules), _p(self.plan_scratch), _p(self.src), _p(self.kind),
            _p(self.split_rank), _p(self.totals), _stream()))
        self._apply(_p(self.rules), _p(self.z))

    def _apply(self, rules, z):
        L = _lib.load()
        _lib.check(L.egs_densify_apply(self.capacity, _p(self.gaussians.active_count), _p(self.src), _p(self.kind), _p(self.split_rank),
                                       _p(self.totals), rules, len(self._names), self._table, self._index["xyz"], self._index["scaling"],
                                       self._index["rotation"], z, _p(self.scratch), _p(self.status), _stream()))

    def _count_moved(self):
        mark = getattr(self.gaussians, "mark_active_stale", None)
        if mark is not None:
            mark()

    def enqueue(self, max_grad, min_opacity, extent, max_screen_size, clone=True, split=True, curr_gen=None, prune_prev_gen=True,
                which_object=None, split_prev_gen=True):
        """densify_and_prune's arguments and argument errors; plan and apply run on the current stream, nothing is read back."""
        rules = dict(max_grad=max_grad, min_opacity=min_opacity, extent=extent, max_screen_size=max_screen_size, clone=clone, split=split,
                     curr_gen=curr_gen, prune_prev_gen=prune_prev_gen, split_prev_gen=split_prev_gen, which_object=which_object)
        _check_rules(**rules)
        self._check_addresses()
        with torch.cuda.device(self.dev), torch.no_grad():
            self._write_rules(**rules)
            self._chain()
        self._count_moved()

    def enqueue_prune(self, mask):
        """prune_points(mask) the same way (egs_prune_plan_dev): rows where `mask` is True leave; a mask shorter than the capacity covers
        the first rows, the rest being beyond the live count anyway."""
        self._check_addresses()
        L, g = _lib.load(), self.gaussians
        m = _hip(mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0, "mask").contiguous().view(torch.uint8).reshape(-1)
        with torch.cuda.device(self.dev), torch.no_grad():
            if m.shape[0] < self.capacity:
                if self._mask is None:
                    self._mask = torch.zeros(self.capacity, dtype=torch.uint8, device=self.dev)
                self._mask[:m.shape[0]].copy_(m)
                m = self._mask
            _lib.check(L.egs_prune_plan_dev(self.capacity, _p(g.active_count), _p(m), _p(self.plan_scratch), _p(self.src), _p(self.kind),
                                            _p(self.split_rank), _p(self.totals), _stream()))
            self._apply(None, None)
        self._count_moved()

    def capture(self):
        """Records the chain of enqueue() (with the torch.randn, when this object owns z) into a hipGraph of its own -> self.  Nothing
        runs.  Baked in: the addresses of the model's arrays and of this object's buffers, and the capacity.  Not baked in: any rule value
        (replay() writes the block), any count (device words), the draws (a fresh Philox offset per replay)."""
        from .graph import begin_capture, end_capture
        self._check_addresses()
        _lib.load()
        graph = torch.cuda.CUDAGraph()
        if self._owns_z and self.generator is not None and hasattr(graph, "register_generator_state"):
            graph.register_generator_state(self.generator)
        side = torch.cuda.Stream(self.dev)
        main = torch.cuda.current_stream(self.dev)
        with torch.cuda.device(self.dev), torch.no_grad():
            side.wait_stream(main)
            with torch.cuda.stream(side):
                begin_capture(graph)
                try:
                    self._chain()
                finally:
                    end_capture(graph)
            main.wait_stream(side)
        self.graph = graph
        return self

    def replay(self, max_grad, min_opacity, extent, max_screen_size, clone=True, split=True, curr_gen=None, prune_prev_gen=True,
               which_object=None, split_prev_gen=True):
        """enqueue() through the captured chain: writes the rule block, launches the graph."""
        if self.graph is None:
            raise RuntimeError("DeviceDensify.replay: capture() first")
        rules = dict(max_grad=max_grad, min_opacity=min_opacity, extent=extent, max_screen_size=max_screen_size, clone=clone, split=split,
                     curr_gen=curr_gen, prune_prev_gen=prune_prev_gen, split_prev_gen=split_prev_gen, which_object=which_object)
        _check_rules(**rules)
        self._check_addresses()
        with torch.cuda.device(self.dev), torch.no_grad():
            self._write_rules(**rules)
            self.graph.replay()
        self._count_moved()

    def check(self):
        """Reads `status` (the one read: synchronises) -> its four words and whether a refusal happened since the last check()."""
        w = [int(v) & 0xffffffff for v in self.status.tolist()]
        out = dict(refusals=w[0], rows_needed=w[1], applications=w[2], n_new=w[3], refused_since_last_check=w[0] != self._refusals_seen)
        self._refusals_seen = w[0]
        return out


def reset_opacity(gaussians):
    """GaussianModel.reset_opacity (:484): opacity <- inverse_sigmoid(min(opacity, 0.01)), Adam moments of that group zeroed."""
    o = torch.minimum(torch.sigmoid(gaussians._opacity.detach()), torch.full_like(gaussians._opacity, 0.01))
    new = torch.log(o / (1 - o))
    opt = gaussians.optimizer
    if getattr(gaussians, "capacity", None) is not None:            # capacity-sized model: same tensors, new contents
        with torch.no_grad():
            gaussians._opacity.copy_(new)
            stored = opt.state.get(gaussians._opacity, None) if opt is not None else None
            if stored is not None and "exp_avg" in stored:
                stored["exp_avg"].zero_(); stored["exp_avg_sq"].zero_()
        return
    for group in opt.param_groups:
        if group.get("name") == "opacity":
            stored = opt.state.get(group["params"][0], None)
            p_new = nn.Parameter(new.requires_grad_(True))
            if stored is not None:
                stored["exp_avg"] = torch.zeros_like(new); stored["exp_avg_sq"] = torch.zeros_like(new)
                del opt.state[group["params"][0]]
                opt.state[p_new] = stored
            group["params"][0] = p_new
            gaussians._opacity = p_new
