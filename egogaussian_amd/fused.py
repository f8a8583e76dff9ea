"""Autograd wrappers of the fused HIP ops on the "next" rows of SURVEY.md section 8f, bound through the same C ABI:

  covariance_from_scaling_rotation / rotated_covariance_from_scaling_rotation   (row f-1)
      drop-in for the reference's covariance activations (/root/reference/scene/gaussian_model.py:29-33,46-63).  A
      reference GaussianModel can be pointed at them after construction:
          gaussians.covariance_activation = egogaussian_amd.fused.covariance_from_scaling_rotation
  l1_ssim_loss   (row f-3)
      (1 - lambda) * l1_loss + lambda * (1 - ssim), /root/reference/trainers/train_static.py:92-95.

HIP device tensors only.  Their oracles are the PyTorch versions in covariance.py / losses.py, which are pinned by
fixtures captured from the reference (tests/golden/covariance.npz, losses.npz).
"""
import ctypes as C

import torch

from . import lib as _lib
from . import _hip


def _p(t):
    return None if t is None else t.data_ptr()


_stream = _hip.stream_of           # (device) -> c_void_p of its current stream


def _need_hip(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: fused HIP op has no CPU path (use egogaussian_amd.covariance / losses)")
    return t.float().contiguous()


class _Cov3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, rotation, M, selected, modifier, row0_mult, log_scaling=False, opacity_raw=None):
        L = _lib.load()
        scaling, rotation = _need_hip(scaling, "scaling"), _need_hip(rotation, "rotation")
        N = scaling.shape[0]
        Mc = None if M is None else _need_hip(M, "M").reshape(9)
        sel = None if selected is None else selected.to(torch.uint8).contiguous()
        cov = torch.empty((N, 6), device=scaling.device, dtype=torch.float32)
        o_raw = None if opacity_raw is None else _need_hip(opacity_raw, "opacity_raw")
        opacity = None if o_raw is None else torch.empty_like(o_raw)
        with _hip.device_ctx(scaling.device):
            _lib.check(L.egs_cov3d_forward(N, _p(scaling), int(bool(log_scaling)), float(modifier), _p(rotation), _p(Mc), _p(sel), _p(cov),
                                           _p(o_raw), _p(opacity), _stream(scaling.device)))
        empty = torch.empty(0, device=scaling.device)
        ctx.save_for_backward(scaling, rotation, Mc if Mc is not None else empty, sel if sel is not None else empty,
                              opacity if opacity is not None else empty)
        mult_dev = row0_mult if torch.is_tensor(row0_mult) else None          # device float[1]: no host read of the selection count
        ctx.mult_dev = None if mult_dev is None else mult_dev.detach().float().reshape(1).contiguous()
        ctx.modifier, ctx.row0_mult, ctx.has_M, ctx.has_sel = float(modifier), (1.0 if mult_dev is not None else float(row0_mult)), M is not None, selected is not None
        ctx.log_scaling, ctx.has_opacity = int(bool(log_scaling)), opacity is not None
        return cov if opacity is None else (cov, opacity)

    @staticmethod
    def backward(ctx, dcov, dopacity=None):
        L = _lib.load()
        scaling, rotation, Mc, sel, opacity = ctx.saved_tensors
        Mc = Mc if ctx.has_M else None
        sel = sel if ctx.has_sel else None
        N = scaling.shape[0]
        dcov = torch.zeros((N, 6), device=scaling.device) if dcov is None else dcov.float().contiguous()
        ds, dr = torch.empty_like(scaling), torch.empty_like(rotation)
        dM = torch.empty(9, device=scaling.device) if (ctx.has_M and ctx.needs_input_grad[2]) else None
        dM_scratch = torch.empty(L.egs_cov3d_dm_scratch_floats(N), device=scaling.device) if dM is not None else None
        o = do = do_raw = None
        if ctx.has_opacity:
            o = opacity
            do = torch.zeros_like(o) if dopacity is None else dopacity.float().contiguous()
            do_raw = torch.empty_like(o)
        with _hip.device_ctx(scaling.device):
            _lib.check(L.egs_cov3d_backward(N, _p(scaling), ctx.log_scaling, ctx.modifier, _p(rotation), _p(Mc), _p(sel), ctx.row0_mult,
                                            _p(ctx.mult_dev), _p(dcov), _p(ds), _p(dr), _p(dM), _p(dM_scratch), _p(o), _p(do), _p(do_raw), _stream(scaling.device)))
        return ds, dr, (None if dM is None else dM.view(3, 3)), None, None, None, None, do_raw


def covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
    return _Cov3D.apply(scaling, rotation, None, None, scaling_modifier, 1.0)


def covariance_from_log_scaling(log_scaling, scaling_modifier, rotation):
    """Same, fed with the RAW scaling parameters (GaussianModel._scaling): exp() and its derivative run inside the kernels,
    which saves the two elementwise launches of `get_scaling` per step.  For a reference GaussianModel:
        gaussians.get_covariance = lambda m=1: fused.covariance_from_log_scaling(gaussians._scaling, m, gaussians._rotation)"""
    return _Cov3D.apply(log_scaling, rotation, None, None, scaling_modifier, 1.0, True)


def covariance_and_opacity(log_scaling, scaling_modifier, rotation, opacity_raw):
    """(cov3D [N,6], opacity [N,1]) from the raw parameters in ONE launch each way: covariance_from_log_scaling plus the opacity
    activation sigmoid (gaussian_model.py:40) and its derivative.  render() uses it when the model offers
    `get_covariance_and_opacity(scaling_modifier)`:
        gaussians.get_covariance_and_opacity = lambda m=1: fused.covariance_and_opacity(gaussians._scaling, m, gaussians._rotation, gaussians._opacity)"""
    return _Cov3D.apply(log_scaling, rotation, None, None, scaling_modifier, 1.0, True, opacity_raw)


def object_selection(is_object, which_object, n, n_live=None):
    """(selected uint8[N] or None, row-0 gradient multiplier: python float or float32[1] device tensor) for the rows the reference's
    build_covariance_from_scaling_rotation_w_rot rotates -- including its [N,1]-index quirk (covariance.py): Gaussian 0 is rotated
    too whenever any Gaussian is selected, and its gradient is multiplied by (count + [0 selected]).  Evaluated on the device, no
    host read.  The result depends only on (is_object, which_object, n_live): callers may keep it across steps.
    n_live: a capacity-sized model's live row count -- rows beyond it are not Gaussians: never selected, never counted (the
    reference's model has exactly n_live rows)."""
    sel, mult = None, 1.0
    if n_live is not None and n_live < n:
        n_eff = int(n_live)
    else:
        n_eff = n
    if which_object is not None and is_object is not None:
        sel = (is_object.reshape(-1) == which_object)
        if n_eff < n:
            sel = sel.clone(); sel[n_eff:] = False
        if is_object.dim() == 2 and n_eff > 0:
            cnt = sel.sum()
            mult = (cnt + sel[0]).to(torch.float32).reshape(1)
            first = torch.logical_or(sel[0:1], (cnt > 0).reshape(1))
            sel = sel.clone(); sel[0:1] = first
        sel = sel.to(torch.uint8).contiguous()
    elif is_object is not None and is_object.dim() == 2 and n_eff > 0:
        mult = float(n_eff + 1)
    return sel, mult


def rotated_covariance_from_scaling_rotation(scaling, scaling_modifier, rotation, accum_R, is_object=None, which_object=None,
                                             rot_matrix=None, scaling_is_log=False, selection=None, opacity_raw=None):
    """`rot_matrix` (3x3, may require grad) is the trainable object rotation applied on top of accum_R during training
    (trainable_object_move.rot_L in the reference).  Keeps the reference's [N,1]-index quirk, see covariance.py.
    selection: a cached object_selection(is_object, which_object, N); opacity_raw: also return sigmoid(opacity_raw) from the
    same launch -> (cov3D, opacity)."""
    dev = scaling.device
    if accum_R is None:
        accum_R = torch.eye(3, device=dev)
    M = accum_R.to(dev).float()
    if rot_matrix is not None:
        M = rot_matrix @ M
    sel, mult = selection if selection is not None else object_selection(is_object, which_object, scaling.shape[0])
    return _Cov3D.apply(scaling, rotation, M, sel, scaling_modifier, mult, scaling_is_log, opacity_raw)


class _MovePoints(torch.autograd.Function):
    """xyz' = A xyz + b for the rows of `moved` (include/egs_raster.h egs_object_move_points / _backward)."""

    @staticmethod
    def forward(ctx, xyz, A12, moved, active_count):
        L = _lib.load()
        xyz, A = _need_hip(xyz, "xyz"), _need_hip(A12, "A12").reshape(12)
        N, dev = xyz.shape[0], xyz.device
        mv = None if moved is None else moved.reshape(-1).to(torch.uint8).contiguous()
        if mv is not None and (mv.numel() != N or mv.device != dev):
            raise RuntimeError("object_move_points: `moved` must hold one byte per row on the points' device")
        out = torch.empty_like(xyz)
        with _hip.device_ctx(dev):
            _lib.check(L.egs_object_move_points(N, _p(xyz), _p(A), _p(mv), _p(active_count), _p(out), _stream(dev)))
        ctx.save_for_backward(xyz, A, mv if mv is not None else torch.empty(0, device=dev))
        ctx.has_mask, ctx.active_count, ctx.A_shape = mv is not None, active_count, A12.shape
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        xyz, A, mv = ctx.saved_tensors
        mv = mv if ctx.has_mask else None
        N, dev = xyz.shape[0], xyz.device
        g = g.float().contiguous()
        dxyz = torch.empty_like(xyz) if ctx.needs_input_grad[0] else None
        dA = torch.empty(12, device=dev) if ctx.needs_input_grad[1] else None
        scratch = torch.empty(max(int(L.egs_object_motion_scratch_bytes(N)), 4), device=dev, dtype=torch.uint8) if dA is not None else None
        if dxyz is not None or dA is not None:
            with _hip.device_ctx(dev):
                _lib.check(L.egs_object_move_points_backward(N, _p(xyz), _p(A), _p(mv), _p(ctx.active_count), _p(g), _p(dxyz), _p(dA), _p(scratch),
                                                             _stream(dev)))
        return dxyz, (None if dA is None else dA.view(ctx.A_shape)), None, None


def object_move_points(xyz, A12, moved=None, active_count=None):
    """The placed positions [N,3] as a tensor: p' = A p + b for the rows of `moved` (the exact mask, None = every row), a bit-for-bit copy
    for the others and for rows at or beyond *active_count (int32[1] device tensor).  One launch each way instead of the reference's
    cat / matmul / slice / where (apply_T_xyz, gaussian_model.py:939-986); differentiable w.r.t. xyz and A12 (motion.ObjectMotion.compose),
    the pose gradient being a deterministic reduction.  For evaluation, the export of a posed frame and comparisons -- a render takes the
    motion as an input instead (renderer.render(object_motion=...)).  HIP tensors only; motion.move_points is the tensor expression."""
    return _MovePoints.apply(xyz, A12, moved, active_count)


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt, lambda_dssim, gate, running_sum=None, defer_value=False, raster_node=None, lossgrad=False):
        L = _lib.load()
        img, gt = _need_hip(img, "image"), _need_hip(gt, "gt")
        assert img.dim() == 3 and img.shape == gt.shape
        Cc, H, W = img.shape
        dev = img.device
        partial = torch.empty(L.egs_l1_ssim_partial_count(Cc, H, W), device=dev)
        maps = torch.empty((3, Cc, H, W), device=dev)
        loss = torch.empty((), device=dev)
        side = None
        if lossgrad and raster_node is not None and Cc == 3:
            # raster_lossgrad: the rasterizer's backward blend will compute this loss's image gradient itself; what the loss BACKWARD launch
            # used to carry for it (tile order, cleared accumulator, optimizer bookkeeping) rides in this forward launch instead
            from .rasterizer import backward_prologue_of
            side = backward_prologue_of(raster_node)
        with _hip.device_ctx(dev):
            if side is not None:
                _lib.check(L.egs_l1_ssim_forward_ex(Cc, H, W, _p(img), _p(gt), float(lambda_dssim), _p(partial), _p(maps[0]), _p(maps[1]),
                                                    _p(maps[2]), None if defer_value else _p(loss), None if defer_value else _p(running_sum),
                                                    C.byref(side), _stream(dev)))
            else:
                _lib.check(L.egs_l1_ssim_forward(Cc, H, W, _p(img), _p(gt), float(lambda_dssim), _p(partial), _p(maps[0]), _p(maps[1]),
                                                 _p(maps[2]), None if defer_value else _p(loss), None if defer_value else _p(running_sum), _stream(dev)))
        ctx.lossgrad = side is not None
        ctx.save_for_backward(img, gt, maps, gate if gate is not None else torch.empty(0))
        ctx.lam, ctx.has_gate = float(lambda_dssim), gate is not None
        ctx.deferred = (partial, loss, running_sum) if defer_value else None
        ctx.raster_node = raster_node
        return loss

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        img, gt, maps, gate = ctx.saved_tensors
        gate = gate.float().contiguous() if ctx.has_gate else None
        Cc, H, W = img.shape
        g = g.reshape(1)
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.float().contiguous()
        dimg = torch.empty_like(img)
        if ctx.lossgrad:
            # no launch here: the rasterizer backward that follows computes dL/dimage inside its blend kernel (include/egs_raster.h
            # egs_backward_lossgrad) -- bit-identical to what this launch would have written.  `dimg` goes back uninitialised and unread.
            lg = _lib.LossGrad()
            lg.image, lg.gt, lg.dm_dmu1, lg.dm_dexx, lg.dm_dexy = img.data_ptr(), gt.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr()
            lg.gate = gate.data_ptr() if gate is not None else None
            lg.upstream_grad, lg.lambda_dssim = g.data_ptr(), ctx.lam
            d = ctx.deferred
            if d:
                lg.deferred_partial_sums, lg.deferred_loss = d[0].data_ptr(), d[1].data_ptr()
                lg.loss_running_sum = d[2].data_ptr() if d[2] is not None else None
            # (the third element is how the rasterizer's backward recognises THIS tensor: anything autograd put between the two nodes -- a second
            # consumer of the image whose gradient was added, a hook that returned another tensor -- arrives as a different one and is refused
            # there instead of being silently dropped)
            ctx.raster_node.loss_grad = (lg, (img, gt, maps, gate, g, d), (dimg.data_ptr(), dimg._version))
            return dimg, None, None, None, None, None, None, None
        side = None
        if ctx.raster_node is not None:
            from .rasterizer import backward_prologue_of
            side = backward_prologue_of(ctx.raster_node)
        with _hip.device_ctx(img.device):
            d = ctx.deferred
            _lib.check(L.egs_l1_ssim_backward_ex(Cc, H, W, _p(img), _p(gt), ctx.lam, _p(g), _p(gate), _p(maps[0]), _p(maps[1]),
                                                 _p(maps[2]), _p(dimg), _p(d[0]) if d else None, _p(d[1]) if d else None,
                                                 _p(d[2]) if d else None, C.byref(side) if side is not None else None, _stream(img.device)))
        return dimg, None, None, None, None, None, None, None


class _L1SSIMPair(torch.autograd.Function):
    """(mean|img - gt|, mean SSIM(img, gt)) from one forward launch; one backward launch for both upstream scalars
    (include/egs_raster.h egs_l1_ssim_pair_forward / _backward)."""

    @staticmethod
    def forward(ctx, img, gt, raster_node=None):
        L = _lib.load()
        img, gt = _need_hip(img, "image"), _need_hip(gt, "gt")
        assert img.dim() == 3 and img.shape == gt.shape
        Cc, H, W = img.shape
        dev = img.device
        partial = torch.empty(L.egs_l1_ssim_partial_count(Cc, H, W), device=dev)
        maps = torch.empty((3, Cc, H, W), device=dev)
        vals = torch.empty(2, device=dev)
        ctx.raster_node = raster_node
        with _hip.device_ctx(dev):
            _lib.check(L.egs_l1_ssim_pair_forward(Cc, H, W, _p(img), _p(gt), _p(partial), _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(vals[0:1]),
                                                  _p(vals[1:2]), _stream(dev)))
        ctx.save_for_backward(img, gt, maps)
        return vals[0], vals[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        L = _lib.load()
        img, gt, maps = ctx.saved_tensors
        Cc, H, W = img.shape
        ups = torch.zeros(2, device=img.device) if (g_l1 is None or g_ssim is None) else None
        up = lambda g, k: (ups[k:k + 1] if g is None else g.reshape(1).float().contiguous())
        u1, u2 = up(g_l1, 0), up(g_ssim, 1)
        dimg = torch.empty_like(img)
        side = None
        if ctx.raster_node is not None:
            from .rasterizer import backward_prologue_of
            side = backward_prologue_of(ctx.raster_node)
        with _hip.device_ctx(img.device):
            _lib.check(L.egs_l1_ssim_pair_backward(Cc, H, W, _p(img), _p(gt), _p(u1), _p(u2), None, _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(dimg),
                                                   C.byref(side) if side is not None else None, _stream(img.device)))
        return dimg, None, None


def l1_and_ssim(image, gt, raster_prologue=True):
    """-> (mean |image - gt|, mean SSIM(image, gt)) as two differentiable scalars from ONE HIP launch each way: the reference's
    l1_loss(x, gt) and ssim(x, gt) (/root/reference/utils/loss_utils.py:57-58,79-107) when a loop combines them itself.
    raster_prologue: when `image` is the rasterizer's output itself, the backward launch also carries the preparation of the rasterizer's
    backward (as l1_ssim_loss(raster_prologue=True)): one launch less per iteration, results unchanged (a gradient hook on the image,
    the reference's hand mask, sits between the two backwards and is unaffected)."""
    node = None
    if raster_prologue:
        fn = image.grad_fn
        if fn is not None and getattr(fn, "egs_raster_node", False):
            node = fn
    return _L1SSIMPair.apply(image, gt, node)


def l1_ssim_loss(image, gt, lambda_dssim=0.2, grad_gate=None, running_sum=None, defer_value=False, raster_prologue=False, raster_lossgrad=False):
    """(1 - lambda) * mean|image - gt| + lambda * (1 - SSIM(image, gt)).  `grad_gate` [H,W] multiplies d loss / d image
    per pixel (the reference's `render_image.register_hook(lambda grad: grad * (1 - hand_mask))`).
    running_sum: optional device scalar the loss value is also added to (logging without a launch or a host read per iteration).
    defer_value=True: the returned tensor receives its value during backward() instead of right away -- one launch less per
    iteration, for steps whose loss is only read after the backward (graph.GraphedTrainStep).
    raster_prologue=True: see below -- one launch less per iteration when `image` is the rasterizer's output itself.
    raster_lossgrad=True (with raster_prologue, three channels, and a loss.backward() that is SURE to follow -- the optimizer bookkeeping of a
    fused Adam rides in the FORWARD launch then): this loss has no backward launch at all; the rasterizer's backward blend computes the image
    gradient from the maps this forward leaves, bit-identical to the launch it replaces (include/egs_raster.h egs_backward_lossgrad).  The
    gradient tensor autograd hands from this loss to the rasterizer is uninitialised memory: hooks on `image` must not read it (use grad_gate)."""
    if running_sum is not None:
        running_sum = _need_hip(running_sum, "running_sum")
    node = None
    if raster_prologue:
        # `image` straight from the rasterizer: this loss's backward launch also carries the preparation of the rasterizer's backward
        # (tile order, cleared accumulator, fused-optimizer bookkeeping; include/egs_raster.h egs_l1_ssim_backward_ex) in extra
        # workgroups, which otherwise is a launch of its own right after this one.  Results are the same either way.
        fn = image.grad_fn
        if fn is not None and getattr(fn, "egs_raster_node", False):
            node = fn
    return _L1SSIM.apply(image, gt, lambda_dssim, grad_gate, running_sum, defer_value, node, bool(raster_lossgrad and node is not None))


class _ObjectLoss(torch.autograd.Function):
    """The object stages' loss on (image, alpha): include/egs_raster.h egs_object_loss_forward[_ex] / egs_object_loss_backward_ex /
    egs_backward_object_lossgrad.  Two differentiable inputs, one forward launch, at most one backward launch."""

    @staticmethod
    def forward(ctx, img, alpha, gtm, mask, lambda_dssim, weights, gate, running_sum, terms, defer_value, raster_node, lossgrad):
        L = _lib.load()
        img, gtm = _need_hip(img, "image"), _need_hip(gtm, "gt")
        a, mask = _need_hip(alpha, "alpha"), _need_hip(mask, "obj_mask")
        assert img.dim() == 3 and img.shape == gtm.shape
        Cc, H, W = img.shape
        if a.numel() != H * W or mask.numel() != H * W:
            raise RuntimeError("object_stage_loss: alpha and obj_mask hold one value per pixel of the image ([1,H,W] or [H,W])")
        dev = img.device
        partial = torch.empty(L.egs_l1_ssim_partial_count(Cc, H, W) + L.egs_l1_ssim_partial_count(1, H, W), device=dev)
        apartial = partial[L.egs_l1_ssim_partial_count(Cc, H, W):]
        maps = torch.empty((3, Cc, H, W), device=dev)
        loss = torch.empty((), device=dev)
        ob = _lib.ObjectLoss()
        ob.alpha, ob.obj_mask, ob.alpha_partial_sums = a.data_ptr(), mask.data_ptr(), apartial.data_ptr()
        ob.lambda_image, ob.lambda_l1_alpha, ob.lambda_l2_alpha = float(weights[0]), float(weights[1]), float(weights[2])
        ob.terms = None if terms is None else terms.data_ptr()
        side = None
        if lossgrad and raster_node is not None and Cc == 3:
            # as _L1SSIM: the blend will compute BOTH gradients itself; what the loss backward launch carried for it rides in this forward
            from .rasterizer import backward_prologue_of
            side = backward_prologue_of(raster_node)
        with _hip.device_ctx(dev):
            _lib.check(L.egs_object_loss_forward_ex(Cc, H, W, _p(img), _p(gtm), float(lambda_dssim), _p(partial), _p(maps[0]), _p(maps[1]), _p(maps[2]),
                                                    None if defer_value else _p(loss), None if defer_value else _p(running_sum), C.byref(ob),
                                                    C.byref(side) if side is not None else None, _stream(dev)))
        ctx.lossgrad = side is not None
        ctx.save_for_backward(img, gtm, maps, a, mask, gate if gate is not None else torch.empty(0))
        ctx.lam, ctx.has_gate, ctx.ob, ctx.alpha_shape = float(lambda_dssim), gate is not None, ob, alpha.shape
        ctx.keep = (partial, terms)
        ctx.deferred = (partial, loss, running_sum) if defer_value else None
        ctx.raster_node = raster_node
        return loss

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        img, gtm, maps, a, mask, gate = ctx.saved_tensors
        gate = gate.float().contiguous() if ctx.has_gate else None
        Cc, H, W = img.shape
        g = g.reshape(1)
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.float().contiguous()
        dimg = torch.empty_like(img)
        dalpha = torch.empty(ctx.alpha_shape, device=img.device, dtype=torch.float32)
        d = ctx.deferred
        none = (None,) * 10
        if ctx.lossgrad:
            # no launch: the rasterizer backward that follows forms dL/dimage AND dL/dalpha inside its blend kernel (bit-identical to the
            # launch below).  Both tensors go back uninitialised and unread; the rasterizer recognises each by address and version.
            lg = _lib.LossGrad()
            lg.image, lg.gt, lg.dm_dmu1, lg.dm_dexx, lg.dm_dexy = img.data_ptr(), gtm.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr()
            lg.gate = gate.data_ptr() if gate is not None else None
            lg.upstream_grad, lg.lambda_dssim = g.data_ptr(), ctx.lam
            if d:
                lg.deferred_partial_sums, lg.deferred_loss = d[0].data_ptr(), d[1].data_ptr()
                lg.loss_running_sum = d[2].data_ptr() if d[2] is not None else None
            ctx.raster_node.loss_grad = (lg, (img, gtm, maps, gate, g, d, a, mask, ctx.keep), (dimg.data_ptr(), dimg._version), ctx.ob,
                                         (dalpha.data_ptr(), dalpha._version))
            return (dimg, dalpha) + none
        side = None
        if ctx.raster_node is not None:
            from .rasterizer import backward_prologue_of
            side = backward_prologue_of(ctx.raster_node)
        with _hip.device_ctx(img.device):
            _lib.check(L.egs_object_loss_backward_ex(Cc, H, W, _p(img), _p(gtm), ctx.lam, _p(g), _p(gate), _p(maps[0]), _p(maps[1]), _p(maps[2]),
                                                     _p(dimg), _p(dalpha), _p(d[0]) if d else None, _p(d[1]) if d else None, _p(d[2]) if d else None,
                                                     C.byref(ctx.ob), C.byref(side) if side is not None else None, _stream(img.device)))
        return (dimg, dalpha) + none


def object_stage_loss(image, alpha, gt, obj_mask, lambda_dssim=0.2, lambda_image=1.0, lambda_l1_alpha=0.0, lambda_l2_alpha=0.5, grad_gate=None,
                      running_sum=None, terms=None, defer_value=False, raster_prologue=False, raster_lossgrad=False, gt_premasked=False):
    """The loss of the stages that recover the object's motion (losses.object_stage_loss is its torch mirror;
    /root/reference/trainers/coarse_obj_pose.py:239-260, trainers/fine_obj.py:128-151):
        lambda_image * [(1 - lambda) L1 + lambda (1 - SSIM)](image, gt * obj_mask) + lambda_l1_alpha * mean|obj_mask - alpha|
            + lambda_l2_alpha * mean (obj_mask - alpha)^2
    One autograd node with two differentiable inputs, `image` [3,H,W] and `alpha` ([1,H,W] as the rasterizer returns it, or [H,W]): one
    HIP launch forward, one backward -- instead of the image loss plus five torch launches each way for the alpha terms.
    grad_gate [H,W] multiplies BOTH gradients per pixel: it replaces the reference's two hooks, `grad * (1 - hand_mask)` on the image and
    on alpha.  gt_premasked=True: `gt` already is gt * obj_mask (graph.pack_frame stores it so) -- no multiply here.
    terms: optional device float32[3] that receives (image loss, mean|m - alpha|, mean (m - alpha)^2), unweighted, whenever the value
    is assembled -- what the trainers log.  running_sum / defer_value / raster_prologue: as l1_ssim_loss.
    raster_lossgrad=True (image AND alpha straight from one rasterizer call, three channels, a backward that is sure to follow): no
    backward launch; the rasterizer's backward blend forms both gradients itself, bit-identical to that launch.  Both gradient tensors
    autograd hands on are uninitialised memory; the rasterizer's backward recognises each and refuses (RuntimeError) when the image
    or alpha has a second consumer or a hook that replaced the gradient, or when the depth output received a gradient.
    With both alpha weights 0 and lambda_image 1 the value and the image gradient are l1_ssim_loss's, bit for bit."""
    if running_sum is not None:
        running_sum = _need_hip(running_sum, "running_sum")
    if terms is not None and not (terms.is_cuda and terms.dtype == torch.float32 and terms.numel() == 3 and terms.is_contiguous()):
        raise RuntimeError("object_stage_loss: `terms` is a contiguous float32[3] tensor on the image's device")
    mask = obj_mask.detach()
    if mask.dtype != torch.float32:
        mask = mask.float()
    gtm = gt if gt_premasked else gt * mask
    node = None
    if raster_prologue:
        fn = image.grad_fn
        if fn is not None and getattr(fn, "egs_raster_node", False):
            node = fn
    lossgrad = bool(raster_lossgrad and node is not None and alpha.grad_fn is node)
    return _ObjectLoss.apply(image, alpha, gtm, mask, lambda_dssim, (lambda_image, lambda_l1_alpha, lambda_l2_alpha), grad_gate, running_sum, terms,
                             defer_value, node, lossgrad)


class _LabelBCE(torch.autograd.Function):
    """The label phase's loss (losses.label_bce_loss) as one node: the HIP forward (per-quadrant partial sums in a fixed order + a finishing
    launch, or deferred), and either the HIP backward launch or -- lossgrad -- no launch at all: the scalar colours-only blend of the label
    render in front forms the gradient itself (include/egs_raster.h egs_backward_label)."""

    @staticmethod
    def forward(ctx, img, mask, gate, running_sum, defer_value, raster_node, lossgrad):
        from . import _C
        img, mask = _need_hip(img, "image"), _need_hip(mask, "obj_mask")
        assert img.dim() == 3 and img.shape[0] == 3 and mask.numel() == img.shape[1] * img.shape[2]
        loss = torch.empty((), device=img.device)
        _, partial = _C.label_bce_forward(img, mask, loss=loss.view(1), running_sum=running_sum, defer_value=defer_value)
        ctx.save_for_backward(img, mask, gate if gate is not None else torch.empty(0))
        ctx.has_gate = gate is not None
        ctx.deferred = (partial, loss, running_sum) if defer_value else None
        ctx.partial = partial
        ctx.raster_node, ctx.lossgrad = raster_node, bool(lossgrad)
        return loss

    @staticmethod
    def backward(ctx, g):
        from . import _C
        img, mask, gate = ctx.saved_tensors
        gate = gate.float().contiguous() if ctx.has_gate else None
        g = g.reshape(1)
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.float().contiguous()
        d = ctx.deferred
        if ctx.lossgrad:
            # no launch here: the label render's backward blend forms dL/dx per pixel itself, and its last launch assembles a deferred value.
            # `dimg` goes back uninitialised and unread; the rasterizer's node refuses any other tensor in its place.
            dimg = torch.empty_like(img)
            st, keep = _C.label_loss_struct(img, mask, g, gate, ctx.partial, d[1].view(1) if d else None, d[2] if d else None)
            ctx.raster_node.label_loss = (st, keep, (dimg.data_ptr(), dimg._version))
            return dimg, None, None, None, None, None, None
        dimg = _C.label_bce_backward(img, mask, g, gate, d[0] if d else None, d[1].view(1) if d else None, d[2] if d else None)
        return dimg, None, None, None, None, None, None


def label_bce_loss(image, obj_mask, grad_gate=None, running_sum=None, defer_value=False, raster_lossgrad=False):
    """BCEWithLogitsLoss()(image.mean(0, keepdim=True), obj_mask) for the label render `image` [3,H,W] (losses.label_bce_loss is the torch mirror;
    /root/reference/trainers/train_static.py:104-109).  `grad_gate` [H,W] multiplies d loss / d mean per pixel -- the reference's
    `render_label.register_hook(lambda g: g * (1 - hand_mask))`.  running_sum / defer_value: as l1_ssim_loss.
    raster_lossgrad=True (when `image` is get_render_label(..., scalar=True)'s output itself and loss.backward() is sure to follow): this loss has
    no backward launch; the label render's backward blend forms the gradient from the image, the mask and the gate.  The gradient tensor handed
    to the rasterizer is uninitialised memory, and the rasterizer's node refuses any other gradient contribution to the image."""
    if running_sum is not None:
        running_sum = _need_hip(running_sum, "running_sum")
    node = None
    if raster_lossgrad:
        fn = image.grad_fn
        if fn is not None and getattr(fn, "egs_label_node", False):
            node = fn
    m = obj_mask.reshape(image.shape[-2], image.shape[-1])
    return _LabelBCE.apply(image, m, grad_gate, running_sum, defer_value, node, node is not None)


class _OpacityEntropy(torch.autograd.Function):
    """weight * (mean entropy of the visible opacities) over the stand-alone kernels (include/egs_raster.h egs_opacity_entropy_forward /
    _backward): a deterministic reduction forward (two launches), one launch backward."""

    @staticmethod
    def forward(ctx, opacity, radii, weight, logit, active_count):
        from . import _C
        o = _need_hip(opacity, "opacity")
        term = _C.EntropyTerm(weight, o.device)
        _C.opacity_entropy_forward(o.detach(), radii, term, logit=logit, active_count=active_count)
        ctx.save_for_backward(o, radii)
        ctx.term, ctx.logit, ctx.active_count, ctx.shape = term, bool(logit), active_count, opacity.shape
        ctx.n_vis = term.n_vis
        return (term.value * term.weight).reshape(())

    @staticmethod
    def backward(ctx, g):
        from . import _C
        o, radii = ctx.saved_tensors
        ctx.term.upstream = g.detach().reshape(1).float().contiguous()
        d = _C.opacity_entropy_backward(o.detach(), radii, ctx.term, logit=ctx.logit, active_count=ctx.active_count)
        return d.view(ctx.shape), None, None, None, None


def opacity_entropy(opacity, radii, weight=1.0, logit=False, active_count=None):
    """weight * mean over the visible Gaussians (radii > 0) of -o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10): the static stages' entropy
    regulariser (losses.opacity_entropy is the torch mirror; /root/reference/trainers/train_static.py:97-102 adds it with weight 0.1).
    opacity: [P] or [P,1], the activated opacities -- or, with logit=True, the raw parameter (`_opacity`), activated inside the kernels; the
    gradient comes back w.r.t. what was given.  radii: the render's int32[P].  weight: a float or a float32 device scalar (a constant of the
    loss).  active_count: int32[1] device tensor of a capacity-sized model -- rows at or beyond it are skipped whatever they hold.
    Three HIP launches in all instead of the expression's dozen each way; deterministic (no float atomics).  No visible Gaussian: NaN and a
    zero gradient.  For a trainer that does not fuse its optimizer; one that does asks render(opacity_entropy=) for the term instead."""
    return _OpacityEntropy.apply(opacity, radii, weight, logit, active_count)


EVAL_ROW_WORDS = 4      # include/egs_raster.h egs_eval_row as int64 words: sse, ssim_sum (float64 bits), clipped, instances


def eval_rows(capacity, device):
    """(rows int64[capacity, 4] zeroed, cursor int32[1] = 0) for eval_metrics: the caller-owned result array and the device-side frame index."""
    return torch.zeros((int(capacity), EVAL_ROW_WORDS), dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int32, device=device)


def eval_metrics(image, gt, keep=None, rows=None, cursor=None, overflow=None, out8=False):
    """The evaluation figures of one frame by the HIP kernel (include/egs_raster.h egs_eval_metrics; losses.eval_metrics is the torch statement
    of the same definition): the squared error of the 8-bit images over the kept pixels and the SSIM sum of the masked 8-bit images.
    image, gt: [C,H,W], C = 1 or 3; keep: [H,W] (1 - hand mask; binary by contract, thresholded at 0.5) or None.
    rows, cursor: eval_rows(capacity, device) -- the kernel writes row cursor[0] and advances the cursor on the device, so a sweep (or a
    replayed graph) fills one array and the host reads it ONCE; a full array is left untouched while the cursor still counts.  None: a fresh
    one-row array.  overflow: a _C.StepGuard's `overflow` words of the forward that rendered `image`; they travel in the row.
    out8: also the quantised images, uint8[C,H,W] each, unmasked -- what goes into a PNG.
    Does not synchronise.  -> dict(rows, cursor, q_image, q_gt) of device tensors (the last two None without out8); evaluate.decode_rows reads rows.
    HIP tensors only."""
    L = _lib.load()
    img, g = _need_hip(image.detach(), "image"), _need_hip(gt.detach(), "gt")
    if img.dim() != 3 or img.shape != g.shape or img.shape[0] not in (1, 3):
        raise RuntimeError("eval_metrics: image and gt are [C,H,W] tensors of one shape, C = 1 or 3")
    Cc, H, W = img.shape
    dev = img.device
    k = None
    if keep is not None:
        k = _need_hip(keep.detach(), "keep")
        if k.numel() != H * W:
            raise RuntimeError("eval_metrics: keep holds one value per pixel ([H,W])")
    if (rows is None) != (cursor is None):
        raise RuntimeError("eval_metrics: rows and cursor go together (fused.eval_rows)")
    if rows is None:
        rows, cursor = eval_rows(1, dev)
    if not (rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[1] == EVAL_ROW_WORDS and rows.is_contiguous()
            and cursor.is_cuda and cursor.dtype == torch.int32 and cursor.numel() == 1):
        raise RuntimeError("eval_metrics: rows is a contiguous int64[capacity, 4] tensor and cursor an int32[1] tensor on the image's device")
    if overflow is not None and not (overflow.is_cuda and overflow.dtype == torch.int32 and overflow.numel() == 2 and overflow.is_contiguous()):
        raise RuntimeError("eval_metrics: overflow is a StepGuard's int32[2] device tensor")
    partial = torch.empty(max(int(L.egs_eval_metrics_partial_bytes(Cc, H, W)), 8), dtype=torch.uint8, device=dev)
    q_img = torch.empty((Cc, H, W), dtype=torch.uint8, device=dev) if out8 else None
    q_gt = torch.empty((Cc, H, W), dtype=torch.uint8, device=dev) if out8 else None
    with _hip.device_ctx(dev):
        _lib.check(L.egs_eval_metrics(Cc, H, W, _p(img), _p(g), _p(k), _p(overflow), _p(partial), _p(q_img), _p(q_gt), _p(rows), int(rows.shape[0]),
                                      _p(cursor), _stream(dev)))
    return dict(rows=rows, cursor=cursor, q_image=q_img, q_gt=q_gt)


LPIPS_ROW_WORDS = 6     # a row of include/egs_raster.h egs_lpips_forward as float64 words: tap_1 .. tap_5, their sum


def lpips_rows(capacity, device):
    """(rows float64[capacity, 6] zeroed, cursor int32[1] = 0) for lpips.LPIPS: the caller-owned result array and the device-side frame index."""
    return torch.zeros((int(capacity), LPIPS_ROW_WORDS), dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.int32, device=device)


MASK_ROW_WORDS = 6      # include/egs_raster.h egs_mask_row as int64 words: predicted, target, intersection, kept, clipped, instances


def mask_rows(n, dev):
    """(rows int64[n, 6] zeroed, cursor int32[1] = 0) for label_mask: the caller-owned result array and the device-side frame index."""
    return torch.zeros((int(n), MASK_ROW_WORDS), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)


def _mask_plane(t, name, H=None, W=None):
    """A mask as a contiguous float32 [H,W] tensor on its HIP device ([1,H,W] and [H,W] are both accepted; other types are converted first)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: fused HIP op has no CPU path (use egogaussian_amd.losses)")
    t = t.detach()
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 or (H is not None and tuple(t.shape) != (H, W)):
        raise RuntimeError(f"{name}: one value per pixel, [H,W] or [1,H,W]" + ("" if H is None else f" with H, W = {H}, {W}") + f"; got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def label_mask(image, threshold=0.5, target=None, keep=None, rows=None, cursor=None, overflow=None, mask=True, out=None):
    """The predicted object mask of one label render and its counts against the dataset's mask, by the HIP kernel (include/egs_raster.h
    egs_label_mask; losses.label_mask is the torch statement): set = ((c0 + c1) + c2) / 3 > threshold; the mask holds 255 / 0 for EVERY
    pixel, the counts -- predicted, target (target >= 0.5), intersection, kept -- run over the pixels with keep >= 0.5 (None: all).
    image: [3,H,W]; target, keep: [H,W] or [1,H,W] or None.  rows, cursor: mask_rows(capacity, device) -- the kernel writes row cursor[0] and
    advances the cursor on the device (a full array is left untouched while the cursor still counts); None: a fresh one-row array.
    overflow: a _C.StepGuard's `overflow` words of the forward that rendered `image`; they travel in the row.
    mask=False: no mask bytes are written; out: a contiguous uint8[H,W] tensor to write them into.
    Does not synchronise.  -> dict(rows, cursor, mask8) of device tensors.  HIP tensors only."""
    L = _lib.load()
    img = _need_hip(image.detach(), "image")
    if img.dim() != 3 or img.shape[0] != 3:
        raise RuntimeError("label_mask: image is a [3,H,W] label render")
    _, H, W = img.shape
    dev = img.device
    t = None if target is None else _mask_plane(target, "target", H, W)
    k = None if keep is None else _mask_plane(keep, "keep", H, W)
    if (rows is None) != (cursor is None):
        raise RuntimeError("label_mask: rows and cursor go together (fused.mask_rows)")
    if rows is None:
        rows, cursor = mask_rows(1, dev)
    if not (rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[1] == MASK_ROW_WORDS and rows.is_contiguous()
            and cursor.is_cuda and cursor.dtype == torch.int32 and cursor.numel() == 1):
        raise RuntimeError("label_mask: rows is a contiguous int64[capacity, 6] tensor and cursor an int32[1] tensor on the image's device")
    if overflow is not None and not (overflow.is_cuda and overflow.dtype == torch.int32 and overflow.numel() == 2 and overflow.is_contiguous()):
        raise RuntimeError("label_mask: overflow is a StepGuard's int32[2] device tensor")
    if out is not None:
        if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (H, W) and out.is_contiguous()):
            raise RuntimeError("label_mask: out is a contiguous uint8[H,W] tensor on the image's device")
        m8 = out
    else:
        m8 = torch.empty((H, W), dtype=torch.uint8, device=dev) if mask else None
    partial = torch.empty(max(int(L.egs_label_mask_partial_bytes(H, W)), 16), dtype=torch.uint8, device=dev)
    with _hip.device_ctx(dev):
        _lib.check(L.egs_label_mask(H, W, _p(img), float(threshold), _p(t), _p(k), _p(overflow), _p(partial), _p(m8), _p(rows), int(rows.shape[0]),
                                    _p(cursor), _stream(dev)))
    return dict(rows=rows, cursor=cursor, mask8=m8)


def interaction_gate(hand_mask, obj_mask=None, dilate_size=None, out=None):
    """The background stage's gradient gate by the HIP kernel (include/egs_raster.h egs_interaction_gate; losses.interaction_gate is the torch
    statement): 1 - dilate_k(hand_mask | obj_mask), float32 [H,W], 1 where the image gradient passes.  A pixel is set when either mask is
    non-zero there (torch.logical_or's rule); dilate_size = k (odd, 1..31; None: k = 1, the plain OR) is the reference's
    conv2d(ones(k, k), padding = k // 2) > 0.  Masks: [H,W] or [1,H,W], any type (converted to float32 first).
    out: a float32 tensor of H*W elements to write into -- e.g. the `gate` segment of a graph.pack_frame frame (a view; 4-byte alignment is
    enough).  Does not synchronise.  HIP tensors only."""
    L = _lib.load()
    a = _mask_plane(hand_mask, "hand_mask")
    H, W = a.shape
    b = None if obj_mask is None else _mask_plane(obj_mask, "obj_mask", H, W)
    k = 1 if dilate_size is None else int(dilate_size)
    if k < 1 or k > 31 or k % 2 == 0:
        raise ValueError(f"interaction_gate: dilate_size must be odd and within 1..31, got {dilate_size}")
    dev = a.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.numel() == H * W and out.is_contiguous()):
        raise RuntimeError("interaction_gate: out is a contiguous float32 tensor (or view) of H*W elements on the masks' device")
    with _hip.device_ctx(dev):
        _lib.check(L.egs_interaction_gate(H, W, _p(a), _p(b), k, _p(out), _stream(dev)))
    return out
