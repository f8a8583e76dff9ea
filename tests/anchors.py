"""Float64 anchors for the three streaming kernels most of the suite compares with bit for bit: the Adam step (adam.hip), the covariance
producer (cov3d.hip) and the image loss (loss.hip; its two-value form, fused.l1_and_ssim, in the last section).  Input builders, float64 references, float32 CPU yardsticks and the checks themselves;
the GPU tests (tests/test_gpu_anchor_*.py) hand the kernels' outputs to these checks, tests/test_anchors_cpu.py hands them the yardsticks
and deliberately wrong variants.  No bar in here comes from a kernel's own output: each is derived where it is defined, taken from
tests/common.py, or a multiple of what the float32 CPU formulation of the same operation is away from float64 on the same inputs."""
import numpy as np
import torch

from tests.common import ROW_Q_FACTOR, row_errors, row_rule

U = 2.0 ** -24                     # float32 unit roundoff


def f32w(x):
    """A Python float as the C ABI carries it: rounded to float32, widened back."""
    return float(np.float32(x))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


# ================================================================ Adam ================================================================
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-15          # what the training setup passes (optim.py)
# |g| = 10^[lo, hi]; `step` is the step TAKEN; `zero_state`: from exp_avg = exp_avg_sq = 0.  g^2 is a normal float32 everywhere (|g| >= 1e-15).
ADAM_REGIMES = {
    "ordinary": dict(lo=-3.0, hi=1.0, step=7, lr=1.6e-4, zero_state=False),
    "small": dict(lo=-14.0, hi=-6.0, step=7, lr=1.6e-4, zero_state=False),
    "wide": dict(lo=-15.0, hi=2.0, step=7, lr=1.6e-4, zero_state=False),
    "late": dict(lo=-3.0, hi=1.0, step=30000, lr=1.6e-6, zero_state=False),
    "first": dict(lo=-3.0, hi=1.0, step=1, lr=1.6e-4, zero_state=True),
}
ADAM_DOUBLE_BETA_DISTANCE = abs(f32w(ADAM_BETAS[1]) - ADAM_BETAS[1]) / (1.0 - ADAM_BETAS[1])     # 1.29e-5, see adam_double_beta_check


def _log_uniform(rng, n, lo, hi):
    return (10.0 ** rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def adam_case(regime, n=20011, seed=0):
    """One step from a prescribed state: g (one element in seven exactly zero), exp_avg, exp_avg_sq as float32 arrays; p = 0 before the
    step, so the stored p IS the rounded update.  exp_avg has the sign of g: the bar on p is relative to the update, i.e. it assumes that
    b1 m + (1 - b1) g does not cancel (with opposite signs the update's relative error is unbounded in ANY float32 evaluation; the
    trajectory check has mixed signs and is measured against a float32 yardstick instead)."""
    r = ADAM_REGIMES[regime]
    rng = np.random.default_rng(seed + 1000 * sorted(ADAM_REGIMES).index(regime))
    g = _log_uniform(rng, n, r["lo"], r["hi"])
    g[::7] = 0.0
    if r["zero_state"]:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = np.abs(_log_uniform(rng, n, r["lo"], r["hi"])) * np.where(g != 0, np.sign(g), rng.choice([-1.0, 1.0], n)).astype(np.float32)
        v = _log_uniform(rng, n, r["lo"], r["hi"]) ** 2
    return dict(g=g, m=m.astype(np.float32), v=v.astype(np.float32), step=r["step"], lr=r["lr"], n=n)


def adam64(p, g, m, v, step, lr, betas=ADAM_BETAS, eps=ADAM_EPS, widen=True):
    """The header of adam.hip in float64.  widen: betas, eps and lr as the C ABI carries them (float32-rounded) -- the kernel is
    self-consistent in those, its bias corrections use the same values; widen=False: the caller's doubles (adam_double_beta_check)."""
    b1, b2 = (f32w(betas[0]), f32w(betas[1])) if widen else betas
    eps, lr = (f32w(eps), f32w(lr)) if widen else (eps, lr)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v


def _fma32(a, b, c):
    """Round-of-exact a b + c for float32 operands: the product of two float32 is exact in float64; the sum is rounded to float64 and then
    to float32 (a double rounding that differs from a true fma only when the float64 sum lands within 2^-29 ulp of a float32 tie)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam32(p, g, m, v, step, lr, betas=ADAM_BETAS, eps=ADAM_EPS, fault=None):
    """The same formula evaluated in float32 numpy, one rounding per operation, the two moment updates as fused multiply-adds and the two
    coefficients computed in double and rounded once -- written from the formula, not from the kernel.  It is the evidence that the
    single-step bars leave room: it has to stay under HALF of each (tests/test_anchors_cpu.py).
    fault: 'no_bias_correction' | 'b2_for_one_minus_b2' | 'eps_in_sqrt' -- deliberately wrong variants the checks have to catch."""
    f = np.float32
    b1, b2, e = f(betas[0]), f(betas[1]), f(eps)
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    m = _fma32(f(1) - b1, g - m, m)
    v = _fma32(b2 if fault == "b2_for_one_minus_b2" else f(1) - b2, g * g, b2 * v)
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    if fault == "no_bias_correction":
        bc1 = bc2 = 1.0
    ss, ib = f(float(f(lr)) / bc1), f(1.0 / np.sqrt(bc2))
    den = np.sqrt(v * ib * ib + e) if fault == "eps_in_sqrt" else np.sqrt(v) * ib + e
    p = p - ss * (m / den)
    return p.astype(f), m, v


def check_adam_step(p, m, v, case, p_in=None, frac=1.0, what=""):
    """One step against adam64 (u = 2^-24):  |m - m64| <= 4u max(|m_in|, |g|),  |v - v64| <= 4u v64,  |p - p64| <= 16u |p64|  (p_in = 0).
    Where they come from: m = fma(1 - b1, g - m, m) is two roundings, the first relative to |g - m| <= 2 max(|m_in|, |g|) and scaled by
    1 - b1; v = fma(1 - b2, g g, b2 v) is three roundings of non-negative terms; the update is sqrt (which halves v's error), multiply,
    add, divide, multiply, with m's error (<= 2u of itself when m_in and g agree in sign, adam_case) and two coefficients rounded once.
    frac: the fraction of each bar the subject gets (0.5 for the emulation).  -> the largest error of each kind in units of u."""
    g, m_in = case["g"].astype(np.float64), case["m"].astype(np.float64)
    p0 = np.zeros_like(g) if p_in is None else np.asarray(p_in, np.float64)
    p64, m64, v64 = adam64(p0, g, m_in, case["v"], case["step"], case["lr"])
    p, m, v = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (p, m, v))
    scale_m = np.maximum(np.abs(m_in), np.abs(g))
    upd64 = p64 - p0
    fig, fails = {}, []
    for name, err, unit, k in (("m", np.abs(m - m64), scale_m, 4.0), ("v", np.abs(v - v64), v64, 4.0), ("p", np.abs(p - p64), np.abs(upd64), 16.0)):
        nz = unit > 0
        fig[name] = float((err[nz] / unit[nz]).max() / U) if nz.any() else 0.0
        over = err > frac * k * U * unit
        if over.any():
            i = int(np.argmax(err - frac * k * U * unit))
            fails.append(f"{name}: {int(over.sum())} of {err.size} elements over {frac * k:g}u of their unit (worst {fig[name]:.2f}u; element {i}: g {g[i]:.9e}, "
                         f"m_in {m_in[i]:.9e}, v_in {case['v'][i]:.9e}, got {(p, m, v)['pmv'.index(name)][i]:.9e}, float64 {(p64, m64, v64)['pmv'.index(name)][i]:.9e})")
    assert not fails, f"{what}: " + "; ".join(fails)
    return fig


def adam_double_beta_check(v, case):
    """The float64 reference above uses the float32-rounded betas.  How far that is from Adam with the caller's double betas is known:
    v' = b2 v + (1 - b2) g^2 moves by |b2f - b2| |v - g^2| <= |b2f - b2| max(v, g^2) <= |b2f - b2| v' / (1 - b2), i.e.
    |dv| / v <= |b2f - b2| / (1 - b2) = 1.29e-5 for b2 = 0.999.  Asserted once, at twice that figure (the kernel's own 4u on top is 2e-7).
    -> the measured distance."""
    _, _, vd = adam64(np.zeros_like(case["g"]), case["g"], case["m"], case["v"], case["step"], case["lr"], widen=False)
    v = np.asarray(v, np.float64).reshape(-1)
    nz = vd > 0
    d = float((np.abs(v - vd)[nz] / vd[nz]).max())
    assert d <= 2.0 * ADAM_DOUBLE_BETA_DISTANCE, f"exp_avg_sq is {d:.3e} from Adam with double betas; the float32 rounding of b2 explains {ADAM_DOUBLE_BETA_DISTANCE:.3e}"
    return d


ADAM_TRAJ_STEPS, ADAM_TRAJ_TENSORS, ADAM_TRAJ_NUMEL, ADAM_TRAJ_ZEROS = 200, 4, 5000, 0.3


def adam_trajectory_inputs(regime, seed=0):
    """200 steps of four tensors of 5 000 elements, gradients redrawn every step (mixed signs, 30 % exactly zero), from the regime's start:
    p = 0, the prescribed state of adam_case (zero for 'first') and the regime's step number."""
    r = ADAM_REGIMES[regime]
    rng = np.random.default_rng(seed + 77 + 1000 * sorted(ADAM_REGIMES).index(regime))
    T, K, n = ADAM_TRAJ_STEPS, ADAM_TRAJ_TENSORS, ADAM_TRAJ_NUMEL
    g = _log_uniform(rng, T * K * n, r["lo"], r["hi"]).reshape(T, K, n)
    g[rng.random((T, K, n)) < ADAM_TRAJ_ZEROS] = 0.0
    if r["zero_state"]:
        m, v = np.zeros((K, n), np.float32), np.zeros((K, n), np.float32)
    else:
        m = _log_uniform(rng, K * n, r["lo"], r["hi"]).reshape(K, n)
        # a state Adam can be in: sqrt(exp_avg_sq) = 1 .. 10 |exp_avg| (an exp_avg_sq unrelated to exp_avg makes single updates of 1e13 lr,
        # and |p - p64| would then measure those few elements only)
        v = ((np.abs(m) * (10.0 ** rng.uniform(0.0, 1.0, (K, n))).astype(np.float32)) ** 2).astype(np.float32)
    return dict(g=g, m=m, v=v, step0=r["step"] - 1, lr=r["lr"], sigma_g=float(np.sqrt(np.mean(g.astype(np.float64) ** 2))))


def adam_trajectory64(inp):
    p, m, v = np.zeros(inp["m"].shape), inp["m"].astype(np.float64), inp["v"].astype(np.float64)
    for t in range(inp["g"].shape[0]):
        p, m, v = adam64(p, inp["g"][t], m, v, inp["step0"] + 1 + t, inp["lr"])
    return p, m, v


def adam_trajectory_numpy32(inp, fault=None):
    p, m, v = np.zeros(inp["m"].shape, np.float32), inp["m"], inp["v"]
    for t in range(inp["g"].shape[0]):
        p, m, v = adam32(p, inp["g"][t], m, v, inp["step0"] + 1 + t, inp["lr"], fault=fault)
    return p, m, v


def adam_trajectory_optimizer(inp, make_optimizer, device="cpu"):
    """The trajectory through an optimizer object: make_optimizer(params, lr) -> optimizer.  The state is set through optimizer.state the
    way the densification code does it.  -> (p, m, v) as numpy [K, n]."""
    K = inp["m"].shape[0]
    params = [torch.nn.Parameter(torch.zeros(inp["m"].shape[1], device=device)) for _ in range(K)]
    opt = make_optimizer(params, inp["lr"])
    for k, p in enumerate(params):
        opt.state[p] = {"step": torch.tensor(float(inp["step0"])), "exp_avg": torch.tensor(inp["m"][k], device=device),
                        "exp_avg_sq": torch.tensor(inp["v"][k], device=device)}
    g = torch.tensor(inp["g"], device=device)
    for t in range(g.shape[0]):
        for k, p in enumerate(params):
            p.grad = g[t, k]
        opt.step()
    out = lambda f: np.stack([f(p).detach().cpu().numpy() for p in params])
    return out(lambda p: p), out(lambda p: opt.state[p]["exp_avg"]), out(lambda p: opt.state[p]["exp_avg_sq"])


def torch_adam32(params, lr):
    """The yardstick: torch.optim.Adam in float32 with the betas / eps / lr the C ABI carries."""
    return torch.optim.Adam(params, lr=f32w(lr), betas=(f32w(ADAM_BETAS[0]), f32w(ADAM_BETAS[1])), eps=f32w(ADAM_EPS), foreach=False)


def adam_trajectory_stats(pmv, ref64, sigma_g):
    """Per element |v - v64| / v64, |m - m64| / sigma_g, |p - p64| -> {name: (q50, q90, max)}."""
    (p, m, v), (p64, m64, v64) = pmv, ref64
    e = {"v": np.abs(v - v64) / v64, "m": np.abs(m - m64) / sigma_g, "p": np.abs(p - p64)}
    return {k: tuple(float(x) for x in (*np.quantile(a, [0.5, 0.9]), a.max())) for k, a in e.items()}


def check_adam_trajectory(subject, yardstick, what=""):
    """q50, q90 and max of each of the three measures: subject <= ROW_Q_FACTOR x the float32 yardstick's."""
    fails = [f"{k} {q}: {s:.3e} > {ROW_Q_FACTOR:g} x {y:.3e}" for k in ("v", "m", "p") for q, s, y in zip(("q50", "q90", "max"), subject[k], yardstick[k])
             if not s <= ROW_Q_FACTOR * y]
    assert not fails, f"{what}: " + "; ".join(fails)
    return "; ".join(f"{k} q50 {subject[k][0]:.2e} ({yardstick[k][0]:.2e}) q90 {subject[k][1]:.2e} ({yardstick[k][1]:.2e}) max {subject[k][2]:.2e} ({yardstick[k][2]:.2e})"
                     for k in ("v", "m", "p"))


# ========================================================= covariance producer =========================================================
COV_FAMILIES = ("bench", "anisotropic", "needles", "quat_norms", "near_identity", "half_turns", "opacity_logits")
COV_VARIANTS = ("plain", "modifier", "selection", "rot_matrix", "opacity")
COV_MODIFIER = f32w(1.3)           # the modifier crosses the C ABI as a float: every side gets the float32 value
COV_VALUE_BAR = 4e-6               # per row, relative to the row's largest entry: the float32 torch form's worst case over the seven families
                                   # (1.2e-6, tests/test_anchors_cpu.py re-measures it) x ROW_Q_FACTOR, rounded up
SIGMOID_BAR = 4.0 * U


def cov_inputs(family, N=4096, seed=0):
    """float32 CPU tensors: raw log-scales [N,3], quaternions [N,4], opacity logits [N,1], the weights of the scalar the gradients are taken
    of (w [N,6], wo [N,1]), an object mask [N] (40 %), the accumulated rotation A and the trainable one Rt (orthonormal)."""
    gen = torch.Generator().manual_seed(seed * 100 + COV_FAMILIES.index(family))
    rn = lambda *s: torch.randn(*s, generator=gen)
    raw, q, o = rn(N, 3) * 0.7 - 3.0, rn(N, 4), rn(N, 1) * 2.0
    if family == "anisotropic":
        raw = torch.rand(N, 3, generator=gen) * 12.0 - 10.0
    elif family == "needles":
        raw = torch.tensor([0.0, -9.0, -9.0]) + 0.1 * rn(N, 3)
    elif family == "quat_norms":
        q = q / q.norm(dim=1, keepdim=True) * 10.0 ** (torch.rand(N, 1, generator=gen) * 6.0 - 3.0)
    elif family == "near_identity":
        q = torch.cat([torch.ones(N, 1), 1e-4 * rn(N, 3)], dim=1)
    elif family == "half_turns":
        v = rn(N, 3)
        q = torch.cat([(torch.rand(N, 1, generator=gen) * 2.0 - 1.0) * 1e-6, v / v.norm(dim=1, keepdim=True)], dim=1)
    elif family == "opacity_logits":
        o = torch.rand(N, 1, generator=gen) * 24.0 - 12.0
    is_object = (torch.rand(N, generator=gen) < 0.4).float()
    A = torch.linalg.qr(rn(3, 3))[0]
    Rt = torch.linalg.qr(rn(3, 3))[0]
    return dict(raw=raw.float(), quat=q.float(), opac=o.float(), w=rn(N, 6), wo=rn(N, 1), is_object=is_object, A=A, Rt=Rt, N=N)


def cov_head(inp, n):
    """The first n Gaussians of an input set (the per-Gaussian arrays cut, the matrices kept)."""
    return {k: (v[:n] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == inp["N"] else v) for k, v in inp.items()} | {"N": n}


def cov_eval(variant, inp, impl, dtype=torch.float32, device="cpu", is_object=None, terms=False):
    """One variant through `impl` ('fused': the HIP producer, 'torch': covariance.py in `dtype`) and the gradients of
    sum(w cov) [+ sum(wo opacity)] -> numpy dict: cov, opacity, d_raw, d_quat, d_opac, dM (the trainable rotation's gradient) -- those that exist.
    is_object: overrides inp['is_object'] (the [N,1] form carries the reference's duplicated-index quirk).
    terms: also 'dM_terms' = sum over the Gaussians of |each Gaussian's contribution| to every dM entry (float64 runs: the unit of the
    rounding floor of a float32 sum)."""
    T = lambda a: a.detach().clone().to(device=device, dtype=dtype)          # (a float32 CPU run must not turn the inputs themselves into leaves)
    raw, q, o = (T(inp[k]).requires_grad_(True) for k in ("raw", "quat", "opac"))
    w, wo, A = T(inp["w"]), T(inp["wo"]), T(inp["A"])
    io = T(inp["is_object"] if is_object is None else is_object)
    Rt = T(inp["Rt"]).requires_grad_(True) if variant == "rot_matrix" else None
    mod = COV_MODIFIER if variant == "modifier" else 1.0
    op, cap = None, {}
    if impl == "fused":
        from egogaussian_amd import fused as F
        if variant in ("plain", "modifier"):
            cov = F.covariance_from_log_scaling(raw, mod, q)
        elif variant == "opacity":
            cov, op = F.covariance_and_opacity(raw, mod, q, o)
        else:
            cov = F.rotated_covariance_from_scaling_rotation(raw, mod, q, A, io, 1, rot_matrix=Rt, scaling_is_log=True)
    else:
        from egogaussian_amd import covariance as R
        s = torch.exp(raw)
        if variant in ("plain", "modifier", "opacity"):
            cov = R.covariance_from_scaling_rotation(s, mod, q)
            op = torch.sigmoid(o) if variant == "opacity" else None
        else:
            def rot_L(L):
                out = torch.matmul(Rt, L)
                if terms:
                    out.retain_grad(); cap["in"], cap["out"] = L, out
                return out
            cov = R.rotated_covariance_from_scaling_rotation(s, mod, q, A, io, 1, rot_L=rot_L if Rt is not None else None)
    loss = (cov * w).sum() + ((op * wo).sum() if op is not None else 0.0)
    loss.backward()
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    out = dict(cov=n(cov), opacity=n(op), d_raw=n(raw.grad), d_quat=n(q.grad), d_opac=n(o.grad) if op is not None else None, dM=n(Rt.grad) if Rt is not None else None)
    if terms and cap:
        out["dM_terms"] = (cap["out"].grad[:, :, None, :] * cap["in"][:, None, :, :]).abs().sum(dim=(0, 3)).detach().numpy()   # [a, b] of d Rt
    return out


def cov_numpy64(raw, quat, mod, dcov, fault=None):
    """The plain variant written out in float64 numpy, forward and backward (q / |q| -> R -> L = R diag(mod exp(raw)) -> Sigma = L L^T ->
    six entries; back through each) -- a second, independent float64 form that the CPU tests hold against covariance.py, and the carrier of
    deliberately wrong variants.  fault: 'modifier_not_squared' | 'unsymmetrised_gradient'.  -> (cov [N,6], d_raw [N,3], d_quat [N,4])."""
    raw, q0, g6 = (np.asarray(a, np.float64) for a in (raw, quat, dcov))
    inv = 1.0 / np.sqrt((q0 * q0).sum(1, keepdims=True))
    q = q0 * inv
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    s = np.exp(raw)
    sc = (np.sqrt(mod) if fault == "modifier_not_squared" else mod) * s
    L = R * sc[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)
    h = 0.5
    G = np.zeros_like(S)
    G[:, 0, 0], G[:, 1, 1], G[:, 2, 2] = g6[:, 0], g6[:, 3], g6[:, 5]
    for (a, b), k in (((0, 1), 1), ((0, 2), 2), ((1, 2), 4)):
        if fault == "unsymmetrised_gradient":
            G[:, a, b] = g6[:, k]
        else:
            G[:, a, b] = G[:, b, a] = h * g6[:, k]
    gL = 2.0 * G @ L                                                  # d/dL of <G, L L^T> for a SYMMETRIC G (the fault skips the symmetrisation)
    d_sc = (gL * R).sum(1)
    d_raw = d_sc * sc
    gR = (gL * sc[:, None, :]).reshape(-1, 9).T
    gq = np.stack([2 * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]),
                   2 * (y * gR[1] + z * gR[2] + y * gR[3] - 2 * x * gR[4] - r * gR[5] + z * gR[6] + r * gR[7] - 2 * x * gR[8]),
                   2 * (-2 * y * gR[0] + x * gR[1] + r * gR[2] + x * gR[3] + z * gR[5] - r * gR[6] + z * gR[7] - 2 * y * gR[8]),
                   2 * (-2 * z * gR[0] - r * gR[1] + x * gR[2] + r * gR[3] - 2 * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7])], axis=1)
    d_quat = (gq - q * (q * gq).sum(1, keepdims=True)) * inv
    return cov, d_raw, d_quat


def check_cov_values(sub, ref64, what=""):
    """Every covariance row max_c |a - a64| / max_c |a64| <= COV_VALUE_BAR; the sigmoid |o - o64| <= 4u.  -> figures."""
    e = row_errors(sub["cov"], ref64["cov"], np.arange(ref64["cov"].shape[0]))
    fig = {"cov": float(e.max())}
    assert e.max() <= COV_VALUE_BAR, f"{what}: covariance row {int(e.argmax())} is {e.max():.3e} of its largest entry from float64 (bar {COV_VALUE_BAR:g}; {int((e > COV_VALUE_BAR).sum())} rows over)"
    if ref64.get("opacity") is not None:
        eo = np.abs(sub["opacity"].astype(np.float64) - ref64["opacity"])
        fig["sigmoid"] = float(eo.max())
        assert eo.max() <= SIGMOID_BAR, f"{what}: sigmoid off by {eo.max():.3e} at row {int(eo.argmax())} (bar 4u = {SIGMOID_BAR:.3e})"
    return fig


def check_cov_grad_rows(sub, yard, ref64, what="", names=("d_raw", "d_quat", "d_opac")):
    """Rows of each gradient against their own magnitude, by the rule of check_grad_rows_vs_float64 (tests/common.py row_rule) with the
    float32 torch form as the yardstick.  A fixed bar would be wrong: the float32 form itself reaches 3e-4 on single rows, from the
    cancellation in the projection of the quaternion gradient.  -> figures per array."""
    fig, fails = {}, []
    for name in names:
        a64 = ref64.get(name)
        if a64 is None:
            continue
        a64 = np.asarray(a64, np.float64).reshape(a64.shape[0], -1)
        rows = np.nonzero(np.abs(a64).max(1) > 0)[0]
        e_s, e_y = row_errors(sub[name], a64, rows), row_errors(yard[name], a64, rows)
        q_s, q_o, c_s, c_o, bad = row_rule(e_s, [e_y])
        fig[name] = dict(rows=int(rows.size), q50=(float(q_s[0]), float(q_o[0])), q90=(float(q_s[1]), float(q_o[1])), tails=(tuple(c_s), tuple(c_o)),
                         max=(float(e_s.max()), float(e_y.max())))
        if bad:
            k = int(np.argmax(e_s))
            fails.append(f"{name}: " + "; ".join(bad) + f" (worst row {int(rows[k])}: e {e_s[k]:.2e}, yardstick {e_y[k]:.2e})")
    assert not fails, f"{what}: " + " | ".join(fails)
    return fig


def check_cov_dM(sub, yard, ref64, what=""):
    """Each of the nine: |dM - dM64| <= max(3 x the yardstick's distance, 8u sum|terms|) -- the floor is what a float32 sum of those terms
    may lose whatever its order, with the terms' magnitudes taken from the float64 run.  -> the largest error in units of u sum|terms|."""
    d_s, d_y = np.abs(sub["dM"].astype(np.float64) - ref64["dM"]), np.abs(yard["dM"].astype(np.float64) - ref64["dM"])
    floor = 8.0 * U * ref64["dM_terms"]
    bar = np.maximum(ROW_Q_FACTOR * d_y, floor)
    assert (d_s <= bar).all(), (f"{what}: dM off by {d_s.ravel().tolist()} (float64 {ref64['dM'].ravel().tolist()}); yardstick {d_y.ravel().tolist()}, "
                                f"floor {floor.ravel().tolist()}")
    unit = U * np.maximum(ref64["dM_terms"], 1e-300)
    return dict(dM_in_u_terms=float((d_s / unit).max()), yard_in_u_terms=float((d_y / unit).max()))


# ============================================================= image loss =============================================================
LOSS_SHAPES = [(1, 1, 1), (3, 3, 105), (1, 5, 5), (1, 10, 64), (1, 11, 11), (3, 14, 53), (3, 15, 54), (3, 16, 55), (1, 30, 108), (1, 31, 109), (3, 29, 107)]
LOSS_LAMBDAS = (0.2, 1.0)
LOSS_VALUE_BAR, LOSS_GRAD_BAR, LOSS_FACTOR = 2e-6, 1e-4, 3.0      # the existing test's value bar; the project's bar; x the float32 yardstick
LOSS_STRIP_W, LOSS_STRIP_H, LOSS_HALO = 54, 15, 5                 # loss.hip: a wave's strip, the 11-tap window's reach


def loss_inputs(C, H, W, seed=0):
    gen = torch.Generator().manual_seed(seed * 7919 + (C * 1000 + H) * 1000 + W)
    img = torch.rand(C, H, W, generator=gen)
    gt = (img + 0.1 * torch.randn(C, H, W, generator=gen)).clamp(0, 1)
    gate = (torch.rand(H, W, generator=gen) > 0.3).float()
    return img, gt, gate


def loss_reference(img, gt, lam, gate, dtype):
    """losses.training_loss on the CPU in `dtype` -> (value, gradient [C,H,W] float64 numpy, gated when a gate is given)."""
    from egogaussian_amd.losses import training_loss
    x = img.detach().clone().to(dtype).requires_grad_(True)
    l = training_loss(x, gt.to(dtype), lam)
    l.backward()
    g = x.grad if gate is None else x.grad * gate.to(dtype)[None]
    return float(l.detach()), g.double().numpy()


def loss_zones(H, W):
    """bool[H,W] masks: within 5 pixels of a strip seam (x mod 54, y mod 15; the image border is no seam), within 5 of the border."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    def near(i, period, n):
        d = np.minimum(i % period, period - 1 - i % period)
        return (d < LOSS_HALO) & ~((i < LOSS_HALO) & (i // period == 0)) & ~((n - 1 - i < LOSS_HALO) & (i // period == (n - 1) // period))
    seam = near(x, LOSS_STRIP_W, W) | near(y, LOSS_STRIP_H, H)
    border = (x < LOSS_HALO) | (x >= W - LOSS_HALO) | (y < LOSS_HALO) | (y >= H - LOSS_HALO)
    return seam | np.zeros((H, W), bool), border | np.zeros((H, W), bool)


def _loss_grad_rule(grad, g64, g32, gate=None, factors=None):
    """The gradient rule of check_loss (and of check_pair): per pixel e = |g - g64| / max|g64|; max e <= 1e-4; max e and q99 e <= 3 x the float32
    yardstick's; gated pixels exactly zero.  -> (figures, what failed, e)."""
    g = np.asarray(grad, np.float64)
    scale = float(np.abs(g64).max())
    e, e_y = np.abs(g - g64) / scale, np.abs(g32 - g64) / scale
    seam, border = loss_zones(*g.shape[1:])
    zone = lambda a, m: float(a[:, m].max()) if m.any() else 0.0
    fig = dict(max=(float(e.max()), float(e_y.max())),
               q99=(float(np.quantile(e, 0.99)), float(np.quantile(e_y, 0.99))), seam=(zone(e, seam), zone(e_y, seam)), border=(zone(e, border), zone(e_y, border)),
               interior=(zone(e, ~(seam | border)), zone(e_y, ~(seam | border))))
    fails = []
    if gate is not None and np.any(g[:, np.asarray(gate) == 0] != 0):
        fails.append("a gated pixel has a non-zero gradient")
    if not e.max() <= LOSS_GRAD_BAR:
        c, y, x = np.unravel_index(int(e.argmax()), e.shape)
        fails.append(f"max e {e.max():.3e} > {LOSS_GRAD_BAR:g} at (c, y, x) = ({c}, {y}, {x}); seams {fig['seam'][0]:.2e}, border {fig['border'][0]:.2e}, interior {fig['interior'][0]:.2e}")
    for stat in ("max", "q99"):
        f = (factors or {}).get(stat, LOSS_FACTOR)
        if not fig[stat][0] <= f * fig[stat][1]:
            fails.append(f"{stat} e {fig[stat][0]:.3e} > {f:g} x the float32 form's {fig[stat][1]:.3e}; seams {fig['seam']}, border {fig['border']}, interior {fig['interior']}")
    return fig, fails, e


def check_loss(value, grad, ref64, ref32, gate=None, what="", factors=None):
    """value: |l - l64| <= 2e-6 max(1, |l64|).  Gradient per pixel e = |g - g64| / max|g64|: max e <= 1e-4; max e and q99 e <= 3 x the float32
    yardstick's; gated pixels exactly zero.  factors: {'max' | 'q99': factor} replaces the 3 of one statistic (a recorded finding only).
    -> figures, the maxima on the strip seams and on the border among them."""
    l64, g64 = ref64
    l32, g32 = ref32
    fig, fails, _ = _loss_grad_rule(grad, g64, g32, gate, factors)
    fig = dict(value=abs(value - l64), value_yard=abs(l32 - l64), **fig)
    if not abs(value - l64) <= LOSS_VALUE_BAR * max(1.0, abs(l64)):
        fails.insert(0, f"value {value!r} vs float64 {l64!r}")
    assert not fails, f"{what}: " + "; ".join(fails)
    return fig


def _window11():
    g = np.exp(-(np.arange(11) - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return g / g.sum()


def blur11(x, drop=None):
    """The 11x11 Gaussian window (sigma 1.5, zero padding) as its two 1-D passes, float64 numpy.  drop=(column, tap): the horizontal pass
    loses that tap at that OUTPUT column -- the deliberately wrong variant."""
    w = _window11()
    C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (5, 5), (0, 0)))
    v = sum(w[k] * xp[:, k:k + H, :] for k in range(11))
    vp = np.pad(v, ((0, 0), (0, 0), (5, 5)))
    out = sum(w[k] * vp[:, :, k:k + W] for k in range(11))
    if drop is not None and drop[0] < W:
        out[:, :, drop[0]] -= w[drop[1]] * vp[:, :, drop[0] + drop[1]]
    return out


def loss_numpy64(img, gt, lam, gate=None, drop=None):
    """(1 - lam) L1 + lam (1 - SSIM) and its image gradient in float64 numpy, from the windowed moments and the three partial-derivative
    maps (the blur is self-adjoint: symmetric window, zero padding) -- an independent float64 form for the CPU tests, and the carrier of the
    dropped tap.  -> (value, gradient)."""
    x, y = np.asarray(img, np.float64), np.asarray(gt, np.float64)
    B = lambda a: blur11(a, drop)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = B(x), B(y)
    s1, s2, s12 = B(x * x) - mu1 * mu1, B(y * y) - mu2 * mu2, B(x * y) - mu1 * mu2
    a, b, d, e = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    m = a * b / (d * e)
    n = x.size
    value = (1 - lam) * np.abs(x - y).mean() + lam * (1 - m.mean())
    dm_dmu1 = 2 * mu2 * (b - a) / (d * e) - m * 2 * mu1 * (e - d) / (d * e)      # through mu1 directly and through s1, s12
    dm_ds1, dm_ds12 = -m / e, 2 * a / (d * e)
    dssim = (B(dm_dmu1) + 2 * x * B(dm_ds1) + y * B(dm_ds12)) / n
    grad = (1 - lam) * np.sign(x - y) / n - lam * dssim
    if gate is not None:
        grad = grad * np.asarray(gate, np.float64)[None]
    return float(value), grad


# ============================================================ two-value loss ============================================================
# (mean|x - y|, mean SSIM) as a pair with an upstream scalar each: fused.l1_and_ssim, what the trainers' l1_loss() and ssim() become
PAIR_UPSTREAMS = ((0.8, -0.2), (-0.37, 2.5), (0.0, 1.0), (1.0, 0.0), (2.5, 0.0))      # the first: what (1 - l) l1 + l (1 - ssim) sends down
PAIR_TIE_ROWS, PAIR_TIE_COLS = slice(6, 10), slice(7, 13)
PAIR_L1_ONLY_BAR = 2.0 ** -22      # SSIM switched off: u0 sign(x - y) / n by two float32 roundings (1 / n, the product), see check_pair


def pair_tie_mask(C, H, W):
    """bool[C,H,W]: the block where pair_inputs makes the image EQUAL to the ground truth (none below the 11-tap window: at (1, 1, 1) a tie
    leaves a float64 gradient of ~1e-15 or exactly 0, and an error relative to it means nothing)."""
    m = np.zeros((C, H, W), bool)
    if H >= 11 and W >= 11:
        m[:, PAIR_TIE_ROWS, PAIR_TIE_COLS] = True
    return m


def pair_inputs(C, H, W, seed=0):
    """loss_inputs with a block of exact ties (background pixels the render reproduces): there sign(x - y) = 0 and only SSIM has a gradient."""
    img, gt, gate = loss_inputs(C, H, W, seed)
    tie = torch.from_numpy(pair_tie_mask(C, H, W))
    return torch.where(tie, gt, img), gt, gate


PAIR_FAULTS = ("upstreams_swapped", "ssim_sign_flipped", "ssim_upstream_one", "tie_sign_plus_one")


def pair_reference(img, gt, u, dtype, gate=None, fault=None):
    """losses.l1_loss and losses.ssim on the CPU in `dtype` and the gradient of u[0] l1 + u[1] ssim through autograd -> (l1, ssim, gradient
    [C,H,W] float64 numpy, gated when a gate is given).  The upstream scalars are taken as float32 carries them (f32w): they reach the kernel
    as float32 device scalars, so that is the operation it is asked for.  fault: one of PAIR_FAULTS -- deliberately wrong gradients."""
    from egogaussian_amd.losses import l1_loss, ssim
    u0, u1 = f32w(u[0]), f32w(u[1])
    if fault == "upstreams_swapped":
        u0, u1 = u1, u0
    elif fault == "ssim_sign_flipped":
        u1 = -u1
    elif fault == "ssim_upstream_one":
        u1 = 1.0
    x, y = img.detach().clone().to(dtype).requires_grad_(True), gt.to(dtype)
    l1v, ssv = l1_loss(x, y), ssim(x, y)
    (u0 * l1v + u1 * ssv).backward()
    g = x.grad
    if fault == "tie_sign_plus_one":
        g = g + (u0 / x.numel()) * (x.detach() == y).to(dtype)
    if gate is not None:
        g = g * gate.to(dtype)[None]
    g = g.double().numpy()
    assert np.abs(g).max() > 0
    return float(l1v.detach()), float(ssv.detach()), g


def check_pair(values, grad, ref64, ref32, u, gate=None, what=""):
    """values = (l1, ssim), each |v - v64| <= 2e-6 max(1, |v64|); gated pixels exactly zero; every element finite.  The gradient,
    u[1] != 0: check_loss's rule (_loss_grad_rule), and the tie block (pair_tie_mask: no L1 term there) once more on its own, max e <= 1e-4.
    u[1] == 0 (SSIM switched off): the float32 yardstick is 2e-9 .. 5e-8 there and a multiple of it would be a bar on luck; the definition
    gives one instead.  The float64 gradient is u0 sign(x - y) / n, zero exactly on ties (and under the gate): there the subject must be
    zero (either sign); elsewhere |g - g64| <= 2^-22 |g64| -- float32 reaches it by two roundings, of 1 / n and of the product with u0
    (2^-23 together; the sign and the switched-off SSIM term add none).  -> figures as check_loss's, 'tie' and 'l1_only' among them."""
    l1_64, ss_64, g64 = ref64
    l1_32, ss_32, g32 = ref32
    g = np.asarray(grad, np.float64)
    fig = dict(values=(abs(values[0] - l1_64), abs(values[1] - ss_64)), values_yard=(abs(l1_32 - l1_64), abs(ss_32 - ss_64)))
    fails = [f"{name} {v!r} vs float64 {v64!r}" for name, v, v64 in (("l1", values[0], l1_64), ("ssim", values[1], ss_64))
             if not abs(v - v64) <= LOSS_VALUE_BAR * max(1.0, abs(v64))]
    if not np.isfinite(g).all():
        fails.append(f"{int((~np.isfinite(g)).sum())} elements are not finite")
    tie = pair_tie_mask(*g.shape)
    if u[1] != 0:
        gfig, gfails, e = _loss_grad_rule(g, g64, g32, gate)
        scale = float(np.abs(g64).max())
        fig.update(gfig, tie=((float(e[tie].max()), float((np.abs(g32 - g64) / scale)[tie].max())) if tie.any() else (0.0, 0.0)))
        fails += gfails
        if not fig["tie"][0] <= LOSS_GRAD_BAR:
            fails.append(f"tie block (no L1 term): max e {fig['tie'][0]:.3e} > {LOSS_GRAD_BAR:g}")
    else:
        if gate is not None and np.any(g[:, np.asarray(gate) == 0] != 0):
            fails.append("a gated pixel has a non-zero gradient")
        zero = g64 == 0
        assert zero[tie].all(), "the float64 gradient of the L1 term alone is not zero on a tie"
        if np.any(g[zero] != 0):
            fails.append(f"{int((g[zero] != 0).sum())} elements are not zero where x == y (or under the gate)")
        rel = np.abs(g - g64)[~zero] / np.abs(g64)[~zero]
        fig["l1_only"] = (float(rel.max()), float((np.abs(g32 - g64)[~zero] / np.abs(g64)[~zero]).max()))
        if not rel.max() <= PAIR_L1_ONLY_BAR:
            fails.append(f"u0 sign(x - y) / n: {int((rel > PAIR_L1_ONLY_BAR).sum())} elements over 2^-22 of their float64 value (worst {rel.max() / U:.2f} u)")
    assert not fails, f"{what}: " + "; ".join(fails)
    return fig
