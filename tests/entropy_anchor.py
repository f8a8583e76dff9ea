"""Float64 anchor of the opacity-entropy regulariser (include/egs_raster.h egs_opacity_entropy; csrc/opacity_entropy.h), and the bars
every route is held to -- the torch expression on CPU (the yardstick), the stand-alone kernels, the rasterizer's backward.

Definition, per row with radii > 0, on the FLOAT32 activated opacity o the forward used:
    a = o + 1e-10f    b = (1.0f - o) + 1e-10f    1 - o               formed in float32: they are part of the function's definition at
                                                                     saturation (o = 1 - 2^-24 has 1 - o = 2^-24 exactly; b = 1 when o = 0)
    h = -o ln a - (1 - o) ln b        dh/do = -ln a - o / a + ln b + (1 - o) / b          everything after them in float64
    value = sum h / n_vis             dL/do = c dh/do,  c = weight * upstream / n_vis     (times o (1 - o) for a logit input)

Gradient bar, per element:  |g - g64| <= 12 * 2^-24 * c * (|ln a| + |ln b| + o / a + (1 - o) / b) * o (1 - o)
    two logf at <= 1 ulp, two divisions, three additions each bounded by the sum of the term magnitudes, the coefficient, the two-rounding
    sigmoid factor: 9 roundings, with headroom.  (An activated input has no sigmoid factor: the same bar without o (1 - o).)
    Underflow.  That derivation counts RELATIVE roundings, which holds while the results are normal float32 numbers.  A logit below -87 has
    an activated opacity under 2^-126, and its gradient c dh/do o (1 - o) is a subnormal: float32 then resolves 2^-149 absolute, whatever
    computes it (exact gradient 1.4e-40 at logit -88 with 255 visible rows: its float32 neighbours are 1e-5 of it apart, 84 x 2^-24).  The two
    products that can underflow (o (1 - o) and the final one) each round by at most half that quantum, so the bar carries ONE float32
    subnormal quantum, 2^-149, as an absolute term.  It is 1.4e-45: no row whose bar is a normal number notices it.  (In the yardstick's
    inputs -- n = 20 011, seed 0 -- the rows at -88, -110 happen to be invisible; tests/test_entropy_cpu.py shows torch's own float32
    autograd missing the purely relative bar on exactly that row when every row is visible, and clearing half of this one.)
Value bar:  1e-5 * max(1, |v64|) -- float32 partial sums finished in float64 (the bar tests/test_gpu_object_loss.py holds for such sums).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149          # the float32 subnormal quantum (see "Underflow" above)
GRAD_ULPS = 12.0
VALUE_RTOL = 1e-5
FIXED_LOGITS = (0.0, -0.0, 20, -20, 110, -110, 17, -17, 88, -88, 1e-4, -1e-4, 5, -5, 30, -30)


def inputs(n, seed=0, visible=0.6):
    """-> (logits float32[n], visible bool[n]): uniform in [-12, 12] plus the fixed set (exact zero, both signs, saturation in float32 on
    both sides, far beyond it, the range where exp overflows), `visible` of the rows visible.  n < 16: the first n of the fixed set."""
    rng = np.random.default_rng(seed)
    k = min(n, len(FIXED_LOGITS))
    x = np.concatenate([rng.uniform(-12, 12, n - k), np.asarray(FIXED_LOGITS[:k], dtype=np.float64)]).astype(np.float32)
    if visible >= 1.0:
        vis = np.ones(n, dtype=bool)
    elif visible <= 0.0:
        vis = np.zeros(n, dtype=bool)
    else:
        vis = rng.random(n) < visible
    return x, vis


def _parts(o32):
    o32 = np.asarray(o32, dtype=np.float32)
    one, eps = np.float32(1.0), np.float32(1e-10)
    om32 = (one - o32).astype(np.float32)
    a = (o32 + eps).astype(np.float32).astype(np.float64)
    b = (om32 + eps).astype(np.float32).astype(np.float64)
    return o32.astype(np.float64), om32.astype(np.float64), a, b


def anchor(o32, vis, weight=1.0, upstream=1.0, logit=True):
    """-> dict(value, grad [P] float64, unit [P]: the bar's per-element magnitude (multiply by GRAD_ULPS * U), n_vis)."""
    vis = np.asarray(vis, dtype=bool)
    o, om, a, b = _parts(o32)
    with np.errstate(all="ignore"):
        h = -o * np.log(a) - om * np.log(b)
        dh = -np.log(a) - o / a + np.log(b) + om / b
        mag = np.abs(np.log(a)) + np.abs(np.log(b)) + o / a + om / b
    n = int(vis.sum())
    c = float(weight) * float(upstream) / n if n else 0.0
    chain = o * (1.0 - o) if logit else np.ones_like(o)
    grad = np.where(vis, c * dh * chain, 0.0)
    unit = np.where(vis, abs(c) * mag * chain, 0.0)
    value = float(h[vis].sum() / n) if n else float("nan")
    return dict(value=value, grad=grad, unit=unit, n_vis=n)


def grad_excess(g, ref, tiny=TINY):
    """Worst (|g - g64| - 2^-149) / (2^-24 unit) over the rows with a non-zero bar; rows whose bar is 0 (invisible, or a saturated logit)
    must be EXACTLY 0 and finite -- else inf.  tiny=0: the purely relative measure."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    if not np.isfinite(g).all():
        return float("inf")
    err, unit = np.abs(g - ref["grad"]), ref["unit"]
    zero = unit == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float((np.clip(err[~zero] - tiny, 0.0, None) / (U * unit[~zero])).max()) if (~zero).any() else 0.0


def grad_ok(g, ref, factor=1.0):
    return grad_excess(g, ref) <= GRAD_ULPS * factor


def value_ok(v, ref, factor=1.0):
    v64 = ref["value"]
    if np.isnan(v64):
        return bool(np.isnan(v))
    return bool(np.isfinite(v)) and abs(float(v) - v64) <= factor * VALUE_RTOL * max(1.0, abs(v64))
