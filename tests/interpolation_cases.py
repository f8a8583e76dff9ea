"""What the two pose-interpolation test files share: the recorded cases of tests/golden/interpolation.npz, their float64 and float32
mirrors (egogaussian_amd.poses.decompose_transform, computed once per case and never modified) and the bar.

The bar, per entry of the twelve floats [R | t] of an end point (and of a residual), against the FLOAT64 mirror:
    max(3 x the float32 mirror's largest distance from the float64 mirror on that case, 2 float32 ulps of max(1, |entry|))
3 is the factor tests/anchors.py uses for its float32 yardsticks; the floor is what rounding the stored floats costs."""
import functools
import os

import numpy as np
import torch

FACTOR = 3.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interpolation.npz")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case_names():
    return [str(s) for s in golden()["dec_names"]]


def case_inputs(name):
    """(T float32 [4,4], n) of a recorded decompose_transform case."""
    g = golden()
    i = case_names().index(name)
    return torch.tensor(g["dec_T"][i]), int(g["dec_n"][i])


def row12(t, R):
    """[R | t] row-major, float64 [12]."""
    return torch.cat([torch.as_tensor(R).double().reshape(3, 3), torch.as_tensor(t).double().reshape(3, 1)], dim=1).reshape(12)


@functools.lru_cache(maxsize=None)
def _mirrors(T_bytes, n):
    from egogaussian_amd import poses
    T = torch.tensor(np.frombuffer(T_bytes, dtype=np.float32).reshape(4, 4).copy())
    out = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        t, R, res = poses.decompose_transform(T, n, dtype=dtype)
        out["row" + tag], out["res" + tag] = row12(t, R), float(res)
    out["d32"] = float((out["row32"] - out["row64"]).abs().max())
    out["dres32"] = abs(out["res32"] - out["res64"])
    return out


def mirrors(T, n):
    """dict(row64, row32 [12] float64 tensors, res64, res32, d32 = max |row32 - row64|, dres32 = |res32 - res64|) of one transform."""
    T = torch.as_tensor(T, dtype=torch.float32)
    if T.numel() == 12:
        T = torch.cat([T.reshape(3, 4), torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
    return _mirrors(T.reshape(4, 4).numpy().tobytes(), int(n))


def _floor(ref):
    return 2.0 * torch.tensor(np.spacing(np.maximum(1.0, np.abs(np.asarray(ref, dtype=np.float64))).astype(np.float32)).astype(np.float64))


def row_bar(ref_row64, d32):
    return torch.maximum(torch.full((12,), FACTOR * d32, dtype=torch.float64), _floor(ref_row64.numpy()))


def row_excess(row, m):
    """max over the twelve entries of |row - row64| / bar: <= 1 passes."""
    return float(((torch.as_tensor(row).double().reshape(12) - m["row64"]).abs() / row_bar(m["row64"], m["d32"])).max())


def residual_excess(res, m):
    return abs(float(res) - m["res64"]) / max(FACTOR * m["dres32"], float(_floor([m["res64"]])[0]))
