"""Float64 anchor of the spherical-harmonics kernels (csrc/sh.hip: k_sh_forward, k_sh_backward, k_sh16_forward<CAT|SPLIT>,
k_sh16_backward<CAT|SPLIT>): the case builder and the table of cases, the Python mirror of the dispatch rule, the float64 reference written
from the definition (the real SH polynomials as monomial tables), the float32 CPU yardstick with its deliberately wrong variants, and the
checks themselves.  tests/test_gpu_sh.py hands the kernels' outputs to these checks, tests/test_sh_anchor_cpu.py the yardstick and the
variants.  Importable without a GPU.

Bars.  No constant is fixed in advance: a bar is MARGIN x the largest error / unit ratio of the float32 yardstick (the same formulas in
numpy float32, one rounding per operation).  The yardstick's ratio is taken over EVERY case of the table with the same active degree: a
case of one or three rows alone is a sample of a few roundings, which can all be exact, and a bar of 4 x 0 says nothing about a kernel.
The GPU test measures it in its own run, with the kernels' dL/dcolour, clamp bits and projection terms as the yardstick's inputs; the CPU
tests, which have no such inputs, with a synthetic upstream (`table_yardstick`).
Units: colour 0.5 + sum |c_k| A_k(d), dL/dSH |g_ch| A_k(d), A_k = the basis polynomial with every monomial taken absolute; the direction
term is measured as the kernel forms it, a = b + t against u (|a| + |b| + |t64|)."""
import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24                     # float32 unit roundoff
MARGIN = 4.0                       # x the float32 yardstick's distance from float64 (as tests/test_gpu_pose_sequence.py)
H = W = 32                         # 2 x 2 tiles
CLAMP_MASK = 7                     # include/egs_raster.h: bits 0-2 of the geometry buffer's `clamped` byte
BAND_CAP = 0.01                    # channels whose |v64| is inside the colour bar (their clamp bit may go either way) / visible channels

PS = (1, 3, 4, 63, 64, 65, 67, 128, 130, 191)
M_ACTIVE = ((1, 0), (4, 0), (4, 1), (9, 0), (9, 1), (9, 2), (16, 0), (16, 1), (16, 2), (16, 3))
LAYOUTS = ("cat", "split", "split-unaligned")
PATTERNS = ("all", "none", "block-1-empty", "only-last-row", "only-row-0-of-each-block", "all-but-one", "alternating", "random-half")

# ---- the real spherical harmonics of degrees 0-3 as monomials (coefficient, power of x, of y, of z); constants from their closed forms ----
_PI = math.pi
_C0 = 0.5 * math.sqrt(1.0 / _PI)
_C1 = math.sqrt(3.0 / (4.0 * _PI))
_C2A, _C2B, _C2C = 0.5 * math.sqrt(15.0 / _PI), 0.25 * math.sqrt(5.0 / _PI), 0.25 * math.sqrt(15.0 / _PI)
_C3A, _C3B, _C3C = 0.25 * math.sqrt(35.0 / (2.0 * _PI)), 0.5 * math.sqrt(105.0 / _PI), 0.25 * math.sqrt(21.0 / (2.0 * _PI))
_C3D, _C3E = 0.25 * math.sqrt(7.0 / _PI), 0.25 * math.sqrt(105.0 / _PI)
C0 = _C0
BASIS = (
    ((_C0, 0, 0, 0),),
    ((-_C1, 0, 1, 0),), ((_C1, 0, 0, 1),), ((-_C1, 1, 0, 0),),
    ((_C2A, 1, 1, 0),), ((-_C2A, 0, 1, 1),), ((2 * _C2B, 0, 0, 2), (-_C2B, 2, 0, 0), (-_C2B, 0, 2, 0)), ((-_C2A, 1, 0, 1),),
    ((_C2C, 2, 0, 0), (-_C2C, 0, 2, 0)),
    ((-3 * _C3A, 2, 1, 0), (_C3A, 0, 3, 0)),                                           # -C y (3 xx - yy)
    ((_C3B, 1, 1, 1),),
    ((-4 * _C3C, 0, 1, 2), (_C3C, 2, 1, 0), (_C3C, 0, 3, 0)),                          # -C y (4 zz - xx - yy)
    ((2 * _C3D, 0, 0, 3), (-3 * _C3D, 2, 0, 1), (-3 * _C3D, 0, 2, 1)),                 #  C z (2 zz - 3 xx - 3 yy)
    ((-4 * _C3C, 1, 0, 2), (_C3C, 3, 0, 0), (_C3C, 1, 2, 0)),                          # -C x (4 zz - xx - yy)
    ((_C3E, 2, 0, 1), (-_C3E, 0, 2, 1)),                                               #  C z (xx - yy)
    ((-_C3A, 3, 0, 0), (3 * _C3A, 1, 2, 0)),                                           # -C x (xx - 3 yy)
)

VARIANTS = ("c2-sign", "c3-derivative-sign", "layout-transposed", "row-shifted", "clamp-ignored", "no-tangent-projection", "no-degree3-dz")


def _derivatives(basis):
    """d/dx, d/dy, d/dz of every basis polynomial, as monomial lists again."""
    out = []
    for axis in range(3):
        per_k = []
        for poly in basis:
            mono = []
            for c, *pw in poly:
                if pw[axis]:
                    q = list(pw); q[axis] -= 1
                    mono.append((c * pw[axis], *q))
            per_k.append(tuple(mono))
        out.append(tuple(per_k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tables(variant=None):
    """(basis, derivatives) -- the definition, or one of the wrong variants that live in the polynomials."""
    basis = [list(p) for p in BASIS]
    if variant == "c2-sign":
        basis[7] = [(-c, a, b, e) for c, a, b, e in basis[7]]
    deriv = [list(map(list, ax)) for ax in _derivatives(tuple(tuple(p) for p in basis))]
    if variant == "c3-derivative-sign":                                # d/dx of C z (xx - yy): 2 C xz with the wrong sign
        c, a, b, e = deriv[0][14][0]
        deriv[0][14][0] = (-c, a, b, e)
    if variant == "no-degree3-dz":
        for k in range(9, 16):
            deriv[2][k] = []
    return tuple(tuple(p) for p in basis), tuple(tuple(tuple(m) for m in ax) for ax in deriv)


def _poly(mono, x, y, z, dtype, absolute=False):
    """sum of c x^a y^b z^c over the monomials, every operation rounded to `dtype`; absolute: |c| |x|^a |y|^b |z|^c."""
    acc = np.zeros(x.shape, dtype)
    first = True
    for c, a, b, e in mono:
        term = np.full(x.shape, abs(c) if absolute else c, dtype)
        for v, n in ((x, a), (y, b), (z, e)):
            for _ in range(n):
                term = term * (np.abs(v) if absolute else v)
        acc = term if first else acc + term
        first = False
    return acc


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def camera():
    """One camera for every case: frame 20 of the synthetic orbit (yaw 4 deg, a camera centre off the origin) at 32 x 32."""
    from egogaussian_amd.scene_synth import make_camera
    cam = make_camera(20, H, W)
    return SimpleNamespace(viewmatrix=cam.world_view_transform.clone(), projmatrix=cam.full_proj_transform.clone(), campos=cam.camera_center.clone(),
                           tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2))


def visibility(P, pattern, rng):
    i = np.arange(P)
    if pattern == "all":
        return np.ones(P, bool)
    if pattern == "none":
        return np.zeros(P, bool)
    if pattern == "block-1-empty":
        return (i < 64) | (i >= 128)
    if pattern == "only-last-row":
        return i == P - 1
    if pattern == "only-row-0-of-each-block":
        return i % 64 == 0
    if pattern == "all-but-one":
        return i != P // 2
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "random-half":
        return rng.random(P) < 0.5
    raise ValueError(pattern)


AXIS_DIRECTIONS = ((0.0, 0.0, 1.0), (0.3, 0.0, 1.0), (0.0, 0.2, 1.0), (-0.25, 0.0, 1.0), (0.0, -0.3, 1.0))      # on the z axis; in the y = 0 and x = 0 planes


def case_seed(P, M, active, pattern):
    return zlib.crc32(f"{P},{M},{active},{pattern}".encode())


def sh_case(P, M, layout, active, pattern, seed):
    """Rasterizer inputs (float32 CPU tensors, cov3D_precomp given) of one case; `layout` is only recorded: the data depend on the other
    arguments alone, so the layouts of one case can be compared bit for bit.  Rows i % 21 == 2 look along a coordinate axis / plane
    (exact zeros in p - campos); about 30 % of the rows sit 0.3-0.6 in front of the camera; culled rows lie behind the near plane."""
    assert M in (1, 4, 9, 16) and (active + 1) ** 2 <= M and layout in LAYOUTS and pattern in PATTERNS
    rng = np.random.default_rng(seed)
    cam = camera()
    vis = visibility(P, pattern, rng)
    V = cam.viewmatrix.double().numpy()
    R, t = V[:3, :3], V[3, :3]                                         # row vectors: view = p R + t
    z = np.where(rng.random(P) < 0.3, rng.uniform(0.3, 0.6, P), rng.uniform(1.5, 6.0, P))
    z = np.where(vis, z, rng.uniform(-3.0, 0.15, P))
    depth = np.maximum(np.abs(z), 0.3)
    view = np.stack([rng.uniform(-0.8, 0.8, P) * cam.tanfovx * depth, rng.uniform(-0.8, 0.8, P) * cam.tanfovy * depth, z], 1)
    p = ((view - t) @ R.T).astype(np.float32)
    campos = cam.campos.numpy().astype(np.float32)
    dist = rng.uniform(1.5, 4.0, P)
    for i in range(2, P, 21):
        if vis[i]:
            d = np.asarray(AXIS_DIRECTIONS[(i // 21) % len(AXIS_DIRECTIONS)])
            p[i] = campos + (d * dist[i]).astype(np.float32)
            depth[i] = dist[i]
    # covariance: a random rotation of diag(s^2), s = 3-8 % of the depth (a radius of 3-8 pixels: every row in front touches a tile)
    q = rng.normal(size=(P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, zq = q.T
    Rot = np.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - r * zq), 2 * (x * zq + r * y),
                    2 * (x * y + r * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - r * x),
                    2 * (x * zq - r * y), 2 * (y * zq + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    s = depth[:, None] * rng.uniform(0.03, 0.08, (P, 3))
    S = np.einsum("pij,pj,pkj->pik", Rot, s * s, Rot)
    cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
    opac = rng.uniform(0.1, 0.5, (P, 1)).astype(np.float32)
    shs = rng.normal(0.0, 1.0, (P, M, 3))
    shs[:, 0] = rng.uniform(-2.0, 2.0, (P, 3)) / C0
    shs = shs.astype(np.float32)
    shs[:, (active + 1) ** 2:] = np.nan                                # never read: coefficients above the active degree ...
    shs[~vis] = np.nan                                                 # ... and every coefficient of a culled row
    # the case is what it claims: visible rows project inside the image with room, culled rows are behind the near plane
    pv = p.astype(np.float64) @ R + t
    assert np.all(pv[~vis, 2] <= 0.19) and np.all(pv[vis, 2] >= 0.29)
    px = (pv[vis, 0] / pv[vis, 2] / cam.tanfovx + 1) * W / 2
    py = (pv[vis, 1] / pv[vis, 2] / cam.tanfovy + 1) * H / 2
    assert np.all((px > 2) & (px < W - 2) & (py > 2) & (py < H - 2))
    tt = torch.from_numpy
    return SimpleNamespace(P=P, M=M, layout=layout, active=active, pattern=pattern, seed=seed, visible=vis, id=f"P{P}-M{M}-{layout}-D{active}-{pattern}",
                           means3D=tt(p), cov3D_precomp=tt(cov), opacities=tt(opac), shs=tt(shs), bg=torch.tensor([0.1, 0.2, 0.3]), cam=cam)


def oracle_inputs(case):
    """keyword arguments of oracle.oracle.Oracle.forward for the case (the poison taken out: the oracle copies whole arrays)."""
    cam = case.cam
    return dict(means3D=case.means3D, opacities=case.opacities, shs=torch.nan_to_num(case.shs), cov3D_precomp=case.cov3D_precomp,
                viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, campos=cam.campos, bg=case.bg, image_height=H, image_width=W,
                tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, sh_degree=case.active)


# (P, pattern) pairs the table walks through: every P, every pattern, the combinations that mean something (a whole block culled needs P >= 128)
_PAIRS = ((1, "all"), (130, "block-1-empty"), (3, "all"), (64, "all"), (191, "random-half"), (65, "only-last-row"), (4, "all-but-one"),
          (63, "alternating"), (128, "block-1-empty"), (67, "random-half"), (130, "all"), (1, "none"), (191, "block-1-empty"),
          (64, "only-row-0-of-each-block"), (65, "all"), (3, "only-last-row"), (130, "only-row-0-of-each-block"), (63, "random-half"),
          (191, "all"), (128, "alternating"), (67, "all-but-one"), (4, "all"), (191, "only-last-row"), (65, "none"))
_PER_COMBO = 5


@functools.lru_cache(maxsize=None)
def table():
    """[(P, M, layout, active, pattern)]: every (M, active) x layout with five (P, pattern) pairs, the pairs taken in rotation.  M = 1 has
    one layout: an empty rest block is an absent one to the wrapper, and one coefficient is evaluated inside the preprocess kernels."""
    out, c = [], 0
    for M, active in M_ACTIVE:
        for layout in (LAYOUTS if M > 1 else ("cat",)):
            for j in range(_PER_COMBO):
                P, pattern = _PAIRS[(c * _PER_COMBO + j) % len(_PAIRS)]
                out.append((P, M, layout, active, pattern))
            c += 1
    return tuple(out)


def case_id(key):
    P, M, layout, active, pattern = key
    return f"P{P}-M{M}-{layout}-D{active}-{pattern}"


@functools.lru_cache(maxsize=None)
def get_case(key):
    P, M, layout, active, pattern = key
    return sh_case(P, M, layout, active, pattern, case_seed(P, M, active, pattern))


# ------------------------------------------------------- the dispatch rule, mirrored ---------------------------------------------------
def expected_path(case):
    """-> (kernel family, {(direction, loader)}) the launches of this case take (csrc/sh.hip egs_launch_sh_forward / _backward).
    family: 'inline' (M = 1: no launch of its own), 'sh16-cat' / 'sh16-split' (M = 16 and every base 16-byte aligned), else 'generic'.
    loader, per 64-row block and array: 'vector' iff the block's base is 16-byte aligned, (nvalid rw) % 4 == 0 and rw <= 48 (a store has no
    limit on rw); else 'tail' -- the generic kernels' scalar loop, the ragged tails of SPLIT (`lane < 3`), the `row < nvalid` guard of CAT
    (whose float4 never straddle a row: a ragged block only ends early).  The forward of a block with no visible row returns before it loads;
    the backward loads only with a visible row and active > 0, and always stores."""
    P, M, D = case.P, case.M, case.active
    if M == 1:
        return "inline", set()
    aligned = case.layout != "split-unaligned"
    family = ("sh16-cat" if case.layout == "cat" else "sh16-split") if (M == 16 and aligned) else "generic"
    cells = set()
    for i0 in range(0, P, 64):
        nvalid = min(64, P - i0)
        any_vis = bool(case.visible[i0:i0 + nvalid].any())
        if family == "sh16-cat":
            load_f = load_b = store = ["vector" if nvalid == 64 else "tail"]
        elif family == "sh16-split":
            load_f = load_b = store = ["vector" if nvalid % 4 == 0 else "tail"]
        else:
            vec = lambda rw, al, load: "vector" if al and (nvalid * rw) % 4 == 0 and (rw <= 48 or not load) else "tail"
            if case.layout == "cat":
                load_f = load_b = [vec(3 * M, True, True)]
                store = [vec(3 * M, True, False)]
            else:                                                      # DC block, rest block (read only above degree 0; the backward reads it alone)
                load_b = [vec(3 * M - 3, aligned, True)] if D > 0 else []
                load_f = [vec(3, True, True)] + load_b
                store = [vec(3, True, False), vec(3 * M - 3, True, False)]
        if any_vis:
            cells |= {("forward", k) for k in load_f}
            if D > 0:
                cells |= {("backward", k) for k in load_b}
        cells |= {("backward", k) for k in store}
    return family, cells


def split_tail_residues(case):
    """nvalid % 4 of every block of a case the SPLIT kernels take (their float4 / `lane < 3` boundary)."""
    return {min(64, case.P - i0) % 4 for i0 in range(0, case.P, 64)} if expected_path(case)[0] == "sh16-split" else set()


# ------------------------------------------------------------- the formulas ------------------------------------------------------------
def evaluate(case, dtype, variant=None):
    """Forward of the visible rows in `dtype` (float64: the reference; float32: the yardstick, one rounding per operation).
    -> v [P,3] before the clamp, color, neg (v < 0), unit [P,3], and what the backward needs.  Culled rows hold zeros."""
    rows = np.flatnonzero(case.visible)
    nb = (case.active + 1) ** 2
    basis, deriv = tables(variant)
    sh = case.shs.numpy()
    if variant == "layout-transposed":                                 # [P,M,3] memory read as [P,3,M]
        sh = np.ascontiguousarray(sh.reshape(case.P, 3, case.M).transpose(0, 2, 1))
    if variant == "row-shifted":                                       # row i reads row i + 1
        sh = np.roll(sh, -1, axis=0)
    with np.errstate(invalid="ignore"):
        c = sh[rows][:, :nb].astype(dtype)                            # [n, nb, 3]
        d = case.means3D.numpy()[rows].astype(dtype) - case.cam.campos.numpy().astype(dtype)
        inv = dtype(1.0) / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        x, y, z = d[:, 0] * inv, d[:, 1] * inv, d[:, 2] * inv
        B = np.stack([_poly(basis[k], x, y, z, dtype) for k in range(nb)], 1)                  # [n, nb]
        A = np.stack([_poly(BASIS[k], x, y, z, np.float64, absolute=True) for k in range(nb)], 1)
        v = c[:, 0] * B[:, 0, None]
        for k in range(1, nb):
            v = v + c[:, k] * B[:, k, None]
        v = v + dtype(0.5)
        unit = 0.5 + (np.abs(c.astype(np.float64)) * A[:, :, None]).sum(1)
    full = lambda a, fill=0: _scatter(a, rows, case.P, fill)
    return SimpleNamespace(rows=rows, c=c, x=x, y=y, z=z, inv=inv, B=B, A=A, deriv=deriv, dtype=dtype, variant=variant,
                           v=full(v), color=full(np.maximum(v, dtype(0.0))), neg=full(v < 0, False), unit=full(unit))


def _scatter(a, rows, P, fill=0):
    out = np.full((P,) + a.shape[1:], fill, a.dtype)
    out[rows] = a
    return out


def backward(case, fw, g, neg):
    """dL/dSH [P,M,3] and the direction term t [P,3] of `fw` (an `evaluate` result) for dL/dcolour g [P,3] (float32) with the channels of
    `neg` [P,3] clamped; unit_dsh [P,M,3].  Culled rows and coefficients above the active degree hold zeros."""
    dtype, rows, nb = fw.dtype, fw.rows, fw.B.shape[1]
    variant = fw.variant
    with np.errstate(invalid="ignore"):
        gz = np.asarray(g, np.float32)[rows].astype(dtype)
        if variant != "clamp-ignored":
            gz = np.where(np.asarray(neg)[rows], dtype(0.0), gz)
        dsh = np.zeros((len(rows), case.M, 3), dtype)
        dsh[:, :nb] = fw.B[:, :, None] * gz[:, None, :]
        unit = np.zeros((len(rows), case.M, 3))
        unit[:, :nb] = fw.A[:, :, None] * np.abs(gz.astype(np.float64))[:, None, :]
        gdir = []
        for axis in range(3):
            acc = np.zeros(len(rows), dtype)
            for ch in range(3):
                dv = np.zeros(len(rows), dtype)
                for k in range(1, nb):
                    dv = dv + _poly(fw.deriv[axis][k], fw.x, fw.y, fw.z, dtype) * fw.c[:, k, ch]
                acc = acc + dv * gz[:, ch]
            gdir.append(acc)
        dot = fw.x * gdir[0] + fw.y * gdir[1] + fw.z * gdir[2]
        if variant == "no-tangent-projection":
            t = np.stack([gdir[0] * fw.inv, gdir[1] * fw.inv, gdir[2] * fw.inv], 1)
        else:
            t = np.stack([(gdir[0] - fw.x * dot) * fw.inv, (gdir[1] - fw.y * dot) * fw.inv, (gdir[2] - fw.z * dot) * fw.inv], 1)
    return SimpleNamespace(dsh=_scatter(dsh, rows, case.P), unit=_scatter(unit, rows, case.P), t=_scatter(t, rows, case.P))


def synthetic_upstream(case):
    """What the CPU tests use for the two inputs only a GPU run has: dL/dcolour g ~ N(0, 1) and the projection term b of dL/dmeans3D, N(0, 1)
    scaled over four decades (the direction term is then anywhere from dominant to two decades below it).  float32 [P,3] each."""
    rng = np.random.default_rng(case.seed ^ 0x5EED)
    g = rng.normal(size=(case.P, 3)).astype(np.float32)
    b = (rng.normal(size=(case.P, 3)) * 10.0 ** rng.uniform(-2, 2, (case.P, 1))).astype(np.float32)
    return g, b


# --------------------------------------------------------------- the checks ------------------------------------------------------------
def _ratio(err, unit):
    """largest err / (U unit); a zero unit (a basis polynomial that vanishes on an axis) admits no error at all -> inf."""
    err, unit = np.abs(np.asarray(err, np.float64)), np.asarray(unit, np.float64)
    if err.size == 0:
        return 0.0
    bad = ~np.isfinite(err) | ((unit == 0) & (err != 0))
    if bad.any():
        return math.inf
    r = np.divide(err, U * unit, out=np.zeros_like(err), where=unit > 0)
    return float(r.max())


def color_ratio(case, color, ref):
    vis = case.visible
    return _ratio(np.asarray(color, np.float64)[vis] - ref.color[vis], ref.unit[vis])


def clamp_mismatches(case, neg, ref, bar):
    """-> (visible channels outside the band whose bit differs from v64 < 0, channels inside the band)."""
    vis = case.visible
    band = np.abs(ref.v[vis]) <= bar * U * ref.unit[vis]
    wrong = (np.asarray(neg, bool)[vis] != ref.neg[vis]) & ~band
    return int(wrong.sum()), int(band.sum())


def dsh_ratio(case, dsh, bw):
    vis = case.visible
    return _ratio(np.asarray(dsh, np.float64)[vis] - bw.dsh[vis], bw.unit[vis])


def dsh_exact_zeros(case, dsh, neg):
    """The words that are exactly 0.0: clamped channels, coefficients above the active degree, every word of a culled row.
    -> list of complaints."""
    dsh = np.asarray(dsh)
    nb = (case.active + 1) ** 2
    zero = lambda a: bool(np.all(a == 0.0))                            # (NaN != 0: a poisoned word fails)
    out = []
    if not zero(dsh[~case.visible]):
        out.append("a word of a culled row is not 0.0")
    if not zero(dsh[:, nb:]):
        out.append("a coefficient above the active degree is not 0.0")
    cl = np.asarray(neg, bool) & case.visible[:, None]
    if not zero(np.broadcast_to(cl[:, None, :], dsh.shape) * np.nan_to_num(dsh, nan=1.0)):
        out.append("a clamped channel is not 0.0")
    return out


def position_ratio(case, a, b, t64):
    """a = dL/dmeans3D with the direction term, b = without (the colours-mode twin): (a - b) - t64 in units of u (|a| + |b| + |t64|) --
    the rounding of the +=, the term's own roundings and the twin's."""
    vis = case.visible
    a, b, t64 = (np.asarray(v, np.float64)[vis] for v in (a, b, t64))
    return _ratio((a - b) - t64, np.abs(a) + np.abs(b) + np.abs(t64))


def yardstick_ratios(case, g=None, b=None, neg=None):
    """The float32 formulation against float64 on this case -> dict(color, dsh, pos: largest ratios; zeros: complaints).
    g, b: dL/dcolour and the projection term (default: synthetic_upstream); neg: the clamp bits the backward honours (default: its own)."""
    if g is None:
        g, b = synthetic_upstream(case)
    ref, y = evaluate(case, np.float64), evaluate(case, np.float32)
    used = y.neg if neg is None else np.asarray(neg, bool)
    bw64, bw32 = backward(case, ref, g, used), backward(case, y, g, used)
    a32 = np.asarray(b, np.float32) + bw32.t.astype(np.float32)
    return dict(color=color_ratio(case, y.color, ref), dsh=dsh_ratio(case, bw32.dsh, bw64), pos=position_ratio(case, a32, b, bw64.t),
                zeros=dsh_exact_zeros(case, bw32.dsh, used))


@functools.lru_cache(maxsize=None)
def table_yardstick(active):
    """The yardstick's largest ratios over every case of the table with this active degree (synthetic upstream) -> dict(color, dsh, pos)."""
    out = dict(color=0.0, dsh=0.0, pos=0.0)
    for key in table():
        if key[3] == active:
            r = yardstick_ratios(get_case(key))
            for q in out:
                out[q] = max(out[q], r[q])
    return out


def bars(case, yard=None):
    """MARGIN x the yardstick's largest ratios over the table's cases of this active degree: `yard` (the GPU test's, measured on the
    kernels' own dL/dcolour, clamp bits and projection terms), else table_yardstick (synthetic upstream)."""
    ty = table_yardstick(case.active) if yard is None else yard
    return {q: MARGIN * ty[q] for q in ("color", "dsh", "pos")}


def verdict(case, got, g, b, yard=None):
    """All checks of one result `got` = dict(color [P,3], neg [P,3] bool, dsh [P,M,3], a [P,3]) computed from dL/dcolour g and the projection
    term b -> (list of failures, figures).  Used on the kernels (tests/test_gpu_sh.py) and on the yardstick's variants."""
    ref = evaluate(case, np.float64)
    bar = bars(case, yard)
    vis = case.visible
    fails, fig = [], {}
    if not np.all(np.isfinite(np.asarray(got["color"])[vis])):
        fails.append("a visible row's colour is not finite")
    fig["color"] = color_ratio(case, got["color"], ref)
    if fig["color"] > bar["color"]:
        fails.append(f"colour: {fig['color']:.3g} u over the bar {bar['color']:.3g} u")
    wrong, band = clamp_mismatches(case, got["neg"], ref, bar["color"])
    if wrong:
        fails.append(f"{wrong} clamp bits differ from v64 < 0 outside the band")
    fig["band"] = band                                                 # (capped over the whole table: tests/test_sh_anchor_cpu.py)
    bw64 = backward(case, ref, g, got["neg"])
    fig["dsh"] = dsh_ratio(case, got["dsh"], bw64)
    if fig["dsh"] > bar["dsh"]:
        fails.append(f"dL/dSH: {fig['dsh']:.3g} u over the bar {bar['dsh']:.3g} u")
    fails += dsh_exact_zeros(case, got["dsh"], got["neg"])
    fig["pos"] = position_ratio(case, got["a"], b, bw64.t)
    if fig["pos"] > bar["pos"]:
        fails.append(f"direction term of dL/dmeans3D: {fig['pos']:.3g} u over the bar {bar['pos']:.3g} u")
    fig["bar"] = bar
    return fails, fig


def variant_result(case, variant, g, b):
    """What a kernel with this defect would hand to `verdict`."""
    y = evaluate(case, np.float32, variant)
    bw = backward(case, y, g, y.neg)
    with np.errstate(invalid="ignore"):
        return dict(color=y.color, neg=y.neg, dsh=bw.dsh, a=np.asarray(b, np.float32) + bw.t.astype(np.float32))
