"""GPU: the spherical-harmonics kernels (csrc/sh.hip k_sh_forward / k_sh_backward / k_sh16_forward / k_sh16_backward, CAT and SPLIT)
against float64 over every layout, active degree and visibility pattern of tests/sh_anchor.py's table: one 32 x 32 forward and
deterministic backward per case through _C.rasterize_gaussians(_backward), and the same geometry once more with the record's colours as
colors_precomp (the twin), whose dL/dmeans3D is the projection term alone.  Every gradient array is carved from a NaN-filled buffer for
the duration of a test, so a word a kernel never writes shows.  Bars (tests/sh_anchor.py): MARGIN x the float32 yardstick's largest
ratio over the cases of the same active degree, measured here on the kernels' own inputs -- the first test of a degree runs all its cases."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sh_anchor as sa
from tests.common import seeded_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DET = 0x20                                                             # EGS_CALL_DETERMINISTIC: the twin's sums are the SH run's, bit for bit
KEYS = sa.table()
FIGURES = {}                                                           # case id -> the figures of its checks (printed by the last test)


@pytest.fixture(autouse=True)
def _nan_filled_gradient_arrays(monkeypatch):
    """_C._carve with its one allocation NaN-filled: same offsets, same 256-byte alignment of every view."""
    from egogaussian_amd import _C
    plain = _C._carve

    def carve(dev, shapes):
        out = plain(dev, shapes)
        bases = {id(v._base): v._base for v in out if v is not None}   # the views share the one buffer they were cut from
        assert len(bases) <= 1 and all(v.data_ptr() % 256 == 0 for v in out if v is not None)
        for buf in bases.values():
            buf.fill_(float("nan"))
        return out
    carve.poisons = True
    monkeypatch.setattr(_C, "_carve", carve)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _sh_tensors(case, layout):
    """(sh, sh_rest or None) on the device in this layout; split-unaligned: the rest block starts 4 bytes past a 16-byte boundary."""
    shs = case.shs.to(DEV)
    if layout == "cat":
        return shs.contiguous(), None
    dc = shs[:, :1].clone()                                            # (a copy even at P = 1, where the slice is contiguous as it stands)
    if layout == "split":
        rest = shs[:, 1:].clone()
    else:
        store = torch.zeros(case.P * (case.M - 1) * 3 + 1, device=DEV)
        store[1:] = shs[:, 1:].reshape(-1)
        rest = store[1:].view(case.P, case.M - 1, 3)
        assert rest.data_ptr() % 16 == 4
    assert dc.data_ptr() % 16 == 0 and (layout == "split-unaligned" or rest.data_ptr() % 16 == 0)
    return dc, rest


def _forward_backward(case, sh, sh_rest, colors):
    from egogaussian_amd import _C
    assert getattr(_C._carve, "poisons", False), "the backward's gradient arrays are not NaN-filled"
    cam = case.cam
    e = torch.empty(0, device=DEV)
    t = lambda x: x.to(DEV)
    bg, p, op, cov = t(case.bg), t(case.means3D), t(case.opacities), t(case.cov3D_precomp)
    view, proj, campos = t(cam.viewmatrix), t(cam.projmatrix), t(cam.campos)
    col = e if colors is None else colors
    sh_arg = e if sh is None else sh
    out = _C.rasterize_gaussians(bg, p, col, op, e, e, 1.0, cov, view, proj, cam.tanfovx, cam.tanfovy, sa.H, sa.W, sh_arg, case.active, campos,
                                 False, DET, sh_rest=sh_rest)
    R, color, depth, alpha, radii, geom, binning, img = out
    gv = _C.geom_views(geom, case.P)
    rec_color, clamped = gv["rec"][:, 6:9].clone(), gv["clamped"].clone()
    gc, gd, ga = [t(x) for x in seeded_grads(sa.H, sa.W, 5)]
    hb = _C.rasterize_gaussians_backward(bg, p, radii, col, e, e, 1.0, cov, view, proj, cam.tanfovx, cam.tanfovy, gc, gd, ga, sh_arg, case.active,
                                         campos, geom, R, binning, img, alpha, DET, sh_rest=sh_rest)
    torch.cuda.synchronize()
    return dict(radii=radii, rec_color=rec_color, clamped=clamped, image=color, dcolors=hb[1], dmeans3D=hb[3], dsh=hb[5],
                dsh_rest=hb[8] if sh_rest is not None else None)


@functools.lru_cache(maxsize=None)
def _twin(data_key):
    """The case's data (whatever the layout) with its concatenated SH run -> (cat run, colours-mode twin of the same geometry)."""
    P, M, active, pattern = data_key
    case = sa.get_case((P, M, "cat", active, pattern))
    sh, _ = _sh_tensors(case, "cat")
    cat = _forward_backward(case, sh, None, None)
    colors = cat["rec_color"].clone()                                  # bit copies; a culled row's record is never written
    colors[~torch.from_numpy(case.visible).to(DEV)] = 0.0
    return cat, _forward_backward(case, None, None, colors)


def _run(key):
    case = sa.get_case(key)
    cat, twin = _twin((case.P, case.M, case.active, case.pattern))
    if case.layout == "cat":
        return case, cat, cat, twin
    sh, rest = _sh_tensors(case, case.layout)
    return case, _forward_backward(case, sh, rest, None), cat, twin


def _full_dsh(res):
    return res["dsh"] if res["dsh_rest"] is None else torch.cat((res["dsh"], res["dsh_rest"]), dim=1)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    """The runs of a case and what its backward checks take from them: the kernel's own clamp bits and dL/dcolour g (the SH backward's
    inputs) and the twin's dL/dmeans3D b (the projection term the direction term is added to)."""
    case, res, cat, twin = _run(key)
    clamped = res["clamped"].cpu().numpy()
    neg = ((clamped[:, None] >> np.arange(3)) & 1).astype(bool)
    neg[~case.visible] = False                                         # (a culled row's byte is never written)
    return SimpleNamespace(case=case, res=res, cat=cat, twin=twin, clamped=clamped, neg=neg, g=res["dcolors"].cpu().numpy(),
                           b=twin["dmeans3D"].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _degree_yardstick(active):
    """The float32 yardstick's largest error / unit ratios over every case of the table with this active degree, on the inputs the kernels
    had in this run -- what the bars are MARGIN times of."""
    out = dict(color=0.0, dsh=0.0, pos=0.0)
    for key in KEYS:
        if key[3] == active:
            x = _inputs(key)
            assert np.isfinite(x.g).all() and np.isfinite(x.b).all(), f"{x.case.id}: dL/dcolours or the twin's dL/dmeans3D is not finite"
            r = sa.yardstick_ratios(x.case, g=x.g, b=x.b, neg=x.neg)
            assert not r["zeros"], (x.case.id, r["zeros"])
            for q in out:
                out[q] = max(out[q], r[q])
    assert all(np.isfinite(v) for v in out.values()), out
    return out


@pytest.mark.parametrize("key", KEYS, ids=sa.case_id)
def test_case_against_float64(key):
    x = _inputs(key)
    case, res, cat, twin, neg = x.case, x.res, x.cat, x.twin, x.neg
    vis = case.visible
    # ---- forward: the case is what it claims, the twin has its geometry
    assert np.array_equal((res["radii"] > 0).cpu().numpy(), vis), "radii > 0 is not the intended pattern"
    assert torch.equal(res["radii"], twin["radii"]) and torch.equal(_bits(res["image"]), _bits(twin["image"]))
    upper = np.uint8(0xFF & ~sa.CLAMP_MASK)
    assert np.array_equal((x.clamped & upper)[vis], (twin["clamped"].cpu().numpy() & upper)[vis]), "bits 3-5 of `clamped` changed"
    color = res["rec_color"].cpu().numpy()
    assert np.array_equal(color[vis] == 0, neg[vis] | (color[vis] == 0)), "a channel flagged clamped holds a colour"
    # ---- backward: the kernel's own dL/dcolour is the SH backward's input; the twin's is the same sums
    assert torch.equal(_bits(res["dcolors"]), _bits(twin["dcolors"])), "dL/dcolours of the SH run and of its colours-mode twin differ"
    assert np.isfinite(res["dmeans3D"].cpu().numpy()).all()
    yard = _degree_yardstick(case.active)
    got = dict(color=color, neg=neg, dsh=_full_dsh(res).cpu().numpy(), a=res["dmeans3D"].cpu().numpy())
    fails, fig = sa.verdict(case, got, x.g, x.b, yard=yard)
    FIGURES[case.id] = fig
    print(f"{case.id} {sa.expected_path(case)[0]}: kernel / yardstick of the degree (u)  " + "  ".join(f"{q} {fig[q]:.2f} / {yard[q]:.2f}" for q in ("color", "dsh", "pos")))
    assert not fails, fails
    # ---- every layout of a case gives the concatenated call's bits
    vis_t = torch.from_numpy(vis)
    assert torch.equal(_bits(res["rec_color"])[vis_t], _bits(cat["rec_color"])[vis_t]), "the record's colours differ from the concatenated call's"
    assert torch.equal(_bits(_full_dsh(res)), _bits(_full_dsh(cat))), "dL/dSH differs from the concatenated call's"
    if res["dsh_rest"] is not None:
        assert res["dsh"].shape == (case.P, 1, 3) and res["dsh_rest"].shape == (case.P, case.M - 1, 3)


def test_yardstick_ratios_of_this_run():
    """The figures the bars are MARGIN times of, per active degree, next to the kernels' largest ratios (over the cases that ran)."""
    for active in range(4):
        yard = _degree_yardstick(active)
        ran = [f for cid, f in FIGURES.items() if f"-D{active}-" in cid]
        worst = {q: max((f[q] for f in ran), default=0.0) for q in yard}
        print(f"active degree {active}, {len(ran)} cases: " + "  ".join(f"{q}: kernel {worst[q]:.2f} u, yardstick {yard[q]:.2f} u" for q in yard))
        assert all(yard[q] > 0 for q in ("color", "dsh")) and (yard["pos"] > 0) == (active > 0), yard
