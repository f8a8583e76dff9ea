"""CPU: frame ingest -- the torch statement of the reference's load path (ingest.resize_u8 / binarize / target_size) against what the
reference itself recorded (tests/golden/ingest.npz, written by tests/golden/make_golden_ingest.py from PILtoTorch, binarize_mask and loadCam),
the numpy coefficient tables against the library's, six plausible wrong statements that the fixture must tell apart, the C ABI of the three
new entries and their argument errors, and what FrameIngest refuses.  The definition is integer arithmetic: every comparison is an equality."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_resample_ksize", "egs_resample_tables", "egs_frame_ingest")


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ingest.npz"))


def cases(g):
    """-> [(k, (h, w), (W, H))]"""
    return [(k, (int(r[0]), int(r[1])), (int(r[2]), int(r[3]))) for k, r in enumerate(g["cases"])]


# ---- the statement equals the reference ----------------------------------------------------------------------------------------------------
def test_statement_equals_every_recorded_case():
    from egogaussian_amd import ingest
    g = golden()
    assert len(g["cases"]) == 9
    for k, (h, w), size in cases(g):
        assert g[f"img_{k}"].shape == (h, w, 3) and g[f"mask_l_{k}"].shape == (h, w) and g[f"mask_rgb_{k}"].shape == (h, w, 3)
        for name in ("img", "mask_l", "mask_rgb"):
            got = ingest.resize_u8(g[f"{name}_{k}"], size)
            want = torch.from_numpy(g[f"{name}_out_{k}"])
            assert got.dtype == torch.uint8 and torch.equal(got, want), (k, name, int((got != want).sum()))
            if name != "img":
                assert torch.equal(ingest.binarize(got), torch.from_numpy(g[f"{name}_bin_{k}"]).bool()), (k, name)
    kinds = set(g["mask_kinds"].reshape(-1).tolist())
    assert {"rect", "pixels", "ones", "blue", "zero", "full"} <= kinds


def test_target_size_is_loadcam_rule():
    from egogaussian_amd import ingest
    g = golden()
    rows, scales = g["size_rows"], g["size_resolution_scale"]
    assert len(rows) == 7 and 2.0 in scales.tolist()
    for (ow, oh, res, W, H), rs in zip(rows.tolist(), scales.tolist()):
        assert ingest.target_size(ow, oh, res, rs) == (W, H), (ow, oh, res, rs)
    assert ingest.target_size(1920, 1080) == (1600, 900) and ingest.target_size(1002, 701, 4) == (250, 175)      # round(250.5): half to even


# ---- the coefficients: numpy float64 against the library's double ---------------------------------------------------------------------------
def test_tables_equal_the_library_word_for_word():
    from egogaussian_amd import ingest, lib
    L = lib.load()
    pairs = {(1080, 900), (1920, 1600)}
    for _, (h, w), (W, H) in cases(golden()):
        pairs |= {(w, W), (h, H)}
    for n_in, n_out in sorted(pairs):
        kk, bounds = ingest.resample_tables(n_in, n_out)
        ks = L.egs_resample_ksize(n_in, n_out)
        assert ks == kk.shape[1] == ingest.ksize_of(n_in, n_out) and kk.shape[0] == n_out and bounds.shape == (n_out, 2)
        kk2, b2 = np.full((n_out, ks), -7, np.int32), np.full((n_out, 2), -7, np.int32)
        assert L.egs_resample_tables(n_in, n_out, kk2.ctypes.data, b2.ctypes.data) == 0
        assert np.array_equal(kk, kk2) and np.array_equal(bounds, b2), (n_in, n_out)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ks).all()
    assert L.egs_resample_ksize(256, 32) == 33 and L.egs_resample_ksize(1920, 1600) == 7 and L.egs_resample_ksize(20, 64) == 5
    assert L.egs_resample_ksize(0, 5) == 0 and L.egs_resample_ksize(5, 0) == 0


def test_statement_equals_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    from egogaussian_amd import ingest
    rng = np.random.default_rng(77)
    for n in range(40):
        h, w, H, W = (int(v) for v in rng.integers(1, 48, 4))
        if n % 5 == 0:
            W = w
        if n % 7 == 0:
            H = h
        c = (1, 3)[n % 2]
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        if n % 3 == 0:
            a = np.where(a > 200, 255, 0).astype(np.uint8)                         # hard edges: the clamp of both passes
        src = a[:, :, 0] if c == 1 else a
        want = np.array(Image.fromarray(src).resize((W, H)))
        got = ingest.resize_u8(src, (W, H)).numpy()
        assert np.array_equal(got, want), (n, h, w, W, H, c)


# ---- wrong statements: the fixture must catch each ---------------------------------------------------------------------------------------------
def _float_weights(n_in, n_out):
    """The normalised bicubic weights in float64, not quantised: [n_out, ksize], and xmin."""
    from egogaussian_amd import ingest
    _, bounds = ingest.resample_tables(n_in, n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    center = (np.arange(n_out) + 0.5) * scale
    x = np.arange(ingest.ksize_of(n_in, n_out))[None, :]
    w = np.where(x < bounds[:, 1:2], ingest._bicubic((x + bounds[:, 0:1] - center[:, None] + 0.5) / fs), 0.0)
    return w / w.sum(1, keepdims=True), bounds[:, 0]


def _float_pass(v, n_out, axis, weights):
    """One pass on float64 [h, w, C] with the given weights; no rounding."""
    n_in = v.shape[axis]
    w, lo = weights(n_in, n_out)
    shape = [1, 1, 1]
    shape[axis] = n_out
    acc = np.zeros([n_out if d == axis else s for d, s in enumerate(v.shape)])
    for k in range(w.shape[1]):
        acc += np.take(v, np.minimum(lo + k, n_in - 1), axis=axis) * w[:, k].reshape(shape)
    return acc


def _fixed_weights(n_in, n_out):
    from egogaussian_amd import ingest
    kk, bounds = ingest.resample_tables(n_in, n_out)
    return kk.astype(np.float64) / float(1 << 22), bounds[:, 0]


def _wrong_vertical_first(a, size):
    from egogaussian_amd import ingest
    v = torch.from_numpy(a).to(torch.int32)
    if v.shape[0] != size[1]:
        v = ingest._pass(v, size[1], 0)
    if v.shape[1] != size[0]:
        v = ingest._pass(v, size[0], 1)
    return v.to(torch.uint8).numpy()


def _wrong_two_float_passes(weights):
    def f(a, size):
        v = a.astype(np.float64)
        if v.shape[1] != size[0]:
            v = _float_pass(v, size[0], 1, weights)
        if v.shape[0] != size[1]:
            v = _float_pass(v, size[1], 0, weights)
        return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    return f


def _wrong_interpolate(a, size):
    x = torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0).float()
    y = torch.nn.functional.interpolate(x, size=(size[1], size[0]), mode="bicubic", antialias=True, align_corners=False)
    return y.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).numpy()


def test_wrong_resizes_fail_against_the_fixture():
    g = golden()
    wrong = {"vertical before horizontal": _wrong_vertical_first,
             "no rounding between the passes": _wrong_two_float_passes(_fixed_weights),
             "float coefficients, one final rounding": _wrong_two_float_passes(_float_weights),
             "F.interpolate(bicubic, antialias=True)": _wrong_interpolate}
    for name, fn in wrong.items():
        caught = [k for k, _, size in cases(g) if not np.array_equal(fn(g[f"img_{k}"], size), g[f"img_out_{k}"])]
        print(name, "caught by cases", caught)
        assert caught, f"the fixture cannot tell '{name}' from the reference"


def test_wrong_binarisations_fail_against_the_fixture():
    from egogaussian_amd import ingest
    g = golden()
    at_128, before = [], []
    for k, _, size in cases(g):
        for name in ("mask_l", "mask_rgb"):
            src, want = g[f"{name}_{k}"], g[f"{name}_bin_{k}"].astype(bool)
            resized = ingest.resize_u8(src, size).numpy()
            if not np.array_equal((resized >= 128) if resized.ndim == 2 else (resized >= 128).any(-1), want):
                at_128.append((k, name))
            first = np.where(src > 0, 255, 0).astype(np.uint8)
            if not np.array_equal(ingest.binarize(ingest.resize_u8(first, size)).numpy(), want):
                before.append((k, name))
    print("binarising at >= 128 caught by", at_128, "; binarising before resizing caught by", before)
    assert at_128 and before


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from egogaussian_amd import lib
    L = lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egs_raster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", text))
    for n in NEW:
        assert n in declared and n in lib.SIGNATURES and hasattr(L, n), n
    assert L.egs_abi_version() == 6
    for name, value in (("IMAGE", lib.INGEST_IMAGE), ("HAND_MASK", lib.INGEST_HAND_MASK), ("OBJ_MASK", lib.INGEST_OBJ_MASK)):
        assert re.search(r"#define\s+EGS_INGEST_%s\s+%d\b" % (name, value), text), name
    assert "ingest.hip" in open(os.path.join(ROOT, "egogaussian_amd", "csrc", "Makefile")).read()


def test_ingest_argument_errors_precede_device_work():
    from egogaussian_amd import lib
    L = lib.load()
    p = 4096                                                           # (fake non-null pointers are never dereferenced before the checks)
    GATED, OBJ, LABEL = lib.FRAME_GATED, lib.FRAME_OBJECT_LOSS, lib.FRAME_LABEL_PHASE
    IMG, HAND, MASK = lib.INGEST_IMAGE, lib.INGEST_HAND_MASK, lib.INGEST_OBJ_MASK

    def call(H=8, W=8, flags=GATED, F=3, i=1, plane=IMG, img=p, bits=p, src=p, h=16, w=16, c=3, kh=p, bh=p, kv=p, bv=p):
        return L.egs_frame_ingest(H, W, flags, F, i, plane, img, bits, src, h, w, c, kh, bh, kv, bv, None)

    ARG, MODE, RANGE = -1, -2, -3
    for kw, want in [(dict(H=0), ARG), (dict(W=-1), ARG), (dict(F=0), ARG), (dict(h=0), ARG), (dict(w=0), ARG), (dict(i=-1), ARG), (dict(i=3), ARG),
                     (dict(flags=64), ARG), (dict(plane=3), ARG), (dict(plane=-1), ARG),
                     (dict(c=1), ARG), (dict(c=4), ARG), (dict(plane=HAND, c=2), ARG), (dict(plane=HAND, c=4), ARG),
                     (dict(src=None), ARG), (dict(img=None), ARG), (dict(plane=HAND, bits=None), ARG),
                     (dict(flags=GATED | OBJ | lib.FRAME_DYNAMIC | lib.FRAME_MOTION, bits=None), ARG),      # the image launch reads the object plane
                     (dict(kh=None), ARG), (dict(bh=None), ARG), (dict(kv=None), ARG), (dict(bv=None), ARG),
                     (dict(flags=0, plane=HAND, c=1), MODE), (dict(plane=MASK, c=1), MODE), (dict(flags=LABEL, plane=IMG), MODE),
                     (dict(flags=LABEL | OBJ), MODE), (dict(flags=lib.FRAME_POSE_ROWS), MODE),
                     (dict(h=65), RANGE), (dict(w=65), RANGE), (dict(h=40000, H=40000), RANGE), (dict(W=32768, w=32768), RANGE),
                     (dict(h=32768, H=32767), RANGE),
                     (dict(h=65, src=None), RANGE)]:                                      # (the sizes come first)
        assert call(**kw) == want, (kw, want)
    # the tables of an axis that does not change are not needed; (a complete call would launch: not made here)
    assert L.egs_resample_tables(0, 4, p, p) == ARG and L.egs_resample_tables(4, 0, p, p) == ARG
    assert L.egs_resample_tables(4, 4, None, p) == ARG and L.egs_resample_tables(4, 4, p, None) == ARG


# ---- what FrameIngest refuses (a CPU store: no kernel call) -------------------------------------------------------------------------------------------
def test_frame_ingest_refusals():
    from egogaussian_amd.frames import FrameStore
    from egogaussian_amd.ingest import FrameIngest
    store = FrameStore(8, 8, 2, "cpu", gated=True)
    with pytest.raises(ValueError, match=r"HIP device.*Pillow.*put\(\)"):
        FrameIngest(store, (16, 16))
    for hw in ((65, 16), (16, 65), (0, 16), (32768, 16)):
        with pytest.raises(ValueError, match=r"supported range.*Pillow.*put\(\)"):
            FrameIngest(store, hw)
    src = FrameIngest.source
    ok = src(np.zeros((16, 12, 3), np.uint8), "image", 16, 12, (3,))
    assert ok.shape == (16, 12, 3) and ok.dtype == torch.uint8
    assert src(torch.zeros((16, 12), dtype=torch.uint8), "hand_mask", 16, 12, (1, 3)).shape == (16, 12, 1)
    refused = [(np.zeros((16, 12, 3), np.float32), (3,), "uint8"), (np.zeros((16, 12), np.uint8), (3,), "uint8"),
               (np.zeros((12, 16, 3), np.uint8), (3,), "uint8"), (np.zeros((16, 12, 2), np.uint8), (1, 3), "uint8"),
               (np.zeros((16, 12, 4), np.uint8), (3,), "premultiplies alpha"), (np.zeros((16, 12, 4), np.uint8), (1, 3), "premultiplies alpha"),
               (np.zeros((16, 12), bool), (1, 3), "nearest")]
    for a, channels, why in refused:
        with pytest.raises(ValueError, match=rf"{why}.*Pillow.*put\(\)"):
            src(a, "x", 16, 12, channels)

    class Pal:                                                                    # what a PIL image of mode P / 1 looks like to the check
        def __init__(self, mode):
            self.mode = mode

        def __array__(self, *a, **kw):
            return np.zeros((16, 12), np.uint8)
    for mode in ("P", "1"):
        with pytest.raises(ValueError, match=r"palette or bilevel.*nearest.*Pillow.*put\(\)"):
            src(Pal(mode), "obj_mask", 16, 12, (1, 3))
    assert src(Pal("L"), "obj_mask", 16, 12, (1, 3)).shape == (16, 12, 1)
