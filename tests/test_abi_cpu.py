"""CPU: the C-ABI library loads, exports every symbol include/egs_raster.h declares, sizes/layouts are sane and
argument errors are reported before any device work.  No compute calls (there is no GPU here)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "egs_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from egogaussian_amd import lib
    L = lib.load()
    names = _declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/egs_raster.h but not exported"
    assert set(lib.SIGNATURES) == set(names), "python binding table and header disagree"
    assert L.egs_abi_version() == lib.ABI_VERSION


def test_sizes_and_layouts():
    from egogaussian_amd import lib
    L = lib.load()
    assert L.egs_geom_bytes(0) >= 0 and L.egs_geom_bytes(1000) < L.egs_geom_bytes(2000)
    assert L.egs_geom_bytes(500000) >= 500000 * (48 + 8 + 4 + 1)
    assert L.egs_binning_bytes(500000, 10**6, 960, 540) >= 10**6 * 20
    assert L.egs_image_bytes(960, 540) >= 960 * 540 * 8 + 60 * 34 * 8
    assert L.egs_backward_scratch_bytes(1000) >= 48000
    g = lib.GeomLayout(); assert L.egs_get_geom_layout(1000, C.byref(g)) == 0
    offs = [g.rec, g.rect, g.offsets, g.clamped, g.scan_scratch, g.total]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[-1] + 8 <= L.egs_geom_bytes(1000)
    b = lib.BinningLayout(); assert L.egs_get_binning_layout(500000, 5000, 960, 540, C.byref(b)) == 0
    assert b.key_bits == 32 + 11 and b.index_passes == 3 and b.bin_blocks == 489     # 60 x 34 = 2040 tiles -> 11 bits; 19 index bits
    assert b.point_list == 0 < b.pairs < b.scratch < b.table < b.spine       # the backward only needs point_list (offset 0)
    assert L.egs_get_binning_layout(1000000, 5000, 1920, 1080, C.byref(b)) == 0 and b.key_bits == 45 and b.index_passes == 3
    assert L.egs_get_binning_layout(200, 5000, 64, 64, C.byref(b)) == 0 and b.key_bits == 37 and b.index_passes == 1 and b.bin_blocks == 1     # workgroups of whole 256-Gaussian blocks, sized by P (binning.hip egs_bin_gpb)
    i = lib.ImageLayout(); assert L.egs_get_image_layout(100, 70, C.byref(i)) == 0 and i.ranges < i.final_T < i.n_contrib
    assert i.n_contrib < i.quad_work < i.tile_order < i.quad_pairs and i.quad_pairs + 7 * 5 * 8 * 4 <= L.egs_image_bytes(100, 70)
    assert L.egs_abi_version() == 6 and L.egs_knn3_grid_scratch_bytes(0) == 0 and L.egs_knn3_grid_scratch_bytes(100000) > 100000 * 20
    assert L.egs_knn3_grid(5, None, None, None, None) == -1 and L.egs_knn3_grid(0, None, None, None, None) == 0
    # ABI 5: the placement buffer = 4 cost words per tile + the tile-order words + (256-byte aligned) eight sums words per tile;
    # which forwards fold the count pass of the bucketing into the preprocess launch (one round of <= 16 groups per workgroup)
    nt = 60 * 34
    assert L.egs_placement_bytes(960, 540) == ((nt * 4 + L.egs_order_words(960, 540)) * 4 + 255) // 256 * 256 + 8 * nt * 4
    assert L.egs_placement_bytes(0, 540) == 0 and L.egs_placement_init(None, 960, 540, None) == -1
    fuses = lambda P, W, H, flags=0: L.egs_forward_fuses_count(P, W, H, flags)
    assert fuses(500000, 960, 540) == 1 and fuses(100000, 960, 540) == 1 and fuses(253202, 960, 540) == 1 and fuses(1, 64, 64) == 1
    assert fuses(1000000, 1920, 1080) == 0        # four rounds of eight groups per workgroup: the separate count launch
    assert fuses(0, 960, 540) == 0
    # ABI 6: a per-call flag, not a process-wide switch -- the answer for one call's flags says nothing about the next call's
    assert fuses(500000, 960, 540, lib.CALL_SEPARATE_COUNT) == 0 and fuses(500000, 960, 540) == 1
    assert fuses(500000, 960, 540, lib.CALL_KEEP_ALL_INSTANCES | lib.CALL_SYNC | lib.CALL_SEPARATE_SORT | lib.CALL_BALLOT_RANK) == 1
    # which launches sort the tile lists (added within ABI 6): host arithmetic on the CAPACITY, the tile count and the call's flags
    plan = lambda P, cap, W, H, flags=0: L.egs_forward_sort_plan(P, cap, W, H, flags)
    IN_BLEND, SECOND, BALLOT = lib.SORT_IN_BLEND, lib.SORT_SECOND_INSTANTIATION, lib.SORT_BALLOT_RANK
    hdr = open(os.path.join(ROOT, "include", "egs_raster.h")).read()
    assert [int(re.search(rf"#define\s+EGS_SORT_{n}\s+0x([0-9a-f]+)", hdr).group(1), 16) for n in ("IN_BLEND", "SECOND_INSTANTIATION", "BALLOT_RANK")] == [IN_BLEND, SECOND, BALLOT]
    assert plan(500000, 2040 * 2048, 960, 540) == IN_BLEND and plan(500000, 2040 * 2048 + 1, 960, 540) == SECOND      # 2040 tiles: `solo` up to 2048 per tile
    assert plan(3000, 32768, 64, 64) == IN_BLEND and plan(3000, 32769, 64, 64) == SECOND                               # 16 tiles
    assert plan(3000, 32768, 49, 64) == IN_BLEND and plan(3000, 32768, 48, 64) == SECOND                               # ragged image: 16 tiles / 12 tiles
    assert plan(3000, 32768, 64, 64, lib.CALL_SEPARATE_SORT) == 0 and plan(3000, 32768, 64, 64, lib.CALL_SYNC) == 0   # kept out of the blend
    assert plan(3000, 32768, 64, 64, lib.CALL_BALLOT_RANK) == IN_BLEND | BALLOT and plan(3000, 32769, 64, 64, lib.CALL_BALLOT_RANK) == SECOND | BALLOT
    assert plan(3000, 32768, 64, 64, lib.CALL_KEEP_ALL_INSTANCES | lib.CALL_SEPARATE_COUNT) == IN_BLEND                # not the sort's flags
    assert plan(3000, 32769, 64, 64, lib.CALL_SEPARATE_SORT | lib.CALL_SYNC) == SECOND
    assert plan(0, 32768, 64, 64) == 0 and plan(0, 32769, 64, 64, lib.CALL_BALLOT_RANK) == 0 and plan(3000, 0, 64, 64) == 0
    # the Python wrapper: the module's default flags are ORed in; a forward that fits its capacity never sees CALL_SYNC (its chain is not
    # synchronised mid-way), the retry of one that did not fit does
    from egogaussian_amd import _C
    assert _C.sort_plan(3000, 64, 64, 32768) == IN_BLEND and _C.sort_plan(3000, 64, 64, 32769, debug=_C.CALL_BALLOT_RANK) == SECOND | BALLOT
    assert _C.sort_plan(3000, 64, 64, 32768, debug=True) == IN_BLEND and _C.sort_plan(3000, 64, 64, 32768, debug=True, retried=True) == 0
    old = _C.set_sort_in_blend(False)
    try:
        assert _C.sort_plan(3000, 64, 64, 32768) == 0
    finally:
        _C.set_sort_in_blend(old)
    assert _C.sort_plan(3000, 64, 64, 32768) == IN_BLEND
    # the launch geometry of the bucketing (added within ABI 6): host arithmetic on the model size, the image size and the culling flag
    q = lib.BinGeometry()
    geo = lambda P, W, H, flags=0: (L.egs_forward_bin_geometry(P, W, H, flags, C.byref(q)), {n: int(getattr(q, n)) for n, _ in lib.BinGeometry._fields_})[1]
    assert re.search(r"int32_t n_tiles, gx, nblocks, stride, n_chunks, gpr, cull, use_map, groups_per_block, rounds, prefixed, can_fuse;\s*int64_t lds;", hdr)
    assert C.sizeof(lib.BinGeometry) == 12 * 4 + 8
    g = geo(500000, 960, 540)
    assert (g["n_tiles"], g["gx"], g["nblocks"], g["stride"], g["n_chunks"]) == (2040, 60, 489, 512, 510)
    assert L.egs_get_binning_layout(500000, 5000, 960, 540, C.byref(b)) == 0 and (g["nblocks"], g["stride"]) == (b.bin_blocks, b.table_stride)
    assert (g["gpr"], g["groups_per_block"], g["rounds"], g["cull"], g["use_map"], g["prefixed"], g["can_fuse"]) == (16, 16, 1, 1, 1, 0, 1)
    assert geo(500000, 960, 540, lib.CALL_KEEP_ALL_INSTANCES)["cull"] == 0 and geo(500000, 960, 540, lib.CALL_SEPARATE_COUNT) == g      # the possibility, not this call's choice
    g = geo(1000000, 1920, 1080)
    assert (g["gpr"], g["groups_per_block"], g["rounds"], g["can_fuse"]) == (8, 32, 4, 0) and fuses(1000000, 1920, 1080) == g["can_fuse"]
    assert geo(0, 64, 64) == dict(dict.fromkeys([n for n, _ in lib.BinGeometry._fields_], 0), n_tiles=16, gx=4)
    assert L.egs_forward_bin_geometry(10, 64, 64, 0, None) == -1 and L.egs_forward_bin_geometry(10, 8192, 8192, 0, C.byref(q)) == -3
    assert _C.bin_geometry(500000, 960, 540) == geo(500000, 960, 540) and _C.bin_geometry(3000, 64, 64, debug=_C.CALL_KEEP_ALL_INSTANCES)["cull"] == 0
    # ... and the library exports no setter of process-wide behaviour any more
    for gone in ("egs_debug_set_tile_culling", "egs_debug_set_fused_count", "egs_debug_set_sort_in_blend", "egs_debug_force_ballot_rank", "egs_debug_set_lossgrad"):
        assert not hasattr(L, gone), gone


def test_argument_errors_precede_device_work():
    from egogaussian_amd import lib
    L = lib.load()
    R = C.c_int64(-7)
    none = None
    # null required pointers
    rc = L.egs_forward_geometry(10, 0, 1, none, none, none, none, none, none, 1.0, none, none, 0, none, none, none, 64, 64, 1.0, 1.0, 0,
                                none, none, C.byref(R), none, none, none, 0)
    assert rc == -1 and R.value == 0
    assert L.egs_forward_geometry(-1, 0, 1, none, none, none, none, none, none, 1.0, none, none, 0, none, none, none, 64, 64, 1.0, 1.0, 0,
                                  none, none, C.byref(R), none, none, none, 0) == -1
    assert L.egs_forward_geometry(10, 0, 1, none, none, none, none, none, none, 1.0, none, none, 0, none, none, none, 70000, 64, 1.0, 1.0,
                                  0, none, none, C.byref(R), none, none, none, 0) == -3
    assert L.egs_forward_geometry(10, 0, 1, none, none, none, none, none, none, 1.0, none, none, 0, none, none, none, 8192, 8192, 1.0, 1.0,
                                  0, none, none, C.byref(R), none, none, none, 0) == -3      # 262144 tiles > 36864 (one LDS counter per tile)
    # P == 0 is a valid no-op
    assert L.egs_forward_geometry(0, 0, 0, none, none, none, none, none, none, 1.0, none, none, 0, none, none, none, 64, 64, 1.0, 1.0, 0,
                                  none, none, C.byref(R), none, none, none, 0) == 0 and R.value == 0
    # mode errors: both shs and colours given (fake non-null pointers are never dereferenced before the check)
    p = C.c_void_p(4096)
    assert L.egs_forward_geometry(10, 0, 1, p, p, none, p, p, none, 1.0, none, p, 0, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R),
                                  none, none, none, 0) == -2
    assert L.egs_forward_geometry(10, 0, 1, p, p, none, none, p, p, 1.0, none, none, 0, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R),
                                  none, none, none, 0) == -2      # scales without rotations
    assert L.egs_forward_geometry(10, 4, 25, p, p, none, none, p, none, 1.0, none, p, 0, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R),
                                  none, none, none, 0) == -3      # SH degree 4 unsupported
    assert L.egs_forward_geometry(10, 0, 1, p, p, none, none, p, none, 1.0, none, p, 1, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R),
                                  none, none, none, 0) == -2      # log-scale activation asked for, but the covariance is given
    assert L.egs_forward_geometry(10, 0, 1, p, p, none, none, p, p, 1.0, p, none, 8, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R),
                                  none, none, none, 0) == -2      # unknown activation flag
    assert L.egs_forward_geometry(10, 0, 1, p, p, p, none, p, none, 1.0, none, p, 0, p, p, p, 64, 64, 1.0, 1.0, 0, p, p, C.byref(R),
                                  none, none, none, 0) == -2      # split spherical harmonics need at least two coefficients
    assert b"exactly one" in L.egs_error_string(-2) and b"capacity" in L.egs_error_string(lib.RETRY_LARGER)
    # one-call forward: argument errors before any device work
    assert L.egs_forward(10, 0, 1, none, none, none, none, none, none, 1.0, none, none, 0, none, none, none, none, 64, 64, 1.0, 1.0, 0,
                         none, none, 100, none, none, none, none, none, none, C.byref(R), none, none, none, none, 0) == -1
    # opaque buffers must be 256-byte aligned (include/egs_raster.h, Conventions): refused before any device work
    q = C.c_void_p(4096 + 16)
    assert L.egs_forward_geometry(10, 0, 1, p, p, none, none, p, none, 1.0, none, p, 0, p, p, p, 64, 64, 1.0, 1.0, 0, p, q, C.byref(R),
                                  none, none, none, 0) == -1
    assert L.egs_forward_render(10, 100, p, 64, 64, p, q, p, p, p, p, none, 0) == -1
    assert L.egs_forward_render(10, 100, p, 64, 64, p, p, q, p, p, p, none, 0) == -1
    assert L.egs_placement_bytes(960, 540) >= (2040 * 4 + 2040) * 4 and L.egs_placement_bytes(0, 5) == 0
    assert L.egs_mark_visible(5, none, none, none, none, none) == -1


def test_pair_loss_argument_errors_precede_device_work():
    """egs_l1_ssim_pair_forward / _backward: every case returns from an argument check (api.hip, loss.hip: read there) before any launch; the
    fake non-null pointers are never dereferenced."""
    from egogaussian_amd import lib
    L = lib.load()
    p, none = C.c_void_p(4096), None
    fwd = lambda c=3, h=16, w=55, img=p, gt=p, partial=p, m0=p, m1=p, m2=p, l1=p, ss=p: L.egs_l1_ssim_pair_forward(c, h, w, img, gt, partial, m0, m1, m2, l1, ss, none)
    assert fwd(l1=none) == -1 and fwd(ss=none) == -1
    assert fwd(c=0) == -1 and fwd(h=0) == -1 and fwd(w=0) == -1 and fwd(c=-3) == -1 and fwd(h=-16) == -1 and fwd(w=-55) == -1
    assert fwd(m0=none) == -1 and fwd(m1=none) == -1 and fwd(m2=none) == -1
    assert fwd(img=none) == -1 and fwd(gt=none) == -1 and fwd(partial=none) == -1
    bwd = lambda c=3, h=16, w=55, img=p, gt=p, u1=p, u2=p, gate=none, m0=p, m1=p, m2=p, dimg=p: L.egs_l1_ssim_pair_backward(c, h, w, img, gt, u1, u2, gate, m0, m1, m2,
                                                                                                                       dimg, none, none)
    assert bwd(u1=none) == -1 and bwd(u2=none) == -1
    assert bwd(c=0) == -1 and bwd(h=0) == -1 and bwd(w=0) == -1 and bwd(c=-3) == -1 and bwd(h=-16) == -1 and bwd(w=-55) == -1
    assert bwd(m0=none) == -1 and bwd(m1=none) == -1 and bwd(m2=none) == -1 and bwd(dimg=none) == -1 and bwd(img=none) == -1 and bwd(gt=none) == -1
    assert bwd(gate=p, u2=none) == -1                                   # (the gate is optional: it changes no check)


_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t}
# pointers the binding types exactly: strings, and the HOST words a call writes (non-const: the caller passes byref); a pointer to a struct
# lib.py mirrors (egs_foo_bar -> lib.FooBar) is POINTER(that); every other pointer, the const HOST arrays included, is c_void_p
_OUT_WORDS = {"int64_t": C.POINTER(C.c_int64), "int": C.POINTER(C.c_int), "double": C.POINTER(C.c_double)}


def _ctype_of(decl, lib):
    """One parameter or return type of include/egs_raster.h (comments stripped, the parameter's name still on it) -> the ctypes type."""
    words = re.findall(r"[A-Za-z_0-9]+|\*", decl)
    const = "const" in words
    words = [w for w in words if w not in ("const", "struct")]
    base, stars = words[0], words.count("*")
    if stars == 0:
        return _SCALARS[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and not const and base in _OUT_WORDS:
        return _OUT_WORDS[base]
    mirror = getattr(lib, "".join(w.capitalize() for w in base.split("_")[1:]), None) if base.startswith("egs_") else None
    return C.POINTER(mirror) if stars == 1 and mirror is not None else C.c_void_p


def _declared_prototypes(lib):
    """name -> (restype, [argtypes]) of every function the header declares."""
    text = open(os.path.join(ROOT, "include", "egs_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^([a-z_0-9]+(?:\s+[a-z_0-9]+)*\s*\**)\s*\b(egs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = [q.strip() for q in params.split(",")]
        out[name] = (_ctype_of(ret, lib), [] if params == ["void"] else [_ctype_of(q, lib) for q in params])
    return out


def test_binding_table_matches_the_header_prototypes():
    """Arity, the type at every position and the return type of every entry of lib.SIGNATURES are those of the header's prototype."""
    from egogaussian_amd import lib
    protos = _declared_prototypes(lib)
    assert set(protos) == set(_declared_symbols()) == set(lib.SIGNATURES)
    for name, (res, args) in sorted(protos.items()):
        got_res, got_args = lib.SIGNATURES[name]
        assert got_res is res, f"{name}: return type {got_res} != {res}"
        assert len(got_args) == len(args), f"{name}: {len(got_args)} argtypes for {len(args)} parameters"
        for k, (g, w) in enumerate(zip(got_args, args)):
            assert g is w, f"{name}: parameter {k} is bound as {g}, the header says {w}"


# ---- return codes of the long entry points ---------------------------------------------------------------------------------------
# Every case below returns from an argument check of api.hip BEFORE any HIP call (read there, not tried): the fake pointers are never
# dereferenced and nothing is launched.  The expected codes are literals: -1 EGS_ERR_ARG, -2 EGS_ERR_MODE, -3 EGS_ERR_RANGE.
_P, _Q = 4096, 4096 + 8                        # a "valid" 256-byte aligned address and a misaligned one
_P2 = 8192
_FWD_BASE = dict(P=10, D=0, M=1, means=_P, shs=_P, rest=None, colors=None, opac=_P, scales=None, mod=1.0, rots=None, cov=_P, act=0,
                 view=_P, proj=_P, campos=_P, bg=_P, W=64, H=64, radii=_P, geom=_P, cap=100, binning=_P, image=_P, color=_P, depth=None,
                 alpha=None, pinned=_P, count=True, rmax=None, active=None, ovf=None, place=None, rot=None, flags=0)


def _forward(L, entry, **kw):
    a = dict(_FWD_BASE); a.update(kw)
    R = C.c_int64(-7)
    scene = [a["P"], a["D"], a["M"], a["means"], a["shs"], a["rest"], a["colors"], a["opac"], a["scales"], a["mod"], a["rots"], a["cov"],
             a["act"], a["view"], a["proj"], a["campos"]]
    count = C.byref(R) if a["count"] else None
    if entry == "egs_forward_geometry":
        return L.egs_forward_geometry(*scene, a["W"], a["H"], 1.0, 1.0, 0, a["radii"], a["geom"], count, a["active"], a["rot"], None, a["flags"])
    mid = [a["bg"], a["W"], a["H"], 1.0, 1.0, 0, a["radii"], a["geom"], a["cap"], a["binning"], a["image"], a["color"], a["depth"], a["alpha"], a["pinned"]]
    if entry == "egs_forward":
        return L.egs_forward(*scene, *mid, count, a["active"], a["place"], a["rot"], None, a["flags"])
    return L.egs_forward_enqueue(*scene, *mid, a["rmax"], a["active"], a["ovf"], a["place"], a["rot"], None, a["flags"])


def _motion(lib, A12=_P, M9=None, grad=None, scratch=None):
    om = lib.ObjectMotion()
    om.A12, om.rot.M9, om.grad, om.scratch = A12, M9, grad, scratch
    return om


def test_forward_return_codes():
    from egogaussian_amd import lib
    L = lib.load()
    ALL, ONE = ("egs_forward_geometry", "egs_forward", "egs_forward_enqueue"), ("egs_forward", "egs_forward_enqueue")
    rot_only = lib.ObjectRotation(); rot_only.M9 = _P
    om_no_A, om_grad, om_rot = _motion(lib, A12=None), _motion(lib, grad=_P), _motion(lib, M9=_P)
    table = [
        # bad dims
        (ALL, dict(P=-1), -1), (ALL, dict(W=0), -1), (ALL, dict(H=-5), -1),
        # range: 15-bit pixel coordinates, one LDS counter per tile
        (ALL, dict(W=70000), -3), (ALL, dict(H=40000), -3), (ALL, dict(W=8192, H=8192), -3),
        (ALL, dict(W=70000, means=None), -3),                                    # (the dims come first)
        # the instance capacity of the one-call forwards is an argument, not a range
        (ONE, dict(cap=2**31), -1), (ONE, dict(cap=-1), -1),
        (("egs_forward_geometry", "egs_forward"), dict(count=False), -1),
        # missing pointers
        (ONE, dict(bg=None), -1), (ONE, dict(image=None), -1), (ONE, dict(color=None), -1), (ONE, dict(depth=_P), -1), (ONE, dict(alpha=_P), -1),
        (ALL, dict(means=None), -1), (ALL, dict(opac=None), -1), (ALL, dict(view=None), -1), (ALL, dict(proj=None), -1),
        (ALL, dict(campos=None), -1), (ALL, dict(radii=None), -1), (ALL, dict(geom=None), -1),
        (("egs_forward",), dict(pinned=None), -1), (ONE, dict(binning=None), -1), (("egs_forward_enqueue",), dict(cap=0), -1),
        # misaligned opaque buffers
        (ALL, dict(geom=_Q), -1), (ONE, dict(binning=_Q), -1), (ONE, dict(image=_Q), -1),
        (ALL, dict(geom=_Q, colors=_P), -1),                                     # (before the modes)
        (("egs_forward",), dict(pinned=None, colors=_P), -1),                    # (so are the buffer checks of the one-call forward)
        # check_modes
        (ALL, dict(colors=_P), -2), (ALL, dict(shs=None), -2), (ALL, dict(scales=_P), -2), (ALL, dict(rots=_P), -2),
        (ALL, dict(scales=_P, rots=_P), -2), (ALL, dict(cov=None), -2), (ALL, dict(act=1), -2), (ALL, dict(act=2), -2), (ALL, dict(act=32), -2),
        (ALL, dict(act=16), -2),                                                 # a scalar colour is of colors_precomp
        (ALL, dict(colors=_P, D=4, M=25), -2),                                   # (before the SH range)
        # SH degree and coefficient range
        (ALL, dict(D=4, M=25), -3), (ALL, dict(D=-1), -3), (ALL, dict(D=2, M=4), -3), (ALL, dict(D=3, M=15), -3),
        (ALL, dict(D=4, M=25, rest=_P), -3),                                     # (before the split rule)
        # shs_rest without shs, or with a single coefficient
        (ALL, dict(rest=_P), -2), (ALL, dict(rest=_P, shs=None, colors=_P), -2),
        (ALL, dict(rest=_P, act=8), -2),
        # object rotation / object motion
        (ALL, dict(act=8), -2),                                                  # the bit without its struct
        (ALL, dict(act=8, rot=lib.rot_pointer(om_no_A)), -1), (ALL, dict(act=8, rot=lib.rot_pointer(om_grad)), -1),
        (ALL, dict(act=8, rot=lib.rot_pointer(om_rot)), -2),                     # a rotation needs scales + rotations
        (ALL, dict(rot=C.byref(rot_only)), -2),
    ]
    for entries, kw, want in table:
        for entry in entries:
            assert _forward(L, entry, **kw) == want, (entry, kw, want)
    # P == 0 with NULL everywhere: a no-op of egs_forward_geometry (the one-call forwards render the background: launches)
    nothing = {k: None for k in ("means", "shs", "opac", "cov", "view", "proj", "campos", "radii", "geom")}
    assert _forward(L, "egs_forward_geometry", P=0, M=0, **nothing) == 0
    assert _forward(L, "egs_forward_geometry", P=0, W=70000, **nothing) == -3


_BWD_BASE = dict(P=10, D=0, M=1, R=100, bg=_P, means=_P, shs=_P, rest=None, colors=None, scales=None, mod=1.0, rots=None, cov=_P, act=0,
                 view=_P, proj=_P, campos=_P, W=64, H=64, radii=_P, geom=_P, binning=_P, image=_P, g_color=_P, g_depth=None, g_alpha=None,
                 lg="valid", obj="valid", ent="valid", d2=_P, dcol=_P, dop=_P, d3=_P, dcov=_P, dsh=_P, drest=None, dscales=None, drots=None,
                 acc=None, den=None, maxr=None, skip=None, sink=None, prologue=0, rot=None, mask=0, scratch=_P, flags=0)
_BACKWARDS = ("egs_backward", "egs_backward_adam", "egs_backward_lossgrad", "egs_backward_object_lossgrad", "egs_backward_entropy_lossgrad")


def _backward(L, lib, entry, **kw):
    a = dict(_BWD_BASE); a.update(kw)
    lg = lib.LossGrad()
    for f in ("image", "gt", "dm_dmu1", "dm_dexx", "dm_dexy", "upstream_grad"):
        setattr(lg, f, _P)
    obj = lib.ObjectLoss(); obj.alpha, obj.obj_mask = _P, _P
    ent = lib.OpacityEntropy(); ent.weight, ent.n_vis, ent.scratch = _P, _P, _P
    ref = lambda given, valid: None if given is None else C.byref(valid if given == "valid" else given)
    grads = [a["g_color"], a["g_depth"], a["g_alpha"]]
    middle = {"egs_backward": grads, "egs_backward_adam": grads, "egs_backward_lossgrad": [ref(a["lg"], lg)],
              "egs_backward_object_lossgrad": [ref(a["lg"], lg), ref(a["obj"], obj)],
              # (the entropy route takes the upstream gradients OR a loss_grad: the base case gives the gradients)
              "egs_backward_entropy_lossgrad": [ref(a["lg"] if a["lg"] != "valid" else None, lg), ref(a["ent"], ent)] + grads}[entry]
    tail = [] if entry == "egs_backward" else [a["sink"], a["prologue"], a["rot"]]
    return getattr(L, entry)(
        a["P"], a["D"], a["M"], a["R"], a["bg"], a["means"], a["shs"], a["rest"], a["colors"], a["scales"], a["mod"], a["rots"], a["cov"], a["act"],
        a["view"], a["proj"], a["campos"], a["W"], a["H"], 1.0, 1.0, a["radii"], a["geom"], a["binning"], a["image"], *middle,
        a["d2"], a["dcol"], a["dop"], a["d3"], a["dcov"], a["dsh"], a["drest"], a["dscales"], a["drots"], a["acc"], a["den"], a["maxr"], a["skip"],
        *tail, a["mask"], a["scratch"], None, a["flags"])


def _sink(lib, coef=_P, **leaves):
    """An egs_adam_sink whose named leaves (means3d, opacity, scales, rotations, sh, sh_rest) own `param`; every other field of them is set."""
    s = lib.AdamSink(); s.coef = coef
    for name, param in leaves.items():
        f = s.leaf[getattr(lib, "SINK_" + name.upper())]
        f.param, f.exp_avg, f.exp_avg_sq, f.lr, f.step = param, _P, _P, _P, _P
    return s


def test_backward_return_codes():
    from egogaussian_amd import lib
    L = lib.load()
    ALL, SINKS = _BACKWARDS, _BACKWARDS[1:]                                    # SINKS: the entry points with sink / prologue_done / rot
    om_no_A, om_grad, om_rot = _motion(lib, A12=None), _motion(lib, grad=_P), _motion(lib, M9=_P)
    rot_only = lib.ObjectRotation(); rot_only.M9 = _P
    no_coef, half_leaf = _sink(lib, coef=None, opacity=_P), _sink(lib, opacity=_P)
    half_leaf.leaf[lib.SINK_OPACITY].exp_avg = None
    lg_short = lib.LossGrad(); lg_short.image = _P
    lg_deferred = lib.LossGrad()
    for f in ("image", "gt", "dm_dmu1", "dm_dexx", "dm_dexy", "upstream_grad", "deferred_partial_sums"):
        setattr(lg_deferred, f, _P)
    obj_short = lib.ObjectLoss(); obj_short.alpha = _P
    ent_short = lib.OpacityEntropy(); ent_short.weight, ent_short.n_vis = _P, _P
    split16 = dict(M=16, D=3, rest=_P2, drest=_P)                              # split harmonics the M = 16 kernel can step
    LG, OBJ, ENT = ("egs_backward_lossgrad", "egs_backward_object_lossgrad"), ("egs_backward_object_lossgrad",), ("egs_backward_entropy_lossgrad",)
    table = [
        # bad dims, range
        (ALL, dict(P=-1), -1), (ALL, dict(W=0), -1), (ALL, dict(W=70000), -3), (ALL, dict(W=8192, H=8192), -3),
        (ALL, dict(R=2**31), -3), (ALL, dict(R=-1), -3),
        (ALL, dict(R=2**31, mask=256), -3),                                      # (R before the gradient mask)
        # a scalar colour's gradient is egs_backward_label's: before anything else of the shared path
        (ALL, dict(act=16, colors=_P, shs=None), -2), (ALL, dict(act=16, R=2**31, means=None), -2),
        # the entry points' own checks
        (("egs_backward",), dict(dcol=None), -1), (("egs_backward",), dict(dop=None), -1), (("egs_backward",), dict(d3=None), -1),
        (("egs_backward",), dict(dcol=None, act=16), -1),
        (("egs_backward",), dict(mask=8, colors=_P, shs=None, dcol=None), -1),
        (LG, dict(lg=None), -1), (LG, dict(lg=None, act=16), -1), (OBJ, dict(obj=None), -1),            # obj_loss without loss_grad: ARG
        (ENT, dict(ent=None), -1), (ENT, dict(ent=None, act=16), -1),
        (ENT, dict(lg=lg_deferred), -2),                                         # a loss_grad AND upstream gradients
        (ENT, dict(lg=lg_deferred, act=16, g_color=None), -2),
        # the entropy term: its words, no object loss, no object motion
        (ENT, dict(ent=ent_short), -1), (ENT, dict(act=8, rot=lib.rot_pointer(om_no_A)), -2),
        # object rotation / motion
        (SINKS, dict(act=8), -2), (("egs_backward",), dict(act=8), -2),
        (SINKS[:3], dict(act=8, rot=lib.rot_pointer(om_no_A)), -1), (SINKS[:3], dict(act=8, rot=lib.rot_pointer(om_grad)), -1),
        (SINKS[:3], dict(act=8, rot=lib.rot_pointer(om_rot)), -2), (SINKS, dict(rot=C.byref(rot_only)), -2),
        (SINKS[:3], dict(act=8, rot=lib.rot_pointer(om_no_A), R=2**31), -1),     # (before the range of R)
        # the loss gradient formed in the blend
        (LG, dict(lg=lg_short), -1), (LG, dict(mask=8, colors=_P, shs=None), -2),
        (OBJ, dict(obj=obj_short), -1), (OBJ, dict(lg=lg_deferred), -1),         # deferred value without the alpha partial sums
        (LG, dict(lg=lg_short, R=2**31), -1),
        # the gradient mask
        (ALL, dict(mask=256), -1), (ALL, dict(mask=-1), -1),
        # missing pointers
        (ALL, dict(bg=None), -1), (ALL, dict(means=None), -1), (ALL, dict(view=None), -1), (ALL, dict(proj=None), -1), (ALL, dict(campos=None), -1),
        (ALL, dict(radii=None), -1), (ALL, dict(geom=None), -1), (ALL, dict(image=None), -1), (ALL, dict(d2=None), -1), (ALL, dict(scratch=None), -1),
        (("egs_backward", "egs_backward_adam") + ENT, dict(g_color=None), -1),
        (ALL, dict(means=None, colors=_P), -1),                                  # (before the modes)
        # misaligned buffers; the scratch needs 16 bytes
        (ALL, dict(geom=_Q), -1), (ALL, dict(binning=_Q), -1), (ALL, dict(image=_Q), -1), (ALL, dict(scratch=_Q), -1),
        # the colours-only route (egs_backward, egs_backward_adam): its own pointer and mode checks
        (("egs_backward_adam",), dict(mask=8, colors=_P, shs=None, dcol=None), -1),
        (("egs_backward", "egs_backward_adam"), dict(mask=8, colors=_P, shs=None, binning=None), -1),
        (("egs_backward", "egs_backward_adam"), dict(mask=8, colors=_P), -2), (("egs_backward", "egs_backward_adam"), dict(mask=8, colors=_P, shs=None, cov=None), -2),
        (ENT, dict(mask=8, colors=_P, shs=None), -2),                            # no opacity gradient on that route
        # the sink
        (SINKS, dict(sink=C.byref(no_coef)), -1), (SINKS, dict(sink=C.byref(half_leaf)), -1),
        (SINKS, dict(sink=C.byref(_sink(lib, scales=_P))), -2),                  # a covariance leaf with cov3D_precomp
        (SINKS, dict(sink=C.byref(_sink(lib, sh=_P)), shs=None, colors=_P), -2),
        (SINKS, dict(sink=C.byref(_sink(lib, sh=_P)), M=4, D=1), -2),           # split-array step only
        (SINKS, dict(sink=C.byref(_sink(lib, sh_rest=_P)), **split16), -2),      # the leaf's param is not shs_rest
        (SINKS, dict(sink=C.byref(_sink(lib, sh_rest=_P2)), M=4, D=1, rest=_P2, drest=_P), -2),
        (SINKS, dict(sink=C.byref(_sink(lib, means3d=_P)), d3=None, **split16), -2),
        (SINKS, dict(sink=C.byref(_sink(lib, sh=_P, sh_rest=_P2)), **dict(split16, drest=None)), -1),      # dL_dsh and dL_dsh_rest: both or neither
        (SINKS, dict(sink=C.byref(_sink(lib, means3d=_P2))), -1),                # a leaf whose param differs from the scene's pointer
        (SINKS, dict(sink=C.byref(_sink(lib, sh=_P2))), -1),
        (SINKS, dict(sink=C.byref(_sink(lib, scales=_P2)), cov=None, scales=_P, rots=_P, dscales=_P, drots=_P), -1),
        (SINKS, dict(sink=C.byref(_sink(lib, rotations=_P2)), cov=None, scales=_P, rots=_P, dscales=_P, drots=_P), -1),
        (SINKS, dict(sink=C.byref(_sink(lib, means3d=_P2)), colors=_P), -1),     # (before the modes)
        # gradient outputs
        (SINKS, dict(dop=None), -1), (SINKS, dict(d3=None), -1), (ALL, dict(colors=_P, shs=None, dcol=None), -1),
        (ALL, dict(dcol=None, **split16), -1), (ALL, dict(binning=None), -1),
        # check_modes
        (ALL, dict(colors=_P), -2), (ALL, dict(shs=None), -2), (ALL, dict(scales=_P), -2), (ALL, dict(cov=None), -2), (ALL, dict(act=1), -2),
        (ALL, dict(act=32), -2), (ALL, dict(scales=_P, rots=_P), -2),
        (ALL, dict(colors=_P, den=_P), -2),                                      # (before the statistics)
        (ALL, dict(binning=None, colors=_P), -1),                                # (after the binning buffer)
        # SH gradients; shs_rest without a second coefficient
        (ALL, dict(dsh=None), -1), (ALL, dict(rest=_P2), -2), (ALL, dict(rest=_P2, dsh=None), -1), (ALL, dict(drest=_P), -1),
        (ALL, dict(split16, drest=None), -1), (ALL, dict(rest=_P2, den=_P), -2),
        # densification statistics
        (ALL, dict(den=_P), -1), (ALL, dict(acc=_P), -1), (ALL, dict(maxr=_P), -1),
        # covariance gradients
        (ALL, dict(dcov=None), -1), (ALL, dict(cov=None, scales=_P, rots=_P), -1), (ALL, dict(cov=None, scales=_P, rots=_P, dscales=_P), -1),
    ]
    for entries, kw, want in table:
        for entry in entries:
            assert _backward(L, lib, entry, **kw) == want, (entry, kw, want)
    # P == 0 with NULL everywhere, where nothing is launched: egs_backward's own pre-check, and the plain path of egs_backward_adam
    nothing = {k: None for k in _BWD_BASE if _BWD_BASE[k] == _P}
    assert _backward(L, lib, "egs_backward", P=0, **nothing) == 0
    assert _backward(L, lib, "egs_backward", P=0, W=0, **nothing) == 0          # (its pre-check comes before the dims)
    assert _backward(L, lib, "egs_backward_adam", P=0, **nothing) == 0
    assert _backward(L, lib, "egs_backward_adam", P=0, W=70000, **nothing) == -3
    assert _backward(L, lib, "egs_backward_adam", P=0, act=16, **nothing) == -2
    assert _backward(L, lib, "egs_backward_adam", P=0, act=8, **nothing) == -2


def test_python_surface_validation_and_no_cpu_fallback():
    import diff_gaussian_rasterization as dgr
    from egogaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    assert dgr.GaussianRasterizer is GaussianRasterizer and hasattr(dgr._C, "rasterize_gaussians") \
        and hasattr(dgr._C, "rasterize_gaussians_backward") and hasattr(dgr._C, "mark_visible")
    rs = GaussianRasterizationSettings(image_height=32, image_width=32, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False)
    r = GaussianRasterizer(raster_settings=rs)
    assert GaussianRasterizer(rs).raster_settings is rs                       # positional ctor (render_helper.py:61)
    x, o = torch.zeros(4, 3), torch.ones(4, 1)
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=x, means2D=x, opacities=o, shs=None, colors_precomp=None, cov3D_precomp=torch.zeros(4, 6))
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=x, means2D=x, opacities=o, shs=torch.zeros(4, 1, 3), colors_precomp=torch.zeros(4, 3), cov3D_precomp=torch.zeros(4, 6))
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=x, means2D=x, opacities=o, shs=torch.zeros(4, 1, 3), scales=torch.ones(4, 3))
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=x, means2D=x, opacities=o, shs=torch.zeros(4, 1, 3), scales=torch.ones(4, 3), rotations=torch.ones(4, 4),
          cov3D_precomp=torch.zeros(4, 6))
    # CPU tensors: loud failure, never a silent fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(means3D=x, means2D=x, opacities=o, shs=torch.zeros(4, 1, 3), cov3D_precomp=torch.zeros(4, 6))


def test_library_is_built_from_the_present_sources():
    """Guards against benchmarking a stale build: the hash of the sources `make` embedded into the library (egs_source_hash) is the
    hash of the sources in the tree -- wherever the tree is (the sources travel with the library), whatever the file dates say."""
    from egogaussian_amd import lib
    assert lib.built_source_hash() == lib.kernel_source_hash(), \
        "libegs_raster.so is stale: run EGS_CLEAN=1 python -c 'import __graft_entry__ as g; g.build()'"


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "egogaussian_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f"{f} imports the oracle"
                assert "liboracle" not in text
    assert not re.search(r"^\s*(from|import)\s+oracle\b", open(os.path.join(ROOT, "diff_gaussian_rasterization", "__init__.py")).read(), flags=re.M)
