"""CPU: the arithmetic of the deterministic backward blend (EGS_CALL_DETERMINISTIC, egogaussian_amd/csrc/det_accum.h) -- the very header the
kernels include, compiled by the host compiler into a small program (tests/det_accum_host.cpp): order independence, the derived error
bound, the edge cases, and the additions to the C ABI."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = 38                                                            # quantum = 2^(e - 38), e = exponent of the pair's largest |partial|
FLT_MAX_BITS, INF_BITS, NAN_BITS = 0x7f7fffff, 0x7f800000, 0x7fc00000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("det_accum") / "det_accum_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "det_accum_host.cpp"), "-o", exe])
    return exe


def _run(host, *args):
    out = subprocess.run([host] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    return [tuple(int(t) for t in line.split()) for line in out.strip().splitlines()]


def _sums(host, tmp_path, arrays):
    """[(max_bits, int64 sum, decoded float32)] of equally long float32 arrays, each summed in its own order."""
    a = np.ascontiguousarray(np.stack(arrays).astype(np.float32))
    path = str(tmp_path / "partials.bin")
    a.tofile(path)
    rows = _run(host, "sum", path, a.shape[1], a.shape[0])
    return [(mb, s, np.array([fb], dtype=np.uint32).view(np.float32)[0]) for mb, s, fb in rows]


def _quantum(max_abs):
    e = max(math.frexp(float(max_abs))[1] - 1, -126)                  # 2^e <= max < 2^(e+1); a denormal maximum scales like the smallest normal binade
    return math.ldexp(1.0, e - SHIFT)


def _bound(values, decoded):
    """N q / 2 (every partial rounded once to the pair's quantum) + half an ulp of the result (the one conversion to float32)."""
    q = _quantum(np.abs(values).max())
    return len(values) * q / 2 + 0.5 * float(np.spacing(np.float32(abs(decoded))))


def _partials(seed, n=10_000):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-20.0, 10.0, n)).astype(np.float32)      # 30 decades, mixed signs


def test_permutation_invariance_and_error_bound(host, tmp_path):
    for seed in range(3):
        x = _partials(seed)
        rng = np.random.default_rng(100 + seed)
        rows = _sums(host, tmp_path, [x] + [rng.permutation(x) for _ in range(20)])
        assert len({(mb, s) for mb, s, _ in rows}) == 1 and len({f.tobytes() for _, _, f in rows}) == 1, "the sum depends on the order"
        mb, s, dec = rows[0]
        assert mb == int(np.abs(x).max().view(np.uint32))
        exact = math.fsum(float(v) for v in x)
        err, bound = abs(float(dec) - exact), _bound(x, dec)
        print(f"seed {seed}: decoded {float(dec)!r}, float64 sum {exact!r}, |error| {err:.3e} <= bound {bound:.3e}")
        assert err <= bound
        # for scale: float32 addition in two of the orders does depend on them (or the case would show nothing)
    a, b = np.float32(0), np.float32(0)
    for v, w in zip(x, x[::-1]):
        a, b = np.float32(a + v), np.float32(b + w)
    assert a != b


def test_cancelling_partials_near_the_maximum(host, tmp_path):
    """Large partials that cancel to something small: the absolute bound N q / 2 holds where a float32 chain's error is ulp(max) per step."""
    rng = np.random.default_rng(7)
    big = (rng.uniform(1.0, 2.0, 2000) * 1e6).astype(np.float32)
    x = np.concatenate([big, -big, rng.normal(0, 1e-3, 500).astype(np.float32)])
    rows = _sums(host, tmp_path, [rng.permutation(x) for _ in range(5)])
    assert len({(mb, s, f.tobytes()) for mb, s, f in rows}) == 1
    dec = rows[0][2]
    assert abs(float(dec) - math.fsum(float(v) for v in x)) <= _bound(x, dec)


def test_edge_cases(host, tmp_path):
    f32 = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)[0]
    # all zeros, either sign
    (mb, s, dec), = _sums(host, tmp_path, [np.array([0.0, -0.0, 0.0], dtype=np.float32)])
    assert (mb, s) == (0, 0) and dec.tobytes() == np.float32(0.0).tobytes()
    # denormal maximum: float32 denormals are multiples of 2^-149, the quantum 2^-164 divides them -- the sum is exact
    den = np.array([f32(1000), -f32(3), f32(77), f32(0x1fff)], dtype=np.float32)
    (mb, s, dec), = _sums(host, tmp_path, [den])
    assert mb == 0x1fff and dec.tobytes() == f32(1000 - 3 + 77 + 0x1fff).tobytes()
    # maximum at FLT_MAX: nothing overflows on the way, and a sum beyond float32 comes back infinite
    fmax = f32(FLT_MAX_BITS)
    (mb, s, dec), = _sums(host, tmp_path, [np.array([fmax, -fmax, fmax / 2, 1.0], dtype=np.float32)])
    assert mb == FLT_MAX_BITS and dec == np.float32(fmax / 2)
    (mb, s, dec), = _sums(host, tmp_path, [np.array([fmax, fmax], dtype=np.float32)])
    assert np.isposinf(dec)
    # 2^18 partials (more than any pair can receive: 36 864 tiles x 4 quadrant-waves), all equal to the maximum: |sum| < 2^57
    n = 1 << 18
    for bits, want in ((int(np.float32(1.5).view(np.uint32)), np.float32(1.5 * n)), (FLT_MAX_BITS, np.float32(np.inf)),
                       (int(np.float32(-1.9999999).view(np.uint32)), np.float32(np.float32(-1.9999999) * np.float32(n)))):
        (mb, s, fb), = _run(host, "repeat", bits, n)
        one = int(round(float(f32(bits)) / _quantum(abs(float(f32(bits))))))
        assert s == one * n and abs(s) < 1 << 57, "the int64 sum overflowed or an encoded partial is off"
        assert f32(fb).tobytes() == want.tobytes()
    # a non-finite partial: the pair is NaN whatever else it received, in every order, and nothing non-finite is converted to an integer
    for bad in (np.inf, -np.inf, np.nan):
        x = np.array([1.0, bad, -3.5, 2.0 ** 100], dtype=np.float32)
        rows = _sums(host, tmp_path, [x, x[::-1].copy(), x[[1, 0, 3, 2]].copy()])
        assert all(mb >= INF_BITS and s == 0 and np.isnan(dec) for mb, s, dec in rows)
        assert len({dec.tobytes() for _, _, dec in rows}) == 1 and rows[0][2].view(np.uint32) == NAN_BITS


def test_abi_additions(host):
    from egogaussian_amd import lib
    (abi, flag), = _run(host, "abi")
    assert abi == 6 and flag == 0x20 == lib.CALL_DETERMINISTIC
    L = lib.load()
    assert L.egs_abi_version() == 6
    for P in (0, 1, 255, 3000, 500000):
        base = L.egs_backward_scratch_bytes(P)
        assert L.egs_backward_scratch_bytes_ex(P, 0) == base
        assert L.egs_backward_scratch_bytes_ex(P, lib.CALL_SYNC | lib.CALL_KEEP_ALL_INSTANCES | lib.CALL_BALLOT_RANK) == base
        det = L.egs_backward_scratch_bytes_ex(P, lib.CALL_DETERMINISTIC)
        # behind the float accumulator: 12 uint32 maxima and 12 int64 sums per Gaussian, rounded up to 256 bytes
        assert det == base + (P * 12 * 12 + 255) // 256 * 256 and (det > base or P == 0)
    from egogaussian_amd import _C
    assert _C.CALL_DETERMINISTIC == 0x20
    old = _C.deterministic_backward(True)
    try:
        assert old is False and _C.backward_flags() & _C.CALL_DETERMINISTIC and _C.backward_scratch_bytes(3000) == L.egs_backward_scratch_bytes_ex(3000, 0x20)
        assert _C.backward_flags(True) == _C.CALL_SYNC | _C.CALL_DETERMINISTIC
    finally:
        assert _C.deterministic_backward(old) is True
    assert _C.backward_flags() == 0 and _C.backward_scratch_bytes(3000) == L.egs_backward_scratch_bytes(3000)
