"""The backward's scratch as the host sizes it: one 64-byte accumulator line per Gaussian (csrc/egs_common.h EGS_GRAD_STRIDE 16), the hot replica
lines behind them; the deterministic mode's integer lines keep twelve words per Gaussian (EGS_DET_STRIDE; tests/test_det_accum_cpu.py pins them)."""
import pytest

SIZES = (0, 1, 255, 3000, 500000)


@pytest.mark.parametrize("P", SIZES)
def test_scratch_holds_a_64_byte_line_per_gaussian(P):
    from egogaussian_amd import lib
    L = lib.load()
    base = L.egs_backward_scratch_bytes(P)
    assert base >= 64 * P
    assert base % 256 == 0
    # behind the float lines: 8 replicas x ceil(P / 256) x 7 hot lines of 64 bytes
    assert base >= 64 * P + 8 * ((P + 255) // 256) * 7 * 64


@pytest.mark.parametrize("P", SIZES)
def test_deterministic_extra_is_twelve_words_per_gaussian(P):
    from egogaussian_amd import lib
    L = lib.load()
    det = L.egs_backward_scratch_bytes_ex(P, lib.CALL_DETERMINISTIC)
    assert det - L.egs_backward_scratch_bytes(P) == (P * 12 * 12 + 255) // 256 * 256      # (uint32 maximum + int64 sum) x 12, as tests/test_det_accum_cpu.py
    assert det % 256 == 0
