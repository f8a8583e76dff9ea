"""GPU: the stand-alone Adam step (adam.hip k_adam, egs_adam1) against Adam in float64 -- the kernel that the step inside the rasterizer
backward, the label phase's finish launch and the captured steps are each asserted bit-identical to.  Single steps from prescribed states
against derived bars, 200-step trajectories against torch.optim.Adam in float32 as the yardstick, and the launch geometry (unaligned
tensors, workgroup edges, more tensors than one launch takes, empty tensors) bit for bit.  Figures: profiles/anchor_parity.md."""
import functools

import numpy as np
import pytest
import torch

from tests import anchors as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fused(capturable):
    from egogaussian_amd.optim import FusedAdam

    def make(params, lr):
        lrs = lr if isinstance(lr, (list, tuple)) else [lr] * len(params)
        return FusedAdam([{"params": [p], "lr": l, "name": f"g{i}"} for i, (p, l) in enumerate(zip(params, lrs))], lr=0.0, betas=A.ADAM_BETAS, eps=A.ADAM_EPS,
                         capturable=capturable)
    return make


def _one_step(capturable, tensors, step, lrs, views=None):
    """One step() of ONE optimizer over `tensors` = [(p, g, m, v) float32 numpy, any shape]: the state goes in through optimizer.state the way
    the densification code does it.  views: per tensor the number of floats its parameter starts into its buffer (a contiguous view).
    -> [(p, m, v) numpy] after the step."""
    params, keep = [], []
    for k, (p, g, m, v) in enumerate(tensors):
        off = 0 if views is None else views[k]
        buf = torch.full((p.size + off + 8,), 7.0, device=DEV)                  # sentinels on both sides of the view
        buf[off:off + p.size] = torch.tensor(p.reshape(-1), device=DEV)
        par = torch.nn.Parameter(buf[off:off + p.size].view(p.shape))
        assert par.data_ptr() % 16 == (4 * off) % 16
        par.grad = torch.tensor(g, device=DEV)
        params.append(par); keep.append(buf)
    opt = _fused(capturable)(params, list(lrs))
    for par, (p, g, m, v) in zip(params, tensors):
        opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(m, device=DEV), "exp_avg_sq": torch.tensor(v, device=DEV)}
    opt.step()
    torch.cuda.synchronize()
    out = []
    for par, buf, (p, g, m, v) in zip(params, keep, tensors):
        off = par.storage_offset()
        assert bool((buf[:off] == 7.0).all()) and bool((buf[off + p.size:] == 7.0).all()), "the step wrote outside its tensor"
        st = opt.state[par]
        if p.size:
            assert int(round(float(st["step"]))) == step
        out.append((par.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()))
    return out


def _case_tensor(case, n=None, p=None):
    n = case["n"] if n is None else n
    return (np.zeros(n, np.float32) if p is None else p[:n], case["g"][:n], case["m"][:n], case["v"][:n])


# ---- single step from a prescribed state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("regime", sorted(A.ADAM_REGIMES))
def test_single_step_against_float64(regime, capturable):
    case = A.adam_case(regime)
    (p, m, v), = _one_step(capturable, [_case_tensor(case)], case["step"], [case["lr"]])
    fig = A.check_adam_step(p, m, v, case, what=f"{regime} capturable={capturable}")
    print(f"ANCHOR adam step {regime} capturable={capturable}: m {fig['m']:.2f}u (bar 4u), v {fig['v']:.2f}u (4u), p {fig['p']:.2f}u (16u)")
    if regime == "ordinary":
        d = A.adam_double_beta_check(v, case)
        print(f"ANCHOR adam exp_avg_sq vs Adam with double betas: {d:.3e} (derived {A.ADAM_DOUBLE_BETA_DISTANCE:.3e})")


@pytest.mark.parametrize("capturable", [False, True])
def test_elements_with_nothing_to_do_are_left_bit_unchanged(capturable):
    case = A.adam_case("ordinary", n=4099)
    z = np.arange(case["n"]) % 3 == 0
    for k in ("g", "m", "v"):
        case[k] = np.where(z, np.float32(0), case[k])
    p0 = np.random.default_rng(3).standard_normal(case["n"]).astype(np.float32)
    (p, m, v), = _one_step(capturable, [_case_tensor(case, p=p0)], case["step"], [case["lr"]])
    assert A.same_bits(p[z], p0[z]) and A.same_bits(m[z], np.zeros(int(z.sum()))) and A.same_bits(v[z], np.zeros(int(z.sum())))
    assert not np.array_equal(p[~z & (case["g"] != 0)], p0[~z & (case["g"] != 0)])


# ---- trajectories -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trajectory(regime):
    inp = A.adam_trajectory_inputs(regime)
    ref = A.adam_trajectory64(inp)
    return inp, ref, A.adam_trajectory_stats(A.adam_trajectory_optimizer(inp, A.torch_adam32), ref, inp["sigma_g"])


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("regime", sorted(A.ADAM_REGIMES))
def test_trajectory_is_as_close_to_float64_as_torch_adam_in_float32(regime, capturable):
    inp, ref, yard = _trajectory(regime)
    sub = A.adam_trajectory_stats(A.adam_trajectory_optimizer(inp, _fused(capturable), device=DEV), ref, inp["sigma_g"])
    print(f"ANCHOR adam trajectory {regime} capturable={capturable} (torch float32 on the CPU): " + A.check_adam_trajectory(sub, yard, what=f"{regime} capturable={capturable}"))


# ---- geometry, bit for bit --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(step):
    """The aligned one-tensor, non-capturable step over 8 193 elements that the geometry cases are compared with; itself held to float64."""
    case = A.adam_case("late" if step == 30000 else "ordinary", n=8193, seed=11) | {"step": step}
    p0 = np.zeros(8193, np.float32)
    base, = _one_step(False, [_case_tensor(case)], step, [case["lr"]])
    A.check_adam_step(*base, case, what=f"base step {step}")
    return case, p0, base


def _same(a, b, what):
    for x, y, name in zip(a, b, ("p", "exp_avg", "exp_avg_sq")):
        assert A.same_bits(x, y), f"{what}: {name} differs in {int((A._bits(x) != A._bits(y)).sum())} of {x.size} elements"


@pytest.mark.parametrize("step", [1, 2, 1000, 30000])
def test_capturable_and_plain_variant_take_the_same_step(step):
    case, p0, base = _base(step)
    got, = _one_step(True, [_case_tensor(case, p=p0)], step, [case["lr"]])
    _same(got, base, f"capturable vs plain at step {step}")


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 8193])
def test_element_counts_around_the_vector_and_workgroup_edges(n, capturable):
    case, p0, base = _base(7)
    got, = _one_step(capturable, [_case_tensor(case, n=n, p=p0)], 7, [case["lr"]])
    _same(got, tuple(a[:n] for a in base), f"{n} elements")


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("offset_bytes", [4, 8, 12])
def test_unaligned_parameter_view_equals_the_aligned_tensor(offset_bytes, capturable):
    """A parameter that starts 4, 8 or 12 bytes into its buffer takes the kernel's scalar branch."""
    case, p0, base = _base(7)
    for n in (4099, 5):
        got, = _one_step(capturable, [_case_tensor(case, n=n, p=p0)], 7, [case["lr"]], views=[offset_bytes // 4])
        _same(got, tuple(a[:n] for a in base), f"view {offset_bytes} bytes into its buffer, {n} elements")


TENSOR_SIZES = (1, 37, 4096, 260, 4097, 3, 1025, 12, 8193, 5, 300, 64, 4095, 7, 129, 2000, 33)       # tensor k holds TENSOR_SIZES[k % 17] elements


@functools.lru_cache(maxsize=None)
def _many(count):
    """`count` tensors with their own learning rates and what a one-tensor optimizer does to each."""
    rng = np.random.default_rng(count)
    tensors, lrs = [], []
    for k in range(count):
        n = TENSOR_SIZES[k % len(TENSOR_SIZES)]
        c = A.adam_case("ordinary", n=n, seed=100 + k)
        tensors.append((rng.standard_normal(n).astype(np.float32), c["g"], c["m"], c["v"]))
        lrs.append(float(10.0 ** rng.uniform(-4, -2)))
    alone = [_one_step(False, [t], 7, [lr])[0] for t, lr in zip(tensors, lrs)]
    return tensors, lrs, alone


def _check_many(count, capturable, empty_at=None):
    tensors, lrs, alone = _many(count)
    tensors, lrs, alone = list(tensors), list(lrs), list(alone)
    if empty_at is not None:                                          # features_rest at SH degree 0: [n, 0, 3], with an (empty) gradient
        e = np.zeros((50, 0, 3), np.float32)
        tensors.insert(empty_at, (e, e, e, e)); lrs.insert(empty_at, 2.5e-3); alone.insert(empty_at, (e, e, e))
    got = _one_step(capturable, tensors, 7, lrs)
    bad = [k for k in range(len(tensors)) if not all(A.same_bits(x, y) for x, y in zip(got[k], alone[k]))]
    assert not bad, f"{len(tensors)} tensors in one optimizer (empty tensor at {empty_at}): tensors {bad} differ from what a one-tensor optimizer does to them"


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("count", [16, 17, 33])
def test_more_tensors_than_one_launch_takes(count, capturable):
    _check_many(count, capturable)


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("empty_at", [0, 5, 15])
@pytest.mark.parametrize("count", [18, 34])
def test_an_empty_tensor_does_not_shift_the_next_launch(count, empty_at, capturable):
    """An empty tensor takes no slot of a launch; the chunk after it must start where the launch stopped, not 16 indices on (tensor 16 used
    to be stepped twice)."""
    _check_many(count - 1, capturable, empty_at=empty_at)
