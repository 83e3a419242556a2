"""Host side of the ensemble CRPS loss (anemoi_core_amd/losses, ops.kernel_crps): the constructor's validation, the refusals by name, and -
with no GPU - the identities the kernel's formula rests on: sum_m x_m s_m = sum_{i<j} |x_i - x_j| with ties, and stable == naive."""
import pytest
import torch

from anemoi_core_amd import ops
from anemoi_core_amd.losses import CRPS


@pytest.mark.parametrize("kwargs, match", [(dict(alpha=-0.1), "alpha must be in the range"), (dict(alpha=1.5), "alpha must be in the range"),
                                           (dict(backend="fast"), "Unknown CRPS backend 'fast'")])
def test_constructor_refuses(kwargs, match):
    with pytest.raises(ValueError, match=match):
        CRPS(**kwargs)


def test_constructor_and_name():
    loss = CRPS(alpha=0.5, backend="naive", no_autocast=False, ignore_nans=True, some_factory_argument=1)
    assert (loss.alpha, loss.backend, loss.no_autocast, loss.ignore_nans) == (0.5, "naive", False, True)
    assert loss.name == "crps0.50" and CRPS().name == "crps0.95"


@pytest.mark.parametrize("dimension, scaler, match", [(0, torch.ones(2), "dimension 0"), (2, torch.ones(2), "dimension 2"),
                                                      ((3, 4), torch.ones(2, 2), "several dimensions"), (3, torch.ones(2, 2), "multi-dimensional")])
def test_scalers_not_built_are_refused_by_name(dimension, scaler, match):
    with pytest.raises(NotImplementedError, match=match):
        CRPS().add_scaler(dimension, scaler)


@pytest.mark.parametrize("kwarg", ["scaler_indices", "without_scalers", "grid_shard_slice", "group"])
def test_forward_arguments_not_built_are_refused_by_name(kwarg):
    loss = CRPS()
    loss.add_scaler(3, torch.ones(4))
    with pytest.raises(NotImplementedError, match=kwarg):
        loss(torch.zeros(1, 1, 2, 4, 1), torch.zeros(1, 1, 1, 4, 1), **{kwarg: (slice(None),)})


def test_scalers_multiply_and_grid_is_required():
    loss = CRPS()
    with pytest.raises(RuntimeError, match="GRID"):
        loss(torch.zeros(1, 1, 2, 4, 1), torch.zeros(1, 1, 1, 4, 1))
    loss.add_scaler(3, torch.full((4,), 2.0), name="area")
    loss.add_scaler(-2, torch.full((4,), 3.0))
    assert torch.equal(loss.w3, torch.full((4,), 6.0)) and loss.w1 is None and loss.w4 is None
    with pytest.raises(ValueError, match="already exists"):
        loss.add_scaler(4, torch.ones(1), name="area")


@pytest.mark.parametrize("E, error, match", [(1, ValueError, "Ensemble size must be greater than 1"), (17, NotImplementedError, "ensemble size 17"),
                                             (2, RuntimeError, "no CPU fallback")])
def test_ensemble_sizes_and_cpu_tensors_raise(E, error, match):
    with pytest.raises(error, match=match):
        ops.kernel_crps(torch.zeros(1, 1, E, 4, 1), torch.zeros(1, 1, 1, 4, 1), torch.ones(4))


@pytest.mark.parametrize("alpha", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("E", [2, 3, 8, 16])
def test_rank_sum_identity_and_stable_equals_naive(alpha, E):
    torch.manual_seed(E)
    x = torch.randint(-2, 3, (500, E)).double()  # ties in most columns
    y = torch.randint(-2, 3, (500,)).double()
    diff = x[:, :, None] - x[:, None, :]
    pairs = diff.abs().sum((1, 2)) / 2  # sum_{i<j} |x_i - x_j|
    s = torch.sign(diff).sum(2)
    assert torch.equal((x * s).sum(1), pairs)  # every unordered pair once: (x_i - x_j) sign(x_i - x_j)
    assert torch.equal(((x - y[:, None]) * s).sum(1), pairs)  # sum_m s_m = 0: the kernel subtracts the target first
    err = (x - y[:, None]).abs()
    coef = -(alpha / (E * (E - 1)) + (1 - alpha) / E**2)
    naive = err.mean(1) + coef * pairs
    off = ~torch.eye(E, dtype=torch.bool)
    mem = err[:, None, :] * off
    stable = (mem + mem.transpose(1, 2) - (1 - (1 - alpha) / E) * diff.abs()).sum((1, 2)) / (2 * E * (E - 1))
    torch.testing.assert_close(stable, naive, rtol=0, atol=1e-13)
    # the closed-form gradient, with zeros at ties and where a member equals the target, is autograd's
    xg = x.clone().requires_grad_()
    d = xg[:, :, None] - xg[:, None, :]
    ((xg - y[:, None]).abs().mean(1) + coef * d.abs().sum((1, 2)) / 2).sum().backward()
    torch.testing.assert_close(xg.grad, torch.sign(x - y[:, None]) / E + coef * s, rtol=0, atol=1e-15)
