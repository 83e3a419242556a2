"""The training side of the EDM diffusion objective without a GPU, against the imported reference's records
(tests/golden/transport_train.pt): the sigma distributions, the loss weight, ``prepare_edm_training``; the float64 restatements of
tests/transport_train_refs.py pinned to the reference's own float64 gradients; and the refusals that come before any kernel."""
import pytest
import torch

from anemoi_core_amd import ops
from anemoi_core_amd.transport import SIGMA_TRAINING_DISTRIBUTIONS, edm_loss_weight
from tests import transport_train_refs as TR

FX = TR.load_train_fixture()
CASES = sorted(FX["models"])


def _rel(got, want) -> float:
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


# ---------------------------------------------------------------------------------------------- distributions, weight
def test_the_four_distributions_are_registered():
    assert sorted(SIGMA_TRAINING_DISTRIBUTIONS) == ["cosine", "exponential", "karras", "linear"]
    from anemoi_core_amd import transport

    for name in ("karras_sigma_from_unit_time", "exponential_sigma_from_unit_time", "cosine_sigma_from_unit_time", "edm_loss_weight"):
        assert callable(getattr(transport, name)), name


@pytest.mark.parametrize("kind", sorted(SIGMA_TRAINING_DISTRIBUTIONS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_distribution_draws_what_the_reference_draws(kind, dtype, monkeypatch):
    d = FX["distributions"]
    rec = d["draws"][(kind, dtype)]
    dist = SIGMA_TRAINING_DISTRIBUTIONS[kind](**d["kwargs"][kind])
    torch.manual_seed(d["seed"])
    out = dist.sample(d["shape"], device=torch.device("cpu"), dtype=dtype)
    B, E = d["shape"]["a"][0], d["shape"]["a"][2]
    assert sorted(out) == sorted(d["shape"]) and out["a"] is out["b"]  # one tensor object shared by the datasets
    assert out["a"].shape == (B, 1, E, 1, 1) and out["a"].dtype == dtype
    if dtype == torch.float64:
        assert _rel(out["a"], rec["sigma"]) <= 1e-12
    # the same torch.rand draw gives the same values
    monkeypatch.setattr(torch, "rand", lambda shape, device=None, dtype=None: rec["rand"].clone())
    again = dist.sample(d["shape"], device=torch.device("cpu"), dtype=dtype)["a"]
    if dtype == torch.float32:
        assert torch.equal(again, rec["sigma"])
    else:
        assert _rel(again, rec["sigma"]) <= 1e-12


def test_distribution_validation_errors_are_the_reference_texts():
    K = SIGMA_TRAINING_DISTRIBUTIONS["karras"]
    with pytest.raises(ValueError, match="sigma_min must be strictly positive"):
        K(sigma_max=1.0, sigma_min=0.0)
    with pytest.raises(ValueError, match="sigma_max must be strictly positive"):
        K(sigma_max=0.0, sigma_min=0.1)
    with pytest.raises(ValueError, match="sigma_max must be greater than or equal to sigma_min"):
        K(sigma_max=0.1, sigma_min=1.0)
    dist = K(sigma_max=100.0, sigma_min=0.02)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="requires at least one dataset shape"):
        dist.sample({}, device=cpu)
    with pytest.raises(ValueError, match=r"Expected 5D tensor shape \(batch, time, ensemble, grid, vars\) for transport conditions"):
        dist.sample({"a": (2, 1, 3, 4)}, device=cpu)
    with pytest.raises(ValueError, match="Expected 5D tensor shape for dataset 'b'"):
        dist.sample({"a": (2, 1, 3, 4, 5), "b": (2, 1, 3)}, device=cpu)
    with pytest.raises(ValueError, match="Batch or ensemble dimension mismatch across datasets when sampling conditions"):
        dist.sample({"a": (2, 1, 3, 4, 5), "b": (2, 1, 2, 4, 5)}, device=cpu)


def test_edm_loss_weight_is_the_closed_form():
    sigma = torch.tensor([0.02, 0.5, 1.0, 7.0, 100.0], dtype=torch.float64)
    for sd in (1.0, 0.5):
        want = 1 / sigma**2 + 1 / sd**2  # (sigma^2 + sd^2) / (sigma sd)^2
        assert _rel(edm_loss_weight(sigma, sd), want) <= 1e-14
    assert edm_loss_weight(sigma.float(), 1.0).dtype == torch.float32


# ---------------------------------------------------------------------------------------------- prepare_edm_training
@pytest.mark.parametrize("name", CASES)
def test_prepare_reproduces_the_reference_from_its_draws(name, monkeypatch):
    rec = FX["models"][name]
    model, _, target = TR.training_model(FX, name)
    prep = rec["prepare"]
    monkeypatch.setattr(torch, "rand", lambda shape, device=None, dtype=None: prep["rand"].clone())
    model.transport_source.draw = lambda shape, dtype, device: prep["randn"].clone().to(dtype)
    y_noised, sigma, weights = model.prepare_edm_training({"data": target})
    assert torch.equal(sigma["data"], prep["sigma"]) and sigma["data"].shape == (target.shape[0], 1, 1, 1, 1)
    assert torch.equal(weights["data"], prep["weights"])
    assert torch.equal(y_noised["data"], prep["y_noised"])
    # sigma and source handed over: the step the gradients are recorded at
    y2, s2, w2 = model.prepare_edm_training({"data": target}, source={"data": prep["randn"]}, sigma={"data": rec["sigma"]})
    assert s2["data"] is rec["sigma"] and torch.equal(y2["data"], rec["y_noised"]) and torch.equal(w2["data"], rec["weights"])


def test_prepare_refuses_a_missing_or_unknown_distribution():
    model, _, target = TR.training_model(FX, CASES[0])
    model.training_condition = {}
    with pytest.raises(ValueError, match="EDM training_condition must define 'distribution'."):
        model.prepare_edm_training({"data": target})
    model.training_condition = {"distribution": "lognormal"}
    with pytest.raises(ValueError, match="Unknown EDM training condition distribution: lognormal"):
        model.prepare_edm_training({"data": target})


def test_training_condition_comes_from_the_config():
    from anemoi_core_amd.models.configs import transport_model_config

    cond = {"distribution": "karras", "sigma_max": 100.0, "sigma_min": 0.02, "rho": 7.0}
    assert transport_model_config("gt", 64, 2, 2, 8, training_condition=cond)["model"]["model"]["transport"]["training_condition"] == cond
    assert "training_condition" not in transport_model_config("gt", 64, 2, 2, 8)["model"]["model"]["transport"]


# ---------------------------------------------------------------------------------------------- the restatements, pinned
def _mlp64(model):
    emb = model.noise_embedder
    freq, pi = emb.embedding_operands()
    l1, l2 = model.noise_cond_mlp.linear1_no_gradscaling, model.noise_cond_mlp.linear2_no_gradscaling
    params = [p.detach().double().requires_grad_(True) for p in (l1.weight, l1.bias, l2.weight, l2.bias)]
    return freq.double(), None if pi is None else pi.double(), params


@pytest.mark.parametrize("name", CASES)
def test_restated_noise_conditioning_gives_the_reference_gradients(name):
    """From the reference's float64 gradient of the conditioning vector, spread over the rows of two destinations: the restated edge
    differentiated by torch and the restated backward formula both give the reference's float64 noise_cond_mlp gradients."""
    rec = FX["models"][name]
    model, _, _ = TR.training_model(FX, name)
    freq, pi, params = _mlp64(model)
    values, rows, d_cond = rec["sigma"].reshape(-1).double(), (5, 3), rec["d_cond64"]
    keep = {}
    outs = TR.noise_cond_torch(values, freq, *params, pi=pi, log_quarter=True, rows=rows, keep=keep)
    # row gradients that sum to d_cond per group: unequal shares, so that the sum over rows and destinations matters
    share = [torch.linspace(1.0, 2.0, r, dtype=torch.float64) for r in rows]
    total = sum(float(s.sum()) for s in share)
    d_outs = [(d_cond[:, None, :] * s[None, :, None] / total).reshape(-1, d_cond.shape[1]) for s in share]
    torch.autograd.backward(outs, d_outs)
    assert _rel(keep["cond"].grad, d_cond) <= 1e-12
    want = [rec["grads"][f"noise_cond_mlp.{k}"] for k in ("linear1_no_gradscaling.weight", "linear1_no_gradscaling.bias",
                                                         "linear2_no_gradscaling.weight", "linear2_no_gradscaling.bias")]
    ref, bound = TR.noise_cond_bwd_ref(d_outs, rows, values, freq, pi, *[p.detach() for p in params], log_quarter=True)
    assert _rel(ref["s"], d_cond) <= 1e-12
    for got, key, w in zip([p.grad for p in params], ["d_w1", "d_b1", "d_w2", "d_b2"], want):
        assert _rel(got.float(), w) <= 2.0**-23  # the fixture stores the float64 gradient rounded to fp32
        # the formula forms the argument of sin / cos in fp32, as the kernel does, where the reference's float64 run keeps it in float64:
        # that is the d_e term of its own bound
        assert bool(((got - ref[key].view(got.shape)).abs() <= bound[key].view(got.shape)).all()), key


@pytest.mark.parametrize("name", CASES)
def test_restated_output_edge_gives_the_reference_gradient(name):
    """The loss differentiated through the restated output edge at the reference's float64 network output: the reference's gradient with
    respect to that output, to 1e-10; the restated backward formula gives the same."""
    rec = FX["models"][name]
    _, _, target = TR.training_model(FX, name)
    pred = rec["pred64"].clone().requires_grad_(True)
    y, sigma, w = rec["y_noised"].double(), rec["sigma"].double(), rec["weights"].double()
    D = TR.edm_output_torch(pred, y, sigma.reshape(-1), tuple(y.shape), sigma_data=1.0, out_dtype=torch.float64)
    assert _rel(D.detach(), rec["out64"]) <= 1e-12
    loss = (w * (D - target.double()) ** 2).mean()
    assert abs(float(loss.detach()) - float(rec["loss64"])) <= 1e-12 * abs(float(rec["loss64"]))
    (d_out,) = torch.autograd.grad(loss, D, retain_graph=True)
    loss.backward()
    assert _rel(pred.grad[::rec["row_step"]], rec["d_pred64"]) <= 1e-10
    formula, _ = TR.edm_output_bwd_ref(d_out, sigma.reshape(-1), 1.0, pred.shape[1], torch.float64)
    assert _rel(formula, pred.grad) <= 1e-10  # (edm_coefficients reads sigma as fp32, as the kernel does: sigma is fp32 in the fixture)


def test_restated_input_edge_gradient_is_the_sum_over_groups():
    gen = torch.Generator().manual_seed(5)
    B, E, N, A = 2, 3, 7, 4
    x, y = torch.randn(B, 2, E, N, 3, generator=gen, dtype=torch.float64), torch.randn(B, 1, E, N, 2, generator=gen, dtype=torch.float64)
    attrs = torch.randn(N, A, generator=gen, dtype=torch.float64, requires_grad=True)
    sigma = torch.rand(B * E, generator=gen, dtype=torch.float64) + 0.1
    rows = TR.assemble_input_torch(x, y, attrs, 16, sigma=sigma, sigma_data=1.0)
    assert rows.shape == (B * E * N, 16) and torch.equal(rows[:, 12:], torch.zeros(B * E * N, 4, dtype=torch.float64))
    d_rows = torch.randn(rows.shape, generator=gen, dtype=torch.float64)
    rows.backward(d_rows)
    formula, _ = TR.assemble_input_bwd_ref(d_rows, 8, N, A)
    assert _rel(attrs.grad, formula) <= 1e-14


# ---------------------------------------------------------------------------------------------- refusals before any kernel
def test_cpu_tensors_under_grad_are_still_refused_first():
    w1, b1 = torch.randn(4, 4, requires_grad=True), torch.randn(4, requires_grad=True)
    w2, b2 = torch.randn(3, 4, requires_grad=True), torch.randn(3, requires_grad=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.noise_cond(torch.ones(2), torch.ones(2), w1, b1, w2, b2)
    x, y = torch.randn(1, 1, 1, 5, 2), torch.randn(1, 1, 1, 5, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.transport_assemble_input(x, y, torch.randn(5, 3, requires_grad=True), 7, sigma=torch.ones(1))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.edm_output(torch.randn(5, 2, requires_grad=True), y, torch.ones(1), (1, 1, 1, 5, 2))
