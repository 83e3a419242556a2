"""Training the EDM diffusion model on the MI355X against the imported reference's float64 gradients (tests/golden/transport_train.pt):
one training step - forward under autograd through the three edge kernels and the network, the weighted loss, backward through
csrc/transport_bwd.hip - in fp32 and with a bf16 network; an optimiser step; the step captured as one graph; and the inference forward
left as it was."""
import pytest
import torch

from anemoi_core_amd import ops
from tests import transport_refs as R
from tests import transport_train_refs as TR
from tests.test_training_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = TR.load_train_fixture()
CASES = sorted(FX["models"])
_built = {}


def _case(name: str, dtype=torch.float32):
    """(model on the device, x, y_noised, sigma, weights, target): built once per (case, dtype); tests leave the parameters as they are."""
    key = (name, dtype)
    if key not in _built:
        rec = FX["models"][name]
        model, x, target = TR.training_model(FX, name)
        if dtype != torch.float32:
            model.cast_network(dtype)
        _built[key] = (model.to(DEV), x.to(DEV), rec["y_noised"].to(DEV), rec["sigma"].to(DEV), rec["weights"].to(DEV), target.to(DEV))
    return _built[key]


def _step(model, x, y_noised, sigma, weights, target):
    model.zero_grad(set_to_none=True)
    loss = TR.training_loss(model, x, y_noised, sigma, weights, target)
    loss.backward()
    return loss.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _err(got, want) -> float:
    return float((got.double().cpu() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize("name", CASES)
def test_fp32_gradients_match_the_reference(name):
    """Loss and every recorded parameter gradient against the reference's float64 run under the project's fp32 training tolerance (_close of
    tests/test_training_gpu.py); every parameter has a gradient.  Measured on the MI355X (error / the reference's own fp32 error, over the
    tensors whose gradient is above 1e-6 of the largest): see DESIGN section 16a."""
    rec = FX["models"][name]
    loss, grads = _step(*_case(name))
    print(f"{name}: loss {float(loss):.9f} reference float64 {float(rec['loss64']):.9f} fp32 {float(rec['loss32']):.9f}")
    _close(loss.reshape(1), rec["loss64"].reshape(1), f"{name} loss")
    assert sorted(grads) == sorted(list(rec["err32"]) + rec["zero_grads"])
    for k in rec["zero_grads"]:  # identically zero in the reference: zero or absent here
        assert grads[k] is None or not bool(grads[k].any()), k
    ratios = []
    for k in rec["err32"]:
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        if k in rec["grads"]:
            err = _err(grads[k], rec["grads"][k])
            ratios.append(err / rec["err32"][k])
            print(f"  {k}: err {err:.3e} reference fp32 {rec['err32'][k]:.3e} ratio {ratios[-1]:.2f} max|g| {float(rec['grads'][k].abs().max()):.3e}")
            _close(grads[k], rec["grads"][k], f"{name} {k}")
    assert len(ratios) == len(rec["grad_keys"]) and (name != "sin_b2" or len(ratios) == len(grads))  # sin_b2: no parameter is skipped
    print(f"{name}: {len(ratios)} tensors, error / reference fp32 error in [{min(ratios):.2f}, {max(ratios):.2f}]")


@pytest.mark.parametrize("name", CASES)
def test_bf16_network_gradients_stay_within_twice_the_restated_route(name):
    """bf16 network, fp32 data.  Yardstick: the same bf16 network with the three edges as torch operations (tests/transport_train_refs.py:
    restated_edges), against the same float64 gradients.  The kernel route differs from it only in the rounding order of the three edges:
    its error per tensor is at most twice the yardstick's."""
    rec = FX["models"][name]
    args = _case(name, torch.bfloat16)
    loss, grads = _step(*args)
    with TR.restated_edges():
        loss_y, grads_y = _step(*args)
    print(f"{name} bf16: loss {float(loss):.6f} restated {float(loss_y):.6f} reference {float(rec['loss64']):.6f}")
    assert abs(float(loss) - float(rec["loss64"])) <= 2 * abs(float(loss_y) - float(rec["loss64"])) + 2.0**-8 * abs(float(rec["loss64"]))
    worst = []
    for k in rec["grad_keys"]:
        assert grads[k] is not None and grads[k].dtype == dict(args[0].named_parameters())[k].dtype, k
        e, ey = _err(grads[k], rec["grads"][k]), _err(grads_y[k], rec["grads"][k])
        print(f"  {k}: kernel route {e:.3e} restated route {ey:.3e} ratio {e / ey:.2f}")
        if e > 2 * ey:
            worst.append((k, e, ey))
    assert not worst, worst


def test_optimiser_step_lowers_the_loss_and_the_caches_follow():
    """One SGD step, then a second forward: the loss decreases, and the fused / projected weight caches of the blocks pick up the updated
    parameters - a forward under no_grad equals, bit for bit, that of a freshly built model loaded with the same state_dict."""
    name = "sin_b2"
    model, x, target = TR.training_model(FX, name)
    rec = FX["models"][name]
    model = model.to(DEV)
    x, y_noised, sigma, weights, target = x.to(DEV), rec["y_noised"].to(DEV), rec["sigma"].to(DEV), rec["weights"].to(DEV), target.to(DEV)
    with torch.no_grad():
        model({"data": x}, {"data": y_noised}, {"data": sigma})  # the caches exist before the step
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    loss0, _ = _step(model, x, y_noised, sigma, weights, target)
    opt.step()
    with torch.no_grad():
        out = model({"data": x}, {"data": y_noised}, {"data": sigma})["data"]
        loss1 = (weights * (out - target) ** 2).mean()
    print(f"loss {float(loss0):.6f} -> {float(loss1):.6f}")
    assert float(loss1) < float(loss0)
    fresh, _, _ = TR.training_model(FX, name)
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=True)
    fresh = fresh.to(DEV)
    with torch.no_grad():
        assert torch.equal(fresh({"data": x}, {"data": y_noised}, {"data": sigma})["data"], out)


def test_training_step_captured_as_one_graph_equals_eager():
    """Forward + loss + backward captured into one graph (modelled on test_training_step_captured_as_one_hip_graph_equals_eager): sigma and
    the noised target are read from device memory, so two replays on new values are bit-equal to eager steps in the loss and every gradient."""
    name = "sin_b2"
    model, x, target = TR.training_model(FX, name)
    rec = FX["models"][name]
    model = model.to(DEV)
    x, target = x.to(DEV), target.to(DEV)
    y_static, s_static, w_static = rec["y_noised"].to(DEV).clone(), rec["sigma"].to(DEV).clone(), rec["weights"].to(DEV).clone()
    box = {}

    def step():
        model.zero_grad(set_to_none=True)
        box["loss"] = TR.training_loss(model, x, y_static, s_static, w_static, target)
        box["loss"].backward()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # static caches are built outside the capture
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    captured_loss = box["loss"]
    assert len(captured) == len(rec["err32"])
    source = rec["prepare"]["randn"].to(DEV)
    first = None
    for sigmas in ([2.5, 0.07], [0.3, 40.0]):
        sig = torch.tensor(sigmas, device=DEV).view(2, 1, 1, 1, 1)
        y_new, _, w_new = model.prepare_edm_training({"data": target}, source={"data": source}, sigma={"data": sig})
        s_static.copy_(sig), y_static.copy_(y_new["data"]), w_static.copy_(w_new["data"])
        graph.replay()
        torch.cuda.synchronize()
        got, got_loss = {k: g.clone() for k, g in captured.items()}, captured_loss.clone()
        step()  # eager, same values
        torch.cuda.synchronize()
        assert torch.equal(got_loss, box["loss"])
        for k, p in model.named_parameters():
            if p.grad is not None:
                assert torch.equal(got[k], p.grad), k
        if first is None:
            first = got
    assert any(not torch.equal(first[k], got[k]) for k in got)  # the replay really depends on sigma and the noised target


def test_inference_forward_is_untouched(monkeypatch):
    """After a training step on the same model, a no_grad forward of a transport.pt case equals the one before it bit for bit and matches the
    fixture, and the three forward entry points are launched once each, no backward entry among them."""
    fx = R.load_fixture()
    model, x, y, sigma, _ = R.transport_model(fx, "sin_b2")
    model, x, y, sigma = model.to(DEV), x.to(DEV), y.to(DEV), sigma.to(DEV)
    with torch.no_grad():
        before = model({"data": x}, {"data": y}, {"data": sigma})["data"].clone()
    target = torch.zeros_like(y)
    _step(model, x, y, sigma, torch.ones_like(sigma), target)
    model.zero_grad(set_to_none=True)
    seen = []
    lib = ops._lib.load()
    names = ("anemoi_noise_cond_fwd", "anemoi_transport_assemble_input", "anemoi_edm_output", "anemoi_noise_cond_bwd",
             "anemoi_transport_assemble_input_bwd", "anemoi_edm_output_bwd")
    for n in names:
        real = getattr(lib, n)
        monkeypatch.setattr(lib, n, lambda *a, _r=real, _n=n: (seen.append(_n), _r(*a))[1])
    with torch.no_grad():
        after = model({"data": x}, {"data": y}, {"data": sigma})["data"]
    assert sorted(seen) == sorted(names[:3]), seen
    assert torch.equal(before, after)
    assert R.rel_err(after.cpu(), fx["models"]["sin_b2"]["out64"]) <= 8 * fx["models"]["sin_b2"]["err32"]
    seen.clear()
    _step(model, x, y, sigma, torch.ones_like(sigma), target)  # a training step: each forward and each backward entry exactly once
    assert sorted(seen) == sorted(names), seen
