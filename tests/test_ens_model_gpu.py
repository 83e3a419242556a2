"""AnemoiEnsModelEncProcDec and its ConditionalLayerNorm routes on the MI355X.

* Every case of tests/golden/ens.pt that the reference can run, with the noise the reference drew substituted through
  ``NoiseConditioning.draw``, in fp32 and bf16 against the reference's fp32 output, with the bounds of the model-fixture test of
  tests/test_transformer_gpu.py (``_check``: fp32 max err / scale <= 5e-5; bf16 max <= 2e-2, mean <= 5e-3 of scale).
  ``gt_cond_residual`` has no reference output (the reference's forward raises, see tests/golden/make_golden_ens.py): it is run for its
  shape, finiteness and its dependence on the residual columns only.
* ConditionalLayerNorm: the fused route (``ops.cond_layer_norm_proj``) against the two-step route (GEMM + ``ops.cond_layer_norm``).
* The default draw: two forwards differ; a captured forward with fixed noise replays bit-equal; 2 ranks on one GPU match one.
"""
import pytest
import torch

from tests import ens_helpers as E
from tests.test_fullsize_parity_gpu import _check
from tests.test_kernels_gpu import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = E.load_fixture()
RUNNABLE = sorted(k for k, v in FX.items() if isinstance(v, dict) and "out" in v)


def _forward(name, dtype, fused=True, monkeypatch=None):
    model, x, _ = E.ens_model(FX, name)
    if "noise" in FX[name]:
        E.fix_noise(model, FX[name]["noise"])
    model = model.to(DEV, dtype)
    with torch.no_grad():
        return model({"data": x.to(DEV, dtype)}, fcstep=FX[name]["fcstep"])["data"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", RUNNABLE)
def test_fixture_case_against_the_reference(name, dtype):
    y = _forward(name, dtype)
    want = FX[name]["out"]
    assert y.shape == want.shape and y.dtype == dtype
    _check(f"ens {name}", y.float().cpu(), want, dtype, fp32_tol=5e-5)


def test_fused_route_is_taken_by_the_fixture_models(monkeypatch):
    from anemoi_core_amd import ops

    calls = []
    real = ops.cond_layer_norm_proj
    monkeypatch.setattr(ops, "cond_layer_norm_proj", lambda *a, **k: calls.append(a[1].shape[-1]) or real(*a, **k))
    _forward("gt_3members", torch.bfloat16)
    assert calls == [4] * 4  # two blocks x two ConditionalLayerNorms
    calls.clear()
    _forward("gt_noise_injector", torch.bfloat16)
    assert calls == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_condition_on_residual_runs(dtype):
    """No reference output exists (its forward raises).  Shape, finiteness, and the appended columns are read: the same model with the
    residual's columns zeroed in the encoder input gives another result."""
    model, x, _ = E.ens_model(FX, "gt_cond_residual")
    E.fix_noise(model, FX["gt_3members"]["noise"])
    model = model.to(DEV, dtype)
    with torch.no_grad():
        y = model({"data": x.to(DEV, dtype)}, fcstep=1)["data"]
        assert y.shape == (1, 1, 3, x.shape[3], 4) and torch.isfinite(y).all()
        w = model.encoder["data"].emb_nodes_src.weight
        w[:, -4:] = 0  # the residual's columns are the last four of the input rows
        y0 = model({"data": x.to(DEV, dtype)}, fcstep=1)["data"]
    assert not torch.equal(y, y0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("N,D,C", [(1926, 64, 4), (10242, 512, 4), (1030, 1024, 16), (333, 100, 5)])
def test_conditional_layer_norm_fused_route_agrees_with_the_two_step_route(N, D, C, dtype, monkeypatch):
    from anemoi_core_amd import ops
    from anemoi_core_amd.layers.normalization import ConditionalLayerNorm

    torch.manual_seed(D + C)
    ln = ConditionalLayerNorm(D, condition_shape=C, zero_init=False).eval().to(DEV, dtype)
    x = (1.5 * torch.randn(N, D) + 0.3).to(DEV, dtype)
    cond, res = torch.randn(N, C).to(DEV, dtype), torch.randn(N, D).to(DEV, dtype)
    calls = []
    real = ops.cond_layer_norm_proj
    monkeypatch.setattr(ops, "cond_layer_norm_proj", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        fused, fused_res = ln(x, cond), ln(x, cond, res)
        assert len(calls) == 2
        monkeypatch.setattr(ConditionalLayerNorm, "_proj_route_ok", lambda self, x, cond: False)
        two, two_res = ln(x, cond), ln(x, cond, res)
        assert len(calls) == 2
    assert_close(fused, two.double(), dtype, "fused vs two-step")
    assert_close(fused_res, two_res.double(), dtype, "fused vs two-step, residual")
    p = {k: v.double().cpu() for k, v in ln.state_dict().items()}
    xd, cd = x.double().cpu(), cond.double().cpu()
    want = torch.nn.functional.layer_norm(xd, (D,)) * (1 + cd @ p["scale.weight"].T + p["scale.bias"]) + cd @ p["bias.weight"].T + p["bias.bias"]
    assert_close(fused, want, dtype, "fused vs float64")


def test_wide_conditionings_keep_the_two_step_route(monkeypatch):
    """C = 32 was measured slower on the fused route (layers/normalization.py: COND_PROJ_ROUTE_MAX); the op itself still takes it."""
    from anemoi_core_amd import ops
    from anemoi_core_amd.layers.normalization import ConditionalLayerNorm

    ln = ConditionalLayerNorm(512, condition_shape=32, zero_init=False).eval().to(DEV, torch.bfloat16)
    x, cond = torch.randn(1030, 512).to(DEV, torch.bfloat16), torch.randn(1030, 32).to(DEV, torch.bfloat16)
    with torch.no_grad():
        direct = ops.cond_layer_norm_proj(x, cond, *ln._proj.get(ln), ln.eps)
        monkeypatch.setattr(ops, "cond_layer_norm_proj", lambda *a, **k: pytest.fail("C = 32 belongs to the two-step route"))
        two = ln(x, cond)
    assert_close(direct, two.double(), torch.bfloat16, "C = 32: the op against the module's two-step route")


def test_autograd_keeps_the_two_step_route(monkeypatch):
    from anemoi_core_amd import ops
    from anemoi_core_amd.layers.normalization import ConditionalLayerNorm

    monkeypatch.setattr(ops, "cond_layer_norm_proj", lambda *a, **k: pytest.fail("the fused route has no backward"))
    ln = ConditionalLayerNorm(64, condition_shape=4, zero_init=False).to(DEV)
    y = ln(torch.randn(10, 64, device=DEV), torch.randn(10, 4, device=DEV))
    y.sum().backward()
    assert ln.scale.weight.grad is not None and torch.isfinite(ln.scale.weight.grad).all()


def test_weight_image_follows_a_parameter_update():
    from anemoi_core_amd.layers.normalization import ConditionalLayerNorm

    ln = ConditionalLayerNorm(64, condition_shape=4, zero_init=False).eval().to(DEV)
    x, cond = torch.randn(10, 64, device=DEV), torch.randn(10, 4, device=DEV)
    with torch.no_grad():
        a = ln(x, cond)
        assert torch.equal(a, ln(x, cond))
        ln.bias.bias.add_(1.0)
        b = ln(x, cond)
    assert torch.allclose(b, a + 1.0, atol=1e-5)


def test_default_draw_gives_different_finite_members():
    model, x, _ = E.ens_model(FX, "gt_3members")
    model = model.to(DEV, torch.bfloat16)
    xin = {"data": x.to(DEV, torch.bfloat16)}
    with torch.no_grad():
        a, b = model(xin, fcstep=1)["data"], model(xin, fcstep=1)["data"]
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, b)
    assert not torch.equal(a[:, :, 0], a[:, :, 1])  # members of one forward differ too


@pytest.mark.parametrize("name", ["gt_3members", "gt_noise_injector", "transformer_3members"])
def test_captured_forward_with_fixed_noise_replays_bit_equal(name):
    model, x, _ = E.ens_model(FX, name)
    noise = FX[name]["noise"].to(DEV)  # resident: the substitution involves no host -> device copy inside the capture
    E.fix_noise(model, noise)
    model = model.to(DEV, torch.bfloat16)
    xin = {"data": x.to(DEV, torch.bfloat16)}
    with torch.no_grad():
        eager = model(xin, fcstep=1)["data"].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(xin, fcstep=1)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(xin, fcstep=1)["data"]
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_default_draw_is_capturable():
    model, x, _ = E.ens_model(FX, "gt_3members")
    model = model.to(DEV, torch.bfloat16)
    xin = {"data": x.to(DEV, torch.bfloat16)}
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(xin, fcstep=1)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(xin, fcstep=1)["data"]
        graph.replay()
        a = out.clone()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(out).all() and not torch.equal(a, out)  # the generator advances between replays


def _sharded_worker(rank, world, group, kind):
    fx = E.load_fixture()
    name = "gt_3members" if kind == "gt" else "transformer_3members"
    model, x, _ = E.ens_model(fx, name)
    E.fix_noise(model, fx[name]["noise"][:, :1])  # one member per device when the model is sharded
    model = model.to("cuda", torch.bfloat16)
    xin = {"data": x[:, :, :1].to("cuda", torch.bfloat16)}
    with torch.no_grad():
        full = model(xin, fcstep=1)["data"]
        part = model(xin, fcstep=1, model_comm_group=group)["data"]
    return dict(full=full.float().cpu(), part=part.float().cpu())


@pytest.mark.parametrize("kind", ["gt", "transformer"])
def test_two_ranks_on_one_gpu_match_the_unsharded_model(kind):
    from tests.test_distributed_gpu import _spawn

    for o in _spawn(_sharded_worker, 2, kind):
        assert o["part"].shape == o["full"].shape
        _check(f"sharded ens {kind}", o["part"], o["full"], torch.bfloat16)
