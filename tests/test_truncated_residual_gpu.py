"""The truncated residual on the MI355X: the layer and whole models against the reference's outputs (tests/golden/truncation.pt)."""
import pytest
import torch

from anemoi_core_amd import ops
from tests import truncation_helpers as H
from tests.test_fullsize_parity_gpu import _check
from tests.test_kernels_gpu import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = H.load_fixture()


def _layer():
    from anemoi_core_amd.layers.residual import TruncatedConnection

    _, gd = H.graph_data(FX)
    layer = TruncatedConnection(graph=gd, truncation_down_edges_name=H.DOWN, truncation_up_edges_name=H.UP, row_normalize=True)
    lf = FX["layer"]
    x = torch.randn(lf["batch"], H.N_STEP_IN, 1, gd["data"].num_nodes, H.N_VARS, generator=torch.Generator().manual_seed(lf["input_seed"]))
    return layer, x


def test_layer_matches_the_reference_under_the_composed_bound():
    """Two projections: the error of the first (bound b1 on the coarse grid) passes through |U|, the second adds its own bound on the rounded
    intermediate; the reference itself is fp32 torch.sparse.mm twice, which stays inside the same two terms - hence twice the sum."""
    layer, x = _layer()
    y = layer(x.to(DEV))
    assert y.shape == FX["layer"]["out"].shape and y.dtype == torch.float32
    d, u = layer.provider_down, layer.provider_up
    x64 = x[:, -1].double()
    coarse = H.project64(d.indptr, d.indices, d.values, d.shape[0], x64)
    b1 = H.projection_bound(d.indptr, d.indices, d.values, d.shape, x64.abs(), coarse, torch.float32)
    want = H.project64(u.indptr, u.indices, u.values, u.shape[0], coarse)
    b2 = H.projection_bound(u.indptr, u.indices, u.values, u.shape, coarse.abs() + b1, want, torch.float32)
    bound = b2 + H.project64(u.indptr, u.indices, abs(u.values), u.shape[0], b1)
    err = (y.double().cpu() - want).abs()
    print(f"layer vs float64: max err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    ref_err = (y.double().cpu() - FX["layer"]["out"].double()).abs()
    print(f"layer vs reference: max err {float(ref_err.max()):.3e}, worst err / (2 bound) {float((ref_err / (2 * bound)).max()):.3f}")
    assert bool((ref_err <= 2 * bound).all())
    y2 = layer(x.to(DEV), n_step_output=2)
    assert y2.shape == FX["layer"]["out_2steps"].shape and torch.equal(y2[:, 0], y) and torch.equal(y2[:, 1], y)
    cols = torch.tensor([3, 0], dtype=torch.int32, device=DEV)
    assert torch.equal(layer(x.to(DEV), cols=cols), y[..., [3, 0]])  # a column's result does not depend on which others are selected


def _run(name, dtype, residual=None):
    model, x = H.build_model(FX, name, residual=residual)
    entry = FX["models"][name]
    if "noise" in entry:
        from tests.ens_helpers import fix_noise

        fix_noise(model, entry["noise"])
    model = model.to(DEV, dtype)
    kw = {"fcstep": 1} if entry["case"]["model"] == "ens" else {}
    with torch.no_grad():
        return model({"data": x.to(DEV, dtype)}, **kw)["data"]


@pytest.mark.parametrize("name", sorted(H.MODEL_CASES))
def test_fp32_model_matches_the_reference(name):
    want = FX["models"][name]["out"]
    y = _run(name, torch.float32)
    assert y.shape == want.shape and y.dtype == torch.float32
    print(f"{name}: max err {float((y.cpu() - want).abs().max()):.3e} on max |ref| {float(want.abs().max()):.3f}")
    assert_close(y, want, torch.float32, name)
    _check(f"truncated {name}", y.float().cpu(), want, torch.float32, fp32_tol=5e-5)


def test_the_plain_skip_computes_something_else():
    """The same model and draw with the SkipConnection residual is far from the truncated reference: what a model that ignores
    ``model.residual`` returns."""
    want = FX["models"]["gt_batch1"]["out"]
    y = _run("gt_batch1", torch.float32, residual={"_target_": "anemoi.models.layers.residual.SkipConnection", "step": -1})
    assert float((y.cpu() - want).abs().max()) > 0.5


@pytest.mark.parametrize("name", sorted(H.MODEL_CASES))
def test_bf16_model_agrees_with_its_fp32_twin(name):
    y32 = _run(name, torch.float32)
    y16 = _run(name, torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and torch.isfinite(y16).all()
    _check(f"truncated {name} bf16 vs fp32 twin", y16.float().cpu(), y32.cpu(), torch.bfloat16)
    _check(f"truncated {name} bf16 vs reference", y16.float().cpu(), FX["models"][name]["out"], torch.bfloat16)


def _normalizer(n_vars, device):
    from types import SimpleNamespace

    import numpy as np

    from anemoi_core_amd.models.configs import make_data_indices
    from anemoi_core_amd.preprocessing import InputNormalizer, Processors

    rng = np.random.default_rng(3)
    mean, stdev = rng.normal(size=n_vars).astype(np.float32), (0.5 + rng.random(n_vars)).astype(np.float32)
    stats = {"mean": mean, "stdev": stdev, "minimum": mean - 3 * stdev, "maximum": mean + 3 * stdev}
    di = make_data_indices(H.N_VARS, H.N_PROG)["data"]
    full = list(range(n_vars))
    di.data.input.full, di.data.output = full, SimpleNamespace(full=list(range(H.N_PROG)), name_to_index={f"v{i}": i for i in range(H.N_PROG)})
    nm = InputNormalizer(config={"default": "mean-std"}, data_indices=di, statistics=stats).to(device)
    return nm, Processors([["normalizer", nm]]), Processors([["normalizer", nm]], inverse=True)


class _Opaque(torch.nn.Module):
    """Hides a Processors chain from the fusion: forces normalise-then-forward."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, **kw):
        return self.inner(x, **kw)


def test_predict_step_with_a_fused_normaliser_equals_normalise_then_forward(monkeypatch):
    model, x = H.build_model(FX, "gt_batch1")
    model = model.to(DEV)
    nm, pre, post = _normalizer(H.N_VARS, DEV)
    batch = {"data": (3.0 * x[:, :, 0] + 1.0).to(DEV)}  # raw data: [batch, time, grid, vars]
    unfused = model.predict_step(batch, {"data": _Opaque(pre)}, {"data": _Opaque(post)}, H.N_STEP_IN)["data"]
    seen = []
    real = ops.sparse_project
    monkeypatch.setattr(ops, "sparse_project", lambda x_, m_, cols=None, mul=None, add=None, out_dtype=None: (
        seen.append(mul is not None and add is not None), real(x_, m_, cols, mul, add, out_dtype))[1])

    def boom(*a, **k):
        raise AssertionError("the stand-alone normaliser kernel ran inside the fused predict_step")

    monkeypatch.setattr(ops, "affine_columns", boom)
    fused = model.predict_step(batch, {"data": pre}, {"data": post}, H.N_STEP_IN)["data"]
    assert seen == [True, False]  # the down projection carries the column program, the up projection none
    scale = max(1.0, float(unfused.abs().max()))
    print(f"fused vs unfused predict_step: max diff {float((fused - unfused).abs().max()):.3e} at scale {scale:.3f}")
    assert float((fused - unfused).abs().max()) <= 2e-6 * scale  # same arithmetic, fused or not (tests/test_edges_gpu.py)


@pytest.mark.parametrize("name,dtype", [("gt_batch1", torch.bfloat16), ("gt_batch2", torch.float32), ("ens_gt_2x2", torch.bfloat16)])
def test_whole_forward_captured_as_a_graph_replays_bit_equal(name, dtype):
    model, x = H.build_model(FX, name)
    entry = FX["models"][name]
    kw = {"fcstep": 1} if entry["case"]["model"] == "ens" else {}
    if "noise" in entry:
        from tests.ens_helpers import fix_noise

        fix_noise(model, entry["noise"].to(DEV))
    model = model.to(DEV, dtype)
    xin = {"data": x.to(DEV, dtype)}
    with torch.no_grad():
        eager = model(xin, **kw)["data"]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(xin, **kw)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(xin, **kw)["data"]
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_rollout_gradient_flows_through_the_skip():
    """Rollout training feeds an output back as the next input, so the residual carries gradients: d out / d x through the two projections
    equals the float64 U D applied to the prognostic columns (the model part is cut off by comparing the layer alone)."""
    layer, x = _layer()
    cols = torch.arange(H.N_PROG, dtype=torch.int32, device=DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = layer(xg, cols=cols)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    (gx,) = torch.autograd.grad(y, xg, g)
    d, u = layer.provider_down, layer.provider_up
    D, U = H.dense(d.indptr, d.indices, d.values, d.shape), H.dense(u.indptr, u.indices, u.values, u.shape)
    want = torch.zeros(x.shape, dtype=torch.float64)
    want[:, -1, ..., :H.N_PROG] = torch.einsum("tn,mt,bemc->benc", D, U, g.double().cpu())
    assert float((gx.double().cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
