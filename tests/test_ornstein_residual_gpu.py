"""The spectral Ornstein residual on the MI355X: the layer against every recorded case of the reference (tests/golden/sht.pt) under 8 x the
reference's own fp32 error (the rule of tests/test_sht_gpu.py), its cache and refusals, and the model with it against the reference's
model."""
import pytest
import torch

from anemoi_core_amd import ops
from tests import sht_refs as R
from tests.test_fullsize_parity_gpu import _check
from tests.test_kernels_gpu import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = R.load_fixture()
CASES = sorted(k for k in FX["ornstein"] if k != "init")


@pytest.mark.parametrize("key", CASES)
def test_layer_matches_the_reference(key):
    e = FX["ornstein"][key]
    layer, _, _, variant = R.build_layer(key, e)
    layer = layer.to(DEV)
    x = R.layer_input(layer, e).to(DEV)
    before = x.clone()
    with torch.no_grad():
        y = layer(x)
        y2 = layer(x, n_step_output=2)
    assert tuple(y.shape) == e["out_shape"] and tuple(y2.shape) == e["out_shape_2steps"] and y.dtype == torch.float32
    assert torch.equal(y2[:, 0], y) and torch.equal(y2[:, 1], y)
    assert torch.equal(x, before)  # the input is read in place and left as it was
    prog = layer._internal_input_idx
    rest = [c for c in range(R.ORN_VARS) if c not in prog]
    assert float(y[..., rest].abs().max()) == 0.0
    err = R.rel_err(y[..., prog].cpu().numpy(), e["out64"].numpy())
    print(f"{key}: {err:.3e} (bound {8 * e['err32']:.3e})")
    assert err <= 8 * e["err32"]
    with torch.no_grad():
        assert torch.equal(layer.compact(x[:, -1]), y[..., prog])
        xb = x.clone()
        assert torch.equal(layer.compact(xb[:, -1], write_back=True), y[..., prog])  # the same skip, and the filtered fields left in xb
        changed = (xb != x).any(dim=0).any(dim=0).any(dim=0).any(dim=0).cpu().tolist()
        want = [variant["truncate"] and c in layer._truncation_input_idx for c in range(R.ORN_VARS)]
        assert changed == want and torch.equal(xb[:, 0], x[:, 0])


def test_launch_counts(monkeypatch):
    """Five launches with truncation (two per transform, one combine), the combine alone without - once the synthesised fields are cached."""
    for key, want in (("oct_lmax5/trunc_aa", ["fwd", "inv", "combine"]), ("oct_lmax5/plain", ["combine"])):
        e = FX["ornstein"][key]
        layer = R.build_layer(key, e)[0].to(DEV)
        x = R.layer_input(layer, e).to(DEV)
        with torch.no_grad():
            layer.compact(x[:, -1])  # builds the cache
        seen = []
        lib = ops._lib.load()
        for tag, name in (("fwd", "anemoi_sht_fwd"), ("inv", "anemoi_sht_inv"), ("combine", "anemoi_ornstein_combine_fwd")):
            real = getattr(lib, name)
            monkeypatch.setattr(lib, name, lambda *a, _r=real, _t=tag: (seen.append(_t), _r(*a))[1])
        with torch.no_grad():
            layer.compact(x[:, -1])
        assert seen == want, key
        monkeypatch.undo()


def test_cache_is_rebuilt_after_a_parameter_changes_in_place():
    key = "oct_lmax2/trunc_aa"
    e = FX["ornstein"][key]
    layer = R.build_layer(key, e)[0].to(DEV)
    x = R.layer_input(layer, e).to(DEV)
    with torch.no_grad():
        y0 = layer(x)
        assert layer._fields() is layer._fields()  # cached
        for name in ("weight", "filter", "walias"):
            getattr(layer, name).mul_(1.5)
            y1 = layer(x)
            assert not torch.equal(y1, y0), name
            twin = R.build_layer(key, e)[0].to(DEV)
            twin.load_state_dict(layer.state_dict())
            assert torch.equal(twin(x), y1), name  # what a fresh module computes from the same parameters
            y0 = y1


def test_grad_mode_and_dtype_refusals():
    key = "reg_lmax2/trunc_noaa"
    e = FX["ornstein"][key]
    layer = R.build_layer(key, e)[0].to(DEV)
    x = R.layer_input(layer, e).to(DEV)
    with pytest.raises(NotImplementedError, match="adjoint kernels"):
        layer(x)  # grad mode, parameters require grad
    layer.requires_grad_(False)
    assert layer(x).shape == e["out_shape"]
    with pytest.raises(NotImplementedError, match="adjoint kernels"):
        layer(x.clone().requires_grad_(True))
    with torch.no_grad():
        with pytest.raises(TypeError, match="float32"):
            layer(x.bfloat16())
        with pytest.raises(NotImplementedError, match="sharded"):
            layer(x, grid_shard_sizes=[272, 272])
    with pytest.raises(RuntimeError, match="MI355X"):
        layer(x.cpu())


def _model_run(residual="fixture"):
    model, x = R.build_model(FX, residual=residual)
    model = model.to(DEV)
    with torch.no_grad():
        return model, x, model({"data": x.to(DEV)})["data"]


def test_model_matches_the_reference():
    want = FX["model"]["out"]
    _, _, y = _model_run()
    assert y.shape == want.shape and y.dtype == torch.float32
    print(f"ornstein model: max err {float((y.cpu() - want).abs().max()):.3e} on max |ref| {float(want.abs().max()):.3f}")
    assert_close(y, want, torch.float32, "ornstein model")
    _check("ornstein model", y.float().cpu(), want, torch.float32, fp32_tol=5e-5)  # the truncated-residual model test's tolerance


def test_predict_step_equals_forward_on_normalised_inputs():
    from tests.test_truncated_residual_gpu import _normalizer

    model, x, _ = _model_run()
    case = FX["model"]["case"]
    nm, pre, post = _normalizer(case["n_vars"], DEV)
    batch = {"data": (3.0 * x[:, :, 0] + 1.0).to(DEV)}  # raw data [batch, time, grid, vars]
    got = model.predict_step(batch, {"data": pre}, {"data": post}, case["n_step_input"])["data"]
    with torch.no_grad():
        xn = pre(batch["data"][:, :, None], in_place=False)
        want = post(model({"data": xn})["data"], in_place=False)
    scale = max(1.0, float(want.abs().max()))
    print(f"predict_step vs forward: max diff {float((got - want).abs().max()):.3e} at scale {scale:.3f}")
    assert got.shape == want.shape and float((got - want).abs().max()) <= 2e-6 * scale  # same kernels on the same values


def test_default_forward_is_untouched_by_the_residual_option():
    """The default residual is still the skip: the same draw without ``model.residual`` is far from the Ornstein reference."""
    want = FX["model"]["out"]
    model, x = R.build_model(FX)
    plain, _ = R.build_model(FX, residual=None)
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("residual.")}
    plain.load_state_dict(sd)
    with torch.no_grad():
        y = plain.to(DEV)({"data": x.to(DEV)})["data"]
    assert float((y.cpu() - want).abs().max()) > 0.1
