"""The EDM diffusion family without a GPU: schedules, settings, sources and state_dict against the imported reference's records
(tests/golden/transport.pt), the float64 restatements of tests/transport_refs.py against the same records, and the C ABI's new entries."""
import math
import os
import re

import pytest
import torch

from anemoi_core_amd import _lib, ops
from tests import transport_refs as R
from tests.test_abi_cpu import HEADER, header_functions

NEW_ENTRIES = ("anemoi_noise_cond_fwd", "anemoi_transport_assemble_input", "anemoi_edm_output", "anemoi_edm_update")


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


# ---------------------------------------------------------------------------------------------- schedules
def test_schedules_match_the_reference(fx):
    from anemoi_core_amd.transport import SIGMA_SCHEDULES

    assert set(SIGMA_SCHEDULES) == {kind for kind, _ in fx["schedules"]}
    for (kind, n), rec in fx["schedules"].items():
        got = SIGMA_SCHEDULES[kind](**rec["kwargs"]).get_schedule(None, torch.float64)
        want = rec["values"]
        assert got.dtype == torch.float64 and got.shape == want.shape == (n + 1,)
        assert float(got[-1]) == 0.0  # the exact final zero
        assert float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) <= 1e-12, (kind, n)
        assert float(got[0]) == pytest.approx(100.0, rel=1e-12) and (n == 1 or float(got[-2]) == pytest.approx(0.02, rel=1e-12))


def test_schedule_validation():
    from anemoi_core_amd.transport import KarrasSigmaSchedule, LinearSigmaSchedule

    for kw, text in ((dict(sigma_max=1.0, sigma_min=0.0, num_steps=2), "sigma_min must be strictly positive"),
                     (dict(sigma_max=-1.0, sigma_min=0.1, num_steps=2), "sigma_max must be strictly positive"),
                     (dict(sigma_max=0.1, sigma_min=1.0, num_steps=2), "greater than or equal"),
                     (dict(sigma_max=1.0, sigma_min=0.1, num_steps=0), "num_steps must be at least 1")):
        with pytest.raises(ValueError, match=text):
            KarrasSigmaSchedule(**kw)

    class Explicit(LinearSigmaSchedule):  # a schedule that brings its own final value
        def __init__(self, last):
            super().__init__(1.0, 0.5, 2)
            self.last = last

        def _build_schedule(self, dtype_compute):
            return torch.tensor([1.0, 0.5, self.last], dtype=dtype_compute)

    assert Explicit(1e-11).get_schedule().tolist() == [1.0, 0.5, 0.0]
    with pytest.raises(ValueError, match="must end at zero"):
        Explicit(1e-3).get_schedule()

    class Short(LinearSigmaSchedule):
        def _build_schedule(self, dtype_compute):
            return torch.ones(1, dtype=dtype_compute)

    with pytest.raises(ValueError, match="must contain 3 values"):
        Short(1.0, 0.5, 3).get_schedule()


def test_host_and_device_schedules_are_the_same_values():
    from anemoi_core_amd.transport import ExponentialSigmaSchedule

    sched = ExponentialSigmaSchedule(100.0, 0.02, 5)
    host = sched.get_host_schedule(torch.float64)
    assert host.device.type == "cpu" and host.dtype == torch.float64 and host.shape == (6,) and float(host[-1]) == 0.0
    assert torch.equal(sched.get_schedule(None), host) and torch.equal(sched.get_schedule("cpu"), host)


# ---------------------------------------------------------------------------------------------- settings, sources, objectives
def test_settings_read_mappings_and_objects():
    from types import SimpleNamespace

    from anemoi_core_amd.transport import EdmSettings, NoiseConditioningSettings, TransportSourceSettings

    assert NoiseConditioningSettings.from_config({}) == NoiseConditioningSettings(32, 16)
    assert NoiseConditioningSettings.from_config({"noise_channels": 8, "noise_cond_dim": "4"}) == NoiseConditioningSettings(8, 4)
    assert EdmSettings.from_config({}) == EdmSettings(1.0, 100.0, 0.02, 7.0)
    assert EdmSettings.from_config(SimpleNamespace(sigma_data=0.5, rho=3)) == EdmSettings(0.5, 100.0, 0.02, 3.0)
    assert TransportSourceSettings.from_config({}) == TransportSourceSettings("default", 1.0, 0.0)
    assert TransportSourceSettings.from_config({"source": {"kind": "zero", "scale": 2}}) == TransportSourceSettings("zero", 2.0, 0.0)
    with pytest.raises(Exception):
        EdmSettings().sigma_data = 2.0  # frozen


def test_sources():
    from anemoi_core_amd.transport import TransportSourceBuilder, sampling_source_specs

    x = {"data": torch.zeros(2, 3, 4, 5, 6), "other": torch.zeros(2, 3, 4, 7, 6, dtype=torch.float64)}
    specs = sampling_source_specs(x, n_step_output=2, num_output_channels={"data": 3, "other": 1})
    assert specs["data"].shape == (2, 2, 4, 5, 3) and specs["other"].shape == (2, 2, 4, 7, 1) and specs["other"].dtype == torch.float64
    zero = TransportSourceBuilder.from_config({"source": {"kind": "zero"}}).build(specs)
    assert all(tuple(zero[ds].shape) == specs[ds].shape and not zero[ds].any() for ds in x)
    b = TransportSourceBuilder.from_config({"source": {"scale": 3.0}})
    assert b.resolve_kind("gaussian") == "gaussian" and b.resolve_kind("zero") == "zero"
    b.draw = lambda shape, dtype, device: torch.ones(shape, dtype=dtype, device=device)
    got = b.build(specs, default_kind="gaussian")
    assert all(got[ds].dtype == x[ds].dtype and bool((got[ds] == 3.0).all()) for ds in x)
    torch.manual_seed(3)
    fresh = TransportSourceBuilder().build(specs)["data"]
    torch.manual_seed(3)
    assert torch.equal(fresh, torch.randn(specs["data"].shape))  # the Gaussian source is torch.randn, drawn once per dataset in order


def test_objective_registry():
    from anemoi_core_amd.transport import EDMDiffusionModelObjective, get_transport_model_objective

    assert isinstance(get_transport_model_objective("edm_diffusion"), EDMDiffusionModelObjective)
    with pytest.raises(ValueError, match="Unknown transport model objective"):
        get_transport_model_objective("nope")


# ---------------------------------------------------------------------------------------------- embedders and the model's state
def test_embedders_match_the_reference(fx):
    from anemoi_core_amd.layers import diffusion

    for cls, rec in fx["embedders"].items():
        torch.manual_seed(77)
        emb = getattr(diffusion, cls)(**rec["kwargs"])
        assert list(emb.state_dict()) == list(rec["buffers"])
        for k, v in rec["buffers"].items():
            assert torch.equal(emb.state_dict()[k], v), (cls, k)  # same construction, same random stream
        assert torch.allclose(emb(rec["sigma"]), rec["out"], rtol=0, atol=1e-6)
        freq, pi = emb.embedding_operands()
        assert freq is emb.frequencies and (pi is None) == (cls == "SinusoidalEmbeddings")
        # the restated kernel with an identity-free tail: its embedding is the reference's, within its own bound on the argument
        a = (rec["sigma"] * freq * (1 if pi is None else 2 * pi)).double()
        assert float((torch.cat([a.sin(), a.cos()], -1) - rec["out"].double()).abs().max()) <= 2.0**-22 * float(a.abs().max()) + 1e-6


@pytest.mark.parametrize("name", ["sin_b1", "rff_b2", "sin_2steps_out", "sin_forcing"])
def test_state_dict_matches_the_reference(fx, name):
    model, x, y, sigma, psum = R.transport_model(fx, name)
    entry = fx["models"][name]
    sd = model.state_dict()
    assert list(sd) == list(entry["keys"])  # same keys in the same order: the parameter draw depends on it
    assert {k: tuple(v.shape) for k, v in sd.items()} == entry["keys"]
    assert psum == pytest.approx(entry["param_sum"], rel=1e-12)
    assert dict(model.input_dim) == entry["input_dim"]
    assert tuple(y.shape)[1:] == tuple(entry["out"].shape)[1:]
    for k in ("noise_cond_mlp.linear1_no_gradscaling.weight", "noise_cond_mlp.linear2_no_gradscaling.bias", "noise_embedder.frequencies"):
        assert k in sd
    other = R.transport_model(fx, name)[0]
    with torch.no_grad():
        for p in other.state_dict().values():
            if torch.is_floating_point(p):
                p.zero_()
    assert other.load_state_dict(sd, strict=True).missing_keys == []
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))


def test_model_attributes_and_metadata(fx):
    from anemoi_core_amd.transport import EdmSettings, NoiseConditioningSettings

    model = R.transport_model(fx, "sin_forcing")[0]
    assert model.edm == EdmSettings() and model.noise_conditioning == NoiseConditioningSettings()
    assert (model.noise_channels, model.noise_cond_dim) == (32, 16)
    assert model.input_dim["data"] == 2 * 6 + 4 + model.node_attributes.attr_ndims["data"]
    md = {"metadata_inference": {"data": {}}}
    model.fill_metadata(md)
    assert md["metadata_inference"]["data"]["shapes"] == {"variables": model.input_dim["data"], "input_timesteps": 2, "ensemble": 1, "grid": None}
    # a 16-bit network keeps the embedder's buffers in fp32
    model.cast_network(torch.bfloat16)
    assert model.noise_embedder.frequencies.dtype == torch.float32 and model.noise_cond_mlp.linear1_no_gradscaling.weight.dtype == torch.bfloat16


def test_fixture_notes_record_the_references_ensemble_error(fx):
    assert "index" in fx["notes"]["ensemble"] and "out of bounds" in fx["notes"]["ensemble"]


# ---------------------------------------------------------------------------------------------- the restated samplers
@pytest.mark.parametrize("name", ["heun_karras4", "heun_churn4", "dpmpp_exp3", "dpmpp_exp5"])
def test_restated_samplers_reproduce_the_reference(fx, name):
    """The float64 restatements around the fixture's closed-form denoiser against the reference's sampler classes in float64: within the
    reference's own fp32 error (they agree to ~1e-15; err32 is the yardstick the GPU tests scale).  The model's own sampler cases need the
    network, which has no CPU path: tests/test_transport_model_gpu.py holds them to the same records on the GPU."""
    rec = fx["analytic"][name]
    gen = torch.Generator().manual_seed(rec["input_seed"])
    x = torch.randn(2, fx["n_step_input"], 1, 37, 3, generator=gen)
    y0 = torch.randn(2, 1, 1, 37, 3, generator=gen, dtype=torch.float64) * rec["sigmas"][0]
    spec = dict(rec["spec"]["sampler"])
    if spec.pop("sampler") == "heun":
        got = R.heun_ref(x.double(), y0, rec["sigmas"], R.analytic_denoise, rec["draws"], **spec)
    else:
        got = R.dpmpp_ref(x.double(), y0, rec["sigmas"], R.analytic_denoise)
    err = R.rel_err(got, rec["out64"])
    print(f"{name}: {err:.3e} (err32 {rec['err32']:.3e})")
    assert err <= rec["err32"] and 1e-8 < rec["err32"] < 1e-4
    assert R.rel_err(rec["out"], rec["out64"]) == pytest.approx(rec["err32"])


@pytest.mark.parametrize("name", ["sin_b2", "rff_b2"])
def test_restated_edge_kernels_reproduce_the_references_float64_forward(fx, name):
    """The restatements the GPU tests hold the kernels to, against the pieces of the reference's float64 forward recorded in the fixture:
    the conditioning vector of every group (kernel 1), the assembled input rows (kernel 2), and the EDM blend of the recorded network
    output, which must be the recorded forward (kernel 3).  Each within its own bound for fp32 output."""
    entry = fx["models"][name]
    model, x, y, sigma, _ = R.transport_model(fx, name)
    sd = model.edm.sigma_data
    freq, pi = model.noise_embedder.embedding_operands()
    l1, l2 = model.noise_cond_mlp.linear1_no_gradscaling, model.noise_cond_mlp.linear2_no_gradscaling
    with torch.no_grad():
        cond, bound = R.noise_cond_ref(sigma.reshape(-1), freq, pi, l1.weight, l1.bias, l2.weight, l2.bias, True, torch.float32)
        assert cond.shape == entry["cond64"].shape
        err = (cond - entry["cond64"]).abs()
        print(f"{name} cond: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
        assert bool((err <= bound).all())
        attrs = model.node_attributes("data", batch_size=1)
        rows, bound = R.assemble_input_ref(x, y, attrs, model.input_dim["data"], sigma.reshape(-1), sd, torch.float32)
        step = entry["row_step"]
        assert rows[::step].shape == entry["rows64"].shape
        assert bool(((rows[::step] - entry["rows64"]).abs() <= bound[::step]).all())
        B, T, E, N, V = entry["pred64"].shape
        pred = entry["pred64"].permute(0, 2, 3, 1, 4).reshape(B * E * N, T * V)  # the network's output rows
        D, bound = R.edm_output_ref(pred, y, sigma.reshape(-1), tuple(y.shape), sd, torch.float32)
        assert bool(((D - entry["out64"]).abs() <= bound).all())


def test_restated_kernels_are_self_consistent():
    """The restatements the GPU tests compare against, on the CPU: the update modes compose into the restated Heun / DPM++ steps, the two edges
    with sigma_data = 1 reproduce the closed forms, and every bound is positive where something is computed and zero where values are copied."""
    g = torch.Generator().manual_seed(5)
    y, D = torch.randn(7, generator=g, dtype=torch.float64), torch.randn(7, generator=g, dtype=torch.float64)
    params = torch.tensor([3.0, 1.5, 1e-10, 0.5, -0.5, 1.25, -0.25, 0.0], dtype=torch.float64)
    pred = R.edm_update_ref(R.HEUN_PREDICT, params, y, D, None, None, torch.float64)
    d1, y_next = pred["aux1"][0], pred["aux2"][0]
    assert torch.allclose(y_next, y + (1.5 - 3.0) * (y - D) / (3.0 + 1e-10), rtol=1e-15)
    assert torch.equal(R.edm_update_ref(R.HEUN_FINAL, params, y, D, None, None, torch.float64)["y"][0], y_next)
    cor = R.edm_update_ref(R.HEUN_CORRECT, params, y, D, d1, y_next, torch.float64)["y"]
    assert torch.allclose(cor[0], y - 1.5 * (d1 + (y_next - D) / (1.5 + 1e-10)) / 2, rtol=1e-15) and bool((cor[1] > 0).all())
    multi = R.edm_update_ref(R.DPMPP_MULTI, params, y, D, d1, None, torch.float64)
    assert torch.allclose(multi["y"][0], 0.5 * y + 0.5 * (1.25 * D - 0.25 * d1), rtol=1e-15) and torch.equal(multi["aux1"][0], D)
    assert torch.equal(R.edm_update_ref(R.DPMPP_FIRST, params, y, D, None, None, torch.float64)["y"][0], 0.5 * y + 0.5 * D)
    assert torch.equal(R.edm_update_ref(R.DPMPP_FINAL, params, y, D, None, None, torch.float64)["y"][0], D)
    # edges
    x, yy = torch.randn(2, 2, 1, 5, 3, generator=g), torch.randn(2, 1, 1, 5, 2, generator=g, dtype=torch.float64)
    attrs, sigma = torch.randn(5, 3, generator=g), torch.tensor([0.5, 20.0], dtype=torch.float64)
    out, bound = R.assemble_input_ref(x, yy, attrs, 16, sigma, 1.0, torch.float32)
    assert out.shape == (10, 16) and not out[:, 11:].any() and not bound[:, 11:].any()
    assert torch.equal(out[5:, :3], x[1, 0, 0].double()) and torch.equal(out[:5, 8:11], attrs.double())
    assert torch.allclose(out[5:, 6:8], yy[1, 0, 0] / math.sqrt(401.0), rtol=1e-12)
    predn = torch.randn(10, 2, generator=g)
    Dd, b = R.edm_output_ref(predn, yy, sigma, (2, 1, 1, 5, 2), 1.0, torch.float64)
    assert torch.allclose(Dd[1, 0, 0], yy[1, 0, 0] / 401.0 + 20.0 / math.sqrt(401.0) * predn[5:].double(), rtol=1e-12) and bool((b > 0).all())
    plain, _ = R.edm_output_ref(predn, None, None, (2, 1, 1, 5, 2), 1.0, torch.float32)
    assert torch.equal(plain[0, 0, 0], predn[:5].double())
    # conditioning: the restatement is the reference's modules (fp32) within its own bound
    lin1, lin2 = torch.nn.Linear(8, 8).requires_grad_(False), torch.nn.Linear(8, 4).requires_grad_(False)
    freq, vals = torch.randn(4, generator=g) * 16, torch.tensor([0.02, 1.0, 100.0])
    pi = torch.tensor(math.pi)
    cond, cb = R.noise_cond_ref(vals, freq, pi, lin1.weight, lin1.bias, lin2.weight, lin2.bias, True, torch.float32)
    with torch.no_grad():
        a = (vals.log() / 4.0)[:, None] * freq * 2 * pi
        want = lin2(torch.nn.functional.silu(lin1(torch.cat([a.sin(), a.cos()], -1))))
    assert bool(((cond - want.double()).abs() <= cb).all()) and float(cb.max()) < 1e-4


# ---------------------------------------------------------------------------------------------- the C ABI
def test_new_entries_are_declared_bound_built_and_cited():
    decl = header_functions()
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW_ENTRIES:
        assert name in decl and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][0]) == decl[name], name
        assert hasattr(lib, name), name
        head = text[:re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M).start()]
        comment = head[head.rindex("/*"):]
        assert "Replaces:" in comment and comment.count("*/") == 1, name
        assert re.search(r"\w+/\w+\.py:\d+", comment), name
    assert lib.anemoi_hip_abi_version() == _lib.ABI_VERSION  # entries were added without a bump: nothing earlier changed meaning
    for fn in ("noise_cond", "transport_assemble_input", "edm_output", "edm_update_"):
        assert callable(getattr(ops, fn))
    from anemoi_core_amd.models import AnemoiTransportModelEncProcDec  # noqa: F401  (exported)
    from anemoi_core_amd.samplers import DIFFUSION_SAMPLERS

    assert set(DIFFUSION_SAMPLERS) == {"heun", "dpmpp_2m"}
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "csrc", "transport.hip"))
