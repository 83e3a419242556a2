"""AnemoiTransportModelEncProcDec and the EDM samplers on the MI355X against the imported reference's records (tests/golden/transport.pt):
the forward of every case in fp32 and bf16, ``sample()`` on the recorded draws against the reference's float64 result under 8 x its own
fp32 error (the rule of tests/test_sht_gpu.py: two fp32 evaluation orders of one computation), graph replay against eager sampling bit for
bit, ensemble members against batch entries, ``predict_step``, and the launches of one denoiser call."""
import pytest
import torch

from anemoi_core_amd import ops
from tests import transport_refs as R
from tests.test_fullsize_parity_gpu import _check

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = R.load_fixture()
MODEL_CASES = sorted(FX["models"])
SAMPLER_CASES = sorted(FX["samplers"])
_built = {}


def _model(name: str, dtype=torch.float32):
    """(model on the device, x, y, sigma), built once per (case, dtype) and left unchanged."""
    key = (name, dtype)
    if key not in _built:
        model, x, y, sigma, _ = R.transport_model(FX, name)
        if dtype != torch.float32:
            model.cast_network(dtype)
        _built[key] = (model.to(DEV), x.to(DEV), y.to(DEV), sigma.to(DEV))
    return _built[key]


def _replay(monkeypatch, model, draws):
    from anemoi_core_amd.samplers import EDMHeunSampler

    queue, draw = R.replay_draws(model, {}, draws)
    monkeypatch.setattr(EDMHeunSampler, "draw", lambda self, shape, dtype, device: draw(shape, dtype, device))
    return queue


def _count_replays(monkeypatch) -> list:
    """Every replay of a captured graph from here on appends to the returned list."""
    replays, real = [], torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), real(self))[1])
    return replays


@pytest.mark.parametrize("name", MODEL_CASES)
def test_forward_fp32(name):
    model, x, y, sigma = _model(name)
    with torch.no_grad():
        out = model({"data": x}, {"data": y}, {"data": sigma})["data"]
    want = FX["models"][name]["out"]
    assert out.shape == want.shape and out.dtype == torch.float32
    _check(f"transport {name}", out.cpu(), want, torch.float32, fp32_tol=5e-5)


@pytest.mark.parametrize("name", MODEL_CASES)
def test_forward_bf16(name):
    model, x, y, sigma = _model(name, torch.bfloat16)
    with torch.no_grad():
        out = model({"data": x}, {"data": y}, {"data": sigma})["data"]
    assert out.dtype == torch.float32  # the data dtype, whatever the network's
    _check(f"transport {name} bf16", out.cpu(), FX["models"][name]["out"], torch.bfloat16)


@pytest.mark.parametrize("key", SAMPLER_CASES)
def test_sample_matches_the_reference(key, monkeypatch):
    """sample() on the recorded draws against the reference's float64 run: error <= 8 x the reference's own fp32 error."""
    rec = FX["samplers"][key]
    model, x, _, _ = _model(rec["model"])
    queue = _replay(monkeypatch, model, rec["draws"])
    with torch.no_grad():
        out = model.sample({"data": x}, schedule_params=dict(rec["spec"]["schedule"]), sampler_params=dict(rec["spec"]["sampler"]))["data"]
    assert not queue and out.dtype == torch.float32 and out.shape == rec["out64"].shape
    err = R.rel_err(out.cpu(), rec["out64"])
    print(f"{key}: {err:.3e} (bound {8 * rec['err32']:.3e}; the reference's fp32 run: {rec['err32']:.3e})")
    assert err <= 8 * rec["err32"]


# expected replays: Heun over 4 steps captures predictor and corrector at step 1 and replays them at steps 1 and 2 (step 3 is the final
# kind); DPM++ over 5 steps runs first, multi (eager), multi (captured + replayed), multi (replayed), final
@pytest.mark.parametrize("key,replays", [("sin_b1/heun_churn4", 4), ("rff_b2/dpmpp_exp5", 2), ("sin_b1/dpmpp_exp5", 2)])
def test_graphed_sampling_is_bit_equal(key, replays, monkeypatch):
    rec = FX["samplers"][key]
    model, x, _, _ = _model(rec["model"])
    outs, counts = [], []
    for graphed in (False, True):
        queue = _replay(monkeypatch, model, rec["draws"])
        seen = _count_replays(monkeypatch)
        with torch.no_grad():
            outs.append(model.sample({"data": x}, schedule_params=dict(rec["spec"]["schedule"]),
                                     sampler_params=dict(rec["spec"]["sampler"], graphed=graphed))["data"])
        assert not queue
        counts.append(len(seen))
    assert counts == [0, replays], counts  # the graphed run really replayed captured steps
    assert torch.equal(outs[0], outs[1])
    assert R.rel_err(outs[1].cpu(), rec["out64"]) <= 8 * rec["err32"]


@pytest.mark.parametrize("name,captured,replays", [("heun_churn4", ["correct", "predict"], 4), ("dpmpp_exp5", ["multi"], 2)])
def test_samplers_around_any_denoiser(name, captured, replays, monkeypatch):
    """The sampler classes around a callable that is not the model's (the fixture's closed-form denoiser, evaluated in fp32 as the reference
    hands it its arguments): the reference's float64 run within 8 x its fp32 error; graphed - the kinds of step that occur more than once
    captured and replayed - bit-equal to eager."""
    from anemoi_core_amd.samplers import DIFFUSION_SAMPLERS

    rec = FX["analytic"][name]
    gen = torch.Generator().manual_seed(rec["input_seed"])
    x = torch.randn(2, FX["n_step_input"], 1, 37, 3, generator=gen).to(DEV)
    y0 = (torch.randn(2, 1, 1, 37, 3, generator=gen, dtype=torch.float64) * rec["sigmas"][0]).to(DEV)
    seen = []

    def denoise(xa, ya, sa, *_):
        seen.append((ya["data"].dtype, sa["data"].dtype, tuple(sa["data"].shape)))
        return {"data": R.analytic_denoise(xa["data"], ya["data"], sa["data"])}

    spec = dict(rec["spec"]["sampler"])
    sampler = spec.pop("sampler")
    outs = []
    for graphed in (False, True):
        s = DIFFUSION_SAMPLERS[sampler](dtype=torch.float64, graphed=graphed, **spec)
        queue = [t.clone() for t in rec["draws"]]
        s.draw = lambda shape, dtype, device: queue.pop(0).to(device=device, dtype=dtype)
        count = _count_replays(monkeypatch)
        # (once with the host schedule handed over, once with the device tensor alone: the same values either way)
        kw = dict(sigmas_host=rec["sigmas"]) if graphed else {}
        outs.append(s.sample({"data": x}, {"data": y0.clone()}, rec["sigmas"].to(DEV), denoise, **kw)["data"])
        assert not queue
        assert sorted(s.last_steps.graphs) == (captured if graphed else []) and len(count) == (replays if graphed else 0)
    assert all(rec_ == (torch.float32, torch.float32, (2, 1, 1, 1, 1)) for rec_ in seen)  # the reference's casts for a foreign callable
    assert torch.equal(outs[0], outs[1]) and outs[0].dtype == torch.float32
    err = R.rel_err(outs[0].cpu(), rec["out64"])
    print(f"{name}: {err:.3e} (bound {8 * rec['err32']:.3e})")
    assert err <= 8 * rec["err32"]


@pytest.mark.parametrize("key", ["sin_b1/heun_churn4", "sin_b1/dpmpp_exp5"])
def test_restated_samplers_around_the_model(key):
    """The float64 restatements of the samplers (tests/transport_refs.py) around this model's fp32 forward, on the recorded draws: the
    reference's float64 run within 8 x its fp32 error, and the sampler classes' result within the same distance of the restatement."""
    rec = FX["samplers"][key]
    model, x, _, _ = _model(rec["model"])
    def denoise(xa, ya, s):
        sig = torch.full((ya.shape[0], 1, ya.shape[2], 1, 1), s, dtype=torch.float32, device=DEV)
        with torch.no_grad():
            return model({"data": xa}, {"data": ya.float()}, {"data": sig})["data"].double()

    from anemoi_core_amd.transport import SIGMA_SCHEDULES

    sched = dict(rec["spec"]["schedule"])
    sigmas = SIGMA_SCHEDULES[sched.pop("schedule_type")](**sched).get_host_schedule()
    y0 = rec["draws"][0].to(DEV).double() * float(sigmas[0])  # the source field times the first sigma, as the objective starts
    spec = dict(rec["spec"]["sampler"])
    if spec.pop("sampler") == "heun":
        got = R.heun_ref(x, y0, sigmas, denoise, [d.to(DEV) for d in rec["draws"][1:]], **spec)
    else:
        got = R.dpmpp_ref(x, y0, sigmas, denoise, data_dtype=torch.float32)
    err = R.rel_err(got.cpu(), rec["out64"])
    print(f"{key} restated: {err:.3e} (bound {8 * rec['err32']:.3e})")
    assert err <= 8 * rec["err32"]


def test_ensemble_members_equal_batch_entries():
    """Members are folded into the batch: [1, T, 2, N, V] computes what [2, T, 1, N, V] computes on the same rows."""
    model, x, y, sigma = _model("sin_b2")
    to_members = lambda t: t.transpose(0, 2).contiguous()  # noqa: E731  [2, T, 1, ...] -> [1, T, 2, ...]
    with torch.no_grad():
        batch = model({"data": x}, {"data": y}, {"data": sigma})["data"]
        members = model({"data": to_members(x)}, {"data": to_members(y)}, {"data": to_members(sigma)})["data"]
    assert members.shape == (1, 1, 2) + tuple(batch.shape[3:])
    assert torch.equal(to_members(members), batch)


def test_predict_step_is_preprocess_sample_postprocess(monkeypatch):
    from types import SimpleNamespace as NS

    import numpy as np

    from anemoi_core_amd.preprocessing import InputNormalizer, Processors

    rec = FX["samplers"]["sin_b1/heun_karras4"]
    model, x, _, _ = _model("sin_b1")
    v = x.shape[-1]
    names = {f"v{i}": i for i in range(v)}
    group = lambda: NS(name_to_index=names, full=list(range(v)))  # noqa: E731
    stats = {"mean": np.array([0.3 * i for i in range(v)]), "stdev": np.array([1.0 + 0.5 * i for i in range(v)]), "minimum": np.full(v, -9.0),
             "maximum": np.full(v, 9.0)}
    norm = InputNormalizer(config={"default": "mean-std", "mean-std": list(names)}, data_indices=NS(data=NS(input=group(), output=group()), model=NS(input=group(), output=group())),
                           statistics=stats).to(DEV)
    pre, post = Processors([["normalizer", norm]]), Processors([["normalizer", norm]], inverse=True)
    raw = (x[:, :, 0] * 2.0 + 1.0).contiguous()  # [batch, time, grid, vars]
    kw = dict(schedule_params=dict(rec["spec"]["schedule"]), sampler_params=dict(rec["spec"]["sampler"]))
    _replay(monkeypatch, model, rec["draws"])
    got = model.predict_step({"data": raw}, {"data": pre}, {"data": post}, FX["n_step_input"], **kw)["data"]
    _replay(monkeypatch, model, rec["draws"])
    with torch.no_grad():
        want = post(model.sample({"data": pre(raw[:, :, None], in_place=False)}, **kw)["data"], in_place=False)
    assert got.shape == want.shape == (1, 1, 1) + tuple(raw.shape[2:]) and torch.isfinite(got).all() and torch.equal(got, want)


def test_launches_of_one_denoiser_call(monkeypatch):
    """Around the network run exactly one launch each of the three edge kernels, and no torch operation that produces a tensor as large as the
    state, 5-D or flattened."""
    model, x, y, sigma = _model("sin_b2")
    with torch.no_grad():
        model({"data": x}, {"data": y}, {"data": sigma})  # builds what the network caches
    seen = []
    lib = ops._lib.load()
    for tag, name in (("cond", "anemoi_noise_cond_fwd"), ("in", "anemoi_transport_assemble_input"), ("out", "anemoi_edm_output"),
                      ("update", "anemoi_edm_update")):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _r=real, _t=tag: (seen.append(_t), _r(*a))[1])
    state_numel = y.numel()  # the smallest tensor that holds a whole state, in any layout
    big = []
    from torch.utils._python_dispatch import TorchDispatchMode

    views = ("view", "expand", "permute", "reshape", "slice", "select", "unsqueeze", "squeeze", "alias", "detach", "as_strided", "transpose", "t.default")

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func)
            # the network's own launches and views are not the edge's; an operation that hands back its argument computed nothing
            if name.startswith("anemoi_hip.") or any(v in name for v in views):
                return out
            for t in (out if isinstance(out, (tuple, list)) else (out,)):
                if isinstance(t, torch.Tensor) and t.numel() >= state_numel and not any(
                        isinstance(a, torch.Tensor) and a.data_ptr() == t.data_ptr() and a.dtype == t.dtype for a in args):
                    big.append(name)
            return out

    with torch.no_grad(), Watch():
        model({"data": x}, {"data": y}, {"data": sigma})
    assert sorted(seen) == ["cond", "in", "out"], seen
    # no torch operation produces a tensor as large as the state, in whatever layout (5-D or flattened rows): what is left are the
    # allocations of the kernels' outputs
    assert big and all(name.startswith("aten.empty") for name in big), big
