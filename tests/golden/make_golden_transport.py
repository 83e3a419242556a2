"""Generate tests/golden/transport.pt by IMPORTING the Python reference's transport (EDM diffusion) family: its sigma schedules
(transport/schedules.py), its noise embedders (layers/diffusion.py), AnemoiTransportModelEncProcDec
(models/transport_encoder_processor_decoder.py) and its samplers (samplers/transport_samplers.py), CPU.

As in make_golden_ens.py, parameters and inputs are not stored: they are drawn from seeded CPU generators in state_dict order
(``tests.transformer_helpers.fill`` - which draws the embedders' ``frequencies`` / ``pi`` buffers as well, so the kernels must read
them), which the tests repeat.  The fixture holds, per model case, the configuration, the seeds, the reference's state_dict keys /
shapes, the checksum of the drawn parameters, the reference's forward in fp32, the same forward with model and inputs in float64, and
``err32 = max|y32 - y64| / max|y64|``; per sampler case the random numbers the reference drew (``torch.randn`` is wrapped while
``sample`` runs: the source field first, then the churn noise of every step), its fp32 result, the float64 rerun on the same draws,
and ``err32``.  Runs only where the reference is available (ref_standins).

One thing the reference does not do as written (recorded in ``notes``): with more than one ensemble member its forward raises - the hidden
node attributes are built for ``batch_size`` instead of ``batch_size * ensemble_size`` rows
(transport_encoder_processor_decoder.py:291).

Usage:  python tests/golden/make_golden_transport.py
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_standins as rs  # noqa: E402

rs.install()

from make_golden import make_data_indices, make_hetero  # noqa: E402

from anemoi_core_amd.graphs.synthetic import build_synthetic_graph  # noqa: E402
from anemoi_core_amd.models.configs import transport_model_config  # noqa: E402
from tests.transformer_helpers import fill  # noqa: E402  (the tests draw the same parameters)

N_STEP_IN = 2
SIGMAS = (0.02, 1.0, 100.0)
# name -> what differs from (SinusoidalEmbeddings, batch 1, 4 input = 4 output variables, one output step); tests/transport_refs.py
# (``transport_model``) builds this package's model from the same dict
MODEL_CASES = {
    "sin_b1": dict(sigma=[1.7]),
    "sin_b2": dict(batch=2, sigma=[0.3, 40.0]),
    "rff_b2": dict(batch=2, embedder="RandomFourierEmbeddings", sigma=[0.05, 6.0]),
    "sin_2steps_out": dict(n_step_output=2, sigma=[2.5]),
    "sin_forcing": dict(n_vars_in=6, n_vars_out=4, sigma=[0.8]),
}
SAMPLER_CASES = {
    "heun_karras4": dict(schedule=dict(schedule_type="karras", sigma_max=100.0, sigma_min=0.02, rho=7.0, num_steps=4), sampler=dict(sampler="heun")),
    "heun_churn4": dict(schedule=dict(schedule_type="karras", sigma_max=100.0, sigma_min=0.02, rho=7.0, num_steps=4),
                        sampler=dict(sampler="heun", S_churn=2.0)),  # gamma = min(2 / 4, sqrt 2 - 1) = sqrt 2 - 1
    "dpmpp_exp3": dict(schedule=dict(schedule_type="exponential", sigma_max=100.0, sigma_min=0.02, num_steps=3), sampler=dict(sampler="dpmpp_2m")),
    # five steps: the multistep update occurs three times (a graphed sampler runs it eagerly, captures it, replays it)
    "dpmpp_exp5": dict(schedule=dict(schedule_type="exponential", sigma_max=100.0, sigma_min=0.02, num_steps=5), sampler=dict(sampler="dpmpp_2m")),
}
EDGE_CASES = ("sin_b2", "rff_b2")  # model cases whose edges are recorded in float64: conditioning, input rows, network output
EDGE_ROW_STEP = 16  # every 16th input row is kept
SAMPLED_MODELS = ("sin_b1", "rff_b2")


def config_of(case: dict) -> dict:
    kw = {"scale": 16} if case.get("embedder") == "RandomFourierEmbeddings" else {"max_period": 1000}
    return transport_model_config("gt", 64, 2, 2, 8, noise_embedder=case.get("embedder", "SinusoidalEmbeddings"),
                                  inference_defaults={"sampling_schedule": {}, "sampler": {}}, **kw)  # (every sampler case brings its own)


def build(case: dict, index: int, batch=None, members: int = 1):
    from anemoi.models.models.transport_encoder_processor_decoder import AnemoiTransportModelEncProcDec

    g = build_synthetic_graph("o8", 3)
    v_in, v_out = case.get("n_vars_in", 4), case.get("n_vars_out", 4)
    torch.manual_seed(0)
    model = AnemoiTransportModelEncProcDec(model_config=rs.DotDict(config_of(case)), data_indices=make_data_indices(v_in, v_out),
                                           statistics={"data": None}, n_step_input=N_STEP_IN, n_step_output=case.get("n_step_output", 1),
                                           graph_data=make_hetero(g)).eval()
    param_seed, input_seed = 8000 + index, 9000 + index
    psum = fill(model, param_seed)
    B = batch or case.get("batch", 1)
    gen = torch.Generator().manual_seed(input_seed)
    x = torch.randn(B, N_STEP_IN, members, g.num_data, v_in, generator=gen)
    sigma = torch.tensor((case["sigma"] * (B * members))[:B * members], dtype=torch.float32).view(B, 1, members, 1, 1)
    y = torch.randn(B, case.get("n_step_output", 1), members, g.num_data, v_out, generator=gen) * (1 + sigma**2).sqrt()
    return model, x, y, sigma, dict(case=case, param_seed=param_seed, input_seed=input_seed, param_sum=psum,
                                    keys={k: tuple(v.shape) for k, v in model.state_dict().items()}, input_dim=dict(model.input_dim))


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def gen_model(name: str, case: dict, index: int) -> dict:
    model, x, y, sigma, built = build(case, index)
    with torch.no_grad():
        out32 = model({"data": x}, {"data": y}, {"data": sigma})["data"]
        model.double()
        out64 = model({"data": x.double()}, {"data": y.double()}, {"data": sigma.double()})["data"]
        edges = {}
        if name in EDGE_CASES:
            # the pieces of the float64 forward the edge kernels restate (tests/transport_refs.py): the conditioning vector of every group,
            # the assembled input rows, and the network's output that the EDM blend turns into out64
            s64, y64 = {"data": sigma.double()}, y.double()
            c_skip, c_out, c_in, c_noise = model.transport_model_objective._get_preconditioning(model, s64, model.edm.sigma_data)
            cond = model._embed_noise_conditioning(c_noise["data"][:, 0, :, 0])
            rows = model._assemble_input(x.double(), c_in["data"] * y64, x.shape[0] * x.shape[2], None, None, "data")[0]
            pred = model._forward_transport_network({"data": x.double()}, {"data": c_in["data"] * y64}, c_noise)["data"]
            assert torch.equal(c_skip["data"] * y64 + c_out["data"] * pred, out64)
            edges = dict(cond64=cond.reshape(-1, cond.shape[-1]).clone(), rows64=rows[::EDGE_ROW_STEP].clone(), row_step=EDGE_ROW_STEP,
                         pred64=pred.clone())
    print(name, tuple(out32.shape), "err32", rel_err(out32, out64))
    return dict(built, out=out32.clone(), out64=out64.clone(), err32=rel_err(out32, out64), **edges)


def gen_sampler(model_name: str, index: int, name: str, spec: dict) -> dict:
    model, x, _, _, _ = build(MODEL_CASES[model_name], index)
    real_randn, drawn = torch.randn, []

    def recording(*a, **kw):
        t = real_randn(*a, **kw)
        drawn.append(t.clone())
        return t

    def replaying(queue):
        def randn(shape, *a, dtype=None, device=None, **kw):
            t = queue.pop(0)
            assert tuple(t.shape) == tuple(shape), (t.shape, shape)
            return t.to(dtype=dtype)
        return randn

    noise_seed = 10000 + 10 * index + list(SAMPLER_CASES).index(name)
    torch.manual_seed(noise_seed)
    try:
        torch.randn = recording
        with torch.no_grad():
            out32 = model.sample({"data": x}, schedule_params=dict(spec["schedule"]), sampler_params=dict(spec["sampler"]))["data"]
        model.double()
        torch.randn = replaying([t.clone() for t in drawn])
        with torch.no_grad():
            out64 = model.sample({"data": x.double()}, schedule_params=dict(spec["schedule"]), sampler_params=dict(spec["sampler"]))["data"]
    finally:
        torch.randn = real_randn
    print(model_name, name, tuple(out32.shape), "draws", len(drawn), "err32", rel_err(out32, out64))
    return dict(model=model_name, spec=spec, noise_seed=noise_seed, draws=drawn, out=out32.clone(), out64=out64.clone(), err32=rel_err(out32, out64))


def analytic_denoiser(x: dict, y: dict, sigma: dict, *_):
    """A closed-form stand-in for the network, smooth in y and sigma: the EDM blend of tanh(c_in y + the last input step), evaluated in y's
    dtype.  tests/transport_refs.py restates it."""
    out = {}
    for ds, yd in y.items():
        s = sigma[ds].to(yd.dtype)
        t = s**2 + 1.0
        out[ds] = yd / t + s / t.sqrt() * torch.tanh(yd / t.sqrt() + x[ds][:, -1:].to(yd.dtype))
    return out


def gen_analytic(name: str, spec: dict, index: int) -> dict:
    """The reference's SAMPLER CLASSES alone, around ``analytic_denoiser``: the denoiser in fp32 (solver in float64, as in the model's
    sample) and everything in float64, on the same draws.  Checkable without a network: the CPU tests pin the restated samplers to it."""
    from anemoi.models.samplers.transport_samplers import DIFFUSION_SAMPLERS
    from anemoi.models.transport.schedules import SIGMA_SCHEDULES

    gen = torch.Generator().manual_seed(11000 + index)
    x = torch.randn(2, N_STEP_IN, 1, 37, 3, generator=gen)
    sched, samp = dict(spec["schedule"]), dict(spec["sampler"])
    sigmas = SIGMA_SCHEDULES[sched.pop("schedule_type")](**sched).get_schedule(None, torch.float64)
    y0 = torch.randn(2, 1, 1, 37, 3, generator=gen, dtype=torch.float64) * sigmas[0]
    sampler = DIFFUSION_SAMPLERS[samp.pop("sampler")](dtype=torch.float64, **samp)
    real_randn, drawn = torch.randn, []

    def recording(*a, **kw):
        t = real_randn(*a, **kw)
        drawn.append(t.clone())
        return t

    def replaying(shape, *a, dtype=None, device=None, **kw):
        return queue.pop(0).to(dtype=dtype)

    torch.manual_seed(12000 + index)
    try:
        torch.randn = recording
        out32 = sampler.sample({"data": x}, {"data": y0.clone()}, sigmas, analytic_denoiser)["data"]
        queue = [t.clone() for t in drawn]
        torch.randn = replaying
        out64 = sampler.sample({"data": x.double()}, {"data": y0.clone()}, sigmas, analytic_denoiser)["data"]
    finally:
        torch.randn = real_randn
    print("analytic", name, "draws", len(drawn), "err32", rel_err(out32, out64))
    return dict(spec=spec, input_seed=11000 + index, draws=drawn, sigmas=sigmas.clone(), out=out32.clone(), out64=out64.clone(),
                err32=rel_err(out32, out64))


def gen_schedules() -> dict:
    from anemoi.models.transport.schedules import SIGMA_SCHEDULES

    out = {}
    for kind, cls in SIGMA_SCHEDULES.items():
        for n in (1, 4):
            kw = dict(sigma_max=100.0, sigma_min=0.02, num_steps=n)
            out[(kind, n)] = dict(kwargs=kw, values=cls(**kw).get_schedule(None, torch.float64).clone())
    return out


def gen_embedders() -> dict:
    from anemoi.models.layers import diffusion

    sig = torch.tensor(SIGMAS, dtype=torch.float32).view(-1, 1)
    out = {}
    for cls, kw in (("SinusoidalEmbeddings", dict(num_channels=32, max_period=1000)), ("RandomFourierEmbeddings", dict(num_channels=32, scale=16))):
        torch.manual_seed(77)
        emb = getattr(diffusion, cls)(**kw)
        out[cls] = dict(kwargs=kw, buffers={k: v.clone() for k, v in emb.state_dict().items()}, sigma=sig.clone(), out=emb(sig).clone())
    return out


def main() -> None:
    obj = {"schedules": gen_schedules(), "embedders": gen_embedders(), "models": {}, "samplers": {}, "n_step_input": N_STEP_IN}
    for i, (name, case) in enumerate(MODEL_CASES.items()):
        obj["models"][name] = gen_model(name, case, i)
    for model_name in SAMPLED_MODELS:
        for name, spec in SAMPLER_CASES.items():
            obj["samplers"][f"{model_name}/{name}"] = gen_sampler(model_name, list(MODEL_CASES).index(model_name), name, spec)
    obj["analytic"] = {name: gen_analytic(name, spec, i) for i, (name, spec) in enumerate(SAMPLER_CASES.items())}
    model, x, y, sigma, _ = build(MODEL_CASES["sin_b1"], 0, batch=2, members=2)
    try:
        with torch.no_grad():
            model({"data": x}, {"data": y}, {"data": sigma})
        error = None
    except Exception as e:  # noqa: BLE001
        error = f"{type(e).__name__}: {' '.join(str(e).split())}"
    print("batch 2 x ensemble 2 ->", error)
    obj["notes"] = {"ensemble": "the reference's forward at batch 2 x ensemble 2 raises (hidden attributes built for batch_size rows, "
                                f"transport_encoder_processor_decoder.py:291): {error}"}
    path = os.path.join(HERE, "transport.pt")
    torch.save(obj, path)
    print(f"transport.pt: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
