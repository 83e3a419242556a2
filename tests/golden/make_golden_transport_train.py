"""Generate tests/golden/transport_train.pt (and its gradient parts) by IMPORTING the Python reference: one EDM training step of
AnemoiTransportModelEncProcDec on the CPU - the sigma distributions (transport/schedules.py), the loss weight (transport/paths.py), the
source field (transport/sources.py), the model's forward under autograd and torch's backward - in fp32 and in float64.

The steps of the reference's training objective (training/train/methods/edm_diffusion.py: ``prepare``) are called one by one on its own
functions; the training package itself needs pytorch_lightning, which is not installed where this runs.

As in make_golden_transport.py (which stays as it is, and whose ``build`` draws the model here too), parameters and inputs are not
stored: they are drawn from seeded CPU generators, which the tests repeat (tests/transport_train_refs.py).  Per model case the fixture
holds the seeds; what ``prepare`` computes from a recorded ``torch.rand`` / ``torch.randn`` draw (sigma from the case's
``training_condition``, the source, y_noised, the weights); then, for the case's FIXED sigmas and the same source: y_noised, the weights,
the loss mean(w (D - target)^2) in fp32 and float64, the float64 gradient of every parameter (stored rounded to fp32), per parameter
``err32 = max|g32 - g64| / max|g64|`` of the reference's own fp32 backward, the float64 gradient with respect to the network's output rows
"(batch ensemble grid) (time vars)" (every 16th row) and with respect to the per-group conditioning vector [G, cond_dim], and the float64
network output rows and denoised state themselves (what the loss gradient is taken at).  ``distributions``
holds what each of the four training distributions draws from a fixed seed, in fp32 and float64.

No committed file may exceed 1 MiB and one case's gradients are 1.2 MB: the gradients of the first case go to the part files
``transport_train_grads_<i>.pt`` ({"case/parameter": tensor}), the second case keeps the gradients of the noise MLP, the node attributes,
the embeddings, the extractor and the ConditionalLayerNorm parameters (``err32`` is kept for every parameter of both).

Usage:  python tests/golden/make_golden_transport_train.py
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_transport as T  # noqa: E402  (installs the stand-ins; build(): the reference's model of a case, filled)

CASES = {
    "sin_b2": (dict(T.MODEL_CASES["sin_b2"]), list(T.MODEL_CASES).index("sin_b2")),  # the same model and x as transport.pt's case
    "rff_b2_2out_forcing": (dict(batch=2, embedder="RandomFourierEmbeddings", n_step_output=2, n_vars_in=6, n_vars_out=4, sigma=[0.05, 6.0]), 20),
}
TRAINING_CONDITION = {"sin_b2": dict(distribution="karras", sigma_max=100.0, sigma_min=0.02, rho=7.0),
                      "rff_b2_2out_forcing": dict(distribution="exponential", sigma_max=80.0, sigma_min=0.05)}
FULL_GRADS = ("sin_b2",)  # every parameter's gradient is kept (in the part files)
KEPT = ("noise_cond_mlp.", "node_attributes.", "emb_nodes", "node_data_extractor", "layer_norm")  # the other cases keep these
ROW_STEP = 16
PART_BYTES = 900 * 1024
DIST_SEED, DIST_SHAPE = 4242, {"a": (3, 2, 2, 7, 5), "b": (3, 1, 2, 9, 4)}
DIST_KW = {"karras": dict(sigma_max=100.0, sigma_min=0.02, rho=7.0), "linear": dict(sigma_max=100.0, sigma_min=0.02),
           "cosine": dict(sigma_max=100.0, sigma_min=0.02, s=0.008), "exponential": dict(sigma_max=100.0, sigma_min=0.02)}


class Recorder:
    """While active, torch.rand / torch.randn hand out fresh draws and keep a copy of each."""

    def __enter__(self):
        self.rand, self.randn, self._real = [], [], (torch.rand, torch.randn)
        torch.rand = lambda *a, **kw: self._keep(self.rand, self._real[0](*a, **kw))
        torch.randn = lambda *a, **kw: self._keep(self.randn, self._real[1](*a, **kw))
        return self

    @staticmethod
    def _keep(where, t):
        where.append(t.clone())
        return t

    def __exit__(self, *exc):
        torch.rand, torch.randn = self._real


def step(model, x, y_noised, sigma, weights, target):
    """One training step: (loss, {parameter: gradient}, d loss / d network output rows, d loss / d conditioning vector, the network's output
    rows, the denoised state D)."""
    kept = {}
    real_net = model._forward_transport_network

    def net(*a, **kw):
        out = real_net(*a, **kw)
        out["data"].retain_grad()
        kept["pred"] = out["data"]
        return out

    def keep_cond(_m, _i, out):
        out.retain_grad()
        kept["cond"] = out

    hook = model.noise_cond_mlp.register_forward_hook(keep_cond)
    model._forward_transport_network = net
    try:
        model.zero_grad(set_to_none=True)
        D = model({"data": x}, {"data": y_noised}, {"data": sigma})["data"]
        loss = (weights * (D - target) ** 2).mean()
        loss.backward()
    finally:
        hook.remove()
        del model._forward_transport_network
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    B, Tn, E, N, V = kept["pred"].shape
    d_pred = kept["pred"].grad.permute(0, 2, 3, 1, 4).reshape(B * E * N, Tn * V)  # "(batch ensemble grid) (time vars)"
    rows = lambda t: t.detach().permute(0, 2, 3, 1, 4).reshape(B * E * N, Tn * V).clone()  # noqa: E731
    return loss.detach().clone(), grads, d_pred.clone(), kept["cond"].grad.reshape(B * E, -1).clone(), rows(kept["pred"]), D.detach().clone()


def gen_case(name: str, case: dict, index: int):
    from anemoi.models.transport import TransportSourceRequest
    from anemoi.models.transport.paths import edm_loss_weight
    from anemoi.models.transport.schedules import SIGMA_TRAINING_DISTRIBUTIONS

    model, x, _, sigma, built = T.build(case, index)
    model.training_condition = dict(TRAINING_CONDITION[name])
    target_seed, noise_seed = 9500 + index, 9700 + index
    target = torch.randn(x.shape[0], case.get("n_step_output", 1), 1, x.shape[3], case.get("n_vars_out", 4),
                         generator=torch.Generator().manual_seed(target_seed))
    # -- prepare, step by step as the reference's objective takes them: sigma, the weights, the source, the noised target
    torch.manual_seed(noise_seed)
    with Recorder() as rec:
        config = dict(model.training_condition)
        dist = SIGMA_TRAINING_DISTRIBUTIONS[config.pop("distribution")](**config)
        sigma_drawn = dist.sample({"data": target.shape}, device=target.device)["data"]
        weights_drawn = edm_loss_weight(sigma_drawn, model.edm.sigma_data)
        source = model.transport_source.build(TransportSourceRequest.from_tensors({"data": target}, default_kind="gaussian", error_context="training"))["data"]
        noised_drawn = target + source * sigma_drawn
    assert len(rec.rand) == 1 and len(rec.randn) == 1 and torch.equal(rec.randn[0], source)
    prepare = dict(rand=rec.rand[0], randn=rec.randn[0], sigma=sigma_drawn.clone(), weights=weights_drawn.clone(), y_noised=noised_drawn.clone())
    # -- the step at the case's fixed sigmas, same source
    weights = edm_loss_weight(sigma, model.edm.sigma_data)
    y_noised = target + source * sigma
    loss32, g32, *_ = step(model, x, y_noised, sigma, weights, target)
    model.double()
    loss64, g64, d_pred64, d_cond64, pred64, out64 = step(model, x.double(), y_noised.double(), sigma.double(), weights.double(), target.double())
    err32, zero, grads = {}, [], {}
    for k, g in g64.items():
        if g is None or float(g.abs().max()) == 0.0:
            zero.append(k)
            assert g32[k] is None or float(g32[k].abs().max()) == 0.0, k
            continue
        err32[k] = float((g32[k].double() - g).abs().max() / g.abs().max())
        if name in FULL_GRADS or any(s in k for s in KEPT):
            grads[k] = g.float()
    print(name, "loss", float(loss32), float(loss64), "parameters", len(g64), "zero", zero, "kept", len(grads), "err32 max", max(err32.values()))
    rec_ = dict(built, training_condition=dict(model.training_condition), target_seed=target_seed, noise_seed=noise_seed, prepare=prepare,
                sigma=sigma.clone(), y_noised=y_noised.clone(), weights=weights.clone(), loss32=loss32, loss64=loss64, err32=err32, zero_grads=zero,
                grad_keys=sorted(grads), d_pred64=d_pred64[::ROW_STEP].clone(), row_step=ROW_STEP, d_cond64=d_cond64,
                pred64=pred64, out64=out64)
    return rec_, grads


def gen_distributions() -> dict:
    from anemoi.models.transport.schedules import SIGMA_TRAINING_DISTRIBUTIONS

    out = {"seed": DIST_SEED, "shape": DIST_SHAPE, "kwargs": DIST_KW, "draws": {}}
    for kind, cls in SIGMA_TRAINING_DISTRIBUTIONS.items():
        for dtype in (torch.float32, torch.float64):
            torch.manual_seed(DIST_SEED)
            with Recorder() as rec:
                sig = cls(**DIST_KW[kind]).sample(DIST_SHAPE, device=torch.device("cpu"), dtype=dtype)
            assert sig["a"] is sig["b"]
            out["draws"][(kind, dtype)] = dict(rand=rec.rand[0], sigma=sig["a"].clone())
    return out


def main() -> None:
    obj = {"n_step_input": T.N_STEP_IN, "models": {}, "distributions": gen_distributions(), "parts": []}
    parts, size = [{}], 0
    for name, (case, index) in CASES.items():
        rec, grads = gen_case(name, case, index)
        if name in FULL_GRADS:
            for k, g in grads.items():
                if size + g.numel() * 4 > PART_BYTES:
                    parts.append({})
                    size = 0
                parts[-1][f"{name}/{k}"] = g
                size += g.numel() * 4
        else:
            rec["grads"] = grads
        obj["models"][name] = rec
    for i, part in enumerate(parts):
        obj["parts"].append(f"transport_train_grads_{i}.pt")
        torch.save(part, os.path.join(HERE, obj["parts"][-1]))
    path = os.path.join(HERE, "transport_train.pt")
    torch.save(obj, path)
    for f in ["transport_train.pt", *obj["parts"]]:
        kib = os.path.getsize(os.path.join(HERE, f)) / 1024
        print(f"{f}: {kib:.0f} KiB")
        assert kib < 1024, f


if __name__ == "__main__":
    main()
