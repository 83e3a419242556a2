"""How a transport model runs its forward pass and its inference sampler - mirror of the reference's
``anemoi.models.transport.objectives`` for the EDM diffusion objective (EDMDiffusionModelObjective :102-219).

The reference's forward computes the four EDM factors as tensors, scales the noised target, runs the network and blends its output -
about ten element-wise launches around the network.  Here the factors never exist as tensors: ``c_noise`` is the transform flag of the
noise-conditioning kernel, ``c_in`` is applied where the network's input rows are assembled, ``c_skip`` / ``c_out`` where its output rows
are rearranged (``AnemoiTransportModelEncProcDec._forward_transport_network(..., edm=...)``), each from sigma in device memory."""
from __future__ import annotations

from typing import Any, Optional

import torch


def _inference_config(model: Any, section: str, overrides: Optional[dict]) -> dict:
    defaults = model.inference_defaults.get(section) if model.inference_defaults is not None else None
    config = dict(defaults) if defaults is not None else {}
    config.update(overrides or {})
    return config


def _registry_entry(config: dict, selector: str, registry: dict, context: str):
    if selector not in config:
        raise ValueError(f"{context} must define '{selector}'.")
    name = config.pop(selector)
    if name not in registry:
        raise ValueError(f"Unknown {context}: {name}")
    return registry[name]


class TransportModelObjective:
    """Interface: ``forward(model, x, conditioned_target, condition, ...)`` and ``sample(model, x, ...)``."""

    def forward(self, model: Any, x: dict, conditioned_target: dict, condition: dict, model_comm_group=None, grid_shard_sizes=None, **kwargs) -> dict:
        raise NotImplementedError

    def sample(self, model: Any, x: dict, model_comm_group=None, grid_shard_sizes=None, schedule_params: Optional[dict] = None,
               sampler_params: Optional[dict] = None, **kwargs) -> dict:
        raise NotImplementedError


class EDMDiffusionModelObjective(TransportModelObjective):
    """EDM diffusion: D(y; sigma) = c_skip y + c_out F(c_in y; log(sigma) / 4)."""

    def forward(self, model: Any, x: dict, y_noised: dict, sigma: dict, model_comm_group=None, grid_shard_sizes=None, **kwargs) -> dict:
        return model._forward_transport_network(x, y_noised, sigma, model_comm_group=model_comm_group, grid_shard_sizes=grid_shard_sizes,
                                                edm=model.edm, **kwargs)

    def sample(self, model: Any, x: dict, model_comm_group=None, grid_shard_sizes=None, schedule_params: Optional[dict] = None,
               sampler_params: Optional[dict] = None, **kwargs) -> dict:
        from ..samplers import transport_samplers
        from .schedules import SIGMA_SCHEDULES

        device = next(iter(x.values())).device
        source = model.build_sampling_source(x, model_comm_group=model_comm_group, grid_shard_sizes=grid_shard_sizes)
        schedule_config = _inference_config(model, "sampling_schedule", schedule_params)
        schedule = _registry_entry(schedule_config, "schedule_type", SIGMA_SCHEDULES, "EDM sampling schedule")(**schedule_config)
        sigmas_host = schedule.get_host_schedule(torch.float64)  # computed once on the host; the sampler's control flow reads this copy
        sigmas = sigmas_host.to(device)
        y_init = {ds: source[ds].to(dtype=sigmas.dtype) * sigmas[0] for ds in x}
        sampler_config = _inference_config(model, "sampler", sampler_params)
        sampler = _registry_entry(sampler_config, "sampler", transport_samplers.DIFFUSION_SAMPLERS, "EDM sampler")(dtype=sigmas.dtype,
                                                                                                                   **sampler_config)

        def denoising_fn(x_arg: dict, y_arg: dict, sigma_arg: dict, comm_arg=None, shard_sizes_arg=None) -> dict:
            # the solver's state and sigma come in uncast and the denoised state goes out in the solver dtype: the casts of the
            # reference's sampler happen inside the model-edge kernels
            return model._forward_transport_network(x_arg, y_arg, sigma_arg, model_comm_group=comm_arg, grid_shard_sizes=shard_sizes_arg,
                                                    edm=model.edm, out_dtype=next(iter(y_arg.values())).dtype)

        denoising_fn.solver_native = True
        return sampler.sample(x, y_init, sigmas, denoising_fn, model_comm_group, grid_shard_sizes=grid_shard_sizes, sigmas_host=sigmas_host)


TRANSPORT_MODEL_OBJECTIVES = {"edm_diffusion": EDMDiffusionModelObjective}


def get_transport_model_objective(name: str) -> TransportModelObjective:
    if name == "stochastic_interpolant":
        raise NotImplementedError("transport objective 'stochastic_interpolant' (the bridge objective and its vector-field samplers) is not "
                                  "implemented; supported: 'edm_diffusion'")
    try:
        return TRANSPORT_MODEL_OBJECTIVES[name]()
    except KeyError as exc:
        raise ValueError(f"Unknown transport model objective: {name}") from exc
