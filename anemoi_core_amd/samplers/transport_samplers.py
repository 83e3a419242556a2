"""EDM diffusion samplers - mirror of the reference's ``anemoi.models.samplers.transport_samplers`` (EDMHeunSampler :85-212,
DPMpp2MSampler :215-285, DIFFUSION_SAMPLERS): same constructor keywords, same ``sample(x, y, sigmas, denoising_fn, model_comm_group,
grid_shard_sizes, **kwargs)``.

What differs is where the arithmetic runs.  The reference's step is a dozen element-wise torch passes over the [batch, time, ensemble,
grid, vars] state in the solver dtype and reads device scalars on the host (``if sigma_next != 0``); here a step is ONE launch of
``ops.edm_update_`` per dataset, whose coefficients are eight fp64 values in device memory, and the control flow comes from the host
copy of the schedule (transport/schedules.py).  Between two steps only those eight values and the sigma vector change - by
stream-ordered copies from pinned host memory - so with ``graphed=True`` each kind of step (denoiser call + update) is captured once
with ``torch.cuda.graph`` and replayed for every later step of its kind.  A kind's first occurrence runs eagerly (it builds whatever the
denoiser caches), its second is captured; the one-off kinds (a final step, DPM++'s first-order step) are never captured.  The churn
add stays outside the captured part.

``denoising_fn`` is called as in the reference.  One that sets ``solver_native = True`` (the model's own, transport/objectives.py)
receives the solver state and sigma in the solver dtype, uncast, and returns the denoised state in the solver dtype: the casts happen
inside the model-edge kernels.  Any other callable gets the reference's casts, as torch operations.

``sigmas_host`` (keyword of ``sample``): the schedule as a host tensor, from which control flow and coefficients are taken; without it
the device ``sigmas`` is copied to the host once, at the start.  DPM++ 2M leaves every update in the data dtype, as the reference does
(transport_samplers.py:283): for fp32 data the rounding is the update kernel's (its eighth coefficient), so the state buffer stays in
the solver dtype and holds data-dtype values.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import Tensor

from .. import ops
from ..distributed.shapes import comm_size

_LOG_EPS = 1e-10  # transport_samplers.py:261-262


class _Steps:
    """Runs the kinds of step of one ``sample`` call: eagerly, or (graphed) eagerly once, then captured once and replayed."""

    def __init__(self, graphed: bool) -> None:
        self.graphed, self.seen, self.graphs = graphed, set(), {}

    def run(self, kind: str, fn: Callable[[], None], capture: bool = True) -> None:
        if not (self.graphed and capture) or kind not in self.seen:
            self.seen.add(kind)
            fn()
            return
        graph = self.graphs.get(kind)
        if graph is None:
            graph = self.graphs[kind] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
        graph.replay()


class EDMDiffusionSampler:
    """Base class of the EDM samplers: the static buffers of one ``sample`` call and the denoiser call on them."""

    dtype: torch.dtype = torch.float64
    graphed: bool = False

    def sample(self, x: dict, y: dict, sigmas: Tensor, denoising_fn: Callable, model_comm_group=None, grid_shard_sizes: Optional[dict] = None,
               **kwargs) -> dict:
        raise NotImplementedError

    @staticmethod
    def _check(x: dict, y: dict, model_comm_group, grid_shard_sizes) -> None:
        if (model_comm_group is not None and comm_size(model_comm_group) > 1) or (
                grid_shard_sizes is not None and any(v is not None for v in grid_shard_sizes.values())):
            raise NotImplementedError("EDM samplers: a sharded model or grid (model_comm_group of more than one rank, grid_shard_sizes) is "
                                      "not implemented")
        for ds, t in y.items():
            if t.dim() != 5 or (t.shape[0], t.shape[2]) != (x[ds].shape[0], x[ds].shape[2]):
                raise ValueError(f"EDM samplers: y['{ds}'] {tuple(t.shape)} is not [batch, time, ensemble, grid, vars] over x's batch and ensemble")

    @staticmethod
    def _host(sigmas: Tensor, kwargs: dict) -> Tensor:
        host = kwargs.get("sigmas_host")
        return sigmas.detach().cpu() if host is None else host

    def _begin(self, y: dict, dtype: torch.dtype, n_uploads: int):
        """(state, sigma vector, parameter block, pinned staging rows) of one call.  The state is a private contiguous copy of y in the
        solver dtype; sigma [batch ensemble] (solver dtype) and params [8] (fp64) live on the device and are rewritten between steps."""
        first = next(iter(y.values()))
        groups, device = first.shape[0] * first.shape[2], first.device
        state = {ds: t.to(dtype=dtype, copy=True).contiguous() for ds, t in y.items()}
        sigma = torch.zeros(groups, dtype=dtype, device=device)
        params = torch.zeros(8, dtype=torch.float64, device=device)
        pin = device.type == "cuda"
        stage_sigma = torch.zeros((n_uploads, groups), dtype=dtype, pin_memory=pin)
        stage_params = torch.zeros((n_uploads, 8), dtype=torch.float64, pin_memory=pin)
        return state, sigma, params, stage_sigma, stage_params

    def _denoise(self, fn: Callable, x: dict, ys: dict, sigma: Tensor, dtype: torch.dtype, group, shards) -> dict:
        """denoising_fn on the static buffers -> {dataset: contiguous denoised state in the solver dtype}."""
        native = getattr(fn, "solver_native", False)
        cond, y_in = {}, {}
        for ds, t in ys.items():
            c = sigma.view(t.shape[0], 1, t.shape[2], 1, 1)
            y_in[ds] = t if native else t.to(x[ds].dtype)
            cond[ds] = c if native else c.to(x[ds].dtype)
        out = fn(x, y_in, cond, group, shards)
        return {ds: d.to(dtype).contiguous() for ds, d in out.items()}


class EDMHeunSampler(EDMDiffusionSampler):
    """EDM Heun sampler with stochastic churn (Karras et al.)."""

    def __init__(self, S_churn: float = 0.0, S_min: float = 0.0, S_max: float = float("inf"), S_noise: float = 1.0,
                 dtype: torch.dtype = torch.float64, eps_prec: float = 1e-10, graphed: bool = False):
        self.S_churn, self.S_min, self.S_max, self.S_noise = S_churn, S_min, S_max, S_noise
        self.dtype, self.eps_prec, self.graphed = dtype, eps_prec, graphed

    def draw(self, shape, dtype, device) -> Tensor:
        """The churn noise of one dataset and step (the single place this sampler's random numbers come from)."""
        return torch.randn(shape, device=device, dtype=dtype)

    def sample(self, x: dict, y: dict, sigmas: Tensor, denoising_fn: Callable, model_comm_group=None, grid_shard_sizes: Optional[dict] = None,
               **kwargs) -> dict:
        S_churn, S_min, S_max = kwargs.get("S_churn", self.S_churn), kwargs.get("S_min", self.S_min), kwargs.get("S_max", self.S_max)
        S_noise, dtype, eps = kwargs.get("S_noise", self.S_noise), kwargs.get("dtype", self.dtype), kwargs.get("eps_prec", self.eps_prec)
        self._check(x, y, model_comm_group, grid_shard_sizes)
        host = self._host(sigmas, kwargs).to(dtype)  # (host: every scalar below is a 0-d CPU tensor in the solver dtype)
        num_steps = len(host) - 1
        state, sigma, params, stage_sigma, stage_params = self._begin(y, dtype, 2 * num_steps)
        d1 = {ds: torch.empty_like(t) for ds, t in state.items()}
        y_next = {ds: torch.empty_like(t) for ds, t in state.items()}
        steps = self.last_steps = _Steps(kwargs.get("graphed", self.graphed))

        def stage(mode: int, source: dict):
            def run() -> None:
                D = self._denoise(denoising_fn, x, source, sigma, dtype, model_comm_group, grid_shard_sizes)
                for ds in state:
                    ops.edm_update_(mode, params, state[ds], D[ds], d1[ds], y_next[ds])
            return run

        predict, correct, final = stage(ops.HEUN_PREDICT, state), stage(ops.HEUN_CORRECT, y_next), stage(ops.HEUN_FINAL, state)
        for i in range(num_steps):
            sigma_i, sigma_next = host[i], host[i + 1]
            sigma_eff = sigma_i
            if bool(S_min <= sigma_i <= S_max) and S_churn > 0.0:
                gamma = min(S_churn / num_steps, torch.sqrt(torch.tensor(2.0, dtype=dtype)) - 1)
                sigma_eff = sigma_i + gamma * sigma_i
                scale = torch.sqrt(sigma_eff**2 - sigma_i**2).item()
                for ds, t in state.items():
                    t.add_(self.draw(tuple(t.shape), dtype, t.device) * S_noise, alpha=scale)
            stage_params[2 * i, 0], stage_params[2 * i, 1], stage_params[2 * i, 2] = sigma_eff.item(), sigma_next.item(), eps
            stage_sigma[2 * i].fill_(sigma_eff.item())
            params.copy_(stage_params[2 * i], non_blocking=True)
            sigma.copy_(stage_sigma[2 * i], non_blocking=True)
            if sigma_next.item() == 0:
                steps.run("final", final, capture=False)
                continue
            steps.run("predict", predict)
            stage_sigma[2 * i + 1].fill_(sigma_next.item())
            sigma.copy_(stage_sigma[2 * i + 1], non_blocking=True)
            steps.run("correct", correct)
        return {ds: t.to(x[ds].dtype) for ds, t in state.items()}


class DPMpp2MSampler(EDMDiffusionSampler):
    """DPM++ 2M sampler (DPM-Solver++, second-order multistep)."""

    def __init__(self, dtype: torch.dtype = torch.float64, graphed: bool = False):
        self.dtype, self.graphed = dtype, graphed

    def sample(self, x: dict, y: dict, sigmas: Tensor, denoising_fn: Callable, model_comm_group=None, grid_shard_sizes: Optional[dict] = None,
               **kwargs) -> dict:
        dtype = kwargs.get("dtype", self.dtype)
        self._check(x, y, model_comm_group, grid_shard_sizes)
        host = self._host(sigmas, kwargs).to(dtype)
        num_steps = len(host) - 1
        # (the reference hands the denoiser y in the data dtype from the first step on: the state starts from those values)
        state, sigma, params, stage_sigma, stage_params = self._begin({ds: t.to(x[ds].dtype) for ds, t in y.items()}, dtype, num_steps)
        old = {ds: torch.empty_like(t) for ds, t in state.items()}
        steps = self.last_steps = _Steps(kwargs.get("graphed", self.graphed))
        # y leaves every update in the data dtype (:283): fp32 data is rounded by the kernel, any other data dtype by a cast pair behind it
        kernel_rounds = all(x[ds].dtype == torch.float32 for ds in state) and dtype == torch.float64
        stage_params[:, 7] = 1.0 if kernel_rounds else 0.0

        def stage(mode: int):
            def run() -> None:
                D = self._denoise(denoising_fn, x, state, sigma, dtype, model_comm_group, grid_shard_sizes)
                for ds in state:
                    ops.edm_update_(mode, params, state[ds], D[ds], old[ds], None)
                    if not kernel_rounds and x[ds].dtype != dtype and mode != ops.DPMPP_FINAL:
                        state[ds].copy_(state[ds].to(x[ds].dtype))
            return run

        first, multi, final = stage(ops.DPMPP_FIRST), stage(ops.DPMPP_MULTI), stage(ops.DPMPP_FINAL)
        for i in range(num_steps):
            s, s_next = host[i], host[i + 1]
            stage_sigma[i].fill_(s.item())
            sigma.copy_(stage_sigma[i], non_blocking=True)
            if s_next.item() == 0:
                steps.run("final", final, capture=False)
                break
            t, t_next = -torch.log(s + _LOG_EPS), -torch.log(s_next + _LOG_EPS)
            h = t_next - t
            stage_params[i, 3], stage_params[i, 4] = (s_next / s).item(), (torch.exp(-h) - 1).item()
            if i > 0:
                r = (t - (-torch.log(host[i - 1] + _LOG_EPS))) / h
                stage_params[i, 5], stage_params[i, 6] = (1 + 1 / (2 * r)).item(), (-1 / (2 * r)).item()
            params.copy_(stage_params[i], non_blocking=True)
            if i == 0:
                steps.run("first", first, capture=False)
            else:
                steps.run("multi", multi)
        return {ds: t.to(x[ds].dtype) for ds, t in state.items()}


DIFFUSION_SAMPLERS = {"heun": EDMHeunSampler, "dpmpp_2m": DPMpp2MSampler}
