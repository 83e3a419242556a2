"""Sigma schedules of the EDM samplers and the sigma distributions EDM training draws from - mirror of the reference's ``anemoi.models.transport.schedules`` (KarrasSigmaSchedule,
LinearSigmaSchedule, CosineSigmaSchedule, ExponentialSigmaSchedule, SIGMA_SCHEDULES; SIGMA_TRAINING_DISTRIBUTIONS and the ``*_sigma_from_unit_time`` maps) with its validation and the exact final zero.

A schedule is a handful of numbers: ``get_host_schedule`` computes it in float64 on the HOST, ``get_schedule(device)`` is that tensor
uploaded.  The samplers take their control flow (``sigma_next == 0``, the churn window) and their per-step coefficients from the host
tensor, which the caller hands them explicitly (``sample(..., sigmas_host=...)``, as the model's objective does), so no step reads a
device scalar back; a caller that passes the device tensor alone pays one device-to-host copy at the start of ``sample``."""
from __future__ import annotations

import math

import torch
from torch import Tensor

from .paths import karras_sigma_from_unit_time

DEFAULT_FINAL_SIGMA_EPS = 1e-10  # tolerance for a schedule that provides its final value itself


class SigmaSchedule:
    """Base class: ``num_steps`` strictly positive sigmas from sigma_max down to sigma_min, followed by an exact zero."""

    def __init__(self, sigma_max: float, sigma_min: float, num_steps: int) -> None:
        self._validate_sigma_parameters(sigma_max=sigma_max, sigma_min=sigma_min)
        self.sigma_max, self.sigma_min = float(sigma_max), float(sigma_min)
        if int(num_steps) < 1:
            raise ValueError("num_steps must be at least 1.")
        self.num_steps = int(num_steps)

    @staticmethod
    def _validate_sigma_parameters(sigma_max: float, sigma_min: float) -> None:
        if sigma_min <= 0:
            raise ValueError("sigma_min must be strictly positive; the final zero is added separately.")
        if sigma_max <= 0:
            raise ValueError("sigma_max must be strictly positive.")
        if sigma_max < sigma_min:
            raise ValueError("sigma_max must be greater than or equal to sigma_min.")

    def _build_schedule(self, dtype_compute: torch.dtype) -> Tensor:  # host tensor
        raise NotImplementedError

    def _validate_schedule(self, values: Tensor) -> None:
        if values.ndim != 1:
            raise ValueError(f"Sampling schedule must be 1D, got shape {tuple(values.shape)}.")
        if values.numel() == 0:
            raise ValueError("Sampling schedule must contain at least one value.")
        if not torch.isfinite(values).all():
            raise ValueError("Sampling schedule must contain only finite values.")
        if values.numel() == self.num_steps + 1:
            last = values[-1].item()
            if last < 0 or last > DEFAULT_FINAL_SIGMA_EPS:
                raise ValueError("Sigma schedule with an explicit final value must end at zero.")

    def _finalize_schedule(self, values: Tensor) -> Tensor:
        if values.numel() == self.num_steps + 1:
            if values[-1].item() != 0.0:
                values = values.clone()
                values[-1] = 0.0
            return values
        if values.numel() != self.num_steps:
            raise ValueError(f"Sigma schedule must contain {self.num_steps} values before the final zero, "
                             f"or {self.num_steps + 1} including it; got {values.numel()}.")
        return torch.cat((values, values.new_zeros(1)))

    def get_host_schedule(self, dtype_compute: torch.dtype = torch.float64) -> Tensor:
        """The schedule as a host tensor: num_steps + 1 values, the last an exact zero."""
        values = self._build_schedule(dtype_compute)
        self._validate_schedule(values)
        return self._finalize_schedule(values)

    def get_schedule(self, device=None, dtype_compute: torch.dtype = torch.float64) -> Tensor:
        host = self.get_host_schedule(dtype_compute)
        return host if device is None else host.to(device)


class KarrasSigmaSchedule(SigmaSchedule):
    """Karras et al.: linear in sigma^(1 / rho)."""

    def __init__(self, sigma_max: float, sigma_min: float, num_steps: int, rho: float = 7.0) -> None:
        super().__init__(sigma_max=sigma_max, sigma_min=sigma_min, num_steps=num_steps)
        self.rho = float(rho)

    def _build_schedule(self, dtype_compute: torch.dtype) -> Tensor:
        if self.num_steps == 1:
            return torch.tensor([self.sigma_max], dtype=dtype_compute)
        t = torch.arange(self.num_steps, dtype=dtype_compute) / (self.num_steps - 1.0)
        hi, lo = self.sigma_max ** (1.0 / self.rho), self.sigma_min ** (1.0 / self.rho)
        return (hi + t * (lo - hi)) ** self.rho


class LinearSigmaSchedule(SigmaSchedule):
    """Linear in sigma."""

    def _build_schedule(self, dtype_compute: torch.dtype) -> Tensor:
        return torch.linspace(self.sigma_max, self.sigma_min, self.num_steps, dtype=dtype_compute)


class CosineSigmaSchedule(SigmaSchedule):
    """The cosine alpha-bar path expressed as sigma = sqrt((1 - alpha_bar) / alpha_bar)."""

    def __init__(self, sigma_max: float, sigma_min: float, num_steps: int, s: float = 0.008) -> None:
        super().__init__(sigma_max=sigma_max, sigma_min=sigma_min, num_steps=num_steps)
        self.s = float(s)

    def _build_schedule(self, dtype_compute: torch.dtype) -> Tensor:
        unit = torch.linspace(0.0, 1.0, self.num_steps, dtype=dtype_compute)
        s = self.s
        t_max = (2 * math.atan(self.sigma_max) / math.pi) * (1 + s) - s
        t_min = (2 * math.atan(self.sigma_min) / math.pi) * (1 + s) - s
        t = t_max + unit * (t_min - t_max)
        alpha_bar = torch.cos((t + s) / (1 + s) * torch.pi / 2) ** 2
        return torch.sqrt((1 - alpha_bar) / alpha_bar)


class ExponentialSigmaSchedule(SigmaSchedule):
    """Linear in log sigma."""

    def _build_schedule(self, dtype_compute: torch.dtype) -> Tensor:
        unit = torch.linspace(0.0, 1.0, self.num_steps, dtype=dtype_compute)
        hi, lo = math.log(self.sigma_max), math.log(self.sigma_min)
        return torch.exp(hi + unit * (lo - hi))


SIGMA_SCHEDULES = {"karras": KarrasSigmaSchedule, "linear": LinearSigmaSchedule, "cosine": CosineSigmaSchedule,
                   "exponential": ExponentialSigmaSchedule}


# ---------------------------------------------------------------------------------------------- training: one sigma per sample and member
def exponential_sigma_from_unit_time(unit_time: Tensor, *, sigma_max: float, sigma_min: float) -> Tensor:
    """Unit time -> sigma, linear in log sigma."""
    hi, lo = math.log(sigma_max), math.log(sigma_min)
    return torch.exp(hi + unit_time * (lo - hi))


def cosine_sigma_from_unit_time(unit_time: Tensor, *, sigma_max: float, sigma_min: float, s: float = 0.008) -> Tensor:
    """Unit time -> sigma along the cosine alpha-bar path."""
    t_max = (2 * math.atan(sigma_max) / math.pi) * (1 + s) - s
    t_min = (2 * math.atan(sigma_min) / math.pi) * (1 + s) - s
    t = t_max + unit_time * (t_min - t_max)
    alpha_bar = torch.cos((t + s) / (1 + s) * torch.pi / 2) ** 2
    return torch.sqrt((1 - alpha_bar) / alpha_bar)


def _validate_condition_shape(shape: dict) -> tuple:
    names = list(shape)
    if not names:
        raise ValueError("Condition distribution requires at least one dataset shape.")
    ref = shape[names[0]]
    if len(ref) != 5:
        raise ValueError("Expected 5D tensor shape (batch, time, ensemble, grid, vars) for transport conditions.")
    for name, sh in shape.items():
        if len(sh) != 5:
            raise ValueError(f"Expected 5D tensor shape for dataset '{name}'.")
        if sh[0] != ref[0] or sh[2] != ref[2]:
            raise ValueError("Batch or ensemble dimension mismatch across datasets when sampling conditions.")
    return ref[0], ref[2]


class SigmaTrainingDistribution:
    """One sigma per sample and ensemble member: ``sample`` draws one ``torch.rand((batch, ensemble))`` and maps it through
    ``_sigma_from_unit_time``; the datasets share the one resulting tensor [batch, 1, ensemble, 1, 1]."""

    def __init__(self, sigma_max: float, sigma_min: float) -> None:
        SigmaSchedule._validate_sigma_parameters(sigma_max=sigma_max, sigma_min=sigma_min)
        self.sigma_max, self.sigma_min = float(sigma_max), float(sigma_min)

    def _sigma_from_unit_time(self, unit_time: Tensor) -> Tensor:
        raise NotImplementedError

    def sample(self, shape: dict, *, device, dtype=None) -> dict:
        batch_size, ensemble_size = _validate_condition_shape(shape)
        unit_time = torch.rand((batch_size, ensemble_size), device=device, dtype=dtype)
        base = self._sigma_from_unit_time(unit_time)[:, None, :, None, None]
        return {name: base for name in shape}


class KarrasSigmaTrainingDistribution(SigmaTrainingDistribution):
    def __init__(self, sigma_max: float, sigma_min: float, rho: float = 7.0) -> None:
        super().__init__(sigma_max=sigma_max, sigma_min=sigma_min)
        self.rho = float(rho)

    def _sigma_from_unit_time(self, unit_time: Tensor) -> Tensor:
        return karras_sigma_from_unit_time(unit_time, sigma_max=self.sigma_max, sigma_min=self.sigma_min, rho=self.rho)


class LinearSigmaTrainingDistribution(SigmaTrainingDistribution):
    def _sigma_from_unit_time(self, unit_time: Tensor) -> Tensor:
        return self.sigma_max + unit_time * (self.sigma_min - self.sigma_max)


class ExponentialSigmaTrainingDistribution(SigmaTrainingDistribution):
    def _sigma_from_unit_time(self, unit_time: Tensor) -> Tensor:
        return exponential_sigma_from_unit_time(unit_time, sigma_max=self.sigma_max, sigma_min=self.sigma_min)


class CosineSigmaTrainingDistribution(SigmaTrainingDistribution):
    def __init__(self, sigma_max: float, sigma_min: float, s: float = 0.008) -> None:
        super().__init__(sigma_max=sigma_max, sigma_min=sigma_min)
        self.s = float(s)

    def _sigma_from_unit_time(self, unit_time: Tensor) -> Tensor:
        return cosine_sigma_from_unit_time(unit_time, sigma_max=self.sigma_max, sigma_min=self.sigma_min, s=self.s)


SIGMA_TRAINING_DISTRIBUTIONS = {"karras": KarrasSigmaTrainingDistribution, "linear": LinearSigmaTrainingDistribution,
                                "cosine": CosineSigmaTrainingDistribution, "exponential": ExponentialSigmaTrainingDistribution}
