"""Closed forms of the EDM noise path - mirror of the names ``anemoi.models.transport.paths`` gives them: the Karras map from unit time to
sigma and the loss weight of a noise level.  Plain torch expressions on whatever device and dtype the argument has."""
from __future__ import annotations

from torch import Tensor


def karras_sigma_from_unit_time(t: Tensor, *, sigma_max: float, sigma_min: float, rho: float) -> Tensor:
    """sigma(t) = (sigma_max^(1/rho) + t (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho for t in [0, 1]."""
    hi, lo = sigma_max ** (1.0 / rho), sigma_min ** (1.0 / rho)
    return (hi + t * (lo - hi)) ** rho


def edm_loss_weight(sigma: Tensor, sigma_data: float) -> Tensor:
    """lambda(sigma) = (sigma^2 + sigma_data^2) / (sigma sigma_data)^2: the weight under which every noise level contributes equally."""
    return (sigma**2 + sigma_data**2) / (sigma * sigma_data) ** 2
