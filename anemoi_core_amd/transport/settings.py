"""Settings of the transport (diffusion) family - mirror of the reference's ``anemoi.models.transport.settings``: frozen dataclasses read
from the ``model.model.transport`` section of the model config (a mapping or an attribute object), with the reference's names and
defaults."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any


def _value(config: Any, name: str, default: Any) -> Any:
    return config.get(name, default) if hasattr(config, "get") else getattr(config, name, default)


@dataclass(frozen=True)
class NoiseConditioningSettings:
    """Widths of the noise embedding (``noise_channels``) and of the conditioning it is mapped to (``noise_cond_dim``)."""

    channels: int = 32
    cond_dim: int = 16

    @classmethod
    def from_config(cls, config: Any) -> "NoiseConditioningSettings":
        return cls(channels=int(_value(config, "noise_channels", cls.channels)), cond_dim=int(_value(config, "noise_cond_dim", cls.cond_dim)))


@dataclass(frozen=True)
class EdmSettings:
    """The EDM objective's data scale and the range and shape of its noise schedule."""

    sigma_data: float = 1.0
    sigma_max: float = 100.0
    sigma_min: float = 0.02
    rho: float = 7.0

    @classmethod
    def from_config(cls, config: Any) -> "EdmSettings":
        return cls(**{name: float(_value(config, name, getattr(cls, name))) for name in ("sigma_data", "sigma_max", "sigma_min", "rho")})


@dataclass(frozen=True)
class TransportSourceSettings:
    """Which field sampling starts from (``kind``: default, zero, gaussian, reference_state) and how it is scaled / perturbed."""

    kind: str = "default"
    scale: float = 1.0
    noise_scale: float = 0.0

    @classmethod
    def from_config(cls, config: Any) -> "TransportSourceSettings":
        source = _value(config, "source", {})
        return cls(kind=str(_value(source, "kind", cls.kind)), scale=float(_value(source, "scale", cls.scale)),
                   noise_scale=float(_value(source, "noise_scale", cls.noise_scale)))
