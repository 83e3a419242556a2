"""The field transport sampling starts from - mirror of the reference's ``anemoi.models.transport.sources`` for the kinds this package
builds: ``zero`` and ``gaussian`` (``default`` resolves to the caller's default kind), with ``scale``.  ``reference_state`` and a
``noise_scale`` other than 0 raise.  The Gaussian field comes from ``torch.randn`` through the builder's one overridable ``draw``
method, so that a test can substitute recorded noise."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional

import torch
from torch import Tensor

from .settings import TransportSourceSettings

TRANSPORT_SOURCE_KINDS = frozenset({"zero", "gaussian", "reference_state"})


@dataclass(frozen=True)
class TransportSourceSpec:
    """Shape, device and dtype of one dataset's source tensor."""

    shape: tuple
    device: torch.device
    dtype: torch.dtype
    grid_shard_sizes: Any = None


def sampling_source_specs(x: dict, *, n_step_output: int, num_output_channels: dict, grid_shard_sizes: Optional[dict] = None) -> dict:
    """{dataset: spec of [batch, n_step_output, ensemble, grid, output variables]} from the sampling input batch."""
    return {ds: TransportSourceSpec(shape=(t.shape[0], n_step_output, t.shape[2], t.shape[-2], num_output_channels[ds]), device=t.device,
                                    dtype=t.dtype, grid_shard_sizes=grid_shard_sizes.get(ds) if grid_shard_sizes is not None else None)
            for ds, t in x.items()}


class TransportSourceBuilder:
    """Builds the source fields of a request: {dataset: spec} plus the kind to use when the settings say ``default``."""

    def __init__(self, settings: Optional[TransportSourceSettings] = None) -> None:
        self.settings = settings or TransportSourceSettings()
        if self.settings.kind not in TRANSPORT_SOURCE_KINDS | {"default"}:
            raise ValueError(f"Unknown transport source kind '{self.settings.kind}'.")

    @classmethod
    def from_config(cls, config: Any) -> "TransportSourceBuilder":
        return cls(TransportSourceSettings.from_config(config))

    @property
    def kind(self) -> str:
        return self.settings.kind

    @property
    def scale(self) -> float:
        return float(self.settings.scale)

    @property
    def noise_scale(self) -> float:
        return float(self.settings.noise_scale)

    def resolve_kind(self, default_kind: str) -> str:
        return default_kind if self.kind == "default" else self.kind

    def draw(self, shape, dtype, device) -> Tensor:
        """The Gaussian field of one dataset (the single place random numbers of a source come from)."""
        return torch.randn(shape, device=device, dtype=dtype)

    def build(self, specs: dict, default_kind: str = "gaussian", error_context: str = "transport source") -> dict:
        kind = self.resolve_kind(default_kind)
        if kind == "reference_state":
            raise NotImplementedError(f"transport source kind 'reference_state' ({error_context}): starting from the latest input state is "
                                      "not implemented; use 'gaussian' or 'zero'")
        if self.noise_scale != 0.0:
            raise NotImplementedError(f"transport source noise_scale={self.noise_scale} ({error_context}): perturbing the source is not "
                                      "implemented; use noise_scale = 0")
        if kind == "zero":
            sources = {ds: torch.zeros(s.shape, device=s.device, dtype=s.dtype) for ds, s in specs.items()}
        elif kind == "gaussian":
            for ds, s in specs.items():
                if s.grid_shard_sizes is not None:
                    raise NotImplementedError(f"transport source for the sharded grid of '{ds}' is not implemented; pass the whole grid")
            sources = {ds: self.draw(s.shape, s.dtype, s.device) for ds, s in specs.items()}
        else:
            raise ValueError(f"Transport source kind '{kind}' is not valid for {error_context}.")
        if self.scale != 1.0:
            sources = {ds: self.scale * t for ds, t in sources.items()}
        return sources
