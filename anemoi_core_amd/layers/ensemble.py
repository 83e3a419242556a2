"""Noise injectors of the ensemble model - mirror of the reference's ``anemoi.models.layers.ensemble`` (NoOpNoiseInjector :84-105,
NoiseConditioning :108-221, NoiseInjector :224-321): same constructor keywords, forward signatures and state_dict keys
(``noise_mlp.*``; ``_noise_conditioning.noise_mlp.*``, ``projection.*``).

Every member of an ensemble sees its own noise: ``randn(batch, ensemble, grid, channels) * noise_std`` flattened to the rows of the latent,
passed through ``noise_mlp`` and either handed to the processor as the conditioning of its ConditionalLayerNorms (NoiseConditioning) or
projected into the latent (NoiseInjector).  The draw goes through ``NoiseConditioning.draw`` so that a test (or a reproducible forecast)
can substitute recorded noise; by default it uses the device's default generator, which is legal under hipGraph capture.

Not implemented: noise on a coarser grid projected through a sparse matrix (``noise_matrix`` / ``noise_edges_name``: the reference's
ProjectionGraphProvider + SparseProjector); both reference configs leave them null.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from ..distributed.primitives import shard_tensor
from ..distributed.shapes import get_shard_sizes
from .kernels import Linear, PaddedLinear
from .mlp import MLP
from .utils import load_layer_kernels


class BaseNoiseInjector(nn.Module):
    """forward(x, batch_size, ensemble_size, grid_size, grid_shard_sizes, noise_dtype, model_comm_group) -> (x', noise or None)."""


class NoOpNoiseInjector(BaseNoiseInjector):
    """Reference ensemble.py:84-105: the input unchanged, no noise."""

    def __init__(self, **kwargs) -> None:
        super().__init__()

    def forward(self, x: Tensor, batch_size: int, ensemble_size: int, grid_size: int, grid_shard_sizes, noise_dtype: torch.dtype = torch.float32,
                model_comm_group=None) -> tuple[Tensor, None]:
        return x, None


class NoiseConditioning(BaseNoiseInjector):
    """Reference ensemble.py:108-221: returns (x, noise_mlp(noise)) - the rows the processor's ConditionalLayerNorms are conditioned on."""

    def __init__(self, *, noise_std: int, noise_channels_dim: int, noise_mlp_hidden_dim: int, layer_kernels, noise_matrix: Optional[str] = None,
                 noise_edges_name: Optional[tuple] = None, edge_weight_attribute: Optional[str] = None, row_normalize_noise_matrix: bool = False,
                 autocast: bool = False, sparse_projector_num_chunks: int = 1, num_channels: Optional[int] = None, graph_data=None) -> None:
        super().__init__()
        assert noise_channels_dim > 0, "Noise channels must be a positive integer"
        assert noise_mlp_hidden_dim > 0, "Noise channels must be a positive integer"
        assert not (noise_matrix is not None and noise_edges_name is not None), "Specify either noise_matrix or noise_edges_name, not both."
        for name, value in (("noise_matrix", noise_matrix), ("noise_edges_name", noise_edges_name)):
            if value is not None:
                raise NotImplementedError(f"NoiseConditioning({name}={value!r}): noise drawn on another grid needs ProjectionGraphProvider and "
                                          "SparseProjector, which this package does not have; set it to null (noise on the hidden grid).")
        self.noise_std = noise_std
        self.noise_channels = noise_channels_dim
        self.layer_factory = load_layer_kernels(layer_kernels)
        self.noise_mlp = MLP(noise_channels_dim, noise_mlp_hidden_dim, noise_channels_dim, layer_kernels=self.layer_factory, n_extra_layers=0,
                             final_activation=False, layer_norm=True)
        self.noise_graph_provider = None

    def draw(self, shape: tuple, dtype: torch.dtype, device) -> Tensor:
        """Standard-normal noise of ``shape`` = (batch, ensemble, grid, channels), from the device's default generator.  Override (or
        assign) to substitute recorded noise."""
        return torch.randn(size=shape, dtype=dtype, device=device)

    def forward(self, x: Tensor, batch_size: int, ensemble_size: int, grid_size: int, grid_shard_sizes, noise_dtype: torch.dtype = torch.float32,
                model_comm_group=None) -> tuple[Tensor, Tensor]:
        noise = self.draw((batch_size, ensemble_size, grid_size, self.noise_channels), noise_dtype, x.device) * self.noise_std
        noise = noise.detach().reshape(batch_size * ensemble_size * grid_size, self.noise_channels)  # "(batch ensemble grid) vars": the rows of x
        noise = shard_tensor(noise, 0, get_shard_sizes(noise, 0, model_comm_group), model_comm_group)  # sharded grid dim, full channels
        # (the reference wraps noise_mlp in torch.utils.checkpoint: recomputation instead of stored activations, same values)
        return x, self.noise_mlp(noise)


class NoiseInjector(BaseNoiseInjector):
    """Reference ensemble.py:224-321: ``projection([x | noise_mlp(noise)])`` replaces the latent; no conditioning is returned."""

    def __init__(self, *, noise_std: int, noise_channels_dim: int, noise_mlp_hidden_dim: int, num_channels: int, layer_kernels,
                 noise_matrix: Optional[str] = None, graph_data=None) -> None:
        super().__init__()
        self._noise_conditioning = NoiseConditioning(noise_std=noise_std, noise_channels_dim=noise_channels_dim,
                                                     noise_mlp_hidden_dim=noise_mlp_hidden_dim, layer_kernels=layer_kernels,
                                                     noise_matrix=noise_matrix, graph_data=graph_data)
        self.noise_channels = noise_channels_dim
        self.projection = Linear(num_channels + self.noise_channels, num_channels)  # nn.Linear parameters and keys (ensemble.py:272)
        self._pad = PaddedLinear()

    def forward(self, x: Tensor, batch_size: int, ensemble_size: int, grid_size: int, grid_shard_sizes, noise_dtype: torch.dtype = torch.float32,
                model_comm_group=None) -> tuple[Tensor, None]:
        x, noise = self._noise_conditioning(x=x, batch_size=batch_size, ensemble_size=ensemble_size, grid_size=grid_size,
                                            grid_shard_sizes=grid_shard_sizes, noise_dtype=noise_dtype, model_comm_group=model_comm_group)
        return self._pad(torch.cat([x, noise.to(x.dtype)], dim=-1), self.projection), None
