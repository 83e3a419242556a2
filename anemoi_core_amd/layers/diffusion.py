"""Noise-level embedders - mirror of the reference's ``anemoi.models.layers.diffusion`` (RandomFourierEmbeddings :15-25,
SinusoidalEmbeddings :28-38): same constructor keywords, same buffers (``frequencies``, and ``pi`` for the random-Fourier one), same
state_dict keys.

Inside the transport model the embedding never runs on its own: ``ops.noise_cond`` computes it together with the conditioning MLP in one
launch and reads ``frequencies`` / ``pi`` from these modules (``embedding_operands``).  ``forward`` is that kernel with an identity MLP
left out: the plain torch expression, kept for callers that want the embedding alone (a handful of values per call).
"""
from __future__ import annotations

import math

import torch
from torch import Tensor, nn


class RandomFourierEmbeddings(nn.Module):
    """Random Fourier embeddings for noise levels: [sin | cos] of ``x * frequencies * 2 * pi``."""

    def __init__(self, num_channels: int = 32, scale: int = 16):
        super().__init__()
        self.register_buffer("frequencies", torch.randn(num_channels // 2) * scale)
        self.register_buffer("pi", torch.tensor(math.pi))

    def embedding_operands(self) -> tuple:
        """(frequencies, pi) as ``ops.noise_cond`` takes them."""
        return self.frequencies, self.pi

    def forward(self, x: Tensor) -> Tensor:
        arg = x * self.frequencies.unsqueeze(0) * 2 * self.pi
        return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)


class SinusoidalEmbeddings(nn.Module):
    """Sinusoidal embeddings for noise levels: [sin | cos] of ``x * frequencies``, frequencies = max_period^(-i / (C / 2))."""

    def __init__(self, num_channels: int = 32, max_period: int = 10000):
        super().__init__()
        half = num_channels // 2
        self.register_buffer("frequencies", torch.exp(-math.log(max_period) * torch.arange(0, half) / half))

    def embedding_operands(self) -> tuple:
        return self.frequencies, None

    def forward(self, x: Tensor) -> Tensor:
        arg = x[:] * self.frequencies
        return torch.cat((arg.sin(), arg.cos()), dim=-1)
