"""Spherical-harmonic transforms on grids of latitude rings - mirror of the reference's layers/spectral_helpers.py
(SphericalHarmonicTransform :109-340, InverseSphericalHarmonicTransform :343-553): same constructors, attributes, buffers and output shapes.

The reference runs one ``torch.fft.rfft`` / ``irfft`` launch per latitude ring of a reduced grid and two einsums over the dense ``[m, l, k]``
Legendre table; here a transform is two launches of csrc/sht.hip (``ops.sht_forward`` / ``ops.sht_inverse``): direct ring DFTs with host-built
twiddles, and a Legendre step that skips l < m.  ``use_graphed_rfft`` / ``use_graphed_irfft`` are accepted and inert: there is no per-ring
loop to graph.

The tables are computed here in numpy float64 from the textbook recurrences: Gauss-Legendre nodes by Newton iteration on P_n from the
Chebyshev-like first guess (Abramowitz & Stegun 25.4.29; Press et al., Numerical Recipes, gauleg) and the orthonormalised associated
Legendre functions by the three-term recurrence in degree at fixed order (Holmes & Featherstone 2002, eqs. 11-13; Schaeffer 2013, section
2.1), without the Condon-Shortley phase and scaled as the reference's tables are: P_00 = 1 for the analysis, 1 / (4 pi) for the synthesis.

Forward only: with grad enabled and an input that requires grad the transforms raise NotImplementedError (the adjoint kernels are a
follow-up, as the window attention's backward was).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor
from torch.nn import Module

from .. import ops


def gauss_legendre(n: int) -> tuple[np.ndarray, np.ndarray]:
    """Nodes (ascending in [-1, 1]) and weights of the n-point Gauss-Legendre rule, float64."""
    i = np.arange(n, dtype=np.float64)
    x = -np.cos(np.pi * (i + 0.75) / (n + 0.5))  # first guess, ascending
    for _ in range(100):
        p0, p1 = np.ones_like(x), x.copy()  # P_0, P_1
        for d in range(2, n + 1):
            p0, p1 = p1, ((2 * d - 1) * x * p1 - (d - 1) * p0) / d
        dp = n * (x * p1 - p0) / (x * x - 1.0)  # P_n'
        dx = p1 / dp
        x = x - dx
        if np.max(np.abs(dx)) < 1e-16:
            break
    p0, p1 = np.ones_like(x), x.copy()
    for d in range(2, n + 1):
        p0, p1 = p1, ((2 * d - 1) * x * p1 - (d - 1) * p0) / d
    dp = n * (x * p1 - p0) / (x * x - 1.0)
    w = 2.0 / ((1.0 - x * x) * dp * dp)
    x = 0.5 * (x - x[::-1])  # the rule is symmetric: remove the last-bit asymmetry of the iteration
    w = 0.5 * (w + w[::-1])
    return x, w


def gaussian_colatitudes(nlat: int) -> tuple[np.ndarray, np.ndarray]:
    """(cos(colatitude) north to south, quadrature weight) of the nlat Gaussian latitudes."""
    x, w = gauss_legendre(nlat)
    theta = np.flip(np.arccos(x))  # colatitudes ascending from the north pole, as the reference derives its abscissae (:195-199)
    return np.cos(theta), w


def legendre_table(truncation: int, x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """float64 [m, l, k], m, l <= truncation: the orthonormalised associated Legendre functions at x_k, positive on the diagonal, times
    sqrt(4 pi) (analysis) or 1 / sqrt(4 pi) (synthesis); zero for l < m."""
    n = truncation + 1
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((n, n, x.shape[0]), dtype=np.float64)
    sin2 = (1.0 + x) * (1.0 - x)
    pmm = np.full_like(x, 1.0 / (4.0 * np.pi) if inverse else 1.0)  # P_00
    for m in range(n):
        if m > 0:
            pmm = np.sqrt((2 * m + 1) * sin2 / (2 * m)) * pmm  # sectoral step P_mm from P_{m-1, m-1}
        out[m, m] = pmm
        if m + 1 < n:
            out[m, m + 1] = np.sqrt(2 * m + 3) * x * pmm
        for l in range(m + 2, n):
            a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            out[m, l] = a * (x * out[m, l - 1] - b * out[m, l - 2])
    return out


def legendre_tables(nlat: int, truncation: int) -> tuple[np.ndarray, np.ndarray]:
    """(weight, pct) float64 [m, l, k] as the reference's two modules hold them: the quadrature-weighted analysis table and the synthesis
    table."""
    x, w = gaussian_colatitudes(nlat)
    return legendre_table(truncation, x) * w[None, None, :], legendre_table(truncation, x, inverse=True)


def kernel_table(table_mlk: Tensor, device) -> Tensor:
    """[m, l, k] float64 -> the kernels' fp32 [l, k, m] (m fastest) on ``device``."""
    return table_mlk.permute(1, 2, 0).to(torch.float32).contiguous().to(device)


class _RingTransform(Module):
    """What the two directions share: the reference's attributes and the device-side constants, built on first use per device."""

    def _setup(self, lons_per_lat, truncation: int) -> None:
        self.lons_per_lat = lons_per_lat
        self.nlat = len(self.lons_per_lat)
        self.truncation = truncation
        self.n_grid_points = int(sum(self.lons_per_lat))
        self.slon = [0] + [int(v) for v in np.cumsum(self.lons_per_lat)[:-1]]
        number_of_latitude_bands = 3  # kept as an attribute of the reference's modules; nothing here is banded
        self.latitude_bands = [(b * self.nlat // number_of_latitude_bands, (b + 1) * self.nlat // number_of_latitude_bands)
                               for b in range(number_of_latitude_bands)]
        self._device_tables: dict = {}

    def _constants(self, table: Tensor, device) -> tuple:
        key = str(device)
        hit = self._device_tables.get(key)
        if hit is None:
            hit = (ops.sht_grid(self.lons_per_lat, device), kernel_table(table, device))
            self._device_tables[key] = hit
        return hit


class SphericalHarmonicTransform(_RingTransform):
    """Direct transform: field ``[..., grid]`` -> complex coefficients ``[..., l, m]``.  ``weight`` (float64 [m, l, k], non-persistent) is the
    reference's buffer; the kernels read an fp32 ``[l, k, m]`` copy of it."""

    def __init__(self, lons_per_lat: list[int], truncation: int, use_graphed_rfft: bool = False) -> None:
        super().__init__()
        self._setup(lons_per_lat, truncation)
        assert 0 < self.truncation <= self.nlat, (
            f"Truncation {self.truncation} must be between 1 and number of latitudes {self.nlat}")
        self.rlon = [max(self.lons_per_lat) // 2 - nlon // 2 for nlon in self.lons_per_lat]
        self._graphed_rfft_cache = {}
        weight, _ = legendre_tables(self.nlat, self.truncation)
        self.register_buffer("weight", torch.from_numpy(weight), persistent=False)

    def forward(self, x: Tensor, cols: Tensor | None = None, columns: bool = False) -> Tensor:
        """x fp32 ``[..., grid]`` -> complex64 ``[..., l, m]``.  With ``columns=True`` x is ``[..., grid, V]``, read in place (``cols``: int32
        device vector of the columns to transform, default all), and the result is ``[..., C, l, m]``."""
        ops._dev(x)
        grid, table = self._constants(self.weight, x.device)
        return ops.sht_forward(x, grid, table, cols=cols, columns=columns)


class InverseSphericalHarmonicTransform(_RingTransform):
    """Inverse transform: complex coefficients ``[..., l, m]`` -> field ``[..., grid]``.  ``pct`` (float64 [m, l, k], non-persistent) is the
    reference's buffer."""

    def __init__(self, lons_per_lat: list[int], truncation: int, use_graphed_irfft: bool = False) -> None:
        super().__init__()
        self._setup(lons_per_lat, truncation)
        if not 0 < self.truncation <= self.nlat:  # (the reference's inverse has no such check; the kernels' plan shares the forward's)
            raise ValueError(f"Truncation {self.truncation} must be between 1 and number of latitudes {self.nlat}")
        self._graphed_irfft_cache = {}
        _, pct = legendre_tables(self.nlat, self.truncation)
        self.register_buffer("pct", torch.from_numpy(pct), persistent=False)

    def forward(self, x: Tensor, lscale: Tensor | None = None, columns: bool = False) -> Tensor:
        """x complex64 ``[..., l, m]`` -> fp32 ``[..., grid]``.  ``lscale`` fp32 [S, l]: a per-degree factor applied to field f % S on the way
        in.  With ``columns=True`` x is ``[..., C, l, m]`` and the result the point-major ``[..., grid, C]``."""
        ops._dev(x)
        grid, table = self._constants(self.pct, x.device)
        return ops.sht_inverse(x, grid, table, lscale=lscale, columns=columns)
