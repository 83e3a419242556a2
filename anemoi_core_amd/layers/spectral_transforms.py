"""Spectral transforms of model fields - mirror of the reference's layers/spectral_transforms.py for the spherical-harmonic transforms on
regular and octahedral grids (SHT :214-225, RegularSHT :228-261, OctahedralSHT :328-369 and the inverses :372-407, :468-503).

The forward transforms take the model's ``[b, t, e, p, v]`` layout and return ``[b, t, e, L, M, v]`` complex coefficients.  The reference
copies the input to ``(b t e v) p`` order first; here the kernels read the variables in place (csrc/sht.hip) and the result is a view of the
``[b, t, e, v, L, M]`` coefficients, as the reference's rearrange is.  ``ReducedSHT`` (needs anemoi.transform's grid lookup), ``FFT2D`` and
``DCT2D`` are not part of this package.
"""
from __future__ import annotations

import abc

import torch

from .spectral_helpers import InverseSphericalHarmonicTransform, SphericalHarmonicTransform


def octahedral_lons_per_lat(nlat: int) -> list[int]:
    """Points per ring of the octahedral grid with ``nlat`` latitudes: 20 + 4 i from either pole."""
    half = [20 + 4 * i for i in range(nlat // 2)]
    return half + list(reversed(half))


class SpectralTransform(torch.nn.Module):
    """Abstract base class for spectral transforms: ``[b, t, e, p, v]`` -> ``[b, t, e, y_freq, x_freq, v]``."""

    @abc.abstractmethod
    def forward(self, data: torch.Tensor) -> torch.Tensor: ...


class SHT(SpectralTransform):
    """Spherical-harmonic transform base class."""

    _sht: SphericalHarmonicTransform

    def power_spectral_density(self, spectral_coeffs: torch.Tensor) -> torch.Tensor:
        """Per-L power spectral density: the sum over M of |coeff|^2."""
        return (spectral_coeffs.real**2 + spectral_coeffs.imag**2).sum(dim=-2)

    def cross_spectral_density(self, spectral_coeffs_a: torch.Tensor, spectral_coeffs_b: torch.Tensor) -> torch.Tensor:
        """Per-L cross-spectral density."""
        return (spectral_coeffs_a.real * spectral_coeffs_b.real + spectral_coeffs_a.imag * spectral_coeffs_b.imag).sum(dim=-2)

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        b, t, e, p, v = data.shape
        assert p == self._sht.n_grid_points, f"Input points={p} does not match the grid's {self._sht.n_grid_points}"
        coeffs = self._sht(data, columns=True)  # [b, t, e, v, L, M], the variables read in place
        return coeffs.permute(0, 1, 2, 4, 5, 3)


class RegularSHT(SHT):
    """SHT on a regular lon-lat grid of ``nlat`` x ``2 nlat`` points."""

    def __init__(self, nlat: int, truncation: int | None = None, **kwargs) -> None:
        super().__init__()
        self.nlat = nlat
        self.nlon = 2 * self.nlat
        self.lons_per_lat = [self.nlon] * self.nlat
        self._sht = SphericalHarmonicTransform(lons_per_lat=self.lons_per_lat, truncation=truncation or self.nlat // 2 - 1)


class OctahedralSHT(SHT):
    """SHT on an octahedral reduced grid."""

    def __init__(self, nlat: int, truncation: int | None = None, use_graphed_rfft: bool = False, **kwargs) -> None:
        super().__init__()
        self.nlat = nlat
        self.lons_per_lat = octahedral_lons_per_lat(nlat)
        self._sht = SphericalHarmonicTransform(lons_per_lat=self.lons_per_lat, truncation=truncation or self.nlat // 2 - 1,
                                               use_graphed_rfft=use_graphed_rfft)


class InverseSpectralTransform(torch.nn.Module):
    """Inverse spectral transforms: complex ``[..., l, m]`` -> real ``[..., points]``."""

    _isht: InverseSphericalHarmonicTransform

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        return self._isht(data)


class InverseRegularSHT(InverseSpectralTransform):
    """Inverse SHT on a regular lon-lat grid."""

    def __init__(self, nlat: int, truncation: int | None = None, **kwargs) -> None:
        super().__init__()
        self.nlat = nlat
        self.nlon = 2 * nlat
        self.lons_per_lat = [self.nlon] * self.nlat
        self._isht = InverseSphericalHarmonicTransform(lons_per_lat=self.lons_per_lat, truncation=truncation or self.nlat // 2 - 1)


class InverseOctahedralSHT(InverseSpectralTransform):
    """Inverse SHT on an octahedral reduced grid."""

    def __init__(self, nlat: int, truncation: int | None = None, use_graphed_irfft: bool = False, **kwargs) -> None:
        super().__init__()
        self.nlat = nlat
        self.lons_per_lat = octahedral_lons_per_lat(nlat)
        self._isht = InverseSphericalHarmonicTransform(lons_per_lat=self.lons_per_lat, truncation=truncation or self.nlat // 2 - 1,
                                                       use_graphed_irfft=use_graphed_irfft)
