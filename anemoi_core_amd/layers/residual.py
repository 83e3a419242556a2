"""Residual connections of the encoder-processor-decoder models - mirror of the reference's layers/residual.py (SkipConnection :60-81,
TruncatedConnection :84-296, SpectralOrnsteinConnection :415-588; the ScalarOrnsteinConnection is not part of this package).

``TruncatedConnection`` coarse-grains the last input step through one sparse matrix and reconstructs it through a second one,
``x_skip = U (D x_last)``; both products are launches of ``ops.sparse_project`` (csrc/sparse_project.hip).  The model asks for the
prognostic columns only (``cols``) and may fold its input normaliser into the down projection (``mul`` / ``add``): truncation does not
commute with an affine map unless every row sums to 1, so the map is applied to each gathered value, not to the result.

``SpectralOrnsteinConnection`` is ``(1 - theta(s)) x + mu(s) + sum_i beta_i(s) f_i`` with fields synthesised from spherical-harmonic
coefficients, optionally on low-pass filtered inputs: at most five launches of csrc/sht.hip (two per transform, one row-wise combine), the
synthesised fields cached per parameter version.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch
from torch import Tensor, nn

from .graph_provider import ProjectionGraphProvider
from .sparse_projector import SparseProjector

LOGGER = logging.getLogger(__name__)

DEFAULT_EDGE_WEIGHT_ATTRIBUTE = "gauss_weight"
_FILE_KEYS = ("truncation_up_file_path", "truncation_down_file_path")
_ON_THE_FLY_KEYS = ("grid", "node_builder", "num_nearest_neighbours", "sigma")  # the reference's on-the-fly truncation_config


class BaseResidualConnection(nn.Module):
    def __init__(self, graph=None, **_) -> None:
        super().__init__()

    @staticmethod
    def _expand_time(x: Tensor, n_step_output: Optional[int]) -> Tensor:
        if n_step_output is None:
            return x
        return x.unsqueeze(1).expand(-1, n_step_output, -1, -1, -1)


class SkipConnection(BaseResidualConnection):
    """Returns one step (default: the most recent) of the input sequence [batch, time, ensemble, nodes, features]."""

    def __init__(self, step: int = -1, **_) -> None:
        super().__init__()
        self.step = step

    def forward(self, x: Tensor, grid_shard_sizes=None, model_comm_group=None, n_step_output: Optional[int] = None) -> Tensor:
        return self._expand_time(x[:, self.step, ...], n_step_output)


class TruncatedConnection(BaseResidualConnection):
    """Truncated skip connection: the most recent input step, coarse-grained and reconstructed by two sparse projections.

    The projections come from two edge sets of ``graph`` (``truncation_down_edges_name`` / ``truncation_up_edges_name``, weighted by
    ``edge_weight_attribute``, default ``gauss_weight``, optionally times ``src_node_weight_attribute`` of the source nodes) or from two
    scipy ``.npz`` files (``truncation_config = {truncation_up_file_path, truncation_down_file_path}``, or the deprecated top-level
    keywords of the same names).  An on-the-fly ``truncation_config`` (grid / node_builder / ...) needs the graph builders of
    ``anemoi-graphs`` and raises NotImplementedError.  The module has no parameters and no buffers."""

    def __init__(self, graph=None, src_node_weight_attribute: Optional[str] = None, edge_weight_attribute: Optional[str] = None,
                 truncation_config: Optional[dict] = None, truncation_up_edges_name: Optional[tuple] = None,
                 truncation_down_edges_name: Optional[tuple] = None, data_node_name: str = "data", autocast: bool = False,
                 sparse_projector_num_chunks: int = 1, row_normalize: bool = False, truncation_up_file_path: Optional[str] = None,
                 truncation_down_file_path: Optional[str] = None, **_) -> None:
        super().__init__()
        if truncation_up_file_path is not None or truncation_down_file_path is not None:
            LOGGER.warning("Passing 'truncation_up_file_path' / 'truncation_down_file_path' as top-level kwargs is deprecated. "
                           "Move them inside 'truncation_config' instead.")
            truncation_config = dict(truncation_config or {})
            for key, val in zip(_FILE_KEYS, (truncation_up_file_path, truncation_down_file_path)):
                if val is not None:
                    truncation_config.setdefault(key, val)
        up_file = down_file = None
        if truncation_config is not None:
            up_file, down_file = (truncation_config.get(k) for k in _FILE_KEYS)
            has_file = up_file is not None or down_file is not None
            if has_file and set(truncation_config) & set(_ON_THE_FLY_KEYS):
                raise ValueError("truncation_config mixes file-based and on-the-fly keys. Use one mode only.")
            if up_file is None or down_file is None:
                raise NotImplementedError("TruncatedConnection: building the truncation subgraph on the fly (truncation_config without both "
                                          "file paths) needs the graph builders of anemoi-graphs; pass pre-resolved "
                                          "truncation_up_edges_name / truncation_down_edges_name or two .npz files")
        weight_attr = edge_weight_attribute if edge_weight_attribute is not None else DEFAULT_EDGE_WEIGHT_ATTRIBUTE
        if up_file is not None:
            assert truncation_up_edges_name is None and truncation_down_edges_name is None, (
                "Specify either file paths or edge names for truncation, not both.")
            up_edges = down_edges = None
        else:
            assert graph is not None, "graph must be provided when file paths are not specified."
            assert truncation_up_edges_name is not None and truncation_down_edges_name is not None, (
                "Both truncation_up_edges_name and truncation_down_edges_name must be provided.")
            up_edges, down_edges = tuple(truncation_up_edges_name), tuple(truncation_down_edges_name)
            types = [tuple(t) for t in graph.edge_types]
            assert up_edges in types, f"Graph must contain edges {up_edges} for up-projection."
            assert down_edges in types, f"Graph must contain edges {down_edges} for down-projection."
        common = dict(graph=graph, edge_weight_attribute=weight_attr, src_node_weight_attribute=src_node_weight_attribute,
                      row_normalize=row_normalize)
        self.provider_down = ProjectionGraphProvider(edges_name=down_edges, file_path=down_file, **common)
        self.provider_up = ProjectionGraphProvider(edges_name=up_edges, file_path=up_file, **common)
        if self.provider_up.shape[1] != self.provider_down.shape[0]:
            raise ValueError(f"truncation matrices do not chain: down is {self.provider_down.shape}, up is {self.provider_up.shape}")
        self.projector = SparseProjector(autocast=autocast, num_chunks=sparse_projector_num_chunks)

    def forward(self, x: Tensor, grid_shard_sizes=None, model_comm_group=None, n_step_output: Optional[int] = None, *,
                cols: Optional[Tensor] = None, mul: Optional[Tensor] = None, add: Optional[Tensor] = None) -> Tensor:
        """x [batch, time, ensemble, nodes, features] -> U (D f(x[:, -1, ..., cols])) as [batch, (n_step_output,) ensemble, nodes, columns]
        in x's dtype.  ``cols`` (int32, device): the feature columns to project (default: all); ``mul`` / ``add`` (fp32 per selected
        column): f(v) = v * mul + add applied to every gathered value of the down projection."""
        return self._expand_time(self.project(x[:, -1, ...], grid_shard_sizes, cols=cols, mul=mul, add=add), n_step_output)

    def project(self, x_last: Tensor, grid_shard_sizes=None, *, cols: Optional[Tensor] = None, mul: Optional[Tensor] = None,
                add: Optional[Tensor] = None) -> Tensor:
        """The two projections of one step [..., nodes, features] (read in place, whatever its strides)."""
        if grid_shard_sizes is not None:
            raise NotImplementedError("TruncatedConnection on a sharded data grid needs the reference's grid-to-channel all-to-all transposes "
                                      "(residual.py:287-293), which this package does not have; run the residual on the unsharded grid")
        coarse = self.projector(x_last, self.provider_down, cols=cols, mul=mul, add=add, out_dtype=torch.float32)  # stays fp32
        out = self.projector(coarse, self.provider_up)
        return out if out.dtype == x_last.dtype else out.to(x_last.dtype)


def _ornstein_init_theta(theta_init, theta_buff: float, statistics: Optional[dict]) -> np.ndarray:
    """The reference's first guess of theta (layers/residual.py:299-319): ``theta_init``, or with theta_init = 0 and tendency statistics
    0.5 (stdev_tend / stdev)^2, mapped into the (theta_buff, 1) interval and clipped to (0.01, 0.99)."""
    statistics = statistics or {}
    if theta_init == 0 and {"stdev", "stdev_tend"}.issubset(statistics):
        theta_init = 0.5 * (statistics["stdev_tend"] / statistics["stdev"]) ** 2
    theta = (np.asarray(theta_init) - theta_buff) / (1 - theta_buff)
    theta = np.where(theta < 1, theta, 0.99)
    return np.where(theta > 0, theta, 0.01)


def _grid_shape_from_graph(graph, dataset_name) -> tuple[int, int]:
    """(nlat, nlon) = the numbers of distinct latitudes and longitudes of a node set (``graph[name].x``, ``graph[name]["x"]`` or a plain
    tensor of coordinates)."""
    assert graph is not None and dataset_name is not None, (
        "Ornstein residuals need both `graph` and `dataset_name` to derive nlat/nlon. These are passed by the model's `_build_residual`.")
    store = graph[dataset_name]
    x = store if isinstance(store, Tensor) else (store["x"] if isinstance(store, dict) else store.x)
    x = torch.as_tensor(x)
    return int(torch.unique(x[:, 0]).numel()), int(torch.unique(x[:, 1]).numel())


class SpectralOrnsteinConnection(BaseResidualConnection):
    """Ornstein residual with spatially varying theta, mu and beta_i given by ``lmax x lmax`` spherical-harmonic coefficients per prognostic
    variable (the reference's keywords, parameters ``weight`` [R + 2, n_prog, lmax, lmax, 2], ``filter`` [n_trunc, nlat], ``walias``
    [n_trunc, lmax, lmax, 2] and buffer ``muzero``: its state_dict loads).  With ``truncate`` the truncated input columns are low-pass
    filtered first: forward transform, per-degree filter, inverse transform, blended with the input by sigmoid(isht(walias)) when
    ``anti_aliasing``.

    Inference only, fp32: ``compact`` is one forward transform (2 launches) + one filtered inverse transform (2) + the combine (1), or the
    combine alone without ``truncate``; the fields synthesised from the parameters are cached per parameter version (point-major, so the
    combine reads them coalesced).  Under grad mode with a parameter or input that requires grad it raises NotImplementedError: the
    adjoint kernels of the transforms are not built.  The reference writes the filtered fields back into the caller's ``x`` (its
    rearranged view aliases it); ``forward`` leaves ``x`` as it is (``compact(.., write_back=True)`` reproduces the side effect for the
    model) and regressors are read from the unfiltered input, so a regressor that is itself a truncated prognostic variable is refused."""

    def __init__(self, lmax: int = 2, grid: str = "regular", theta_init: float = 0.00, theta_buff: float = 0.00, use_mean: bool = True,
                 regressors: Optional[list] = None, truncate: bool = False, skip_truncate_variables: Optional[list] = None,
                 anti_aliasing: bool = True, graph=None, statistics: Optional[dict] = None, data_indices=None,
                 dataset_name: Optional[str] = None, **_) -> None:
        super().__init__()
        from .block import _FusedWeights
        from .spectral_helpers import InverseSphericalHarmonicTransform, SphericalHarmonicTransform
        from .spectral_transforms import InverseOctahedralSHT, InverseRegularSHT, octahedral_lons_per_lat

        regressors = list(regressors or [])
        assert data_indices is not None, "SpectralOrnsteinConnection needs `data_indices`."
        self._internal_input_idx = list(data_indices.model.input.prognostic)
        variables = data_indices.model.input.name_to_index
        self._regressors_input_idx = [variables[f] for f in regressors]
        self.nlat, self.nlon = _grid_shape_from_graph(graph, dataset_name)
        stats = {}
        if statistics:
            idx = data_indices.data.input.prognostic
            stats = {k: v[idx] for k, v in statistics.items() if hasattr(v, "__getitem__")}
        theta = _ornstein_init_theta(theta_init, theta_buff, stats)
        theta = 4 * np.pi * np.log(theta / (1 - theta))
        n_prog = len(self._internal_input_idx)
        weight = torch.zeros(len(regressors) + 2, n_prog, lmax, lmax, 2)
        weight[0, :, 0, 0, 0] = torch.from_numpy(np.broadcast_to(theta, (n_prog,)).copy())
        self.weight = nn.Parameter(weight)
        if grid == "octahedral":
            self.isht = InverseOctahedralSHT(self.nlat, truncation=lmax - 1)
        elif grid == "regular":
            self.isht = InverseRegularSHT(self.nlat, truncation=lmax - 1)
        else:
            raise ValueError(f"Unsupported grid type {grid!r}. Supported types: ['octahedral', 'regular']")
        muzero = torch.ones_like(weight)
        muzero[1] = 1.0 if use_mean else 0.0
        self.register_buffer("muzero", muzero)
        self.theta_buff = theta_buff
        self.truncate = truncate
        self.anti_aliasing = bool(anti_aliasing)
        col = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
        self.register_buffer("_prog_cols", col(self._internal_input_idx), persistent=False)
        self.register_buffer("_reg_cols", col(self._regressors_input_idx) if regressors else None, persistent=False)
        if truncate:
            lons = octahedral_lons_per_lat(self.nlat) if grid == "octahedral" else [self.nlon] * self.nlat
            trunc = self.nlat - 1
            self.x_fsht = SphericalHarmonicTransform(lons_per_lat=lons, truncation=trunc)
            self.x_isht = InverseSphericalHarmonicTransform(lons_per_lat=lons, truncation=trunc)
            skip_idx = {variables[v] for v in (skip_truncate_variables or []) if v in variables}
            self._truncation_input_idx = [int(i) for i in self._internal_input_idx if i not in skip_idx]
            if set(self._truncation_input_idx) & set(self._regressors_input_idx):
                raise NotImplementedError("SpectralOrnsteinConnection: a regressor that is itself a truncated prognostic variable (the "
                                          "reference reads its filtered values) is not supported")
            blur_lmax = trunc + 1
            filt = torch.ones(len(self._truncation_input_idx), blur_lmax) * max(theta_init, 0.01) / (0.5 - max(theta_init, 0.01))
            self.filter = nn.Parameter(torch.sqrt(filt / blur_lmax))
            self.walias = nn.Parameter(torch.zeros(len(self._truncation_input_idx), lmax, lmax, 2))
            where = {c: t for t, c in enumerate(self._truncation_input_idx)}
            self.register_buffer("_trunc_cols", col(self._truncation_input_idx), persistent=False)
            self.register_buffer("_trunc_map", col([where.get(int(c), -1) for c in self._internal_input_idx]), persistent=False)
        self._derived = _FusedWeights()

    # -- what is synthesised from the parameters, cached until one of them changes in place ------------------------------------------
    def _fields(self) -> Tensor:
        """fp32 [R + 2, grid, n_prog]: the gain 1 - sigmoid(theta) (1 - theta_buff) - theta_buff, mu, beta_i."""
        def build():
            f = self.isht._isht(torch.view_as_complex((self.weight * self.muzero).float().contiguous()), columns=True)
            f[0] = 1 - torch.sigmoid(f[0]) * (1 - self.theta_buff) - self.theta_buff
            return f
        return self._derived.derived("fields", [self.weight, self.muzero], build)

    def _x_filter(self) -> Tensor:
        """fp32 [n_trunc, nlat]: the low-pass factor 1 - f of every degree, f = cumsum(filter^2) / (1 + cumsum(filter^2))."""
        def build():
            f = torch.cumsum(torch.square(self.filter.float()), -1)
            return (1 - f / (1 + f)).contiguous()
        return self._derived.derived("filter", [self.filter], build)

    def _w_filter(self) -> Tensor:
        """fp32 [grid, n_trunc]: sigmoid(isht(walias))."""
        def build():
            return torch.sigmoid(self.isht._isht(torch.view_as_complex(self.walias.float().contiguous()), columns=True))
        return self._derived.derived("walias", [self.walias], build)

    def compact(self, x_last: Tensor, grid_shard_sizes=None, write_back: bool = False) -> Tensor:
        """x_last [..., grid, vars] (fp32, read in place) -> the residual on the prognostic columns [..., grid, n_prog].  ``write_back``
        (with ``truncate``): the filtered fields are also written into the truncated columns of x_last, as the reference's residual leaves
        them in its caller's input - its model builds the encoder's input from that, so the model here asks for it on a copy."""
        from .. import ops

        if grid_shard_sizes is not None:
            raise NotImplementedError("SpectralOrnsteinConnection on a sharded data grid: a spherical-harmonic transform needs whole latitude "
                                      "rings on one device; run the residual on the unsharded grid")
        ops._dev(x_last)
        params = [self.weight] + ([self.filter, self.walias] if self.truncate else [])
        if ops._needs_grad(x_last, *params):
            raise NotImplementedError("SpectralOrnsteinConnection is forward-only: the adjoint kernels of the spherical-harmonic transforms "
                                      "(csrc/sht.hip) are not built; run it under torch.no_grad()")
        if x_last.dtype != torch.float32:
            raise TypeError(f"SpectralOrnsteinConnection: expected float32 input, got {x_last.dtype}")
        if x_last.dim() < 2 or x_last.shape[-2] != self.isht._isht.n_grid_points:
            raise ValueError(f"SpectralOrnsteinConnection: input {tuple(x_last.shape)} does not have the grid's {self.isht._isht.n_grid_points} points")
        if max(self._internal_input_idx + self._regressors_input_idx) >= x_last.shape[-1]:  # the kernels index columns unchecked
            raise ValueError(f"SpectralOrnsteinConnection: input with {x_last.shape[-1]} variables, column "
                             f"{max(self._internal_input_idx + self._regressors_input_idx)} needed")
        low = walias = tmap = None
        if self.truncate:
            coeffs = self.x_fsht(x_last, cols=self._trunc_cols, columns=True)  # [..., n_trunc, L, M]
            low = self.x_isht(coeffs, lscale=self._x_filter(), columns=True)    # [..., grid, n_trunc]
            walias, tmap = (self._w_filter() if self.anti_aliasing else None), self._trunc_map
        return ops.ornstein_combine(x_last, self._prog_cols, self._fields(), self._reg_cols, tmap, low, walias,
                                    write_back=write_back and self.truncate)

    def forward(self, x: Tensor, grid_shard_sizes=None, model_comm_group=None, n_step_output: Optional[int] = None) -> Tensor:
        """x [batch, time, ensemble, grid, vars] -> [batch, (n_step_output,) ensemble, grid, vars]: the residual in the prognostic columns,
        zeros elsewhere (the reference's full-width result: a zero fill and a scatter on top of ``compact``, which the model uses)."""
        x_last = x[:, -1, ...]
        skip = self.compact(x_last, grid_shard_sizes)
        out = torch.zeros_like(x_last)
        out[..., self._internal_input_idx] = skip
        return self._expand_time(out, n_step_output)
