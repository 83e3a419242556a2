"""Residual connections of the encoder-processor-decoder models - mirror of the reference's layers/residual.py (SkipConnection :60-81,
TruncatedConnection :84-296; the Ornstein residuals and their spherical-harmonic transforms are not part of this package).

``TruncatedConnection`` coarse-grains the last input step through one sparse matrix and reconstructs it through a second one,
``x_skip = U (D x_last)``; both products are launches of ``ops.sparse_project`` (csrc/sparse_project.hip).  The model asks for the
prognostic columns only (``cols``) and may fold its input normaliser into the down projection (``mul`` / ``add``): truncation does not
commute with an affine map unless every row sums to 1, so the map is applied to each gathered value, not to the result.
"""
from __future__ import annotations

import logging
from typing import Optional

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
