"""Static graph provider — mirror of reference layers/graph_provider.py:145-291.

Owns the dst-sorted edge list, its attributes and the trainable edge tensor.  ``get_edges`` returns
``(edge_attr [B*M, F+trainable], edge_index int64 [2, B*M], edge_shard_sizes)`` like the reference, but the tensors
are cached across calls (static graph, static parameters at inference), which lets every downstream cache
(CSC, packed edge features, halo plan, local mapper graph) hit.

``ProjectionGraphProvider`` (reference layers/graph_provider.py:464-661) holds a constant sparse projection matrix instead: CSR arrays on
the host, one device copy per device (``ops.SparseMatrix`` with its transpose), consumed by ``ops.sparse_project``."""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch
from torch import Tensor, nn

from ..distributed.partition import edge_shard_plan, take_edge_rows, sort_edge_index_by_dst
from .graph import TrainableTensor
from ..utils.tensors import version

LOGGER = logging.getLogger(__name__)


class StaticGraphProvider(nn.Module):
    _TRAINABLE_LAYOUT_VERSION = 1
    _TRAINABLE_LAYOUT_VERSION_KEY = "trainable_layout_version"

    def __init__(self, edge_index: Tensor, edge_attr: Tensor, src_size: int, dst_size: int, trainable_size: int) -> None:
        """``edge_index`` [2, M] (src, dst) any order; ``edge_attr`` [M, F] the concatenated sub-graph attributes."""
        super().__init__()
        edge_index = torch.as_tensor(edge_index).long()
        edge_attr = torch.as_tensor(edge_attr, dtype=torch.float32)
        edge_index, perm = sort_edge_index_by_dst(edge_index)  # once, at init (graph_provider.py:185-187)
        self.register_buffer("perm", perm, persistent=False)
        self.register_buffer("edge_attr", edge_attr.index_select(0, perm).contiguous(), persistent=False)
        self.register_buffer("edge_index_base", edge_index.contiguous(), persistent=False)
        self.register_buffer("edge_inc", torch.tensor([[src_size], [dst_size]], dtype=torch.int64), persistent=False)
        self.register_buffer(self._TRAINABLE_LAYOUT_VERSION_KEY, torch.tensor(self._TRAINABLE_LAYOUT_VERSION, dtype=torch.int64), persistent=True)
        self.trainable = TrainableTensor(trainable_size=trainable_size, tensor_size=edge_attr.shape[0])
        self._edge_dim = edge_attr.shape[1] + trainable_size
        self._sizes = (int(src_size), int(dst_size))
        self._cache: dict = {}

    @property
    def edge_dim(self) -> int:
        return self._edge_dim

    @property
    def is_sparse(self) -> bool:
        return False

    def _apply(self, fn, recurse=True):
        """Keep the geometric edge attributes in fp32 when the model is cast to bf16/fp16: the fused attention consumes
        fp32 edge features anyway (the reference's autocast likewise leaves edge_attr in fp32)."""
        ea = self.edge_attr
        super()._apply(fn, recurse)
        if self.edge_attr.dtype != torch.float32:
            self.edge_attr = ea.to(self.edge_attr.device)
        self._cache.clear()
        return self

    def get_edges(self, batch_size: int, src_coords=None, dst_coords=None, model_comm_group=None, shard_edges: bool = True,
                  act_checkpoint: bool = True):
        edge_attr = self.trainable(self.edge_attr, batch_size)  # cached by TrainableTensor outside training
        key = (batch_size, shard_edges, id(model_comm_group))  # index part only: edge_attr is a fresh tensor per training step
        hit = self._cache.get("edges")
        if hit is None or hit[0] != key:
            if batch_size == 1:
                edge_index = self.edge_index_base
            else:
                edge_index = torch.cat([self.edge_index_base + i * self.edge_inc for i in range(batch_size)], dim=1)
            plan = (None, None, edge_index, None)
            if shard_edges:
                src_size, dst_size = self._sizes
                plan = edge_shard_plan(edge_index, src_size * batch_size, dst_size * batch_size, model_comm_group)
            hit = self._cache["edges"] = (key, plan)
        perm, rows, edge_index, splits = hit[1]
        return take_edge_rows(edge_attr, perm, rows), edge_index, splits


class NoOpGraphProvider(nn.Module):
    @property
    def edge_dim(self) -> int:
        return 0

    def get_edges(self, *args, **kwargs):
        return None, None, None


def create_graph_provider(graph=None, edge_attributes: Optional[list] = None, src_size: Optional[int] = None,
                          dst_size: Optional[int] = None, trainable_size: int = 0):
    """``graph``: an edge store with ``edge_index`` and the named attribute tensors (a HeteroData edge store or a dict)."""
    if not graph:
        return NoOpGraphProvider()
    get = (lambda k: graph[k]) if isinstance(graph, dict) else (lambda k: getattr(graph, k) if hasattr(graph, k) else graph[k])
    assert edge_attributes is not None, "Edge attributes must be provided"
    ea = torch.cat([torch.as_tensor(get(a), dtype=torch.float32) for a in edge_attributes], dim=1)
    return StaticGraphProvider(torch.as_tensor(get("edge_index")), ea, src_size, dst_size, trainable_size)


class ProjectionGraphProvider(nn.Module):
    """A sparse projection matrix [destination nodes, source nodes], built from the edges of a graph or read from a scipy ``.npz`` file.

    Graph mode: entry (dst, src) = ``edge_weight_attribute`` of the edge (1 without one), times ``src_node_weight_attribute`` of the
    source node if given.  Duplicate entries are summed; ``row_normalize`` divides every non-zero row by its sum.  The arrays are plain
    attributes (``indptr`` / ``indices`` int32, ``values`` fp32, numpy), not buffers: the matrix is a constant, a state_dict carries none of
    it (the reference keeps a sparse CSR tensor as an attribute for the same reason).  ``get_edges(device=...)`` returns the
    ``ops.SparseMatrix`` of that device, copied once per device - nothing is copied inside a captured forward."""

    def __init__(self, graph=None, edges_name: Optional[tuple] = None, edge_weight_attribute: Optional[str] = None,
                 src_node_weight_attribute: Optional[str] = None, file_path=None, row_normalize: bool = False) -> None:
        super().__init__()
        from scipy.sparse import coo_matrix, load_npz

        if file_path is not None:
            for kw, val in (("src_node_weight_attribute", src_node_weight_attribute), ("edge_weight_attribute", edge_weight_attribute)):
                if val is not None:
                    LOGGER.warning("Building ProjectionGraphProvider from file, so %s='%s' will be ignored.", kw, val)
            matrix = load_npz(file_path)
        else:
            assert graph is not None and edges_name is not None, "Must provide graph and edges_name if file_path not given"
            edges_name = tuple(edges_name)
            store = graph[edges_name]
            get = lambda st, k: st[k] if isinstance(st, dict) else getattr(st, k)  # noqa: E731
            edge_index = torch.as_tensor(get(store, "edge_index")).detach().cpu().long()
            if edge_weight_attribute:
                weights = torch.as_tensor(get(store, edge_weight_attribute)).detach().cpu().reshape(-1)
            else:
                weights = torch.ones(edge_index.shape[1])
            if src_node_weight_attribute:
                node_w = torch.as_tensor(get(graph[edges_name[0]], src_node_weight_attribute)).detach().cpu().reshape(-1)
                weights = weights * node_w[edge_index[0]]
            shape = (int(_num_nodes(graph[edges_name[2]])), int(_num_nodes(graph[edges_name[0]])))
            matrix = coo_matrix((weights.to(torch.float32).contiguous().numpy(), (edge_index[1].numpy(), edge_index[0].numpy())), shape=shape,
                                dtype=np.float32)
        matrix = matrix.astype(np.float32, copy=False).tocsr()
        matrix.sum_duplicates()
        if row_normalize:
            sums = np.asarray(matrix.sum(axis=1)).ravel()
            inv = np.zeros_like(sums, dtype=np.float32)
            inv[sums != 0] = 1.0 / sums[sums != 0]  # zero rows stay zero
            matrix = matrix.multiply(inv[:, None]).tocsr()
        sums = np.asarray(matrix.sum(axis=1)).ravel()
        if not np.allclose(sums, np.ones_like(sums), atol=1e-5):
            LOGGER.warning("Projection matrix rows do not sum to 1 (min=%.4f, max=%.4f, mean=%.4f). This is unexpected; please check your "
                           "matrix. Consider using pre-normalized weights or row_normalize=True.", sums.min().item() if sums.size else 0.0,
                           sums.max().item() if sums.size else 0.0, sums.mean().item() if sums.size else 0.0)
        self.shape = (int(matrix.shape[0]), int(matrix.shape[1]))
        self.indptr = np.ascontiguousarray(matrix.indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(matrix.indices, dtype=np.int32)
        self.values = np.ascontiguousarray(matrix.data, dtype=np.float32)
        from .. import ops

        self._host = ops.build_sparse_matrix(self.indptr, self.indices, self.values, self.shape)  # checked once; carries the transpose
        self._edge_dim = self.shape[1]
        self._on_device: dict = {}

    @property
    def edge_dim(self) -> int:
        return self._edge_dim

    @property
    def is_sparse(self) -> bool:
        return True

    def _apply(self, fn, recurse=True):
        """``.to(device)`` / ``.cuda()`` of the owning model makes the device copy (the arrays are not buffers, so nothing else would):
        a forward captured without a warm-up run then finds it in place."""
        super()._apply(fn, recurse)
        dev = fn(torch.empty(0)).device
        if dev.type != "cpu":
            self.get_edges(device=dev)
        return self

    def get_edges(self, batch_size=None, src_coords=None, dst_coords=None, model_comm_group=None, shard_edges: bool = True, device=None,
                  dtype=None):
        """The matrix on ``device`` (default: the host copy).  ``dtype`` and the other keywords of the reference's interface are unused:
        the values are fp32 and the kernel accumulates in fp32 whatever the dtype of the rows."""
        if device is None:
            return self._host
        key = str(torch.device(device))
        hit = self._on_device.get(key)
        if hit is None:
            hit = self._on_device[key] = self._host.to(device)
        return hit


def _num_nodes(store) -> int:
    if isinstance(store, dict) and "num_nodes" in store:
        return store["num_nodes"]
    n = getattr(store, "num_nodes", None)
    return n if n is not None else store["x"].shape[0]
