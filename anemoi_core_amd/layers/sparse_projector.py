"""SparseProjector - mirror of the reference's layers/sparse_projector.py: applies a sparse projection matrix to node rows.

The reference permutes [B, N, C] to [N, B C], calls ``torch.sparse.mm`` and permutes back; here the projection is ONE launch of
``ops.sparse_project`` (csrc/sparse_project.hip), which reads the rows where they are and folds the batch entries in as columns."""
from __future__ import annotations

from typing import Optional

from torch import Tensor, nn

from .. import ops


class SparseProjector(nn.Module):
    """Stateless: the matrix (a ``ProjectionGraphProvider`` or an ``ops.SparseMatrix``) is passed to ``forward``.

    ``autocast`` and ``num_chunks`` are accepted for configuration compatibility and are inert: accumulation is always fp32 (whatever
    the dtype of the rows), and chunking is a memory feature of the reference's permute copies that this path does not make."""

    def __init__(self, autocast: bool = False, num_chunks: int = 1) -> None:
        super().__init__()
        self.autocast = autocast
        self.num_chunks = num_chunks

    def forward(self, x: Tensor, projection_matrix, num_chunks: Optional[int] = None, *, cols: Optional[Tensor] = None,
                mul: Optional[Tensor] = None, add: Optional[Tensor] = None, out_dtype=None) -> Tensor:
        """x [..., input_nodes, channels] -> [..., output_nodes, channels] (or the ``cols`` selection of the channels, each value mapped
        through ``v * mul + add`` before it is summed)."""
        if hasattr(projection_matrix, "get_edges"):
            projection_matrix = projection_matrix.get_edges(device=x.device)
        return ops.sparse_project(x, projection_matrix, cols, mul, add, out_dtype)
