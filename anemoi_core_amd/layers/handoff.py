"""What a launch leaves for the consumer of its output rows (inference): that consumer's projection of the rows, the row statistics its
LayerNorm fold needs, or - sharded - the k|v rows of the next halo exchange.  A ``Handoff`` travels in the forward's ``Carrier`` and is
taken by the consumer whose input rows it describes."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch
from torch import Tensor, nn


@dataclass
class Handoff:
    rows: Tensor                    # the rows it describes (by identity)
    proj: Optional[Tensor] = None   # the consumer's projection of them (q|k|v|self, k|v, q|self, GraphConv's p; sharded: q|self)
    stats: Optional[Tensor] = None  # or their row statistics for a LayerNorm fold (ops.linear_with_row_stats)
    kv: Optional[Tensor] = None     # sharded: the [local + halo, 2A] k|v buffer, local rows filled, halo rows for the exchange


@dataclass
class Carrier:
    """Per-forward: the next consumer of the rows a block produces, the decoder's extractor (LayerNorm, Linear) that may ride on its block's
    tail and that tail's result, and the hand-offs not yet taken."""
    next_block: Optional[nn.Module] = None
    tail_proj: Optional[tuple] = None
    tail_out: Optional[Tensor] = None
    handoffs: list = field(default_factory=list)

    def put(self, rows: Tensor, **what) -> Tensor:
        self.handoffs.append(Handoff(rows, **what))
        return rows

    def take(self, x: Tensor) -> Optional[Handoff]:
        """The hand-off that describes ``x``, removed from the carrier; None if there is none."""
        i = next((i for i, h in enumerate(self.handoffs) if h.rows is x), None)
        return None if i is None else self.handoffs.pop(i)


def plain_layer_norm(ln) -> bool:
    """An affine LayerNorm without conditioning: what the folds and chain kernels apply."""
    return type(ln).__name__ in ("LayerNorm", "AutocastLayerNorm") and ln.weight is not None


def inference_in(x: Tensor, *mods) -> bool:
    """No gradient needed (the chain and fold launches build no autograd graph) and every parameter of ``mods`` in x's dtype (mixed layouts
    take the GEMM launches; the chain ops raise on them)."""
    ps = [p for m in mods for p in m.parameters()]
    return all(p.dtype == x.dtype for p in ps) and not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps)))
