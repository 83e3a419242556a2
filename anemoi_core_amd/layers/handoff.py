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


def side_schedule(host_rows: int, side_panels_left: int, panels_per_rider: int) -> int:
    """How many of a side job's remaining 48-row panels ride on a block-tail launch over ``host_rows`` rows: ``panels_per_rider`` for every
    compute unit the launch leaves idle, per round of its panels (a tail of several rounds lasts that many times longer); 0 for a launch
    that keeps every compute unit busy.  Pure: the hosting decision is this function and nothing else."""
    from ..ops import CHAIN_CHANNELS, chain_plan

    if host_rows <= 0 or side_panels_left <= 0 or panels_per_rider <= 0:
        return 0
    tail = chain_plan("block_tail", host_rows, hidden=CHAIN_CHANNELS)  # (the grid of a tail does not depend on its widths)
    return min(side_panels_left, tail.idle_cus * panels_per_rider * tail.rounds)


@dataclass
class SideJob:
    """A row-chain job (ops.gt_row_chain's operands, outputs preallocated) that does not depend on the launches between its creation and
    its consumer: its panels ride on those launches' idle compute units (``ops.gt_layer_chain2(..., side=...)``), ``cursor`` panels so far."""
    x: Tensor
    we: Tensor
    wqg: Tensor
    vec: Tensor
    q_out_features: int
    ln_eps: float
    y: Tensor
    q: Tensor
    panels_per_rider: int = 4
    cursor: int = 0
    hosted: int = 0  # panels that rode on other launches

    @property
    def n_panels(self) -> int:
        from ..ops import row_chain_panels

        return row_chain_panels(self.x.shape[0], self.x.shape[1], self.q_out_features)

    def slice_for(self, host_rows: int):
        """The next panels for a block-tail launch over ``host_rows`` rows as an ``ops.ChainSide`` (None: none), taken off the job."""
        from .. import ops

        n = side_schedule(host_rows, self.n_panels - self.cursor, self.panels_per_rider)
        if n <= 0:
            return None
        side = ops.ChainSide(self.x, self.we, self.wqg, self.vec, self.q_out_features, self.ln_eps, self.y, self.q, first_panel=self.cursor, panels=n)
        self.cursor += n
        self.hosted += n
        return side

    def finish(self) -> None:
        """The panels no launch hosted, as one launch of their own."""
        from .. import ops

        if self.cursor < self.n_panels:
            ops.gt_row_chain_panels(self.x, self.we, self.wqg, self.vec, self.q_out_features, self.ln_eps, self.y, self.q, self.cursor,
                                    self.n_panels - self.cursor)
        self.cursor = self.n_panels


@dataclass
class Carrier:
    """Per-forward: the next consumer of the rows a block produces, the decoder's extractor (LayerNorm, Linear) that may ride on its block's
    tail and that tail's result, the hand-offs not yet taken, and a side job whose panels ride on the block tails."""
    next_block: Optional[nn.Module] = None
    tail_proj: Optional[tuple] = None
    tail_out: Optional[Tensor] = None
    handoffs: list = field(default_factory=list)
    static_dst: Optional[Tensor] = None  # the encoder's destination rows when they are a static tensor (the hidden mesh's cached attributes)
    side_job: Optional[SideJob] = None  # work for the idle compute units of the block tails on the way (the decoder's destination side)

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
