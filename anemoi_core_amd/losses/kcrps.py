"""The ensemble loss: the reference's ``CRPS`` (training/src/anemoi/training/losses/kcrps.py) over the one fused kernel pair of
``ops.kernel_crps`` (csrc/crps.hip).  Tensors are [bs, t, ens, grid, var].

Built: 1-D fp32 scalers on the TIME, GRID and VARIABLE dimensions (several on one dimension multiply), ``ignore_nans``, ``squash`` with
"avg" / "sum".  Not built, and refused by name: scalers on other or on several dimensions, ``scaler_indices``, ``without_scalers``,
``grid_shard_slice`` / ``group`` (sharded reductions)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from .. import ops

TIME, GRID, VARIABLE = 1, 3, 4  # of [bs, t, ens, grid, var]
_DIM_NAMES = {TIME: "TIME", GRID: "GRID", VARIABLE: "VARIABLE"}
BACKENDS = ("naive", "stable")


class CRPS(nn.Module):
    """Almost-fair kernel CRPS: ``alpha`` = 0 the standard CRPS, 1 the fair one.  Both ``backend`` values select the one kernel (the two
    reference formulas have the same value); ``no_autocast`` is kept for the constructor's sake - the kernel computes in fp32 whatever
    the autocast state."""

    def __init__(self, alpha: float = 0.95, backend: str = "stable", no_autocast: bool = True, ignore_nans: bool = False, **kwargs) -> None:
        super().__init__()
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"alpha must be in the range [0, 1], got {alpha}")
        if backend not in BACKENDS:
            raise ValueError(f"Unknown CRPS backend {backend!r}. Expected one of: 'naive', 'stable'.")
        self.alpha, self.backend, self.no_autocast, self.ignore_nans = alpha, backend, no_autocast, ignore_nans
        self._scalers: dict = {}  # name -> dimension
        for dim in _DIM_NAMES:
            self.register_buffer(f"w{dim}", None, persistent=False)  # the product of the dimension's scalers

    @property
    def name(self) -> str:
        return f"crps{self.alpha:.2f}"

    def add_scaler(self, dimension, scaler: Tensor, name: Optional[str] = None) -> None:
        """Multiply the column weight by a 1-D fp32 ``scaler`` along TIME (1), GRID (3) or VARIABLE (4)."""
        if isinstance(dimension, (tuple, list)):
            if len(dimension) != 1:
                raise NotImplementedError(f"CRPS.add_scaler: a scaler over several dimensions {tuple(dimension)} is not built")
            dimension = dimension[0]
        dimension = int(dimension) % 5
        if dimension not in _DIM_NAMES:
            raise NotImplementedError(f"CRPS.add_scaler: a scaler on dimension {dimension} is not built; TIME (1), GRID (3) and VARIABLE (4) are")
        scaler = torch.as_tensor(scaler)
        if scaler.dim() != 1:
            raise NotImplementedError(f"CRPS.add_scaler: a multi-dimensional scaler {tuple(scaler.shape)} is not built; 1-D scalers are")
        if scaler.dtype != torch.float32:
            raise ValueError(f"CRPS.add_scaler: scalers are float32, got {scaler.dtype}")
        name = name or f"scaler{len(self._scalers)}"
        if name in self._scalers:
            raise ValueError(f"CRPS.add_scaler: scaler {name!r} already exists")
        old = getattr(self, f"w{dimension}")
        if old is not None and old.shape != scaler.shape:
            raise ValueError(f"CRPS.add_scaler: {tuple(scaler.shape)} against the {_DIM_NAMES[dimension]} scalers' {tuple(old.shape)}")
        self._scalers[name] = dimension
        setattr(self, f"w{dimension}", scaler.detach().clone().contiguous() if old is None else old * scaler.detach().to(old.device))

    def forward(self, y_pred: Tensor, y_target: Tensor, squash: bool = True, *, scaler_indices=None, without_scalers=None, grid_shard_slice=None,
                group=None, squash_mode: str = "avg") -> Tensor:
        for what, value in (("scaler_indices", scaler_indices), ("without_scalers", without_scalers), ("grid_shard_slice", grid_shard_slice),
                            ("group", group)):
            if value is not None and not (what == "without_scalers" and len(value) == 0):
                raise NotImplementedError(f"CRPS.forward: {what} is not built")
        w_grid = getattr(self, f"w{GRID}")
        if w_grid is None:
            raise RuntimeError("CRPS: a scaler on the GRID dimension is required; add uniform weights for plain scaling")
        return ops.kernel_crps(y_pred, y_target, w_grid, alpha=self.alpha, w_var=getattr(self, f"w{VARIABLE}"), w_time=getattr(self, f"w{TIME}"),
                               ignore_nans=self.ignore_nans, squash=squash, squash_mode=squash_mode)
