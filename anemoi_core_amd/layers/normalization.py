"""Normalisation layers - mirror of the reference's ``anemoi.models.layers.normalization`` (AutocastLayerNorm :19-31,
ConditionalLayerNorm :34-94) on the HIP kernels, plus the one call site (``apply_layer_norm``) the blocks use for whichever of
them a ``layer_kernels`` config selected."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .. import ops
from .kernels import LayerNorm, Linear, PaddedLinear


class AutocastLayerNorm(LayerNorm):
    """Reference layers/normalization.py:19-31: output in the input dtype — always true for the HIP kernel."""


# Conditioning widths ConditionalLayerNorm sends to the in-kernel modulation.  The kernel takes up to ops.COND_PROJ_MAX = 32, but beyond 4 its
# weights live in LDS and the 2 C FMAs per element (plus the 16-bit -> fp32 conversions of the weights) are VALU work the GEMM does on the
# matrix cores.  Measured (tools/ens_time.py, profiles/r08_ens_time.json: 40 968 rows, bf16, us without / with residual, fused against
# two-step): C = 4: 22.0 / 25.8 against 77.7 / 95.9 (D = 512), 42.1 / 49.7 against 136.0 / 183.1 (D = 1024); C = 16: 50.0 / 50.8 against
# 68.5 / 86.7 and 98.7 / 101.3 against 131.7 / 176.8; C = 32: 88.0 / 89.7 against 68.2 / 87.6 and 207.1 / 216.0 against 131.6 / 177.0 -
# slower beyond the run-to-run spread (<= 1.8 us), so the route stops at 16.
COND_PROJ_ROUTE_MAX = 16


class ConditionalLayerNorm(nn.Module):
    """Reference layers/normalization.py:34-94: ``LN(x) * (scale(cond) + 1) + bias(cond)``, same parameters and
    state_dict keys (``scale.*``, ``bias.*``; ``norm`` has none).  At inference, for a conditioning width up to COND_PROJ_ROUTE_MAX = 16,
    the two Linear maps of the conditioning are computed INSIDE the LayerNorm kernel (one launch, no modulation tensor); under autograd (and for wider
    conditionings) they run as ONE fused GEMM [N, 2D] whose halves feed the modulated LayerNorm kernel (forward and backward)."""

    def __init__(self, normalized_shape, condition_shape: int = 16, zero_init: bool = True, autocast: bool = True) -> None:
        super().__init__()
        D = normalized_shape if isinstance(normalized_shape, int) else int(tuple(normalized_shape)[0])
        self.norm = nn.LayerNorm(D, elementwise_affine=False)
        self.scale = Linear(condition_shape, D)
        self.bias = Linear(condition_shape, D)
        self.autocast = autocast
        self.eps = self.norm.eps
        if zero_init:
            for lin in (self.scale, self.bias):
                nn.init.zeros_(lin.weight)
                nn.init.zeros_(lin.bias)
        self._pad = PaddedLinear()
        self._proj = _ProjWeights()

    def _proj_route_ok(self, x: Tensor, cond: Tensor) -> bool:
        """The modulation computed inside the LayerNorm kernel (``ops.cond_layer_norm_proj``, one launch): inference, a conditioning
        width at which it was measured faster than the two-step route (COND_PROJ_ROUTE_MAX).  Under autograd the GEMM +
        ``CondLayerNormFunction`` path below stays as it is."""
        return (x.is_cuda and 0 < cond.shape[-1] <= COND_PROJ_ROUTE_MAX and self.scale.bias is not None and self.bias.bias is not None
                and not ops._needs_grad(x, cond, self.scale.weight, self.scale.bias, self.bias.weight, self.bias.bias))

    def forward(self, x: Tensor, cond: Tensor, residual: Tensor | None = None) -> Tensor:  # noqa: D102
        D = x.shape[-1]
        if self._proj_route_ok(x, cond):
            w, b = self._proj.get(self)
            c2 = cond.reshape(-1, cond.shape[-1])
            c2 = c2 if c2.dtype == w.dtype else c2.to(w.dtype)
            # the residual rides in the launch when nothing is cast between the LayerNorm and the add
            fused_res = residual is not None and x.dtype == w.dtype and residual.dtype == w.dtype
            y = ops.cond_layer_norm_proj(x.reshape(-1, D).to(w.dtype), c2, w, b, self.eps, residual.reshape(-1, D) if fused_res else None).view(x.shape)
            y = y.to(x.dtype) if self.autocast else y
            return y if residual is None or fused_res else y + residual
        w = torch.cat([self.scale.weight, self.bias.weight], 0)
        b = torch.cat([self.scale.bias, self.bias.bias], 0)
        c2 = cond.reshape(-1, cond.shape[-1]).to(w.dtype)
        pad = (-c2.shape[1]) % 8
        if pad and c2.dtype != torch.float32:  # 16-bit operand rows must be 16-byte aligned
            c2, w = torch.nn.functional.pad(c2, (0, pad)), torch.nn.functional.pad(w, (0, pad))
        mod = ops.linear(c2, w, b)  # [N, 2D] = [scale | shift]
        y = ops.cond_layer_norm(x.reshape(-1, D).to(w.dtype), mod[:, :D], mod[:, D:], self.eps).view(x.shape)
        y = y.to(x.dtype) if self.autocast else y
        return y if residual is None else y + residual


class _ProjWeights:
    """The prepared operands of ``ops.cond_layer_norm_proj`` (C-major image of [scale.weight ; bias.weight] and the two biases), rebuilt
    only when one of the four parameters changes - the keyed builder the blocks' ``_FusedWeights`` use."""

    def __init__(self):
        self._fused = None

    def get(self, ln: "ConditionalLayerNorm"):
        if self._fused is None:
            from .block import _FusedWeights  # (block.py imports this module)

            self._fused = _FusedWeights()
        ps = [ln.scale.weight, ln.scale.bias, ln.bias.weight, ln.bias.bias]
        return self._fused.derived("cond_proj", ps, lambda: ops.cond_layer_norm_proj_weights(*ps))


def apply_layer_norm(ln: nn.Module, x: Tensor, cond: Tensor | None = None, residual: Tensor | None = None) -> Tensor:
    """One call site for both kinds of normalisation layer a ``layer_kernels`` config can select."""
    if isinstance(ln, ConditionalLayerNorm):
        if cond is None:
            raise ValueError("ConditionalLayerNorm needs the conditioning tensor (cond=...)")
        return ln(x, cond, residual)
    return ops.layer_norm(x, ln.weight, ln.bias, ln.eps, residual)
