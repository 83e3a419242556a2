"""Multi-head self-attention - mirror of the reference's layers/attention.py (MultiHeadSelfAttention :41-262, get_alibi_slopes :545-565):
same constructor keywords, forward signature and state_dict keys (``lin_q``, ``lin_k``, ``lin_v``, ``projection``, ``q_norm``, ``k_norm``).

Both of the reference's ``attention_implementation`` values select the one HIP kernel (csrc/window_attention.hip), which has the
flash-attention semantics: the sliding window, softcap and ALiBi.  ``use_rotary_embeddings`` is accepted and ignored, exactly as in the
reference, whose TransformerProcessor never passes it to its blocks.  Training runs through csrc/window_attention_bwd.hip
(``autograd.WindowAttentionFunction``); ``forbid_autograd`` names the three cases the backward kernel does not cover."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor, nn

from .. import ops
from ..distributed import primitives as comm
from ..distributed.shapes import comm_rank, comm_size, model_is_distributed

_IMPLEMENTATIONS = ("flash_attention", "scaled_dot_product_attention")


def get_alibi_slopes(num_heads: int) -> Tensor:
    """Linearly decreasing ALiBi slopes (reference layers/attention.py:545-565)."""
    n = 2 ** math.floor(math.log2(num_heads))
    slope_0 = 2 ** (-8 / n)
    alibi_slopes = torch.pow(slope_0, torch.arange(1, 1 + n))
    if n < num_heads:
        slope_hat_0 = 2 ** (-4 / n)
        alibi_slopes_hat = torch.pow(slope_hat_0, torch.arange(1, 1 + 2 * (num_heads - n), 2))
        alibi_slopes = torch.cat([alibi_slopes, alibi_slopes_hat])
    return alibi_slopes


def forbid_autograd(module: nn.Module, *tensors: Optional[Tensor], dropout_p: float = 0.0, model_comm_group=None) -> None:
    """Fail before autograd would record through what the window attention's backward kernel does not cover: tensors off the GPU,
    attention dropout, and heads sharded over a model-parallel group."""
    name = type(module).__name__
    if module.training and dropout_p > 0:
        raise NotImplementedError(
            f"{name}: attention dropout (dropout_p = {dropout_p}) is not in the window attention's backward kernel, nor in its forward. "
            "Use dropout_p = 0, or eval mode for inference.")
    if not torch.is_grad_enabled():
        return
    params = list(module.parameters())
    if not (any(t is not None and t.requires_grad for t in tensors) or any(p.requires_grad for p in params)):
        return
    if any(t is not None and not t.is_cuda for t in (*tensors, *params)):
        raise NotImplementedError(
            f"{name}: training through the window attention needs its HIP backward kernel, which runs on the GPU only - there is no CPU "
            "fallback. Move the module and its input to the device, or run inference under torch.no_grad() / torch.inference_mode().")
    if model_is_distributed(model_comm_group):
        raise NotImplementedError(
            f"{name}: training with the heads sharded over a model-parallel group is not supported - the backward kernel is built for "
            "unsharded heads only. Train on one GPU per model instance, or run inference under torch.no_grad().")


class MultiHeadSelfAttention(nn.Module):
    """Multi-head self-attention over (batch grid) rows with a sliding window of half-width ``window_size``.  Differentiable on the GPU:
    the q|k|v GEMM, the qk-norm LayerNorms and the window attention each run their HIP backward kernel."""

    def __init__(self, num_heads: int, embed_dim: int, layer_kernels, attn_channels: Optional[int] = None, qkv_bias: bool = False,
                 qk_norm: bool = False, is_causal: bool = False, window_size: Optional[int] = None, dropout_p: float = 0.0,
                 attention_implementation: str = "flash_attention", softcap: Optional[float] = None, use_alibi_slopes: bool = False,
                 use_rotary_embeddings: bool = False):
        super().__init__()
        self.attn_channels = embed_dim if attn_channels is None else attn_channels
        if self.attn_channels <= 0:
            raise ValueError(f"attn_channels must be > 0, got {self.attn_channels}")
        if self.attn_channels % num_heads != 0:
            raise ValueError(f"attn_channels ({self.attn_channels}) must be divisible by number of heads ({num_heads})")
        if attention_implementation not in _IMPLEMENTATIONS:
            raise ValueError(f"backend '{attention_implementation}' not supported; use one of {_IMPLEMENTATIONS}")
        if is_causal:
            raise NotImplementedError("causal attention is not used by the reference's processors")
        self.attention_implementation = attention_implementation
        self.use_alibi_slopes = use_alibi_slopes
        self.num_heads = num_heads
        self.head_dim = self.attn_channels // num_heads
        self.window_size = window_size
        self.dropout_p = dropout_p
        self.is_causal = is_causal
        self.qk_norm = qk_norm
        self.softcap = softcap
        self.use_rotary_embeddings = use_rotary_embeddings  # inert, as in the reference (see the module docstring)
        # a plain attribute, not a buffer: the reference's state_dict has no slopes
        self.alibi_slopes = get_alibi_slopes(num_heads) if use_alibi_slopes else None
        self._slopes_dev: dict = {}

        Linear = layer_kernels.Linear
        self.lin_q = Linear(embed_dim, self.attn_channels, bias=qkv_bias)
        self.lin_k = Linear(embed_dim, self.attn_channels, bias=qkv_bias)
        self.lin_v = Linear(embed_dim, self.attn_channels, bias=qkv_bias)
        self.projection = Linear(self.attn_channels, embed_dim, bias=True)
        if self.qk_norm:
            self.q_norm = layer_kernels.QueryNorm(self.head_dim)
            self.k_norm = layer_kernels.KeyNorm(self.head_dim)

    def slopes(self, device, heads: Optional[slice] = None) -> Optional[Tensor]:
        """fp32 ALiBi slopes on ``device`` (copied once per device and head slice: nothing is copied inside a captured forward)."""
        if self.alibi_slopes is None:
            return None
        key = (str(device), None if heads is None else (heads.start, heads.stop))
        t = self._slopes_dev.get(key)
        if t is None:
            s = self.alibi_slopes if heads is None else self.alibi_slopes[heads]
            t = self._slopes_dev[key] = s.to(device=device, dtype=torch.float32).contiguous()
        return t

    def _window(self) -> int:
        return -1 if self.window_size is None else int(self.window_size)

    def attend(self, q: Tensor, k: Tensor, v: Tensor, batch_size: int, shard_sizes=None, model_comm_group=None,
               qkv: Optional[Tensor] = None) -> Tensor:
        """The attention of q, k, v [rows, A] (column slices of one projection are read in place) -> [rows, A], before ``projection``.
        ``qkv``: the [rows, 3A] buffer q, k, v are the thirds of; under autograd it receives ONE gradient written by the backward kernels."""
        H, d = self.num_heads, self.head_dim
        if qkv is not None and not self.qk_norm and ops._needs_grad(qkv) and not model_is_distributed(model_comm_group):
            from ..autograd import window_attention_qkv

            return window_attention_qkv(qkv, H, self._window(), softcap=self.softcap if self.softcap else None,
                                        alibi_slopes=self.slopes(qkv.device), batch_size=batch_size)
        if self.qk_norm:  # per-head LayerNorm over d, no bias (attention.py:206-208)
            q = self.q_norm(q.reshape(-1, H, d)).view(-1, H * d)
            k = self.k_norm(k.reshape(-1, H, d)).view(-1, H * d)
        softcap = self.softcap if self.softcap else None
        if not model_is_distributed(model_comm_group):
            return ops.window_attention(q, k, v, H, self._window(), softcap=softcap, alibi_slopes=self.slopes(q.device), batch_size=batch_size)
        # heads sharded for the attention (attention.py:190-227): local rows x all heads -> all rows x H / P heads -> kernel -> back
        P, rank = comm_size(model_comm_group), comm_rank(model_comm_group)
        if batch_size != 1:
            raise ValueError("Only batch size of 1 is supported when the model is sharded across GPUs")
        if H % P:
            raise ValueError(f"num_heads ({H}) must be divisible by the model-parallel size ({P})")
        Hl, n_loc, A = H // P, q.shape[0], H * d
        sizes = list(shard_sizes)

        def to_heads(t):  # [n_loc, A] all heads -> [n_full, Hl*d] this rank's heads
            send = t.reshape(n_loc, P, Hl * d).permute(1, 0, 2).reshape(P * n_loc, Hl * d)
            return comm.all_to_all_rows(send, [n_loc] * P, sizes, model_comm_group)

        heads = slice(rank * Hl, (rank + 1) * Hl)
        o = ops.window_attention(to_heads(q), to_heads(k), to_heads(v), Hl, self._window(), softcap=softcap,
                                 alibi_slopes=self.slopes(q.device, heads))
        back = comm.all_to_all_rows(o, sizes, [n_loc] * P, model_comm_group)  # [P * n_loc, Hl*d]: block r = the heads of rank r
        return back.reshape(P, n_loc, Hl * d).permute(1, 0, 2).reshape(n_loc, A)

    def forward(self, x: Tensor, grid_shard_sizes, batch_size: int, model_comm_group=None) -> Tensor:
        forbid_autograd(self, x, dropout_p=self.dropout_p, model_comm_group=model_comm_group)
        w = torch.cat([self.lin_q.weight, self.lin_k.weight, self.lin_v.weight], 0)
        b = None if self.lin_q.bias is None else torch.cat([self.lin_q.bias, self.lin_k.bias, self.lin_v.bias])
        qkv = ops.linear(x, w, b)
        A = self.attn_channels
        o = self.attend(qkv[:, :A], qkv[:, A:2 * A], qkv[:, 2 * A:], batch_size, grid_shard_sizes.nodes, model_comm_group, qkv=qkv)
        return ops.linear(o, self.projection.weight, self.projection.bias)
