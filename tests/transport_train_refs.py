"""Float64 restatements of the three backward kernels of the EDM denoiser edges (csrc/transport_bwd.hip), each with its componentwise
error bound - computed from the operands, not chosen (the habit of tests/transport_refs.py) - the same three edges written as
differentiable torch operations (the "restated route": the yardstick of the bf16 training test and of tools/transport_train_time.py), and
the shared pieces of the training tests: the fixture with its gradient parts, this package's model of a case.

Rounding units as in tests/transport_refs.py: u = 2^-24 (fp32), 2^-8 (bf16), 2^-11 (fp16).  An n-term fp32 sum, in whatever order, is off
by at most gamma_n = n u / (1 - n u) of the summed magnitudes.

  noise_cond_bwd:  s_g sums n = rows_0 + rows_1 values that are exact in fp32: gamma_n of their magnitudes.  The recomputed e, p, h carry
    the forward's errors (tests/transport_refs.py, kernel 1): d_e = 2^-23 |arg| + 2 u, d_p through |W1| with (C + 2) u of the accumulated
    magnitude, d_h = 1.1 d_p + 4 u |h|.  Products and fused multiply-adds are carried as |a| d_b + d_a (|b| + d_b) plus gamma_(terms + 1)
    of the accumulated magnitudes.  silu'(p) = sig (1 + p (1 - sig)): its second derivative is at most 1 / 2 in magnitude, so the error of p
    costs d_p / 2; its own evaluation - exp within 2 ulp, a sum, a quotient (sig: <= 8 u), the difference 1 - sig (<= 9 u absolute), the
    product with p, a sum, the product with sig - is bounded by 20 u (1 + |p|).
  transport_assemble_input_bwd:  a G-term fp32 sum of values exact in fp32: gamma_G of the magnitudes, then one rounding of the output dtype.
  edm_output_bwd:  c_out costs five fp32 roundings (square, sum, root, product, quotient), the cast of d_out one, the product one: 8 u of the
    magnitude (the rearrange-only mode: the cast alone, u), then one rounding of the output dtype.  The extra columns are exact zeros.
"""
from __future__ import annotations

import contextlib
import os

import torch

from tests.transport_refs import GOLDEN, U, edm_coefficients


def gamma(n: int) -> float:
    u = U[torch.float32]
    return n * u / (1 - n * u)


# ---------------------------------------------------------------------------------------------- fixture
def load_train_fixture() -> dict:
    """tests/golden/transport_train.pt with the gradients of its part files put back: fx["models"][case]["grads"] = {parameter: float64
    gradient rounded to fp32}."""
    fx = torch.load(os.path.join(GOLDEN, "transport_train.pt"), weights_only=False)
    for part in fx["parts"]:
        for key, g in torch.load(os.path.join(GOLDEN, part), weights_only=False).items():
            case, name = key.split("/", 1)
            fx["models"][case].setdefault("grads", {})[name] = g
    return fx


def training_model(fx: dict, name: str):
    """(model, x, target) of case ``name``, parameters and inputs drawn as the generator drew them; the case's training_condition is set."""
    from tests.transport_refs import transport_model

    rec = fx["models"][name]
    model, x, _, _, _ = transport_model(fx, name)
    model.training_condition = dict(rec["training_condition"])
    case = rec["case"]
    target = torch.randn(x.shape[0], case.get("n_step_output", 1), 1, x.shape[3], case.get("n_vars_out", 4),
                         generator=torch.Generator().manual_seed(rec["target_seed"]))
    return model, x, target


# ---------------------------------------------------------------------------------------------- backward 1: noise conditioning
def noise_cond_pieces(values, freq, pi, w1, b1, log_quarter: bool) -> dict:
    """e, p, h of every group in float64 with the bounds of what the device's fp32 evaluation may be off by (CPU tensors)."""
    u = U[torch.float32]
    v = values.to(torch.float32)
    if log_quarter:
        v = v.log() / 4.0
    arg32 = v[:, None] * freq.float()[None, :]
    if pi is not None:
        arg32 = arg32 * 2 * pi.float()
    arg = arg32.double()
    e = torch.cat([arg.sin(), arg.cos()], dim=-1)
    d_e = (2.0**-23 * arg.abs() + 2 * u).repeat(1, 2)
    W1, B1 = w1.double(), b1.double()
    C = W1.shape[1]
    p = e @ W1.T + B1
    d_p = d_e @ W1.abs().T + (C + 2) * u * (e.abs() @ W1.abs().T + B1.abs())
    h = p * torch.sigmoid(p)
    return dict(e=e, d_e=d_e, p=p, d_p=d_p, h=h, d_h=1.1 * d_p + 4 * u * h.abs())


def noise_cond_bwd_ref(d_outs, rows, values, freq, pi, w1, b1, w2, b2, log_quarter: bool):
    """({name: float64 gradient}, {name: bound}) for d_w1, d_b1, d_w2, d_b2 and s (the per-group sums [G, cond_dim]).  d_outs[k]: [G rows[k],
    cond_dim] holding the values the kernel reads, or None."""
    u = U[torch.float32]
    G, cd = values.numel(), w2.shape[0]
    s, s_abs, n = torch.zeros(G, cd, dtype=torch.float64), torch.zeros(G, cd, dtype=torch.float64), 0
    for d, r in zip(d_outs, rows):
        if d is None or r == 0:
            continue
        d = d.double().reshape(G, r, cd)
        s, s_abs, n = s + d.sum(1), s_abs + d.abs().sum(1), n + r
    d_s = gamma(max(n, 1)) * s_abs
    f = noise_cond_pieces(values, freq, pi, w1, b1, log_quarter)
    e, d_e, p, d_p, h, d_h = (f[k] for k in ("e", "d_e", "p", "d_p", "h", "d_h"))
    W2 = w2.double()
    mag = lambda a, da: a.abs() + da  # noqa: E731
    out, bound = {"s": s}, {"s": d_s}
    out["d_b2"] = s.sum(0)
    bound["d_b2"] = d_s.sum(0) + gamma(G) * mag(s, d_s).sum(0)
    out["d_w2"] = s.T @ h
    bound["d_w2"] = s.abs().T @ d_h + d_s.T @ mag(h, d_h) + gamma(G + 1) * (mag(s, d_s).T @ mag(h, d_h))
    dh = s @ W2
    d_dh = d_s @ W2.abs() + gamma(cd + 1) * (mag(s, d_s) @ W2.abs())
    sig = torch.sigmoid(p)
    fp = sig * (1 + p * (1 - sig))
    d_fp = 0.5 * d_p + 20 * u * (1 + p.abs())
    dp = dh * fp
    d_dp = d_dh * mag(fp, d_fp) + dh.abs() * d_fp + u * mag(dh, d_dh) * mag(fp, d_fp)
    out["d_b1"] = dp.sum(0)
    bound["d_b1"] = d_dp.sum(0) + gamma(G) * mag(dp, d_dp).sum(0)
    out["d_w1"] = dp.T @ e
    bound["d_w1"] = dp.abs().T @ d_e + d_dp.T @ mag(e, d_e) + gamma(G + 1) * (mag(dp, d_dp).T @ mag(e, d_e))
    return out, bound


# ---------------------------------------------------------------------------------------------- backward 2: input assembly
def assemble_input_bwd_ref(d_rows, col0: int, n_nodes: int, n_attrs: int):
    """(d_attrs [N, A] float64, its bound): d_rows [G N, >= col0 + A] holding the values the kernel reads; the result has d_rows' dtype."""
    G = d_rows.shape[0] // n_nodes
    blk = d_rows.double()[:, col0:col0 + n_attrs].reshape(G, n_nodes, n_attrs)
    out, acc = blk.sum(0), gamma(G) * blk.abs().sum(0)
    return out, acc + U[d_rows.dtype] * (out.abs() + acc)


# ---------------------------------------------------------------------------------------------- backward 3: output assembly
def edm_output_bwd_ref(d_out, sigma, sigma_data: float, n_cols: int, pred_dtype):
    """(d_pred [B E N, n_cols] float64, its bound): d_out [B, T, E, N, V] fp32 / fp64 (any strides), sigma [B E] or None (the rearrange alone).
    The bound of the columns beyond T V is 0: they are exact zeros."""
    B, T, E, N, V = d_out.shape
    d = d_out.double().permute(0, 2, 3, 1, 4).reshape(B * E * N, T * V)
    if sigma is None:
        val, acc = d, U[torch.float32] * d.abs() * (d_out.dtype == torch.float64)
    else:
        c_out = edm_coefficients(sigma, sigma_data)[2].repeat_interleave(N)[:, None]
        val = c_out * d
        acc = 8 * U[torch.float32] * val.abs()
    acc = acc + U[pred_dtype] * (val.abs() + acc)
    pad = n_cols - T * V
    return torch.nn.functional.pad(val, (0, pad)), torch.nn.functional.pad(acc, (0, pad))


# ---------------------------------------------------------------------------------------------- the restated route
def _compute_dtype(t: torch.Tensor):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def noise_cond_torch(values, frequencies, w1, b1, w2, b2, *, pi=None, log_quarter=False, rows=(1,), out_dtype=None, keep=None) -> tuple:
    """``ops.noise_cond`` as differentiable torch operations, evaluated in float64 when the weights are float64 and in fp32 otherwise.
    ``keep``: a dict that receives the conditioning vector [G, cond_dim] under "cond" (gradient retained when it has one)."""
    ct = _compute_dtype(w1)
    v = values.reshape(-1).to(ct)
    if log_quarter:
        v = v.log() / 4.0
    arg = v[:, None] * frequencies.to(ct)[None, :]
    if pi is not None:
        arg = arg * 2 * pi.to(ct)
    e = torch.cat([arg.sin(), arg.cos()], dim=-1)
    p = e @ w1.to(ct).T + b1.to(ct)
    cond = (p * torch.sigmoid(p)) @ w2.to(ct).T + b2.to(ct)
    if keep is not None:
        if cond.requires_grad:
            cond.retain_grad()
        keep["cond"] = cond
    out_dtype = out_dtype or w1.dtype
    return tuple(None if r == 0 else cond.to(out_dtype).repeat_interleave(r, dim=0) for r in rows)


def _coefficients_torch(sigma, sigma_data: float, ct):
    s = sigma.reshape(-1).to(ct)
    t = s * s + sigma_data**2
    return 1.0 / t.sqrt(), sigma_data**2 / t, s * sigma_data / t.sqrt()


def assemble_input_torch(x, y, attrs, width: int, *, sigma=None, sigma_data: float = 1.0, out_dtype=None, out=None):
    """``ops.transport_assemble_input`` as differentiable torch operations."""
    assert out is None
    B, _, E, N, _ = x.shape
    ct = _compute_dtype(x)
    flat = lambda t: t.to(ct).permute(0, 2, 3, 1, 4).reshape(B * E * N, -1)  # noqa: E731
    yf = flat(y)
    if sigma is not None:
        yf = yf * _coefficients_torch(sigma, sigma_data, ct)[0].repeat_interleave(N)[:, None]
    out_dtype = out_dtype or (attrs.dtype if attrs is not None else x.dtype)
    cols = [flat(x).to(out_dtype), yf.to(out_dtype)] + ([] if attrs is None else [attrs.to(out_dtype).repeat(B * E, 1)])
    rows = torch.cat(cols, dim=-1)
    return torch.nn.functional.pad(rows, (0, width - rows.shape[1]))


def edm_output_torch(pred, y, sigma, shape, *, sigma_data: float = 1.0, out_dtype=torch.float32, out=None):
    """``ops.edm_output`` as differentiable torch operations."""
    assert out is None
    B, T, E, N, V = shape
    ct = _compute_dtype(pred)
    p = pred[:, :T * V].to(ct).reshape(B, E, N, T, V).permute(0, 3, 1, 2, 4)
    if y is None:
        return p.to(out_dtype).contiguous()
    _, c_skip, c_out = _coefficients_torch(sigma, sigma_data, ct)
    return (c_skip.view(B, 1, E, 1, 1) * y.to(ct) + c_out.view(B, 1, E, 1, 1) * p).to(out_dtype)


@contextlib.contextmanager
def restated_edges():
    """Inside, ``ops.noise_cond`` / ``ops.transport_assemble_input`` / ``ops.edm_output`` are the torch restatements above: a model's forward
    and backward take the restated route around the same network."""
    from anemoi_core_amd import ops

    real = (ops.noise_cond, ops.transport_assemble_input, ops.edm_output)
    ops.noise_cond, ops.transport_assemble_input, ops.edm_output = noise_cond_torch, assemble_input_torch, edm_output_torch
    try:
        yield
    finally:
        ops.noise_cond, ops.transport_assemble_input, ops.edm_output = real


def training_loss(model, x, y_noised, sigma, weights, target):
    """mean(w (D - target)^2) of one dataset named "data": the loss the fixture records."""
    D = model({"data": x}, {"data": y_noised}, {"data": sigma})["data"]
    return (weights * (D - target) ** 2).mean()
