"""Float64 restatements of the four EDM diffusion kernels (csrc/transport.hip) and of both samplers, with the componentwise error
bound of each kernel - computed from the operands, not chosen (the habit of tests/chain_refs.py) - plus the shared pieces of the transport
tests: the fixture, this package's model built from one of its cases, the substitution of recorded random numbers.

Rounding units: u = 2^-p for a significand of p bits - 2^-24 (fp32), 2^-8 (bf16), 2^-11 (fp16), 2^-53 (fp64): the largest relative error of
one rounding to nearest.

  kernel 1 (noise_cond): the argument of sin / cos is formed in fp32 in the reference's order - the restatement forms it the same way - so what
    is left is the device's log (transform 1) and sin / cos against the exact ones: |d arg| <= 2^-23 |arg| and two units on the value.
    That is carried through the absolute-value matrix products, with (C + 2) u of each accumulated magnitude for the fp32 dot products, and
    through SiLU (Lipschitz constant <= 1.1, four units for its own evaluation); one rounding of the output dtype closes it.
  kernels 2, 3 (edges): a coefficient costs at most four fp32 roundings (square, sum, root, quotient), the cast of y one, each product one and
    the sum one: <= 7 on any term, bounded as 8 u (|c_skip y| + |c_out pred|) (8 u |c_in y| for the input), plus one rounding of the
    output dtype.  Copied values (x, the attributes, the padding zeros) are exact up to that last rounding.
  kernel 4 (update): every mode is at most seven operations deep: 16 u_solver of the summed magnitudes of its terms; the DPM++ modes
    with the data-dtype rounding switched on add one fp32 rounding of the result.
"""
from __future__ import annotations

import os

import torch

U = {torch.float32: 2.0**-24, torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float64: 2.0**-53}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEUN_PREDICT, HEUN_CORRECT, HEUN_FINAL, DPMPP_FIRST, DPMPP_MULTI, DPMPP_FINAL = range(6)


def load_fixture() -> dict:
    return torch.load(os.path.join(GOLDEN, "transport.pt"), weights_only=False)


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


# ---------------------------------------------------------------------------------------------- kernel 1
def noise_cond_ref(values, freq, pi, w1, b1, w2, b2, log_quarter: bool, out_dtype):
    """(cond [G, cond_dim] float64, its bound).  All arguments are CPU tensors holding the values the kernel reads."""
    u = U[torch.float32]
    v = values.to(torch.float32)
    if log_quarter:
        v = v.log() / 4.0
    arg32 = v[:, None] * freq.float()[None, :]
    if pi is not None:
        arg32 = arg32 * 2 * pi.float()
    arg = arg32.double()
    emb = torch.cat([arg.sin(), arg.cos()], dim=-1)
    d_emb = (2.0**-23 * arg.abs() + 2 * u).repeat(1, 2)
    W1, B1, W2, B2 = w1.double(), b1.double(), w2.double(), b2.double()
    C = W1.shape[1]
    pre = emb @ W1.T + B1
    d_pre = d_emb @ W1.abs().T + (C + 2) * u * (emb.abs() @ W1.abs().T + B1.abs())
    hid = pre * torch.sigmoid(pre)
    d_hid = 1.1 * d_pre + 4 * u * hid.abs()
    cond = hid @ W2.T + B2
    d_cond = d_hid @ W2.abs().T + (C + 2) * u * (hid.abs() @ W2.abs().T + B2.abs())
    return cond, d_cond + U[out_dtype] * (cond.abs() + d_cond)


# ---------------------------------------------------------------------------------------------- kernels 2, 3
def edm_coefficients(sigma, sigma_data: float):
    """(c_in, c_skip, c_out) float64 [G] of sigma as the kernels read it: cast to fp32 first."""
    s = sigma.reshape(-1).to(torch.float32).double()
    t = s * s + sigma_data**2
    return 1.0 / t.sqrt(), sigma_data**2 / t, s * sigma_data / t.sqrt()


def assemble_input_ref(x, y, attrs, width: int, sigma, sigma_data: float, out_dtype):
    """(out [B E N, width] float64, its bound): x [B, T_in, E, N, V_in], y [B, T_out, E, N, V_out], attrs [N, A] or None, sigma [B E] or None."""
    B, _, E, N, _ = x.shape
    flat = lambda t: t.double().permute(0, 2, 3, 1, 4).reshape(B * E * N, -1)  # noqa: E731  "(batch ensemble grid) (time vars)"
    xf, yf = flat(x), flat(y)
    c_in = torch.ones(B * E, dtype=torch.float64) if sigma is None else edm_coefficients(sigma, sigma_data)[0]
    ys = yf * c_in.repeat_interleave(N)[:, None]
    cols = [xf, ys] + ([] if attrs is None else [attrs.double().repeat(B * E, 1)])
    out = torch.cat(cols, dim=-1)
    bound = torch.zeros_like(out)
    bound[:, xf.shape[1]:xf.shape[1] + ys.shape[1]] = 8 * U[torch.float32] * ys.abs()
    pad = width - out.shape[1]
    out, bound = torch.nn.functional.pad(out, (0, pad)), torch.nn.functional.pad(bound, (0, pad))
    return out, bound + U[out_dtype] * (out.abs() + bound)


def edm_output_ref(pred, y, sigma, shape, sigma_data: float, out_dtype):
    """(D [B, T_out, E, N, V_out] float64, its bound): pred [B E N, >= T_out V_out]; y, sigma None: the rearrange alone."""
    B, T, E, N, V = shape
    p = pred.double()[:, :T * V].reshape(B, E, N, T, V).permute(0, 3, 1, 2, 4)
    if y is None:
        return p.contiguous(), U[out_dtype] * p.abs()
    _, c_skip, c_out = edm_coefficients(sigma, sigma_data)
    a, b = c_skip.view(B, 1, E, 1, 1) * y.double(), c_out.view(B, 1, E, 1, 1) * p
    bound = 8 * U[torch.float32] * (a.abs() + b.abs())
    return a + b, bound + U[out_dtype] * ((a + b).abs() + bound)


# ---------------------------------------------------------------------------------------------- kernel 4
def edm_update_ref(mode: int, params, y, D, aux1, aux2, solver_dtype):
    """{name: (value float64, bound)} of what mode writes.  params: 8 float64 values, rounded to the solver dtype first, as the kernel does."""
    p = params.to(solver_dtype).double()
    s_eff, s_next, eps, ratio, em1, c1, c2, round32 = (float(v) for v in p[:8])
    y, D = y.double(), D.double()
    k = 16 * U[solver_dtype]
    if mode in (HEUN_PREDICT, HEUN_FINAL):
        d1 = (y - D) / (s_eff + eps)
        m1 = (y.abs() + D.abs()) / abs(s_eff + eps)
        y_next, m2 = y + (s_next - s_eff) * d1, y.abs() + abs(s_next - s_eff) * m1
        return {"aux1": (d1, k * m1), "aux2": (y_next, k * m2)} if mode == HEUN_PREDICT else {"y": (y_next, k * m2)}
    if mode == HEUN_CORRECT:
        d2 = (aux2.double() - D) / (s_next + eps)
        m = y.abs() + abs(s_next - s_eff) * (aux1.double().abs() + (aux2.double().abs() + D.abs()) / abs(s_next + eps)) / 2
        return {"y": (y + (s_next - s_eff) * (aux1.double() + d2) / 2, k * m)}
    if mode in (DPMPP_FIRST, DPMPP_MULTI):
        dm, mm = (D, D.abs()) if mode == DPMPP_FIRST else (c1 * D + c2 * aux1.double(), abs(c1) * D.abs() + abs(c2) * aux1.double().abs())
        v, b = ratio * y - em1 * dm, k * (abs(ratio) * y.abs() + abs(em1) * mm)
        if round32:  # the new state is rounded to fp32, the data dtype: one more rounding, of the value and of what it may be off by
            b = b + U[torch.float32] * (v.abs() + b)
        return {"y": (v, b), "aux1": (D, torch.zeros_like(D))}
    return {"y": (D, torch.zeros_like(D))}


# ---------------------------------------------------------------------------------------------- samplers
def heun_ref(x, y0, sigmas, denoise, draws, S_churn=0.0, S_min=0.0, S_max=float("inf"), S_noise=1.0, eps=1e-10):
    """EDM Heun with churn in float64 on single tensors: denoise(x, y, sigma float) -> D; ``draws``: the churn noise, consumed in order."""
    s = [float(v) for v in sigmas.double()]
    n, y, draws = len(s) - 1, y0.double().clone(), list(draws)
    for i in range(n):
        s_eff = s[i]
        if S_min <= s[i] <= S_max and S_churn > 0:
            gamma = min(S_churn / n, 2.0**0.5 - 1)
            s_eff = s[i] + gamma * s[i]
            y = y + (s_eff**2 - s[i]**2)**0.5 * (draws.pop(0).double() * S_noise)
        d1 = (y - denoise(x, y, s_eff)) / (s_eff + eps)
        y_next = y + (s[i + 1] - s_eff) * d1
        if s[i + 1] != 0:
            d2 = (y_next - denoise(x, y_next, s[i + 1])) / (s[i + 1] + eps)
            y = y + (s[i + 1] - s_eff) * (d1 + d2) / 2
        else:
            y = y_next
    return y


def dpmpp_ref(x, y0, sigmas, denoise, data_dtype=torch.float64):
    """DPM++ 2M in float64 on single tensors; y starts and leaves every update in ``data_dtype``, as in the reference (in its float64
    run that is float64: no rounding)."""
    import math

    s = [float(v) for v in sigmas.double()]
    y, old = y0.to(data_dtype).double().clone(), None
    for i in range(len(s) - 1):
        D = denoise(x, y, s[i])
        if s[i + 1] == 0:
            return D
        t, t_next = -math.log(s[i] + 1e-10), -math.log(s[i + 1] + 1e-10)
        h = t_next - t
        if old is None:
            Dm = D
        else:
            r = (t - (-math.log(s[i - 1] + 1e-10))) / h
            Dm = (1 + 1 / (2 * r)) * D + (-1 / (2 * r)) * old
        y, old = ((s[i + 1] / s[i]) * y - (math.exp(-h) - 1) * Dm).to(data_dtype).double(), D
    return y


def analytic_denoise(x, y, sigma):
    """The closed-form denoiser of the fixture's ``analytic`` cases (tests/golden/make_golden_transport.py): x [B, T, E, N, V], y like D; sigma a
    float or a [B, 1, E, 1, 1] tensor."""
    s = torch.as_tensor(sigma, dtype=y.dtype, device=y.device)
    t = s**2 + 1.0
    return y / t + s / t.sqrt() * torch.tanh(y / t.sqrt() + x[:, -1:].to(y.dtype))


# ---------------------------------------------------------------------------------------------- the model of a fixture case
N_CHANNELS, N_LAYERS, N_HEADS, TRAINABLE = 64, 2, 2, 8


def config_of(case: dict) -> dict:
    from anemoi_core_amd.models.configs import transport_model_config

    kw = {"scale": 16} if case.get("embedder") == "RandomFourierEmbeddings" else {"max_period": 1000}
    return transport_model_config("gt", N_CHANNELS, N_LAYERS, N_HEADS, TRAINABLE, noise_embedder=case.get("embedder", "SinusoidalEmbeddings"),
                                  inference_defaults={"sampling_schedule": {}, "sampler": {}}, **kw)


def transport_model(fx: dict, name: str, batch=None, members: int = 1):
    """(model, x, y, sigma, parameter checksum) of model case ``name``: parameters and inputs drawn as the generator drew them."""
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiTransportModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices
    from tests.transformer_helpers import fill

    entry = fx["models"][name]
    case = entry["case"]
    g = build_synthetic_graph("o8", 3)
    v_in, v_out, t_out = case.get("n_vars_in", 4), case.get("n_vars_out", 4), case.get("n_step_output", 1)
    model = AnemoiTransportModelEncProcDec(model_config=config_of(case), data_indices=make_data_indices(v_in, v_out), statistics={"data": None},
                                           n_step_input=fx["n_step_input"], n_step_output=t_out, graph_data=g).eval()
    psum = fill(model, entry["param_seed"])
    B = batch or case.get("batch", 1)
    gen = torch.Generator().manual_seed(entry["input_seed"])
    x = torch.randn(B, fx["n_step_input"], members, g.num_data, v_in, generator=gen)
    sigma = torch.tensor((case["sigma"] * (B * members))[:B * members], dtype=torch.float32).view(B, 1, members, 1, 1)
    y = torch.randn(B, t_out, members, g.num_data, v_out, generator=gen) * (1 + sigma**2).sqrt()
    return model, x, y, sigma, psum


def replay_draws(model, sampler_params: dict, draws: list):
    """Make ``model.sample`` consume the recorded random numbers: the first is the source field (the model's source builder is pointed at
    the queue), the rest the churn noise.  Returns the queue (empty when every draw was used) and the ``draw`` function reading it, for the
    caller to install as ``EDMHeunSampler.draw``."""
    queue = [t.clone() for t in draws]

    def draw(shape, dtype, device):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(device=device, dtype=dtype)

    model.transport_source.draw = draw
    return queue, draw
