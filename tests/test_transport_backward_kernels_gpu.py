"""The three backward kernels of the EDM denoiser edges (csrc/transport_bwd.hip) on the MI355X, each against its float64 restatement under
the componentwise bound computed from the operands (tests/transport_train_refs.py), at the sizes their loops branch on: the 512-row tile of
the noise conditioning's first stage, the 64-lane wave of the two element-wise kernels; every run repeated and compared bit for bit; and the
refusals that stay."""
import itertools

import pytest
import torch

from anemoi_core_amd import ops
from tests import transport_train_refs as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _within(got, want, bound, what):
    got = got.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    worst = float((err - bound).max())
    assert bool((err <= bound).all()), f"{what}: exceeds its bound by {worst:.3e} (max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e})"


# ---------------------------------------------------------------------------------------------- 1. noise conditioning
def _noise_cases():
    """rows per group at the tile edge x the destination combinations, the other parameters cycling through their values at different
    periods, so that every value meets every kind of tile count."""
    edge = [1, 511, 512, 513, 1025]
    cases = []
    for i, (r, combo) in enumerate(itertools.product(edge, ("first", "second", "both"))):
        rows = {"first": (r, 0), "second": (0, r), "both": (r, edge[(i + 2) % 5])}[combo]
        cases.append(dict(rows=rows, G=(1, 3)[i % 2], C=(2, 32, 64)[i % 3], cond_dim=(1, 16, 32)[(i // 3) % 3], dtype=DTYPES[(i // 2) % 3],
                          log_quarter=bool((i // 2) % 2), pi=bool((i // 4) % 2), pad=(0, 8, 3, 0)[i % 4], shift=0))
    # a gradient that starts off a 16-byte boundary (the scalar path), and full-width vector paths in every dtype
    cases.append(dict(rows=(513, 70), G=3, C=64, cond_dim=32, dtype=torch.float32, log_quarter=True, pi=True, pad=4, shift=1))
    for dt in DTYPES:
        cases.append(dict(rows=(1025, 513), G=3, C=64, cond_dim=32, dtype=dt, log_quarter=True, pi=False, pad=8, shift=0))
        cases.append(dict(rows=(512, 1), G=1, C=32, cond_dim=16, dtype=dt, log_quarter=False, pi=True, pad=0, shift=0))
    return cases


NOISE_CASES = _noise_cases()


@pytest.mark.parametrize("i", range(len(NOISE_CASES)))
def test_noise_cond_backward(i):
    c = NOISE_CASES[i]
    gen = torch.Generator().manual_seed(100 + i)
    G, C, cd = c["G"], c["C"], c["cond_dim"]
    values = torch.rand(G, generator=gen) * 20 + 0.05
    freq = torch.randn(C // 2, generator=gen) * 3
    pi = torch.tensor([3.14159], dtype=torch.float32) if c["pi"] else None
    w1, b1, w2, b2 = (torch.randn(s, generator=gen) * 0.3 for s in ((C, C), (C,), (cd, C), (cd,)))
    d_outs = []
    for r in c["rows"]:
        if r == 0:
            d_outs.append(None)
            continue
        wide = torch.randn(G * r, cd + c["pad"] + c["shift"], generator=gen).to(c["dtype"]).to(DEV)
        d_outs.append(wide[:, c["shift"]:c["shift"] + cd])
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    run = lambda: ops.noise_cond_backward(tuple(d_outs), c["rows"], dev(values), dev(freq), dev(w1), dev(b1), dev(w2), dev(b2), pi=dev(pi),  # noqa: E731
                                          log_quarter=c["log_quarter"])
    got, again = run(), run()
    for a, b in zip(got, again):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    ref, bound = TR.noise_cond_bwd_ref([None if d is None else d.cpu() for d in d_outs], c["rows"], values, freq, pi, w1, b1, w2, b2, c["log_quarter"])
    for g, key in zip(got, ("d_w1", "d_b1", "d_w2", "d_b2")):
        _within(g, ref[key].reshape(g.shape), bound[key].reshape(g.shape), f"noise_cond_bwd {c} {key}")


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
def test_noise_cond_autograd_returns_parameter_dtypes(wdt):
    """Through ``ops.noise_cond`` under autograd: 16-bit parameters get 16-bit gradients, the fp32 result of the kernel rounded once; the
    forward under grad equals the forward without."""
    gen = torch.Generator().manual_seed(7)
    G, C, cd, rows = 3, 32, 16, (600, 37)
    values = (torch.rand(G, generator=gen) * 5 + 0.1).to(DEV)
    freq = torch.randn(C // 2, generator=gen).to(DEV)
    params = [(torch.randn(s, generator=gen) * 0.3).to(wdt).to(DEV).requires_grad_(True) for s in ((C, C), (C,), (cd, C), (cd,))]
    outs = ops.noise_cond(values, freq, *params, log_quarter=True, rows=rows, out_dtype=wdt)
    with torch.no_grad():
        plain = ops.noise_cond(values, freq, *params, log_quarter=True, rows=rows, out_dtype=wdt)
    assert all(torch.equal(a, b) for a, b in zip(outs, plain)) and all(o.grad_fn is not None for o in outs)
    d_outs = [torch.randn(o.shape, generator=gen).to(wdt).to(DEV) for o in outs]
    torch.autograd.backward(outs, d_outs)
    want = ops.noise_cond_backward(tuple(d_outs), rows, values, freq, *[p.detach() for p in params], log_quarter=True)
    for p, w in zip(params, want):
        assert p.grad.dtype == wdt and p.grad.shape == p.shape and torch.equal(p.grad, w.to(wdt).view(p.shape))
    # one destination unused by the loss: its gradient is absent, not zeros read from nowhere
    for p in params:
        p.grad = None
    o0, _ = ops.noise_cond(values, freq, *params, log_quarter=True, rows=rows, out_dtype=wdt)
    o0.backward(d_outs[0])
    want = ops.noise_cond_backward((d_outs[0], None), rows, values, freq, *[p.detach() for p in params], log_quarter=True)
    for p, w in zip(params, want):
        assert torch.equal(p.grad, w.to(wdt).view(p.shape))


# ---------------------------------------------------------------------------------------------- 2. input assembly
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_transport_assemble_input_backward(dtype):
    gen = torch.Generator().manual_seed(11)
    for N, (B, E), A, pad in itertools.product((1, 63, 64, 65), ((1, 1), (2, 1), (2, 3)), (1, 4, 12), (0, 5)):
        G, T_in, V_in, T_out, V_out = B * E, 2, 3, 1, 2
        col0 = T_in * V_in + T_out * V_out
        width = col0 + A + pad
        d_rows = torch.randn(G * N, width, generator=gen).to(dtype)
        run = lambda: ops.transport_assemble_input_backward(d_rows.to(DEV), col0, N, A)  # noqa: E731
        got, again = run(), run()
        assert got.dtype == dtype and got.shape == (N, A) and torch.equal(got, again)
        want, bound = TR.assemble_input_bwd_ref(d_rows, col0, N, A)
        _within(got, want, bound, f"assemble_input_bwd N={N} G={G} A={A} pad={pad} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_transport_assemble_input_autograd(dtype):
    """Through ``ops.transport_assemble_input`` under autograd, attributes that are the concatenation of a constant and a trainable block (the
    model's node attributes): the gradient arrives at the trainable leaf in its dtype; the forward under grad equals the forward without."""
    gen = torch.Generator().manual_seed(12)
    B, E, N, width = 2, 3, 65, 24
    x, y = torch.randn(B, 2, E, N, 4, generator=gen).to(DEV), torch.randn(B, 1, E, N, 4, generator=gen).to(DEV)
    sigma = (torch.rand(B * E, generator=gen) + 0.1).to(DEV)
    fixed = torch.randn(N, 4, generator=gen).to(dtype).to(DEV)
    leaf = torch.randn(N, 5, generator=gen).to(dtype).to(DEV).requires_grad_(True)
    rows = ops.transport_assemble_input(x, y, torch.cat([fixed, leaf], dim=1), width, sigma=sigma, out_dtype=dtype)
    with torch.no_grad():
        plain = ops.transport_assemble_input(x, y, torch.cat([fixed, leaf], dim=1), width, sigma=sigma, out_dtype=dtype)
    assert torch.equal(rows, plain) and rows.shape == (B * E * N, width)
    d_rows = torch.randn(rows.shape, generator=gen).to(dtype).to(DEV)
    rows.backward(d_rows)
    want, bound = TR.assemble_input_bwd_ref(d_rows.cpu(), 12, N, 9)
    assert leaf.grad.dtype == dtype
    _within(leaf.grad, want[:, 4:], bound[:, 4:], f"assemble_input autograd {dtype}")


# ---------------------------------------------------------------------------------------------- 3. output assembly
def _layout(d: torch.Tensor, kind: str) -> torch.Tensor:
    """The same values (for "expanded": one value) behind different strides."""
    if kind == "contiguous":
        return d.contiguous()
    if kind == "permuted":  # stored "(batch ensemble grid) (time vars)"-like: no dimension where the contiguous layout has it
        return d.permute(4, 2, 0, 3, 1).contiguous().permute(2, 4, 1, 3, 0)
    return d.flatten()[:1].reshape(1, 1, 1, 1, 1).expand(d.shape)  # what sum().backward() hands over: every stride 0


def test_edm_output_backward():
    gen = torch.Generator().manual_seed(13)
    variants = list(itertools.product((torch.float32, torch.bfloat16), (torch.float32, torch.float64), ("contiguous", "permuted", "expanded"),
                                      (True, False)))
    B, E = 2, 2
    sigma = torch.tensor([0.05, 0.7, 3.0, 80.0])  # different noise levels inside one batch
    for i, (T, V, N, extra) in enumerate(itertools.product((1, 2), (1, 3, 8), (1, 63, 64, 65), (0, 5))):
        for j in (0, 1):  # two of the 24 variants per shape, each variant at 4 shapes
            pdt, gdt, kind, precond = variants[(2 * i + j * 13) % len(variants)]
            d_out = _layout(torch.randn(B, T, E, N, V, generator=gen, dtype=gdt), kind)
            P = T * V + extra
            sig = sigma if precond else None

            def run():
                out = torch.full((B * E * N, P), float("nan"), dtype=pdt, device=DEV)  # every element must be written
                return ops.edm_output_backward(d_out.to(DEV) if kind != "expanded" else d_out[:1, :1, :1, :1, :1].to(DEV).expand(d_out.shape),
                                               None if sig is None else sig.to(DEV), (B * E * N, P), pdt, sigma_data=1.0, out=out)

            got, again = run(), run()
            what = f"edm_output_bwd T={T} V={V} N={N} extra={extra} {pdt} {gdt} {kind} precondition={precond}"
            assert not torch.isnan(got).any(), what
            assert torch.equal(got, again), what
            assert torch.equal(got[:, T * V:], torch.zeros(B * E * N, extra, dtype=pdt, device=DEV)), what  # exactly 0.0
            want, bound = TR.edm_output_bwd_ref(d_out, sig, 1.0, P, pdt)
            _within(got, want, bound, what)


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("precond", [True, False])
def test_edm_output_autograd(pdt, precond):
    """Through ``ops.edm_output`` under autograd, ``pred`` 5 columns wider than the state: out.sum().backward() hands over an expanded
    gradient; a weighted loss a dense one.  The forward under grad equals the forward without."""
    gen = torch.Generator().manual_seed(14)
    B, T, E, N, V = 2, 2, 1, 65, 3
    pred = torch.randn(B * E * N, T * V + 5, generator=gen).to(pdt).to(DEV).requires_grad_(True)
    y = torch.randn(B, T, E, N, V, generator=gen).to(DEV) if precond else None
    sigma = torch.tensor([0.3, 40.0]).to(DEV) if precond else None
    out = ops.edm_output(pred, y, sigma, (B, T, E, N, V))
    with torch.no_grad():
        assert torch.equal(out, ops.edm_output(pred, y, sigma, (B, T, E, N, V)))
    out.sum().backward()
    ones = torch.ones(B, T, E, N, V)
    want, bound = TR.edm_output_bwd_ref(ones, None if sigma is None else sigma.cpu(), 1.0, pred.shape[1], pdt)
    assert pred.grad.dtype == pdt and pred.grad.shape == pred.shape
    _within(pred.grad, want, bound, "edm_output autograd, expanded gradient")
    pred.grad = None
    w = torch.randn(B, T, E, N, V, generator=gen, dtype=torch.float64).to(DEV)
    out64 = ops.edm_output(pred, y, sigma, (B, T, E, N, V), out_dtype=torch.float64)
    (out64 * w).sum().backward()
    want, bound = TR.edm_output_bwd_ref(w.cpu(), None if sigma is None else sigma.cpu(), 1.0, pred.shape[1], pdt)
    _within(pred.grad, want, bound, "edm_output autograd, float64 gradient")


# ---------------------------------------------------------------------------------------------- refusals that stay
def test_refusals_name_the_operand():
    gen = torch.Generator().manual_seed(15)
    C, cd = 4, 3
    w1, b1, w2, b2 = (torch.randn(s, generator=gen).to(DEV) for s in ((C, C), (C,), (cd, C), (cd,)))
    freq = torch.randn(C // 2, generator=gen).to(DEV)
    with pytest.raises(NotImplementedError, match="noise_cond: a gradient with respect to values"):
        ops.noise_cond(torch.ones(2, device=DEV, requires_grad=True), freq, w1, b1, w2, b2)
    B, E, N = 1, 1, 5
    x, y = torch.randn(B, 1, E, N, 2, generator=gen).to(DEV), torch.randn(B, 1, E, N, 2, generator=gen).to(DEV)
    sigma, attrs = torch.ones(1, device=DEV), torch.randn(N, 3, generator=gen).to(DEV)
    g = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    with pytest.raises(NotImplementedError, match="transport_assemble_input: a gradient with respect to x "):
        ops.transport_assemble_input(g(x), y, attrs, 7, sigma=sigma)
    with pytest.raises(NotImplementedError, match="transport_assemble_input: a gradient with respect to y "):
        ops.transport_assemble_input(x, g(y), attrs, 7, sigma=sigma)
    with pytest.raises(NotImplementedError, match="transport_assemble_input: a gradient with respect to sigma "):
        ops.transport_assemble_input(x, y, attrs, 7, sigma=g(sigma))
    pred = torch.randn(N, 2, generator=gen).to(DEV)
    with pytest.raises(NotImplementedError, match="edm_output: a gradient with respect to y "):
        ops.edm_output(pred, g(y), sigma, (B, 1, E, N, 2))
    with pytest.raises(NotImplementedError, match="edm_output: a gradient with respect to sigma "):
        ops.edm_output(pred, y, g(sigma), (B, 1, E, N, 2))
    params = torch.zeros(8, dtype=torch.float64, device=DEV)
    state = torch.randn(B, 1, E, N, 2, generator=gen, dtype=torch.float64).to(DEV)
    for k in range(2):
        ops_args = [state.clone(), state.clone()]
        ops_args[k].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="edm_update_: differentiating through the sampler is not built"):
            ops.edm_update_(ops.HEUN_FINAL, params, *ops_args)
    # under no_grad nothing is refused and nothing is recorded
    with torch.no_grad():
        out = ops.edm_output(g(pred), y, sigma, (B, 1, E, N, 2))
    assert not out.requires_grad
