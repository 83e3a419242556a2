"""The four EDM diffusion kernels (csrc/transport.hip) against their float64 restatements (tests/transport_refs.py) within the bound
computed there, at the smallest shapes their paths branch on: one grid point and more than one workgroup, rows that are and are not whole
8-column groups (the vector path of the 16-bit input assembly), both model dtypes, both solver dtypes, sigma at both ends of the
schedule, sigma_next = 0, a strided x, a skipped destination."""
import math

import pytest
import torch

from anemoi_core_amd import ops
from tests import transport_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIGMAS = (0.02, 1.0, 100.0)
GUARD = 7.5  # fill value of guard-padded outputs: exactly representable in every dtype


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: exceeds its bound by {worst:.3e}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- kernel 1
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G,rows,C,cond_dim,two_pi,log_quarter,values_dtype", [
    (1, (1, 0), 32, 16, False, True, torch.float32),      # cond itself, second destination skipped
    (3, (63, 257), 32, 16, True, True, torch.float64),    # random Fourier, fp64 sigma, two destinations
    (3, (513, 64), 64, 32, False, False, torch.float32),  # the widest MLP, more than one row tile (512), identity transform
    (1, (1025, 1), 8, 5, True, False, torch.float64),     # three tiles, odd cond_dim
])
def test_noise_cond(dtype, G, rows, C, cond_dim, two_pi, log_quarter, values_dtype):
    g = _gen(C + cond_dim + G)
    values = torch.tensor((SIGMAS * G)[:G], dtype=values_dtype)
    freq = torch.randn(C // 2, generator=g) * (16 if two_pi else 1)
    pi = torch.tensor(math.pi) if two_pi else None
    w1, b1 = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(dtype), (0.1 * torch.randn(C, generator=g)).to(dtype)
    w2, b2 = (torch.randn(cond_dim, C, generator=g) / math.sqrt(C)).to(dtype), (0.1 * torch.randn(cond_dim, generator=g)).to(dtype)
    want, bound = R.noise_cond_ref(values, freq, pi, w1, b1, w2, b2, log_quarter, dtype)
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    outs = ops.noise_cond(d(values), d(freq), d(w1), d(b1), d(w2), d(b2), pi=d(pi), log_quarter=log_quarter, rows=rows, out_dtype=dtype)
    assert len(outs) == 2 and (outs[1] is None) == (rows[1] == 0)
    for out, r in zip(outs, rows):
        if out is None:
            continue
        assert out.shape == (G * r, cond_dim) and out.dtype == dtype
        _within(out, want.repeat_interleave(r, dim=0), bound.repeat_interleave(r, dim=0), f"noise_cond rows={r}")
        assert torch.equal(out.view(G, r, cond_dim), out.view(G, r, cond_dim)[:, :1].expand(G, r, cond_dim))  # every row of a group is the same


# ---------------------------------------------------------------------------------------------- kernel 2
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("y_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("B,E,N,T_in,V_in,T_out,V_out,A,pad", [
    (1, 1, 1, 1, 3, 1, 1, 0, 0),     # one point, no attributes, exact width
    (1, 3, 63, 2, 4, 1, 5, 3, 0),    # ensemble folded into the batch; 16 columns: the 8-column path for bf16
    (3, 1, 64, 2, 3, 2, 8, 3, 7),    # 25 columns + 7 zeros = 32
    (1, 1, 257, 2, 5, 1, 8, 3, 2),   # more than one workgroup; 23 columns: the scalar path
])
def test_transport_assemble_input(dtype, y_dtype, B, E, N, T_in, V_in, T_out, V_out, A, pad):
    g = _gen(N + V_out)
    long_x = torch.randn(B, T_in + 2, E, N, V_in, generator=g)
    x = long_x[:, 1:1 + T_in]  # a time slice of a longer tensor: strided
    y = (torch.randn(B, T_out, E, N, V_out, generator=g, dtype=torch.float64) * 30).to(y_dtype)
    attrs = None if A == 0 else torch.randn(N, A, generator=g).to(dtype)
    sigma = torch.tensor((SIGMAS * (B * E))[:B * E], dtype=y_dtype)
    width = T_in * V_in + T_out * V_out + A + pad
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    xd = d(long_x)[:, 1:1 + T_in]
    assert xd.data_ptr() != xd.untyped_storage().data_ptr() and (B == 1 or not xd.is_contiguous())  # offset, and strided beyond one sample
    for sig, sd in ((sigma, 1.0), (sigma, 0.5), (None, 1.0)):
        want, bound = R.assemble_input_ref(x, y, attrs, width, sig, sd, dtype)
        extra = 8 if width % 8 == 0 else 3  # (whole 8-column groups keep their alignment: the vector path writes next to the guard too)
        guard = torch.full((B * E * N + 2, width + extra), GUARD, dtype=dtype, device=DEV)  # rows and columns around the written range
        out = guard[1:-1]
        got = ops.transport_assemble_input(xd, d(y), d(attrs), width, sigma=d(sig), sigma_data=sd, out_dtype=dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        _within(out[:, :width], want, bound, f"assemble_input sigma_data={sd} scale={sig is not None}")
        if pad:
            assert not out[:, width - pad:width].any()  # exact zeros
        assert bool((guard[0] == GUARD).all()) and bool((guard[-1] == GUARD).all()) and bool((guard[:, width:] == GUARD).all())
    fresh = ops.transport_assemble_input(xd, d(y), d(attrs), width, sigma=d(sigma), sigma_data=0.5, out_dtype=dtype)  # aligned rows of its own
    want, bound = R.assemble_input_ref(x, y, attrs, width, sigma, 0.5, dtype)
    assert fresh.shape == (B * E * N, width) and fresh.dtype == dtype and (pad == 0 or not fresh[:, width - pad:].any())
    _within(fresh, want, bound, "assemble_input (own output)")


# ---------------------------------------------------------------------------------------------- kernel 3
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("out_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("B,E,N,T_out,V_out,ld_extra", [(1, 1, 1, 1, 1, 0), (1, 3, 63, 2, 5, 6), (3, 1, 64, 1, 8, 0), (1, 1, 257, 2, 8, 3)])
def test_edm_output(dtype, out_dtype, B, E, N, T_out, V_out, ld_extra):
    g = _gen(N + V_out + 1)
    shape = (B, T_out, E, N, V_out)
    pred = torch.randn(B * E * N, T_out * V_out + ld_extra, generator=g).to(dtype)  # (the decoder pads its output rows to 16 bytes)
    y = (torch.randn(*shape, generator=g, dtype=torch.float64) * 30).to(out_dtype)
    sigma = torch.tensor((SIGMAS * (B * E))[:B * E], dtype=out_dtype)
    for sd in (1.0, 0.5):
        want, bound = R.edm_output_ref(pred, y, sigma, shape, sd, out_dtype)
        guard = torch.full((math.prod(shape) + 16,), GUARD, dtype=out_dtype, device=DEV)
        out = guard[8:-8].view(shape)
        ops.edm_output(pred.to(DEV), y.to(DEV), sigma.to(DEV), shape, sigma_data=sd, out=out)
        _within(out, want, bound, f"edm_output sigma_data={sd}")
        assert bool((guard[:8] == GUARD).all()) and bool((guard[-8:] == GUARD).all())
    want, bound = R.edm_output_ref(pred, None, None, shape, 1.0, out_dtype)
    plain = ops.edm_output(pred.to(DEV), None, None, shape, out_dtype=out_dtype)
    assert plain.dtype == out_dtype and plain.is_contiguous()
    assert torch.equal(plain.double().cpu(), want)  # the rearrange and the cast alone: exact


# ---------------------------------------------------------------------------------------------- kernel 4
@pytest.mark.parametrize("solver", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 63, 257, 64 * 5 + 1])
@pytest.mark.parametrize("s_eff,s_next", [(100.0, 15.4), (1.0, 0.02), (0.02, 0.0)])
def test_edm_update(solver, n, s_eff, s_next):
    g = _gen(n)
    mk = lambda scale=1.0: (torch.randn(n, generator=g, dtype=torch.float64) * scale).to(solver)  # noqa: E731
    h = -math.log(s_next + 1e-10) + math.log(s_eff + 1e-10)
    params = torch.tensor([s_eff, s_next, 1e-10, s_next / s_eff, math.exp(-h) - 1, 1.3, -0.3, 0.0], dtype=torch.float64)
    for mode, round32 in [(m, 0.0) for m in range(6)] + [(ops.DPMPP_FIRST, 1.0), (ops.DPMPP_MULTI, 1.0)]:
        params[7] = round32  # the DPM++ modes also with the state rounded to fp32, the data dtype
        before = {"y": mk(s_eff), "D": mk(), "aux1": mk(), "aux2": mk(s_eff)}
        want = R.edm_update_ref(mode, params, before["y"], before["D"], before["aux1"], before["aux2"], solver)
        guard = torch.full((4, n + 16), GUARD, dtype=solver, device=DEV)  # eight guard values on either side of every operand
        bufs = {name: guard[i, 8:8 + n] for i, name in enumerate(before)}
        for name, t in before.items():
            bufs[name].copy_(t)
        got = ops.edm_update_(mode, params.to(DEV), bufs["y"], bufs["D"], bufs["aux1"], bufs["aux2"])
        assert got.data_ptr() == bufs["y"].data_ptr()
        for name, t in bufs.items():
            if name in want:
                _within(t, want[name][0], want[name][1], f"edm_update mode {mode} round32={round32} {name}")
                if round32 and name == "y":
                    assert torch.equal(t, t.float().to(solver))  # every value is an fp32 value
            else:
                assert torch.equal(t.cpu(), before[name]), (mode, name)  # what a mode does not write stays as it was
        assert bool((guard[:, :8] == GUARD).all()) and bool((guard[:, -8:] == GUARD).all())
    params[7] = 0.0
    # DPMPP_FIRST does not read D_old: NaN there must not reach y
    y, D = mk(), mk()
    nan = torch.full((n,), float("nan"), dtype=solver, device=DEV)
    out = ops.edm_update_(ops.DPMPP_FIRST, params.to(DEV), y.to(DEV), D.to(DEV), nan, None)
    assert torch.isfinite(out).all() and torch.equal(nan.cpu(), D)


def test_edm_update_checks_its_operands():
    p = torch.zeros(8, dtype=torch.float64, device=DEV)
    y = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="aux2"):
        ops.edm_update_(ops.HEUN_PREDICT, p, y, y.clone(), y.clone(), None)
    with pytest.raises(ValueError, match="contiguous"):
        ops.edm_update_(ops.DPMPP_FINAL, p, y, y.float())
    with pytest.raises(ValueError, match="8 contiguous float64"):
        ops.edm_update_(ops.DPMPP_FINAL, p.float(), y, y.clone())
