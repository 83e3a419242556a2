"""``ops.cond_layer_norm_proj`` (csrc/rowwise.hip: cond_layernorm_proj_fwd_kernel) - the conditional LayerNorm whose modulation is
computed in the kernel - against a float64 restatement on the CPU of

    y = LN(x) * (1 + c Ws^T + bs) + (c Wb^T + bb) [+ residual]

evaluated on the inputs *after* they were rounded to the test dtype, within ``tests.test_kernels_gpu.assert_close`` (the bounds of the
existing conditional-LayerNorm test: fp32 atol 1e-4 + rtol 1e-5; 16 bit 2e-2 max|want| + 2e-2 |want|).  Every element is compared.

The shapes walk the kernel's three homes of the weight image: registers (C <= 4 with one 16-byte chunk per lane: D = 512 16-bit,
D = 100 / 33 / ... at narrow vectors), LDS (image <= 160 KiB) and global memory (fp32 D = 1024 at C = 32: 256 KiB); the conditioning rows
contiguous and as the column slab ``wide[:, 1:1 + C]`` of a wider buffer (misaligned, neighbours filled with 3.0).
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import DEV, assert_close
from tests.test_rowwise_backward_gpu import DTYPES, NAME, _slab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from anemoi_core_amd import ops as _ops

    return _ops


def _case(N, D, C, dtype, seed=0):
    """Rounded CPU operands: x, cond, the two Linear maps (weights [D, C], biases [D]) and a residual."""
    gen = torch.Generator().manual_seed(7 * N + 3 * D + C + seed)
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=gen)).to(dtype)  # noqa: E731
    return dict(x=(1.5 * torch.randn(N, D, generator=gen) + 0.3).to(dtype), cond=r(N, C), ws=r(D, C, k=0.3), bs=r(D, k=0.3), wb=r(D, C, k=0.3),
                bb=r(D, k=0.3), res=r(N, D))


def _want(c, residual: bool):
    d = {k: v.double() for k, v in c.items()}
    D = d["x"].shape[1]
    y = F.layer_norm(d["x"], (D,), None, None, 1e-5) * (1.0 + d["cond"] @ d["ws"].T + d["bs"]) + (d["cond"] @ d["wb"].T + d["bb"])
    return y + d["res"] if residual else y


def _run(ops, c, residual: bool, slab: bool):
    w, b = ops.cond_layer_norm_proj_weights(c["ws"].to(DEV), c["bs"].to(DEV), c["wb"].to(DEV), c["bb"].to(DEV))
    cond = _slab(c["cond"], 1 if slab else None)
    return ops.cond_layer_norm_proj(c["x"].to(DEV), cond, w, b, 1e-5, c["res"].to(DEV) if residual else None)


# (cond layout, residual): the full cross for the small row counts; the 40 968-row shapes take two of the four
_VARIANTS = {"contig": (False, False), "contig-res": (False, True), "slab": (True, False), "slab-res": (True, True)}


def _params():
    out = []
    for N in (1, 5, 1030, 40968):
        for D in (512, 100, 33, 1024):
            for C in (1, 4, 5, 16, 32):
                for dtype in DTYPES:
                    for name in (("contig-res", "slab") if N == 40968 else _VARIANTS):
                        out.append(pytest.param(N, D, C, dtype, name, id=f"N{N}-D{D}-C{C}-{NAME[dtype]}-{name}"))
    return out


@pytest.mark.parametrize("N,D,C,dtype,variant", _params())
def test_cond_layer_norm_proj_vs_float64(ops, N, D, C, dtype, variant):
    slab, residual = _VARIANTS[variant]
    c = _case(N, D, C, dtype)
    y = _run(ops, c, residual, slab)
    assert y.dtype == dtype and y.shape == (N, D)
    want = _want(c, residual)
    err = (y.double().cpu() - want).abs().max().item()
    print(f"cond_layer_norm_proj N={N} D={D} C={C} {NAME[dtype]} {variant}: max err {err:.3e} (max|want| {want.abs().max().item():.3e})")
    assert_close(y, want, dtype, "y")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("D", [512, 100, 33, 1024])
@pytest.mark.parametrize("C", [4, 16])
def test_zero_weights_and_biases_are_layer_norm(ops, C, D, dtype):
    N = 1030
    c = _case(N, D, C, dtype)
    for k in ("ws", "bs", "wb", "bb"):
        c[k] = torch.zeros_like(c[k])
    y = _run(ops, c, False, False)
    want = F.layer_norm(c["x"].double(), (D,), None, None, 1e-5)
    plain = ops.layer_norm(c["x"].to(DEV), torch.ones(D, dtype=dtype, device=DEV), None)
    assert_close(y, want, dtype, "cond_layer_norm_proj(w=0, b=0)")
    assert_close(y, plain.double(), dtype, "cond_layer_norm_proj(w=0, b=0) vs layer_norm(weight=1)")


def test_three_dimensional_input_and_column_slab_x(ops):
    """x as [batch, rows, D] (flattened like ops.layer_norm) and as a column slab of a wider buffer (its own leading dimension)."""
    c = _case(600, 512, 4, torch.bfloat16)
    want = _want(c, True)
    w, b = ops.cond_layer_norm_proj_weights(*(c[k].to(DEV) for k in ("ws", "bs", "wb", "bb")))
    y3 = ops.cond_layer_norm_proj(c["x"].to(DEV).view(2, 300, 512), c["cond"].to(DEV), w, b, 1e-5, c["res"].to(DEV).view(2, 300, 512))
    assert y3.shape == (2, 300, 512)
    assert_close(y3.view(600, 512), want, torch.bfloat16, "3-D x")
    ys = ops.cond_layer_norm_proj(_slab(c["x"], 8), c["cond"].to(DEV), w, b, 1e-5, _slab(c["res"], 8))
    assert_close(ys, want, torch.bfloat16, "x and residual as slabs")
    assert torch.equal(ys, y3.view(600, 512))


def test_unsupported_shapes_are_refused_with_their_messages(ops):
    c = _case(8, 64, 33, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="C=33"):
        _run(ops, c, False, False)
    c = _case(4, 4096, 4, torch.float32)  # fp32 rows hold 2048 elements at most
    with pytest.raises(ValueError, match="too large for the register-resident row"):
        _run(ops, c, False, False)
    c = _case(8, 64, 4, torch.bfloat16)
    w, b = ops.cond_layer_norm_proj_weights(*(c[k].to(DEV) for k in ("ws", "bs", "wb", "bb")))
    with pytest.raises(ValueError, match="cond must be"):
        ops.cond_layer_norm_proj(c["x"].to(DEV), c["cond"].to(DEV)[:5], w, b)
    with pytest.raises(ValueError, match="image"):
        ops.cond_layer_norm_proj(c["x"].to(DEV), c["cond"].to(DEV), w.t().contiguous(), b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cond_layer_norm_proj(c["x"], c["cond"], w.cpu(), b.cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_zero_rows(ops, dtype, monkeypatch):
    from anemoi_core_amd import _ext

    c = _case(4, 512, 4, dtype)
    w, b = ops.cond_layer_norm_proj_weights(*(c[k].to(DEV) for k in ("ws", "bs", "wb", "bb")))
    x0, c0 = torch.empty(0, 512, dtype=dtype, device=DEV), torch.empty(0, 4, dtype=dtype, device=DEV)
    assert ops.cond_layer_norm_proj(x0, c0, w, b).shape == (0, 512)
    assert ops.cond_layer_norm_proj(x0, c0, w, b, residual=x0).shape == (0, 512)
    monkeypatch.setattr(_ext, "ops", lambda: None)  # and through ctypes: the entry returns before it looks at the (null) pointers
    assert ops.cond_layer_norm_proj(x0, c0, w, b).shape == (0, 512)


@pytest.mark.parametrize("D,C", [(512, 4), (1024, 32), (100, 5)])
def test_hipgraph_replay_is_bit_equal_to_eager(ops, D, C):
    c = _case(1030, D, C, torch.bfloat16)
    w, b = ops.cond_layer_norm_proj_weights(*(c[k].to(DEV) for k in ("ws", "bs", "wb", "bb")))
    x, cond, res = c["x"].to(DEV), _slab(c["cond"], 1), c["res"].to(DEV)
    eager = ops.cond_layer_norm_proj(x, cond, w, b, 1e-5, res).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.cond_layer_norm_proj(x, cond, w, b, 1e-5, res)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.cond_layer_norm_proj(x, cond, w, b, 1e-5, res)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_ctypes_path_matches_the_torch_op(ops, dtype, monkeypatch):
    from anemoi_core_amd import _ext

    c = _case(700, 512, 5, dtype)
    a = _run(ops, c, True, True)
    assert _ext.ops() is not None
    monkeypatch.setattr(_ext, "ops", lambda: None)
    b = _run(ops, c, True, True)
    assert torch.equal(a, b)
