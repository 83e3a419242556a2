"""ops.sparse_project (csrc/sparse_project.hip) on the MI355X against the float64 product of the ROUNDED operands.

The tolerance is a summation bound, not a measurement.  Per element, for k entries in the row,

    |err| <= (k + 4) 2^-24 sum_j |w_j| (|x_j mul| + |add|)  +  u_out |y|,     u_out = 0 (fp32), 2^-8 (bf16), 2^-11 (fp16, + 2^-24 absolute):

k fused multiply-adds into one fp32 accumulator in CSR order (k roundings), two roundings of the affine map per value, the headroom of the
standard (1 + u)^n bound, and one rounding of the result to the output dtype.  fp32 ``torch.sparse.mm`` on the CPU stays at 0.36 of the first
term (rows of 0 to 40 entries, one row of 5 000 entries, 3-entry rows), so a failure of this bound is a kernel fault, not noise."""
import numpy as np
import pytest
import torch

from anemoi_core_amd import _ext, ops
from tests import truncation_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _matrix(kind: str, seed: int = 0):
    """(indptr, indices, values, (n_dst, n_src)) as numpy arrays."""
    rng = np.random.default_rng(seed)
    if kind == "up":  # an up-projection: the 3 nearest of 10 944 coarse rows for each of 40 320 fine rows
        n_dst, n_src = 40320, 10944
        counts = np.full(n_dst, 3)
    elif kind == "ragged":  # a down-projection with ragged rows, empty ones included; part of the source rows is never referenced
        n_dst, n_src = 1500, 9000
        counts = rng.integers(0, 41, n_dst)
        counts[[0, 7, 8, n_dst - 1]] = 0
    elif kind == "heavy":  # one row of 5 000 entries among light ones
        n_dst, n_src = 300, 7000
        counts = np.full(n_dst, 3)
        counts[17] = 5000
    elif kind == "no_entries":
        n_dst, n_src = 70, 50
        counts = np.zeros(n_dst, dtype=np.int64)
    else:
        raise KeyError(kind)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    hi = n_src if kind != "ragged" else n_src // 2  # ragged: the upper half of the source rows is unreferenced
    indices = rng.integers(0, hi, int(indptr[-1]))
    values = rng.standard_normal(int(indptr[-1])).astype(np.float32)
    return indptr, indices, values, (n_dst, n_src)


_MATS: dict = {}


def _mat(kind):
    if kind not in _MATS:
        ip, ix, v, shape = _matrix(kind)
        _MATS[kind] = ((ip, ix, v, shape), ops.build_sparse_matrix(ip, ix, v, shape).to(DEV))
    return _MATS[kind]


def _reference(arrays, x, cols, mul, add, out_dtype):
    """(float64 result, bound) from the rounded operands: x as stored, fp32 weights / mul / add."""
    ip, ix, v, shape = arrays
    xs = x.detach().double().cpu()
    if cols is not None:
        xs = xs.index_select(-1, cols.long().cpu())
    m = torch.ones(xs.shape[-1], dtype=torch.float64) if mul is None else mul.double().cpu()
    a = torch.zeros(xs.shape[-1], dtype=torch.float64) if add is None else add.double().cpu()
    want = H.project64(ip, ix, v, shape[0], xs * m + a)
    return want, H.projection_bound(ip, ix, v, shape, (xs * m).abs() + a.abs(), want, out_dtype)


def _check(got, want, bound, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got.double().cpu() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: worst err / bound {ratio:.3f}"


def _x(shape, dtype, seed=1):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 4, 17, 64, 100, 257])
def test_ragged_matrix_every_width(C, batch):
    arrays, m = _mat("ragged")
    x = _x((batch, m.n_cols, C), torch.float32)
    y = ops.sparse_project(x, m)
    assert y.dtype == torch.float32 and y.shape == (batch, m.n_rows, C)
    _check(y, *_reference(arrays, x, None, None, None, torch.float32), f"ragged C={C} batch={batch}")
    empty = np.flatnonzero(np.diff(arrays[0]) == 0)
    assert len(empty) >= 4 and torch.equal(y[:, empty.tolist()], torch.zeros_like(y[:, empty.tolist()]))  # exact zeros


@pytest.mark.parametrize("out", ["native", "fp32"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kind,C,batch", [("up", 3, 1), ("up", 64, 3), ("ragged", 17, 3), ("ragged", 100, 1), ("heavy", 4, 3), ("heavy", 257, 1)])
def test_dtypes_and_matrix_kinds(kind, C, batch, dtype, out):
    dt = DTYPES[dtype]
    odt = dt if out == "native" else torch.float32
    arrays, m = _mat(kind)
    x = _x((batch, m.n_cols, C), dt)
    y = ops.sparse_project(x, m, out_dtype=odt)
    assert y.dtype == odt
    _check(y, *_reference(arrays, x, None, None, None, odt), f"{kind} C={C} batch={batch} {dtype}->{out}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kind", ["ragged", "up"])
def test_strided_step_view_column_selection_and_affine_map(kind, dtype):
    """The model's call: the last step of [B, T, E, N, V] read in place, 80 of 101 columns, the normaliser's (mul, add), fp32 intermediate."""
    dt = DTYPES[dtype]
    arrays, m = _mat(kind)
    B, T, V = 2, 2, 101
    x5 = _x((B, T, 1, m.n_cols, V), dt)
    g = torch.Generator().manual_seed(5)
    cols = torch.randperm(V, generator=g)[:80].to(torch.int32).to(DEV)
    mul, add = (0.5 + torch.rand(80, generator=g)).to(DEV), torch.randn(80, generator=g).to(DEV)
    view = x5[:, -1]
    assert not view.is_contiguous()
    y = ops.sparse_project(view, m, cols, mul, add, out_dtype=torch.float32)
    assert y.shape == (B, 1, m.n_rows, 80) and y.dtype == torch.float32
    _check(y, *_reference(arrays, view, cols, mul, add, torch.float32), f"{kind} view {dtype}")
    y_sel = ops.sparse_project(view, m, cols)  # selection alone, output in the input dtype
    _check(y_sel, *_reference(arrays, view, cols, None, None, dt), f"{kind} view cols only {dtype}")
    assert torch.equal(ops.sparse_project(view, m, cols, mul, add, out_dtype=torch.float32), y)  # two runs are bit-equal


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_unreferenced_rows_and_unselected_columns_are_never_read(dtype):
    dt = DTYPES[dtype]
    arrays, m = _mat("ragged")
    V = 12
    x = _x((3, m.n_cols, V), dt)
    cols = torch.tensor([0, 2, 3, 7, 11, 5], dtype=torch.int32, device=DEV)
    mul, add = torch.full((6,), 1.5, device=DEV), torch.full((6,), -0.25, device=DEV)
    y = ops.sparse_project(x, m, cols, mul, add)
    unref = sorted(set(range(m.n_cols)) - set(arrays[1].tolist()))
    assert len(unref) > m.n_cols // 2
    unsel = [c for c in range(V) if c not in cols.tolist()]
    for poison in (1e4, float("nan")):
        xp = x.clone()
        xp[:, unref, :] = poison
        xp[:, :, unsel] = poison
        assert torch.equal(ops.sparse_project(xp, m, cols, mul, add), y), poison


def test_empty_matrices_and_zero_batch():
    arrays, m = _mat("no_entries")
    y = ops.sparse_project(_x((2, m.n_cols, 5), torch.bfloat16), m)
    assert y.shape == (2, m.n_rows, 5) and torch.equal(y, torch.zeros_like(y))
    none = ops.build_sparse_matrix([0], [], [], (0, 9)).to(DEV)
    assert ops.sparse_project(_x((2, 9, 5), torch.float32), none).shape == (2, 0, 5)
    no_src = ops.build_sparse_matrix([0, 0, 0], [], [], (2, 0)).to(DEV)
    y = ops.sparse_project(torch.empty(3, 0, 4, device=DEV), no_src)
    assert y.shape == (3, 2, 4) and torch.equal(y, torch.zeros_like(y))
    _, r = _mat("ragged")
    assert ops.sparse_project(torch.empty(0, r.n_cols, 7, device=DEV), r).shape == (0, r.n_rows, 7)
    assert ops.sparse_project(torch.empty(2, r.n_cols, 0, device=DEV), r).shape == (2, r.n_rows, 0)
    with pytest.raises(ValueError):
        ops.sparse_project(torch.empty(2, r.n_cols + 1, 3, device=DEV), r)
    with pytest.raises(ValueError):
        ops.sparse_project(_x((2, r.n_cols, 3), torch.bfloat16), r, out_dtype=torch.float16)


def test_graph_capture_replays_bit_equal():
    arrays, m = _mat("up")
    x = _x((2, m.n_cols, 80), torch.bfloat16)
    eager = ops.sparse_project(x, m, out_dtype=torch.float32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sparse_project(x, m, out_dtype=torch.float32)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sparse_project(x, m, out_dtype=torch.float32)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_ctypes_and_torch_op_paths_are_bit_equal():
    arrays, m = _mat("ragged")
    x5 = _x((2, 2, 1, m.n_cols, 20), torch.float16)
    cols = torch.arange(0, 20, 2, dtype=torch.int32, device=DEV)
    mul, add = torch.rand(10, device=DEV) + 0.5, torch.randn(10, device=DEV)
    assert _ext.ENABLED
    via_op = [ops.sparse_project(x5[:, -1], m, cols, mul, add, out_dtype=torch.float32), ops.sparse_project(x5[:, 0], m)]
    saved = _ext.ENABLED
    _ext.ENABLED = False
    try:
        via_ctypes = [ops.sparse_project(x5[:, -1], m, cols, mul, add, out_dtype=torch.float32), ops.sparse_project(x5[:, 0], m)]
    finally:
        _ext.ENABLED = saved
    for a, b in zip(via_op, via_ctypes):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["ragged", "up", "heavy"])
def test_backward_is_the_transposed_product(kind, dtype):
    """grad_x[..., cols] = mul * (A^T g): the same kernel on the transposed matrix, under the same bound with the transposed matrix's k."""
    dt = DTYPES[dtype]
    arrays, m = _mat(kind)
    V = 9
    x = _x((2, m.n_cols, V), dt).requires_grad_(True)
    cols = torch.tensor([8, 1, 4, 2], dtype=torch.int32, device=DEV)
    mul, add = torch.tensor([0.5, 2.0, 1.25, 3.0], device=DEV), torch.randn(4, device=DEV)
    y = ops.sparse_project(x, m, cols, mul, add, out_dtype=torch.float32)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (gx,) = torch.autograd.grad(y, x, g)
    assert gx.shape == x.shape and gx.dtype == dt
    t = m.t
    t_arrays = (t.indptr.cpu().numpy(), t.indices.cpu().numpy(), t.values.cpu().numpy(), (t.n_rows, t.n_cols))
    want_c, bound_c = _reference(t_arrays, g, None, mul, None, torch.float32)  # the kernel's fp32 result; mul applied per value
    want = torch.zeros(x.shape, dtype=torch.float64)
    want[..., cols.long().cpu()] = want_c
    bound = torch.zeros_like(want)
    bound[..., cols.long().cpu()] = bound_c
    bound = bound + H.U_OUT[dt] * want.abs()  # one more rounding: the fp32 gradient stored in x's dtype
    _check(gx, want, bound, f"backward {kind} {dtype}")
    unsel = [c for c in range(V) if c not in cols.tolist()]
    assert torch.equal(gx[..., unsel], torch.zeros_like(gx[..., unsel]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_and_ensemble_step_slice_is_read_in_place(dtype):
    """The ensemble model's call: the [B, E] last-step slice of [B, T, E, N, V] with T > 1 and E > 1 needs two leading strides; it is
    passed as a view (no copy) and the result is [B, E, n_dst, C]."""
    dt = DTYPES[dtype]
    arrays, m = _mat("ragged")
    x5 = _x((2, 2, 3, m.n_cols, 6), dt)
    view = x5[:, -1]
    k = ops._two_leading(view)
    assert k.data_ptr() == view.data_ptr() and k.shape == (2, 3, m.n_cols, 6) and k.stride()[:2] == (view.stride(0), view.stride(1))
    cols = torch.tensor([5, 0, 2], dtype=torch.int32, device=DEV)
    y = ops.sparse_project(view, m, cols, out_dtype=torch.float32)
    assert y.shape == (2, 3, m.n_rows, 3)
    _check(y, *_reference(arrays, view, cols, None, None, torch.float32), f"[B, E] slice {dtype}")
    assert torch.equal(y, ops.sparse_project(view.contiguous(), m, cols, out_dtype=torch.float32))
    saved = _ext.ENABLED
    _ext.ENABLED = False
    try:
        assert torch.equal(y, ops.sparse_project(view, m, cols, out_dtype=torch.float32))  # the ctypes path, same strides
    finally:
        _ext.ENABLED = saved


def test_backward_with_a_column_selected_twice_accumulates_in_fp32():
    arrays, m = _mat("ragged")
    x = _x((2, m.n_cols, 5), torch.bfloat16).requires_grad_(True)
    cols = torch.tensor([3, 3, 1], dtype=torch.int32, device=DEV)
    y = ops.sparse_project(x, m, cols, out_dtype=torch.float32)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    (gx,) = torch.autograd.grad(y, x, g)
    t = m.t
    t_arrays = (t.indptr.cpu().numpy(), t.indices.cpu().numpy(), t.values.cpu().numpy(), (t.n_rows, t.n_cols))
    want_c, bound_c = _reference(t_arrays, g, None, None, None, torch.float32)
    want, bound = torch.zeros(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.float64)
    want.index_add_(-1, cols.long().cpu(), want_c)
    bound.index_add_(-1, cols.long().cpu(), bound_c)
    # one fp32 add of the two contributions (2^-24 relative), then ONE rounding to bf16
    bound = bound + (2.0 ** -24 + H.U_OUT[torch.bfloat16]) * want.abs()
    _check(gx, want, bound, "backward, duplicate column")
