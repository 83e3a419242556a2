"""The imputer kernels of csrc/model_edge.hip - impute_columns_kernel, restore_nan_columns_kernel, the IMPUTE instantiations
assemble_input_chain_kernel<TI, TO, true, false>, assemble_input_chain_vec8_kernel<TI, TO, true, false> and
assemble_output_chain_kernel<TM, TS, true, false>, and column_program_kernel<T, 1> - called directly through their ``ops`` wrappers
with the discipline of tests/test_model_edge_kernels_gpu.py: past one 256-thread block, every dtype pair, every route of the chain
entry points, operands as column slabs of sentinel-filled buffers, against the plain-torch restatements of tests/imputer_refs.py (which
tests/test_imputer_cpu.py holds to the reference's recorded outputs).

Everything is BIT-equal (NaN at the same places, every other element the same bits, -0.0 and +-inf included) except the finite results of the
column program's kinds 1..9, which keep the per-op bound of model_edge_refs.bounding_ref; op 10 itself is exact.  The restatement alone
decides where NaN may remain (a non-imputed column, a NaN copy source, a member other than 0): no comparison drops or masks a position.
No number below comes from a kernel's output."""
import pytest
import torch

from tests import imputer_refs as I
from tests import model_edge_refs as R
from tests.model_edge_refs import BF16, F16, F32, NAME

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = [1, 257, 333]
PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)]  # (data dtype, model dtype)
LAYOUTS = [(2, 7, 5, 21), (2, 7, 5, 24), (3, 5, 0, 16), (1, 11, 0, 16), (1, 8, 0, 8), (2, 8, 4, 24), (2, 12, 0, 24)]  # (T, V, A, W)
# (2, 12, 0, 24): the smallest layout whose mask rows are 4-byte aligned (ldm = V = 12) AND whose 8-column groups do both things the mask
# store branches on: group 0 lies within step 0 (the packed two-word store), group 1 straddles t0|t1 (columns 8-11 of step 0: byte stores)
FILL = 7.0
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from anemoi_core_amd import ops as _ops

    return _ops


def _pair_id(p):
    return f"{NAME[p[0]]}-{NAME[p[1]]}"


def _slab(t, off, pad=4):
    wide = torch.full((*t.shape[:-1], t.shape[-1] + pad), FILL, dtype=t.dtype, device=DEV)
    wide[..., off:off + t.shape[-1]] = t.to(DEV)
    return wide[..., off:off + t.shape[-1]]


def _dev(t):
    return None if t is None else t.to(DEV)


def _program(V, mean, dtype):
    """Column 0 and the last column: constants (a statistic rounded once to the data dtype); column 2: a copy of column 1; the rest -
    column 1, the copy source, and column 3 among them - not imputed.  V >= 5."""
    kinds, values, sources = [0] * V, [0.0] * V, [0] * V
    for c in (0, V - 1):
        kinds[c], values[c] = 1, float(mean[c].to(dtype))
    kinds[2], sources[2] = 2, 1
    return kinds, values, sources


def _plant(x):
    """NaN on top of raw_data's specials, x [T, N, V] (V >= 5, program of ``_program``): in imputed columns at the first row, the last row,
    a whole row and a whole column; at one step but not the other; in a non-imputed column; in the copy source under a NaN target."""
    T, N, V = x.shape
    x[0, 0, 0] = NAN                 # first row, a constant column
    x[T - 1, N - 1, V - 1] = NAN     # last row, last column
    x[0, N // 2, :] = NAN            # a whole row of step 0 (not of the others when T > 1)
    x[T - 1, :, 2] = NAN             # the whole copy-target column of the last step
    x[0, N // 3, V - 1] = NAN        # step 0 only
    x[0, min(2, N - 1), 3] = NAN     # not imputed: stays
    x[T - 1, min(1, N - 1), 1] = NAN  # the copy source, where the target is NaN: NaN is what gets copied
    return x


def _on_device(ops, program):
    return ops.impute_program(*program, DEV)


# ------------------------------------------------------------------------------------------------------------ input assembly
def _route(W, to):
    """anemoi_assemble_input_chain: a 16-bit output of W % 8 == 0 takes the 8-column kernel, everything else the scalar one."""
    return "vec8" if to != F32 and W % 8 == 0 else "scalar"


def test_layouts_reach_both_routes_and_every_straddle():
    routes = {(lay, _route(lay[3], to)) for lay in LAYOUTS for _, to in PAIRS}
    assert {r for _, r in routes} == {"scalar", "vec8"}
    assert {lay for lay, r in routes if r == "vec8"} == set(LAYOUTS) - {(2, 7, 5, 21)} and {lay for lay, r in routes if r == "scalar"} == set(LAYOUTS)
    groups = lambda T, V, A, W: {(c // 8) for c in range(W)}  # noqa: E731
    straddles = lambda T, V, A, W, edge: 0 < edge < W and edge % 8 != 0 and edge // 8 in groups(T, V, A, W)  # noqa: E731
    assert straddles(2, 7, 5, 24, 7) and straddles(2, 7, 5, 24, 14) and straddles(2, 7, 5, 24, 19)  # t0|t1, x|attrs, attrs|zeros
    assert straddles(3, 5, 0, 16, 5) and straddles(3, 5, 0, 16, 10) and straddles(1, 11, 0, 16, 11)
    assert straddles(2, 12, 0, 24, 12) and 12 % 4 == 0 and 0 + 8 <= 12  # t0|t1 inside group 1, aligned mask rows, group 0 within step 0


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda s: "T%d-V%d-A%d-W%d" % s)
def test_assemble_input_impute_bit_equal(ops, layout, N, pair, norm):
    """ops.assemble_input(impute=, nan_mask=) == assemble_input_ref(impute_ref(x)) bit for bit, the mask == isnan(x[0]); x a row-strided
    slab, attrs a column slab.  Each step is imputed by its own NaN test and the copy source is read from the same step and row."""
    (T, V, A, W), (ti, to) = layout, pair
    mul, add, mean, stdev = R.column_stats(V, ti, seed=V)
    x = _plant(R.raw_data((T, N, V), ti, mean, stdev, seed=N + W, specials=True))
    attrs = torch.randn(N, A, generator=torch.Generator().manual_seed(50 + N)).to(to) if A else None
    program = _program(V, mean, ti)
    m, a = (mul, add) if norm else (None, None)
    want, want_mask = I.assemble_input_impute_ref(x, attrs, W, program, m, a, to)
    assert torch.equal(want_mask, x[0].isnan())
    mask = torch.zeros(N, V, dtype=torch.bool, device=DEV)
    got = ops.assemble_input(_slab(x, 2), None if attrs is None else _slab(attrs, 1), W, _dev(m), _dev(a), out_dtype=to,
                             impute=_on_device(ops, program), nan_mask=mask)
    R.assert_bits_equal(got, want, f"{_route(W, to)} N={N}")
    assert torch.equal(mask.cpu(), want_mask)
    body = want[:, :T * V].reshape(N, T, V)
    assert bool(body[..., 3].isnan().any()) and bool(body[..., 2].isnan().any())  # the non-imputed column and the NaN copy source kept theirs
    if T > 1 and N > 2:
        assert not bool(body[N // 2, 0, [0, V - 1]].isnan().any()) and bool(x[0, N // 2, 0].isnan())  # the whole NaN row: imputed
        assert bool(x[T - 1, 5 % N, 2].isnan()) and not bool(x[0, 5 % N, 2].isnan())  # NaN at one step, not the other ...
        if m is None:
            assert torch.equal(body[5 % N, T - 1, 2], body[5 % N, T - 1, 1])  # ... copied from the same step and row


def test_assemble_input_without_the_new_keywords_is_unchanged(ops):
    """A call without impute / nan_mask takes the routes it took: the same bits as the unchanged restatement, NaN passing through."""
    T, V, A, N = 2, 7, 5, 257
    for (ti, to), W in ((p, w) for p in PAIRS for w in (21, 24)):
        mul, add, mean, stdev = R.column_stats(V, ti, seed=3)
        x = _plant(R.raw_data((T, N, V), ti, mean, stdev, seed=W))
        attrs = torch.randn(N, A, generator=torch.Generator().manual_seed(1)).to(to)
        R.assert_bits_equal(ops.assemble_input(x.to(DEV), attrs.to(DEV), W, mul.to(DEV), add.to(DEV), out_dtype=to),
                            R.assemble_input_ref(x, attrs, W, mul, add, to), "normaliser only")
        if ti == to:
            R.assert_bits_equal(ops.assemble_input(x.to(DEV), attrs.to(DEV), W), R.assemble_input_ref(x, attrs, W), "plain")


# ------------------------------------------------------------------------------------------------------------ residual
V_IN = 53


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
@pytest.mark.parametrize("V_out", [5, 37])
def test_assemble_output_impute_bit_equal(ops, V_out, pair, norm):
    """ops.assemble_output(impute=) == assemble_output_ref on the imputed skip, bit for bit; N in ROWS, the skip contiguous and a slab; the
    column map names imputed, copied, source and plain skip columns."""
    ts, tm = pair
    mul, add, mean, stdev = R.column_stats(V_IN, ts, seed=V_out)
    m, a = (mul, add) if norm else (None, None)
    program = _program(V_IN, mean, ts)
    col_map = torch.full((V_out,), -1, dtype=torch.int32)
    col_map[:5] = torch.tensor([0, 2, 1, V_IN - 1, 3], dtype=torch.int32)
    for N in ROWS:
        skip = _plant(R.raw_data((1, N, V_IN), ts, mean, stdev, seed=N))[0]
        x_out = torch.randn(N, V_out, generator=torch.Generator().manual_seed(N + V_out)).to(tm)
        if N > 1:
            x_out[N // 2, 1], x_out[3, 0] = NAN, float("inf")
        want = I.assemble_output_impute_ref(x_out, skip, col_map, program, m, a)
        assert bool(want[:, 4].isnan().any()) and not bool(want[0, [0, 3]].isnan().any())
        for lay, sd in (("contiguous", skip.to(DEV)), ("slab", _slab(skip, 3, pad=5))):
            got = ops.assemble_output(x_out.to(DEV), sd, col_map.to(DEV), _dev(m), _dev(a), impute=_on_device(ops, program))
            R.assert_bits_equal(got, want, f"N={N} x_skip {lay}")
        # without the keyword: the bits of before
        R.assert_bits_equal(ops.assemble_output(x_out.to(DEV), skip.to(DEV), col_map.to(DEV), _dev(m), _dev(a)),
                            R.assemble_output_ref(x_out, skip, col_map, m, a), f"N={N} no imputer")


# ------------------------------------------------------------------------------------------------------------ output column program
def _tables(prog):
    from anemoi_core_amd.layers.bounding import program_tables

    return program_tables(prog, DEV)


def _masked(prog):
    """(op table, parameter table), {n_nan_ops: the count of kind-10 ops, taken on the host when the tables are built}."""
    from anemoi_core_amd.layers.bounding import masked_program_tables

    t = masked_program_tables(prog, DEV)
    return (t.ops, t.params), {"n_nan_ops": t.n_nan_ops}


def _mask(N, V, seed):
    mask = torch.rand(N, V, generator=torch.Generator().manual_seed(seed)) < 0.2
    mask[0, :], mask[N - 1, V - 1], mask[:, 1] = True, True, True  # first row, last element, a whole column
    return mask


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("N", [1, 256, 257, 333])
def test_op_10_alone_is_exact(ops, N, dtype):
    """Kind 10 alone: NaN exactly where mask[n, src], every other bit untouched (-0.0, +-inf, the columns no op names)."""
    V, VM = 6, 9
    x = R.raw_data((1, 1, 1, N, V), dtype, torch.zeros(V, dtype=torch.float64), torch.ones(V, dtype=torch.float64), seed=N)
    mask = _mask(N, VM, N)
    prog = [(10, 0, 8, 0.0, 0.0), (10, 4, 1, 0.0, 0.0), (10, 5, 0, 0.0, 0.0)]
    want = I.restore_nan_ref(x, mask[None], [(d, s) for _, d, s, _, _ in prog])
    xd = x.to(DEV)
    tables, count = _masked(prog)
    assert count == {"n_nan_ops": 3}
    assert ops.bound_columns_(xd, *tables, nan_mask=mask.to(DEV), **count) is xd
    R.assert_bits_equal(xd, want, "op 10")
    assert bool(xd[0, 0, 0, :, 4].isnan().all()) and torch.equal(xd[..., 0].isnan().cpu().reshape(N), mask[:, 8] | x[..., 0].isnan().reshape(N))


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("N", [1, 257, 1000])
def test_op_10_after_boundings_and_denormalisation(ops, N, dtype):
    """The predict_step program: boundings, kind 9 on every column, then kind 10 - one launch.  NaN exactly where the float64 evaluation
    or the mask has it, +-inf exactly, the finite rest within bounding_ref's per-op bound; the same program without a mask is unchanged."""
    V = 10
    x = (1.5 * torch.randn(1, 1, 1, N, V, generator=torch.Generator().manual_seed(N))).to(dtype)
    if N > 1:
        x[0, 0, 0, N // 2, 0], x[0, 0, 0, N - 1, 3], x[0, 0, 0, N // 4, 1] = NAN, NAN, float("inf")
    g = torch.Generator().manual_seed(77)
    mul, add = (0.5 + 3.5 * torch.rand(V, generator=g)).tolist(), (4.0 * torch.rand(V, generator=g) - 2.0).tolist()
    base = [(1, 0, 0, 0.0, 0.0), (7, 1, 0, 0.0, 1.0), (5, 4, 0, -0.5, 0.7), (4, 4, 0, 0.1, 0.0)] + [(9, c, 0, add[c], mul[c]) for c in range(V)]
    nan_ops = [(10, 1, 0, 0.0, 0.0), (10, 4, 6, 0.0, 0.0), (10, 9, 1, 0.0, 0.0)]
    mask = _mask(N, 7, N)
    want, bound = I.bounding_mask_ref(x, base + nan_ops, mask.reshape(1, 1, 1, N, 7))
    assert bool(want[..., 9].isnan().all())
    xd = x.to(DEV)
    tables, count = _masked(base + nan_ops)
    ops.bound_columns_(xd, *tables, nan_mask=mask.to(DEV), **count)
    R.check_bounding(xd.cpu(), want, bound, "boundings + kind 9 + kind 10")
    # the mask kernel and the plain kernel make the same bits of the kinds 1..9
    a, b = x.to(DEV), x.to(DEV)
    ops.bound_columns_(a, *_tables(base))
    ops.bound_columns_(b, *_tables(base), nan_mask=torch.zeros(N, 7, dtype=torch.bool, device=DEV))
    R.assert_bits_equal(b, a.cpu(), "kinds 1..9 through the mask kernel")
    R.check_bounding(a.cpu(), *R.bounding_ref(x, base), "no keyword: as before")


def test_error_paths(ops):
    x = torch.zeros(9, 4, device=DEV)
    prog = [(10, 0, 1, 0.0, 0.0)]
    with pytest.raises(ValueError, match="need a mask"):  # the unmasked tables cannot hold an op 10 at all
        _tables(prog)
    tables, count = _masked(prog)
    with pytest.raises(ValueError, match="no mask"):
        ops.bound_columns_(x, *tables, **count)
    with pytest.raises(ValueError):
        ops.bound_columns_(x, *tables, nan_mask=torch.zeros(8, 4, dtype=torch.bool, device=DEV), **count)  # rows do not match
    with pytest.raises(ValueError):
        ops.bound_columns_(x, *tables, nan_mask=torch.zeros(9, 4, dtype=torch.uint8, device=DEV), **count)
    program = ops.impute_program([1, 0, 0, 0], [1.0, 0, 0, 0], [0, 0, 0, 0], DEV)
    with pytest.raises(ValueError, match="go together"):
        ops.assemble_input(torch.zeros(1, 9, 4, device=DEV), None, 4, impute=program)
    with pytest.raises(ValueError):
        ops.assemble_input(torch.zeros(1, 9, 4, device=DEV), None, 4, impute=program, nan_mask=torch.zeros(9, 5, dtype=torch.bool, device=DEV))
    with pytest.raises(NotImplementedError):  # a copy from an imputed column
        ops.impute_program([1, 2, 0], [1.0, 0.0, 0.0], [0, 0, 0], DEV)
    with pytest.raises(NotImplementedError):  # a copy from a column past the width
        ops.impute_program([0, 2, 0], [0.0, 0.0, 0.0], [0, 3, 0], DEV)
    with pytest.raises(ValueError):
        ops.impute_columns(torch.zeros(9, 4, device=DEV), program)


# ------------------------------------------------------------------------------------------------------------ stand-alone kernels
def _batch(shape, dtype, mean, stdev, seed):
    """[B, T, (E,) N, V] raw data with ``_plant`` applied to every (batch, member) slice and, with members, NaN in member 1 ONLY at one
    place (it stays) and a member-0 NaN whose other member holds a number (it is imputed all the same)."""
    x = R.raw_data(shape, dtype, mean, stdev, seed=seed)
    B, T = shape[:2]
    if len(shape) == 4:
        for b in range(B):
            _plant(x[b])
    else:
        for b in range(B):
            for e in range(shape[2]):
                _plant(x[b, :, e])
        if shape[2] > 1 and shape[3] > 8:
            x[0, 0, 1, 7, 0] = NAN
            x[0, 0, 0, 7, 0] = 1.0
            x[B - 1, T - 1, 0, 8, 0] = NAN
            x[B - 1, T - 1, 1, 8, 0] = 2.0
    return x


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("shape", [(1, 1, 1, 7), (2, 2, 257, 7), (2, 2, 2, 333, 5), (1, 3, 1, 257, 11)], ids=lambda s: "x".join(map(str, s)))
def test_impute_columns_bit_equal(ops, shape, dtype):
    """ops.impute_columns == impute_ref bit for bit: out of place (x untouched), into a given out, in place; x contiguous and a row-strided
    slab; two members with the member-0 rule; batch 2; the mask == isnan of step 0, member 0, every column."""
    V = shape[-1]
    _, _, mean, stdev = R.column_stats(V, dtype, seed=V)
    x = _batch(shape, dtype, mean, stdev, seed=sum(shape))
    program = _program(V, mean, dtype)
    want, want_mask = I.impute_ref(x, program)
    prog = _on_device(ops, program)
    for what, xd in (("contiguous", x.to(DEV)), ("slab", _slab(x, 2))):
        mask = torch.zeros(want_mask.shape, dtype=torch.bool, device=DEV)
        got = ops.impute_columns(xd, prog, mask=mask)
        R.assert_bits_equal(got, want, f"{what}, out of place")
        R.assert_bits_equal(xd, x, f"{what}: x untouched")
        assert torch.equal(mask.cpu(), want_mask)
        out = torch.full(shape, FILL, dtype=dtype, device=DEV)
        assert ops.impute_columns(xd, prog, out=out) is out
        R.assert_bits_equal(out, want, f"{what}, given out")
        assert ops.impute_columns(xd, prog, out=xd) is xd
        R.assert_bits_equal(xd, want, f"{what}, in place")
    if len(shape) == 5 and shape[2] > 1:
        assert bool(want[0, 0, 1, 7, 0].isnan()) and not bool(want[-1, -1, :, 8, 0].isnan().any())


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("shape", [(1, 1, 5), (2, 1, 257, 6), (2, 1, 2, 333, 6), (1, 2, 1, 257, 9)], ids=lambda s: "x".join(map(str, s)))
def test_restore_nan_columns_bit_equal(ops, shape, dtype):
    """ops.restore_nan_columns == restore_nan_ref bit for bit, out of place and in place; the [batch, grid, vars] mask is broadcast over
    every dimension between batch and grid."""
    B, N, V = shape[0], shape[-2], shape[-1]
    x = R.raw_data(shape, dtype, torch.zeros(V, dtype=torch.float64), torch.ones(V, dtype=torch.float64), seed=N)
    VM = 7
    mask = torch.stack([_mask(N, VM, 10 + b) for b in range(B)])
    pairs = [(0, 6), (V - 1, 1), (2, 0)]
    src_of = torch.full((V,), -1, dtype=torch.int32)
    for dst, src in pairs:
        src_of[dst] = src
    want = I.restore_nan_ref(x, mask, pairs)
    xd = x.to(DEV)
    got = ops.restore_nan_columns(xd, mask.to(DEV), src_of.to(DEV))
    R.assert_bits_equal(got, want, "out of place")
    R.assert_bits_equal(xd, x, "x untouched")
    assert ops.restore_nan_columns(xd, mask.to(DEV), src_of.to(DEV), out=xd) is xd
    R.assert_bits_equal(xd, want, "in place")


@pytest.mark.parametrize("name", ["InputImputer", "ConstantImputer", "CopyImputer"])
def test_modules_on_device_equal_the_reference(golden, name):
    """The three imputer classes on CUDA tensors (preprocessing/imputer.py -> ops.impute_columns / ops.restore_nan_columns) against the
    reference's recorded outputs, both widths, with and without an ensemble dimension, in place and out of place."""
    from tests.imputer_helpers import KEYS, build

    fx = golden("imputer.pt")
    for key in KEYS:
        want = fx["cases"][name][key]
        imp = build(fx, name)
        x = fx["inputs"][key].to(DEV)
        R.assert_bits_equal(imp.transform(x, in_place=False), want["transform"], f"{key} transform")
        R.assert_bits_equal(x, fx["inputs"][key], "x untouched")
        assert torch.equal(imp.nan_locations.cpu(), want["nan_locations"])
        if want["loss_mask_training"] is not None:
            assert torch.equal(imp.loss_mask_training.cpu(), want["loss_mask_training"])
        o = fx["outputs"][key].to(DEV)
        R.assert_bits_equal(imp.inverse_transform(o, in_place=False), want["inverse"], f"{key} inverse")
        assert imp.transform(x) is x and imp.inverse_transform(o) is o
        R.assert_bits_equal(x, want["transform"], "in place")
        R.assert_bits_equal(o, want["inverse"], "in place inverse")
