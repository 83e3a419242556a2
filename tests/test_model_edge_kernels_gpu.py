"""The seven model-edge kernels of csrc/model_edge.hip without an imputer or a remapper - assemble_input_kernel,
assemble_input_chain_kernel<TI, TO, false, false>, assemble_input_chain_vec8_kernel<TI, TO, false, false>, assemble_output_kernel,
assemble_output_chain_kernel<TM, TS, false, false>, affine_columns_kernel and column_program_kernel<T, 0> - called directly through their ``ops`` wrappers, past one 256-thread block, at every branch the wrappers
and the entry points take, NaN and +-inf included, against the plain-torch CPU restatements of tests/model_edge_refs.py (which
tests/test_model_edge_refs_cpu.py holds to the reference's recorded outputs).

What is exact and what carries a bound:

* ``assemble_input``, ``assemble_output``, ``affine_columns`` / ``InputNormalizer``: BIT-equal (NaN at the same places, every
  other element the same bits, -0.0 included).  The kernels make the roundings torch makes: x * mul + add in two fp32 roundings
  (``mul_then_add``: contraction off), then one rounding to the output dtype; 16-bit ``affine_columns`` rounds to fp32 and then
  to T after each of its two steps, as torch's in-place ops do.
* ``bound_columns_``: NaN exactly where the float64 evaluation of the program has it and nowhere else, +-inf exactly, the finite
  rest within U[T] * s per op (model_edge_refs.bounding_ref derives it: fp32 2^-22, bf16 2^-7, fp16 2^-10 of
  s = max(|want|, |v|, |p0|, |p1|, |x[tot]|)).  Kinds 1 and 5 on fp32 are exact.  The leaky kinds are NOT asserted bit-equal to
  torch: the compiler contracts p0 + 0.01f * (t - p0) into one FMA where torch rounds twice, which the 2^-22 bound allows.

No number below comes from a kernel's output."""
import pytest
import torch

from tests import model_edge_refs as R
from tests.model_edge_refs import BF16, F16, F32, NAME

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = [1, 257, 333]  # N * W and N * W / 8 past one 256-thread block and no multiple of 256
PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)]  # (data dtype, model dtype)
FILL = 7.0  # what the columns around a slab hold: a kernel that reads or writes a neighbour changes a result


@pytest.fixture(scope="module")
def ops():
    from anemoi_core_amd import ops as _ops

    return _ops


def _pair_id(p):
    return f"{NAME[p[0]]}-{NAME[p[1]]}"


def _slab(t, off, pad=4):
    """The CPU tensor t [..., D] on the device as the column slab wide[..., off:off + D] of a [..., D + pad] buffer of FILL."""
    wide = torch.full((*t.shape[:-1], t.shape[-1] + pad), FILL, dtype=t.dtype, device=DEV)
    wide[..., off:off + t.shape[-1]] = t.to(DEV)
    return wide[..., off:off + t.shape[-1]]


def _attrs(N, A, dtype, seed=0):
    return torch.randn(N, A, generator=torch.Generator().manual_seed(50 + seed)).to(dtype) if A else None


def _dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------------------ assemble_input
def _input_route(T, V, A, W, ti, to, norm):
    """The kernel ops.assemble_input reaches for a contiguous input: ``plain_pad`` in ops.assemble_input (the plain kernel only without
    a normaliser, in one dtype and not plain_pad), then anemoi_assemble_input_chain (assemble_input_chain_launch: a 16-bit output with
    W % 8 == 0 takes the vec8 kernel, whose first branch is T == 1 && A == 0) or anemoi_assemble_input (Q = 4 when V, A, W are multiples
    of 4)."""
    plain_pad = T == 1 and A == 0 and to != F32 and W % 8 == 0
    if not norm and ti == to and not plain_pad:
        return "plain-q4" if V % 4 == 0 and A % 4 == 0 and W % 4 == 0 else "plain-q1"
    if to != F32 and W % 8 == 0:
        return "vec8-pad" if T == 1 and A == 0 else "vec8"
    return "scalar"


# (T, V, A, W): scalar norm kernel for every dtype (W % 8 != 0) | vec8 with 8-column groups across t0|t1 (7), x|attrs (14), attrs|zeros (19)
# | vec8 across two time boundaries, no attributes | the GNN embeddings' cast + pad, V < W and V == W | Q = 4 of the plain kernel
LAYOUTS = [(2, 7, 5, 21), (2, 7, 5, 24), (3, 5, 0, 16), (1, 11, 0, 16), (1, 8, 0, 8), (2, 8, 4, 24)]
EXPECTED_ROUTES = {  # layout -> the kernels it reaches over the dtype pairs, with and without a normaliser (checked below: no case drifts)
    (2, 7, 5, 21): {"scalar", "plain-q1"}, (2, 7, 5, 24): {"scalar", "vec8", "plain-q1"}, (3, 5, 0, 16): {"scalar", "vec8", "plain-q1"},
    (1, 11, 0, 16): {"scalar", "vec8-pad", "plain-q1"}, (1, 8, 0, 8): {"scalar", "vec8-pad", "plain-q4"}, (2, 8, 4, 24): {"scalar", "vec8", "plain-q4"},
}


def test_assemble_input_cases_reach_every_kernel_and_branch():
    """The table above selects what it says: every layout reaches exactly the kernels listed for it over the dtype pairs with and
    without a normaliser, and all five routes (``_input_route``) occur."""
    seen = set()
    for lay in LAYOUTS:
        routes = {_input_route(*lay, ti, to, norm) for ti, to in PAIRS for norm in (False, True)}
        assert routes == EXPECTED_ROUTES[lay], (lay, routes)
        seen |= routes
    assert seen == {"scalar", "vec8", "vec8-pad", "plain-q1", "plain-q4"}
    assert _input_route(2, 7, 5, 21, F32, BF16, True) == "scalar" and _input_route(1, 11, 0, 16, BF16, BF16, False) == "vec8-pad"


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda s: "T%d-V%d-A%d-W%d" % s)
def test_assemble_input_bit_equal(ops, layout, N, pair, norm):
    """ops.assemble_input on contiguous inputs == assemble_input_ref bit for bit.  The (layout, dtype pair, normaliser) triple
    picks the kernel (``_input_route``): assemble_input_kernel<T, 1 | 4> (anemoi_assemble_input),
    assemble_input_chain_kernel<TI, TO, false, false> (fp32 output, or W % 8 != 0: the vec8 route of assemble_input_chain_launch not
    taken), assemble_input_chain_vec8_kernel<TI, TO, false, false> general branch (8-column groups straddling t0|t1, x|attrs,
    attrs|zeros) or its T == 1 && A == 0 branch, which without col_mul is the plain_pad route of ops.assemble_input with mul == nullptr.  All six <TI, TO> pairs with float input or one
    16-bit dtype are instantiated by the five dtype pairs here."""
    (T, V, A, W), (ti, to) = layout, pair
    mul, add, mean, stdev = R.column_stats(V, ti, seed=V)
    x = R.raw_data((T, N, V), ti, mean, stdev, seed=N + W)
    attrs = _attrs(N, A, to, seed=N)
    m, a = (mul, add) if norm else (None, None)
    want = R.assemble_input_ref(x, attrs, W, m, a, to)
    got = ops.assemble_input(x.to(DEV), _dev(attrs), W, _dev(m), _dev(a), out_dtype=to)
    R.assert_bits_equal(got, want, f"{_input_route(T, V, A, W, ti, to, norm)} N={N}")
    if N > 1:
        assert bool(want.isnan().any()) and bool(want.isinf().any())  # the planted NaN / inf did pass through


@pytest.mark.parametrize("pair", [(F32, F32), (F32, BF16), (BF16, BF16), (F16, F16)], ids=_pair_id)
@pytest.mark.parametrize("W", [21, 24])
def test_assemble_input_model_layout_strided_views(ops, pair, W):
    """The model's real operands (models/encoder_processor_decoder.py, predict_step): x = batch[0, :, 0] of a [1, T, 1, N, V] batch;
    x a [T, N, V] slice of a buffer with a wider row (ldx = V + 4 > V, base pointer off by 2 elements); attrs a column slab of a
    wider buffer (lda = A + 4, off by 1).  assemble_input_chain_kernel (W = 21, or fp32 output) and the general branch of
    assemble_input_chain_vec8_kernel (W = 24, 16-bit output) index x by x.stride(0) / x.stride(1) (ops.assemble_input)."""
    ti, to = pair
    T, N, V, A = 2, 257, 7, 5
    mul, add, mean, stdev = R.column_stats(V, ti, seed=3)
    x = R.raw_data((T, N, V), ti, mean, stdev, seed=W)
    attrs = _attrs(N, A, to)
    want = R.assemble_input_ref(x, attrs, W, mul, add, to)
    batch = x.reshape(1, T, 1, N, V).to(DEV)
    for what, xd, ad in (("batch view", batch[0, :, 0], attrs.to(DEV)), ("row-strided x, attrs slab", _slab(x, 2), _slab(attrs, 1))):
        assert xd.shape == (T, N, V) and (what == "batch view" or (xd.stride(1) == V + 4 and ad.stride(0) == A + 4))
        R.assert_bits_equal(ops.assemble_input(xd, ad, W, mul.to(DEV), add.to(DEV), out_dtype=to), want, what)
    if ti == to:  # and the plain kernel on the same views (Q = 1: V = 7)
        R.assert_bits_equal(ops.assemble_input(_slab(x, 2), _slab(attrs, 1), W), R.assemble_input_ref(x, attrs, W), "plain kernel, strided")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("N", [257, 333])
def test_assemble_input_plain_q4_and_its_fallbacks(ops, dtype, N):
    """assemble_input_kernel<T, 4> (V, A, W multiples of 4, every stride a multiple of 4, every pointer 4-element aligned:
    ``q4`` in anemoi_assemble_input) and each way it falls back to <T, 1>: x with ldx % 4 != 0; attrs a slab starting at column 1, 2, 3 (lda % 4 == 0,
    pointer misaligned); the time stride ld_t % 4 != 0; and a slab that keeps Q = 4 (offset 4).  Pure data movement: bit-equal."""
    T, V, A, W = 2, 8, 4, 24
    _, _, mean, stdev = R.column_stats(V, dtype, seed=1)
    x = R.raw_data((T, N, V), dtype, mean, stdev, seed=N)
    attrs = _attrs(N, A, dtype)
    want = R.assemble_input_ref(x, attrs, W)
    xd, ad = x.to(DEV), attrs.to(DEV)
    R.assert_bits_equal(ops.assemble_input(xd, ad, W), want, "Q = 4, contiguous")
    R.assert_bits_equal(ops.assemble_input(_slab(x, 4, pad=8), _slab(attrs, 4, pad=4), W), want, "Q = 4, aligned slabs")
    x_odd = _slab(x, 0, pad=1)
    assert x_odd.stride(1) == V + 1
    R.assert_bits_equal(ops.assemble_input(x_odd, ad, W), want, "Q = 1: ldx % 4 != 0")
    for off in (1, 2, 3):
        a_off = _slab(attrs, off, pad=4)
        assert a_off.stride(0) % 4 == 0 and (a_off.data_ptr() // a_off.element_size()) % 4 == off
        R.assert_bits_equal(ops.assemble_input(xd, a_off, W), want, f"Q = 1: attrs slab at column {off}")
    flat = torch.full((T * (N * V + 2),), FILL, dtype=dtype, device=DEV)
    x_t = flat.as_strided((T, N, V), (N * V + 2, V, 1))
    x_t.copy_(xd)
    assert x_t.stride(0) % 4 == 2
    R.assert_bits_equal(ops.assemble_input(x_t, ad, W), want, "Q = 1: ld_t % 4 != 0")


def test_assemble_input_error_paths(ops):
    """ops.assemble_input refuses (ValueError) col_mul without col_add, width < T * V + A and attrs of another dtype, and 16-bit x
    with another 16-bit out_dtype (the shared argument checks of ops.assemble_input)."""
    x = torch.zeros(2, 9, 7, device=DEV)
    attrs = torch.zeros(9, 5, device=DEV)
    mul = torch.ones(7, device=DEV)
    with pytest.raises(ValueError):
        ops.assemble_input(x, attrs, 24, col_mul=mul)
    with pytest.raises(ValueError):
        ops.assemble_input(x, attrs, 24, col_add=mul)
    with pytest.raises(ValueError):
        ops.assemble_input(x, attrs, 18, mul, mul)
    with pytest.raises(ValueError):
        ops.assemble_input(x, attrs.to(BF16), 24, mul, mul)
    with pytest.raises(ValueError):
        ops.assemble_input(x, attrs, 24, mul, mul, out_dtype=BF16)  # attrs must be in the OUTPUT dtype
    with pytest.raises(ValueError):
        ops.assemble_input(x.to(BF16), attrs.to(F16), 24, mul, mul, out_dtype=F16)
    with pytest.raises(ValueError):
        ops.assemble_input(x.to(F16), None, 24, out_dtype=BF16)


# ------------------------------------------------------------------------------------------------------------ assemble_output
V_IN = 53


def _col_maps(V_out):
    g = torch.Generator().manual_seed(V_out)
    mixed = torch.full((V_out,), -1, dtype=torch.int32)
    mixed[torch.randperm(V_out, generator=g)[:(V_out + 1) // 2]] = torch.randint(0, V_IN, ((V_out + 1) // 2,), generator=g, dtype=torch.int32)
    mixed[0], mixed[V_out - 1] = 11, 11  # the same skip column twice
    mixed[V_out // 2] = V_IN - 1         # the last skip column
    return {"none": torch.full((V_out,), -1, dtype=torch.int32), "all": torch.randint(0, V_IN, (V_out,), generator=g, dtype=torch.int32), "mixed": mixed}


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
@pytest.mark.parametrize("V_out", [5, 37, 84])
def test_assemble_output_bit_equal(ops, V_out, pair, norm):
    """ops.assemble_output == assemble_output_ref bit for bit, for N in {1, 257, 333}, col_map all -1 / all mapped / mixed (one
    skip column mapped twice, the last skip column mapped), x_skip contiguous and a row-strided slab.  (TS, TM) = (data, model)
    dtype: with a normaliser, or with fp32 data under a 16-bit model, assemble_output_chain_kernel<TM, TS, false, false> (the plain route of
    ops.assemble_output not taken; anemoi_assemble_output_chain picks TS = float or TM); the same dtype without a normaliser is
    assemble_output_kernel<T, 1 | 4> (``q4`` in anemoi_assemble_output: Q = 4 at V_out = 84)."""
    ts, tm = pair
    mul, add, mean, stdev = R.column_stats(V_IN, ts, seed=V_out)
    m, a = (mul, add) if norm else (None, None)
    for N in ROWS:
        skip = R.raw_data((N, V_IN), ts, mean, stdev, seed=N)
        x_out = torch.randn(N, V_out, generator=torch.Generator().manual_seed(N + V_out)).to(tm)
        if N > 1:
            x_out[N // 2, V_out // 2], x_out[3, 0] = float("nan"), float("inf")
        for name, col_map in _col_maps(V_out).items():
            want = R.assemble_output_ref(x_out, skip, col_map, m, a)
            for lay, sd in (("contiguous", skip.to(DEV)), ("slab", _slab(skip, 3, pad=5))):
                got = ops.assemble_output(x_out.to(DEV), sd, col_map.to(DEV), _dev(m), _dev(a))
                R.assert_bits_equal(got, want, f"N={N} col_map={name} x_skip {lay}")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_assemble_output_plain_q4_and_its_fallbacks(ops, dtype):
    """assemble_output_kernel<T, 4> (V_out = 84, contiguous, and a slab at column offset 4) and its fall-backs to <T, 1>
    (``q4`` in anemoi_assemble_output): row-strided x_out with ldx % 4 != 0, and x_out a slab at an odd column offset (ldx % 4 == 0, pointer
    misaligned).  V_out % 4 != 0 is covered by test_assemble_output_bit_equal (5, 37)."""
    N, V_out = 257, 84
    _, _, mean, stdev = R.column_stats(V_IN, dtype)
    skip = R.raw_data((N, V_IN), dtype, mean, stdev)
    x_out = torch.randn(N, V_out, generator=torch.Generator().manual_seed(5)).to(dtype)
    col_map = _col_maps(V_out)["mixed"]
    want = R.assemble_output_ref(x_out, skip, col_map)
    for what, xd in (("Q = 4 contiguous", x_out.to(DEV)), ("Q = 4 slab at 4", _slab(x_out, 4, pad=8)), ("Q = 1: ldx = 85", _slab(x_out, 0, pad=1)),
                     ("Q = 1: slab at 1", _slab(x_out, 1, pad=4)), ("Q = 1: slab at 3", _slab(x_out, 3, pad=4))):
        R.assert_bits_equal(ops.assemble_output(xd, _slab(skip, 3, pad=5), col_map.to(DEV)), want, what)


def test_assemble_output_unsupported_pairs_raise(ops):
    """fp32 x_out with 16-bit x_skip, and two different 16-bit dtypes, are refused by ops.assemble_output and
    anemoi_assemble_output_chain (check_chain) as a ValueError: no tensor comes back that could be mistaken for a result."""
    col_map = torch.tensor([0, -1, 2], dtype=torch.int32, device=DEV)
    for tm, ts in ((F32, BF16), (F32, F16), (BF16, F16), (F16, BF16)):
        with pytest.raises(ValueError):
            ops.assemble_output(torch.zeros(9, 3, dtype=tm, device=DEV), torch.zeros(9, 4, dtype=ts, device=DEV), col_map)
    with pytest.raises(ValueError):  # col_mul without col_add (check_chain in model_edge.hip)
        ops.assemble_output(torch.zeros(9, 3, device=DEV), torch.zeros(9, 4, device=DEV), col_map, col_mul=torch.ones(4, device=DEV))


# ------------------------------------------------------------------------------------------------------------ affine_columns
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("lead", [(), (2, 3)], ids=["2d", "4d"])
@pytest.mark.parametrize("NV", [(1, 1), (37, 7), (300, 7), (257, 101)], ids=lambda s: "N%d-V%d" % s)
def test_affine_columns_bit_equal(ops, NV, lead, dtype, inverse):
    """ops.affine_columns == torch's own in-place sequence on a CPU tensor of the same dtype (x.mul_(mul).add_(add) /
    x.subtract_(add).div_(mul)), bit for bit: affine_columns_kernel<T>, forward (fp32: mul_then_add; 16 bit: a rounding to T after
    each step) and inverse, the row / column split i / V, i % V up to 6 * 257 * 101 elements
    (607 blocks); out of place, in place (out = x) and into a given out (ops.affine_columns).  N257-V101-4d-fp16-forward is the case that
    found the fp16 forward rounding its product ONCE (x * mul and the conversion selected as one v_fma_mixlo_f16) where torch rounds to
    fp32 and then to fp16: 4 of 155 742 elements, those whose fp32 product is a tie between two fp16 values (``mul_f32`` in
    model_edge.hip keeps the fp32 value)."""
    N, V = NV
    mul, add, mean, stdev = R.column_stats(V, dtype, seed=N)
    x = R.raw_data((*lead, N, V), dtype, mean, stdev, seed=V)
    if inverse:
        x = R.affine_ref(x, mul, add)  # normalised values are what the inverse sees
    want = R.affine_ref(x, mul, add, inverse)
    md, ad = mul.to(DEV), add.to(DEV)
    xd = x.to(DEV)
    got = ops.affine_columns(xd, md, ad, inverse=inverse)
    assert got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu().view(R.INT_VIEW[dtype]), x.view(R.INT_VIEW[dtype]))  # x untouched
    R.assert_bits_equal(got, want, "out of place")
    out = torch.full_like(xd, FILL)
    assert ops.affine_columns(xd, md, ad, inverse=inverse, out=out) is out
    R.assert_bits_equal(out, want, "given out")
    assert ops.affine_columns(xd, md, ad, inverse=inverse, out=xd) is xd
    R.assert_bits_equal(xd, want, "in place")


def test_affine_columns_refuses_a_non_contiguous_input(ops):
    """ops.affine_columns: a non-contiguous x (a column slab, a transposed view) raises instead of being read with the wrong stride."""
    one = torch.ones(7, device=DEV)
    with pytest.raises(ValueError):
        ops.affine_columns(torch.zeros(9, 11, device=DEV)[:, 2:9], one, one)
    with pytest.raises(ValueError):
        ops.affine_columns(torch.zeros(7, 9, device=DEV).t(), one, one)
    with pytest.raises(ValueError):
        ops.affine_columns(torch.zeros(9, 7, device=DEV), one, one, out=torch.zeros(9, 7, dtype=BF16, device=DEV))


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_input_normalizer_on_device_equals_the_cpu_sequence(golden, dtype):
    """InputNormalizer.transform / inverse_transform with data_index on a CUDA [2, 2, 1, 300, V] tensor (preprocessing/normalizer.py
    of this package: _affine -> ops.affine_columns) == the same in-place torch sequence on the CPU, with the statistics the
    reference's normaliser recorded (tests/golden/edges.pt)."""
    from anemoi_core_amd.preprocessing import InputNormalizer
    from tests.helpers import indices_from_fixture

    c = golden("edges.pt")["normalizer"]
    nm = InputNormalizer(config=c["data_config"]["normalizer"], data_indices=indices_from_fixture(c["indices"]),
                         statistics={k: v.numpy().copy() for k, v in c["statistics"].items()}).to(DEV)
    idx = [0, 2, 7, 5, 1]
    mul, add = c["buffers"]["_norm_mul"][idx], c["buffers"]["_norm_add"][idx]
    x = (4.0 * torch.randn(2, 2, 1, 300, len(idx), generator=torch.Generator().manual_seed(9))).to(dtype)
    x[1, 0, 0, 299, 4], x[0, 1, 0, 17, 2] = float("nan"), float("-inf")
    for inverse, fn in ((False, nm.transform), (True, nm.inverse_transform)):
        want = R.affine_ref(x, mul, add, inverse)
        R.assert_bits_equal(fn(x.to(DEV), in_place=False, data_index=idx), want, f"inverse={inverse}")
        xd = x.to(DEV)
        assert fn(xd, data_index=idx) is xd
        R.assert_bits_equal(xd, want, f"inverse={inverse}, in place")


# ------------------------------------------------------------------------------------------------------------ bound_columns_
def _tables(prog):
    from anemoi_core_amd.layers.bounding import program_tables

    return program_tables(prog, DEV)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("pair", R.BOUND_PAIRS, ids=lambda p: "p%g_%g" % p)
@pytest.mark.parametrize("kind", range(1, 10))
def test_bound_columns_each_kind_at_its_bounds(ops, kind, pair, dtype):
    """column_program_kernel<T, 0> through ops.bound_columns_, one op of ``kind`` (the kernel's one switch) on column 0 of a [n, 3] tensor (column 1: the
    total of kinds 7 / 8; column 2: not named by the program), on inputs dense around the bounds - p0, p1, their neighbours on both
    sides, 0, -0.0, +-tiny, +-large, +-inf, NaN - plus 320 random ones (model_edge_refs.bounding_inputs): some 335 rows, two blocks.
    NaN exactly where the float64 evaluation has it (kinds 1, 3, 5, 7 returned 0 / p0 for NaN while they used fmaxf / fminf),
    +-inf exactly, the rest within U[T] * s; kinds 1 and 5 exact in fp32; the leaky kinds are one FMA where torch rounds twice,
    hence the bound and not bit-equality (see the module docstring).  Columns 1 and 2 come back bit-unchanged."""
    p0, p1 = pair
    v = R.bounding_inputs(p0, p1, dtype, seed=kind)
    x = torch.stack([v, R.total_column(v.numel(), dtype, seed=kind), torch.full_like(v, FILL)], -1).contiguous()
    prog = [(kind, 0, 1, p0, p1)]
    want, bound = R.bounding_ref(x, prog)
    assert float(want[want.isfinite()].abs().max()) < 0.9 * torch.finfo(dtype).max  # the input set overflows in no kind
    xd = x.to(DEV)
    assert ops.bound_columns_(xd, *_tables(prog)) is xd
    got = xd.cpu()
    R.check_bounding(got, want, bound, f"kind {kind}")
    R.assert_bits_equal(got[:, 1:], x[:, 1:], "columns the program does not name")
    assert bool(want[:, 0].isnan().any())
    if dtype == F32 and kind in (1, 5):
        fin = want[:, 0].isfinite()
        assert torch.equal(got[:, 0].double()[fin], want[:, 0][fin]), "kinds 1 and 5 are exact on fp32"
    if kind in (7, 8):  # a NaN total makes the fraction NaN, whatever the bounded value
        assert bool(got[x[:, 1].isnan(), 0].isnan().all())


ORDER_PROGRAM = [
    (1, 0, 0, 0.0, 0.0), (7, 1, 0, 0.0, 1.0), (8, 2, 0, 0.0, 1.0),  # relu on the total column, then two fractions of it
    (7, 5, 3, 0.0, 1.0), (3, 3, 0, 0.25, 0.0),                       # a fraction of column 3, bounded only LATER: takes the unbounded value
    (5, 4, 0, -0.5, 0.7), (4, 4, 0, 0.1, 0.0),                       # the same column bounded twice
]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_bound_columns_order_dependent_programs(ops, N, dtype):
    """column_program_kernel<T, 0> on a contiguous [1, 1, 1, N, 10] tensor as the model passes it (``_assemble_output``), one
    row per thread across the block boundary (N = 255, 256, 257, 1000), with programs whose result depends on
    the order of the ops (the kernel's loop over the ops reads and writes the row in place): relu on the total column THEN two
    fractions of it; a fraction whose total is bounded later (it takes the unbounded value, as the reference's sequence of modules
    does); one column bounded twice; and all of it followed by kind 9 on every column - the predict_step program of
    encoder_processor_decoder.py:314-317.  A NaN in a total column makes the fractions of that row NaN; the columns the first program
    does not name (6 .. 9) come back bit-unchanged."""
    V = 10
    x = (1.5 * torch.randn(1, 1, 1, N, V, generator=torch.Generator().manual_seed(N))).to(dtype)
    rows = x[0, 0, 0]
    if N > 1:
        rows[N // 2, 0], rows[N - 1, 3], rows[N // 3, 4] = float("nan"), float("nan"), float("nan")
        rows[N // 4, 0], rows[N // 5, 1], rows[N - 2, 2] = float("inf"), float("-inf"), float("inf")
    else:
        rows[0, 3] = float("nan")
    want, bound = R.bounding_ref(x, ORDER_PROGRAM)
    # the fraction of column 3 used the UNBOUNDED total: with the bounded one (>= 0.25) the result would differ where x[3] < 0.25
    low = (rows[:, 3].double() < 0.25) & rows[:, 5].isfinite() & (rows[:, 5] != 0)
    assert torch.equal(want[0, 0, 0, low, 5], torch.clamp(rows[low, 5].double(), 0.0, 1.0) * rows[low, 3].double())
    xd = x.to(DEV)
    ops.bound_columns_(xd, *_tables(ORDER_PROGRAM))
    got = xd.cpu()
    R.check_bounding(got, want, bound, "boundings")
    R.assert_bits_equal(got[..., 6:], x[..., 6:], "columns the program does not name")
    nan_total = rows[:, 0].isnan()
    assert bool(got[0, 0, 0, nan_total][:, 1:3].isnan().all()) and bool(got[0, 0, 0, rows[:, 3].isnan(), 5].isnan().all())
    # ... followed by the de-normalisation of every column
    g = torch.Generator().manual_seed(77)
    mul, add = (0.5 + 3.5 * torch.rand(V, generator=g)).tolist(), (4.0 * torch.rand(V, generator=g) - 2.0).tolist()
    prog = ORDER_PROGRAM + [(9, c, 0, add[c], mul[c]) for c in range(V)]
    want, bound = R.bounding_ref(x, prog)
    xd = x.to(DEV)
    ops.bound_columns_(xd, *_tables(prog))
    R.check_bounding(xd.cpu(), want, bound, "boundings + kind 9")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: NAME[d])
def test_bounding_modules_on_device_equal_the_torch_program(ops, dtype):
    """BaseBounding.forward of all eight bounding classes in sequence on a CUDA tensor (layers/bounding.py:74-80 -> ops.bound_columns_,
    one launch per module) == apply_program_torch of the concatenated program on the CPU (torch's fp32 ops on the same T-rounded
    input) and == the float64 evaluation, both to the bound of bounding_ref, NaN and +-inf exactly."""
    from anemoi_core_amd.layers import bounding as B

    n2i = {f"v{i}": i for i in range(10)}
    stats = {k: torch.linspace(lo, hi, 12).double().numpy() for k, (lo, hi) in (("mean", (-1, 1)), ("stdev", (0.5, 2)), ("min", (-3, -1)), ("max", (1, 4)))}
    kw = dict(name_to_index=n2i, statistics=stats, name_to_index_stats={f"v{i}": i + 1 for i in range(10)})
    mods = [B.ReluBounding(variables=["v0", "v3"], **kw), B.LeakyReluBounding(variables=["v1"], **kw),
            B.NormalizedReluBounding(variables=["v2", "v4"], min_val=[0.1, -0.2], normalizer=["mean-std", "min-max"], **kw),
            B.NormalizedLeakyReluBounding(variables=["v5", "v9"], min_val=[0.3, 0.0], normalizer=["max", "std"], **kw),
            B.HardtanhBounding(variables=["v6"], min_val=-0.5, max_val=0.7, **kw), B.LeakyHardtanhBounding(variables=["v7"], min_val=0.0, max_val=1.0, **kw),
            B.FractionBounding(variables=["v8"], min_val=0.0, max_val=1.0, total_var="v0", **kw),
            B.LeakyFractionBounding(variables=["v1"], min_val=0.0, max_val=1.0, total_var="v3", **kw)]
    prog = [op for m in mods for op in m.program()]
    assert sorted({op[0] for op in prog}) == list(range(1, 9))
    N = 257
    x = (1.5 * torch.randn(1, 1, 1, N, 10, generator=torch.Generator().manual_seed(11))).to(dtype)
    for c in range(10):
        x[0, 0, 0, 20 + c, c], x[0, 0, 0, 40 + c, c], x[0, 0, 0, 60 + c, c] = float("nan"), float("inf"), float("-inf")
    want, bound = R.bounding_ref(x, prog)
    on_cpu = B.apply_program_torch(x.float(), prog).double()
    assert torch.equal(on_cpu.isnan(), want.isnan()) and torch.equal(on_cpu.isinf(), want.isinf())
    y = x.clone().to(DEV)
    for m in mods:
        y = m.to(DEV)(y)
    R.check_bounding(y.cpu(), want, bound, "modules vs float64")
    R.check_bounding(y.cpu(), on_cpu, bound, "modules vs apply_program_torch")
