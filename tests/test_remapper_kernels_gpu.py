"""The remapper / post-processor kernels of csrc/model_edge.hip (remap_core.h) - remap_columns_kernel, the REMAP instantiations
assemble_input_chain_kernel<TI, TO, IMPUTE, true>, assemble_input_chain_vec8_kernel<TI, TO, IMPUTE, true> and
assemble_output_chain_kernel<TM, TS, IMPUTE, true>, and the extended column program (column_program_kernel<T, 2>) - called directly
through their ``ops`` wrappers with the discipline of tests/test_imputer_kernels_gpu.py: past one 256-thread block, every dtype
pair, both assembly routes, operands as column slabs of sentinel-filled buffers, against the plain-torch restatements of
tests/remapper_refs.py (which tests/test_remapper_cpu.py holds to the reference's recorded outputs).

Comparison rule.  NaN sits at exactly the restatement's positions and no position is dropped.  The exactly rounded paths - none, affine,
displaced atoms and their clamp, sqrt and its inverse, the power with lambd = 0.5 and its tangent-linear branch, every clamp, relu / hardtanh,
both conditional fills - are BIT-equal to the restatement evaluated on the device in the same dtype.  For the libm methods (log1p / expm1,
general powers, boxcox, atanh, asinh) the kernel and the eager restatement on the device are each compared with a float64 evaluation of the
same formula on the same rounded inputs: per method and dtype the kernel's largest error must not exceed twice the eager route's plus one
ulp of the data dtype at the largest |result| (both routes make the same number of roundings; the factor 2 plus one ulp covers one libm
call rounding the other way and its propagation through the exactly rounded steps that follow).  Measured on the MI355X
(profiles/r16_remapper_edge_time.json, 65 536 elements per method, direction and dtype): log1p / expm1, boxcox, atanh and asinh are bit-equal
to eager torch in fp32, bf16 and fp16, the general power in fp32 - these are held to equality with eager torch on top of the bound (equality
of values: at -0.0 the kernel's asinh / sinh return -0.0, torch's fp16 kernels +0.0); the general power in a 16-bit dtype is not equal (both
routes err by the same amount against float64) and keeps the bound alone.  The fused kernels share the device function
of the stand-alone kernel: with libm methods they are held BIT-equal to the stand-alone kernel followed by the unchanged assembly kernel.
No number below comes from a kernel's output."""
import math

import pytest
import torch

from tests import imputer_refs as I
from tests import model_edge_refs as E
from tests import remapper_refs as R
from tests.model_edge_refs import BF16, F16, F32, NAME

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = 7.0
NAN = float("nan")
PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)]  # (data dtype, model dtype)
LAYOUTS = [(2, 7, 5, 21), (2, 7, 5, 24), (3, 5, 0, 16), (1, 11, 0, 16), (1, 8, 0, 8), (2, 8, 4, 24), (2, 12, 0, 24)]  # (T, V, A, W), as the imputer's
SHAPES = [(1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 1, 257), (2, 2, 333), (2, 1, 2, 257)]  # [batch, time, (ensemble,) grid]
EPS = {F32: 2.0 ** -23, BF16: 2.0 ** -7, F16: 2.0 ** -10}
ATOMS = {"lower_atom": 0.0, "upper_atom": 1.0, "lower_target": -0.25, "upper_target": 1.25, "eps": 0.0}
# (method, kwargs, how its column is drawn); a program of V columns takes the first V.  Exactly rounded: 0, 1, 3, 4, 9, 10, 11
COLUMNS = [("none", {}, "n"), ("affine", {"scale": 2.5, "shift": -0.75}, "n"), ("log1p", {}, "3r"), ("sqrt", {}, "4r"),
           ("displace_boundary_atoms", ATOMS, "atoms"), ("power", {"lambd": 0.33, "clip_negative": True, "tangent_linear_above_one": True}, "3r-"),
           ("boxcox", {"lambd": 0.25}, "r+"), ("atanh", {"rho": 2.0}, "r"), ("asinh", {"c": 3.0}, "3n"),
           ("power", {"lambd": 0.5, "clip_negative": True, "tangent_linear_above_one": True}, "3r-"), ("none", {}, "n"),
           ("affine", {"scale": 0.5, "shift": 1.25}, "n")]  # (the twelfth: the layout (2, 12, 0, 24) needs it)
LIBM = {2, 5, 6, 7, 8}
EXACT_ONLY = [0, 1, 3, 4, 9, 10, 1, 3, 4, 9, 0, 11]  # a 12-column program of exactly rounded methods only (indices into COLUMNS)


@pytest.fixture(scope="module")
def ops():
    from anemoi_core_amd import ops as _ops

    return _ops


def _entries(columns, inverse):
    from anemoi_core_amd.preprocessing.remapper import METHODS

    return [METHODS[m](inverse, **kw) for m, kw, _ in columns]


def _program(ops, columns, inverse=False):
    from anemoi_core_amd.preprocessing.remapper import device_entry

    return ops.remap_program([device_entry(e) for e in _entries(columns, inverse)], DEV)


def _draw(shape, columns, dtype, seed, inverse=False):
    """[..., V] in ``dtype``: every column inside its map's forward domain (``inverse``: 1.5 N(0, 1) + 0.5 everywhere), exact 0.0 / 1.0 in the
    atoms' column, -0.0 and one NaN in every column when there is room."""
    g = torch.Generator().manual_seed(seed)
    V = len(columns)
    x = torch.empty(*shape, V, dtype=torch.float64)
    flat = x.view(-1, V)
    for c, (_, _, how) in enumerate(columns):
        r, n = torch.rand(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
        x[..., c] = 1.5 * n + 0.5 if inverse else {"n": n, "3r": 3 * r, "4r": 4 * r, "atoms": r, "3r-": 3 * r - 0.5, "r+": 0.99 * r + 0.01, "r": r, "3n": 3 * n}[how]
        if flat.shape[0] >= 16:
            if how == "atoms":
                flat[1, c], flat[2, c], flat[9, c] = 0.0, 1.0, 0.0
            flat[(3 + 2 * c) % flat.shape[0], c] = NAN
            if how in ("n", "3n", "3r-"):
                flat[(4 + 2 * c) % flat.shape[0], c] = -0.0
    return x.to(dtype)


def _slab(t, off, pad=4):
    """(the sentinel-filled parent, the view of it that holds t)."""
    wide = torch.full((*t.shape[:-1], t.shape[-1] + pad), FILL, dtype=t.dtype, device=DEV)
    wide[..., off:off + t.shape[-1]] = t.to(DEV)
    return wide, wide[..., off:off + t.shape[-1]]


def _sentinels_intact(wide, off, V):
    return bool((wide[..., :off] == FILL).all()) and bool((wide[..., off + V:] == FILL).all())


def _restated(x_dev, columns, inverse):
    """The restatement on the device, column by column, in x's dtype (no domain assertion: a NaN or a negative is what torch computes)."""
    table = R.INVERSE if inverse else R.FORWARD
    y = x_dev.clone()
    for c, (m, kw, _) in enumerate(columns):
        extra = {"check": False} if not inverse and m in ("sqrt", "power", "boxcox") else {}
        y[..., c] = table[m](x_dev[..., c], **kw, **extra)
    return y


def _float64(x, columns, inverse, c):
    m, kw, _ = columns[c]
    extra = {"check": False} if not inverse and m in ("sqrt", "power", "boxcox") else {}
    return (R.INVERSE if inverse else R.FORWARD)[m](x[..., c].double(), **kw, **extra)


def _check(got, x, columns, inverse, what):
    """got (device) against the comparison rule of the module text; returns {column: (kernel error, eager error)} of the libm columns."""
    eager = _restated(x.to(DEV), columns, inverse).cpu()
    got = got.cpu()
    figures = {}
    for c in range(len(columns)):
        if c not in LIBM or columns[c][0] != COLUMNS[c][0]:
            E.assert_bits_equal(got[..., c], eager[..., c], f"{what}, column {c} ({columns[c][0]})")
            continue
        ref = _float64(x, columns, inverse, c)
        finite = ref.isfinite() & eager[..., c].isfinite()
        assert torch.equal(got[..., c].isnan(), eager[..., c].isnan()), f"{what}, column {c}: NaN elsewhere"
        assert torch.equal(got[..., c][~finite].nan_to_num(0.0), eager[..., c][~finite].nan_to_num(0.0)), f"{what}, column {c}: non-finite values differ"
        if not bool(finite.any()):
            continue
        ek = float((got[..., c].double() - ref)[finite].abs().max())
        ee = float((eager[..., c].double() - ref)[finite].abs().max())
        top = float(ref[finite].abs().max())
        ulp = EPS[x.dtype] * 2.0 ** math.floor(math.log2(top)) if top > 0 else 0.0
        figures[c] = (ek, ee)
        print(f"{what} column {c} {columns[c][0]} {NAME[x.dtype]}: kernel error {ek:.3e}, eager error {ee:.3e}, ulp at max {ulp:.3e}")
        assert ek <= 2.0 * ee + ulp, f"{what}, column {c} ({columns[c][0]}, {NAME[x.dtype]}): kernel error {ek:.3e} > 2 x {ee:.3e} + {ulp:.3e}"
        if not (columns[c][0] == "power" and x.dtype != F32):  # measured equal to eager torch (module text): held to it
            same = torch.equal(got[..., c].nan_to_num(0.0), eager[..., c].nan_to_num(0.0))  # (== : a zero of either sign is a zero)
            assert same, f"{what}, column {c} ({columns[c][0]}, {NAME[x.dtype]}): not equal to eager torch on the device"
    return figures


# ------------------------------------------------------------------------------------------------------------ stand-alone kernel
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("V", [5, 8, 11])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_remap_columns(ops, inverse, shape, V, dtype):
    """ops.remap_columns, every method of the first V columns in one program: out of place (x untouched), into a given out, in place; x a
    row-strided slab whose sentinels stay; ``none`` columns bit-untouched; 4-D and 5-D inputs."""
    columns = COLUMNS[:V]
    x = _draw(shape, columns, dtype, seed=sum(shape) + V, inverse=inverse)
    prog = _program(ops, columns, inverse)
    assert prog.active.tolist() == [c for c in range(V) if columns[c][0] != "none"]
    wide, xd = _slab(x, 2)
    got = ops.remap_columns(xd, prog)
    _check(got, x, columns, inverse, "out of place")
    E.assert_bits_equal(xd, x, "x untouched")
    out_wide, out = _slab(torch.zeros_like(x), 1)
    assert ops.remap_columns(xd, (_program(ops, columns), _program(ops, columns, True)), inverse=inverse, out=out) is out
    E.assert_bits_equal(out, got.cpu(), "given out == out of place")
    assert ops.remap_columns(xd, prog, out=xd) is xd
    E.assert_bits_equal(xd, got.cpu(), "in place == out of place")
    assert _sentinels_intact(wide, 2, V) and _sentinels_intact(out_wide, 1, V)
    for c in (0, 10):
        if c < V:
            E.assert_bits_equal(xd[..., c], x[..., c], f"none column {c}")


def test_program_of_nothing_launches_nothing(ops):
    x = _draw((1, 1, 33), COLUMNS[:5], F32, 1)
    prog = ops.remap_program([(0, 0, 0.0, 0.0, 0.0, 0.0)] * 5, DEV)
    xd = x.to(DEV)
    assert ops.remap_columns(xd, prog, out=xd) is xd and prog.active.numel() == 0
    E.assert_bits_equal(xd, x, "in place")
    E.assert_bits_equal(ops.remap_columns(xd, prog), x, "out of place: a copy")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_violation_counters(ops, dtype):
    """The reference's forward domain assertion as per-column counters: 0 on valid input; three negatives planted in the sqrt column count
    3 there and nowhere else (a clipped power counts nothing); a NaN counts too, as the reference's ``x.ge(0).all()`` has it."""
    columns = COLUMNS[:8]
    x = _draw((2, 2, 257), columns, dtype, 5)
    x[..., 3] = x[..., 3].nan_to_num(1.0)  # (no NaN in the sqrt column) ...
    x[..., 6] = x[..., 6].nan_to_num(0.5)  # ... nor in the boxcox column
    prog = _program(ops, columns)
    counters = torch.zeros(8, dtype=torch.int32, device=DEV)
    ops.remap_columns(x.to(DEV), prog, violations=counters)
    assert counters.tolist() == [0] * 8
    x[0, 0, 0, 3], x[1, 1, 256, 3], x[0, 1, 100, 3], x[1, 0, 7, 5] = -1.0, -0.5, -2.0, -3.0
    ops.remap_columns(x.to(DEV), prog, violations=counters)
    assert counters.tolist() == [0, 0, 0, 3, 0, 0, 0, 0]
    x[0, 0, 5, 6] = NAN
    counters.zero_()
    ops.remap_columns(x.to(DEV), prog, violations=counters)
    assert counters.tolist() == [0, 0, 0, 3, 0, 0, 1, 0]


def test_remap_columns_replays_from_a_graph(ops):
    """One hipGraph capture of the in-place launch replays bit-equal to the eager call (no host synchronisation in the wrapper)."""
    columns = COLUMNS
    x = _draw((2, 2, 257), columns, F32, 9)
    prog = _program(ops, columns)
    want = ops.remap_columns(x.to(DEV), prog)
    static = x.to(DEV)
    ops.remap_columns(static.clone(), prog)  # (the library is loaded before the capture)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        work = static.clone()
        with torch.cuda.graph(graph, stream=stream):
            out = ops.remap_columns(work, prog, out=work)
    for _ in range(2):
        work.copy_(static)
        graph.replay()
        torch.cuda.synchronize()
        E.assert_bits_equal(out, want.cpu(), "replay")


def test_error_paths(ops):
    prog = ops.remap_program([(1, 0, 0.0, 0.0, 0.0, 0.0)] * 4, DEV)
    with pytest.raises(ValueError):
        ops.remap_columns(torch.zeros(9, 4, device=DEV), prog)  # not [batch, time, grid, vars]
    with pytest.raises(ValueError):
        ops.remap_columns(torch.zeros(1, 1, 9, 5, device=DEV), prog)  # the program has 4 columns
    with pytest.raises(ValueError):
        ops.remap_columns(torch.zeros(1, 1, 9, 4, device=DEV), prog, violations=torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.remap_program([(17, 0, 0.0, 0.0, 0.0, 0.0)], DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.remap_columns(torch.zeros(1, 1, 9, 4), prog)
    with pytest.raises(ValueError):
        ops.assemble_input(torch.zeros(1, 9, 5, device=DEV), None, 5, remap=prog)


# ------------------------------------------------------------------------------------------------------------ the modules on the device
def test_modules_on_device_equal_the_reference(golden):
    """Remapper and the post-processors on CUDA tensors against the reference's recorded CPU outputs (fp32), every width, with and without
    an ensemble dimension, in place and out of place.  The post-processors are exact: bit-equal.  The remapper's libm methods meet the
    recorded values within 32 fp32 ulp (rtol 2^-18, atol 1e-6): two libms of a few ulp each, amplified at most 4x by the power 1 / lambd."""
    from tests.remapper_helpers import KEYS, POST_CONFIGS, REMAP_CONFIGS, post, remapper

    fx = golden("remapper.pt")
    for config in REMAP_CONFIGS:
        rm = remapper(fx, config)
        for key in KEYS:
            want = fx["remapper"][config][key]
            for direction, src in (("transform", fx["inputs"][key]), ("inverse", fx["outputs"][key])):
                fn = rm.transform if direction == "transform" else rm.inverse_transform
                x = src.to(DEV)
                got = fn(x, in_place=False)
                E.assert_bits_equal(x, src, "x untouched")
                assert torch.equal(got.isnan().cpu(), want[direction].isnan()), f"{config} {key} {direction}: NaN elsewhere"
                torch.testing.assert_close(got.cpu(), want[direction], rtol=2.0 ** -18, atol=1e-6, equal_nan=True, msg=f"{config} {key} {direction}")
                assert fn(x) is x
                E.assert_bits_equal(x, got.cpu(), "in place == out of place")
    for name in POST_CONFIGS:
        pp = post(fx, name)
        for key in KEYS:
            y = fx["outputs"][key].to(DEV)
            E.assert_bits_equal(pp.inverse_transform(y, in_place=False), fx["post"][name][key]["inverse"], f"{name} {key}")
            E.assert_bits_equal(y, fx["outputs"][key], "y untouched")
            assert pp.inverse_transform(y) is y and pp.transform(y) is y
            E.assert_bits_equal(y, fx["post"][name][key]["inverse"], f"{name} {key} in place")


def test_module_raises_the_reference_assertion_on_the_device(golden):
    from tests.remapper_helpers import remapper

    fx = golden("remapper.pt")
    x = fx["inputs"]["training"].clone()
    x[0, 1, 2, fx["indices"]["data_input_name_to_index"]["h"]] = -0.5
    rm = remapper(fx, {"default": "none", "sqrt": ["h"]})
    with pytest.raises(AssertionError) as e:
        rm.transform(x.to(DEV), in_place=False)
    assert f"AssertionError: {e.value}" == fx["errors"]["sqrt_negative"]
    rm.check_domain = False  # what a captured forward runs: no read-back, the negative is a NaN
    got = rm.transform(x.to(DEV), in_place=False)
    assert bool(got[0, 1, 2, fx["indices"]["data_input_name_to_index"]["h"]].isnan())


# ------------------------------------------------------------------------------------------------------------ fused assembly
def _impute_program(V, dtype):
    kinds, values, sources = [0] * V, [0.0] * V, [0] * V
    for c in (1, V - 2):
        kinds[c], values[c] = 1, float(torch.tensor(0.625 + c).to(dtype))
    return kinds, values, sources


def _route(W, to):
    return "vec8" if to != F32 and W % 8 == 0 else "scalar"


def test_layouts_reach_both_routes():
    routes = {(lay, _route(lay[3], to)) for lay in LAYOUTS for _, to in PAIRS}
    assert {r for _, r in routes} == {"scalar", "vec8"}


@pytest.mark.parametrize("impute", [True, False], ids=["imputer", "noimputer"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{NAME[p[0]]}-{NAME[p[1]]}")
@pytest.mark.parametrize("N", [1, 257, 333])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda s: "T%d-V%d-A%d-W%d" % s)
def test_assemble_input_remap(ops, layout, N, pair, impute):
    """ops.assemble_input(remap=[, impute=, nan_mask=]): impute -> remap forward -> normalise, then the assembly.  Exactly rounded methods:
    bit-equal to impute_ref -> the restatement on the device -> assemble_input_ref; the mask is isnan of the raw step 0.  All methods: bit-equal
    to the stand-alone kernels followed by the unchanged assembly kernel."""
    (T, V, A, W), (ti, to) = layout, pair
    mul, add = (0.5 + torch.rand(V, generator=torch.Generator().manual_seed(V))), torch.randn(V, generator=torch.Generator().manual_seed(V + 1))
    attrs = torch.randn(N, A, generator=torch.Generator().manual_seed(50 + N)).to(to) if A else None
    program = _impute_program(V, ti)
    for label, columns in (("exact", [COLUMNS[i] for i in EXACT_ONLY[:V]]), ("all", COLUMNS[:V])):
        x = _draw((T, N), columns, ti, seed=N + W)
        remap = _program(ops, columns)
        mask = torch.zeros(N, V, dtype=torch.bool, device=DEV) if impute else None
        _, xs = _slab(x, 2)
        ad = None if attrs is None else _slab(attrs, 1)[1]
        got = ops.assemble_input(xs, ad, W, mul.to(DEV), add.to(DEV), out_dtype=to, impute=ops.impute_program(*program, DEV) if impute else None,
                                 nan_mask=mask, remap=remap)
        filled = I.impute_ref(x.unsqueeze(0), program)[0][0] if impute else x
        if impute:
            assert torch.equal(mask.cpu(), x[0].isnan())
        if label == "exact":
            mapped = _restated(filled.to(DEV), columns, False).cpu()
            E.assert_bits_equal(got, E.assemble_input_ref(mapped, attrs, W, mul, add, to), f"{_route(W, to)} N={N} exact methods")
        alone = ops.remap_columns(filled.to(DEV).unsqueeze(0), remap)[0]
        E.assert_bits_equal(got, ops.assemble_input(alone, None if attrs is None else attrs.to(DEV), W, mul.to(DEV), add.to(DEV), out_dtype=to).cpu(),
                            f"{_route(W, to)} N={N} {label}: fused == stand-alone")
        none = ops.assemble_input(xs, ad, W, None, None, out_dtype=to, remap=remap)  # without a normaliser
        E.assert_bits_equal(none, ops.assemble_input(ops.remap_columns(x.to(DEV).unsqueeze(0), remap)[0], None if attrs is None else attrs.to(DEV), W,
                                                     out_dtype=to).cpu(), f"{label}: no normaliser")


@pytest.mark.parametrize("impute", [True, False], ids=["imputer", "noimputer"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{NAME[p[0]]}-{NAME[p[1]]}")
@pytest.mark.parametrize("V_out", [5, 37])
def test_assemble_output_remap(ops, V_out, pair, impute):
    """ops.assemble_output(remap=[, impute=]) on the raw skip: the same chain before the residual add; N in {1, 257, 333}, the skip
    contiguous and a slab; the column map names remapped, imputed and plain skip columns."""
    ts, tm = pair
    V_in = 11
    mul, add = (0.5 + torch.rand(V_in, generator=torch.Generator().manual_seed(3))), torch.randn(V_in, generator=torch.Generator().manual_seed(4))
    program = _impute_program(V_in, ts)
    col_map = torch.full((V_out,), -1, dtype=torch.int32)
    col_map[:5] = torch.tensor([1, 3, 9, 4, 0], dtype=torch.int32)
    for label, columns in (("exact", [COLUMNS[i] for i in EXACT_ONLY[:V_in]]), ("all", COLUMNS[:V_in])):
        if label == "all":
            col_map[:5] = torch.tensor([2, 5, 9, 7, 8], dtype=torch.int32)
        remap = _program(ops, columns)
        for N in (1, 257, 333):
            skip = _draw((N,), columns, ts, seed=N)
            x_out = torch.randn(N, V_out, generator=torch.Generator().manual_seed(N + V_out)).to(tm)
            filled = I.impute_ref(skip[None, None], program)[0][0, 0] if impute else skip
            imp = ops.impute_program(*program, DEV) if impute else None
            for lay, sd in (("contiguous", skip.to(DEV)), ("slab", _slab(skip, 3, pad=5)[1])):
                got = ops.assemble_output(x_out.to(DEV), sd, col_map.to(DEV), mul.to(DEV), add.to(DEV), impute=imp, remap=remap)
                if label == "exact":
                    mapped = _restated(filled.to(DEV), columns, False).cpu()
                    E.assert_bits_equal(got, E.assemble_output_ref(x_out, mapped, col_map, mul, add), f"N={N} {lay} exact methods")
                alone = ops.remap_columns(filled.to(DEV)[None, None], remap)[0, 0]
                E.assert_bits_equal(got, ops.assemble_output(x_out.to(DEV), alone, col_map.to(DEV), mul.to(DEV), add.to(DEV)).cpu(),
                                    f"N={N} {lay} {label}: fused == stand-alone")


# ------------------------------------------------------------------------------------------------------------ output column program
def _ext(prog, V):
    from anemoi_core_amd.layers.bounding import extended_program_tables

    return extended_program_tables(prog, V, DEV)


def _evaluate(x_dev, prog, mask=None):
    from anemoi_core_amd.layers.bounding import apply_program_torch

    return apply_program_torch(x_dev, prog, mask=mask)


def _remap_op(method, kw, col):
    from anemoi_core_amd.preprocessing.remapper import METHODS

    e = METHODS[method](True, **kw)
    return (16 + e[0], col, 0, e[2], e[3], e[1], e[4])


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 333])
def test_new_kinds_alone_are_exact(ops, N, dtype):
    """Kinds 11 / 12 and the exactly rounded inverses (affine, the atoms' clamp, sqrt's and the lambd = 0.5 power's inverse with the tangent
    branch, atanh's clamp at rho = 0): bit-equal to the same program evaluated with torch ops on the device.  The conditional fill of the
    masking column itself comes last in its group, so the other fills see the zeros / NaN the reference's one mask sees; NaN in a masking
    column is no zero."""
    V = 9
    x = (1.5 * torch.randn(1, 1, N, V, generator=torch.Generator().manual_seed(N)) + 0.5).to(dtype)
    flat = x.view(-1, V)
    if N > 8:
        flat[0, 4], flat[3, 4], flat[N - 1, 4], flat[5, 4], flat[6, 4] = 0.0, 0.0, 0.0, NAN, -0.0
        flat[2, 7], flat[N - 2, 7], flat[4, 0] = NAN, NAN, NAN
    prog = [_remap_op("affine", {"scale": 2.5, "shift": -0.75}, 0), _remap_op("displace_boundary_atoms", ATOMS, 1), _remap_op("sqrt", {}, 2),
            _remap_op("power", {"lambd": 0.5, "clip_negative": True, "tangent_linear_above_one": True}, 3), _remap_op("atanh", {"rho": 0.0}, 5),
            (11, 0, 4, 3.0, 0.0), (11, 6, 4, -1.5, 0.0), (11, 4, 4, 5.0, 0.0),  # fills where column 4 is zero; column 4 itself last
            (12, 8, 7, 0.0, 0.0), (12, 7, 7, 0.0, 0.0), (12, 1, 7, 0.0, 0.0)]
    want = _evaluate(x.to(DEV), prog)
    xd = x.to(DEV)
    assert ops.column_program_(xd, *_ext(prog, V)) is xd
    E.assert_bits_equal(xd, want.cpu(), "new kinds")
    if N > 8:
        got = xd.cpu().view(-1, V)
        assert got[0, 0] == 3.0 and got[0, 6] == -1.5 and got[0, 4] == 5.0 and got[6, 4] == 5.0 and bool(got[5, 4].isnan()) and got[5, 6] == flat[5, 6]
        assert bool(got[2, 8].isnan()) and bool(got[2, 1].isnan()) and not bool(got[3, 8].isnan())


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("N", [1, 257, 333])
def test_new_kinds_interleaved_with_the_old(ops, N, dtype):
    """A predict_step program: boundings (relu, hardtanh), a thresholded relu, kind 9 on every column, the remapper's inverse, kind 10, then
    conditional fills - one launch.  The kinds used here are exactly rounded in the kernel, so the result is bit-equal to the torch
    evaluation on the device; the kinds 1..10 alone make the same bits through ``bound_columns_`` and through ``column_program_``."""
    V, VM = 8, 5
    g = torch.Generator().manual_seed(N)
    x = (1.5 * torch.randn(1, 1, 1, N, V, generator=g)).to(dtype)
    if N > 1:
        x[0, 0, 0, N // 2, 0], x[0, 0, 0, N - 1, 3] = NAN, float("inf")
    mul = [float(torch.tensor(v).to(torch.float32)) for v in (0.5, 2.0, 0.25, 4.0, 1.5, 0.75, 3.0, 1.25)]
    add = [float(torch.tensor(v).to(torch.float32)) for v in (0.25, -1.0, 0.5, 0.0, -0.75, 2.0, 1.0, -0.5)]
    old = [(1, 0, 0, 0.0, 0.0), (5, 4, 0, -0.5, 0.75), (5, 1, 0, 0.0, 1.0)] + [(9, c, 0, add[c], mul[c]) for c in range(V)]
    new = [_remap_op("sqrt", {}, 0), _remap_op("affine", {"scale": 0.5, "shift": 0.25}, 2),
           _remap_op("power", {"lambd": 0.5, "clip_negative": True, "tangent_linear_above_one": True}, 3), (10, 5, 1, 0.0, 0.0), (10, 0, 4, 0.0, 0.0),
           (11, 6, 3, 2.5, 0.0), (11, 3, 3, -1.0, 0.0), (12, 7, 5, 0.0, 0.0), (1, 2, 0, 0.0, 0.0)]
    mask = torch.rand(N, VM, generator=g) < 0.3
    want = _evaluate(x.to(DEV), old + new, mask=mask.to(DEV).reshape(1, 1, 1, N, VM))
    xd = x.to(DEV)
    ops.column_program_(xd, *_ext(old + new, V), nan_mask=mask.to(DEV))
    E.assert_bits_equal(xd, want.cpu(), "interleaved")
    assert N < 8 or bool((xd[..., 3] == -1.0).any())  # the power's inverse clamps to exact zeros, which the fills then see
    # every old kind: the same bits from the kernel as it was and from its extension
    every = [(1, 0, 0, 0.0, 0.0), (2, 1, 0, 0.0, 0.0), (3, 2, 0, 0.3, 0.0), (4, 3, 0, -0.2, 0.0), (5, 4, 0, -0.5, 0.75), (6, 5, 0, 0.0, 1.0),
             (7, 6, 0, 0.0, 1.0), (8, 7, 1, 0.0, 1.0)] + [(9, c, 0, add[c], mul[c]) for c in range(V)]
    from anemoi_core_amd.layers.bounding import masked_program_tables, program_tables

    a, b = x.to(DEV), x.to(DEV)
    ops.bound_columns_(a, *program_tables(every, DEV))
    ops.column_program_(b, *_ext(every, V))
    E.assert_bits_equal(b, a.cpu(), "kinds 1..9: column_program_ == bound_columns_")
    with_nan = every + [(10, 2, 0, 0.0, 0.0)]
    t = masked_program_tables(with_nan, DEV)
    a, b = x.to(DEV), x.to(DEV)
    ops.bound_columns_(a, t.ops, t.params, nan_mask=mask.to(DEV), n_nan_ops=t.n_nan_ops)
    ops.column_program_(b, *_ext(with_nan, V), nan_mask=mask.to(DEV))
    E.assert_bits_equal(b, a.cpu(), "kinds 1..10: column_program_ == bound_columns_")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_inverse_ops_of_the_program_equal_the_stand_alone_kernel(ops, dtype):
    """Every method's inverse as ops 16 + r of the column program: the same bits as ops.remap_columns(inverse) (one device function)."""
    N, V = 333, len(COLUMNS)
    x = _draw((1, 1, N), COLUMNS, dtype, seed=3, inverse=True)
    prog = [_remap_op(m, kw, c) for c, (m, kw, _) in enumerate(COLUMNS) if m != "none"]
    xd = x.to(DEV)
    ops.column_program_(xd, *_ext(prog, V))
    E.assert_bits_equal(xd, ops.remap_columns(x.to(DEV), _program(ops, COLUMNS, True)).cpu(), "program == stand-alone")
