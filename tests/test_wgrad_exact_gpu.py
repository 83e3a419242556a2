"""The transpose-read weight gradient (csrc/wgrad.hip: dW = dZ^T X and db = column sums of dZ for every 16-bit Linear in
training) called through ``ops.linear_wgrad``, through the C ABI with buffers of the test's own, and through the autograd of
``ops.linear``, held to the EXACT bits of a float64 reference evaluated on the CPU.

Why exact: the operands are integers in [-2, 2] (tests/wgrad_cases.py).  Every product is exact in bf16 / fp16 and every fp32
partial sum is an integer below 2^24, exact in any order, any split over workgroups and any MFMA grouping; the reduce kernel
rounds that integer once, to nearest even like torch, so ``torch.equal(got, want.to(dtype))`` must hold for every element.
Losing, doubling or misplacing one row changes thousands of elements after rounding (tests/test_wgrad_cases_cpu.py proves that
for the first and last row of every split and every row of the last 64-row step of every case, in both dtypes, and asserts the
preconditions of exactness per case), as does a neighbouring column read in place of the zero line.

NO TEST HERE ASSERTS A PLAN-DEPENDENT FACT: the expected bits do not depend on how the reduction is split.  That lets
``test_developer_switches`` run this whole file again in child processes under ANEMOI_WGRAD_RING=1 (4 stages of 32 rows: other
step counts and wait counts) and ANEMOI_WGRAD_WGS=3 (three splits on one tile, a single long split elsewhere).  Which branches of
the default plan the case lists reach is asserted without a GPU in tests/test_wgrad_cases_cpu.py.

Families:

* row ladder, width ladder, product-like plan: EXACT, dW and db, both dtypes; dW without the bias gradient and a repeated call
  give the same bits.
* poisoned surroundings: the operands are views buf[1:1+n, 8:8+W] of a NaN-filled [n + 2, W + 16] buffer; EXACT.  A fetch of the
  row before the first, a row past n_rows or a column outside the slab - where the zero line belongs - returns NaN.
* guards: the C entry point writes dW into rows 1..O of a [O + 2, I + 4] tensor, db into [8:8+O] of a longer vector and its
  partial tiles into a workspace of exactly the queried size (NaN-filled, 64 floats spare behind it): EXACT results, every guard
  element unchanged, no NaN out (every partial element the reduce kernel reads was written).
* autograd of ``ops.linear``: weight.grad / bias.grad EXACT for x contiguous, [3, 427, K], one element into a buffer, and with a
  row stride of K + 4 (``_granule_rows`` copies the last two).
  Outside autograd a [3, 427, K] input (with a residual of the same leading dimensions) gives the bits of the 2-D call.
* refusals: ValueError before anything is launched.
* real-valued data, per element against float64 with a bound that is derived, not measured:
  |err| <= u |want| + (n_rows + 8) 2^-23 (|dZ|^T |X|), u = 2^-8 (bf16) / 2^-11 (fp16): one final rounding plus the classical bound
  of an fp32 accumulation of exact products over n_rows terms and at most 8 partial tiles, with 2^-23 in place of 2^-24 because
  the MFMA's internal rounding is not documented.  The worst err / bound is printed per case; see MEASURED below.

What these tests found, and the fixes (the kernel itself met every check as it stood: csrc/wgrad.hip is unchanged):

* ``autograd._granule_rows`` copied with ``t.contiguous()``.  A dense [n, K] view that starts one element into its buffer is
  contiguous already, so it came back as it was and the backward of ``ops.linear`` ended in "linear_wgrad: operands must be
  16-byte aligned" (``test_through_autograd[*-offset-1]``).  It now clones into a fresh allocation; what the kernel takes in place
  still passes through untouched (tests/test_wgrad_cases_cpu.py holds both halves without a GPU).
* ``ops.linear`` refused an input with leading dimensions ([3, 427, K]: "x and weight must be 2-D") although
  ``LinearFunction.backward`` provides for one (``x.reshape(-1, K)``).  ``ops.linear`` now treats leading dimensions as rows, like
  torch.nn.Linear: it flattens x (and a residual) and gives y the leading dimensions back; 2-D calls are untouched.

MEASURED on an MI355X, default plan, worst |err| / bound over all elements of the real-valued cases (an fp32 matmul of the same
operands on the CPU gives the same figures to three digits - the final rounding dominates):

    (n, O, I)            dtype   dW      db
    (1281, 264, 136)     bf16    0.664   0.546
    (1281, 264, 136)     fp16    0.281   0.153
    (2100, 1024, 1024)   bf16    0.606   0.524
    (2100, 1024, 1024)   fp16    0.161   0.082

Run time of the file on an MI355X: 15 s for its 253 tests, of which 6 to 7 s for each of the two child runs (mostly start-up);
no other test takes more than 0.7 s.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import wgrad_cases as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
NAME = {BF16: "bf16", F16: "fp16"}
UNIT_ROUNDOFF = {BF16: 2.0 ** -8, F16: 2.0 ** -11}


@pytest.fixture(scope="module")
def ops():
    from anemoi_core_amd import ops as _ops

    return _ops


def _params(cases):
    return [pytest.param(c, dtype, id=f"{C.case_id(c)}-{NAME[dtype]}") for dtype in DTYPES for c in cases]


def _device_operands(case, dtype):
    dz, x = C.operands(*case)
    return dz.to(dtype).to(DEV), x.to(dtype).to(DEV)


def _expected(case, dtype):
    dw, db = C.reference(*case)
    return dw.to(dtype), db.to(dtype)


def _assert_bits(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        rows = sorted(set(bad[:, 0].tolist()))
        cols = sorted(set(bad[:, -1].tolist())) if bad.shape[1] > 1 else []
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} elements differ; rows {rows[:8]}..{rows[-1:]}, "
                             f"columns {cols[:8]}..{cols[-1:]}; first got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}")


def _check_exact(ops, case, dtype):
    dz, x = _device_operands(case, dtype)
    want_dw, want_db = _expected(case, dtype)
    dw, db = ops.linear_wgrad(dz, x, with_bias_grad=True)
    _assert_bits(dw, want_dw, "dW")
    _assert_bits(db, want_db, "db")
    _assert_bits(ops.linear_wgrad(dz, x), want_dw, "dW without the bias gradient")
    dw2, db2 = ops.linear_wgrad(dz, x, with_bias_grad=True)
    _assert_bits(dw2, want_dw, "dW of the repeated call")
    _assert_bits(db2, want_db, "db of the repeated call")


@pytest.mark.parametrize("case,dtype", _params(C.ROW_LADDER))
def test_row_ladder(ops, case, dtype):
    _check_exact(ops, case, dtype)


@pytest.mark.parametrize("case,dtype", _params(C.WIDTH_LADDER))
def test_width_ladder(ops, case, dtype):
    _check_exact(ops, case, dtype)


@pytest.mark.parametrize("case,dtype", _params(C.PRODUCT_LIKE))
def test_product_like_plan(ops, case, dtype):
    # The float64 product of these two may be formed with torch on the device - it is exact either way; it is formed on the CPU
    # like every other reference here (tests/wgrad_cases.reference, once per process), which keeps one reference for all cases.
    _check_exact(ops, case, dtype)


def _poisoned_view(t, dtype):
    """t [n, W] as buf[1:1+n, 8:8+W] of a [n + 2, W + 16] buffer whose other elements are NaN: 16-byte aligned, row stride % 8 == 0."""
    n, w = t.shape
    buf = torch.full((n + 2, w + 16), float("nan"), dtype=dtype, device=DEV)
    view = buf[1:1 + n, 8:8 + w]
    view.copy_(t.to(dtype))
    assert view.data_ptr() % 16 == 0 and (n == 1 or view.stride(0) % 8 == 0) and view.stride(1) == 1
    return view


@pytest.mark.parametrize("case,dtype", _params(C.POISONED))
def test_poisoned_surroundings(ops, case, dtype):
    dz_i, x_i = C.operands(*case)
    dz, x = _poisoned_view(dz_i, dtype), _poisoned_view(x_i, dtype)
    want_dw, want_db = _expected(case, dtype)
    dw, db = ops.linear_wgrad(dz, x, with_bias_grad=True)
    _assert_bits(dw, want_dw, "dW from views in NaN")
    _assert_bits(db, want_db, "db from views in NaN")
    dw_c, db_c = ops.linear_wgrad(dz.contiguous(), x.contiguous(), with_bias_grad=True)
    assert torch.equal(dw, dw_c) and torch.equal(db, db_c)
    # one operand in NaN, the other contiguous: a stray fetch on either side alone
    _assert_bits(ops.linear_wgrad(dz, x.contiguous()), want_dw, "dW, dz a view in NaN")
    _assert_bits(ops.linear_wgrad(dz.contiguous(), x), want_dw, "dW, x a view in NaN")


GUARD = 7.5


def _abi_wgrad(ops, dz, x, with_db):
    """anemoi_linear_wgrad (include/anemoi_hip.h: dz, lddz, x, ldx, dw, lddw, db, workspace, n_rows, O, I, dtype, stream) on
    guarded buffers.  Returns the buffers; every tensor stays referenced by the caller until after its synchronize."""
    from anemoi_core_amd import _lib

    lib = _lib.load()
    n, O = dz.shape
    I = x.shape[1]
    assert x.shape[0] == n and dz.is_contiguous() and x.is_contiguous()
    dw_buf = torch.full((O + 2, I + 4), GUARD, dtype=dz.dtype, device=DEV)
    db_buf = torch.full((O + 16,), GUARD, dtype=dz.dtype, device=DEV)
    ws_bytes = int(lib.anemoi_linear_wgrad_workspace_bytes(n, O, I))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws_buf = torch.full((4 + ws_bytes // 4 + 64,), GUARD, dtype=torch.float32, device=DEV)
    ws_buf[4:4 + ws_bytes // 4] = float("nan")
    dw_ptr = dw_buf.data_ptr() + (I + 4) * dw_buf.element_size()
    db_ptr = db_buf.data_ptr() + 8 * db_buf.element_size()
    ws_ptr = ws_buf.data_ptr() + 16
    assert dw_buf[1:1 + O].data_ptr() == dw_ptr and db_buf[8:8 + O].data_ptr() == db_ptr and ws_buf[4:].data_ptr() == ws_ptr
    assert dz.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and dw_ptr % 8 == 0 and ws_ptr % 16 == 0
    torch.cuda.synchronize()
    rc = lib.anemoi_linear_wgrad(ctypes.c_void_p(dz.data_ptr()), O, ctypes.c_void_p(x.data_ptr()), I, ctypes.c_void_p(dw_ptr), I + 4,
                                 ctypes.c_void_p(db_ptr) if with_db else None, ctypes.c_void_p(ws_ptr), n, O, I, ops._dt(dz),
                                 ctypes.c_void_p(ops._stream()))
    torch.cuda.synchronize()
    _lib.check(rc, "linear_wgrad")
    return dw_buf, db_buf, ws_buf, ws_bytes // 4


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("case,dtype", _params(C.GUARDED))
def test_guards_through_the_c_abi(ops, case, dtype, with_db):
    dz, x = _device_operands(case, dtype)
    n, O, I = case
    ref_dw, ref_db = ops.linear_wgrad(dz, x, with_bias_grad=True)
    dw_buf, db_buf, ws_buf, ws_len = _abi_wgrad(ops, dz, x, with_db)
    dw_buf, db_buf, ws_buf = dw_buf.cpu(), db_buf.cpu(), ws_buf.cpu()
    want_dw, want_db = _expected(case, dtype)
    _assert_bits(dw_buf[1:1 + O, :I].contiguous(), want_dw, "dW through the C ABI")
    assert torch.equal(dw_buf[1:1 + O, :I], ref_dw.cpu())
    assert not bool(torch.isnan(dw_buf).any()) and not bool(torch.isnan(db_buf).any())
    guards = [dw_buf[0], dw_buf[O + 1], dw_buf[:, I:], db_buf[:8], db_buf[8 + O:], ws_buf[:4], ws_buf[4 + ws_len:]]
    if with_db:
        _assert_bits(db_buf[8:8 + O].contiguous(), want_db, "db through the C ABI")
        assert torch.equal(db_buf[8:8 + O], ref_db.cpu())
    else:
        guards.append(db_buf)
    for i, gd in enumerate(guards):
        assert bool((gd == GUARD).all()), f"guard region {i} was written"


def _autograd_x(layout, x):
    """x [n, K] (device, contiguous) in the memory layout under test."""
    n, K = x.shape
    if layout == "contiguous":
        return x
    if layout == "leading-dims":
        assert n % 3 == 0
        return x.view(3, n // 3, K)
    if layout == "offset-1":
        buf = torch.full((n * K + 1,), float("nan"), dtype=x.dtype, device=DEV)
        buf[1:] = x.reshape(-1)
        view = buf[1:].view(n, K)
        assert view.data_ptr() % 16 != 0
        return view
    assert layout == "row-stride-K+4"
    buf = torch.full((n, K + 4), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, :K] = x
    view = buf[:, :K]
    assert view.stride(0) % 8 != 0
    return view


@pytest.mark.parametrize("layout", ["contiguous", "leading-dims", "offset-1", "row-stride-K+4"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[NAME[d] for d in DTYPES])
def test_through_autograd(ops, dtype, layout):
    """No activation, so dz is d_out; weight.grad = d_out^T x and bias.grad = column sums of d_out, exactly."""
    n, O, K = C.AUTOGRAD
    d_out, x = _device_operands(C.AUTOGRAD, dtype)
    gen = torch.Generator().manual_seed(11)
    weight = C.ints(gen, (O, K)).to(dtype).to(DEV).requires_grad_(True)
    bias = C.ints(gen, (O,)).to(dtype).to(DEV).requires_grad_(True)
    xin = _autograd_x(layout, x)
    y = ops.linear(xin, weight, bias)
    assert y.shape == xin.shape[:-1] + (O,)
    y.backward(d_out.view(y.shape))
    want_dw, want_db = _expected(C.AUTOGRAD, dtype)
    _assert_bits(weight.grad, want_dw, "weight.grad")
    _assert_bits(bias.grad, want_db, "bias.grad")
    # the forward of the same call: an exact integer in fp32, rounded once
    want_y = (x.cpu().double() @ weight.detach().cpu().double().t() + bias.detach().cpu().double()).to(dtype)
    _assert_bits(y.detach().reshape(n, O), want_y, "y")


@pytest.mark.parametrize("dtype", DTYPES, ids=[NAME[d] for d in DTYPES])
def test_linear_leading_dimensions_without_autograd(ops, dtype):
    """The same flattening outside autograd: y of a [3, 427, K] input (with a [3, 427, O] residual) has the bits of the 2-D call."""
    n, O, K = C.AUTOGRAD
    res, x = _device_operands(C.AUTOGRAD, dtype)
    gen = torch.Generator().manual_seed(11)
    weight, bias = C.ints(gen, (O, K)).to(dtype).to(DEV), C.ints(gen, (O,)).to(dtype).to(DEV)
    y2 = ops.linear(x, weight, bias, residual=res)
    y3 = ops.linear(x.view(3, n // 3, K), weight, bias, residual=res.view(3, n // 3, O))
    assert y3.shape == (3, n // 3, O) and torch.equal(y3.view(n, O), y2)
    with pytest.raises(ValueError):
        ops.linear(x.view(3, n // 3, K), weight, bias, out=torch.empty((n, O), dtype=dtype, device=DEV))


def test_refusals(ops):
    """Shapes and types the kernel does not take are ValueErrors of the wrapper: nothing is launched."""
    def t(n, w, dtype=BF16):
        return torch.ones((n, w), dtype=dtype, device=DEV)

    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 16, torch.float32), t(64, 16, torch.float32))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 16, BF16), t(64, 16, F16))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 12), t(64, 16))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 16), t(64, 12))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 16), t(65, 16))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(0, 16), t(0, 16))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 20)[:, :16], t(64, 16))
    with pytest.raises(ValueError):
        ops.linear_wgrad(t(64, 16), t(64, 20)[:, :16])
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,dtype", _params(C.REAL_VALUED))
def test_real_valued_data_within_the_fp32_accumulation_bound(ops, case, dtype):
    n, O, I = case
    gen = torch.Generator().manual_seed(7 * n + O + I)
    dz = (0.5 * torch.randn((n, O), generator=gen)).to(dtype)
    x = torch.randn((n, I), generator=gen).to(dtype)
    dz64, x64 = dz.double(), x.double()
    want, want_b = dz64.t() @ x64, dz64.sum(0)
    mag, mag_b = dz64.abs().t() @ x64.abs(), dz64.abs().sum(0)
    dw, db = ops.linear_wgrad(dz.to(DEV), x.to(DEV), with_bias_grad=True)
    u, acc = UNIT_ROUNDOFF[dtype], (n + C.SPLITS_MAX) * 2.0 ** -23
    ratio = float(((dw.cpu().double() - want).abs() / (u * want.abs() + acc * mag)).max())
    ratio_b = float(((db.cpu().double() - want_b).abs() / (u * want_b.abs() + acc * mag_b)).max())
    print(f"\nwgrad real-valued {C.case_id(case)} {NAME[dtype]}: worst err / bound dW {ratio:.3f}, db {ratio_b:.3f}")
    assert ratio <= 1.0 and ratio_b <= 1.0, (ratio, ratio_b)


@pytest.mark.parametrize("env", [{"ANEMOI_WGRAD_RING": "1"}, {"ANEMOI_WGRAD_WGS": "3"}], ids=["ring-4x32", "three-workgroups"])
def test_developer_switches(env):
    """The two developer switches are compiled and shipped but read once per process: this file again, in a child, under each."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "not test_developer_switches",
                        "-p", "no:cacheprovider"], cwd=REPO, env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
