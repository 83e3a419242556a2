"""The training row-wise kernels (csrc/rowwise_bwd.hip: scope row f1) and two neighbours (``transpose_pad`` and the split-K
GEMM behind ``autograd._weight_grad``) called directly through their ``ops`` wrappers - not through autograd - against a plain
int64 / float64 restatement evaluated on the CPU on the inputs *after* they were rounded to the test dtype.

Which checks are exact and which carry a tolerance, per family:

* ``colsum``; ``d_beta`` of ``layer_norm_backward``; ``segment_sum_rows``; ``linear_splitk`` and ``_weight_grad``: EXACT.  The
  operands are small integers, so every fp32 partial sum is an integer below 2^24 (exact in any summation order) and every
  result is representable in the output dtype (|integer| <= 2^8 bf16, 2^11 fp16).  The tests assert that range on the
  expected values and on the sums of absolute values, then require ``torch.equal``: one dropped, duplicated or misplaced
  row fails them.
* ``gather_add_rows``: EXACT on real-valued data (one fp32 add, one rounding).  ``transpose_pad``: EXACT (data movement).
  ReGLU's gate gradient at gate = 0 and the GELU derivative's saturated tails (x = +-30: ``d_y`` and 0): EXACT.
* run-to-run determinism of ``colsum``, ``layer_norm_backward``, ``segment_sum_rows``: EXACT (``torch.equal``).
* ``dx`` of ``layer_norm_backward``; ``y``, ``dx``, ``d_scale`` of the conditional LayerNorm; ``gelu`` / ``gelu_backward``;
  ``glu`` / ``glu_backward``: ``tests.test_kernels_gpu.assert_close`` in the tensor's dtype (fp32: atol 1e-4 + rtol 1e-5;
  16 bit: 2e-2 max|want| + 2e-2 |want|) against float64.
* ``dgamma`` / ``dbeta`` of ``layer_norm_backward`` on real-valued data come back in fp32 for every dtype and are held to
  fp32 accuracy: per case the test runs torch's own fp32 CPU autograd of ``F.layer_norm`` on the same rounded inputs, takes
  its maximum error against the float64 result relative to max|want|, and requires the kernel's error to stay within 8x that
  (a different but equally valid summation order: per-wave sequential, 8 waves, a tree over up to 512 partial rows; and
  ``rsqrtf`` against 1/sqrt), with a floor of 2e-5 max|want| (the fp32 bound tests/test_training_gpu.py applies to this op).
  One dropped row out of 40 320 moves a ``dgamma`` column by about 1e-3 of max|want|.  Both errors are printed per case.
  Worst measured on an MI355X: kernel error at most 1.47x torch's fp32 error and at most 0.015 of the bound (figures below).

No test skips or masks elements: every element of every output is compared.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import DEV, assert_close

pytestmark = pytest.mark.gpu

# dgamma / dbeta of the LayerNorm-backward float64 tests, worst over their 68 cases x 2 outputs on an MI355X (errors relative
# to max|want|): kernel 2.9e-7 (dgamma, 4 097 x 512 fp32 at |mean| / sigma up to 16) where torch's fp32 CPU autograd has 5.4e-7;
# torch's own worst is 6.6e-7 (dbeta, 40 320 x 1024 fp32: kernel 1.4e-7).  Worst kernel / torch-fp32 ratio 1.47 (dgamma of the
# one-row case: 6.2e-8 against 4.2e-8), against the 8x allowed; the 2e-5 floor governs every case, and the worst kernel error
# is 0.015 of it.

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
EXACT_INT = {F32: 2 ** 24, BF16: 2 ** 8, F16: 2 ** 11}  # integers up to this magnitude are exact in the dtype
SLAB_PAD = 16  # a slab is wide[:, off:off + D] of a [N, D + SLAB_PAD] buffer


@pytest.fixture(scope="module")
def ops():
    from anemoi_core_amd import ops as _ops

    return _ops


def _slab(t, off, fill=3.0):
    """The CPU tensor t [N, D] on the device: contiguous (off None) or as the column slab wide[:, off:off + D] of a wider buffer
    whose other columns hold ``fill`` (a kernel that reads a neighbouring column changes its result).  off = 8 keeps every row
    16-byte aligned (the widest vector instantiation the width allows); off = 1 misaligns the base pointer: the scalar one."""
    if off is None:
        return t.to(DEV)
    n, d = t.shape
    wide = torch.full((n, d + SLAB_PAD), fill, dtype=t.dtype, device=DEV)
    wide[:, off:off + d] = t.to(DEV)
    return wide[:, off:off + d]


def _path(D, dtype, off):
    """'v<VEC>c<CH>': the rowwise_bwd_kernel instantiation that pick_vec / pick_chunks (csrc/rowwise_common.h, the one copy both
    row-wise sources use) select for this slab (for the test ids)."""
    vec = 16 // torch.empty((), dtype=dtype).element_size() if off != 1 else 1
    ld = D if off is None else D + SLAB_PAD
    while vec > 1 and (D % vec or ld % vec):
        vec //= 2
    ch = next((c for c in (1, 2, 4, 8) if D <= 64 * vec * c), 0)
    return f"v{vec}c{ch}"


def _id(N, D, dtype, off):
    lay = {None: "contig", 8: "slab8", 1: "slab1"}[off]
    return f"N{N}-D{D}-{NAME[dtype]}-{lay}-{_path(D, dtype, off)}"


def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int8)


# ------------------------------------------------------------------------------------------------------------- colsum (exact)
# rowwise_bwd_kernel runs min(ceil(N / 8), 512) blocks of 8 waves (at most 4 096 waves walking rows w, w + nw, ...); each block
# writes one partial row for reduce_partials_kernel.
#      N      partial rows                                              rows per wave
#      0      0   (the nw = 0 branch: zero sums)                        -
#      1, 7, 8    1   (63 of the 64 groups own no partial row)          0 or 1 (N = 1, 7: idle waves in the block)
#      9      2                                                         0 or 1
#    511     64   (every group owns exactly one)                        0 or 1
#  1 029    129   (tail loop: up to three rows per group)               0 or 1
#  1 544    193   (the four-accumulator main loop runs, for group 0)    1
#  1 545    194   (main loop for groups 0 and 1)                        0 or 1
#  2 500    313   (main loop once, then a tail row for groups 0..56)    0 or 1
#  4 096    512   (main loop twice per group, no tail)                  1
#  4 097    512                                                         1, wave 0: 2
# 12 345    512                                                         3 or 4
# 40 320    512                                                         9 or 10
# 81 840    512                                                         19 or 20
COLSUM_N = [0, 1, 7, 8, 9, 511, 1029, 1544, 1545, 2500, 4096, 4097, 12345, 40320, 81840]
COLSUM_SHAPES = [(N, 512) for N in COLSUM_N] + [(N, D) for N in (4097, 40320) for D in (100, 33, 2048, 4096)]


def _row_cases(shapes, offs, max_scalar_d=512):
    """shapes x dtypes x slab offsets; D = 4096 in 16 bit only (fp32 rows hold 64 * 4 * 8 = 2048), and the scalar instantiation
    of a misaligned slab holds 64 * 8 = 512 elements."""
    out = []
    for dtype in DTYPES:
        for off in offs:
            for N, D in shapes:
                if (D == 4096 and dtype == F32) or (off == 1 and D > max_scalar_d):
                    continue
                out.append(pytest.param(N, D, dtype, off, id=_id(N, D, dtype, off)))
    return out


@pytest.mark.parametrize("N,D,dtype,off", _row_cases(COLSUM_SHAPES, (8, 1)))
def test_colsum_exact(ops, N, D, dtype, off):
    gen = torch.Generator().manual_seed(131 * N + D)
    xi = _ints(gen, -4, 4, (N, D))
    want = xi.sum(0, dtype=torch.int64)
    assert int(xi.abs().sum(0, dtype=torch.int64).max()) < 2 ** 24  # every partial sum is exact in fp32, in any order
    got = ops.colsum(_slab(xi.to(dtype), off))
    assert got.dtype == F32 and got.shape == (D,)
    assert torch.equal(got.cpu().double(), want.double()), f"{int((got.cpu().double() != want.double()).sum())} of {D} columns differ"


def test_colsum_misaligned_slab_refuses_rows_beyond_the_scalar_instantiation(ops):
    x = torch.zeros(9, 1024 + SLAB_PAD, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="too large for the register-resident row"):
        ops.colsum(x[:, 1:1025])
    assert torch.equal(ops.colsum(x[:, 8:1032]), torch.zeros(1024, device=DEV))  # the same width, aligned: accepted


# --------------------------------------------------------------------------------------------------- LayerNorm backward
LN_SHAPES = ([(4097, D) for D in (512, 64, 100, 33, 1024, 2048, 4096)] + [(N, 512) for N in (1, 9, 1029, 12345, 40320)]
             + [(40320, 1024)])
LN_CASES = _row_cases(LN_SHAPES, (8, 1))


def _ln_inputs(N, D, dtype, offset_over_sigma=0.0):
    gen = torch.Generator().manual_seed(7 * N + D)
    if offset_over_sigma:  # rows far from zero: mean / sigma up to the given ratio, both signs
        x = torch.randn(N, D, generator=gen) + torch.linspace(-offset_over_sigma, offset_over_sigma, N)[:, None]
    else:
        x = 1.5 * torch.randn(N, D, generator=gen) + 0.3
    dy = torch.randn(N, D, generator=gen)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=gen)
    return x.to(dtype), dy.to(dtype), gamma.to(dtype)


def _ln_autograd(x, dy, gamma, prec):
    D = x.shape[1]
    xs, gs = x.to(prec).requires_grad_(True), gamma.to(prec).requires_grad_(True)
    bs = torch.zeros(D, dtype=prec, requires_grad=True)
    F.layer_norm(xs, (D,), gs, bs, 1e-5).backward(dy.to(prec))
    return xs.grad, gs.grad, bs.grad


def _check_ln_backward(ops, N, D, dtype, off, offset_over_sigma=0.0):
    x, dy, gamma = _ln_inputs(N, D, dtype, offset_over_sigma)
    want_dx, want_dg, want_db = _ln_autograd(x, dy, gamma, torch.float64)
    _, ref_dg, ref_db = _ln_autograd(x, dy, gamma, torch.float32)
    xd, dyd, gd = _slab(x, off), _slab(dy, off, fill=-2.0), gamma.to(DEV)
    dx, dg, db = ops.layer_norm_backward(dyd, xd, gd)
    assert dx.dtype == dtype and dg.dtype == F32 and db.dtype == F32 and dg.shape == (D,) and db.shape == (D,)
    assert_close(dx, want_dx, dtype, "dx")
    for name, got, want, ref in (("dgamma", dg, want_dg, ref_dg), ("dbeta", db, want_db, ref_db)):
        scale = float(want.abs().max())
        err_kernel = float((got.cpu().double() - want).abs().max()) / scale
        err_torch = float((ref.double() - want).abs().max()) / scale
        bound = max(8.0 * err_torch, 2e-5)
        print(f"LNBWD {_id(N, D, dtype, off)} o/s={offset_over_sigma:g} {name}: kernel {err_kernel:.3e} torch-fp32 {err_torch:.3e} "
              f"kernel/torch {err_kernel / max(err_torch, 1e-30):.2f} kernel/bound {err_kernel / bound:.4f}")
        assert err_kernel <= bound, f"{name}: kernel error {err_kernel:.3e} of max|want| > bound {bound:.3e} (torch fp32: {err_torch:.3e})"
    dx_only, no_dg, no_db = ops.layer_norm_backward(dyd, xd, gd, need_param_grads=False)
    assert no_dg is None and no_db is None and torch.equal(dx_only, dx)


@pytest.mark.parametrize("N,D,dtype,off", LN_CASES)
def test_layer_norm_backward_vs_float64(ops, N, D, dtype, off):
    _check_ln_backward(ops, N, D, dtype, off)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_layer_norm_backward_rows_far_from_zero(ops, dtype):
    """|mean| / sigma up to 16 (what tests/test_chain_gpu.py does for the forward): the two-pass statistics hold."""
    _check_ln_backward(ops, 4097, 512, dtype, 8, offset_over_sigma=16.0)


@pytest.mark.parametrize("N,D,dtype,off", LN_CASES)
def test_layer_norm_backward_dbeta_exact(ops, N, D, dtype, off):
    """d_beta is the column sum of d_y: integer d_y, random x."""
    gen = torch.Generator().manual_seed(11 * N + D)
    x, _, gamma = _ln_inputs(N, D, dtype)
    dyi = _ints(gen, -4, 4, (N, D))
    want = dyi.sum(0, dtype=torch.int64)
    assert int(dyi.abs().sum(0, dtype=torch.int64).max()) < 2 ** 24
    _, _, db = ops.layer_norm_backward(_slab(dyi.to(dtype), off), _slab(x, off), gamma.to(DEV))
    assert torch.equal(db.cpu().double(), want.double()), f"{int((db.cpu().double() != want.double()).sum())} of {D} columns differ"


def test_layer_norm_backward_refusals(ops):
    for D, dtype in ((4096, F32), (8192, BF16)):
        x = torch.zeros(5, D, dtype=dtype, device=DEV)
        with pytest.raises(ValueError, match="too large for the register-resident row"):
            ops.layer_norm_backward(x, x, torch.ones(D, dtype=dtype, device=DEV))
    x = torch.zeros(64, 64, dtype=F32, device=DEV)
    g = torch.ones(64, dtype=F32, device=DEV)
    with pytest.raises(ValueError, match="last dimension must be contiguous"):
        ops.layer_norm_backward(x, x.t(), g)
    with pytest.raises(ValueError, match="last dimension must be contiguous"):
        ops.layer_norm_backward(x.t(), x, g)
    with pytest.raises(ValueError, match="does not match"):
        ops.layer_norm_backward(x.to(BF16), x, g)


# -------------------------------------------------------------------------------------------- conditional LayerNorm (float64)
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("D", [512, 100, 33, 1024])
@pytest.mark.parametrize("N", [1, 5, 1030, 10242])
def test_cond_layer_norm_forward_backward_vs_float64(ops, N, D, dtype):
    gen = torch.Generator().manual_seed(3 * N + D)
    x = (1.5 * torch.randn(N, D, generator=gen) + 0.3).to(dtype)
    ss = (0.5 * torch.randn(N, 2 * D, generator=gen)).to(dtype)  # [scale | shift]: one projection output, as layers/normalization.py passes it
    dy = torch.randn(N, D, generator=gen).to(dtype)
    xs, sc, sh = x.double().requires_grad_(True), ss[:, :D].double().requires_grad_(True), ss[:, D:].double()
    want_y = F.layer_norm(xs, (D,), None, None, 1e-5) * (sc + 1.0) + sh
    want_y.backward(dy.double())
    xd, ssd, dyd = x.to(DEV), ss.to(DEV), dy.to(DEV)
    y = ops.cond_layer_norm(xd, ssd[:, :D], ssd[:, D:])
    dx, ds = ops.cond_layer_norm_backward(dyd, xd, ssd[:, :D])
    assert y.dtype == dtype and dx.dtype == dtype and ds.dtype == dtype
    assert_close(y, want_y.detach(), dtype, "y")
    assert_close(dx, xs.grad, dtype, "dx")
    assert_close(ds, sc.grad, dtype, "d_scale")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("D", [512, 100, 33, 1024])
def test_cond_layer_norm_zero_scale_shift_is_layer_norm(ops, D, dtype):
    gen = torch.Generator().manual_seed(D)
    N = 1030
    x = (1.5 * torch.randn(N, D, generator=gen) + 0.3).to(dtype)
    want = F.layer_norm(x.double(), (D,), None, None, 1e-5)
    zeros = torch.zeros(N, 2 * D, dtype=dtype, device=DEV)
    y = ops.cond_layer_norm(x.to(DEV), zeros[:, :D], zeros[:, D:])
    plain = ops.layer_norm(x.to(DEV), torch.ones(D, dtype=dtype, device=DEV), None)
    assert_close(y, want, dtype, "cond_layer_norm(scale=0, shift=0)")
    assert_close(plain, want, dtype, "layer_norm(weight=1)")
    assert_close(y, plain.double(), dtype, "cond_layer_norm(scale=0, shift=0) vs layer_norm(weight=1)")


# ------------------------------------------------------------------------------------------------------------- GELU (float64)
def _phi_cdf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _phi_pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _activation_points(n, D):
    """[n, D]: [-8, 8] densely, then +-0 and the saturated tails +-30 (the last six elements of the last row)."""
    tail = torch.tensor([0.0, -0.0, 30.0, -30.0, 30.0, -30.0])
    return torch.cat([torch.linspace(-8.0, 8.0, n * D - tail.numel()), tail]).view(n, D)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("off", [None, 8, 1], ids=["contig", "slab8", "slab1"])
@pytest.mark.parametrize("D", [512, 100, 33])
def test_gelu_forward_backward_vs_float64(ops, D, off, dtype):
    gen = torch.Generator().manual_seed(D)
    n = 40
    x = _activation_points(n, D).to(dtype)
    dy = torch.randn(n, D, generator=gen).to(dtype)
    x64, dy64 = x.double(), dy.double()
    want_y = x64 * _phi_cdf(x64)
    want_dx = dy64 * (_phi_cdf(x64) + x64 * _phi_pdf(x64))
    xd, dyd = x.to(DEV), _slab(dy, off)  # row-strided d_y
    y = ops.gelu(xd.view(4, n // 4, D))  # inference call on a 3-D input
    assert y.shape == (4, n // 4, D) and y.dtype == dtype
    assert_close(y.view(n, D), want_y, dtype, "gelu")
    dx = ops.gelu_backward(xd, dyd)
    assert_close(dx, want_dx, dtype, "gelu_backward")
    # the derivative's saturated tails: d_y itself at +30, 0 at -30 (erf(+-21) = +-1 and exp(-450) = 0 in fp32)
    assert torch.equal(dx[-1, -4:].cpu()[[0, 2]], dy[-1, -4:][[0, 2]]) and float(dx[-1, -4:].cpu()[[1, 3]].abs().max()) == 0.0
    if off is not None:  # pre as the strided operand, too
        assert torch.equal(ops.gelu_backward(_slab(x, off), dyd), dx)


# -------------------------------------------------------------------------------------------------------------- GLU (float64)
def _glu_ref(kind, g, v, d):
    """(out, d_gate, d_value) in the precision of the arguments."""
    s = torch.sigmoid(g)
    if kind == "glu":
        act, grad = s, s * (1.0 - s)
    elif kind == "swiglu":
        act, grad = g * s, s * (1.0 + g * (1.0 - s))
    elif kind == "geglu":
        act, grad = g * _phi_cdf(g), _phi_cdf(g) + g * _phi_pdf(g)
    else:
        act, grad = torch.relu(g), (g > 0).to(g.dtype)
    return act * v, d * v * grad, d * act


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("D", [512, 100, 33])
@pytest.mark.parametrize("kind", ["glu", "swiglu", "geglu", "reglu"])
def test_glu_forward_backward_vs_float64(ops, kind, D, dtype):
    gen = torch.Generator().manual_seed(D)
    n = 40
    gate = _activation_points(n, D)
    gate[:, 5::7] = 0.0  # gate = 0: ReGLU's kink
    gate[:, 6::14] = -0.0
    gv = torch.cat([gate, torch.randn(n, D, generator=gen)], dim=1).to(dtype)
    d = torch.randn(n, D, generator=gen).to(dtype)
    want_out, want_dg, want_dv = _glu_ref(kind, gv[:, :D].double(), gv[:, D:].double(), d.double())
    gvd = _slab(gv, 8)  # [N, 2D] as a column slab of a wider buffer
    out = ops.glu(gvd, kind)
    assert out.shape == (n, D) and out.dtype == dtype
    assert_close(out, want_out, dtype, f"{kind} out")
    dgv = ops.glu_backward(gvd, d.to(DEV), kind)
    assert dgv.shape == (n, 2 * D) and dgv.dtype == dtype
    assert_close(dgv[:, :D], want_dg, dtype, f"{kind} d_gate")
    assert_close(dgv[:, D:], want_dv, dtype, f"{kind} d_value")
    if kind == "reglu":  # the kernel's g > 0: no gradient through a gate of exactly zero
        at_zero = (gv[:, :D] == 0)
        assert int(at_zero.sum()) > 0 and float(dgv[:, :D].cpu()[at_zero].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- segment_sum_rows (exact)
SEG_DEGREES = [0, 1, 2, 3, 5, 8, 37, 200, 0, 1, 3, 8, 0]  # first and last segment empty; one empty in the middle


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("off", [None, 8, 1], ids=["contig", "slab8", "slab1"])
@pytest.mark.parametrize("with_ids", [False, True], ids=["sorted", "ids"])
@pytest.mark.parametrize("D", [512, 100, 33])
def test_segment_sum_rows_exact(ops, D, with_ids, off, dtype):
    gen = torch.Generator().manual_seed(D + with_ids)
    deg = torch.tensor(SEG_DEGREES)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    E = int(ptr[-1])
    hi = EXACT_INT[dtype] // max(SEG_DEGREES) if dtype != F32 else 4  # bf16: 1, fp16: 10 -> the longest segment stays exact
    hi = min(hi, 4)
    if with_ids:  # rows used several times (E draws from 120 rows) and rows never used (rows 120.. of E + 30)
        n_src, ids = E + 30, torch.randint(0, 120, (E,), generator=gen)
        assert ids.unique().numel() < E
    else:
        n_src, ids = E, torch.arange(E)
    xi = _ints(gen, -hi, hi, (n_src, D)).to(torch.int64)
    want = torch.stack([xi[ids[ptr[r]:ptr[r + 1]]].sum(0) for r in range(len(SEG_DEGREES))])
    abs_sum = torch.stack([xi[ids[ptr[r]:ptr[r + 1]]].abs().sum(0) for r in range(len(SEG_DEGREES))])
    assert int(abs_sum.max()) <= EXACT_INT[dtype]
    got = ops.segment_sum_rows(_slab(xi.to(dtype), off), ptr.to(torch.int32).to(DEV), ids.to(torch.int32).to(DEV) if with_ids else None)
    assert got.dtype == dtype and got.shape == want.shape
    assert torch.equal(got.cpu().double(), want.double())
    assert float(got[[0, 8, 12]].abs().max()) == 0.0  # empty segments: exact zero rows


# ----------------------------------------------------------------------------------------------------- gather_add_rows (exact)
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("off", [None, 8, 1], ids=["contig", "slab8", "slab1"])
@pytest.mark.parametrize("D", [512, 100, 33])
def test_gather_add_rows_bit_exact(ops, D, off, dtype):
    """One fp32 add and one rounding (the precedent: test_assemble_output_residual_columns)."""
    gen = torch.Generator().manual_seed(D)
    n, n_b = 301, 50
    a, b = torch.randn(n, D, generator=gen).to(dtype), torch.randn(n_b, D, generator=gen).to(dtype)
    idx = torch.randint(0, 40, (n,), generator=gen)  # repeated indices; rows 40.. of b are never used
    want = (a.float() + b.float()[idx]).to(dtype)
    got = ops.gather_add_rows(_slab(a, off), b.to(DEV), idx.to(torch.int32).to(DEV))  # row-strided a
    assert got.dtype == dtype and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------------- transpose_pad (exact)
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("off", [None, 1], ids=["contig", "slab1"])
@pytest.mark.parametrize("mult", [64, 512, 64 * 157])
@pytest.mark.parametrize("n,c", [(1, 1), (63, 65), (64, 64), (65, 63), (1029, 36), (10242, 100)])
def test_transpose_pad_exact(ops, n, c, mult, off, dtype):
    gen = torch.Generator().manual_seed(n + c)
    x = (torch.randn(n, c, generator=gen) + 4.0).to(dtype)
    got = ops.transpose_pad(_slab(x, off), mult)  # off = 1: a row-strided source
    n_pad = (n + mult - 1) // mult * mult
    assert got.shape == (c, n_pad) and got.dtype == dtype and got.is_contiguous()
    want = torch.zeros(c, n_pad, dtype=dtype)
    want[:, :n] = x.t()
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------- split-K weight-gradient GEMM (exact)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=NAME.get)
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("splits", [1, 2, 5, 19, 157])
@pytest.mark.parametrize("C", [36, 100, 512])
@pytest.mark.parametrize("R", [36, 100, 512])
def test_linear_splitk_exact(ops, R, C, splits, m, dtype):
    """Integer operands: every fp32 partial product sum is an integer below 2^24, so the result is the integer product in
    whatever order the atomics land.  (The product is evaluated in float64, which is exact for these magnitudes.)"""
    gen = torch.Generator().manual_seed(R + 7 * C + splits)
    K = 64 * splits * m
    a, b = _ints(gen, -2, 2, (R, K)), _ints(gen, -2, 2, (C, K))
    assert 4 * K < 2 ** 24
    want = (a.double() @ b.double().t()).to(torch.int64)
    got = ops.linear_splitk(a.to(dtype).to(DEV), b.to(dtype).to(DEV), splits)
    assert got.dtype == F32 and got.shape == (R, C)
    assert torch.equal(got.cpu().double(), want.double()), f"{int((got.cpu().double() != want.double()).sum())} of {R * C} elements differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", [77, 5000, 40320])
def test_weight_grad_fallback_route_exact(ops, N, dtype):
    """Widths that are multiples of 4 but not of 8: 16-bit operands take transpose_pad + linear_splitk with
    splits = 1 / 19 / 157 (and a reduction length padded to 64 * splits), fp32 operands transpose_pad + the forward GEMM."""
    from anemoi_core_amd import autograd

    gen = torch.Generator().manual_seed(N)
    dz, x = _ints(gen, -2, 2, (N, 36)), _ints(gen, -2, 2, (N, 20))
    assert 4 * N < 2 ** 24
    want = (dz.double().t() @ x.double()).to(torch.int64)
    assert not ops.linear_wgrad_eligible(dz.to(dtype), x.to(dtype))
    got = autograd._weight_grad(dz.to(dtype).to(DEV), x.to(dtype).to(DEV))
    assert got.shape == (36, 20)
    assert torch.equal(got.cpu().double(), want.double())


# ------------------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_fixed_order_reductions_are_deterministic(ops, dtype):
    """csrc/rowwise_bwd.hip promises fixed-order reductions: the same call twice gives the same bits on real-valued data."""
    N, D = 40320, 512
    x, dy, gamma = _ln_inputs(N, D, dtype)
    xd, dyd, gd = x.to(DEV), dy.to(DEV), gamma.to(DEV)
    assert torch.equal(ops.colsum(xd), ops.colsum(xd))
    for a, b in zip(ops.layer_norm_backward(dyd, xd, gd), ops.layer_norm_backward(dyd, xd, gd)):
        assert torch.equal(a, b)
    gen = torch.Generator().manual_seed(1)
    deg = torch.randint(0, 40, (2000,), generator=gen)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32).to(DEV)
    assert int(deg.sum()) <= N
    ids = torch.randint(0, N, (int(deg.sum()),), generator=gen).to(torch.int32).to(DEV)
    assert torch.equal(ops.segment_sum_rows(xd, ptr, ids), ops.segment_sum_rows(xd, ptr, ids))


# -------------------------------------------------------------------------------------------------------------------- zero rows
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_zero_rows(ops, dtype):
    """A rank that owns no edge of a shard: empty results, exact-zero sums (reduce_partials_kernel's nw = 0 branch), no error."""
    D = 100
    z = torch.empty(0, D, dtype=dtype, device=DEV)
    z2 = torch.empty(0, 2 * D, dtype=dtype, device=DEV)
    gamma = torch.ones(D, dtype=dtype, device=DEV)
    zero_sums = torch.zeros(D, dtype=F32, device=DEV)
    ops._reduce_workspace(D, z.device).fill_(7.0)  # stale partial rows of an earlier call must not be read
    assert torch.equal(ops.colsum(z), zero_sums)
    dx, dg, db = ops.layer_norm_backward(z, z, gamma)
    assert dx.shape == (0, D) and dx.dtype == dtype and torch.equal(dg, zero_sums) and torch.equal(db, zero_sums)
    dx, dg, db = ops.layer_norm_backward(z, z, gamma, need_param_grads=False)
    assert dx.shape == (0, D) and dg is None and db is None
    assert ops.cond_layer_norm(z, z2[:, :D], z2[:, D:]).shape == (0, D)
    dx, ds = ops.cond_layer_norm_backward(z, z, z2[:, :D])
    assert dx.shape == (0, D) and ds.shape == (0, D)
    assert ops.gelu(z).shape == (0, D) and ops.gelu(z.view(0, 4, 25)).shape == (0, 4, 25)
    assert ops.gelu_backward(z, z).shape == (0, D)
    for kind in ops.GLU_KINDS:
        assert ops.glu(z2, kind).shape == (0, D) and ops.glu_backward(z2, z, kind).shape == (0, 2 * D)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    assert ops.segment_sum_rows(z, i32(0)).shape == (0, D)  # no output rows
    for ids in (None, i32()):  # output rows, but nothing to sum: exact zeros
        assert torch.equal(ops.segment_sum_rows(z, i32(0, 0, 0), ids), torch.zeros(2, D, dtype=dtype, device=DEV))
    assert ops.gather_add_rows(z, gamma.view(1, D), i32()).shape == (0, D)
    assert ops.transpose_pad(z, 64).shape == (D, 0)
