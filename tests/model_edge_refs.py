"""Plain-torch CPU restatements of the model-edge kernels (csrc/rowwise.hip: assemble_input[_norm[_vec8]], assemble_output[_norm],
affine_columns, bound_columns) and the input sets their tests share.  Nothing here imports ``anemoi_core_amd.ops`` or
``tests.cpu_ops_shim``: each function writes out the reference's op sequence on CPU tensors, with the roundings the reference's
tensors perform, so tests/test_model_edge_kernels_gpu.py can hold the kernels to it and tests/test_model_edge_refs_cpu.py can
hold THESE functions to the reference's recorded outputs.

Reference lines: models/encoder_processor_decoder.py:98-163 (input / output assembly), preprocessing/normalizer.py:154-252 (the
normaliser), layers/bounding.py:81-307 and layers/activations.py:16-42 (the boundings)."""
import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
INT_VIEW = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}

# bound_columns: allowed error per op, |got - want| <= U * s with s = max(|want|, |v|, |p0|, |p1|, |x[tot]|) of the element.
# fp32: one FMA contraction or one rounding-order difference against the float64 evaluation (a few 2^-24, see bounding_ref);
# 16 bit: the final rounding to T plus one intermediate rounding to T (2 * 2^-8 bf16, 2 * 2^-11 fp16) - one rounding to T more
# or fewer than torch makes on a T tensor.
U = {F32: 2.0 ** -22, BF16: 2.0 ** -7, F16: 2.0 ** -10}
# "+-tiny" / "+-large" of the bounding input set: finite in T after every kind (x 0.01, x total, / 0.301) - see bounding_inputs
TINY = {F32: 1e-30, BF16: 1e-30, F16: 1e-3}
LARGE = {F32: 1e30, BF16: 1e30, F16: 1e4}
BOUND_PAIRS = [(0.0, 1.0), (-0.5, 0.7), (0.3, 0.3 + 1e-3), (-3.25, 1e4)]


def assert_bits_equal(got, want, what=""):
    """Same dtype, same shape, NaN at the same places, every other element equal BIT for bit (-0.0 is not +0.0)."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), f"{what}: NaN at {int((got.isnan() != nan).sum())} other places"
    gi, wi = got.contiguous().view(INT_VIEW[got.dtype]), want.contiguous().view(INT_VIEW[want.dtype])
    bad = (gi != wi) & ~nan
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {float(got[at])!r}, want {float(want[at])!r}")


# ------------------------------------------------------------------------------------------------------------ input sets
def column_stats(V, dtype=F32, seed=0):
    """(mul, add) fp32 [V] like real statistics: 1 / stdev and -mean / stdev with |mean|, stdev from 1e-5 to 1e5 (1e4 for fp16
    data, whose largest finite value is 65 504) cycling over the columns; also returns (mean, stdev) float64 to draw data from."""
    g = torch.Generator().manual_seed(1000 + seed)
    top = 1e4 if dtype == F16 else 1e5
    scale = torch.tensor([1e-5, 1e-2, 1.0, 273.15, top], dtype=torch.float64)[torch.arange(V) % 5]
    mean = scale * (torch.rand(V, generator=g, dtype=torch.float64) * 2 - 1)
    stdev = scale * (0.25 + torch.rand(V, generator=g, dtype=torch.float64))
    return (1.0 / stdev).float(), (-mean / stdev).float(), mean, stdev


def raw_data(shape, dtype, mean, stdev, seed=0, specials=True):
    """Raw data [..., V] in ``dtype``: mean + stdev * N(0, 1) per column (so x * mul + add cancels to O(1) and the fp32 product's
    rounding shows in the sum: the two-rounding and the fused result differ on a good share of the elements), with a few NaN,
    +-inf and -0.0 planted when the tensor has room for them."""
    g = torch.Generator().manual_seed(2000 + seed)
    x = (mean + stdev * torch.randn(shape, generator=g, dtype=torch.float64)).to(dtype)
    flat = x.view(-1)
    if specials and flat.numel() >= 64:
        for k, val in enumerate((float("nan"), float("inf"), float("-inf"), -0.0, float("nan"), 0.0)):
            flat[(k * 37 + 5) % flat.numel()] = val
            flat[flat.numel() - 1 - (k * 53 + 3) % flat.numel()] = val
    return x


# ------------------------------------------------------------------------------------------------------------ assembly
def assemble_input_ref(x, attrs, width, mul=None, add=None, out_dtype=None):
    """x [T, N, V] (any strides), attrs [N, A] of the output dtype or None -> [N, width]: columns t * V + v hold
    TO(fp32(x[t, n, v]) * mul[v] + add[v]) - two fp32 roundings, then one to TO - or TO(x[t, n, v]) without a normaliser; then the
    attributes unchanged; then zeros ("batch time ensemble grid vars -> (batch ensemble grid) (time vars)" + cat,
    encoder_processor_decoder.py:98-143, after InputNormalizer.transform, normalizer.py:154-190)."""
    T, N, V = x.shape
    to = x.dtype if out_dtype is None else out_dtype
    v = x.float()
    if mul is not None:
        v = v.mul(mul).add(add)
    parts = [v.to(to).permute(1, 0, 2).reshape(N, T * V)]
    A = 0
    if attrs is not None:
        assert attrs.dtype == to
        parts.append(attrs)
        A = attrs.shape[1]
    parts.append(torch.zeros(N, width - T * V - A, dtype=to))
    return torch.cat(parts, 1)


def assemble_output_ref(x_out, x_skip, col_map, mul=None, add=None):
    """out = TS(x_out); on the columns with col_map[v] >= 0: out = TS(fp32(out) + fp32(sk)), sk = x_skip[n, m] or, with a
    normaliser, TS(fp32(x_skip[n, m]) * mul[m] + add[m]) - two fp32 roundings, then one to TS (x_out.to(dtype=x.dtype) and the
    index_add_ of the skip connection, encoder_processor_decoder.py:145-158, on the normalised input)."""
    ts = x_skip.dtype
    out = x_out.to(ts).clone()  # .to() of the same dtype is x_out itself
    sk = x_skip.float()
    if mul is not None:
        sk = sk.mul(mul).add(add).to(ts).float()
    cols = (col_map >= 0).nonzero().reshape(-1)
    src = col_map[cols].long()
    out[:, cols] = (out[:, cols].float() + sk[:, src]).to(ts)
    return out


def affine_ref(x, mul, add, inverse=False):
    """torch's own in-place sequence on a CPU tensor of x's dtype (normalizer.py:186-190, 246-252): every step rounds to it."""
    if inverse:
        return x.clone().subtract_(add).div_(mul)
    return x.clone().mul_(mul).add_(add)


# ------------------------------------------------------------------------------------------------------------ boundings
def _leaky_hardtanh(v, lo, hi, slope=0.01):  # layers/activations.py:16-42
    y = torch.clamp(v, lo, hi)
    y = torch.where(v < lo, lo + slope * (v - lo), y)
    return torch.where(v > hi, hi + slope * (v - hi), y)


def _fabs(t):
    """|t| where t is finite, 0 elsewhere (an infinite or NaN term says nothing about the size of a rounding error)."""
    return torch.where(t.isfinite(), t.abs(), torch.zeros_like(t))


def bounding_ref(x, program):
    """The column program (kind, column, total column, p0, p1) evaluated in float64, op by op and in order, on the T-rounded input
    x [..., V] with the parameters as the fp32 table holds them: kinds 1..8 with the reference's formulas (bounding.py:81-307:
    relu, leaky_relu, relu(x - m) + m, leaky_relu(x - m) + m, hardtanh, leaky_hardtanh, and the last two times x[total]; slopes
    0.01), kind 9 (x - add) / mul (normalizer.py:246-252).  Returns (want, bound), both float64 [..., V].

    bound: each op adds U[T] * s, s = max(|want|, |v|, |p0|, |p1|, |x[tot]|) over the finite ones the kind reads, to what the op's inputs
    already carry - carried through the op by its Lipschitz constant (1 for kinds 1..6; |f(v)| and |x[tot]| for the products;
    1 / |mul| for kind 9).  For a column touched once, bound = U[T] * s exactly.  Why U[T] * s covers one op:
      fp32  the kernel makes at most four fp32 roundings where float64 makes none - e.g. kind 8: t - p1, the FMA p1 + 0.01f * ..,
            the product, and 0.01f against 0.01 (2^-25.4) - each at most 2^-24 of a quantity no larger than s: < 2^-22 s.  The
            leaky kinds are contracted into one FMA (v_fmamk_f32), so they are not bit-equal to torch's two roundings: that is
            the "one contraction" the bound allows, and the reason the leaky kinds are not asserted exact;
      16bit the result is rounded to T once (2^-8 bf16, 2^-11 fp16, relative to |want|), and kinds 7 / 8 / 9 round one
            intermediate to T as torch does on a T tensor (hardtanh before the product, the difference before the division):
            (1 + d)^2 - 1 < 2 * 2^-8 for |d| <= 2^-8 / (1 + 2^-8); the fp32 arithmetic in between is 2^-16 of that."""
    u = U[x.dtype]
    cols = [c.double() for c in x.unbind(-1)]
    errs = [torch.zeros_like(c) for c in cols]
    for kind, col, tot, p0, p1 in program:
        p0, p1 = float(torch.tensor(p0, dtype=F32)), float(torch.tensor(p1, dtype=F32))
        v, ev = cols[col], errs[col]
        t, et = cols[tot], errs[tot]
        # the parameters the kind reads: none for 1 / 2, the minimum for 3 / 4, both for the rest
        s_terms = [_fabs(v)] + [torch.full_like(v, abs(p)) for p in ((), (p0,), (p0, p1))[0 if kind <= 2 else 1 if kind <= 4 else 2]]
        if kind == 1:
            w, e = torch.relu(v), ev
        elif kind == 2:
            w, e = F.leaky_relu(v, 0.01), ev
        elif kind == 3:
            w, e = torch.relu(v - p0) + p0, ev
        elif kind == 4:
            w, e = F.leaky_relu(v - p0, 0.01) + p0, ev
        elif kind == 5:
            w, e = F.hardtanh(v, p0, p1), ev
        elif kind == 6:
            w, e = _leaky_hardtanh(v, p0, p1), ev
        elif kind in (7, 8):
            f = F.hardtanh(v, p0, p1) if kind == 7 else _leaky_hardtanh(v, p0, p1)
            w = f * t
            e = _fabs(f) * et + _fabs(t) * ev + ev * et
            s_terms.append(_fabs(t))
        elif kind == 9:
            w, e = (v - p0) / p1, ev / abs(p1)
        else:
            raise ValueError(kind)
        s = torch.stack(s_terms + [_fabs(w)]).amax(0)
        cols[col] = w
        errs[col] = torch.where(w.isfinite(), e + u * s, torch.zeros_like(e))  # NaN / +-inf are required exactly
    return torch.stack(cols, -1), torch.stack(errs, -1)


def check_bounding(got, want, bound, what=""):
    """NaN exactly where want has it and nowhere else; +-inf exactly; |got - want| <= bound on the finite rest."""
    g = got.detach().cpu().double()
    assert g.shape == want.shape, (g.shape, want.shape)
    nan, inf = want.isnan(), want.isinf()
    wrong = g.isnan() != nan
    assert not bool(wrong.any()), (f"{what}: NaN mismatch at {int(wrong.sum())} elements, first {tuple(int(i) for i in wrong.nonzero()[0])} "
                                   f"(got {float(g[wrong][0])}, want {float(want[wrong][0])})")
    assert torch.equal(g[inf], want[inf]), f"{what}: infinities differ: got {g[inf].tolist()}, want {want[inf].tolist()}"
    fin = ~(nan | inf)
    err, lim = (g - want).abs()[fin], bound[fin]
    over = err > lim
    if bool(over.any()):
        k = int((err - lim).argmax())
        raise AssertionError(f"{what}: {int(over.sum())} elements beyond the bound; worst: got {float(g[fin][k])!r} want {float(want[fin][k])!r} "
                             f"err {float(err[k]):.3e} bound {float(lim[k]):.3e}")


def neighbours(t):
    """The two representable neighbours of every (non-zero, finite) element of t, in t's own dtype."""
    i = t.view(INT_VIEW[t.dtype])
    return torch.cat([(i + 1).view(t.dtype), (i - 1).view(t.dtype)])


def bounding_inputs(p0, p1, dtype, seed=0):
    """[n] values of ``dtype`` dense around the bounds: T(p0), T(p1) (for fp32 the table's own values: exactly AT the bound) and their
    neighbours on both sides, 0, -0.0, +-tiny, +-large, +-inf, NaN, then 320 random ones - half 1.5 * N(0, 1), half uniform over
    [p0 - (p1 - p0) / 2, p1 + (p1 - p0) / 2].  tiny / large (TINY, LARGE) keep every kind's result finite and normal in T."""
    g = torch.Generator().manual_seed(3000 + seed)
    edge = torch.tensor([p for p in (p0, p1) if p != 0.0], dtype=F32).to(dtype)
    fixed = torch.tensor([p0, p1, 0.0, -0.0, TINY[dtype], -TINY[dtype], LARGE[dtype], -LARGE[dtype], float("inf"), float("-inf"), float("nan")],
                         dtype=F32).to(dtype)
    span = p1 - p0
    rnd = torch.cat([1.5 * torch.randn(160, generator=g), p0 - span / 2 + 2 * span * torch.rand(160, generator=g)]).to(dtype)
    return torch.cat([fixed, neighbours(edge), rnd])


def total_column(n, dtype, seed=0):
    """[n] totals for the fraction kinds: 1.5 * N(0, 1) kept inside [-4, 4], with 0, -0.0, NaN and +-inf at fixed rows (row 8 - where
    bounding_inputs has +inf - gets 0: inf * 0)."""
    g = torch.Generator().manual_seed(4000 + seed)
    t = (1.5 * torch.randn(n, generator=g)).clamp(-4.0, 4.0).to(dtype)
    for row, val in ((8, 0.0), (9, -0.0), (12, float("nan")), (13, float("inf")), (14, float("-inf")), (15, 0.0)):
        if row < n:
            t[row] = val
    return t
