"""The 16-bit MFMA window-attention kernels (csrc/window_attention.hip: win_attn_mfma_kernel; csrc/window_attention_bwd.hip:
win_attn_bwd_query_kernel, win_attn_bwd_key_kernel) with ONE DOMINANT KEY per query, placed at every band edge and carried through
every lane, wave boundary and tile position (tests/window_attention_cases.py), against the float64 dense-mask restatement.

Why: with i.i.d. normal inputs a query of window 64 spreads its softmax over 129 keys of weight ~1/129, and losing one of them moves
``out`` by about 0.008 |v|, under half the 16-bit max-error bound.  tests/test_window_attention_gpu.py and
tests/test_window_attention_backward_gpu.py notice such a loss at wide windows only where it happens to EVERY query (their mean-error
rule and 2 * e_eager then move; see the edits below) - not where it happens to one lane, one wave or one tile position, and their
fp32 cases run other kernels.  Here the key that would be lost carries about two thirds of the softmax of its query, and
tests/test_window_attention_cases_cpu.py shows on the CPU, for every case of this file, that the reference WITHOUT the hot pairs
misses every bound applied here by a factor of two or more in every affected row - with one stated exception: in 12 (case, tensor)
entries of the dominance ladder (dk at p_hot 0.99 in bf16 and at 0.999, dq at 0.999 with d = 32) it does so in 90 % or more of the rows
(asserted there: 80 %, and the median row at 4x), for the reason given in ``Case.weak_rows_allowed``.

Bounds (unchanged, those of the two existing files): forward ``_check`` (16 bit: max err <= 2e-2 max(1, max|ref|), mean <= 5e-3;
fp32 1e-5) and the same rule for the lse; backward, for out, dq, dk, dv each: max err <= 2 * e_eager, e_eager the error of eager
torch autograd of ``transformer_helpers.band_attention`` in the same 16-bit dtype on the same device (fp32: 2e-5 max|want| + 1e-6).
Every case prints "WINEDGE <case> <tensor>: err / bound".

Families:
* band ladder: bf16, d = 32, H = 2, two sequences of N = 200 = 3 * 64 + 8 rows (a partial wave and three waves past the end in the
  last workgroup; sequence 2 starts at row 200, no multiple of 16), w in {1, 15, 16, 17, 47, 48, 63, 64, 65, 100, 128} - both sides of
  the multiples of 16 and 64 the wave-skip and ``full`` conditions compare against, and w mod 64 sets the tile phase through
  lo = q0 - w - times delta in {-w, -w + 1, -1, 0, 1, w - 1, w}: the hot key first and last in every query's band, i.e. the hot query
  last and first in every key's band in the key pass.  Unbounded (None and w = N + 3) with delta in {-(N-1), -64, -63, 63, 64, N-1};
* head dims: d in {64, 128} x {bf16, fp16} x N in {200, 130} (130 = 4 * 32 + 2: the key pass's 32-query tiles at d = 128) at
  w in {17, 64}, delta = +-w; one fp32 case per d as an anchor (the plain kernels);
* FANCY: softcap 30 and / or ALiBi at w = 64, delta = +-64, d in {32, 128}, c tuned per head with the slope term included;
* dominance ladder: w = 64, delta = +-64, p_hot ~ 0.58, 0.9, 0.99, 0.999 for (d, dtype) in {(32, bf16), (64, bf16), (128, fp16)} - the
  question whether Delta = <dO, O>, formed from the 16-bit ``out``, stays inside the backward bound where one key dominates;
* the two backward passes alone (``ops.window_attention_bwd(passes=...)`` with its Delta workspace), bit-equal to autograd's;
* indicator values (v = one-hot of one key j*: out[i, h, :] = p[i, j*, h]): every row with |i - j*| <= w is NON-zero and within the
  forward bound of p, every other row and the whole other sequence an exact 0; one-hot d_out at query i of sequence 2: every dv row
  (and, for w >= 1, dk row) with |j - i| <= w has a non-zero element, every other an exact 0;
* refusals: a 16-bit q, k or v that is 8-byte but not 16-byte aligned raises a ValueError naming the rule, from both entry points,
  through the torch extension and through ctypes.

What these tests found: nothing to fix.  Every case is inside its bound, the dominance ladder included (MEASURED), so Delta stays as
it is: the diagonal of the O dO^T MFMA on the 16-bit ``out``.

What they can and cannot see, from edits made one at a time to a scratch copy of the kernels (tests failing: this file / the forward
file / the backward file):
* `<` for `<=` in the band mask of win_attn_mfma_kernel: 165 / 66 / 86; of win_attn_bwd_key_kernel: 163 / 0 / 78; of
  win_attn_bwd_query_kernel: 141 / 0 / 67.  Here every hot-key case fails (the forward edit also fails the 22 indicator tests, the
  key-pass edit the 22 one-hot tests); the two existing files notice the edit as well, at windows of 64 and 512 through their
  mean-error rule and 2 * e_eager;
* ``hi`` one too small in win_attn_mfma_kernel: 84 / 38 / 50; ``full`` of the key pass evaluated for wave 0: 30 / 0 / 12;
* the wave skip `klast < qw - w` -> `klast <= qw - w` of win_attn_bwd_query_kernel (win_attn_mfma_kernel has the same line) changes
  NOTHING - 0 / 0 / 0 - and no test can fail on it: a tile ends at klast = lo + 64 t + 63 with lo = max(0, q0 - w) and
  qw = q0 + 16 wave.  For lo = q0 - w equality needs 64 t + 63 = 16 wave, and 63 is no multiple of 16; for lo = 0 (q0 <= w) it needs
  16 wave = w - q0 + 63 + 64 t >= 63, i.e. wave >= 4.  The skip and the tile phase share q0 - w.  The argument rests on KT = 64 keys
  per tile and kOwn = 64 queries per workgroup (four waves of 16): with other tile sizes it has to be made again.  (The key pass at
  d = 128 has 32-query tiles and does reach its equality, e.g. k0 = 0, wave 3, w = 17: query 31 is the first in the band of key 48,
  the hot pair of delta = 17 in the head-dims family.)"""
import pytest
import torch

from anemoi_core_amd import ops
from tests import transformer_helpers as T
from tests import window_attention_cases as W
from tests.test_window_attention_gpu import _check

pytestmark = pytest.mark.gpu
DEV = "cuda"

# MEASURED (MI355X): worst err / bound over the cases of a family.  out (fwd) and lse: ops.window_attention without autograd against
# the forward rule; out (bwd), dq, dk, dv: autograd against 2 * e_eager (fp32: the fp32 rule).  The whole file: 204 tests in 14 s, the
# slowest 0.24 s after the first (1.9 s, which loads the library).
#   family            dtype  out (fwd)   lse      out (bwd)   dq       dk       dv
#   band ladder       bf16     0.141    <0.001     0.306     0.348    0.461    0.500
#   unbounded         bf16     0.138    <0.001     0.205     0.530    0.527    0.363
#   head dims         bf16     0.130    <0.001     0.215     0.331    0.333    0.385
#   head dims         fp16     0.016    <0.001     0.214     0.311    0.322    0.351
#   fp32 anchors      fp32     0.077     0.035     0.038     0.079    0.066    0.048
#   FANCY             bf16     0.134    <0.001     0.107     0.182    0.182    0.212
#   dominance 0.58    bf16     0.128    <0.001     0.213     0.388    0.282    0.274
#   dominance 0.9     bf16     0.107    <0.001     0.233     0.260    0.209    0.429
#   dominance 0.99    bf16     0.107    <0.001     0.282     0.827    0.579    0.436
#   dominance 0.999   bf16     0.180    <0.001     0.500     0.631    0.581    0.500
#   dominance 0.58    fp16     0.017    <0.001     0.137     0.223    0.240    0.252
#   dominance 0.9     fp16     0.013    <0.001     0.178     0.155    0.170    0.405
#   dominance 0.99    fp16     0.014    <0.001     0.318     0.486    0.568    0.500
#   dominance 0.999   fp16     0.022    <0.001     0.394     0.807    0.726    0.431
# The lse is fp32 and off by 1e-6: its bound is a 16-bit one.  The dominance ladder's worst: dq 0.827 at (64, bf16), delta = -64,
# p_hot 0.99, and 0.807 at (128, fp16), delta = 64, p_hot 0.999 - Delta from the 16-bit ``out`` costs up to 0.4 of the bound more than
# at p_hot 0.58 and stays inside it.


def _ids(cases):
    return [c.id for c in cases]


def _slopes(case):
    return None if case.slopes is None else case.slopes.float().to(DEV)


def _kw(case):
    return dict(softcap=case.softcap, alibi_slopes=_slopes(case), batch_size=case.batch)


def _run(case):
    H, w, batch, dtype = case.H, case.window, case.batch, case.dtype
    q, k, v, do = (t.to(DEV) for t in W.hot_inputs(case))
    sl64 = None if case.slopes is None else case.slopes.to(DEV)
    lse_box = []

    def ref(a, b, c):
        out, lse = W.dense_reference(a, b, c, H, w, batch, case.softcap, sl64)
        lse_box.append(lse.detach())
        return out

    want = W.autograd_of(ref, q, k, v, do, torch.float64)
    want_lse = lse_box[0]
    eager = None
    if dtype != torch.float32:
        eager = W.autograd_of(lambda a, b, c: T.band_attention(a, b, c, H, w, batch, case.softcap, sl64), q, k, v, do, dtype)
    failures = []

    def report(what, err, bound):
        print(f"WINEDGE {case.id} {what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        if not err <= bound:
            failures.append(f"{what}: err {err:.3e} > {bound:.3e}")

    # forward, no autograd
    out, lse = ops.window_attention(q, k, v, H, w, return_lse=True, **_kw(case))
    assert out.dtype == dtype and out.shape == q.shape and lse.dtype == torch.float32 and torch.isfinite(lse).all()
    report("fwd out", float((out.double() - want[0]).abs().max()), W.forward_bound(want[0], dtype))
    report("fwd lse", float((lse.double() - want_lse).abs().max()), W.forward_bound(want_lse, dtype))
    _check(out, want[0], dtype, f"{case.id} out")

    # autograd
    got = W.autograd_of(lambda a, b, c: ops.window_attention(a, b, c, H, w, **_kw(case)), q, k, v, do, dtype)
    assert torch.equal(got[0], out), f"{case.id}: the forward under autograd differs"
    for i, n in enumerate(W.NAMES):
        assert got[i].dtype == dtype and got[i].shape == q.shape and torch.isfinite(got[i]).all(), f"{case.id}: {n}"
        report(f"bwd {n}", float((got[i].double() - want[i]).abs().max()), W.backward_bound(want[i], None if eager is None else eager[i], dtype))

    # each pass alone: the query pass writes dq and Delta and nothing else, the key pass reads that Delta and writes dk and dv
    delta = torch.full((q.shape[0], H), float("nan"), device=DEV)
    bufs = tuple(torch.full_like(q, 7.0) for _ in range(3))
    ops.window_attention_bwd(do, q, k, v, out, lse, H, w, grads_out=bufs, delta=delta, passes=ops.WINDOW_BWD_QUERY_PASS, **_kw(case))
    assert torch.equal(bufs[0], got[1]) and (bufs[1] == 7).all() and (bufs[2] == 7).all() and torch.isfinite(delta).all(), case.id
    bufs[0].fill_(7.0)
    ops.window_attention_bwd(do, q, k, v, out, lse, H, w, grads_out=bufs, delta=delta, passes=ops.WINDOW_BWD_KEY_PASS, **_kw(case))
    assert (bufs[0] == 7).all() and torch.equal(bufs[1], got[2]) and torch.equal(bufs[2], got[3]), case.id
    assert not failures, f"{case.id}: " + "; ".join(failures)


@pytest.mark.parametrize("case", W.LADDER, ids=_ids(W.LADDER))
def test_band_ladder(case):
    _run(case)


@pytest.mark.parametrize("case", W.UNBOUNDED, ids=_ids(W.UNBOUNDED))
def test_unbounded_windows(case):
    _run(case)


@pytest.mark.parametrize("case", W.HEAD_DIMS + W.FP32_ANCHORS, ids=_ids(W.HEAD_DIMS + W.FP32_ANCHORS))
def test_head_dims_and_dtypes(case):
    _run(case)


@pytest.mark.parametrize("case", W.FANCY, ids=_ids(W.FANCY))
def test_softcap_and_alibi(case):
    _run(case)


@pytest.mark.parametrize("case", W.DOMINANCE, ids=_ids(W.DOMINANCE))
def test_dominance_ladder(case):
    """Delta_i = <dO_i, O_i> from the 16-bit ``out``: for the hot pair dP - Delta cancels to (1 - p) of dP, and the rounding of ``out``
    is what the cancellation leaves.  Same bound as everywhere: 2 * e_eager per tensor."""
    _run(case)


# ------------------------------------------------------------------------------------------------------------ keys inside the band
def _plain_inputs(N, H, d, batch, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(batch * N, H * d, generator=g).to(DEV, dtype) for _ in range(4))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=W.NAME.get)
@pytest.mark.parametrize("window", W.LADDER_W)
def test_indicator_values_every_key_inside_the_band_is_attended(window, dtype):
    N, H, d = W.N_LADDER, 2, 32
    q, k, _, _ = _plain_inputs(N, H, d, 2, dtype, 100 + window)
    i = torch.arange(N, device=DEV)
    for j in W.INDICATOR_KEYS:
        for keys in ((None, j), (j, None)):
            v = W.indicator_values(N, H * d, keys, dtype).to(DEV)
            out = ops.window_attention(q, k, v, H, window, batch_size=2)
            want, _ = W.dense_reference(q, k, v, H, window, 2)
            b = 0 if keys[0] is not None else 1
            mine, other = out[b * N:(b + 1) * N], out[(1 - b) * N:(2 - b) * N]
            inside = (i - j).abs() <= window
            name = f"w={window} j*={j} sequence {b} {dtype}"
            assert (other == 0).all(), f"{name}: the other sequence"
            assert (mine[~inside] == 0).all(), f"{name}: rows outside the band"
            assert (mine[inside] != 0).all(), f"{name}: rows {i[inside][(mine[inside] == 0).any(1)].tolist()} inside the band do not attend the key"
            err, bound = float((out.double() - want).abs().max()), W.forward_bound(want, dtype)
            assert err <= bound, f"{name}: p err {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=W.NAME.get)
@pytest.mark.parametrize("window", W.LADDER_W)
def test_one_hot_d_out_reaches_every_key_inside_the_band(window, dtype):
    N, H, d = W.N_LADDER, 2, 32
    q, k, v, do = _plain_inputs(N, H, d, 2, dtype, 200 + window)
    j = torch.arange(N, device=DEV)
    for i in W.INDICATOR_KEYS:
        one = torch.zeros_like(do)
        one[N + i] = do[N + i]  # query i of sequence 2
        _, dq, dk, dv = W.autograd_of(lambda a, b, c: ops.window_attention(a, b, c, H, window, batch_size=2), q, k, v, one, dtype)
        inside = (j - i).abs() <= window
        name = f"w={window} i={i} {dtype}"
        for n, t in (("dk", dk), ("dv", dv)):
            assert (t[:N] == 0).all() and (t[N:][~inside] == 0).all(), f"{name}: {n} outside the band"
            reached = (t[N:] != 0).any(1)
            assert reached[inside].all(), f"{name}: {n} rows {j[inside & ~reached].tolist()} inside the band get nothing"
        assert (dq[N + i] != 0).any() and (dq[:N + i] == 0).all() and (dq[N + i + 1:] == 0).all(), f"{name}: dq"


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _shifted(t):
    """t's values as a view 4 elements (8 bytes) into a 16-byte aligned buffer: rows 8-byte but not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[4:4 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 8 and view.stride() == t.stride()
    return view


@pytest.mark.parametrize("ctypes_path", [False, True], ids=["torch-ext", "ctypes"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=W.NAME.get)
def test_rows_that_are_not_16_byte_aligned_are_refused(monkeypatch, dtype, ctypes_path):
    from anemoi_core_amd import _ext

    if ctypes_path:
        monkeypatch.setattr(_ext, "ops", lambda: None)
    else:
        assert _ext.ops() is not None, "the torch extension did not load"
    N, H, d, w = 130, 2, 32, 17
    q, k, v, do = _plain_inputs(N, H, d, 1, dtype, 300)
    out, lse = ops.window_attention(q, k, v, H, w, return_lse=True)
    want = ops.window_attention_bwd(do, q, k, v, out, lse, H, w)
    for which in range(3):
        bad = [q, k, v]
        bad[which] = _shifted(bad[which])
        assert torch.equal(bad[which], (q, k, v)[which])
        with pytest.raises(ValueError, match="16-byte aligned rows"):
            ops.window_attention(*bad, H, w)
        with pytest.raises(ValueError, match="16-byte aligned rows"):
            ops.window_attention(*(t.detach().requires_grad_(True) for t in bad), H, w)
        # refused before any launch: NaN-filled outputs and the Delta workspace stay as they were
        into = tuple(torch.full_like(q, float("nan")) for _ in range(3))
        delta = torch.full((N, H), float("nan"), device=DEV)
        with pytest.raises(ValueError, match="16-byte aligned rows"):
            ops.window_attention_bwd(do, *bad, out, lse, H, w, grads_out=into, delta=delta)
        torch.cuda.synchronize()
        assert all(torch.isnan(t).all() for t in (*into, delta)), "a refused call wrote to its outputs"
    for which, n in ((0, "d_out"), (4, "out")):
        args = [do, q, k, v, out]
        args[which] = _shifted(args[which])
        with pytest.raises(ValueError, match="16-byte aligned rows"):
            ops.window_attention_bwd(*args, lse, H, w)
    # nothing was launched or left behind by the refusals: the same calls on the aligned tensors give the same bits as before
    again = ops.window_attention(q, k, v, H, w, return_lse=True)
    assert torch.equal(again[0], out) and torch.equal(again[1], lse)
    for a, b in zip(ops.window_attention_bwd(do, q, k, v, out, lse, H, w), want):
        assert torch.equal(a, b)
