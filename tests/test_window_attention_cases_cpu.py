"""What tests/test_window_attention_edges_gpu.py relies on, checked without a GPU (tests/window_attention_cases.py):

* the dense float64 reference agrees with ``test_window_attention_gpu.reference`` and ``transformer_helpers.band_attention`` to 1e-12,
  softcap, ALiBi, batches and the unbounded window included, and its ``exclude`` takes exactly the named pairs out of the band;
* every case's hot key has the probability the case names (median over the affected rows, per head);
* SENSITIVITY: the reference re-evaluated with the hot pairs excluded - what a kernel that lost those keys would compute - differs from
  the true reference by at least 2x the bound the GPU test applies to that tensor, in at least one element of EVERY affected
  row: out, lse, dq of the queries i with 0 <= i + delta < N; dk, dv of the keys j = i + delta.  780 (case, tensor) entries; the
  bounds are the forward rule (2e-2 max(1, max|ref|)) for out and lse and 2 * e_eager for out, dq, dk, dv, with eager torch run here,
  on the CPU, in the case's 16-bit dtype; for ``out``, which the GPU file holds to both, the larger of the two.
  EXCEPTION, 12 entries, all in the dominance ladder (Case.weak_rows_allowed lists them and says why they cannot hold): dk at
  p_hot 0.99 in bf16 and at p_hot 0.999, dq at p_hot 0.999 with d = 32.  They are held to: at least 80 % of the affected rows at 2x
  the bound and the median row at 4x.  Every other tensor of those cases is held to the rule in every row."""
import pytest
import torch

from tests import transformer_helpers as T
from tests import window_attention_cases as W
from tests.test_window_attention_gpu import reference

F64 = torch.float64


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("window", [0, 1, 7, 64, None, 203])
@pytest.mark.parametrize("softcap,alibi", [(None, False), (30.0, False), (None, True), (2.0, True)])
def test_dense_reference_matches_the_two_existing_restatements(window, softcap, alibi):
    N, H, d, batch = 77, 2, 32, 2
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(batch * N, H * d, generator=g, dtype=F64) for _ in range(3))
    slopes = W.alibi_slopes(H) if alibi else None
    out, lse = W.dense_reference(2 * q, k, v, H, window, batch, softcap, slopes)
    want, want_lse = reference(2 * q, k, v, H, window, batch, softcap, slopes, chunk=32)
    band = T.band_attention(2 * q, k, v, H, window, batch, softcap, slopes, chunk=50)
    assert float((out - want).abs().max()) <= 1e-12 and float((lse - want_lse).abs().max()) <= 1e-12
    assert float((out - band).abs().max()) <= 1e-12
    do = torch.randn(batch * N, H * d, generator=g, dtype=F64)
    a = W.autograd_of(lambda x, y, z: W.dense_reference(x, y, z, H, window, batch, softcap, slopes)[0], q, k, v, do, F64)
    b = W.autograd_of(lambda x, y, z: T.band_attention(x, y, z, H, window, batch, softcap, slopes), q, k, v, do, F64)
    for n, x, y in zip(W.NAMES, a, b):
        assert float((x - y).abs().max()) <= 1e-12, n


def test_excluded_pairs_leave_the_band_and_nothing_else_does():
    """Excluding every pair at distance w is the window w - 1; excluding one pair changes that query's row only."""
    N, H, d, w = 50, 2, 32, 9
    g = torch.Generator().manual_seed(6)
    q, k, v = (torch.randn(2 * N, H * d, generator=g, dtype=F64) for _ in range(3))
    edge = torch.cat([W.hot_pairs(N, w), W.hot_pairs(N, -w)])
    a = W.dense_reference(q, k, v, H, w, 2, exclude=edge)
    b = W.dense_reference(q, k, v, H, w - 1, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    full = W.dense_reference(q, k, v, H, w, 2)
    one = W.dense_reference(q, k, v, H, w, 2, exclude=torch.tensor([[20, 23]]))
    changed = (one[0] != full[0]).any(1)
    assert changed.nonzero().flatten().tolist() == [20, N + 20]
    assert W.hot_pairs(5, -2).tolist() == [[2, 0], [3, 1], [4, 2]] and W.hot_pairs(5, 4).tolist() == [[0, 4]]


def test_the_case_lists_are_the_ones_the_kernels_branch_on():
    assert len({c.id for c in W.ALL_CASES}) == len(W.ALL_CASES)
    assert [c.delta for c in W.LADDER if c.window == 1] == [-1, 0, 1]
    assert [c.delta for c in W.LADDER if c.window == 64] == [-64, -63, -1, 0, 1, 63, 64]
    assert all(abs(c.delta) <= c.window < c.N - 1 for c in W.ALL_CASES if c.family != "unbounded")  # a bounded band holding the hot key
    assert all(c.window is None or c.window >= c.N - 1 for c in W.UNBOUNDED)
    assert {(c.d, c.dtype, c.N) for c in W.HEAD_DIMS} == {(d, t, n) for d in (64, 128) for t in (W.BF16, W.F16) for n in (200, 130)}
    assert len(W.DOMINANCE) == 24 and len(W.FANCY) == 12 and {c.d for c in W.FP32_ANCHORS} == {32, 64, 128}


def test_indicator_values_read_out_one_column_of_p():
    N, H, d, w, j = 40, 2, 32, 5, 16
    g = torch.Generator().manual_seed(7)
    q, k = (torch.randn(2 * N, H * d, generator=g, dtype=F64) for _ in range(2))
    v = W.indicator_values(N, H * d, (None, j), F64)
    out, lse = W.dense_reference(q, k, v, H, w, 2)
    inside = (torch.arange(N) - j).abs() <= w
    assert (out[:N] == 0).all() and (out[N:][~inside] == 0).all() and (out[N:][inside] > 0).all()
    s = (q[N:].view(N, H, d) * k[N + j].view(1, H, d)).sum(-1) / d ** 0.5
    assert float((out[N:].view(N, H, d)[inside][..., 0] - torch.exp(s - lse[N:])[inside]).abs().max()) <= 1e-12


def sensitivity(case):
    """[(tensor, min, median, share of rows at 2x or more)] over the affected rows of |reference without the hot pairs - reference| / the GPU test's bound."""
    q, k, v, do = W.hot_inputs(case)
    N, H, batch, dtype = case.N, case.H, case.batch, case.dtype
    pairs = W.hot_pairs(N, case.delta)
    lses = {}

    def ref(exclude):
        def fn(a, b, c):
            out, lse = W.dense_reference(a, b, c, H, case.window, batch, case.softcap, case.slopes, exclude=exclude)
            lses[exclude is None] = lse.detach()
            return out
        return fn

    want = W.autograd_of(ref(None), q, k, v, do, F64)
    lost = W.autograd_of(ref(pairs), q, k, v, do, F64)
    eager = None
    if dtype != W.F32:
        eager = W.autograd_of(lambda a, b, c: T.band_attention(a, b, c, H, case.window, batch, case.softcap, case.slopes), q, k, v, do, dtype)
    queries, keys = W.all_rows(pairs[:, 0], N, batch), W.all_rows(pairs[:, 1], N, batch)
    report = []
    for i, n in enumerate(W.NAMES):
        bound = W.backward_bound(want[i], None if eager is None else eager[i], dtype)
        if n == "out":
            bound = max(bound, W.forward_bound(want[i], dtype))
        rows = keys if n in ("dk", "dv") else queries
        diff = (lost[i] - want[i]).abs().amax(-1)[rows]  # [affected rows]
        report.append((n, float(diff.min()) / bound, float(diff.median()) / bound, float((diff >= 2 * bound).double().mean())))
    bound = W.forward_bound(lses[True], dtype)
    diff = (lses[False] - lses[True]).abs().amax(-1)[queries]
    report.append(("lse", float(diff.min()) / bound, float(diff.median()) / bound, float((diff >= 2 * bound).double().mean())))
    return report


@pytest.mark.parametrize("case", W.ALL_CASES, ids=_ids(W.ALL_CASES))
def test_hot_key_probability_and_sensitivity(case):
    q, k, _, _ = W.hot_inputs(case)
    p_hot = W.hot_probability(case, q, k)
    med = p_hot.median(0).values
    print(f"{case.id}: c {W.tune_c(case).tolist()} p_hot median {med.tolist()} min {float(p_hot.min()):.3f}")
    assert bool(((med >= case.p_range[0]) & (med <= case.p_range[1])).all()), f"{case.id}: median p_hot {med.tolist()} outside {case.p_range}"
    report = sensitivity(case)
    print(f"{case.id}: lost-key difference / bound, min (median, share of rows at 2x): "
          + ", ".join(f"{n} {a:.1f} ({b:.1f}, {f:.2f})" for n, a, b, f in report))
    assert set(case.weak_rows_allowed) <= {"dq", "dk"}
    weak = [f"{n}: {a:.2f}x" for n, a, _, _ in report if n not in case.weak_rows_allowed and not a >= 2.0]
    weak += [f"{n}: median {b:.1f}x, {100 * f:.0f} % of the rows at 2x" for n, _, b, f in report
             if n in case.weak_rows_allowed and not (b >= 4.0 and f >= 0.8)]
    assert not weak, f"{case.id}: a kernel that loses the hot key could pass: " + "; ".join(weak)


def test_the_exception_is_twelve_entries_of_the_dominance_ladder():
    entries = [(c.id, n) for c in W.ALL_CASES for n in c.weak_rows_allowed]
    assert len(entries) == 12 and all(c.family == "dominance" and c.p_target >= 0.99 for c in W.ALL_CASES if c.weak_rows_allowed)
    assert sum(n == "dk" for _, n in entries) == 10 and sum(n == "dq" for _, n in entries) == 2
