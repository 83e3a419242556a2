"""The window attention's backward (csrc/window_attention_bwd.hip) through ``ops.window_attention`` + ``.backward()``, against float64
autograd of ``tests/transformer_helpers.band_attention`` on the inputs after they are rounded to the test dtype, with a seeded d_out.

Tolerances, per tensor (out, dq, dk, dv):
  fp32:   max |got - want| <= 2e-5 * max |want| + 1e-6 - the kernel-level autograd bound of test_linear_and_layernorm_autograd_vs_torch.
  16-bit: no number fixed in advance.  Eager torch autograd of ``band_attention`` in the 16-bit dtype runs on the same inputs; its max
          error against the float64 reference is e_eager, and the kernel must satisfy max err <= 2 * e_eager.  The factor 2: the kernel
          rounds P and dS to 16 bits at other points than eager torch rounds its intermediates, while it accumulates in fp32.
The errors measured on the MI355X are in DESIGN.md."""
import pytest
import torch

from anemoi_core_amd import autograd as ag
from anemoi_core_amd import ops
from tests import transformer_helpers as T
from tests.test_window_attention_gpu import alibi_slopes

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("out", "dq", "dk", "dv")


def _draw(rows, A, dtype, seed, qscale=1.0):
    """q, k, v, d_out on the device in ``dtype`` (q scaled before it is rounded)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(rows, A, generator=g) for _ in range(4))
    return tuple(t.to(DEV, dtype) for t in (q * qscale, k, v, do))


def _autograd(fn, q, k, v, do, dtype):
    """(out, dq, dk, dv) of ``fn`` on fresh leaves of ``dtype``."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    out = fn(*leaves)
    out.backward(do.to(dtype))
    return (out.detach(), *(t.grad for t in leaves))


def _ours(q, k, v, do, H, window, batch, softcap, slopes):
    fn = lambda a, b, c: ops.window_attention(a, b, c, H, window, softcap=softcap, batch_size=batch,  # noqa: E731
                                              alibi_slopes=None if slopes is None else slopes.float().to(DEV))
    return _autograd(fn, q, k, v, do, q.dtype)


def _band(H, window, batch, softcap, slopes):
    sl = None if slopes is None else slopes.to(DEV)
    return lambda a, b, c: T.band_attention(a, b, c, H, window, batch, softcap, sl)


def _compare(got, q, k, v, do, H, window, batch, softcap, slopes, name):
    dtype = q.dtype
    want = _autograd(_band(H, window, batch, softcap, slopes), q, k, v, do, torch.float64)
    eager = None if dtype == torch.float32 else _autograd(_band(H, window, batch, softcap, slopes), q, k, v, do, dtype)
    failures = []
    for i, n in enumerate(NAMES):
        assert got[i].dtype == dtype and got[i].shape == q.shape and torch.isfinite(got[i]).all(), f"{name}: {n}"
        err = float((got[i].double() - want[i]).abs().max())
        if dtype == torch.float32:
            bound = 2e-5 * float(want[i].abs().max()) + 1e-6
        else:
            bound = 2 * float((eager[i].double() - want[i]).abs().max())
        print(f"{name} {n}: err {err:.3e} bound {bound:.3e} max|want| {float(want[i].abs().max()):.3e}")
        if not err <= bound:
            failures.append(f"{n}: err {err:.3e} > {bound:.3e}")
    assert not failures, f"{name}: " + "; ".join(failures)


def _run(N, window, d, H, batch, dtype, softcap=None, alibi=False, seed=0, qscale=1.0):
    q, k, v, do = _draw(batch * N, H * d, dtype, seed, qscale)
    slopes = alibi_slopes(H) if alibi else None
    got = _ours(q, k, v, do, H, window, batch, softcap, slopes)
    _compare(got, q, k, v, do, H, window, batch, softcap, slopes,
             f"N={N} w={window} d={d} H={H} B={batch} {dtype} cap={softcap} alibi={alibi} qscale={qscale}")


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 127, 129, 642])
@pytest.mark.parametrize("window", [0, 1, 7, 63, 64, 65, None, "ge_n"])
def test_shapes_and_windows_bf16(N, window):
    _run(N, N + 3 if window == "ge_n" else window, 32, 2, 1, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("H,batch", [(2, 3), (16, 1)])
@pytest.mark.parametrize("N,window", [(65, 7), (642, 64)])
def test_dtypes_heads_batches(dtype, d, H, batch, N, window):
    _run(N, window, d, H, batch, dtype, seed=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("softcap,alibi", [(30.0, False), (None, True), (30.0, True)])
@pytest.mark.parametrize("d", [32, 128])
def test_softcap_and_alibi(dtype, softcap, alibi, d):
    _run(642, 64, d, 16, 1, dtype, softcap=softcap, alibi=alibi, seed=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [32, 128])
def test_softcap_bites_on_large_scores(dtype, d):
    """q scaled by 4 and a cap of 2: tanh is far from linear, so its derivative 1 - tanh^2 matters."""
    _run(200, 17, d, 16, 1, dtype, softcap=2.0, alibi=True, seed=3, qscale=4.0)
    _run(200, 17, d, 16, 1, dtype, softcap=30.0, seed=3, qscale=4.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("window", [2**31 - 1, 2**40])
def test_huge_windows_mean_unbounded(dtype, window):
    q, k, v, do = _draw(2 * 300, 64, dtype, 4)
    got = _ours(q, k, v, do, 2, window, 2, None, None)
    unbounded = _ours(q, k, v, do, 2, None, 2, None, None)
    for n, a, b in zip(NAMES, got, unbounded):
        assert torch.equal(a, b), n
    _compare(got, q, k, v, do, 2, None, 2, None, None, f"huge window {window} {dtype}")


# -------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_slices_of_one_buffer_get_one_gradient_equal_to_the_three_tensor_case(dtype):
    N, H, d, w = 321, 4, 32, 20
    A = H * d
    q, k, v, do = _draw(N, A, dtype, 5)
    three = _ours(q, k, v, do, H, w, 1, None, None)
    _compare(three, q, k, v, do, H, w, 1, None, None, f"three tensors {dtype}")
    for how in ("slices", "qkv"):
        buf = torch.cat([q, k, v], 1).requires_grad_(True)
        if how == "slices":  # three slice gradients, summed into the leaf by autograd
            out = ops.window_attention(buf[:, :A], buf[:, A:2 * A], buf[:, 2 * A:], H, w)
        else:  # the whole buffer: ONE gradient, written by the kernels
            out = ag.window_attention_qkv(buf, H, w)
        out.backward(do)
        assert torch.equal(out.detach(), three[0]), how
        assert torch.equal(buf.grad, torch.cat(three[1:], 1)), how


def test_non_contiguous_d_out():
    N, H, d, w = 200, 2, 64, 9
    q, k, v, do = _draw(N, H * d, torch.bfloat16, 6)
    want = _ours(q, k, v, do, H, w, 1, None, None)
    wide = torch.zeros(N, 2 * H * d, device=DEV, dtype=torch.bfloat16)
    wide[:, ::2] = do
    leaves = [t.detach().requires_grad_(True) for t in (q, k, v)]
    out = ops.window_attention(*leaves, H, w)
    assert not wide[:, ::2].is_contiguous()
    out.backward(wide[:, ::2])
    for n, a, b in zip(NAMES[1:], (t.grad for t in leaves), want[1:]):
        assert torch.equal(a, b), n


# -------------------------------------------------------------------------------------------- exact zeros
def _grads(q, k, v, do, H, w, batch):
    return _ours(q, k, v, do, H, w, batch, None, None)[1:]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window", [0, 7, 64, 100])
def test_exact_zeros_outside_the_band_and_the_sequence(dtype, window):
    N, H, d, batch = 700, 2, 64, 2
    q, k, v, do = _draw(batch * N, H * d, dtype, 7)
    j = torch.arange(N, device=DEV)
    for i in (0, 333, N - 1):
        one = torch.zeros_like(do)
        one[N + i] = do[N + i]  # query i of sequence 2
        dq, dk, dv = _grads(q, k, v, one, H, window, batch)
        far = (j - i).abs() > window
        assert dk[N:].abs().sum() > 0 or window == 0  # (a single key: the softmax is constant, dq = dk = 0)
        assert dv[N:].abs().sum() > 0
        assert (dk[N:][far] == 0).all() and (dv[N:][far] == 0).all()
        assert (dq[N:][j != i] == 0).all()
        assert (dq[:N] == 0).all() and (dk[:N] == 0).all() and (dv[:N] == 0).all()  # sequence 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window", [0, 7, 64, 100])
def test_rows_outside_the_windows_leave_the_gradients_bit_identical(dtype, window):
    """1e4 in the k / v rows just outside the windows of a set of queries that alone carry d_out, and in the first rows of the NEXT
    sequence: dq of those queries and dk / dv of every key inside their windows stay bit-identical."""
    N, H, d, batch = 1500, 2, 64, 2
    q, k, v, do = _draw(batch * N, H * d, dtype, 8)
    step = 2 * window + 3
    qs = torch.arange(window + 1, N - window - 1, step, device=DEV)
    bad = torch.cat([qs - window - 1, qs + window + 1, torch.arange(N, N + window + 1, device=DEV)])
    sparse = torch.zeros_like(do)
    sparse[qs] = do[qs]
    base = _grads(q, k, v, sparse, H, window, batch)
    k2, v2 = k.clone(), v.clone()
    k2[bad], v2[bad] = 1e4, 1e4
    got = _grads(q, k2, v2, sparse, H, window, batch)
    inside = torch.ones(batch * N, dtype=torch.bool, device=DEV)
    inside[bad] = False
    assert base[0][qs].abs().sum() > 0 or window == 0
    assert torch.equal(got[0][qs], base[0][qs])
    for n, a, b in zip(("dk", "dv"), got[1:], base[1:]):
        assert torch.equal(a[inside], b[inside]), n
        assert (a[bad] == 0).all(), n  # no query with a d_out sees them


# -------------------------------------------------------------------------------------------- determinism
def test_two_backward_calls_are_bit_equal():
    q, k, v, do = _draw(2 * 1000, 512, torch.bfloat16, 9)
    a = _ours(q, k, v, do, 16, 64, 2, 30.0, alibi_slopes(16))
    b = _ours(q, k, v, do, 16, 64, 2, 30.0, alibi_slopes(16))
    for n, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), n


def test_forward_and_backward_captured_in_a_hipgraph_replay_bit_equal():
    N, A, H, w = 2048, 512, 16, 64
    q, k, v, do = _draw(N, A, torch.bfloat16, 10)
    buf = torch.cat([q, k, v], 1).requires_grad_(True)

    def step():
        buf.grad = None
        out = ag.window_attention_qkv(buf, H, w)
        out.backward(do)
        return out

    eager_out = step().detach().clone()
    eager_grad = buf.grad.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    grad = buf.grad
    grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), eager_out) and torch.equal(grad, eager_grad)


# -------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("d", [16, 48, 256])
def test_unsupported_head_dim_raises_under_grad(d):
    q = torch.zeros(64, 2 * d, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    with pytest.raises(ValueError, match="supported"):
        ops.window_attention(q, q, q, 2, 8)
    with pytest.raises(ValueError, match="supported"):
        ag.window_attention_qkv(torch.zeros(64, 6 * d, device=DEV, dtype=torch.bfloat16, requires_grad=True), 2, 8)
    z = torch.zeros(64, 2 * d, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="supported"):
        ops.window_attention_bwd(z, z, z, z, z, torch.zeros(64, 2, device=DEV), 2, 8)


def test_dropout_in_training_mode_raises():
    from anemoi_core_amd.distributed.shapes import GraphShardInfo

    import os

    kw = torch.load(os.path.join(T.GOLDEN, "transformer.pt"), weights_only=False)["w8_d32"]["kw"]
    proc = T.processor(dict(kw, dropout_p=0.1)).to(DEV).train()
    with pytest.raises(NotImplementedError, match="backward kernel"):
        proc(torch.zeros(T.ROWS, 64, device=DEV), 1, GraphShardInfo(nodes=None))


def test_zero_rows():
    z = torch.zeros(0, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    out = ops.window_attention(z, z, z, 2, 8)
    out.sum().backward()
    assert z.grad.shape == (0, 64)
