"""ops.window_attention (csrc/window_attention.hip) against a float64 dense-masked restatement of the reference's attention
(models/src/anemoi/models/layers/attention.py: the SDPA band mask 283-316 and flash-attention's window / softcap / ALiBi 362-520).

Tolerances, s = max(1, max |ref|): fp32 max |err| <= 1e-5 * s.  16-bit: q, k, v are rounded first and the restatement runs on the
rounded values; max |err| <= 2e-2 * s and mean |err| <= 5e-3."""
import math

import pytest
import torch

from anemoi_core_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def alibi_slopes(num_heads: int) -> torch.Tensor:
    """get_alibi_slopes of the reference (layers/attention.py:545-565), restated."""
    n = 2 ** math.floor(math.log2(num_heads))
    s = torch.pow(2 ** (-8 / n), torch.arange(1, 1 + n, dtype=torch.float64))
    if n < num_heads:
        s = torch.cat([s, torch.pow(2 ** (-4 / n), torch.arange(1, 1 + 2 * (num_heads - n), 2, dtype=torch.float64))])
    return s


def reference(q, k, v, H, window, batch=1, softcap=None, slopes=None, chunk=512):
    """float64 restatement, query chunks x their band of keys with the dense boolean mask |i - j| <= w.  Returns (out, lse)."""
    q, k, v = (t.to(torch.float64) for t in (q, k, v))
    rows, A = q.shape
    N, d = rows // batch, A // H
    w = N if window is None or window < 0 else window
    out = torch.empty_like(q)
    lse = torch.empty(rows, H, dtype=torch.float64, device=q.device)
    for b in range(batch):
        qb, kb, vb = (t[b * N:(b + 1) * N].view(N, H, d).transpose(0, 1) for t in (q, k, v))  # [H, N, d]
        for a in range(0, N, chunk):
            e = min(N, a + chunk)
            lo, hi = max(0, a - w), min(N, e + w + 1)
            i = torch.arange(a, e, device=q.device)[:, None]
            j = torch.arange(lo, hi, device=q.device)[None, :]
            s = torch.einsum("hqd,hkd->hqk", qb[:, a:e], kb[:, lo:hi]) / math.sqrt(d)
            if softcap:
                s = softcap * torch.tanh(s / softcap)
            if slopes is not None:
                s = s - slopes.to(q.device)[:, None, None] * (i - j).abs()
            s = s.masked_fill(((i - j).abs() > w)[None], float("-inf"))
            lse[b * N + a:b * N + e] = torch.logsumexp(s, -1).transpose(0, 1)
            o = torch.einsum("hqk,hkd->hqd", torch.softmax(s, -1), vb[:, lo:hi])
            out[b * N + a:b * N + e] = o.transpose(0, 1).reshape(e - a, A)
    return out, lse


def _inputs(rows, A, dtype, layout, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if layout == "slices":  # column slices of ONE [rows, 3A] projection buffer, read in place
        buf = torch.randn(rows, 3 * A, generator=g).to(DEV, dtype)
        return buf[:, :A], buf[:, A:2 * A], buf[:, 2 * A:]
    return tuple(torch.randn(rows, A, generator=g).to(DEV, dtype) for _ in range(3))


def _check(got, want, dtype, name):
    assert torch.isfinite(got).all(), name
    err = (got.double() - want).abs()
    s = max(1.0, float(want.abs().max()))
    if dtype == torch.float32:
        assert float(err.max()) <= 1e-5 * s, f"{name}: fp32 max err {float(err.max()):.3e} (s {s:.2f})"
    else:
        assert float(err.max()) <= 2e-2 * s and float(err.mean()) <= 5e-3, f"{name}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}"


def _run(N, window, d, H, batch, dtype, softcap=None, alibi=False, layout="slices", seed=0):
    A = H * d
    q, k, v = _inputs(batch * N, A, dtype, layout, seed)
    slopes = alibi_slopes(H) if alibi else None
    out, lse = ops.window_attention(q, k, v, H, window, softcap=softcap, batch_size=batch, return_lse=True,
                                    alibi_slopes=None if slopes is None else slopes.float().to(DEV))
    want, want_lse = reference(q, k, v, H, window, batch, softcap, slopes)
    name = f"N={N} w={window} d={d} H={H} B={batch} {dtype} cap={softcap} alibi={alibi} {layout}"
    assert out.dtype == dtype and out.shape == q.shape
    _check(out, want, dtype, name)
    lse_tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert float((lse.double() - want_lse).abs().max()) <= lse_tol * max(1.0, float(want_lse.abs().max())), f"{name}: lse"


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 642, 10242])
@pytest.mark.parametrize("window", [0, 1, 7, 64, 512, None, "ge_n"])
def test_shapes_and_windows_bf16(N, window):
    _run(N, N + 3 if window == "ge_n" else window, 32, 2, 1, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("H,batch", [(2, 3), (16, 1)])
@pytest.mark.parametrize("N,window", [(65, 7), (642, 64)])
def test_dtypes_heads_batches(dtype, d, H, batch, N, window):
    _run(N, window, d, H, batch, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("softcap,alibi", [(30.0, False), (None, True), (30.0, True)])
@pytest.mark.parametrize("d", [32, 128])
def test_softcap_and_alibi(dtype, softcap, alibi, d):
    """Softcap and ALiBi exist only on the reference's flash-attention backend, which does not run without flash-attn: the check is
    against the restatement above (scores capped, then the slope times |i - j| subtracted)."""
    _run(642, 64, d, 16, 1, dtype, softcap=softcap, alibi=alibi, seed=1)
    # larger scores so that the cap bites
    A = 16 * d
    q, k, v = _inputs(200, A, dtype, "separate", seed=2)
    q = (q.float() * 4).to(dtype)
    out = ops.window_attention(q, k, v, 16, 17, softcap=softcap, alibi_slopes=alibi_slopes(16).float().to(DEV) if alibi else None)
    _check(out, reference(q, k, v, 16, 17, 1, softcap, alibi_slopes(16) if alibi else None)[0], dtype, "capped")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("window", [2**31 - 1, 2**31 - 70, 2**40])
def test_huge_windows_mean_unbounded(dtype, window):
    """A window near or beyond INT32_MAX (a config's way of saying 'unbounded') attends every key: no band edge overflows."""
    _run(700, window, 32, 2, 2, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,window", [(10242, 512), (10242, None), (4000, 7)])
def test_large(dtype, N, window):
    _run(N, window, 32, 16, 1, dtype, layout="separate")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window", [0, 7, 64, 100])
def test_keys_outside_the_window_contribute_exact_zeros(dtype, window):
    """1e4 written into the K / V rows just outside the windows of a set of queries (and into the first rows of the NEXT sequence of a
    batch) leaves those queries' outputs bit-identical."""
    N, H, d, batch = 1500, 2, 64, 2
    A = H * d
    q, k, v = _inputs(batch * N, A, dtype, "separate", seed=3)
    base = ops.window_attention(q, k, v, H, window, batch_size=batch)
    step = 2 * window + 3
    qs = torch.arange(window + 1, N - window - 1, step, device=DEV)
    bad = torch.cat([qs - window - 1, qs + window + 1])
    k2, v2 = k.clone(), v.clone()
    k2[bad], v2[bad] = 1e4, 1e4
    got = ops.window_attention(q, k2, v2, H, window, batch_size=batch)
    assert torch.equal(got[qs], base[qs])
    k3, v3 = k.clone(), v.clone()
    k3[N:N + window + 1], v3[N:N + window + 1] = 1e4, 1e4  # sequence 2's first rows: outside every window of sequence 1
    got = ops.window_attention(q, k3, v3, H, window, batch_size=batch)
    assert torch.equal(got[:N], base[:N])


@pytest.mark.parametrize("d", [16, 48, 256])
def test_unsupported_head_dim_raises(d):
    q = torch.zeros(64, 2 * d, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="supported"):
        ops.window_attention(q, q, q, 2, 8)


def test_hipgraph_capture_replays_bit_equal():
    q, k, v = _inputs(2048, 512, torch.bfloat16, "slices", seed=4)
    eager = ops.window_attention(q, k, v, 16, 64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.window_attention(q, k, v, 16, 64)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.window_attention(q, k, v, 16, 64)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_ctypes_path_matches_the_torch_op(monkeypatch):
    from anemoi_core_amd import _ext

    q, k, v = _inputs(700, 256, torch.bfloat16, "slices", seed=5)
    a = ops.window_attention(q, k, v, 8, 33, return_lse=True)
    monkeypatch.setattr(_ext, "ops", lambda: None)
    b = ops.window_attention(q, k, v, 8, 33, return_lse=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
