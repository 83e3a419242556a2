"""ops.gt_embed_fold (csrc/gt_embed_fold.hip: the encoder's source k|v from raw rows with a composed weight) against an fp64 evaluation of
the reference's op order from the same 16-bit operands - e = x W_emb^T + b_emb rounded to the dtype, LayerNorm of the rounded row,
projection, one final rounding - at the row counts around one and two of its 80-row tiles, every K-step count, every pass
count, both dtypes and a row stride wider than the row.

The tolerance is measured: the existing GEMM pair (ops.linear_with_row_stats + ops.linear_ln_folded) runs on the same inputs, and the new
kernel's max and mean error may be at most 2 x the pair's (the new path projects the unrounded e through a weight rounded once more: one
rounding swapped for another, nothing else).  Every ratio is printed before it is asserted."""
import pytest
import torch

from anemoi_core_amd import ops

pytestmark = pytest.mark.gpu

D = 512
EPS = 1e-5
ROWS = 337  # four full tiles and a 17-row tail


def make_case(K: int, out: int, dtype, seed: int, n: int = ROWS):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    p = dict(w_emb=r(D, K) / K ** 0.5, b_emb=0.1 * r(D), gamma=1.0 + 0.1 * r(D), beta=0.1 * r(D), w_proj=r(out, D) / D ** 0.5, b_proj=0.1 * r(out))
    x = r(n, K)
    x[0::7] = 0.75 * torch.arange(1, x[0::7].shape[0] + 1)[:, None]      # constant rows
    x[3::11] = 100.0 * x[3::11].std(dim=1, keepdim=True) + x[3::11]      # a common offset of 100 x the row's spread
    x[5::13] = -100.0 * x[5::13].std(dim=1, keepdim=True) + x[5::13]
    if dtype == torch.float16:
        x = x.clamp(-200.0, 200.0)
    return {k: v.to(dtype).cuda() for k, v in p.items()}, x.to(dtype).cuda()


def reference(p, x):
    """fp64, the reference's op order from the 16-bit operands; rounded once at the end."""
    q = {k: v.double() for k, v in p.items()}
    e = torch.nn.functional.linear(x.double(), q["w_emb"], q["b_emb"]).to(x.dtype).double()
    y = torch.nn.functional.linear(torch.nn.functional.layer_norm(e, (D,), q["gamma"], q["beta"], EPS), q["w_proj"], q["b_proj"])
    return y.to(x.dtype).double()


def pair(p, x):
    """Today's two launches (K zero-padded to a multiple of 64, as the model pads its rows)."""
    pad = (-x.shape[1]) % 64
    xp = torch.nn.functional.pad(x, (0, pad)) if pad else x
    r = ops.linear_with_row_stats(xp.contiguous(), torch.nn.functional.pad(p["w_emb"], (0, pad)).contiguous(), p["b_emb"])
    assert r is not None
    e, stats = r
    ws, d = ops.fold_layer_norm(p["w_proj"], p["b_proj"], p["gamma"], p["beta"])
    y = ops.linear_ln_folded(e, ws.contiguous(), ws.float().sum(1).contiguous(), d.contiguous(), stats, EPS)
    assert y is not None
    return y


def fold(p, x):
    we, wc, vec = ops.compose_embedding_projection(p["w_emb"], p["b_emb"], p["w_proj"], p["b_proj"], p["gamma"], p["beta"])
    y = ops.gt_embed_fold(x, we, wc, vec, p["w_proj"].shape[0], EPS)
    assert y is not None
    return y


def errors(y, ref):
    scale = ref.abs().max().item()
    d = (y.double() - ref).abs()
    return d.max().item() / scale, d.mean().item() / scale


def check(tag, p, x, ref):
    new, old = fold(p, x), pair(p, x)
    torch.cuda.synchronize()
    assert new.shape == ref.shape and torch.isfinite(new.float()).all()
    (nmax, nmean), (omax, omean) = errors(new, ref), errors(old, ref)
    print(f"embed_fold {tag}: max/scale new {nmax:.3e} pair {omax:.3e} ratio {nmax / omax:.2f} | mean/scale new {nmean:.3e} pair {omean:.3e} "
          f"ratio {nmean / omean:.2f}")
    assert nmax <= 2.0 * omax, (tag, nmax, omax)
    assert nmean <= 2.0 * omean, (tag, nmean, omean)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("out", [512, 1024, 2048])
@pytest.mark.parametrize("K", [64, 184, 192, 256])
def test_matches_the_reference_order_as_closely_as_the_gemm_pair(K, out, dtype):
    p, x = make_case(K, out, dtype, seed=K * 7 + out)
    check(f"K={K} out={out} {str(dtype)[6:]} rows={ROWS}", p, x, reference(p, x))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_row_counts_at_the_tile_branch_points(dtype):
    """80-row tiles: below, at and above one tile and two; a row's result does not depend on how many rows follow it."""
    p, x = make_case(192, 1024, dtype, seed=11)
    ref = reference(p, x)
    whole = fold(p, x)
    for n in (1, 79, 80, 81, 159, 160, 161, 337):
        check(f"K=192 out=1024 {str(dtype)[6:]} rows={n}", p, x[:n], ref[:n])
        assert torch.equal(fold(p, x[:n]), whole[:n]), n


def test_row_stride_wider_than_the_row_and_rows_beyond_untouched():
    p, x = make_case(192, 1024, torch.bfloat16, seed=5, n=161)
    wide = torch.full((161, 256), float("nan"), dtype=torch.bfloat16, device="cuda")
    wide[:, :192] = x
    check("K=192 out=1024 bf16 rows=161 ld=256", p, wide[:, :192], reference(p, x))
    assert torch.equal(fold(p, wide[:, :192]), fold(p, x))


def test_shapes_outside_the_kernel_are_refused_not_computed():
    p, x = make_case(192, 1024, torch.bfloat16, seed=5, n=8)
    we, wc, vec = ops.compose_embedding_projection(p["w_emb"], p["b_emb"], p["w_proj"], p["b_proj"], p["gamma"], p["beta"])
    assert ops.gt_embed_fold(x.float(), we, wc, vec, 1024, EPS) is None                                                     # fp32 rows
    assert ops.gt_embed_fold(torch.zeros(8, 264, dtype=torch.bfloat16, device="cuda"), we, wc, vec, 1024, EPS) is None     # K > 256
    assert ops.gt_embed_fold(torch.zeros(8, 196, dtype=torch.bfloat16, device="cuda")[:, :188], we, wc, vec, 1024, EPS) is None  # K % 8
    assert ops.gt_embed_fold(x, we, wc, vec, 768, EPS) is None                                                             # q_out % 512
    with pytest.raises(ValueError, match="fragment-major image"):
        ops.gt_embed_fold(x, we, wc[:-8], vec, 1024, EPS)
    assert ops.gt_embed_fold(x[:0], we, wc, vec, 1024, EPS).shape == (0, 1024)
