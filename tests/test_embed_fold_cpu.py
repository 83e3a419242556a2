"""Host side of the encoder's composed source projection (ops.compose_embedding_projection): with fp32 weights and fp64 evaluation,

    rstd (W_c x + u - mean s) + d,      (mean, rstd): the LayerNorm statistics of e = W_emb x + b_emb

reproduces Linear -> LayerNorm -> Linear to 1e-5 of the output's scale - rows of constants and rows with a common offset of 100 x their
spread included - and the packed images are what the kernel expects (columns zero-padded to a multiple of 64)."""
import pytest
import torch

from anemoi_core_amd import ops

D = 512
EPS = 1e-5


def unpack_weight_frag(img: torch.Tensor, O: int, K: int) -> torch.Tensor:
    """The inverse of ops.pack_weight_frag."""
    return img.reshape(O // 64, K // 32, 4, 4, 16, 8).permute(0, 2, 4, 1, 3, 5).reshape(O, K)


def make_weights(K: int, out: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(w_emb=r(D, K) / K ** 0.5, b_emb=0.1 * r(D), gamma=1.0 + 0.1 * r(D), beta=0.1 * r(D), w_proj=r(out, D) / D ** 0.5, b_proj=0.1 * r(out))


def make_rows(n: int, K: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, K, generator=g)
    x[1] = 0.75                                   # a row of constants
    x[2] = 0.0
    x[3] = 100.0 * x[3].std() + x[3]              # a common offset of 100 x the row's spread
    x[4] = -100.0 * x[4].std() + x[4]
    return x


@pytest.mark.parametrize("out", [512, 1024, 2048])
@pytest.mark.parametrize("K", [64, 184, 192, 256])
def test_composed_form_reproduces_linear_layernorm_linear(K, out):
    p = make_weights(K, out, seed=K + out)
    x = make_rows(24, K, seed=7)
    we_img, wc_img, vec = ops.compose_embedding_projection(p["w_emb"], p["b_emb"], p["w_proj"], p["b_proj"], p["gamma"], p["beta"])
    kp = (K + 63) // 64 * 64
    assert we_img.shape == (D * kp,) and wc_img.shape == (out * kp,) and we_img.dtype == wc_img.dtype == torch.float32
    assert vec.shape == (D + 3 * out,) and vec.dtype == torch.float32
    we, wc = unpack_weight_frag(we_img, D, kp), unpack_weight_frag(wc_img, out, kp)
    assert torch.equal(we[:, :K], p["w_emb"]) and not we[:, K:].any() and not wc[:, K:].any()
    be, u, s, d = (t.double() for t in vec.split([D, out, out, out]))
    assert torch.equal(be.float(), p["b_emb"])

    x64 = x.double()
    e = x64 @ we[:, :K].double().T + be
    mean, var = e.mean(1, keepdim=True), e.var(1, unbiased=False, keepdim=True)
    got = (var + EPS).rsqrt() * (x64 @ wc[:, :K].double().T + u - mean * s) + d

    q = {k: v.double() for k, v in p.items()}
    e_ref = torch.nn.functional.linear(x64, q["w_emb"], q["b_emb"])
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(e_ref, (D,), q["gamma"], q["beta"], EPS), q["w_proj"], q["b_proj"])
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"K={K} out={out}: max |composed - chain| = {err:.3e}, output scale {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= 1e-5 * scale


def test_composition_without_biases_and_in_16_bit():
    """Missing biases are zeros; with 16-bit weights the composition still runs in fp32 and only W_c is rounded, once."""
    p = make_weights(192, 1024, seed=3)
    we_img, wc_img, vec = ops.compose_embedding_projection(p["w_emb"], None, p["w_proj"], None, p["gamma"], None)
    be, u, s, d = vec.split([D, 1024, 1024, 1024])
    assert not be.any() and not u.any() and not d.any()
    assert torch.allclose(s, (p["w_proj"] * p["gamma"]).sum(1))
    h = {k: v.to(torch.bfloat16) for k, v in p.items()}
    we_img, wc_img, vec = ops.compose_embedding_projection(h["w_emb"], h["b_emb"], h["w_proj"], h["b_proj"], h["gamma"], h["beta"])
    assert we_img.dtype == wc_img.dtype == torch.bfloat16 and vec.dtype == torch.float32
    wg = h["w_proj"].float() * h["gamma"].float()
    assert torch.equal(unpack_weight_frag(wc_img, 1024, 192), (wg @ h["w_emb"].float()).to(torch.bfloat16))
    assert torch.equal(vec[D:D + 1024], wg @ h["b_emb"].float())


def test_cpu_rows_are_refused():
    p = make_weights(192, 1024, seed=3)
    ops_ = ops.compose_embedding_projection(p["w_emb"].bfloat16(), p["b_emb"].bfloat16(), p["w_proj"].bfloat16(), p["b_proj"].bfloat16(),
                                            p["gamma"].bfloat16(), p["beta"].bfloat16())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gt_embed_fold(torch.zeros(4, 192, dtype=torch.bfloat16), *ops_, 1024, EPS)
