"""Shared pieces of the Transformer processor tests: the seeded parameter / input draws of tests/golden/make_golden_transformer.py and a
plain-torch restatement of the reference's TransformerProcessor (layers/processor.py:204-316, block.py:123-196, attention.py:41-262)."""
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = 642


def fill(module, seed: int, scale: float = 0.1) -> float:
    """Every parameter drawn from N(0, scale^2) (LayerNorm weights 1 + N(0, scale^2)) in state_dict order; returns their sum."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    with torch.no_grad():
        for name, p in module.state_dict().items():
            if not torch.is_floating_point(p):
                continue
            v = scale * torch.randn(p.shape, generator=g, dtype=torch.float32)
            if "norm" in name and name.endswith("weight"):
                v = v + 1.0
            p.copy_(v)
            total += float(v.double().sum())
    return total


def inputs(seed: int, rows: int, channels: int) -> torch.Tensor:
    return torch.randn(rows, channels, generator=torch.Generator().manual_seed(seed))


def processor(kw: dict, layer_kernels=None):
    from anemoi_core_amd.layers.processor import TransformerProcessor

    kw = dict(dict(num_layers=2, num_chunks=1, mlp_hidden_ratio=4, dropout_p=0.0), **kw)
    return TransformerProcessor(layer_kernels=layer_kernels, attention_implementation="scaled_dot_product_attention", **kw)


def band_attention(q, k, v, H, window, batch=1, softcap=None, slopes=None, chunk=1024):
    """softmax(q k^T / sqrt(d) [capped, - slope |i - j|], masked to |i - j| <= window) v, per sequence of the batch, in q's dtype;
    query chunks x their band of keys, so that a 10 242-row sequence never forms the whole score matrix."""
    rows, A = q.shape
    N, d = rows // batch, A // H
    w = N if window is None or window < 0 else window
    out = torch.empty_like(q)
    for b in range(batch):
        qb, kb, vb = (t[b * N:(b + 1) * N].reshape(N, H, d).transpose(0, 1) for t in (q, k, v))
        for a in range(0, N, chunk):
            e = min(N, a + chunk)
            lo, hi = max(0, a - w), min(N, e + w + 1)
            i = torch.arange(a, e, device=q.device)[:, None]
            j = torch.arange(lo, hi, device=q.device)[None, :]
            s = torch.einsum("hqd,hkd->hqk", qb[:, a:e], kb[:, lo:hi]) / math.sqrt(d)
            if softcap:
                s = softcap * torch.tanh(s / softcap)
            if slopes is not None:
                s = s - slopes.to(s)[:, None, None] * (i - j).abs()
            s = s.masked_fill(((i - j).abs() > w)[None], float("-inf"))
            out[b * N + a:b * N + e] = torch.einsum("hqk,hkd->hqd", torch.softmax(s, -1), vb[:, lo:hi]).transpose(0, 1).reshape(e - a, A)
    return out


def _ln(x, w, b=None, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)


def processor_forward(p: dict, prefix: str, x, num_layers: int, num_heads: int, window, batch: int = 1, qk_norm: bool = False):
    """The reference's TransformerProcessor, restated: per block x = x + proj(MHSA(LN_att(x))), x = x + MLP(LN_mlp(x))."""
    for layer in range(num_layers):
        q_ = f"{prefix}proc.{layer}."
        h = _ln(x, p[q_ + "layer_norm_attention.weight"], p[q_ + "layer_norm_attention.bias"])
        q, k, v = (h @ p[f"{q_}attention.lin_{n}.weight"].T for n in "qkv")
        if qk_norm:
            d = q.shape[1] // num_heads
            q = _ln(q.reshape(-1, num_heads, d), p[q_ + "attention.q_norm.weight"]).reshape(q.shape)
            k = _ln(k.reshape(-1, num_heads, d), p[q_ + "attention.k_norm.weight"]).reshape(k.shape)
        o = band_attention(q, k, v, num_heads, window, batch)
        x = x + o @ p[q_ + "attention.projection.weight"].T + p[q_ + "attention.projection.bias"]
        h = _ln(x, p[q_ + "layer_norm_mlp.weight"], p[q_ + "layer_norm_mlp.bias"])
        h = torch.nn.functional.gelu(h @ p[q_ + "mlp.mlp.0.weight"].T + p[q_ + "mlp.mlp.0.bias"])
        x = x + h @ p[q_ + "mlp.mlp.2.weight"].T + p[q_ + "mlp.mlp.2.bias"]
    return x


def tiny_model(case: dict):
    """This package's AnemoiModelEncProcDec of the fixture's tiny model (o8 -> res 3, 64 channels, GraphTransformer mappers, a 2-layer
    TransformerProcessor), its graph without hidden -> hidden edges, parameters drawn as the generator drew them."""
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices, model_config

    g = build_synthetic_graph("o8", 3, processor_edges=False)
    cfg = model_config("transformer", 64, 2, 2, 8, window_size=case["window"])
    cfg["model"]["processor"]["attention_implementation"] = "scaled_dot_product_attention"
    model = AnemoiModelEncProcDec(model_config=cfg, data_indices=make_data_indices(case["n_vars"], case["n_vars"]), statistics={"data": None},
                                  n_step_input=case["n_step"], n_step_output=1, graph_data=g).eval()
    psum = fill(model, case["param_seed"])
    x = torch.randn(1, case["n_step"], 1, g.num_data, case["n_vars"], generator=torch.Generator().manual_seed(case["input_seed"]))
    return model, g, x, psum


def model_forward(p: dict, graph, x, num_heads: int, num_layers: int, window):
    """AnemoiModelEncProcDec.forward of the Transformer model (GraphTransformer mappers, TransformerProcessor, no hidden -> hidden edges)
    for one dataset "data", batch 1, ensemble 1, one output step: oracle.gt_oracle's mapper functions around ``processor_forward``,
    the latent skip as an add and the SkipConnection(step=-1) residual (oracle.gt_oracle.enc_proc_dec_forward with the processor
    replaced)."""
    from oracle import gt_oracle as O

    t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a)  # noqa: E731
    B, T, E, N, V = x.shape
    assert B == 1 and E == 1
    x_skip = x[:, -1, ...]
    x_data_latent = torch.cat([x.permute(0, 2, 3, 1, 4).reshape(N, T * V), O.node_attributes(p, "data")], dim=-1)
    x_hidden_latent = O.node_attributes(p, "hidden")
    enc_ea = O.provider_edge_attr(p, "encoder_graph_provider.data", t(graph.enc_edge_attr))
    dec_ea = O.provider_edge_attr(p, "decoder_graph_provider.data", t(graph.dec_edge_attr))
    enc_ei, dec_ei = t(graph.enc_edge_index).long(), t(graph.dec_edge_index).long()
    x_latent = O.gt_forward_mapper(p, "encoder.data", x_data_latent, x_hidden_latent, enc_ea, enc_ei, num_heads)
    x_proc = processor_forward(p, "processor.", x_latent, num_layers, num_heads, window) + x_latent
    x_out = O.gt_backward_mapper(p, "decoder.data", x_proc, x_data_latent, dec_ea, dec_ei, num_heads)
    x_out = x_out.view(B, E, N, 1, -1).permute(0, 3, 1, 2, 4).clone()
    n_prog = x_out.shape[-1]
    x_out[..., :n_prog] += x_skip.unsqueeze(1)[..., :n_prog]
    return x_out
