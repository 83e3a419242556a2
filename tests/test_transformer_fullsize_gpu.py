"""The Transformer model and processor at the sizes where the row-chain routes apply, against the restatement
(tests/transformer_helpers.py: oracle.gt_oracle's mapper functions around the processor restatement, itself checked against the
reference by tests/test_transformer_cpu.py), with the bounds of tests/test_fullsize_parity_gpu._check; and the attention module's
own forward (the reference's signature)."""
import pytest
import torch

from anemoi_core_amd import ops
from anemoi_core_amd.distributed.shapes import GraphShardInfo
from tests import transformer_helpers as T
from tests.test_fullsize_parity_gpu import _check

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rounded(p: dict, dtype) -> dict:
    return {k: (v.to(dtype).float() if v.is_floating_point() else v) for k, v in p.items()}


def test_o96_res5_model_bf16_against_the_restatement(monkeypatch):
    """O96 -> res 5 (10 242 hidden rows), 512 channels, 16 heads, window 512, 2 processor layers, bf16: encoder, the processor's chain
    tails (block 0 hands block 1 its q|k|v), the latent skip and the decoder, against the restatement on the rounded values."""
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices, model_config

    g = build_synthetic_graph("o96", 5, processor_edges=False)
    n_vars, n_step, dtype = 84, 2, torch.bfloat16
    torch.manual_seed(0)
    model = AnemoiModelEncProcDec(model_config=model_config("transformer", 512, 2, 16, 8, window_size=512),
                                  data_indices=make_data_indices(n_vars, n_vars), statistics={"data": None}, n_step_input=n_step,
                                  n_step_output=1, graph_data=g).eval()
    T.fill(model, 11, scale=0.03)
    x = torch.randn(1, n_step, 1, g.num_data, n_vars, generator=torch.Generator().manual_seed(12))
    model = model.to(DEV, dtype)
    calls = []
    real = ops.gt_layer_chain2
    monkeypatch.setattr(ops, "gt_layer_chain2", lambda *a, **k: calls.append(k.get("q_out_features")) or real(*a, **k))
    with torch.inference_mode():
        got = model({"data": x.to(DEV, dtype)})["data"].float().cpu()
    assert calls.count(1536) == 1  # processor block 0 handed block 1 its q|k|v (the mappers' tails run on the chain too)
    p = _rounded({k: v.float().cpu() for k, v in model.state_dict().items()}, dtype)
    with torch.no_grad():
        want = T.model_forward(p, g, x.to(dtype).float(), 16, 2, 512)
    assert got.shape == want.shape == (1, 1, 1, g.num_data, n_vars)
    _check("transformer model O96 -> res 5 bf16", got, want, dtype)


def test_cluster_route_at_res4_bf16(monkeypatch):
    """512 channels below the chain's 4 096-row gate (2 562 rows, res 4): the cluster chain with the next block's 1 536-column q|k|v."""
    calls = []
    real = ops.gt_cluster_chain
    monkeypatch.setattr(ops, "gt_cluster_chain", lambda *a, **k: calls.append(k.get("q_out_features")) or real(*a, **k))
    kw = dict(num_channels=512, num_heads=16, window_size=512)
    proc = T.processor(kw).eval()
    T.fill(proc, 13, scale=0.03)
    x = T.inputs(14, 2562, 512)
    proc = proc.to(DEV, torch.bfloat16)
    with torch.no_grad():
        y = proc(x.to(DEV, torch.bfloat16), 1, GraphShardInfo(nodes=None)).float().cpu()
    assert calls == [1536, 0]
    p = {k: v.float().cpu() for k, v in proc.state_dict().items()}
    _check("transformer cluster route", y, T.processor_forward(p, "", x.to(torch.bfloat16).float(), 2, 16, 512), torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("opts", [dict(), dict(qk_norm=True, attn_channels=256), dict(softcap=20.0, use_alibi_slopes=True)])
def test_attention_module_forward(dtype, opts):
    """MultiHeadSelfAttention(x, shard_info, batch_size) as the reference calls it: projections, window attention, output projection."""
    from anemoi_core_amd.layers.attention import MultiHeadSelfAttention
    from anemoi_core_amd.layers.utils import load_layer_kernels

    H, D, w, batch = 4, 128, 40, 2
    att = MultiHeadSelfAttention(num_heads=H, embed_dim=D, layer_kernels=load_layer_kernels(None), window_size=w, **opts).eval()
    T.fill(att, 15)
    x = T.inputs(16, batch * 300, D)
    with torch.no_grad():
        y = att.to(DEV, dtype)(x.to(DEV, dtype), GraphShardInfo(nodes=None), batch).float().cpu()
    p = {k: v.float().cpu() for k, v in att.state_dict().items()}
    xr = x.to(dtype).float()
    q, k, v = (xr @ p[f"lin_{n}.weight"].T for n in "qkv")
    A = q.shape[1]
    if opts.get("qk_norm"):
        q = T._ln(q.reshape(-1, H, A // H), p["q_norm.weight"]).reshape(q.shape)
        k = T._ln(k.reshape(-1, H, A // H), p["k_norm.weight"]).reshape(k.shape)
    slopes = att.alibi_slopes.double() if opts.get("use_alibi_slopes") else None
    o = T.band_attention(q.double(), k.double(), v.double(), H, w, batch, opts.get("softcap"), slopes).float()
    want = o @ p["projection.weight"].T + p["projection.bias"]
    _check(f"attention module {opts}", y, want, dtype)
