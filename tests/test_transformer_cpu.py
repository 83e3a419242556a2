"""TransformerProcessor on the host: module structure against the reference's fixtures (state_dict keys and shapes), the plain-torch
restatement against the reference's outputs, the Transformer block's tail routes, the op's fake kernel and the inference-only guard.
No GPU: nothing is launched."""
import os

import pytest
import torch

import anemoi_core_amd.layers.block as B
from anemoi_core_amd.layers.block import GraphTransformerMapperBlock, TransformerProcessorBlock
from anemoi_core_amd.layers.handoff import Carrier
from anemoi_core_amd.layers.utils import load_layer_kernels
from tests import transformer_helpers as T

FIXTURES = {name: torch.load(os.path.join(T.GOLDEN, name), weights_only=False) for name in ("transformer.pt", "transformer_model.pt")}
CASES = {k: v for f in FIXTURES.values() for k, v in f.items() if k != "model"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_processor_state_dict_matches_the_reference(name):
    case = CASES[name]
    proc = T.processor(case["kw"]).eval()
    assert {k: tuple(v.shape) for k, v in proc.state_dict().items()} == case["keys"]
    psum = T.fill(proc, case["param_seed"])
    assert psum == pytest.approx(case["param_sum"], rel=1e-9)  # the seeded draw is the generator's
    proc.load_state_dict(proc.state_dict(), strict=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    """The restatement the GPU tests compare against, checked against the reference's own outputs (fp32, CPU)."""
    case = CASES[name]
    kw = case["kw"]
    proc = T.processor(kw).eval()
    T.fill(proc, case["param_seed"])
    x = T.inputs(case["input_seed"], case["batch"] * T.ROWS, kw["num_channels"])
    p = {k: v.double() for k, v in proc.state_dict().items()}
    y = T.processor_forward(p, "", x.double(), 2, kw["num_heads"], kw["window_size"], case["batch"], kw.get("qk_norm", False))
    assert float((y.float() - case["out"]).abs().max()) <= 1e-4 * max(1.0, float(case["out"].abs().max()))


def test_model_builds_without_processor_edges_and_matches_the_reference_keys():
    case = FIXTURES["transformer_model.pt"]["model"]
    model, g, _, psum = T.tiny_model(case)
    assert type(model.processor_graph_provider).__name__ == "NoOpGraphProvider"
    assert type(model.processor).__name__ == "TransformerProcessor"
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == case["keys"]
    assert psum == pytest.approx(case["param_sum"], rel=1e-9)
    model.load_state_dict(model.state_dict(), strict=True)


def test_other_model_kinds_and_default_graph_unchanged():
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models.configs import model_config

    assert model_config("gt", 64, 2, 4, 8)["model"]["processor"]["_target_"].endswith("GraphTransformerProcessor")
    assert model_config("transformer", 64, 2, 4, 8)["model"]["processor"]["_target_"] == "anemoi.models.layers.processor.TransformerProcessor"
    g = build_synthetic_graph("o8", 3)
    assert g.proc_edge_index is not None and g.proc_edge_attr is not None


# -------------------------------------------------------------------------------------------- tail routes of the Transformer block
@pytest.fixture
def on_device():
    torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        del torch.Tensor.is_cuda


def _blocks(D=512, dtype=torch.bfloat16):
    torch.manual_seed(0)
    lk = load_layer_kernels(None)
    kw = dict(num_channels=D, hidden_dim=4 * D, num_heads=16, window_size=512, layer_kernels=lk)
    return [TransformerProcessorBlock(**kw).to(dtype).eval() for _ in range(2)]


def _route(blk, rows, nxt=None, D=512, dtype=torch.bfloat16, extra=False):
    x = torch.empty(rows, D, dtype=dtype)
    return blk._tail_route(x, x, None, Carrier(next_block=nxt), x if extra else None, None)


def test_transformer_tail_routes(on_device):
    b0, b1 = _blocks()
    att = b1.attention
    with torch.no_grad():
        r = _route(b0, 4096, b1)
        assert (r.kind, r.next_block, r.lnq) == ("chain2", b1, b1.layer_norm_attention)
        assert r.projs == (att.lin_q, att.lin_k, att.lin_v)  # the next block's q|k|v: 3A = 1 536 columns, no bias
        r = _route(b0, 4095, b1)
        assert (r.kind, r.next_block, r.projs) == ("cluster", b1, (att.lin_q, att.lin_k, att.lin_v))
        assert _route(b1, 4096).kind == "chain2" and _route(b1, 4096).next_block is None
    assert _route(b0, 4096, b1).kind == "plain"  # gradients wanted
    q0, q1 = _blocks(dtype=torch.float32)
    with torch.no_grad():
        assert _route(q0, 4096, q1, dtype=torch.float32).kind == "plain"
    c0, c1 = _blocks(D=1024)
    with torch.no_grad():
        r = _route(c0, 10242, c1, D=1024)
        assert (r.kind, r.next_block) == ("lnfold", c1)  # the next Transformer block folds the row statistics
        assert (_route(c1, 10242, D=1024).kind, _route(c1, 10242, D=1024).next_block) == ("lnfold", None)


def test_qk_norm_keeps_the_next_projection_off_the_chain(on_device):
    lk = load_layer_kernels(None)
    kw = dict(num_channels=512, hidden_dim=2048, num_heads=16, window_size=512, layer_kernels=lk)
    b0 = TransformerProcessorBlock(**kw).to(torch.bfloat16).eval()
    b1 = TransformerProcessorBlock(**kw, qk_norm=True).to(torch.bfloat16).eval()
    with torch.no_grad():
        r = _route(b0, 4096, b1)
    assert (r.kind, r.next_block, r.projs) == ("chain2", None, ())


def test_graph_transformer_routes_accept_a_transformer_consumer_only_by_duck_type(on_device):
    """A GraphTransformer mapper's tail behind a Transformer block: the decoder is no statistics reader; the routes of the GT blocks
    themselves are pinned by tests/test_tail_route_cpu.py."""
    b0, _ = _blocks()
    lk = load_layer_kernels(None)
    dec = GraphTransformerMapperBlock(in_channels=512, hidden_dim=2048, out_channels=512, num_heads=16, edge_dim=3, layer_kernels=lk)
    dec = dec.to(torch.bfloat16).eval()
    with torch.no_grad():
        r = _route(b0, 4096, dec)
    assert (r.kind, r.next_block, r.projs) == ("chain2", dec, (dec.lin_key, dec.lin_value))
    assert getattr(dec, "folds_row_stats", False) is False
    assert B.TransformerProcessorBlock.folds_row_stats and B.GraphTransformerProcessorBlock.folds_row_stats


# -------------------------------------------------------------------------------------------- op layer
def test_window_attention_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from anemoi_core_amd import _ext

    ext = _ext.ops()
    assert hasattr(ext, "window_attention")
    with FakeTensorMode():
        buf = torch.empty(300, 3 * 256, dtype=torch.bfloat16)
        q, k, v = buf[:, :256], buf[:, 256:512], buf[:, 512:]
        out, lse = ext.window_attention(q, k, v, 8, 64, 32 ** -0.5, 0.0, None, 3, True)
        assert out.shape == (300, 256) and out.dtype == torch.bfloat16
        assert lse.shape == (300, 8) and lse.dtype == torch.float32
        out, lse = ext.window_attention(q, k, v, 8, -1, 32 ** -0.5, 0.0, None, 1, False)
        assert lse.shape == (0, 8)


def test_window_attention_rejects_unsupported_head_dims_and_cpu_tensors():
    from anemoi_core_amd import ops

    x = torch.zeros(16, 96)
    with pytest.raises(ValueError, match="supported"):
        ops.window_attention(x, x, x, 2, 4)  # d = 48
    x = torch.zeros(16, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.window_attention(x, x, x, 2, 4)


# -------------------------------------------------------------------------------------------- inference only
def test_training_through_the_processor_raises():
    from anemoi_core_amd.distributed.shapes import GraphShardInfo

    case = CASES["w8_d32"]
    proc = T.processor(case["kw"])
    x = torch.zeros(T.ROWS, 64)
    with pytest.raises(NotImplementedError, match="backward kernel"):
        proc(x, 1, GraphShardInfo(nodes=None))  # parameters require grad, grad enabled
    proc.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="backward kernel"):
        proc(x.requires_grad_(), 1, GraphShardInfo(nodes=None))
    drop = T.processor(dict(case["kw"], dropout_p=0.1)).requires_grad_(False).train()
    with pytest.raises(NotImplementedError, match="backward kernel"):
        with torch.no_grad():
            drop(torch.zeros(T.ROWS, 64), 1, GraphShardInfo(nodes=None))


# -------------------------------------------------------------------------------------------- model glue
class _HeteroLike:
    """A HeteroData-like graph (``g[name].x``, ``g[(src, "to", dst)].edge_index / edge_length / edge_dirs``, ``node_types``,
    ``edge_types``) whose stores appear on first access, as torch_geometric's do."""

    def __init__(self):
        self._nodes, self._edges = {}, {}

    def __getitem__(self, key):
        from types import SimpleNamespace

        table = self._edges if isinstance(key, tuple) else self._nodes
        return table.setdefault(key, SimpleNamespace())

    @property
    def node_types(self):
        return list(self._nodes)

    @property
    def edge_types(self):
        return list(self._edges)


def test_model_from_a_heterodata_graph_without_processor_edges():
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices, model_config

    g = build_synthetic_graph("o8", 3, processor_edges=False)
    hd = _HeteroLike()
    hd["data"].x, hd["data"].num_nodes = torch.from_numpy(g.data_latlon), g.num_data
    hd["hidden"].x, hd["hidden"].num_nodes = torch.from_numpy(g.hidden_latlon), g.num_hidden
    for key, ei, ea in ((("data", "to", "hidden"), g.enc_edge_index, g.enc_edge_attr), (("hidden", "to", "data"), g.dec_edge_index, g.dec_edge_attr)):
        hd[key].edge_index = torch.from_numpy(ei).to(torch.int32)
        hd[key].edge_length, hd[key].edge_dirs = torch.from_numpy(ea[:, :1].copy()), torch.from_numpy(ea[:, 1:].copy())
    case = FIXTURES["transformer_model.pt"]["model"]
    model = AnemoiModelEncProcDec(model_config=model_config("transformer", 64, 2, 2, 8, window_size=16), data_indices=make_data_indices(4, 4),
                                  statistics={"data": None}, n_step_input=2, n_step_output=1, graph_data=hd)
    assert type(model.processor_graph_provider).__name__ == "NoOpGraphProvider"
    assert ("hidden", "to", "hidden") not in hd.edge_types  # asking for the absent edge type did not create it
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == case["keys"]


def test_model_restatement_reproduces_the_reference():
    """tests/transformer_helpers.model_forward (the restatement of the full-size GPU model test) against the reference's tiny model."""
    case = FIXTURES["transformer_model.pt"]["model"]
    model, g, x, _ = T.tiny_model(case)
    p = {k: v.detach() for k, v in model.state_dict().items()}
    with torch.no_grad():
        y = T.model_forward(p, g, x, 2, 2, case["window"])
    assert y.shape == case["out"].shape
    assert float((y - case["out"]).abs().max()) <= 1e-4 * max(1.0, float(case["out"].abs().max()))
