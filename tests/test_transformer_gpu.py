"""TransformerProcessor and the tiny Transformer model on the MI355X: against the reference's fixtures (tests/golden/transformer*.pt,
fp32) and against the plain-torch restatement (tests/transformer_helpers.py, checked against the reference by test_transformer_cpu.py)
with the bounds of tests/test_fullsize_parity_gpu._check; the chain route of the 512-channel blocks; hipGraph replay."""
import os

import pytest
import torch

from anemoi_core_amd import ops
from anemoi_core_amd.distributed.shapes import GraphShardInfo
from tests import transformer_helpers as T
from tests.test_fullsize_parity_gpu import _check

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = {name: torch.load(os.path.join(T.GOLDEN, name), weights_only=False) for name in ("transformer.pt", "transformer_model.pt")}
CASES = {k: v for f in FIXTURES.values() for k, v in f.items() if k != "model"}


def _processor(case, dtype):
    proc = T.processor(case["kw"]).eval()
    T.fill(proc, case["param_seed"])
    x = T.inputs(case["input_seed"], case["batch"] * T.ROWS, case["kw"]["num_channels"])
    return proc.to(DEV, dtype), x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", sorted(CASES))
def test_processor_against_the_reference(name, dtype):
    case = CASES[name]
    kw = case["kw"]
    proc, x = _processor(case, dtype)
    with torch.no_grad():
        y = proc(x.to(DEV, dtype), case["batch"], GraphShardInfo(nodes=None)).float().cpu()
    if dtype == torch.float32:
        want = case["out"]
    else:  # bf16: the restatement on the rounded parameters and inputs
        p = {k: v.float().cpu().double() for k, v in proc.state_dict().items()}
        want = T.processor_forward(p, "", x.to(dtype).double(), 2, kw["num_heads"], kw["window_size"], case["batch"],
                                   kw.get("qk_norm", False)).float()
    _check(f"transformer {name}", y, want, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiny_model_against_the_reference(dtype):
    case = FIXTURES["transformer_model.pt"]["model"]
    model, _, x, _ = T.tiny_model(case)
    with torch.no_grad():
        y = model.to(DEV, dtype)({"data": x.to(DEV, dtype)})["data"].float().cpu()
    # bf16 against the fp32 reference: every weight, input and activation is rounded, the same bound as the fp32-oracle comparisons
    _check("transformer tiny model", y, case["out"], dtype, fp32_tol=5e-5)


@pytest.mark.parametrize("channels,window", [(512, 512), (1024, 512)])
def test_processor_full_size_bf16(channels, window):
    """10 242 rows (the hidden mesh of res 5), 16 heads, 2 layers, bf16, against the restatement on the rounded values."""
    kw = dict(num_channels=channels, num_heads=16, window_size=window)
    proc = T.processor(kw).eval()
    T.fill(proc, 7, scale=0.03)
    x = T.inputs(8, 10242, channels)
    proc = proc.to(DEV, torch.bfloat16)
    with torch.no_grad():
        y = proc(x.to(DEV, torch.bfloat16), 1, GraphShardInfo(nodes=None)).float().cpu()
    p = {k: v.float().cpu() for k, v in proc.state_dict().items()}
    want = T.processor_forward(p, "", x.to(torch.bfloat16).float(), 2, 16, window)
    _check(f"transformer {channels} ch", y, want, torch.bfloat16)


def test_512_channel_blocks_take_the_chain_launch(monkeypatch):
    calls = []
    real = ops.gt_layer_chain2
    monkeypatch.setattr(ops, "gt_layer_chain2", lambda *a, **k: calls.append(k.get("q_out_features")) or real(*a, **k))
    proc = T.processor(dict(num_channels=512, num_heads=16, window_size=512)).eval()
    T.fill(proc, 9, scale=0.03)
    proc = proc.to(DEV, torch.bfloat16)
    with torch.no_grad():
        proc(T.inputs(10, 10242, 512).to(DEV, torch.bfloat16), 1, GraphShardInfo(nodes=None))
    assert calls == [1536, 0]  # block 0 hands block 1 its q|k|v; the last block has no consumer


def test_model_hipgraph_replay_is_bit_equal_to_eager():
    case = FIXTURES["transformer_model.pt"]["model"]
    model, _, x, _ = T.tiny_model(case)
    model = model.to(DEV, torch.bfloat16)
    xin = {"data": x.to(DEV, torch.bfloat16)}
    with torch.no_grad():
        eager = model(xin)["data"].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(xin)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(xin)["data"]
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
