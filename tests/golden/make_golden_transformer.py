"""Generate tests/golden/transformer.pt and transformer_model.pt by IMPORTING the Python reference (its TransformerProcessor and an
AnemoiModelEncProcDec with GraphTransformer mappers around it), fp32, CPU, ``attention_implementation="scaled_dot_product_attention"``
(flash-attention does not run without a GPU; both names select the same HIP kernel here).

Parameters and inputs are not stored: they are drawn from seeded CPU generators in state_dict order (``fill``), which the tests repeat
on their side; the fixture holds the configuration, the seeds, the reference's state_dict keys / shapes, a checksum of the drawn
parameters and the reference's outputs.  Runs only where the reference is available (needs /root/reference via ref_standins).

Usage:  python tests/golden/make_golden_transformer.py
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_standins as rs  # noqa: E402

rs.install()

from anemoi.models.distributed.shapes import GraphShardInfo  # noqa: E402
from anemoi.models.layers.processor import TransformerProcessor  # noqa: E402

from anemoi_core_amd.graphs.synthetic import build_synthetic_graph  # noqa: E402
from tests.transformer_helpers import fill, inputs  # noqa: E402  (the tests draw the same parameters and inputs)

ROWS = 642
PROC_CASES = {  # name -> (processor keywords, batch size)
    "w8_d32": (dict(num_channels=64, num_heads=2, window_size=8), 1),
    "none_d64": (dict(num_channels=128, num_heads=2, window_size=None), 1),
    "qk_norm": (dict(num_channels=64, num_heads=2, window_size=8, qk_norm=True), 1),
    "attn_channels": (dict(num_channels=64, attn_channels=128, num_heads=4, window_size=16), 1),
    "batch2": (dict(num_channels=64, num_heads=2, window_size=8), 2),
    "window_ge_n": (dict(num_channels=64, num_heads=2, window_size=1000), 1),
}
FILES = {"transformer.pt": ("w8_d32", "none_d64", "qk_norm", "attn_channels"), "transformer_model.pt": ("batch2", "window_ge_n")}


def proc_kwargs(kw: dict) -> dict:
    return dict(num_layers=2, num_chunks=1, mlp_hidden_ratio=4, dropout_p=0.0, layer_kernels=None, **kw)


def gen_processor(name: str) -> dict:
    kw, batch = PROC_CASES[name]
    torch.manual_seed(0)
    proc = TransformerProcessor(**proc_kwargs(kw), attention_implementation="scaled_dot_product_attention").eval()
    psum = fill(proc, 1000 + len(name))
    x = inputs(2000 + len(name), batch * ROWS, kw["num_channels"])
    with torch.no_grad():
        y = proc(x, batch, GraphShardInfo(nodes=None))
    keys = {k: tuple(v.shape) for k, v in proc.state_dict().items()}
    print(name, tuple(y.shape), float(y.abs().mean()))
    return dict(kw=kw, batch=batch, param_seed=1000 + len(name), input_seed=2000 + len(name), param_sum=psum, keys=keys, out=y.clone())


def model_hetero(g):
    """The tiny model's graph as a HeteroData WITHOUT hidden -> hidden edges: the reference then gives its processor a NoOpGraphProvider."""
    hd = rs.HeteroData()
    hd["data"].x = torch.from_numpy(g.data_latlon)
    hd["data"].num_nodes = g.num_data
    hd["hidden"].x = torch.from_numpy(g.hidden_latlon)
    hd["hidden"].num_nodes = g.num_hidden
    for key, ei, ea in ((("data", "to", "hidden"), g.enc_edge_index, g.enc_edge_attr), (("hidden", "to", "data"), g.dec_edge_index, g.dec_edge_attr)):
        hd[key].edge_index = torch.from_numpy(ei).to(torch.int32)
        hd[key].edge_length = torch.from_numpy(ea[:, :1].copy())
        hd[key].edge_dirs = torch.from_numpy(ea[:, 1:].copy())
    return hd


def gen_model() -> dict:
    from anemoi.models.models import AnemoiModelEncProcDec
    from make_golden import make_data_indices

    from anemoi_core_amd.models.configs import model_config

    g = build_synthetic_graph("o8", 3, processor_edges=False)
    n_vars, n_step = 4, 2
    cfg = model_config("transformer", 64, 2, 2, 8, window_size=16)
    cfg["model"]["processor"]["attention_implementation"] = "scaled_dot_product_attention"
    torch.manual_seed(0)
    model = AnemoiModelEncProcDec(model_config=rs.DotDict(cfg), data_indices=make_data_indices(n_vars, n_vars), statistics={"data": None},
                                  n_step_input=n_step, n_step_output=1, graph_data=model_hetero(g)).eval()
    assert type(model.processor_graph_provider).__name__ == "NoOpGraphProvider"
    psum = fill(model, 3000)
    x = torch.randn(1, n_step, 1, g.num_data, n_vars, generator=torch.Generator().manual_seed(4000))
    with torch.no_grad():
        y = model({"data": x})["data"]
    print("model", tuple(y.shape), float(y.abs().mean()))
    return dict(n_vars=n_vars, n_step=n_step, window=16, param_seed=3000, param_sum=psum, input_seed=4000,
                keys={k: tuple(v.shape) for k, v in model.state_dict().items()}, out=y.clone())


def main() -> None:
    for fname, names in FILES.items():
        obj = {name: gen_processor(name) for name in names}
        if fname == "transformer_model.pt":
            obj["model"] = gen_model()
        path = os.path.join(HERE, fname)
        torch.save(obj, path)
        print(f"{fname}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
