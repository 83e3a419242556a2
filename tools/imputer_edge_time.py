#!/usr/bin/env python
"""What the imputer costs at the model edges: ``AnemoiModelEncProcDec.predict_step`` at the O96 benchmark configuration (O96 data grid,
resolution-5 hidden mesh, 16 GraphTransformer layers x 512 channels x 16 heads, 84 variables, 2 input steps), fp32 data into a bf16 model,
batch 1, in three cases that alternate in ONE process:

  (a) normaliser   pre = [InputNormalizer], no NaN in the batch: the path without an imputer (fused normaliser);
  (b) fused        pre = [InputImputer, InputNormalizer], about 5 % NaN in two imputed prognostic variables: the imputation program
                   rides in the model-edge kernels: the launches of (a), each replaced by its sibling (the index collection has
                   no diagnostic variable, so the NaN mask needs no gather; one ``index_select`` more with one);
  (c) modules      the chain of (b) hidden from the fusion (an opaque wrapper, as tests/test_edges_gpu.py does): the imputer's and the
                   normaliser's stand-alone kernels run before and after the forward.

Each repeat times every case once, in the order a b c, with device events around ``--calls`` eager calls and around as many replays of the
case's captured hipGraph (all three capture: no case synchronises with the host).  Reported per case: the per-call time of every repeat, its
median and its spread (max - min over the repeats); (b) - (a) and (c) - (a) of the medians, and whether (b) - (a) lies within the spread of
(a).  The outputs of (b) and (c) are compared once (NaN at the same places, largest difference of the rest).

Writes one JSON (default profiles/r15_imputer_edge_time.json).
usage: python tools/imputer_edge_time.py [--out PATH] [--repeats R] [--calls K] [--warmup W] [--layers L] [--channels C]"""
import argparse
import json
import os
import statistics as st
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from anemoi_core_amd.graphs.synthetic import build_synthetic_graph  # noqa: E402
from anemoi_core_amd.models import AnemoiModelEncProcDec  # noqa: E402
from anemoi_core_amd.models.configs import make_data_indices, model_config  # noqa: E402
from anemoi_core_amd.preprocessing import InputImputer, InputNormalizer, Processors  # noqa: E402

DEV = "cuda"
T_STEPS = 2
IMPUTED = ("v3", "v7")


class Opaque(torch.nn.Module):
    """Hides a Processors chain from the fusion: the member modules run."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, **kw):
        return self.inner(x, **kw)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls  # us per call


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r15_imputer_edge_time.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--vars", type=int, default=84)
    ap.add_argument("--data-grid", default="o96")
    ap.add_argument("--hidden-res", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/imputer_edge_time.py measures on the GPU; none is visible")

    V = args.vars
    g = build_synthetic_graph(args.data_grid, args.hidden_res)
    torch.manual_seed(0)
    di = make_data_indices(V, V)["data"]
    di.data.input.full = list(range(V))
    di.data.output = SimpleNamespace(full=list(range(V)), name_to_index={f"v{i}": i for i in range(V)})
    rng = np.random.default_rng(0)
    mean, stdev = rng.normal(size=V), 0.5 + rng.random(V)
    stats = {"mean": mean, "stdev": stdev, "minimum": mean - 3 * stdev, "maximum": mean + 3 * stdev}
    model = AnemoiModelEncProcDec(model_config=model_config("gt", args.channels, args.layers, args.heads, 8), data_indices={"data": di},
                                  statistics={"data": stats}, n_step_input=T_STEPS, n_step_output=1, graph_data=g).eval().to(DEV).to(torch.bfloat16)
    nm = InputNormalizer(config={"default": "mean-std"}, data_indices=di, statistics=stats).to(DEV)
    imp = InputImputer({"default": "none", "mean": list(IMPUTED)}, di, stats)
    gen = torch.Generator().manual_seed(0)
    clean = (torch.from_numpy(mean).float() + torch.from_numpy(stdev).float() * torch.randn(1, T_STEPS, g.num_data, V, generator=gen)).to(DEV)
    holes = clean.clone()
    masked = torch.rand(g.num_data, generator=gen) < 0.05  # the same grid points at both steps, like a land-sea mask
    for name in IMPUTED:
        holes[0, :, masked.to(DEV), di.model.input.name_to_index[name]] = float("nan")
    pair = lambda inverse: Processors([["imputer", imp], ["normalizer", nm]], inverse=inverse)  # noqa: E731
    step = lambda batch, pre, post: model.predict_step({"data": batch}, {"data": pre}, {"data": post}, T_STEPS)["data"]  # noqa: E731
    pre_a, post_a = Processors([["normalizer", nm]]), Processors([["normalizer", nm]], inverse=True)
    pre_b, post_b = pair(False), pair(True)
    pre_c, post_c = Opaque(pair(False)), Opaque(pair(True))
    cases = {"a_normaliser": lambda: step(clean, pre_a, post_a), "b_fused": lambda: step(holes, pre_b, post_b),
             "c_modules": lambda: step(holes, pre_c, post_c)}

    out_b, out_c = cases["b_fused"]().float(), cases["c_modules"]().float()
    same_nan = bool(torch.equal(out_b.isnan(), out_c.isnan()))
    fin = ~out_c.isnan()
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  config=dict(data_grid=args.data_grid, hidden_res=args.hidden_res, layers=args.layers, channels=args.channels, heads=args.heads,
                              variables=V, input_steps=T_STEPS, data_nodes=int(g.num_data), data_dtype="float32", model_dtype="bfloat16", batch=1,
                              imputed=list(IMPUTED), nan_fraction_in_imputed=round(float(masked.float().mean()), 4)),
                  timing=f"device events around {args.calls} calls, {args.warmup} warm-up calls per case, {args.repeats} repeats alternating a b c",
                  fused_vs_modules=dict(nan_at_the_same_places=same_nan, restored_nan=int(out_b.isnan().sum()),
                                        max_abs_difference=float((out_b[fin] - out_c[fin]).abs().max()), scale=float(out_c[fin].abs().max())))
    graphs = {}
    for name, fn in cases.items():
        for _ in range(args.warmup):
            fn()
        graphs[name] = capture(fn)[0]
        for _ in range(args.warmup):
            graphs[name].replay()
    torch.cuda.synchronize()
    eager, replay = {n: [] for n in cases}, {n: [] for n in cases}
    for _ in range(args.repeats):
        for name, fn in cases.items():
            eager[name].append(round(timed(fn, args.calls), 2))
        for name in cases:
            replay[name].append(round(timed(graphs[name].replay, args.calls), 2))
    for kind, rows in (("eager", eager), ("graph_replay", replay)):
        med = {n: st.median(v) for n, v in rows.items()}
        spread = {n: round(max(v) - min(v), 2) for n, v in rows.items()}
        b_a, c_a = round(med["b_fused"] - med["a_normaliser"], 2), round(med["c_modules"] - med["a_normaliser"], 2)
        result[kind] = dict(us_per_call=rows, median_us=med, spread_us=spread, b_minus_a_us=b_a, c_minus_a_us=c_a,
                            b_minus_a_within_spread_of_a=bool(abs(b_a) <= spread["a_normaliser"]))
        print(f"{kind}: medians {med} spread {spread}  b-a {b_a} us  c-a {c_a} us")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
