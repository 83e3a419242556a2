#!/usr/bin/env python
"""Time of the truncated residual's two sparse projections, kernel route against torch route, in one process.

CSR ``torch.sparse.mm`` cannot be captured into a hipGraph (torch 2.10 on ROCm 7.0: the capture is invalidated), so the two ROUTES are compared
by device events around back-to-back eager launches, alternating (torch, kernel, torch, kernel, ...), the spread taken from the repeated
torch-route runs of the same call.  At small shapes such a figure is mostly the host's launch cost on both sides (the kernel route: two launches
and a cast; the torch route: two permute copies, two sparse products, casts, an index_select), so the kernel route's device time from hipGraph
replays is reported beside it (``kernel_graph_us``, and per projection in ``kernel_projections``).

(a) ``ops.sparse_project`` down then up (the prognostic columns selected inside the down projection, fp32 on the coarse grid) against the path
    it replaces - a restatement of the reference's SparseProjector on the GPU: permute to [N, B C], ``torch.sparse.mm`` with a CSR matrix,
    permute back, for ALL input columns, twice (layers/sparse_projector.py:78-104 as residual.py:290-291 calls it); the prognostic columns
    are selected afterwards, as the reference's model does.  ``torch_selected`` is the same torch route given only the selected columns (an
    index_select first): not what the reference runs, reported for scale.  Shapes: O96 -> O48 -> O96 and N320 -> O96 -> N320, 101 input
    columns of which 80 are selected, fp32 and bf16, batch 1 and 4.  The matrix is fp32 CSR for both dtypes; bf16 rows take an fp32 round trip
    (see ``torch_matrix``) and the row says so.
(b) row-length skew: the down projection (cutoff edges: ragged rows) against a matrix of the same destination rows with the SAME number of
    entries in every row (the k nearest, k = the ragged matrix's mean), as device time per entry - what splitting long rows could gain at most.
(c) the whole O96 -> res 5, 512-channel, 16-layer GraphTransformer forward with the skip and with the truncated residual (bf16, batch 1).

Bandwidth is reported against two byte counts computed from the shapes: every destination row's gathers (entries x columns), and each source
row read once; both include the result's write and the matrix's 8 bytes per entry.
Writes one JSON (default profiles/r09_truncation_time.json), rewritten after every row.
usage: python tools/truncation_time.py [--out PATH] [--kernel-only] [--repeats R]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemm_sweep import timeit  # noqa: E402

from anemoi_core_amd import ops  # noqa: E402
from anemoi_core_amd.graphs.io import GraphData  # noqa: E402
from anemoi_core_amd.graphs.synthetic import (build_synthetic_graph, build_truncation_pair, fibonacci_grid, knn_edges, octahedral_grid,  # noqa: E402
                                              to_graph_data)
from anemoi_core_amd.layers.graph_provider import ProjectionGraphProvider  # noqa: E402
from anemoi_core_amd.layers.residual import TruncatedConnection  # noqa: E402

DEV = "cuda"
V, SELECTED, T = 101, 80, 2
DOWN, UP = ("data", "to", "truncation"), ("truncation", "to", "data")


def eager_time(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def torch_matrix(provider, dtype):
    """(CSR matrix for torch.sparse.mm, description).  The values are fp32 for every dtype of the rows: a bf16 CSR product is not attempted
    (torch 2.10 on ROCm 7.0 ends the process with an uncaught C++ exception from the sparse library instead of raising), so 16-bit rows are
    cast to fp32 for the product and the result back, which is also what the reference's fp32 matrix needs without autocast."""
    m = torch.sparse_csr_tensor(torch.from_numpy(provider.indptr).to(DEV), torch.from_numpy(provider.indices).to(DEV),
                                torch.from_numpy(provider.values).to(DEV), size=provider.shape)
    return m, "csr, float32 values" + ("" if dtype == torch.float32 else " (rows cast to fp32 and back)")


def torch_project(x, m):
    """The reference's SparseProjector._project_flattened: [B, N, C] -> [N, B C], sparse.mm, -> [B, M, C]."""
    B, N, C = x.shape
    rhs = x.permute(1, 0, 2).reshape(N, B * C)
    out = torch.sparse.mm(m, rhs.to(m.dtype)).to(x.dtype)
    return out.reshape(m.shape[0], B, C).permute(1, 0, 2).reshape(B, m.shape[0], C)


def entries(provider):
    n = np.diff(provider.indptr)
    return dict(rows=int(provider.shape[0]), source_rows=int(provider.shape[1]), entries=int(n.sum()), max_per_row=int(n.max()), median_per_row=float(np.median(n)))


def byte_counts(provider, batch, cols, in_size, out_size):
    nnz, (n_dst, n_src) = int(provider.indptr[-1]), provider.shape
    write, matrix = n_dst * cols * batch * out_size, nnz * 8
    return nnz * cols * batch * in_size + write + matrix, n_src * cols * batch * in_size + write + matrix


def projection_rows(repeats, out, save):
    grids = {"o96->o48": (octahedral_grid(96), "o48"), "n320->o96": (fibonacci_grid(542080), "o96")}
    for shape_name, (data, coarse) in grids.items():
        pair = build_truncation_pair(data, coarse, k=3)
        t = torch.from_numpy
        gd = GraphData({"data": {"num_nodes": int(data.shape[0])}, "truncation": {"num_nodes": int(pair["latlon"].shape[0])}},
                       {DOWN: {"edge_index": t(pair["down_edge_index"]), "gauss_weight": t(pair["down_weight"])[:, None]},
                        UP: {"edge_index": t(pair["up_edge_index"]), "gauss_weight": t(pair["up_weight"])[:, None]}})
        layer = TruncatedConnection(graph=gd, truncation_down_edges_name=DOWN, truncation_up_edges_name=UP, row_normalize=True)
        down, up = layer.provider_down, layer.provider_up
        md, mu = down.get_edges(device=DEV), up.get_edges(device=DEV)
        stats = dict(down=entries(down), up=entries(up))
        # the same destination rows with an equal number of entries each: the k nearest, k = the ragged matrix's mean
        k_even = max(1, int(round(stats["down"]["entries"] / stats["down"]["rows"])))
        ei = knn_edges(data, pair["latlon"].astype(np.float64), k_even)
        even = ProjectionGraphProvider(graph=GraphData({"data": {"num_nodes": int(data.shape[0])}, "truncation": {"num_nodes": int(pair["latlon"].shape[0])}},
                                                       {DOWN: {"edge_index": t(ei)}}), edges_name=DOWN, row_normalize=True)
        me = even.get_edges(device=DEV)
        cols = torch.arange(SELECTED, dtype=torch.int32, device=DEV) + 7
        for dtype in (torch.float32, torch.bfloat16):
            td, how = torch_matrix(down, dtype)
            tu, how_up = torch_matrix(up, dtype)
            for batch in (1, 4):
                x5 = torch.randn(batch, T, 1, data.shape[0], V, device=DEV).to(dtype)
                last = x5[:, -1, 0]  # [B, N, V], strided

                def kernel():
                    return ops.sparse_project(ops.sparse_project(last, md, cols, out_dtype=torch.float32), mu).to(dtype)

                def kernel_down():
                    return ops.sparse_project(last, md, cols, out_dtype=torch.float32)

                coarse_rows = kernel_down()

                def kernel_up():
                    return ops.sparse_project(coarse_rows, mu)

                def reference():
                    return torch_project(torch_project(last, td), tu).index_select(-1, cols.long())

                def selected():
                    return torch_project(torch_project(last.index_select(-1, cols.long()), td), tu)

                with torch.inference_mode():
                    err = float((kernel().float() - reference().float()).abs().max())
                    timer, timing = eager_time, "events around eager launches (CSR torch.sparse.mm does not capture)"
                    ref_t, ker_t, sel_t = [], [], []
                    for _ in range(repeats):
                        ref_t.append(timer(reference))
                        ker_t.append(timer(kernel))
                        sel_t.append(timer(selected))
                    t_down, t_up, t_graph = timeit(kernel_down), timeit(kernel_up), timeit(kernel)  # device time: hipGraph replays
                    t_even = timeit(lambda: ops.sparse_project(last, me, cols, out_dtype=torch.float32))
                med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
                spread = max(ref_t) - min(ref_t)
                size = torch.empty((), dtype=dtype).element_size()
                bw = {}
                for name, prov, t, ins in (("down", down, t_down, size), ("up", up, t_up, 4)):
                    gathers, once = byte_counts(prov, batch, SELECTED, ins, 4)
                    bw[name] = dict(us=round(t, 2), gather_bytes=gathers, read_once_bytes=once, gather_TBps=round(gathers / t / 1e6, 3),
                                    read_once_TBps=round(once / t / 1e6, 3))
                row = dict(shape=shape_name, dtype=str(dtype).replace("torch.", ""), batch=batch, input_columns=V, selected_columns=SELECTED,
                           torch_route=dict(down=how, up=how_up), timing=timing, max_abs_difference_of_routes=err, torch_us=[round(t, 2) for t in ref_t],
                           kernel_us=[round(t, 2) for t in ker_t], torch_selected_us=[round(t, 2) for t in sel_t], torch_median_us=round(med(ref_t), 2),
                           kernel_median_us=round(med(ker_t), 2), torch_selected_median_us=round(med(sel_t), 2), torch_spread_us=round(spread, 2),
                           ratio_torch_over_kernel=round(med(ref_t) / med(ker_t), 3), ratio_torch_selected_over_kernel=round(med(sel_t) / med(ker_t), 3),
                           kernel_slower_beyond_spread=bool(med(ker_t) > med(ref_t) + spread), kernel_graph_us=round(t_graph, 2),
                           kernel_projections=bw, matrices=stats,
                           skew=dict(ragged_down_us=round(t_down, 2), ragged_ns_per_entry=round(1e3 * t_down / stats["down"]["entries"], 4),
                                     even_entries_per_row=k_even, even_down_us=round(t_even, 2),
                                     even_ns_per_entry=round(1e3 * t_even / int(even.indptr[-1]), 4),
                                     ragged_over_even_per_entry=round((t_down / stats["down"]["entries"]) / (t_even / int(even.indptr[-1])), 3)))
                print(json.dumps(row), flush=True)
                out.append(row)
                save()
                del x5, last, coarse_rows
                torch.cuda.empty_cache()


def model_rows(repeats, channels=512, layers=16, heads=16):
    from anemoi_core_amd.models import AnemoiModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices, model_config, truncated_residual_config

    g = build_synthetic_graph("o96", 5)
    gd = to_graph_data(g, build_truncation_pair(g.data_latlon, "o48", k=3))
    x = {"data": torch.randn(1, T, 1, g.num_data, V, device=DEV).to(torch.bfloat16)}
    models = {}
    for name, residual in (("skip", None), ("truncated", truncated_residual_config(row_normalize=True))):
        torch.manual_seed(0)
        models[name] = AnemoiModelEncProcDec(model_config=model_config("gt", channels, layers, heads, 8, residual=residual),
                                             data_indices=make_data_indices(V, SELECTED), statistics={"data": None}, n_step_input=T, n_step_output=1,
                                             graph_data=gd).eval().to(DEV, torch.bfloat16)
    skip_t, trunc_t = [], []
    with torch.inference_mode():
        for _ in range(repeats):
            skip_t.append(timeit(lambda: models["skip"](x), reps=3, replays=5))
            trunc_t.append(timeit(lambda: models["truncated"](x), reps=3, replays=5))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    row = dict(graph="o96 -> res 5, truncation grid o48", channels=channels, layers=layers, dtype="bfloat16", batch=1, input_columns=V,
               prognostic_columns=SELECTED, skip_us=[round(t, 1) for t in skip_t], truncated_us=[round(t, 1) for t in trunc_t],
               skip_median_us=round(med(skip_t), 1), truncated_median_us=round(med(trunc_t), 1), skip_spread_us=round(max(skip_t) - min(skip_t), 1),
               added_us=round(med(trunc_t) - med(skip_t), 1))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r09_truncation_time.json"))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/truncation_time.py measures on the GPU; none is visible")
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, projections=[])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)

    projection_rows(args.repeats, result["projections"], save)
    if not args.kernel_only:
        result["model"] = model_rows(args.repeats)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
