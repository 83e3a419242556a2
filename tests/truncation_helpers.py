"""Shared pieces of the truncated-residual tests: the graph, configurations, parameter and input draws of
tests/golden/make_golden_truncation.py, repeated with this package's classes, and the summation bound of the sparse projection."""
import os

import numpy as np
import torch

from tests.transformer_helpers import GOLDEN, fill

N_VARS, N_PROG, N_STEP_IN = 5, 4, 2  # one forcing column: the residual projects 4 of the 5 input columns
N_CHANNELS, N_LAYERS, N_HEADS, TRAINABLE = 64, 2, 2, 8
DOWN, UP = ("data", "to", "truncation"), ("truncation", "to", "data")
# name -> what the model is built with (the generator and the tests read the same dict)
MODEL_CASES = {
    "gt_batch1": dict(model="det", batch=1),
    "gt_batch2": dict(model="det", batch=2),
    "gt_2steps_out": dict(model="det", batch=1, n_step_output=2),
    "ens_gt_2x2": dict(model="ens", batch=2, members=2),
}


def load_fixture() -> dict:
    return torch.load(os.path.join(GOLDEN, "truncation.pt"), weights_only=False)


def synthetic_parts():
    """The o8 / resolution-3 graph and its truncation pair onto the 40-node O1 grid (3 nearest neighbours both ways, Gaussian weights)."""
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph, build_truncation_pair

    g = build_synthetic_graph("o8", 3)
    return g, build_truncation_pair(g.data_latlon, "o1", k=3, down="knn")


def graph_data(fx: dict = None):
    """This package's GraphData with the truncation node and edge sets; from the fixture's recorded graph if given (the same numbers)."""
    from anemoi_core_amd.graphs.synthetic import to_graph_data

    g, pair = synthetic_parts()
    if fx is not None:
        t = fx["graph"]
        pair = {"latlon": t["latlon"].numpy(), "down_edge_index": t["down_edge_index"].numpy(), "down_weight": t["down_weight"].numpy(),
                "up_edge_index": t["up_edge_index"].numpy(), "up_weight": t["up_weight"].numpy()}
    gd = to_graph_data(g, pair)
    if fx is not None:
        gd["data"]["area_weight"] = fx["graph"]["data_area_weight"]
        gd["truncation"]["area_weight"] = fx["graph"]["truncation_area_weight"]
    return g, gd


def residual_config(**extra) -> dict:
    from anemoi_core_amd.models.configs import truncated_residual_config

    return truncated_residual_config(row_normalize=True, **extra)


def model_config_of(case: dict) -> dict:
    from anemoi_core_amd.models.configs import ens_model_config, model_config

    if case["model"] == "ens":
        return ens_model_config("gt", N_CHANNELS, N_LAYERS, N_HEADS, TRAINABLE, noise_channels_dim=4, noise_mlp_hidden_dim=32,
                                residual=residual_config())
    return model_config("gt", N_CHANNELS, N_LAYERS, N_HEADS, TRAINABLE, residual=residual_config())


def build_model(fx: dict, name: str, residual=None):
    """(model, x) of fixture case ``name``; ``residual``: another ``model.residual`` entry (e.g. the default skip) for the same draw."""
    from anemoi_core_amd.models import AnemoiEnsModelEncProcDec, AnemoiModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices

    entry = fx["models"][name]
    case = entry["case"]
    g, gd = graph_data(fx)
    cfg = model_config_of(case)
    if residual is not None:
        cfg["model"]["residual"] = residual
    cls = AnemoiEnsModelEncProcDec if case["model"] == "ens" else AnemoiModelEncProcDec
    model = cls(model_config=cfg, data_indices=make_data_indices(N_VARS, N_PROG), statistics={"data": None}, n_step_input=N_STEP_IN,
                n_step_output=case.get("n_step_output", 1), graph_data=gd).eval()
    psum = fill(model, entry["param_seed"])
    assert abs(psum - entry["param_sum"]) <= 1e-6 * max(1.0, abs(entry["param_sum"])), "parameter draw differs from the generator's"
    x = torch.randn(case["batch"], N_STEP_IN, case.get("members", 1), g.num_data, N_VARS, generator=torch.Generator().manual_seed(entry["input_seed"]))
    return model, x


def dense(indptr, indices, values, shape) -> torch.Tensor:
    """float64 dense image of a CSR matrix (duplicates summed)."""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    a = torch.zeros(shape, dtype=torch.float64)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    a.index_put_((torch.as_tensor(rows).long(), torch.as_tensor(indices).long()), torch.as_tensor(np.asarray(values)).double(), accumulate=True)
    return a


U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def project64(indptr, indices, values, n_dst: int, fx: torch.Tensor) -> torch.Tensor:
    """The float64 product of a CSR matrix with fx [..., n_src, C] (float64): what the dense product gives, without forming the dense matrix."""
    rows = torch.repeat_interleave(torch.arange(n_dst), torch.as_tensor(np.diff(np.asarray(indptr))).long())
    idx, w = torch.as_tensor(np.asarray(indices)).long(), torch.as_tensor(np.asarray(values)).double()
    y = torch.zeros(*fx.shape[:-2], n_dst, fx.shape[-1], dtype=torch.float64)
    return y.index_add_(-2, rows, fx.index_select(-2, idx) * w[:, None])


def projection_bound(indptr, indices, values, shape, fx_abs: torch.Tensor, y_ref: torch.Tensor, out_dtype) -> torch.Tensor:
    """Per element, for k entries in the row:  (k + 4) 2^-24 sum_j |w_j| (|x_j mul| + |add|)  +  u_out |y|  (+ 2^-24 absolute for fp16).
    ``fx_abs``: |x mul| + |add| of the selected columns, float64 [..., n_src, C]; ``y_ref``: the float64 reference [..., n_dst, C]."""
    k = torch.as_tensor(np.diff(np.asarray(indptr))).double()
    first = (k + 4.0)[:, None] * 2.0 ** -24 * project64(indptr, indices, np.abs(np.asarray(values, dtype=np.float64)), shape[0], fx_abs)
    return first + U_OUT[out_dtype] * y_ref.abs() + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
