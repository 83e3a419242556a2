"""Generate tests/golden/truncation.pt by IMPORTING the Python reference's truncated residual (layers/residual.py TruncatedConnection with
its ProjectionGraphProvider and SparseProjector) and its models built with it, fp32, CPU.

As in make_golden_ens.py, parameters and inputs are not stored: they are drawn from seeded CPU generators in state_dict order
(``tests.transformer_helpers.fill``), which the tests repeat.  The fixture holds

  * ``graph``: the truncation node set and the two edge sets with their Gaussian weights (o8 data grid, 40-node O1 truncation grid, the 3
    nearest neighbours both ways - ``tests.truncation_helpers.synthetic_parts``) and a node attribute ``area_weight`` for both node sets;
  * ``providers``: the CSR arrays of the reference's ProjectionGraphProvider for the down and the up edge set - plain, row-normalised, with
    every third edge duplicated, with ``src_node_weight_attribute`` - and for the file mode (with and without row normalisation);
  * ``npz``: the bytes of two scipy ``.npz`` files (the un-normalised down and up matrices); the tests write them to a temporary directory;
  * ``layer``: TruncatedConnection(x) for ``n_step_output`` None and 2 (graph mode, row-normalised) and through the two files;
  * ``models``: per case of ``tests.truncation_helpers.MODEL_CASES`` the seeds, the state_dict keys / shapes, the parameter checksum, the
    noise the ensemble model drew, and the output - or the error text if the reference's own forward raises.

Runs only where the reference is available (ref_standins).   Usage:  python tests/golden/make_golden_truncation.py
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_standins as rs  # noqa: E402

rs.install()


def _schema_standins() -> None:
    """The reference's file mode imports its pydantic schema module (for the names of the on-the-fly keys), which wants ``typing.Self``
    (Python >= 3.11) and ``anemoi.utils.schemas.BaseModel``: both are given their documented meaning here, for this generator only."""
    import types
    import typing

    import pydantic
    import typing_extensions

    if not hasattr(typing, "Self"):
        typing.Self = typing_extensions.Self
    m = types.ModuleType("anemoi.utils.schemas")
    m.BaseModel = pydantic.BaseModel
    sys.modules["anemoi.utils.schemas"] = m


_schema_standins()

from anemoi.models.layers.graph_provider import ProjectionGraphProvider  # noqa: E402
from anemoi.models.layers.residual import TruncatedConnection  # noqa: E402
from make_golden import make_data_indices, make_hetero  # noqa: E402

from tests import truncation_helpers as H  # noqa: E402
from tests.transformer_helpers import fill  # noqa: E402


def hetero(g, pair, area):
    hd = make_hetero(g)
    hd["truncation"].x = torch.from_numpy(pair["latlon"])
    hd["truncation"].num_nodes = int(pair["latlon"].shape[0])
    hd["data"].area_weight, hd["truncation"].area_weight = area
    for key, k in ((H.DOWN, "down"), (H.UP, "up")):
        hd[key].edge_index = torch.from_numpy(pair[f"{k}_edge_index"])
        hd[key].gauss_weight = torch.from_numpy(pair[f"{k}_weight"])[:, None]
    return hd


def csr_of(provider) -> dict:
    m = provider.projection_matrix
    return dict(indptr=m.crow_indices().to(torch.int32), indices=m.col_indices().to(torch.int32), values=m.values().clone(), shape=tuple(m.shape))


def with_duplicates(hd, g, pair, area):
    """The same graph with every third edge of both sets repeated at the end (weights halved): duplicate entries must be summed."""
    dup = hetero(g, pair, area)
    for key in (H.DOWN, H.UP):
        ei, w = hd[key].edge_index, hd[key].gauss_weight
        dup[key].edge_index = torch.cat([ei, ei[:, ::3]], dim=1)
        dup[key].gauss_weight = torch.cat([w, 0.5 * w[::3]], dim=0)
    return dup


def gen_providers(hd, g, pair, area, files) -> dict:
    out = {}
    for k, key in (("down", H.DOWN), ("up", H.UP)):
        mk = lambda graph=hd, **kw: csr_of(ProjectionGraphProvider(graph=graph, edges_name=key, edge_weight_attribute="gauss_weight", **kw))  # noqa: E731
        out[k] = dict(plain=mk(), row_normalize=mk(row_normalize=True), duplicates=mk(graph=with_duplicates(hd, g, pair, area), row_normalize=True),
                      src_node_weight=mk(src_node_weight_attribute="area_weight", row_normalize=True), unit_weights=csr_of(
                          ProjectionGraphProvider(graph=hd, edges_name=key, edge_weight_attribute=None)),
                      file=csr_of(ProjectionGraphProvider(file_path=files[k])), file_row_normalize=csr_of(
                          ProjectionGraphProvider(file_path=files[k], row_normalize=True)))
    return out


def gen_model(name: str, case: dict, index: int, hd) -> dict:
    from anemoi.models.models import AnemoiEnsModelEncProcDec, AnemoiModelEncProcDec

    ens = case["model"] == "ens"
    cfg = H.model_config_of(case)
    torch.manual_seed(0)
    cls = AnemoiEnsModelEncProcDec if ens else AnemoiModelEncProcDec
    model = cls(model_config=rs.DotDict(cfg), data_indices=make_data_indices(H.N_VARS, H.N_PROG), statistics={"data": None},
                n_step_input=H.N_STEP_IN, n_step_output=case.get("n_step_output", 1), graph_data=hd).eval()
    assert type(model.residual["data"]).__name__ == "TruncatedConnection"
    param_seed, input_seed, noise_seed = 8000 + index, 8100 + index, 8200 + index
    psum = fill(model, param_seed)
    x = torch.randn(case["batch"], H.N_STEP_IN, case.get("members", 1), hd["data"].num_nodes, H.N_VARS,
                    generator=torch.Generator().manual_seed(input_seed))
    built = dict(case=case, param_seed=param_seed, input_seed=input_seed, param_sum=psum,
                 keys={k: tuple(v.shape) for k, v in model.state_dict().items()})
    drawn, real_randn = [], torch.randn

    def recording_randn(*a, **kw):
        t = real_randn(*a, **kw)
        drawn.append(t.clone())
        return t

    torch.manual_seed(noise_seed)
    torch.randn = recording_randn
    try:
        with torch.no_grad():
            y = model({"data": x}, fcstep=1)["data"] if ens else model({"data": x})["data"]
    except Exception as e:  # noqa: BLE001  (built, but the reference's own forward does not run: keep the error text instead of an output)
        print(name, "-> forward raised", type(e).__name__, e)
        return dict(built, forward_error=f"{type(e).__name__}: {' '.join(str(e).split())}")
    finally:
        torch.randn = real_randn
    print(name, tuple(y.shape), float(y.abs().max()))
    if ens:
        assert len(drawn) == 1
        built["noise"] = drawn[0]
    return dict(built, out=y.clone())


def main() -> None:
    import scipy.sparse as sp

    g, pair = H.synthetic_parts()
    gen = torch.Generator().manual_seed(77)
    area = (0.5 + torch.rand(g.num_data, generator=gen), 0.5 + torch.rand(pair["latlon"].shape[0], generator=gen))
    hd = hetero(g, pair, area)
    obj = {"graph": {"latlon": torch.from_numpy(pair["latlon"]), "data_area_weight": area[0], "truncation_area_weight": area[1],
                     **{f"{k}_{n}": torch.from_numpy(pair[f"{k}_{n}"]) for k in ("down", "up") for n in ("edge_index", "weight")}}}
    import tempfile

    tmp = tempfile.mkdtemp(prefix="truncation_")
    files, obj["npz"] = {}, {}
    for k, key in (("down", H.DOWN), ("up", H.UP)):
        ei, w = pair[f"{k}_edge_index"], pair[f"{k}_weight"]
        shape = (hd[key[2]].num_nodes, hd[key[0]].num_nodes)
        buf = io.BytesIO()
        sp.save_npz(buf, sp.coo_matrix((w, (ei[1], ei[0])), shape=shape, dtype=np.float32).tocsr())
        obj["npz"][k] = buf.getvalue()
        files[k] = os.path.join(tmp, f"{k}.npz")
        open(files[k], "wb").write(obj["npz"][k])
    obj["providers"] = gen_providers(hd, g, pair, area, files)
    x = torch.randn(2, H.N_STEP_IN, 1, g.num_data, H.N_VARS, generator=torch.Generator().manual_seed(8300))
    layer = TruncatedConnection(graph=hd, truncation_down_edges_name=H.DOWN, truncation_up_edges_name=H.UP, row_normalize=True)
    by_file = TruncatedConnection(truncation_config={"truncation_up_file_path": files["up"], "truncation_down_file_path": files["down"]},
                                  row_normalize=True)
    obj["layer"] = {"input_seed": 8300, "batch": 2, "out": layer(x).clone(), "out_2steps": layer(x, n_step_output=2).clone(),
                    "out_file": by_file(x).clone()}
    obj["models"], notes = {}, {}
    for i, (name, case) in enumerate(H.MODEL_CASES.items()):
        obj["models"][name] = gen_model(name, case, i, hd)
        if "forward_error" in obj["models"][name]:
            notes[name] = "the reference builds this model but its forward raises: " + obj["models"][name]["forward_error"]
    notes["file mode"] = ("generated with stand-ins for typing.Self and anemoi.utils.schemas.BaseModel (pydantic's), which the reference's "
                          "schema module imports")
    obj["notes"] = notes
    path = os.path.join(HERE, "truncation.pt")
    torch.save(obj, path)
    print(f"truncation.pt: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
