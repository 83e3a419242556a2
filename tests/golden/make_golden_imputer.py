"""Generate tests/golden/imputer.pt by IMPORTING the Python reference's imputers (preprocessing/imputer.py: InputImputer, ConstantImputer,
CopyImputer), its ``Processors`` chain [imputer, normalizer] and one ``predict_step`` of its tiny model on a NaN-carrying batch, fp32, CPU.

The fixture holds data only:

  * ``indices`` / ``statistics`` / ``configs``: ONE index collection (7 variables; ``c`` diagnostic, ``e`` forcing - so the data order
    a b c d e f g and the model-input order a b d e f g differ from column 2 on), the statistics and the three processor configurations;
  * ``inputs``: seeded tiny inputs [2, 2, (2,) 7, width] for the training width (7) and the inference width (6), with and without an ensemble
    dimension, NaN planted by variable NAME (``NAN_PLAN`` below): at step 0 only, at step 1 only, in member 1 only, in a variable that is not
    imputed, in a forcing, in the diagnostic's training column;
  * ``cases[class][width key]``: the reference's ``transform`` output, ``nan_locations``, ``loss_mask_training`` and the ``inverse_transform``
    of a seeded output-width tensor - or ``error``: the text of what the reference raised (its ``transform`` raises on an ensemble dimension
    of 2: a boolean mask of member 0 does not broadcast; the ensemble dimension of 1 is recorded beside it);
  * ``chain``: the [imputer, normalizer] ``Processors`` pair, forward on an inference-width input, inverse on a model-output-width tensor;
  * ``predict_step``: the tiny model of ``edges.pt`` (its configuration, indices, statistics and parameters are READ from that fixture, not
    stored again) with pre = [InputImputer, InputNormalizer], post = the inverse pair: the NaN-carrying batch and the reference's output.

Runs only where the reference is available (ref_standins).   Usage:  python tests/golden/make_golden_imputer.py
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

from omegaconf import DictConfig  # noqa: E402

from anemoi.models.data_indices.collection import IndexCollection  # noqa: E402
from anemoi.models.preprocessing import Processors  # noqa: E402
from anemoi.models.preprocessing.imputer import ConstantImputer, CopyImputer, InputImputer  # noqa: E402
from anemoi.models.preprocessing.normalizer import InputNormalizer  # noqa: E402
from make_golden import make_hetero, model_config  # noqa: E402

from anemoi_core_amd.graphs.synthetic import build_synthetic_graph  # noqa: E402

NAMES = ["a", "b", "c", "d", "e", "f", "g"]
DATA_CFG = {"forcing": ["e"], "diagnostic": ["c"]}
CONFIGS = {
    "InputImputer": {"default": "none", "mean": ["a", "e"], "maximum": ["d"], "minimum": ["c"]},
    "ConstantImputer": {"default": "none", 1: ["a"], 3.14: ["d", "e"], -2.5: ["c"]},
    "CopyImputer": {"default": "none", "d": ["f", "a"]},
    "normalizer": {"default": "mean-std", "min-max": ["b"], "max": ["g"], "none": ["e"]},
}
# (variable, batch, step, member or None = all members, grid point); members other than 0 exist in the ensemble inputs only
NAN_PLAN = [
    ("a", 0, 0, None, 1),  # imputed, step 0 only
    ("a", 1, 1, None, 2),  # imputed, step 1 only
    ("d", 0, 0, None, 3), ("d", 0, 1, None, 3),  # imputed, both steps
    ("d", 1, 0, 1, 4),     # imputed, member 1 only: member 0 decides, so it STAYS NaN
    ("b", 0, 0, None, 5),  # not imputed
    ("e", 1, 0, None, 0),  # a forcing (imputed by the statistics and the constant imputer)
    ("c", 0, 0, None, 6),  # the diagnostic: its column exists at the training width only
    ("f", 0, 0, None, 2), ("f", 1, 1, None, 5),  # the copy imputer's own target
]
IMPUTED_ONLY = [p for p in NAN_PLAN if p[0] in ("a", "d", "e") and p[3] is None]  # what a forward chain may carry past its first-batch check


def index_dict(di):
    return dict(data_input_full=di.data.input.full.clone(), data_output_full=di.data.output.full.clone(),
                data_input_name_to_index=dict(di.data.input.name_to_index), data_output_name_to_index=dict(di.data.output.name_to_index),
                model_input_name_to_index=dict(di.model.input.name_to_index), model_output_name_to_index=dict(di.model.output.name_to_index),
                model_input_prognostic=di.model.input.prognostic.clone(), model_output_prognostic=di.model.output.prognostic.clone(),
                model_input_full=di.model.input.full.clone(), model_output_full=di.model.output.full.clone())


def plant(x, n2i, plan):
    for name, b, t, m, g in plan:
        if name not in n2i:
            continue
        if x.dim() == 4:
            if m is None:
                x[b, t, g, n2i[name]] = float("nan")
        elif m is None:
            x[b, t, :, g, n2i[name]] = float("nan")
        elif m < x.shape[2]:
            x[b, t, m, g, n2i[name]] = float("nan")
    return x


def record(fn):
    try:
        return fn()
    except Exception as e:  # noqa: BLE001 - the reference's own failure is the recorded behaviour
        return {"error": f"{type(e).__name__}: {e}"}


def main():
    gen = torch.Generator().manual_seed(2025)
    n2i = {n: i for i, n in enumerate(NAMES)}
    di = IndexCollection(DictConfig(DATA_CFG), n2i)
    stats = {k: (torch.randn(7, generator=gen, dtype=torch.float64) * s).numpy() for k, s in (("mean", 3.0), ("minimum", 5.0), ("maximum", 5.0))}
    stats["stdev"] = (torch.rand(7, generator=gen, dtype=torch.float64) + 0.5).numpy()
    widths = {"training": (n2i, len(di.data.output.name_to_index)), "inference": (dict(di.model.input.name_to_index), len(di.model.output.name_to_index))}
    out = dict(names=NAMES, data_config=DATA_CFG, configs=CONFIGS, indices=index_dict(di), statistics={k: torch.as_tensor(v) for k, v in stats.items()},
               nan_plan=NAN_PLAN, inputs={}, outputs={}, cases={})
    for wkey, (cols, w_out) in widths.items():
        for ens in (0, 1, 2):
            shape = (2, 2, ens, 7, len(cols)) if ens else (2, 2, 7, len(cols))
            key = wkey + (f"_ens{ens}" if ens else "")
            out["inputs"][key] = plant(2.0 * torch.randn(shape, generator=gen) + 0.5, cols, NAN_PLAN)
            oshape = (2, 1, ens, 7, w_out) if ens else (2, 1, 7, w_out)
            out["outputs"][key] = torch.randn(oshape, generator=gen)
    classes = {"InputImputer": InputImputer, "ConstantImputer": ConstantImputer, "CopyImputer": CopyImputer}
    for cname, cls in classes.items():
        out["cases"][cname] = {}
        for key, x in out["inputs"].items():
            def run(cls=cls, cname=cname, x=x, key=key):
                imp = cls(DictConfig(CONFIGS[cname]), di, stats if cname == "InputImputer" else None)
                y = imp.transform(x, in_place=False)
                res = dict(transform=y, nan_locations=imp.nan_locations.clone(),
                           loss_mask_training=None if imp.loss_mask_training is None else imp.loss_mask_training.clone(),
                           attributes={a: list(getattr(imp, a)) for a in ("index_training_input", "index_inference_input", "index_training_output",
                                                                           "index_inference_output", "replacement")},
                           state_dict_keys=list(imp.state_dict().keys()))
                res["inverse"] = record(lambda: imp.inverse_transform(out["outputs"][key], in_place=False))
                if x.dim() == 4:  # the stored [batch, grid, vars] mask is broadcast over whatever lies between batch and grid
                    res["inverse_ens2"] = record(lambda: imp.inverse_transform(out["outputs"][key + "_ens2"], in_place=False))
                return res
            out["cases"][cname][key] = record(run)
            got = out["cases"][cname][key]
            print(cname, key, got.get("error") or ("inverse: " + str(got["inverse"].get("error") if isinstance(got["inverse"], dict) else "ok")))

    # ---- the [imputer, normalizer] pair of Processors, both directions (inference width: what predict_step feeds it)
    cols = widths["inference"][0]
    x = plant(2.0 * torch.randn(2, 2, 1, 7, len(cols), generator=gen) + 0.5, cols, IMPUTED_ONLY)
    imp = InputImputer(DictConfig(CONFIGS["InputImputer"]), di, stats)
    nm = InputNormalizer(DictConfig(CONFIGS["normalizer"]), di, {k: v.copy() for k, v in stats.items()})
    pre = Processors([["imputer", imp], ["normalizer", nm]])
    post = Processors([["imputer", imp], ["normalizer", nm]], inverse=True)
    y = torch.randn(2, 1, 1, 7, widths["inference"][1], generator=gen)
    skip = Processors([["imputer", imp], ["normalizer", nm]])
    skip.first_run = False  # (its first-batch check would refuse the NaN that skip_imputation leaves in)
    out["chain"] = dict(x=x, forward=pre(x, in_place=False), nan_locations=imp.nan_locations.clone(), y=y, inverse=post(y, in_place=False),
                        forward_skip=skip(x, in_place=False, skip_imputation=True))

    # ---- predict_step of the reference's tiny model (configuration, indices, statistics, parameters: those of edges.pt)
    from anemoi.models.models import AnemoiModelEncProcDec

    c = torch.load(os.path.join(HERE, "edges.pt"), weights_only=False)["predict_step"]
    cfg = c["cfg"]
    g = build_synthetic_graph(cfg["data_grid"], cfg["hidden_resolution"])
    di2 = IndexCollection(data_config=DictConfig(c["data_config"]), name_to_index=c["name_to_index"])
    stats2 = {k: v.numpy().copy() for k, v in c["statistics"].items()}
    model = AnemoiModelEncProcDec(model_config=model_config(cfg["kind"], cfg["num_channels"], cfg["num_layers"], cfg["num_heads"], cfg["trainable"]),
                                  data_indices={"data": di2}, statistics={"data": stats2}, n_step_input=cfg["n_step_input"], n_step_output=1,
                                  graph_data=make_hetero(g)).eval()
    model.load_state_dict(c["params"], strict=True)
    imp_cfg = {"default": "none", "mean": ["v0", "v4"], "maximum": ["v3"]}
    imp2 = InputImputer(DictConfig(imp_cfg), di2, stats2)
    nm2 = InputNormalizer(DictConfig(c["data_config"]["normalizer"]), di2, {k: v.copy() for k, v in stats2.items()})
    pre2 = Processors([["imputer", imp2], ["normalizer", nm2]])
    post2 = Processors([["imputer", imp2], ["normalizer", nm2]], inverse=True)
    batch = c["batch"].clone()
    N = batch.shape[2]
    m2i = dict(di2.model.input.name_to_index)
    pts = torch.randperm(N, generator=gen)
    batch[0, 0, pts[:9], m2i["v0"]] = float("nan")       # step 0 (decides the restored NaN) ...
    batch[0, 1, pts[5:14], m2i["v0"]] = float("nan")     # ... and step 1, overlapping
    batch[0, :2, pts[20:27], m2i["v3"]] = float("nan")
    batch[0, 0, pts[30:33], m2i["v4"]] = float("nan")    # the forcing
    batch[0, 2, pts[40:44], m2i["v1"]] = float("nan")    # the spare time step predict_step does not read
    with torch.no_grad():
        y2 = model.predict_step({"data": batch}, {"data": pre2}, {"data": post2}, cfg["n_step_input"])["data"]
    out["predict_step"] = dict(imputer_config=imp_cfg, batch=batch, out=y2, nan_locations=imp2.nan_locations.clone())
    print("predict_step out", tuple(y2.shape), "NaN", int(y2.isnan().sum()), "finite mean", float(y2.nan_to_num().abs().mean()))

    path = os.path.join(HERE, "imputer.pt")
    torch.save(out, path)
    print(f"imputer.pt: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
