#!/usr/bin/env python
"""Device time of the ensemble model's conditional LayerNorm, fused against two-step, in one process (events around hipGraph replays):

(a) ``ops.cond_layer_norm_proj`` (one launch) against the path it replaces - pad + GEMM to a [N, 2D] modulation tensor + ``ops.cond_layer_norm``
    + the residual add, i.e. ``ConditionalLayerNorm.forward`` with the fused route forced off (a width the module does not route to the fused
    kernel is timed by calling the op directly, so that the figure behind the exclusion stays reproducible) - at N = 40 968 rows (4 members x 10 242),
    D in {512, 1024}, C in {4, 16, 32}, bf16, with a residual (the block tails' form) and without;
(b) a whole 4-member forward of the O96 -> res 5, 512-channel, 16-layer GraphTransformer ensemble model with the fused route on and forced off.

The two routes alternate (two-step, fused, two-step, fused, ...); the spread is taken from the repeated two-step runs of the same call.
Writes one JSON (default profiles/r08_ens_time.json).  usage: python tools/ens_time.py [--out PATH] [--kernel-only] [--repeats R]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemm_sweep import timeit  # noqa: E402

from anemoi_core_amd import ops  # noqa: E402
from anemoi_core_amd.layers.normalization import ConditionalLayerNorm  # noqa: E402

DEV, DT = "cuda", torch.bfloat16


class two_step:
    """ConditionalLayerNorm with the in-kernel modulation forced off: the GEMM + cond_layer_norm route (autograd's, and every wider C's)."""

    def __enter__(self):
        self.saved = ConditionalLayerNorm._proj_route_ok
        ConditionalLayerNorm._proj_route_ok = lambda self, x, cond: False

    def __exit__(self, *exc):
        ConditionalLayerNorm._proj_route_ok = self.saved


def alternate(fn, repeats, two_step_fn=None, **kw):
    """([two-step times], [fused times]) in us, alternating.  ``two_step_fn`` defaults to ``fn`` (a module call) with the route forced off."""
    a, b = [], []
    for _ in range(repeats):
        with two_step():
            a.append(timeit(two_step_fn or fn, **kw))
        b.append(timeit(fn, **kw))
    return a, b


def summary(two, fused):
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return dict(two_step_us=[round(t, 2) for t in two], fused_us=[round(t, 2) for t in fused], two_step_median_us=round(med(two), 2),
                fused_median_us=round(med(fused), 2), two_step_spread_us=round(max(two) - min(two), 2), ratio=round(med(two) / med(fused), 3),
                fused_slower_beyond_spread=bool(med(fused) > med(two) + (max(two) - min(two))))


def kernel_rows(repeats):
    out = []
    N = 40968
    for D in (512, 1024):
        for C in (4, 16, 32):
            torch.manual_seed(D + C)
            ln = ConditionalLayerNorm(D, condition_shape=C, zero_init=False).eval().to(DEV, DT)
            x, cond, res = torch.randn(N, D, device=DEV).to(DT), torch.randn(N, C, device=DEV).to(DT), torch.randn(N, D, device=DEV).to(DT)
            with torch.inference_mode():
                routed = ln._proj_route_ok(x, cond)  # False: the module keeps this width on the two-step route; the op is then timed directly
                w, b = ln._proj.get(ln)
            for with_res in (False, True):
                r = res if with_res else None
                with torch.inference_mode():
                    two, fused = alternate((lambda: ln(x, cond, r)) if routed else (lambda: ops.cond_layer_norm_proj(x, cond, w, b, ln.eps, r)), repeats,
                                           two_step_fn=lambda: ln(x, cond, r))
                row = dict(rows=N, D=D, C=C, residual=with_res, dtype="bf16", compulsory_MB=round(N * D * 2 * (3 if with_res else 2) / 1e6, 1),
                           module_route="fused" if routed else "two-step (width excluded by COND_PROJ_ROUTE_MAX)", **summary(two, fused))
                print(json.dumps(row), flush=True)
                out.append(row)
    return out


def model_row(repeats, members=4, channels=512, layers=16, heads=16):
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiEnsModelEncProcDec
    from anemoi_core_amd.models.configs import ens_model_config, make_data_indices

    g = build_synthetic_graph("o96", 5)
    n_vars, n_step = 101, 2
    torch.manual_seed(0)
    model = AnemoiEnsModelEncProcDec(model_config=ens_model_config("gt", channels, layers, heads, 8), data_indices=make_data_indices(n_vars, 90),
                                     statistics={"data": None}, n_step_input=n_step, n_step_output=1, graph_data=g).eval()
    with torch.no_grad():  # the conditioning must matter: zero-initialised modulation weights would time the same launches on zeros
        for name, p in model.named_parameters():
            if ".scale." in name or ".bias." in name:
                p.copy_(0.05 * torch.randn(p.shape))
    model = model.to(DEV, DT)
    x = {"data": torch.randn(1, n_step, members, g.num_data, n_vars, device=DEV).to(DT)}
    with torch.inference_mode():
        two, fused = alternate(lambda: model(x, fcstep=1), repeats, reps=3, replays=5)
    row = dict(graph="o96 -> res 5", data_nodes=g.num_data, hidden_nodes=g.num_hidden, members=members, channels=channels, layers=layers, dtype="bf16",
               cond_layer_norms_per_forward=2 * layers, **summary(two, fused))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08_ens_time.json"))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ens_time.py measures on the GPU; none is visible")
    result = dict(device=torch.cuda.get_device_name(0), blocks_per_cu_env=os.environ.get("ANEMOI_CLNP_BLOCKS_PER_CU"), kernel=kernel_rows(args.repeats))
    if not args.kernel_only:
        result["model"] = model_row(args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
