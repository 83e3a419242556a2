#!/usr/bin/env python
"""Device time of one TRAINING step of the EDM diffusion model - prepare (noise the target, loss weights), forward under autograd, the
weighted loss, backward - in one process, under two routes around the SAME network (O96 -> res 5, 512 channels, 16 layers, bf16 network,
fp32 data, batch 1):

  kernels : the product path - ops.noise_cond / ops.transport_assemble_input / ops.edm_output and their backward kernels
            (csrc/transport.hip, csrc/transport_bwd.hip) around the network;
  restated: the same three edges as differentiable torch operations (tests/transport_train_refs.py: restated_edges).  The baseline: not
            the code under test.

The routes alternate; each is timed as eager steps between synchronisations (host launch cost included) and, if the step can be
captured, as hipGraph replays between events; the spread is that of the repeated runs.  Also: the launches of either route around the
network in one step, and how far the two routes' gradients are apart.  No threshold: the number is a record.  Writes one JSON (default
profiles/r25_transport_train_time.json).
usage: python tools/transport_train_time.py [--out PATH] [--repeats R] [--layers L]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transport_time import DEV, build, count_launches, eager_us  # noqa: E402

from tests.transport_train_refs import restated_edges  # noqa: E402

EDGE_ENTRIES = ("anemoi_noise_cond_fwd", "anemoi_transport_assemble_input", "anemoi_edm_output", "anemoi_noise_cond_bwd",
                "anemoi_transport_assemble_input_bwd", "anemoi_edm_output_bwd")


def tally(lib_calls, torch_ops):
    from collections import Counter

    network = [n for n in lib_calls if n not in EDGE_ENTRIES] + [o for o in torch_ops if o.startswith("anemoi_hip.")]
    around = Counter(o for o in torch_ops if not o.startswith("anemoi_hip."))
    return dict(edge_kernels=[n for n in lib_calls if n in EDGE_ENTRIES], network_launches=len(network), torch_ops=sum(around.values()),
                torch_op_names=dict(sorted(around.items())))


def graph_us(fn, replays=5):
    """Device time of one captured step per replay, or the reason the capture failed."""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / replays
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {' '.join(str(e).split())[:200]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_transport_train_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/transport_train_time.py measures on the GPU; none is visible")
    model, g = build(512, args.layers, 16)
    model.training_condition = dict(distribution="karras", sigma_max=100.0, sigma_min=0.02, rho=7.0)
    x = torch.randn(1, 2, 1, g.num_data, 101, device=DEV)
    target = torch.randn(1, 1, 1, g.num_data, 90, device=DEV)
    source = torch.randn(1, 1, 1, g.num_data, 90, device=DEV)
    sigma = torch.tensor([3.0], device=DEV).view(1, 1, 1, 1, 1)  # fixed: both routes and every repeat take the same step

    def step():
        model.zero_grad(set_to_none=True)
        y_noised, s, w = model.prepare_edm_training({"data": target}, source={"data": source}, sigma={"data": sigma})
        D = model({"data": x}, y_noised, s)["data"]
        (w["data"] * (D - target) ** 2).mean().backward()

    def restated():
        with restated_edges():
            step()

    def grads(fn):
        fn()
        return {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None}

    gk, gr = grads(step), grads(restated)
    apart = max(float((gk[k] - gr[k]).abs().max() / gr[k].abs().max().clamp_min(1e-30)) for k in gk)
    lib_k, torch_k = count_launches(step)
    lib_r, torch_r = count_launches(restated)
    base_e, ours_e, base_g, ours_g = [], [], [], []
    for _ in range(args.repeats):
        base_e.append(eager_us(restated, calls=5))
        ours_e.append(eager_us(step, calls=5))
    for _ in range(args.repeats):
        base_g.append(graph_us(restated))
        ours_g.append(graph_us(step))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731

    def block(base, ours):
        if any(isinstance(t, str) for t in base + ours):
            return dict(capture_failed=[t for t in base + ours if isinstance(t, str)][0])
        return dict(restated=[round(t, 1) for t in base], kernels=[round(t, 1) for t in ours], restated_median=round(med(base), 1),
                    kernels_median=round(med(ours), 1), difference=round(med(base) - med(ours), 1),
                    spread=round(max(max(base) - min(base), max(ours) - min(ours)), 1))

    result = dict(device=torch.cuda.get_device_name(0), graph="o96 -> res 5", data_nodes=g.num_data, hidden_nodes=g.num_hidden, channels=512,
                  layers=args.layers, network_dtype="bf16", data_dtype="fp32", batch=1, step="prepare + forward + weighted loss + backward",
                  parameters_with_gradient=len(gk), routes_gradients_apart_rel_max=apart, eager_us=block(base_e, ours_e),
                  graph_replay_us=block(base_g, ours_g), launches=dict(kernels=tally(lib_k, torch_k), restated=tally(lib_r, torch_r)))
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
