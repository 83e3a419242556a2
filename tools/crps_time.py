#!/usr/bin/env python
"""Device time and peak memory of the ensemble CRPS loss, forward + backward, at the O96 grid (40 320 points) x 84 variables, batch 1, one
output step, for E in {4, 8, 16} in fp32 and bf16, under three routes on the same inputs:

  kernels: ops.kernel_crps and its backward kernel (csrc/crps.hip) through autograd;
  stable : the reference's all-pairs formula restated in torch (pairwise [.., E, E] tensors), backward through autograd;
  naive  : the reference's loop over member pairs restated in torch (E - 1 shrinking slices), backward through autograd.

The restatements are the baseline, never the code under test.  The routes alternate; each figure is the median of --repeats windows of
--calls calls between device events after a warm-up, the spread is max - min of the windows.  Also: the forward kernels alone under
no_grad, and the bytes they must read, (E + 1) values per column, over that time against the 8 TB/s HBM peak.  No threshold: the numbers
are a record.  Writes one JSON (default profiles/crps_time.json).
usage: python tools/crps_time.py [--out PATH] [--repeats R] [--calls C] [--points N] [--vars V]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anemoi_core_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def restated(x, y, w, alpha, backend):
    """x [1, 1, E, N, V], y [1, 1, 1, N, V], w [N, V] -> the reference's loss (squash, "avg") with its tensor expressions."""
    E = x.shape[2]
    p, t = x.float().permute(0, 1, 4, 3, 2), y.float().permute(0, 1, 4, 3, 2).squeeze(-1)  # [.., V, N, E], [.., V, N]
    if backend == "naive":
        crps = (t[..., None] - p).abs().mean(-1)
        coef = -(alpha / (E * (E - 1)) + (1 - alpha) / E**2)
        var = torch.zeros_like(crps)
        for i in range(E - 1):
            var = var + (p[..., i].unsqueeze(-1) - p[..., i + 1:]).abs().sum(-1)
        crps = crps + coef * var
    else:
        var = (p.unsqueeze(-1) - p.unsqueeze(-2)).abs()
        err = (p - t.unsqueeze(-1)).abs().unsqueeze(-2).expand(*p.shape, E)
        mem = err * ~torch.eye(E, dtype=torch.bool, device=x.device)
        crps = (mem + mem.transpose(-1, -2) - (1 - (1 - alpha) / E) * var).sum((-1, -2)) / (2 * E * (E - 1))
    return (crps.permute(0, 1, 3, 2) * w).mean(-1).sum()


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crps_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--points", type=int, default=40320)
    ap.add_argument("--vars", type=int, default=84)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/crps_time.py measures on the GPU; none is visible")
    N, V, alpha = args.points, args.vars, 0.95
    torch.manual_seed(0)
    w_grid, w_var = torch.rand(N, device="cuda") / N, torch.rand(V, device="cuda") + 0.5
    w = w_grid[:, None] * w_var
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for E in (4, 8, 16):
            x = torch.randn(1, 1, E, N, V, device="cuda").to(dtype).requires_grad_()
            y = torch.randn(1, 1, 1, N, V, device="cuda").to(dtype)

            def step(loss_of):
                x.grad = None
                loss_of().backward()

            routes = dict(kernels=lambda: step(lambda: ops.kernel_crps(x, y, w_grid, alpha=alpha, w_var=w_var)),
                          stable=lambda: step(lambda: restated(x, y, w, alpha, "stable")),
                          naive=lambda: step(lambda: restated(x, y, w, alpha, "naive")))

            def forward():
                with torch.no_grad():
                    ops.kernel_crps(x, y, w_grid, alpha=alpha, w_var=w_var)

            for fn in (*routes.values(), forward):  # warm-up
                fn()
            grads = {}
            for name, fn in routes.items():
                fn()
                grads[name] = x.grad.float().clone()
            times = {name: [] for name in (*routes, "forward")}
            for _ in range(args.repeats):
                for name, fn in routes.items():
                    times[name].append(window_us(fn, args.calls if name == "kernels" else max(args.calls // 5, 2)))
                times["forward"].append(window_us(forward, args.calls))
            read = N * V * (E + 1) * x.element_size()
            fwd = med(times["forward"])
            row = dict(E=E, dtype=str(dtype).split(".")[-1], forward_bytes_read=read, forward_us=round(fwd, 1),
                       forward_spread_us=round(max(times["forward"]) - min(times["forward"]), 1), forward_bytes_per_s=round(read / (fwd * 1e-6), -9),
                       forward_share_of_hbm_peak=round(read / (fwd * 1e-6) / HBM_PEAK, 3),
                       kernels_gradient_apart_rel_max=float((grads["kernels"] - grads["stable"]).abs().max() / grads["stable"].abs().max()))
            for name, fn in routes.items():
                row[name] = dict(forward_backward_us=round(med(times[name]), 1), spread_us=round(max(times[name]) - min(times[name]), 1),
                                 peak_bytes=peak_bytes(fn))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x, y, grads
            torch.cuda.empty_cache()
    result = dict(device=torch.cuda.get_device_name(0), points=N, variables=V, batch=1, steps=1, alpha=alpha, hbm_peak_bytes_per_s=HBM_PEAK,
                  step="loss forward + backward to d_pred", repeats=args.repeats, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
