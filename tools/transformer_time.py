"""Time the Transformer processor model and its window-attention kernel on one MI355X; prints ONE JSON line.

Default: O96 -> icosphere res 5 (10 242 hidden rows), GraphTransformer mappers around a 16-layer TransformerProcessor, 512 channels,
16 heads, window 512, bf16; the whole forward captured as a hipGraph, event-timed replays after warm-up.  Beside it, at the processor's
shape (q, k, v column slices of one [rows, 3A] buffer): the attention kernel alone (also captured, event-timed) at the configured
window and, for the band scaling, at window 256 / 512 / unbounded; and the same call's A/B against
torch.nn.functional.scaled_dot_product_attention with the reference's boolean band mask on the same q, k, v.

Floors (a cost model, not a measurement): the softmax's vector issue, SOFTMAX_CYCLES_PER_64 issue cycles per 64 scores on each of the
1 024 SIMDs at CLOCK_HZ, and the MFMAs, 4 * pairs * A flops at the dense bf16 peak.

    python tools/transformer_time.py [--channels 1024] [--hidden-res 6] [--window 512] [--layers 16] [--steps 20]
    python tools/transformer_time.py --backward --channels 1024 [--no-model]     (see backward_report)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from anemoi_core_amd import ops  # noqa: E402

SOFTMAX_CYCLES_PER_64 = 21  # fma 4 + exp 8 + max 2-4 + add 4 + cvt ~2
SIMDS, CLOCK_HZ, BF16_PEAK = 1024, 2.4e9, 2.5e15


def band_pairs(n: int, w) -> int:
    """(i, j) pairs with |i - j| <= w in a sequence of n."""
    if w is None or w < 0 or w >= n:
        return n * n
    return n * (2 * w + 1) - w * (w + 1)


def timed(fn, steps: int, warmup: int = 3) -> float:
    """ms per call of fn captured as a hipGraph, event-timed over ``steps`` replays."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def eager_ms(fn, steps: int) -> float:
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def backward_report(args) -> dict:
    """``--backward``: the window attention's forward, its backward and each backward pass alone (csrc/window_attention_bwd.hip), as
    hipGraph replays, at the hidden meshes of res 5 and 6 (10 242 and 40 962 rows), window ``--window`` and unbounded, bf16; then one
    training step (forward + backward of the whole model, bf16 parameters, fp32 batch) of the O96 -> res ``--hidden-res`` model."""
    dev, dt = "cuda", torch.bfloat16
    H, A = args.heads, args.channels
    res: dict = dict(tool="transformer_time --backward", channels=A, heads=H, head_dim=A // H, dtype="bf16", device=torch.cuda.get_device_name(),
                     shapes=[])
    for N in (10 * 4 ** 5 + 2, 10 * 4 ** 6 + 2):
        torch.manual_seed(0)
        buf = torch.randn(N, 3 * A, device=dev, dtype=dt)
        q, k, v = buf[:, :A], buf[:, A:2 * A], buf[:, 2 * A:]
        d_out = torch.randn(N, A, device=dev, dtype=dt)
        grad = torch.empty_like(buf)
        grads = (grad[:, :A], grad[:, A:2 * A], grad[:, 2 * A:])
        delta = torch.empty(N, H, device=dev, dtype=torch.float32)
        for w in (args.window, None):
            out, lse = ops.window_attention(q, k, v, H, w, return_lse=True)
            bwd = lambda passes, w=w, out=out, lse=lse: ops.window_attention_bwd(d_out, q, k, v, out, lse, H, w, grads_out=grads,  # noqa: E731
                                                                                 delta=delta, passes=passes)
            bwd(ops.WINDOW_BWD_QUERY_PASS)  # the key pass alone reads this delta
            # a timed window of about half a second each: the replay count follows a three-replay estimate
            long_enough = lambda fn: timed(fn, max(args.steps, min(5000, int(500.0 / timed(fn, 3)))))  # noqa: E731
            us = {name: round(long_enough(fn) * 1e3, 1) for name, fn in (
                ("forward", lambda w=w: ops.window_attention(q, k, v, H, w, return_lse=True)),
                ("backward", lambda: bwd(ops.WINDOW_BWD_QUERY_PASS | ops.WINDOW_BWD_KEY_PASS)),
                ("query_pass", lambda: bwd(ops.WINDOW_BWD_QUERY_PASS)),
                ("key_pass", lambda: bwd(ops.WINDOW_BWD_KEY_PASS)))}
            pairs = band_pairs(N, w)
            res["shapes"].append(dict(rows=N, window="none" if w is None else w, band_pairs=pairs, us=us,
                                      backward_over_forward=round(us["backward"] / us["forward"], 2),
                                      forward_tflops=round(4.0 * pairs * A / (us["forward"] * 1e-6) / 1e12, 1),
                                      backward_tflops=round(14.0 * pairs * A / (us["backward"] * 1e-6) / 1e12, 1)))
        del buf, grad
    if not args.no_model:
        from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
        from anemoi_core_amd.models import AnemoiModelEncProcDec
        from anemoi_core_amd.models.configs import make_data_indices, model_config

        g = build_synthetic_graph("o96", args.hidden_res, processor_edges=False)
        n_vars, n_step = 84, 2
        model = AnemoiModelEncProcDec(model_config=model_config("transformer", A, args.layers, H, 8, window_size=args.window),
                                      data_indices=make_data_indices(n_vars, n_vars), statistics={"data": None}, n_step_input=n_step,
                                      n_step_output=1, graph_data=g).train().to(dev, dt)
        x = {"data": torch.randn(1, n_step, 1, g.num_data, n_vars, device=dev)}

        def step():
            model.zero_grad(set_to_none=True)
            model(x)["data"].float().square().mean().backward()

        res.update(train_step_ms=round(timed(step, args.steps), 3), train_step_rows=g.num_hidden, train_step_layers=args.layers,
                   train_step_window=args.window)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--hidden-res", type=int, default=5)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="the attention kernel alone")
    ap.add_argument("--backward", action="store_true", help="time the attention's backward passes and one training step instead")
    args = ap.parse_args()
    if args.backward:
        print(json.dumps(backward_report(args)))
        return
    dev, dt = "cuda", torch.bfloat16
    H, A = args.heads, args.channels
    d = A // H
    res: dict = dict(tool="transformer_time", channels=A, heads=H, head_dim=d, window=args.window, hidden_res=args.hidden_res,
                     layers=args.layers, dtype="bf16", device=torch.cuda.get_device_name())

    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph

    g = build_synthetic_graph("o96", args.hidden_res, processor_edges=False)
    N = g.num_hidden
    res["rows"] = N

    # ---- the kernel alone at the processor's shape
    torch.manual_seed(0)
    buf = torch.randn(N, 3 * A, device=dev, dtype=dt)
    q, k, v = buf[:, :A], buf[:, A:2 * A], buf[:, 2 * A:]
    kern = {}
    for w in sorted({args.window, 256, 512}) + [None]:
        ms = timed(lambda w=w: ops.window_attention(q, k, v, H, w), args.steps)
        kern["none" if w is None else str(w)] = round(ms * 1e3, 2)
    res["attention_us_by_window"] = kern
    us = kern[str(args.window)]
    pairs = band_pairs(N, args.window)
    scores = pairs * H
    floor_sm = scores / 64 * SOFTMAX_CYCLES_PER_64 / (SIMDS * CLOCK_HZ) * 1e6
    floor_mfma = 4.0 * pairs * A / BF16_PEAK * 1e6
    res.update(attention_us_per_layer=us, band_pairs=pairs, scores=scores, scores_per_s=scores / (us * 1e-6),
               tflops=4.0 * pairs * A / (us * 1e-6) / 1e12, floor_softmax_issue_us=round(floor_sm, 2), floor_mfma_us=round(floor_mfma, 2),
               share_of_softmax_floor=round(floor_sm / us, 3), share_of_mfma_floor=round(floor_mfma / us, 3),
               band_scaling={"w256_over_w512": round(kern["256"] / kern["512"], 3), "w512_over_unbounded": round(kern["512"] / kern["none"], 3)})

    # ---- the same call's A/B: SDPA with the reference's boolean band mask on the same q, k, v
    q4, k4, v4 = (t.reshape(N, H, d).transpose(0, 1).unsqueeze(0) for t in (q, k, v))
    i = torch.arange(N, device=dev)
    mask = (i[:, None] - i[None, :]).abs() <= args.window
    sdpa = eager_ms(lambda: torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask), max(3, args.steps // 4)) * 1e3
    ours = ops.window_attention(q, k, v, H, args.window)
    ref = torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask)[0].transpose(0, 1).reshape(N, A)
    res.update(sdpa_masked_us=round(sdpa, 1), speedup_vs_sdpa=round(sdpa / us, 2),
               max_abs_diff_vs_sdpa=float((ours.float() - ref.float()).abs().max()))
    del mask, ref

    # ---- the whole forward
    if not args.no_model:
        from anemoi_core_amd.models import AnemoiModelEncProcDec
        from anemoi_core_amd.models.configs import make_data_indices, model_config

        n_vars, n_step = 84, 2
        model = AnemoiModelEncProcDec(model_config=model_config("transformer", A, args.layers, H, 8, window_size=args.window),
                                      data_indices=make_data_indices(n_vars, n_vars), statistics={"data": None}, n_step_input=n_step,
                                      n_step_output=1, graph_data=g).eval().to(dev, dt)
        x = {"data": torch.randn(1, n_step, 1, g.num_data, n_vars, device=dev, dtype=dt)}
        with torch.no_grad():
            res["forward_ms"] = round(timed(lambda: model(x), args.steps), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
