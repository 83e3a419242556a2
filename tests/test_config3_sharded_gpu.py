"""BASELINE config 3: the O96 GraphTransformer with the hidden mesh partitioned over 4 / 8 ranks (halo exchange per processor
layer, needed-rows exchange in the decoder), at FULL size and under test before an 8-GPU node ever sees it.

The P ranks share the one GPU of the test box; the kernels, the partition (`distributed/partition.py` = reference
`khop_edges.py:154-189`), the halo plans (`distributed/halo.py` = reference `halo.py:106-222`) and the exchange plans are the
product's.  The WIRE is a parameter: "host" = the debug gloo transport through host memory (the RCCL chain's stand-in, RCCL
refuses two ranks per device), "ipc" = the product's device-initiated exchange over hipIpc-mapped peer buffers
(`distributed/peer.py`), which is exactly what runs between 8 GPUs over xGMI.

Checked, for every rank's (replicated) output of the exact 16-layer benchmark model:
  * fp32: equal to the UNSHARDED HIP output within 2e-5 * s (s = max(1, max |ref|); the sharded GEMMs run other tile shapes on
    1.3 k rows than the unsharded ones on 10 k rows, so the K-sums are associated differently - bit-equality is reported, not
    required) and to `oracle.enc_proc_dec_forward` within 5e-5 * s (the unsharded model's own bound, test_fullsize_parity_gpu.py);
  * bf16: within the 16-bit bound of the unsharded model test (max 2e-2 * s, mean 5e-3) against the fp32 oracle on rounded values;
  * all ranks return bit-identical outputs (the output all-gather); a forward on a DIFFERENT input through the same receive
    buffers equals the unsharded forward on that input as well (fp32: bit for bit), and the first input repeated afterwards
    reproduces the first output;
  * N_halo per rank equals an independent count from the global edge list and lies in SURVEY.md §8(e)'s table
    (res 5: 277 at P = 2, 260-501 at P = 4, 188-517 at P = 8; res 6, P = 8: 338-1 066).
"""
import argparse
import os

import pytest
import torch

from tests.test_distributed_gpu import _spawn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SURVEY_HALO = {(5, 2): (277, 277), (5, 4): (260, 501), (5, 8): (188, 517), (6, 8): (338, 1066)}
WIRES = ["host", "ipc"]


def _args(hidden_res, layers):
    return argparse.Namespace(data_grid="o96", hidden_res=hidden_res, kind="gt", channels=512, layers=layers, heads=16, vars=84)


def _worker(rank, world, group, hidden_res, layers, dtype_names, wire):
    """One spawn serves every dtype of a (world, wire) case: the processes, the graph and the fp32 model are built once (the GPU
    suite's wall clock was mostly these spawns - VERDICT r3 item 6)."""
    import bench

    if wire == "ipc":
        from anemoi_core_amd.distributed import peer

        peer.install(group)
    g, model0, x = bench.build(_args(hidden_res, layers), DEV)
    state = {k: v.detach().clone() for k, v in model0.state_dict().items()}
    res = {}
    for dtype_name in dtype_names.split(","):
        dtype = getattr(torch, dtype_name)
        model0.load_state_dict(state)  # (a .to(bf16) rounded the parameters of the previous pass in place)
        model = model0.to(DEV).to(dtype)
        inp = {"data": x.to(DEV).to(dtype)}
        other = {"data": (x * 0.5 + 0.25).to(DEV).to(dtype)}
        with torch.inference_mode():
            y = model(inp, model_comm_group=group)["data"].clone()
            # a DIFFERENT input through the same receive buffers, then the first one again: rows left over from the previous forward
            # (a late peer, a stale cache line) cannot pass for the right ones, as they could with one input repeated
            y_other = model(other, model_comm_group=group)["data"].clone()
            y2 = model(inp, model_comm_group=group)["data"]  # every plan, channel and static cache reused
            torch.cuda.synchronize()
        plan = model.processor._halo_cache["plan"]
        res[dtype_name] = dict(out=y.float().cpu(), out_other=y_other.float().cpu() if rank in (0, world - 1) else None,
                               repeat_equal=bool(torch.equal(y, y2)), n_local=int(plan.info.num_local_nodes),
                               recv_counts=[int(c) for c in plan.recv_counts], send_counts=[int(c) for c in plan.send_counts])
        if wire == "ipc":  # the next dtype's rows have another width: its channels are new ones
            from anemoi_core_amd.distributed import peer

            torch.cuda.synchronize()
            peer.current().reset()
    return res


_REF: dict = {}


def _reference(hidden_res, layers, dtype):
    """(graph, unsharded HIP output, oracle output) of bench.py's model at this size - computed once per configuration."""
    key = (hidden_res, layers, dtype)
    if key not in _REF:
        import bench
        from oracle import gt_oracle as O

        g, model, x = bench.build(_args(hidden_res, layers), DEV)
        params = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if dtype != torch.float32:
            params = {k: (v.to(dtype).float() if v.is_floating_point() else v) for k, v in params.items()}
        m = model.to(DEV).to(dtype)
        with torch.inference_mode():
            hip = m({"data": x.to(DEV).to(dtype)})["data"].float().cpu()
            hip_other = m({"data": (x * 0.5 + 0.25).to(DEV).to(dtype)})["data"].float().cpu()
        del m
        torch.cuda.empty_cache()
        with torch.no_grad():
            want = O.enc_proc_dec_forward(params, dict(kind="gt", num_heads=16, num_layers=layers, num_channels=512), g,
                                          x.to(dtype).float())
        _REF[key] = (g, hip, want, hip_other)
    return _REF[key]


def _independent_halo_counts(g, world):
    """N_halo per rank from the GLOBAL dst-sorted edge list (oracle's integer restatement of halo.py:106-222)."""
    from oracle import gt_oracle as O

    ei = torch.from_numpy(g.proc_edge_index).long()
    dst_splits = O.balanced_partition_sizes(g.num_hidden, world)
    edge_splits = O.edge_splits_from_dst_sorted(ei, g.num_hidden, dst_splits)
    out = []
    for r in range(world):
        e0, d0 = sum(edge_splits[:r]), sum(dst_splits[:r])
        src = ei[0, e0:e0 + edge_splits[r]]
        out.append(int(src[(src < d0) | (src >= d0 + dst_splits[r])].unique().numel()))
    return dst_splits, out


def _check_run(outs, g, hip, want, hidden_res, world, dtype, hip_other):
    s = max(1.0, float(want.abs().max()))
    for r, o in enumerate(outs):
        assert o["repeat_equal"], f"rank {r}: the forward repeated after another input differs from the first"
        assert torch.equal(o["out"], outs[0]["out"]), f"rank {r}: gathered output differs from rank 0's"
        if o["out_other"] is not None:  # the forward on the OTHER input, first and last rank
            e = float((o["out_other"] - hip_other).abs().max())
            assert (e == 0.0) if dtype == torch.float32 else (e <= 2e-2 * max(1.0, float(hip_other.abs().max()))), (r, e)
    got = outs[0]["out"]
    assert got.shape == want.shape == (1, 1, 1, g.num_data, 84) and torch.isfinite(got).all()
    e_hip, e_or = (got - hip).abs(), (got - want).abs()
    print(f"[config3] res {hidden_res} P={world} {dtype}: vs unsharded HIP max {float(e_hip.max()):.3e} (bit-equal: {bool(torch.equal(got, hip))}), "
          f"vs oracle max {float(e_or.max()):.3e} mean {float(e_or.mean()):.3e} (ref max {s:.2f})")
    if dtype == torch.float32:
        assert float(e_hip.max()) <= 2e-5 * s and float(e_or.max()) <= 5e-5 * s
    else:
        assert float(e_or.max()) <= 2e-2 * s and float(e_or.mean()) <= 5e-3 * max(1.0, float(want.abs().mean()))
        assert float(e_hip.max()) <= 2e-2 * s
    # the partition and the halo sets
    dst_splits, halos = _independent_halo_counts(g, world)
    lo, hi = SURVEY_HALO[(hidden_res, world)]
    assert [o["n_local"] for o in outs] == dst_splits
    assert [sum(o["recv_counts"]) for o in outs] == halos
    assert min(halos) == lo and lo <= max(halos) <= hi, (halos, lo, hi)
    for r, o in enumerate(outs):  # what r receives from q is what q sends to r
        assert o["recv_counts"] == [outs[q]["send_counts"][r] for q in range(world)] and o["recv_counts"][r] == 0


# every (world, dtype) on the product wire; the host wire (RCCL's stand-in) at world 4 here and at world 8 through the bench entry
# point below - each case starts `world` processes that build the 16-layer model, the suite's wall clock is mostly these
# (the host wire - RCCL's stand-in - runs a 4-layer model here and the full path at world 8 through the bench entry point below: P processes
# time-slice ONE GPU, every exchange waits for its peers' slices, and the suite has a wall-clock budget - VERDICT r3 item 6)
@pytest.mark.parametrize("world,layers,dtypes,wire", [(4, 4, "float32", "host"), (4, 16, "float32", "ipc"), (8, 16, "float32,bfloat16", "ipc")])
def test_o96_res5_bench_model_sharded_equals_unsharded_and_oracle(world, layers, dtypes, wire):
    """(a) world 4 and 8, O96 -> res 5, the 16-layer 512-channel benchmark model (fp32 and bf16 share one 8-process spawn)."""
    outs = _spawn(_worker, world, 5, layers, dtypes, wire)
    for name in dtypes.split(","):
        dtype = getattr(torch, name)
        g, hip, want, hip_other = _reference(5, layers, dtype)
        _check_run([o[name] for o in outs], g, hip, want, 5, world, dtype, hip_other)


@pytest.mark.parametrize("wire", ["ipc"])
def test_o96_res6_two_layers_sharded_over_eight_ranks(wire):
    """(b) the res-6 variant of config 3 (40 962 hidden nodes, 5 121 + 338..1 058 rows per rank), 2 processor layers, bf16."""
    g, hip, want, hip_other = _reference(6, 2, torch.bfloat16)
    outs = _spawn(_worker, 8, 6, 2, "bfloat16", wire)
    _check_run([o["bfloat16"] for o in outs], g, hip, want, 6, 8, torch.bfloat16, hip_other)


@pytest.mark.parametrize("wire", WIRES)
def test_bench_entry_point_eight_ranks_on_one_gpu(wire):
    """(c) `python bench.py --gpus 8 --layers 2` as invoked, all ranks on the one GPU: n_gpus == 8, the sharded forward replays
    as hipGraph(s) equal to the eager forward; on the ipc wire the whole forward of a rank is ONE graph."""
    import json
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ANEMOI_BENCH_TRANSPORT=wire, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--layers", "2", "--no-cpu-baseline",
           "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=repo)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 8 and res["scaling"] == "strong" and res["value"] > 0
    assert res["rccl"]["world_size"] == 8 and res["rccl"]["halo_rows_recv"] == 188 and res["rccl"]["local_rows"] == 1281
    assert res["config"]["graph_equals_eager"] is True
    if wire == "ipc":
        assert res["config"]["graph_segments"] == 1, res["config"]
        # round 4: the wire check runs three inputs + a repeat before timing, every rank reports its halo rows and what its exchange
        # kernels spent waiting, and the same forward is ALSO timed over the collective chain (here: the host stand-in of RCCL)
        rc = res["rccl"]
        assert rc["wire_check"]["forwards"] == 4 and rc["wire_check"]["max_err_over_scale"] <= 2e-2
        assert len(rc["ranks"]) == 8 and all(188 <= r["n_halo"] <= 512 and r["timeout_peer"] is None and r["exchanges_per_forward"] > 0 for r in rc["ranks"])
        assert rc["ipc_status"] == "ok" and rc["ms_per_step_ipc"] > 0 and rc.get("ms_per_step_rccl", 0) > 0, rc
        assert rc["graph_segments_ipc"] == 1 and rc["graph_segments_rccl"] > 1
