"""CPU checks of the chain kernels' dispatch (csrc/chain_plan.h) through its host-only query, ops.chain_plan -> anemoi_chain_plan: which
kernel, rows per panel, grid, threads and LDS size every shape gets, and which shapes each entry point takes.  No GPU: the query launches
nothing."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from anemoi_core_amd import _lib

from . import chain_refs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ANEMOI_CHAIN_ROWS", "ANEMOI_GNN_NODE_ROWS", "ANEMOI_CHAIN2_EVEN_GRID", "ANEMOI_CHAIN2_MAX_GRID")
DTYPES = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}

# tests/golden/chain_plan_recorded.json -> RECORDED["default" | "ANEMOI_CHAIN_ROWS=17" | "ANEMOI_CHAIN_ROWS=60"]: one row per call,
#   [kind, call, return code, launch]
# RECORDED from the dispatch as it stood before plan_chain existed (the commit under "parent"): the chain entry points of that commit, compiled
# for the host with hipLaunchKernelGGL replaced by a recorder and called with operands that are never dereferenced
# (tools/chain_args_check.cpp and tools/chain2_side_args_check.cpp, --record) - never regenerated from plan_chain.
#   call    block_tail [n_rows, hidden, q_out, rows_per_tile, dtype]      cluster [n_rows, hidden, q_out, dtype]
#           row_chain [n_rows, in_features, q_out, rows_per_tile, dtype]  row_chain_panels [n_rows, in_features, q_out, first, panels, dtype]
#           embed_fold [n_rows, in_features, q_out, dtype]                gnn_edge / gnn_node [n_rows, dtype]    gnn_mlp [n_rows, in_features, dtype]
#           block_tail_side [host rows, hidden, q_out, rows_per_tile, side rows, in_features, q_out, rows_per_tile, first, panels, cap, dtype]
#           (dtype: 0 fp32, 1 bf16, 2 f16)
#   launch  None: nothing launched;  "tail_alone": the side entry point handed the call to anemoi_gt_chain2_fwd;  else
#           [kernel instantiation, grid, threads, LDS bytes, rows per panel, panels, rows of the launch, its first row (panel ranges),
#            host_grid, riders, first, end, riders pipelined (side launches; 0, 0, 0, 0, -1 otherwise)]
# The row counts are those at which some rule flips (0, 1, 47, 48, 49, 255 * 48 (+ 1), 256 * 48 +- 1, 12336, 2 * 256 * 48 (+ 1), 10242, 40320,
# 40962, 542080); the other axes are listed in the two programs' main().  The rows under a switch were recorded with it set.
# The file stores the rows grouped, one group per line: [kind, the call without its varying fields, [[varying fields..., return code,
# launch...], ...]].  The varying fields are n_rows (first, panels of a panel range; first, panels, cap of a side job).  A launch is
# [index into "kernels" = (instantiation, threads, LDS bytes), grid, rows per panel, panels (, rows, first row of a panel range)]; it is absent
# for None and -1 for "tail_alone".  A side job's launch is [riders]: what all launches of its group share stands once behind the group,
# [rows per panel, panels, rows, host_grid, kernel index, riders pipelined], and grid = host_grid + riders, first, end = first + panels
# held for every recorded row when the file was written.
_VARY = {"row_chain_panels": (3, 4), "block_tail_side": (8, 9, 10)}


def _rows(stored, groups):
    out = []
    for kind, fixed, entries, *tail in groups:
        vary = _VARY.get(kind, (0,))
        for e in entries:
            it, iv = iter(fixed), iter(e)
            call = [next(iv) if i in vary else next(it) for i in range(len(fixed) + len(vary))]
            rc, rest = e[len(vary)], e[len(vary) + 1:]
            launch = None
            if rest == [-1]:
                launch = "tail_alone"
            elif rest and kind == "block_tail_side":
                rpt, panels, rows, hg, ki, pipe = tail[0]
                name, threads, lds = stored["kernels"][ki]
                launch = [name, hg + rest[0], threads, lds, rpt, panels, rows, 0, hg, rest[0], call[8], call[8] + call[9], pipe]
            elif rest:
                name, threads, lds = stored["kernels"][rest[0]]
                launch = [name, rest[1], threads, lds, rest[2], rest[3]] + (rest[4:6] if kind == "row_chain_panels" else [call[0], 0]) + [0, 0, 0, 0, -1]
            out.append([kind, call, rc, launch])
    return out


_STORED = json.load(open(os.path.join(REPO, "tests", "golden", "chain_plan_recorded.json")))
RECORDED = {k: _rows(_STORED, v) for k, v in _STORED.items() if k not in ("parent", "kernels")}
CROSS_COUNTS = (0, 1, 49, 256 * 48, 256 * 48 + 1, 40962, 542080)  # the cross products of the widths stand at these; a kind's main shape at every count
ROW_COUNTS = (0, 1, 47, 48, 49, 255 * 48, 255 * 48 + 1, 256 * 48 - 1, 256 * 48, 256 * 48 + 1, 12336, 2 * 256 * 48, 2 * 256 * 48 + 1, 10242, 40320, 40962, 542080)


@pytest.fixture(scope="module")
def ops():
    for name in SWITCHES:
        assert name not in os.environ, f"the recorded plans are those of the default switches: unset {name}"
    if not os.path.exists(_lib.LIB_PATH):
        from anemoi_core_amd.build import build_library

        build_library(verbose=False)
    from anemoi_core_amd import ops as _ops

    return _ops


def _query(ops, kind, call):
    """ops.chain_plan for a recorded call -> (return code, plan or None)"""
    dt = DTYPES[call[-1]]
    if kind == "block_tail":
        kw = dict(kind="block_tail", n_rows=call[0], hidden=call[1], q_out=call[2], rows_per_tile=call[3])
    elif kind == "cluster":
        kw = dict(kind="cluster_tail", n_rows=call[0], hidden=call[1], q_out=call[2])
    elif kind == "row_chain":
        kw = dict(kind="row_chain", n_rows=call[0], in_features=call[1], q_out=call[2], rows_per_tile=call[3])
    elif kind == "row_chain_panels":
        kw = dict(kind="row_chain_panels", n_rows=call[0], in_features=call[1], q_out=call[2], first_panel=call[3], panels=call[4])
    elif kind == "embed_fold":
        kw = dict(kind="embed_fold", n_rows=call[0], in_features=call[1], q_out=call[2])
    elif kind == "gnn_mlp":
        kw = dict(kind="gnn_mlp", n_rows=call[0], in_features=call[1])
    elif kind in ("gnn_edge", "gnn_node"):
        kw = dict(kind=kind, n_rows=call[0])
    else:
        assert kind == "block_tail_side", kind
        kw = dict(kind=kind, n_rows=call[0], hidden=call[1], q_out=call[2], rows_per_tile=call[3],
                  side=ops.ChainSideShape(rows=call[4], in_features=call[5], q_out=call[6], rows_per_tile=call[7], first_panel=call[8], panels=call[9], cap=call[10]))
    try:
        p = ops.chain_plan(kw.pop("kind"), kw.pop("n_rows"), dtype=dt, **kw)
    except ValueError:
        return _lib.E_INVALID, None
    return (_lib.E_UNSUPPORTED, None) if p is None else (0, p)


def _as_recorded(ops, kind, call):
    """the plan in the shape of a recorded row's [return code, launch]"""
    rc, p = _query(ops, kind, call)
    if rc != 0 or p.kernel == "none":
        return [rc, None]
    if kind == "block_tail_side":
        if p.riders == 0:
            return [rc, "tail_alone"]
        return [rc, [p.kernel, p.grid, p.threads, p.lds_bytes, p.rows_per_panel, p.panels, p.n_rows, 0, p.host_grid, p.riders, p.first, p.end, int(p.side_pipelined)]]
    if kind == "embed_fold":  # (its argument block carries no panels)
        return [rc, [p.kernel, p.grid, p.threads, p.lds_bytes, 0, 0, p.n_rows, 0, 0, 0, 0, 0, -1]]
    return [rc, [p.kernel, p.grid, p.threads, p.lds_bytes, p.rows_per_panel, p.panels, p.n_rows, p.row_begin, 0, 0, 0, 0, -1]]


def _wrong(ops, rows):
    return [(kind, call, got, [rc, launch]) for kind, call, rc, launch in rows if (got := _as_recorded(ops, kind, call)) != [rc, launch]]


def test_recorded_plans(ops):
    wrong = _wrong(ops, RECORDED["default"])
    assert not wrong, (len(wrong), wrong[:10])


def test_a_hosted_tail_is_the_tail_alone(ops):
    """where the side entry point hands the call on, and where it launches the tail with riders, the tail's own geometry is that of
    anemoi_gt_chain2_fwd for the same rows"""
    n = 0
    for kind, call, rc, launch in RECORDED["default"]:
        if kind == "block_tail_side" and rc == 0:
            side = _query(ops, kind, call)[1]
            tail = ops.chain_plan("block_tail", call[0], hidden=call[1], q_out=call[2], rows_per_tile=call[3], dtype=DTYPES[call[-1]])
            assert (side.host_grid, side.rows_per_panel, side.panels, side.rounds, side.idle_cus) == (tail.grid, tail.rows_per_panel, tail.panels, tail.rounds, tail.idle_cus)
            assert side.grid == tail.grid + side.riders <= 256 and (side.kernel == tail.kernel) == (side.riders == 0)
            n += 1
    assert n > 1000


def test_the_table_covers_what_the_dispatch_branches_on():
    rows = {(kind, tuple(call)): (rc, launch) for kind, call, rc, launch in RECORDED["default"]}
    assert len(rows) == len(RECORDED["default"])
    full, part, side = "gt_chain2_kernel", "gt_chain2_kernel<false,true>", "gt_chain2_kernel<false,true,true>"
    for n in ROW_COUNTS:
        assert ("block_tail", (n, 2048, 2048, 0, 1)) in rows and ("row_chain", (n, 192, 512, 0, 1)) in rows and ("embed_fold", (n, 64, 512, 1)) in rows
        assert all((kind, (n, 1)) in rows for kind in ("gnn_edge", "gnn_node")) and ("gnn_mlp", (n, 512, 1)) in rows
    for n in CROSS_COUNTS:
        for hidden in (512, 2048, 4096):
            for q in (0, 128, 256, 384, 512, 2048, 3072, 3584):
                rc, launch = rows[("block_tail", (n, hidden, q, 0, 1))]
                want = 0 if n == 0 or 1024 + hidden + q <= 6144 else _lib.E_UNSUPPORTED
                assert rc == want and (launch is None) == (n == 0 or rc != 0)
        for rpt in (17, 41, 48):
            rc, launch = rows[("block_tail", (n, 2048, 2048, rpt, 1))]
            assert rc == 0 and (n == 0 or launch[4:6] == [rpt, -(-n // rpt)])
        for bad in ((n, 2048, 2048, 49, 1), (n, 2000, 0, 0, 1), (n, 2048, 100, 0, 1), (n, 2048, 2048, 0, 0)):
            assert rows[("block_tail", bad)][0] == (0 if n == 0 and bad[-1] == 1 else _lib.E_INVALID), bad
        for k_in in (8, 128, 192, 256, 264, 512, 100, 520):
            for q in (512, 2048, 2560):
                rc, launch = rows[("row_chain", (n, k_in, q, 0, 1))]
                assert rc == (0 if n == 0 or (k_in not in (100, 520) and q != 2560) else _lib.E_INVALID)
        for k_in in (8, 64, 72, 256, 264):
            for q in (512, 2048, 2560):
                assert rows[("embed_fold", (n, k_in, q, 1))][0] == (0 if k_in != 264 and q != 2560 else _lib.E_UNSUPPORTED)
    # the kernel of a block tail flips at 256 panels, its grid evens out the rounds beyond
    tails = {n: rows[("block_tail", (n, 2048, 2048, 0, 1))][1][:2] for n in ROW_COUNTS[1:]}
    assert tails == {1: [part, 1], 47: [part, 1], 48: [part, 1], 49: [part, 2], 12240: [part, 255], 12241: [full, 256], 12287: [full, 256], 12288: [full, 256],
                     12289: [part, 129], 12336: [part, 129], 24576: [full, 256], 24577: [part, 171], 10242: [part, 214], 40320: [part, 210],
                     40962: [part, 214], 542080: [part, 251]}
    # the row chain is pipelined from 257 panels on, up to 256 input columns
    for k_in, pipe in ((8, True), (192, True), (256, True), (264, False), (512, False)):
        assert rows[("row_chain", (12289, k_in, 512, 0, 1))][1][0] == ("gt_rowchain_pipe_kernel" if pipe else "gt_rowchain_kernel")
        assert rows[("row_chain", (12288, k_in, 512, 0, 1))][1][0] == "gt_rowchain_kernel"
    # a panel range takes the schedule of the whole job: first, middle and last panel of 1, 256, 257 and 840 panels, the last one ragged
    for job in (1, 256, 257, 840):
        n = job * 48 - 5
        for k_in in (192, 256, 264, 512):
            for first in (0, job // 2, job - 1):
                rc, launch = rows[("row_chain_panels", (n, k_in, 1024, first, 1, 1))]
                assert rc == 0 and launch[0] == ("gt_rowchain_pipe_kernel" if job > 256 and k_in <= 256 else "gt_rowchain_kernel")
                assert launch[1] == 1 and launch[6:8] == [43 if first == job - 1 else 48, first * 48]
            assert rows[("row_chain_panels", (n, k_in, 1024, job - 1, 2, 1))] == (_lib.E_INVALID, None)
    # the cluster: 1, 8, 9, 64 and 65 panels
    assert [rows[("cluster", (p * 48, 2048, 512, 1))][1][1] for p in (1, 8, 9, 64, 65)] == [32, 32, 64, 256, 256]
    assert rows[("cluster", (48, 512, 0, 1))][0] == _lib.E_UNSUPPORTED and rows[("cluster", (48, 2048, 2560, 1))][0] == _lib.E_INVALID
    # side jobs: the width at which the riders stop being pipelined, the refusals
    for k_in, pipe in ((192, 1), (256, 1), (264, 0)):
        launch = rows[("block_tail_side", (10242, 2048, 2048, 0, 40320, k_in, 1024, 0, 0, 4, 0, 1))][1]
        assert launch[0] == side and launch[-1] == pipe and launch[8:12] == [214, 4, 0, 4]
    assert rows[("block_tail_side", (12288, 2048, 2048, 0, 347, 192, 1024, 0, 0, 8, 0, 1))][0] == _lib.E_UNSUPPORTED  # no idle compute unit
    assert rows[("block_tail_side", (149, 2048, 2048, 0, 347, 100, 1024, 0, 0, 8, 0, 1))][0] == _lib.E_UNSUPPORTED    # the side job's width
    assert rows[("block_tail_side", (149, 2048, 2048, 0, 347, 192, 1024, 0, 3, 6, 0, 1))][0] == _lib.E_INVALID        # range beyond the job
    for n in chain_refs.LADDER_EDGE:
        assert ("gnn_edge", (n, 1)) in rows and ("gnn_mlp", (n, 512, 1)) in rows
    for n in chain_refs.LADDER_NODE:
        assert ("gnn_node", (n, 1)) in rows


def test_graphconv_plans_are_the_restated_panel_split(ops):
    """tests/chain_refs.py panel_split is the tests' independent restatement of the GraphConv chains' geometry: field by field"""
    for kind, cap, ladder in (("gnn_edge", 64, chain_refs.LADDER_EDGE), ("gnn_mlp", 64, chain_refs.LADDER_EDGE), ("gnn_node", 48, chain_refs.LADDER_NODE)):
        for n in ladder + ROW_COUNTS[1:]:
            p = ops.chain_plan(kind, n, in_features=512)
            rows, tiles, last, grid, per_wg = chain_refs.panel_split(n, cap)
            assert (p.rows_per_panel, p.panels, n - (p.panels - 1) * p.rows_per_panel, p.grid, p.rounds) == (rows, tiles, last, grid, per_wg), (kind, n)
            assert p.idle_cus == 256 - grid and p.threads == 512


def test_supported_predicates_are_the_plans_answer(ops):
    """ops.<kind>_supported on a GPU tensor of the recorded shape says what the recorded entry point said (rows that come as CPU tensors,
    as in tests/test_round6_host_cpu.py, are refused whatever the shape)"""
    def rows_like(n, cols, dt, cuda=True):  # what the predicates look at, without a device
        return SimpleNamespace(is_cuda=cuda, dtype=DTYPES[dt], shape=(n, cols), dim=lambda: 2, stride=lambda i: (-(-cols // 8) * 8, 1)[i])  # (a row stride the kernels take)

    n_true = {"block_tail": 0, "cluster": 0, "row_chain": 0, "embed_fold": 0}
    for kind, call, rc, _ in RECORDED["default"]:
        if kind not in n_true or call[0] < 0 or call[-1] == 0:
            continue
        if kind == "block_tail" and call[3] == 0:
            got = ops.gt_layer_chain2_supported(rows_like(call[0], 512, call[-1]), call[1], call[2])
            assert not ops.gt_layer_chain2_supported(rows_like(call[0], 512, call[-1], cuda=False), call[1], call[2])
        elif kind == "cluster":
            got = ops.gt_cluster_chain_supported(rows_like(call[0], 512, call[-1]), call[1], call[2])
        elif kind == "row_chain" and call[3] == 0 and call[1] > 0:
            got = ops.gt_row_chain_supported(rows_like(call[0], call[1], call[-1]), call[2])
        elif kind == "embed_fold" and call[1] > 0:
            got = ops.gt_embed_fold_supported(rows_like(call[0], call[1], call[-1]), call[2])
        else:
            continue
        assert got == (rc == 0) == (_query(ops, kind, call)[0] == 0), (kind, call, got, rc)
        n_true[kind] += got
    assert all(v > 40 for v in n_true.values()), n_true


def test_idle_cus_and_side_schedule_come_from_the_plan(ops):
    from anemoi_core_amd.layers.handoff import side_schedule

    for n in ROW_COUNTS[1:]:
        p = ops.chain_plan("block_tail", n, hidden=2048, q_out=2048)
        assert ops.chain_idle_cus(n) == p.idle_cus == 256 - p.grid
        assert side_schedule(n, 10 ** 6, 3) == p.idle_cus * 3 * p.rounds
    assert ops.chain_idle_cus(0) == 0 and side_schedule(0, 100, 4) == 0
    assert ops.row_chain_panels(840 * 48 - 5, 8, 1024) == 840


def test_query_checks_its_arguments(ops):
    with pytest.raises(ValueError):
        ops.chain_plan("block_tail", -1, hidden=2048)
    with pytest.raises(ValueError):
        ops.chain_plan("block_tail", 100, hidden=2048, dtype=torch.float32)
    with pytest.raises(ValueError):
        ops.chain_plan("no_such_kind", 100)
    assert ops.chain_plan("block_tail", 0, hidden=2048).kernel == "none"
    assert ops.chain_plan("block_tail", 100, hidden=2048, timeline=True) is None  # the product library carries no instrumented kernel


_CHILD = """
import json, sys
sys.path.insert(0, {repo!r})
from tests import test_chain_plan_cpu as t
from anemoi_core_amd import ops
print(json.dumps([[k, c, len(t._wrong(ops, t.RECORDED[k]))] for k in t.RECORDED if k.startswith("ANEMOI_CHAIN_ROWS=")
                  for c in [ops.chain_plan("block_tail", 100, hidden=2048).rows_per_panel]]))
"""


@pytest.mark.parametrize("rows, tail_rows, edge_rows, node_rows", [(17, 17, 17, 17), (60, 48, 60, 48)])
def test_chain_rows_switch_keeps_both_clamps(ops, rows, tail_rows, edge_rows, node_rows):
    """The switch is read once per process: a child plans the rows recorded under it (it launches nothing).  The block tails ignore a
    value above 48; the GraphConv chains lower it to their cap (64 edge and MLP, 48 node); the row chain, the cluster and the embed fold do
    not read it."""
    key = f"ANEMOI_CHAIN_ROWS={rows}"
    for kind, call, rc, launch in RECORDED[key]:
        if rc == 0 and launch is not None and call[0] > 64:
            if kind == "block_tail" and call[3] == 0:
                assert launch[4] == tail_rows
            elif kind in ("gnn_edge", "gnn_mlp"):
                assert launch[4] == edge_rows
            elif kind == "gnn_node":
                assert launch[4] == node_rows
            elif kind in ("row_chain", "cluster") and (kind == "cluster" or call[3] == 0):
                assert launch[4] == 48
    env = {**os.environ, "ANEMOI_CHAIN_ROWS": str(rows)}
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO)], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {k: (c, wrong) for k, c, wrong in json.loads(r.stdout.strip().splitlines()[-1])}
    assert got[key] == (tail_rows, 0), got
    other = [k for k in got if k != key][0]
    assert got[other][1] > 0  # (the other switch's rows are NOT this process's plans: the comparison can fail)
