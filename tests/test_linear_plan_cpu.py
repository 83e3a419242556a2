"""CPU checks of the GEMM dispatch (csrc/linear_plan.h) through its host-only query, ops.linear_plan -> anemoi_linear_plan: which kernel,
tile and row split every GEMM shape of the test suite and of the model gets.  No GPU: the query launches nothing."""
import json
import os
import subprocess
import sys

import pytest
import torch

from anemoi_core_amd import _lib
from tests.linear_shapes import CONCAT_GATHER_SHAPES, EPILOGUE_SHAPES, FOLD_ROWS, planned_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ANEMOI_GEMM_BIG", "ANEMOI_GEMM_BIG_MI", "ANEMOI_GEMM_BIG_MI5_T320", "ANEMOI_GEMM_PP", "ANEMOI_GEMM_SPLITWAVE", "ANEMOI_GEMM_NARROW",
            "ANEMOI_GEMM_FAST_EPI", "ANEMOI_LNFOLD_SMALL_ROWS", "ANEMOI_LNFOLD_MI5")


@pytest.fixture(scope="module")
def ops():
    assert not any(name in os.environ for name in SWITCHES), "the recorded plans are those of the default switches: unset ANEMOI_GEMM_* / ANEMOI_LNFOLD_*"
    if not os.path.exists(_lib.LIB_PATH):
        from anemoi_core_amd.build import build_library

        build_library(verbose=False)
    from anemoi_core_amd import ops as _ops

    return _ops


# (role, n_rows, K1, K2, O) -> (kernel, tile rows, tile columns, ping-pong, main_rows, tail_rows) at default switches, 16-bit operands.
# RECORDED from the dispatch as it stood before plan_gemm existed (the launch functions of csrc/linear.hip with their leaf launchers
# replaced by recorders, run on the host) - never regenerated from plan_gemm.  First the shapes of tests/linear_shapes.py, then the
# model's own GEMMs on the O96 / N320 meshes: [10242 | 40320 | 40962 | 81840] rows x {512 -> 2048, 2048 -> 512, 512 -> 512, 512 -> 1024}
# as plain GEMM, statistics producer and fold consumer.
RECORDED = {
    ("plain", 300, 512, 0, 512): ("splitwave", 64, 128, False, 300, 0),
    ("plain", 1000, 512, 0, 2048): ("splitwave", 64, 128, False, 1000, 0),
    ("plain", 257, 2048, 0, 512): ("splitwave", 64, 128, False, 257, 0),
    ("plain", 129, 64, 0, 128): ("ring", 64, 128, False, 129, 0),
    ("plain", 70, 20, 0, 64): ("generic", 64, 64, False, 70, 0),
    ("plain", 50, 11, 0, 7): ("generic", 64, 64, False, 50, 0),
    ("plain", 333, 512, 0, 100): ("mfma128", 128, 128, False, 333, 0),
    ("plain", 5, 64, 0, 64): ("ring", 64, 128, False, 5, 0),
    ("plain", 1300, 512, 0, 2048): ("ring", 192, 128, True, 1300, 0),
    ("plain", 2100, 2048, 0, 512): ("splitwave", 64, 128, False, 2100, 0),
    ("plain", 1111, 512, 0, 512): ("splitwave", 64, 128, False, 1111, 0),
    ("plain", 1030, 64, 0, 100): ("mfma128", 128, 128, False, 1030, 0),
    ("plain", 1500, 72, 0, 512): ("mfma128", 128, 128, False, 1500, 0),
    ("plain", 4200, 512, 0, 2048): ("ring", 192, 128, True, 4200, 0),
    ("plain", 3000, 192, 0, 3072): ("ring", 192, 128, True, 3000, 0),
    ("plain", 10242, 512, 0, 512): ("ring", 192, 128, True, 10242, 0),
    ("plain", 10242, 512, 0, 2048): ("bigtile", 160, 256, False, 10240, 2),
    ("plain", 10242, 192, 0, 2048): ("bigtile", 160, 256, False, 10240, 2),
    ("plain", 4096, 512, 0, 2048): ("ring", 256, 128, True, 4096, 0),
    ("plain", 5282, 1024, 0, 512): ("splitwave", 160, 128, False, 5280, 2),
    ("plain", 400, 512, 512, 512): ("ring", 64, 128, False, 400, 0),
    ("plain", 400, 512, 0, 512): ("splitwave", 64, 128, False, 400, 0),
    ("plain", 90, 32, 32, 32): ("mfma128", 128, 128, False, 90, 0),
    ("plain", 90, 32, 0, 32): ("mfma128", 128, 128, False, 90, 0),
    ("plain", 200, 128, 64, 256): ("ring", 64, 128, False, 200, 0),
    ("plain", 200, 128, 0, 256): ("splitwave", 64, 128, False, 200, 0),
    ("plain", 1400, 512, 512, 512): ("ring", 64, 128, False, 1400, 0),
    ("plain", 1400, 512, 0, 512): ("splitwave", 64, 128, False, 1400, 0),
    ("plain", 1200, 128, 64, 256): ("ring", 64, 128, False, 1200, 0),
    ("plain", 1200, 128, 0, 256): ("splitwave", 64, 128, False, 1200, 0),
    ("plain", 10242, 256, 256, 2048): ("bigtile", 160, 256, False, 10240, 2),
    ("plain", 10242, 256, 0, 2048): ("bigtile", 160, 256, False, 10240, 2),
    ("stats_producer", 10242, 2048, 0, 512): ("splitwave", 160, 128, False, 10240, 2),
    ("plain", 10242, 2048, 0, 512): ("splitwave", 160, 128, False, 10240, 2),
    ("fold_consumer", 10242, 512, 0, 2048): ("bigtile", 160, 256, False, 10240, 2),
    ("stats_producer", 640, 2048, 0, 512): ("splitwave", 64, 128, False, 640, 0),
    ("plain", 640, 2048, 0, 512): ("splitwave", 64, 128, False, 640, 0),
    ("fold_consumer", 640, 512, 0, 2048): ("splitwave", 64, 128, False, 640, 0),
    ("stats_producer", 4000, 2048, 0, 512): ("splitwave", 64, 128, False, 4000, 0),
    ("plain", 4000, 2048, 0, 512): ("splitwave", 64, 128, False, 4000, 0),
    ("fold_consumer", 4000, 512, 0, 2048): ("ring", 192, 128, False, 4000, 0),
    ("stats_producer", 330, 2048, 0, 512): ("splitwave", 64, 128, False, 330, 0),
    ("plain", 330, 2048, 0, 512): ("splitwave", 64, 128, False, 330, 0),
    ("fold_consumer", 330, 512, 0, 2048): ("splitwave", 64, 128, False, 330, 0),
    ("stats_producer", 5282, 2048, 0, 512): ("splitwave", 160, 128, False, 5282, 0),
    ("plain", 5282, 2048, 0, 512): ("splitwave", 160, 128, False, 5280, 2),
    ("fold_consumer", 5282, 512, 0, 2048): ("bigtile", 320, 256, False, 5282, 0),
    ("stats_producer", 5312, 2048, 0, 512): ("splitwave", 160, 128, False, 5312, 0),
    ("plain", 5312, 2048, 0, 512): ("splitwave", 160, 128, False, 5280, 32),
    ("fold_consumer", 5312, 512, 0, 2048): ("bigtile", 320, 256, False, 5312, 0),
    ("stats_producer", 642, 2048, 0, 512): ("splitwave", 64, 128, False, 642, 0),
    ("plain", 642, 2048, 0, 512): ("splitwave", 64, 128, False, 642, 0),
    ("fold_consumer", 642, 512, 0, 2048): ("splitwave", 64, 128, False, 642, 0),
    ("stats_producer", 1469, 2048, 0, 512): ("splitwave", 64, 128, False, 1469, 0),
    ("plain", 1469, 2048, 0, 512): ("splitwave", 64, 128, False, 1469, 0),
    ("fold_consumer", 1469, 512, 0, 2048): ("ring", 192, 128, False, 1469, 0),
    ("stats_producer", 2562, 2048, 0, 512): ("splitwave", 64, 128, False, 2562, 0),
    ("plain", 2562, 2048, 0, 512): ("splitwave", 64, 128, False, 2562, 0),
    ("fold_consumer", 2562, 512, 0, 2048): ("ring", 192, 128, False, 2562, 0),
    ("stats_producer", 10242, 512, 0, 2048): ("bigtile", 160, 256, False, 10240, 2),
    ("fold_consumer", 10242, 2048, 0, 512): ("bigtile", 160, 256, False, 10240, 2),
    ("stats_producer", 10242, 512, 0, 512): ("ring", 192, 128, True, 10242, 0),
    ("fold_consumer", 10242, 512, 0, 512): ("bigtile", 160, 256, False, 10240, 2),
    ("plain", 10242, 512, 0, 1024): ("ring", 192, 128, True, 10242, 0),
    ("stats_producer", 10242, 512, 0, 1024): ("ring", 192, 128, True, 10242, 0),
    ("fold_consumer", 10242, 512, 0, 1024): ("bigtile", 160, 256, False, 10240, 2),
    ("plain", 40320, 512, 0, 2048): ("bigtile", 320, 256, False, 40320, 0),
    ("stats_producer", 40320, 512, 0, 2048): ("bigtile", 320, 256, False, 40320, 0),
    ("fold_consumer", 40320, 512, 0, 2048): ("bigtile", 160, 256, False, 40320, 0),
    ("plain", 40320, 2048, 0, 512): ("bigtile", 160, 256, False, 40320, 0),
    ("stats_producer", 40320, 2048, 0, 512): ("bigtile", 160, 256, False, 40320, 0),
    ("fold_consumer", 40320, 2048, 0, 512): ("bigtile", 160, 256, False, 40320, 0),
    ("plain", 40320, 512, 0, 512): ("bigtile", 160, 256, False, 40320, 0),
    ("stats_producer", 40320, 512, 0, 512): ("bigtile", 160, 256, False, 40320, 0),
    ("fold_consumer", 40320, 512, 0, 512): ("bigtile", 160, 256, False, 40320, 0),
    ("plain", 40320, 512, 0, 1024): ("bigtile", 160, 256, False, 40320, 0),
    ("stats_producer", 40320, 512, 0, 1024): ("bigtile", 160, 256, False, 40320, 0),
    ("fold_consumer", 40320, 512, 0, 1024): ("bigtile", 160, 256, False, 40320, 0),
    ("plain", 40962, 512, 0, 2048): ("bigtile", 320, 256, False, 40960, 2),
    ("stats_producer", 40962, 512, 0, 2048): ("bigtile", 320, 256, False, 40960, 2),
    ("fold_consumer", 40962, 512, 0, 2048): ("bigtile", 160, 256, False, 40960, 2),
    ("plain", 40962, 2048, 0, 512): ("bigtile", 160, 256, False, 40960, 2),
    ("stats_producer", 40962, 2048, 0, 512): ("bigtile", 160, 256, False, 40960, 2),
    ("fold_consumer", 40962, 2048, 0, 512): ("bigtile", 160, 256, False, 40960, 2),
    ("plain", 40962, 512, 0, 512): ("bigtile", 160, 256, False, 40960, 2),
    ("stats_producer", 40962, 512, 0, 512): ("bigtile", 160, 256, False, 40960, 2),
    ("fold_consumer", 40962, 512, 0, 512): ("bigtile", 160, 256, False, 40960, 2),
    ("plain", 40962, 512, 0, 1024): ("bigtile", 160, 256, False, 40960, 2),
    ("stats_producer", 40962, 512, 0, 1024): ("bigtile", 160, 256, False, 40960, 2),
    ("fold_consumer", 40962, 512, 0, 1024): ("bigtile", 160, 256, False, 40960, 2),
    ("plain", 81840, 512, 0, 2048): ("bigtile", 320, 256, False, 81840, 0),
    ("stats_producer", 81840, 512, 0, 2048): ("bigtile", 320, 256, False, 81840, 0),
    ("fold_consumer", 81840, 512, 0, 2048): ("bigtile", 320, 256, False, 81840, 0),
    ("plain", 81840, 2048, 0, 512): ("bigtile", 160, 256, False, 81840, 0),
    ("stats_producer", 81840, 2048, 0, 512): ("bigtile", 160, 256, False, 81840, 0),
    ("fold_consumer", 81840, 2048, 0, 512): ("bigtile", 320, 256, False, 81840, 0),
    ("plain", 81840, 512, 0, 512): ("bigtile", 160, 256, False, 81840, 0),
    ("stats_producer", 81840, 512, 0, 512): ("bigtile", 160, 256, False, 81840, 0),
    ("fold_consumer", 81840, 512, 0, 512): ("bigtile", 320, 256, False, 81840, 0),
    ("plain", 81840, 512, 0, 1024): ("bigtile", 320, 256, False, 81840, 0),
    ("stats_producer", 81840, 512, 0, 1024): ("bigtile", 320, 256, False, 81840, 0),
    ("fold_consumer", 81840, 512, 0, 1024): ("bigtile", 320, 256, False, 81840, 0),
}
MODEL_ROWS = (10242, 40320, 40962, 81840)
MODEL_K_O = ((512, 2048), (2048, 512), (512, 512), (512, 1024))


def _key(p):
    return (p.kernel, p.tile_m, p.tile_n, p.pingpong, p.main_rows, p.tail_rows)


def test_recorded_plans(ops):
    calls = planned_calls() + [(role, n, k, 0, o) for n in MODEL_ROWS for k, o in MODEL_K_O for role in ("plain", "stats_producer", "fold_consumer")]
    assert set(calls) == set(RECORDED), set(calls) ^ set(RECORDED)
    for dtype in (torch.bfloat16, torch.float16):
        got = {c: _key(ops.linear_plan(c[0], c[1], c[2], c[4], K2=c[3], dtype=dtype)) for c in calls}
        wrong = {c: (got[c], RECORDED[c]) for c in calls if got[c] != RECORDED[c]}
        assert not wrong, wrong


def test_plan_does_not_depend_on_the_plain_epilogue_and_fp32_is_generic(ops):
    for n, k, o in EPILOGUE_SHAPES:
        base = ops.linear_plan("plain", n, k, o)
        for res in (False, True):
            for gelu in (False, True):
                p = ops.linear_plan("plain", n, k, o, residual=res, gelu=gelu)
                assert _key(p) == _key(base)
                assert p.epi == (0 if p.kernel in ("generic", "mfma128") else (1 if res else 0) | (4 if gelu else 0))
        assert ops.linear_plan("plain", n, k, o, dtype=torch.float32).kernel == "generic"


def test_query_refuses_what_the_entry_points_refuse(ops):
    assert ops.linear_plan("stats_producer", 1000, 512, 100) is None  # O % 64
    assert ops.linear_plan("fold_consumer", 1000, 72, 512) is None  # K % 64
    assert ops.linear_plan("plain_pre", 1000, 512, 512) is None  # the pre-activation store needs GELU
    assert ops.linear_plan("plain_pre", 1000, 512, 512, gelu=True).epi == 4 | 32
    assert ops.linear_plan("stats_producer", 1000, 512, 512, dtype=torch.float32) is None
    assert _key(ops.linear_plan("split_k", 512, 10240, 512)) == ("ring", 64, 128, False, 512, 0)
    with pytest.raises(ValueError):
        ops.linear_plan("plain", 0, 512, 512)


def test_fold_protocol_producer_peels_only_rows_the_consumer_recomputes(ops):
    """The two-kernel protocol of include/anemoi_hip.h as a property of the two plans: the producer leaves the strip sums of the rows it
    peels ([main_rows, n_rows)) unwritten, so the consumer must take the statistics of at least those rows from the rows themselves
    (its own tail rows on the big tile, the rows from ln_tail_begin on the small tiles) - for every row count and every GEMM shape of a
    block.  What may be peeled at all is built here from the header's words, by enumeration: up to 32 rows beyond a positive multiple
    of the 320-row tile."""
    n_max = 45000
    may_peel = {base + extra: extra for base in range(320, n_max + 1, 320) for extra in range(1, 33)}
    lib, out = _lib.load(), _lib.LinearPlan()
    producer, consumer = ops.GEMM_ROLES.index("stats_producer"), ops.GEMM_ROLES.index("fold_consumer")
    bigtile = ops.GEMM_KERNELS.index("bigtile")
    bad = []
    for n in range(1, n_max + 1):
        allowed = (0, may_peel.get(n, 0))
        peeled, recomputed = [], []
        for k, o in MODEL_K_O:
            for res in (0, 1):
                assert lib.anemoi_linear_plan(producer, n, o, k, 0, res, _lib.BF16, out) == 0
                assert out.main_rows + out.tail_rows == n
                peeled.append(out.tail_rows)
            for gelu in (0, 4):
                assert lib.anemoi_linear_plan(consumer, n, o, k, 0, gelu, _lib.BF16, out) == 0
                if out.kernel == bigtile:
                    assert out.main_rows + out.tail_rows == n and out.ln_tail_begin > n
                    recomputed.append(out.tail_rows)
                else:
                    assert out.main_rows == n and out.tail_rows == 0
                    recomputed.append(max(n - out.ln_tail_begin, 0))
        if not (set(peeled) | set(recomputed) <= set(allowed) and max(peeled) <= min(recomputed)):
            bad.append((n, peeled, recomputed))
    assert not bad, bad[:5]
    # and the rule is not vacuous: the hidden meshes' "+ 2" is peeled by both sides
    p, c = ops.linear_plan("stats_producer", 10242, 2048, 512, residual=True), ops.linear_plan("fold_consumer", 10242, 512, 2048)
    assert (p.main_rows, p.tail_rows, c.main_rows, c.tail_rows) == (10240, 2, 10240, 2)
    c = ops.linear_plan("fold_consumer", 2562, 512, 2048)
    assert c.kernel == "ring" and c.ln_tail_begin == 2560


def test_every_kernel_is_reached_by_a_test_shape_at_default_settings(ops):
    """The union of the plans of tests/linear_shapes.py: every kind of kernel, every ring tile height (with the ping-pong schedule where
    that is the default), both split-wave tiles with and without the statistics epilogue, both big-tile heights."""
    reached = set()
    for role, n, k1, k2, o in planned_calls():
        p = ops.linear_plan(role, n, k1, o, K2=k2)
        reached.add((p.kernel, p.tile_m, p.pingpong, bool(p.epi & 8)) if p.kernel in ("ring", "splitwave") else (p.kernel, p.tile_m))
    want = {("generic", 64), ("mfma128", 128), ("bigtile", 160), ("bigtile", 320),
            ("ring", 64, False, False), ("ring", 192, True, False), ("ring", 256, True, False), ("ring", 192, False, False),
            ("splitwave", 64, False, False), ("splitwave", 64, False, True), ("splitwave", 160, False, False), ("splitwave", 160, False, True)}
    assert want <= reached, want - reached
    # the two shapes that are in test_linear_epilogues for this
    assert _key(ops.linear_plan("plain", 4096, 512, 2048)) == ("ring", 256, 128, True, 4096, 0)
    assert _key(ops.linear_plan("plain", 5282, 1024, 512)) == ("splitwave", 160, 128, False, 5280, 2)
    assert (4096, 512, 2048) in EPILOGUE_SHAPES and (5282, 1024, 512) in EPILOGUE_SHAPES


_CHILD = """
import json, sys
sys.path.insert(0, {repo!r})
from anemoi_core_amd import ops
from tests.linear_shapes import planned_calls
print(json.dumps([[list(c), ops.linear_plan(c[0], c[1], c[2], c[4], K2=c[3])._asdict()] for c in planned_calls()]))
"""


# the settings and ids of tests/test_gemm_variants_gpu.py, and the kernel each id names
@pytest.mark.parametrize("env,variant", [
    ({"ANEMOI_GEMM_BIG": "1"}, lambda p: p["kernel"] == "bigtile"),
    ({"ANEMOI_GEMM_BIG": "0", "ANEMOI_GEMM_PP": "0"}, lambda p: p["kernel"] == "ring" and p["tile_m"] >= 192 and not p["pingpong"] and not p["epi"] & 16),
    ({"ANEMOI_GEMM_BIG": "0", "ANEMOI_GEMM_PP": "1"}, lambda p: p["kernel"] == "ring" and p["tile_m"] >= 192 and p["pingpong"]),
    ({"ANEMOI_GEMM_SPLITWAVE": "0"}, lambda p: p["kernel"] == "ring" and p["tile_m"] == 64)],
    ids=["bigtile-everywhere", "ring-lockstep", "ring-pingpong", "small-m-two-wave-tiles"])
def test_forced_variant_is_reached_with_a_ragged_last_row_tile(env, variant):
    """The switches are read once per process: one child per setting (it plans, it launches nothing).  Each setting must send at least
    one of the linear tests' shapes to the kernel its id names, with a last row tile that is not whole."""
    if not os.path.exists(_lib.LIB_PATH):
        from anemoi_core_amd.build import build_library

        build_library(verbose=False)
    clean = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO)], cwd=REPO, env={**clean, **env}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plans = json.loads(r.stdout.strip().splitlines()[-1])
    hits = [(c, p) for c, p in plans if variant(p)]
    ragged = [c for c, p in hits if p["main_rows"] % p["tile_m"] != 0]
    assert ragged, (env, len(hits))
