"""CPU checks behind tests/test_wgrad_exact_gpu.py: the Python restatement of the split plan of csrc/wgrad.hip is pinned to the
library through its host-only workspace query, the case lists of tests/wgrad_cases.py are shown to reach every branch of that
plan, every case meets the preconditions that make its expected bits exact, and losing any one of the rows a split or a ragged
step begins or ends with changes the rounded reference - in both dtypes - so that ``torch.equal`` cannot miss it.  No GPU."""
import os

import pytest
import torch

from anemoi_core_amd import _lib
from tests import wgrad_cases as C

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from anemoi_core_amd.build import build_library

        build_library(verbose=False)
    return _lib.load()


def test_plan_restatement_matches_the_library(lib):
    """anemoi_linear_wgrad_workspace_bytes = splits * (O * I + O) * 4 with the splits of ``plan``.  The workgroup target is read
    from ANEMOI_WGRAD_WGS once per process, so the comparison holds only where it is unset."""
    if "ANEMOI_WGRAD_WGS" in os.environ:
        pytest.skip("ANEMOI_WGRAD_WGS overrides the plan's target in this process")
    rows = list(range(1, 1500, 7)) + [2048, 2100, 10242, 14593, 40320, 81840]
    bad = []
    for n in rows:
        for O in (8, 64, 128, 136, 264, 1024, 2048):
            for I in (8, 72, 128, 136, 512, 1024):
                splits, steps, nk = C.plan(n, O, I)
                assert 1 <= splits and (splits - 1) * steps < nk <= splits * steps
                got = int(lib.anemoi_linear_wgrad_workspace_bytes(n, O, I))
                if got != splits * (O * I + O) * 4:
                    bad.append((n, O, I, got, splits))
    assert not bad, bad[:10]
    assert int(lib.anemoi_linear_wgrad_workspace_bytes(0, 8, 8)) == 0


def test_plan_of_the_model_shapes():
    """Two plans worked out by hand from make_plan, so that ``plan`` is not only compared with itself: 10 242 rows of a
    2048 x 512 gradient (64 tiles, 161 steps: 8 splits of 21, 21, ..., 14) and 81 840 rows of 512 x 512 (16 tiles: 32 splits of 40)."""
    assert C.plan(10242, 2048, 512) == (8, 21, 161) and C.split_steps(10242, 2048, 512)[-1] == 14
    assert C.plan(81840, 512, 512) == (32, 40, 1279) and C.split_steps(81840, 512, 512)[-1] == 39


def test_case_lists_reach_every_branch_of_the_plan():
    ladder_n = set(C.ROW_LADDER_N)
    one_tile = (128, 128)

    def steps(n, width=one_tile):
        assert n in ladder_n and width in C.ROW_LADDER_WIDTHS
        return C.split_steps(n, *width)

    # one split whose reduction is shorter than, as long as and longer than the ring (and ragged / full last steps of each)
    assert C.RING_STAGES == 2
    for n, nk in ((1, 1), (7, 1), (8, 1), (9, 1), (63, 1), (64, 1), (65, 2), (127, 2), (129, 3), (448, 7)):
        assert steps(n) == [nk], n
    assert C.last_step_rows(64) == 64 and C.last_step_rows(65) == 1 and C.last_step_rows(127) == 63 and C.last_step_rows(448) == 64
    # two equal splits; the same with a ragged last row
    assert steps(512) == [4, 4] and C.last_step_rows(512) == 64
    assert steps(511) == [4, 4] and C.last_step_rows(511) == 63
    # a shorter last split
    assert steps(513) == [5, 4] and C.last_step_rows(513) == 1
    assert steps(577) == [5, 5] and C.last_step_rows(577) == 1
    assert steps(833) == [5, 5, 4] and C.last_step_rows(833) == 1
    # a last split of one step that holds one row; a last split of two steps whose second holds one row
    assert steps(1281) == [5, 5, 5, 5, 1] and C.last_step_rows(1281) == 1
    assert steps(1345) == [5, 5, 5, 5, 2] and C.last_step_rows(1345) == 1
    # the plan does not depend on the width while the target exceeds the tile count: the other two widths of the ladder split alike
    for n in C.ROW_LADDER_N:
        assert steps(n, (264, 136)) == steps(n) == steps(n, (8, 72))

    # want not clamped by nk // 4 and splits < want; want reached exactly
    assert (2100, 1024, 1024) in C.PRODUCT_LIKE and (2048, 1024, 1024) in C.PRODUCT_LIKE
    tiles = 8 * 8
    want = -(-512 // tiles)
    assert want == 8 and want <= 33 // 4
    assert C.split_steps(2100, 1024, 1024) == [5, 5, 5, 5, 5, 5, 3] and C.plan(2100, 1024, 1024)[0] < want
    assert C.split_steps(2048, 1024, 1024) == [4] * 8 and C.plan(2048, 1024, 1024)[0] == want

    # the width ladder: one granule; both sides of the 64-column half of a piece and of a 128 tile; a last tile of one granule in
    # either direction; more than one tile row and column (the bias gradient belongs to tile column 0 alone)
    widths = set(C.WIDTH_LADDER_WIDTHS)
    assert {(8, 8), (56, 64), (64, 72), (72, 64), (120, 136), (136, 120), (128, 136), (8, 264), (264, 8), (264, 264)} <= widths
    assert any(O % 128 == 8 and O > 128 for O, _ in widths) and any(I % 128 == 8 and I > 128 for _, I in widths)
    assert any(-(-O // 128) > 1 and -(-I // 128) > 1 for O, I in widths)
    for n, multi in ((65, False), (513, True), (1281, True)):
        assert n in C.WIDTH_LADDER_N and all((C.plan(n, O, I)[0] > 1) == multi for O, I in widths)

    # the guarded and poisoned lists hold a one-step last split, a one-row step, one split, and every width of the width ladder
    assert {C.split_steps(*c)[-1] for c in C.GUARDED} >= {1, 2, 4} and any(C.plan(*c)[0] == 1 for c in C.GUARDED)
    assert {(O, I) for _, O, I in C.POISONED} == widths | {(264, 136)}
    assert max(C.plan(*c)[0] for c in C.EXACT_CASES + C.REAL_VALUED) == C.SPLITS_MAX


@pytest.mark.parametrize("case", C.EXACT_CASES, ids=C.case_id)
def test_exactness_preconditions_and_sensitivity(case):
    """The expected bits are exact, and taking out any probed row (first and last of every split, every row of the last 64-row step)
    changes at least one element of the reference after rounding, in bf16 and in fp16.  For the 1024-wide cases the top-left
    128 x 128 block is enough."""
    dz, x = C.operands(*case)
    C.check_exactness_preconditions(dz, x)
    dw, db = C.reference(*case)
    assert torch.equal(dw, dw.round()) and torch.equal(db, db.round())
    rows = C.probe_rows(*case)
    assert rows[0] == 0 and rows[-1] == case[0] - 1
    cut = 128 if max(case[1], case[2]) >= 1024 else max(case[1], case[2])
    dzr = dz[rows][:, :cut].to(torch.float64)
    xr = x[rows][:, :cut].to(torch.float64)
    dwc = dw[:cut, :cut]
    without = dwc.unsqueeze(0) - dzr.unsqueeze(2) * xr.unsqueeze(1)  # [probed rows, O, I]
    for dtype in DTYPES:
        changed = (without.to(dtype) != dwc.to(dtype).unsqueeze(0)).flatten(1).sum(1)
        assert int(changed.min()) >= 1, (dtype, [rows[i] for i in torch.nonzero(changed == 0).flatten().tolist()])
        # and a row counted twice is seen the same way
        twice = (2 * dwc.unsqueeze(0) - without).to(dtype)
        assert int((twice != dwc.to(dtype).unsqueeze(0)).flatten(1).sum(1).min()) >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_granule_rows_hands_the_kernel_what_it_accepts(dtype):
    """autograd._granule_rows: operands the kernel takes in place pass through untouched; a dense view one element into its buffer
    (contiguous as far as torch is concerned, but off the 16-byte boundary) and a view with a row stride of K + 4 are copied."""
    from anemoi_core_amd.autograd import _granule_rows

    n, K = 9, 136

    def accepted(t):
        return t.data_ptr() % 16 == 0 and t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) % 8 == 0)

    base = torch.arange(n * (K + 16) + 1, dtype=torch.float32).remainder(251).to(dtype)
    assert base.data_ptr() % 16 == 0
    dense = base[:n * K].view(n, K)
    slab = base[:n * (K + 16)].view(n, K + 16)[:, 8:8 + K]
    for t in (dense, slab):
        assert accepted(t) and _granule_rows(t) is t
    off_by_one = base[1:1 + n * K].view(n, K)
    strided = base[:n * (K + 4)].view(n, K + 4)[:, :K]
    assert off_by_one.is_contiguous() and not accepted(off_by_one) and not accepted(strided)
    for t in (off_by_one, strided):
        got = _granule_rows(t)
        assert accepted(got) and got.data_ptr() != t.data_ptr() and torch.equal(got, t)


def test_losing_a_row_changes_most_of_the_output():
    """What the method rests on, for EVERY row and not only the probed ones: at (1281, 128, 128) losing any single row changes at
    least a third of the 16 384 elements after rounding, in either dtype.  (An element changes when both of the row's factors
    are non-zero - 16 of 25 - unless the result is past 2^8 in bf16, where odd integers are not representable.)"""
    case = (1281, 128, 128)
    dz, x = C.operands(*case)
    dw, _ = C.reference(*case)
    fewest = {dtype: dw.numel() for dtype in DTYPES}
    for r0 in range(0, case[0], 61):
        dzr, xr = dz[r0:r0 + 61].to(torch.float64), x[r0:r0 + 61].to(torch.float64)
        without = dw.unsqueeze(0) - dzr.unsqueeze(2) * xr.unsqueeze(1)
        for dtype in DTYPES:
            fewest[dtype] = min(fewest[dtype], int((without.to(dtype) != dw.to(dtype).unsqueeze(0)).flatten(1).sum(1).min()))
    assert min(fewest.values()) >= dw.numel() // 3, fewest
