"""Cases, operands and the exact reference of the transpose-read weight gradient (csrc/wgrad.hip), shared by
tests/test_wgrad_cases_cpu.py (which pins ``plan`` to the library and proves the case lists reach every branch of the split
plan) and tests/test_wgrad_exact_gpu.py (which runs them).  Nothing here needs a GPU.

The operands are integers in [-2, 2].  Every product is exact in bf16 / fp16, every fp32 partial sum is an integer below 2^24 and
so exact in any order, any split and any MFMA grouping: the kernel has to return the exact integer dZ^T X rounded once
(to nearest even) to the output dtype, bit for bit.
"""
import functools

import torch

TM = TN = 128  # output tile of wgrad_tn_kernel
TK = 64        # rows per step the plan counts in
RING_STAGES = 2  # the default ring: 2 stages of 64 rows; a reduction of fewer steps never refills a stage
SPLITS_MAX = 8  # the most splits any case below gets at the default target (asserted by the CPU tests)


def _cdiv(a, b):
    return -(-a // b)


def plan(n_rows, O, I, target=512):
    """(splits, steps_per_split, nk): make_plan of csrc/wgrad.hip restated.  ``target`` is the number of workgroups aimed for."""
    tiles = _cdiv(O, TM) * _cdiv(I, TN)
    nk = _cdiv(n_rows, TK)
    want = min(max(1, _cdiv(target, tiles)), max(1, nk // 4))
    steps = _cdiv(nk, want)
    splits = _cdiv(nk, steps)
    return splits, steps, nk


def split_steps(n_rows, O, I, target=512):
    """Steps per split, split by split: [5, 5, 4] for 833 rows on one tile."""
    splits, steps, nk = plan(n_rows, O, I, target)
    return [min(steps, nk - s * steps) for s in range(splits)]


def last_step_rows(n_rows):
    return n_rows - (_cdiv(n_rows, TK) - 1) * TK


ROW_LADDER_N = [1, 7, 8, 9, 63, 64, 65, 127, 129, 448, 511, 512, 513, 577, 833, 1281, 1345]
ROW_LADDER_WIDTHS = [(128, 128), (264, 136), (8, 72)]
ROW_LADDER = [(n, O, I) for (O, I) in ROW_LADDER_WIDTHS for n in ROW_LADDER_N]

WIDTH_LADDER_WIDTHS = [(8, 8), (8, 264), (264, 8), (56, 64), (64, 72), (72, 64), (120, 136), (136, 120), (128, 136), (264, 264)]
WIDTH_LADDER_N = [65, 513, 1281]
WIDTH_LADDER = [(n, O, I) for (O, I) in WIDTH_LADDER_WIDTHS for n in WIDTH_LADDER_N]

PRODUCT_LIKE = [(2100, 1024, 1024), (2048, 1024, 1024)]

POISONED = [(n, 264, 136) for n in ROW_LADDER_N] + [(513, O, I) for (O, I) in WIDTH_LADDER_WIDTHS]
GUARDED = [(1281, 264, 136), (513, 8, 8), (65, 136, 120), (1345, 128, 136)]
AUTOGRAD = (1281, 264, 136)  # (n, O, K)
REAL_VALUED = [(1281, 264, 136), (2100, 1024, 1024)]

EXACT_CASES = list(dict.fromkeys(ROW_LADDER + WIDTH_LADDER + PRODUCT_LIKE + POISONED + GUARDED + [AUTOGRAD]))


def case_id(case):
    return "n%d-O%d-I%d" % case


def ints(gen, shape):
    """Uniform integers in [-2, 2] (int8, CPU) from a seeded CPU generator."""
    return torch.randint(-2, 3, shape, generator=gen, dtype=torch.int8)


def exact_reference(dz, x):
    """(dW, db) = (dz^T x, column sums of dz) in float64: exact for integer operands of these sizes."""
    dz64, x64 = dz.to(torch.float64), x.to(torch.float64)
    return dz64.t() @ x64, dz64.sum(0)


@functools.lru_cache(maxsize=None)
def operands(n_rows, O, I):
    """The integer operands (dz [n, O], x [n, I]) of a case: one seed per case, so every test sees the same data."""
    gen = torch.Generator().manual_seed(1_000_003 * n_rows + 1009 * O + I)
    return ints(gen, (n_rows, O)), ints(gen, (n_rows, I))


@functools.lru_cache(maxsize=None)
def reference(n_rows, O, I):
    """exact_reference of ``operands``, computed once per process; callers must not write to it."""
    return exact_reference(*operands(n_rows, O, I))


def check_exactness_preconditions(dz, x):
    """What makes the expected bits independent of the summation order, and representable: asserted per case."""
    a64, b64 = dz.to(torch.float64).abs(), x.to(torch.float64).abs()
    dw, _ = exact_reference(dz, x)
    assert float((a64.t() @ b64).max()) < 2 ** 24
    assert float(a64.sum(0).max()) < 2 ** 24
    assert float(dw.abs().max()) < 2 ** 15  # fp16 does not overflow


def probe_rows(n_rows, O, I):
    """The rows whose loss a test must notice: first and last row of every split, and every row of the last 64-row step."""
    rows, r0 = set(), 0
    for steps in split_steps(n_rows, O, I):
        r1 = min(n_rows, r0 + steps * TK)
        rows.update((r0, r1 - 1))
        r0 = r1
    assert r0 == n_rows
    rows.update(range(n_rows - last_step_rows(n_rows), n_rows))
    return sorted(rows)
