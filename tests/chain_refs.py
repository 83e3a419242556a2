"""Plain-torch restatements of the row-resident GraphConv chains (csrc/gnn_chain.hip: gnn_edge_chain_kernel, its MLP instantiation
and gnn_node_chain_kernel), the bound their tests hold them to, a Python mirror of the launch code's panel split, and the operands
the tests share.  Nothing here imports ``anemoi_core_amd``: tests/test_gnn_chain_kernels_gpu.py holds the kernels to these
functions, tests/test_chain_refs_cpu.py holds THESE functions to ``oracle.gt_oracle`` and checks that the bound tells a wrong
kernel from a right one row by row.  (Restatements of the GraphTransformer chains - gt_chain2, the cluster chain, the row chain -
belong beside these when their tests are reworked: same ``_Eval`` helper, same ``bound``.)

The operation, reference lines layers/conv.py:29-81, layers/block.py:361-395, layers/mlp.py:29-100:

  edge chain  e' = LayerNorm(W2 gelu(W1 gelu(W0 e + g1[idx1] + g2[idx2] + b0) + b1) + b2) + e
  MLP chain   y  = LayerNorm(W2 gelu(W1 gelu(W0 x + b0) + b1) + b2) [+ residual]
  node chain  x' = LayerNorm(Wc gelu(Wb gelu(Wa [x | agg] + ba) + bb) + bc) + x,  t = x' Wt^T [+ bt]
              agg given, or agg[n] = sum of the edge rows [seg_ptr[n], seg_ptr[n + 1])

Every function takes the operands AFTER they were rounded to the model dtype and evaluates in ``prec`` (float64) with the erf GELU.
``round_points=True`` rounds to the model dtype exactly where the kernels do: h1, h2, z / y in front of the LayerNorm, the output,
agg behind its segment sum (summed in fp32 in edge order, as the kernel and ops.segment_sum_rows do), and t formed from the ROUNDED
x'.  ``mutate`` names ONE deliberate error (MUTATIONS): what a subtly wrong kernel would compute."""
import functools
import math

import torch
import torch.nn.functional as F

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
INT_VIEW = {BF16: torch.int16, F16: torch.int16}
D = 512
EPS = 1e-5

# one rounding to the dtype moves a value by at most U * |value| (8 and 11 significant bits)
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}

MUTATIONS = {
    "drop_b0": "the first Linear without its bias (b0 / ba)",
    "drop_b1": "the second Linear without its bias",
    "drop_b2": "the third Linear without its bias",
    "drop_ln_b": "the LayerNorm without its bias",
    "drop_bt": "the trailing projection without its bias",
    "swap_gather_indices": "g1[idx2] + g2[idx1]",
    "residual_from_next_row": "row r takes the residual of row r + 1 (the last one of row 0)",
    "gather_from_next_edge": "row r takes the gathered rows of edge r + 1 (the last one of edge 0)",
    "swap_adjacent_rows": "the first GEMM reads row r ^ 1 (rows 2 k and 2 k + 1 swapped; an odd last row stays)",
    "drop_last_edge": "every non-empty segment loses its last edge",
    "add_next_edge": "every segment with an edge behind it takes the first edge of what follows",
    "swap_wa_halves": "Wa's K halves swapped: x meets the agg columns and agg the x columns",
}


# ---------------------------------------------------------------------------------------------------------------- bound and split
def bound(want, dtype, k):
    """Elementwise: k * U[dtype] * (1 + |want|), and never more than ``present_rule`` allows for the same tensor.  k is measured, not
    chosen: tests/test_gnn_chain_kernels_gpu.py (K, MEASURED).  The second term binds only in bf16 and only on the largest elements
    of a tensor: k u (1 + |w|) exceeds 2.5e-2 (max|w| + |w|) at |w| = max|w| = m when k > 12.8 m / (1 + m) - for m = 8.3 (1 021
    rows of the edge chain) when k > 11.4, for the m = 3 of a single row when k > 9.6."""
    want = want.to(F64)
    return torch.minimum(k * U[dtype] * (1.0 + want.abs()), present_rule(want))


def units(got, want, dtype):
    """|got - want| in units of U[dtype] * (1 + |want|), elementwise, float64."""
    want = want.to(F64)
    return (got.to(F64) - want).abs() / (U[dtype] * (1.0 + want.abs()))


def present_rule(want, tol=2.5e-2):
    """The bound of tests/test_chain_gpu.py (_close with tol 2.5e-2): tol * max|want| + tol * |want|."""
    want = want.to(F64)
    return tol * max(float(want.abs().max()), 1e-3) + tol * want.abs()


def panel_split(n, cap):
    """The tests' own restatement of gnn_rows_per_tile + the grid rule of the three GraphConv launches in csrc/chain_plan.h (cap = 64: edge
    and MLP chain, 48: node chain; no ANEMOI_CHAIN_ROWS / ANEMOI_GNN_NODE_ROWS) - tests/test_chain_plan_cpu.py holds the plan to it.  -> (rows_per_tile, tiles, last, grid, panels_per_workgroup):
    ``last`` = rows of the last tile, ``panels_per_workgroup`` = what the busiest workgroup walks; tiles - (that - 1) * grid
    workgroups walk that many, the others one fewer."""
    rounds = (n + 256 * cap - 1) // (256 * cap)
    rows = min(max((n + 256 * rounds - 1) // (256 * rounds), 1), cap)
    tiles = (n + rows - 1) // rows
    grid = min(tiles, 256)
    return rows, tiles, n - (tiles - 1) * rows, grid, (tiles + grid - 1) // grid


# the row ladders (cap 64 / cap 48): one-row tiles; two-row tiles with a last tile of 1; 256 tiles of r rows with a last tile of r - 3 for
# r on both sides of every 16-row MFMA band edge and of the stores' 8-row groups; then two and three rounds of panels
R_EDGE = (4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
R_NODE = (4, 15, 16, 17, 31, 32, 33, 47, 48)
MULTI_EDGE = (16385, 32763, 32769)
MULTI_NODE = (12289, 24571, 24577)
LADDER_EDGE = (1, 2, 63, 64, 65, 256, 257) + tuple(256 * r - 3 for r in R_EDGE) + MULTI_EDGE
LADDER_NODE = (1, 2, 47, 48, 49, 256, 257) + tuple(256 * r - 3 for r in R_NODE) + MULTI_NODE
SUBSET_EDGE = (256 * 17 - 3, 256 * 48 - 3, 256 * 64 - 3) + MULTI_EDGE
SUBSET_NODE = (256 * 17 - 3, 256 * 48 - 3) + MULTI_NODE  # (r = 64 / 48: for the node chain both name r = 48)
DEGREE_LADDER = (0, 1, 7, 8, 9, 11, 12, 13, 16, 17, 41)


# ---------------------------------------------------------------------------------------------------------------- restatements
class _Eval:
    """The arithmetic the three restatements share: ``prec`` evaluation, rounding to the model dtype at the kernels' rounding points."""

    def __init__(self, dtype, prec, round_points):
        self.dtype, self.prec, self.on = dtype, prec, round_points

    def up(self, t):
        return None if t is None else t.to(self.prec)

    def rnd(self, t):
        return t.to(self.dtype).to(self.prec) if self.on else t

    def linear(self, x, w, b, drop=False):
        return F.linear(x, self.up(w), None if drop else self.up(b))

    def hidden(self, x, w, b, drop=False, add=None):
        y = self.linear(x, w, b, drop)
        return self.rnd(F.gelu(y if add is None else y + add))

    def ln_res(self, z, g, b, eps, res, drop=False):
        y = F.layer_norm(z, (z.shape[-1],), self.up(g), None if drop else self.up(b), eps)
        return self.rnd(y if res is None else y + res)


def _check(mutate, allowed):
    if mutate is not None and (mutate not in MUTATIONS or mutate not in allowed):
        raise ValueError(f"mutation {mutate!r} is not one of {sorted(allowed)}")


def _swap_adjacent(x):
    n = x.shape[0] // 2 * 2
    idx = torch.arange(x.shape[0], device=x.device)
    idx[:n] ^= 1
    return x[idx]


def edge_chain_ref(e, g1, idx1, g2, idx2, w0, b0, w1, b1, w2, b2, ln_w, ln_b, eps=EPS, *, prec=F64, round_points=True, mutate=None):
    """[M, C] in ``prec``.  e [M, C]; g1, g2 [*, C] gathered by idx1, idx2 [M]; w0, w1, w2 [C, C] (w0: the e block of the first
    Linear); ln_b may be None.  The first epilogue adds (acc + b0) + (g1 row + g2 row), the association of the kernels."""
    _check(mutate, {"drop_b0", "drop_b1", "drop_b2", "drop_ln_b", "swap_gather_indices", "residual_from_next_row", "gather_from_next_edge",
                    "swap_adjacent_rows"})
    ev = _Eval(e.dtype, prec, round_points)
    i1, i2 = idx1.long(), idx2.long()
    if mutate == "swap_gather_indices":
        i1, i2 = i2, i1
    if mutate == "gather_from_next_edge":
        i1, i2 = i1.roll(-1), i2.roll(-1)
    x = ev.up(e)
    res = x.roll(-1, 0) if mutate == "residual_from_next_row" else x
    if mutate == "swap_adjacent_rows":
        x = _swap_adjacent(x)
    h1 = ev.hidden(x, w0, b0, mutate == "drop_b0", add=ev.up(g1)[i1] + ev.up(g2)[i2])
    h2 = ev.hidden(h1, w1, b1, mutate == "drop_b1")
    z = ev.rnd(ev.linear(h2, w2, b2, mutate == "drop_b2"))
    return ev.ln_res(z, ln_w, ln_b, eps, res, mutate == "drop_ln_b")


def mlp_chain_ref(x, w0, b0, w1, b1, w2, b2, ln_w, ln_b, eps=EPS, residual=None, *, prec=F64, round_points=True, mutate=None):
    """[N, C] in ``prec``.  x [N, K] (zero-padded by the caller), w0 [C, K]; ln_b and residual may be None."""
    _check(mutate, {"drop_b0", "drop_b1", "drop_b2", "drop_ln_b", "swap_adjacent_rows"} | ({"residual_from_next_row"} if residual is not None else set()))
    ev = _Eval(x.dtype, prec, round_points)
    xx, res = ev.up(x), ev.up(residual)
    if mutate == "residual_from_next_row":
        res = res.roll(-1, 0)
    if mutate == "swap_adjacent_rows":
        xx = _swap_adjacent(xx)
    h1 = ev.hidden(xx, w0, b0, mutate == "drop_b0")
    h2 = ev.hidden(h1, w1, b1, mutate == "drop_b1")
    z = ev.rnd(ev.linear(h2, w2, b2, mutate == "drop_b2"))
    return ev.ln_res(z, ln_w, ln_b, eps, res, mutate == "drop_ln_b")


def segment_sum_ref(rows, seg_ptr, dtype, *, prec=F64, round_points=True, mutate=None):
    """agg[n] = sum of rows[seg_ptr[n] : seg_ptr[n + 1]] -> [N, C] in ``prec``.  With ``round_points``: summed in fp32 from zero in
    edge order and rounded once to ``dtype`` (bit for bit what ops.segment_sum_rows and the node chain's own aggregation give);
    without: summed in ``prec``."""
    ptr = seg_ptr.long()
    beg, end = ptr[:-1].clone(), ptr[1:].clone()
    M = rows.shape[0]
    if mutate == "drop_last_edge":
        end = torch.where(end > beg, end - 1, end)
    if mutate == "add_next_edge":
        end = torch.where(end < M, end + 1, end)
    acc_t = F32 if round_points else prec
    acc = torch.zeros(beg.shape[0], rows.shape[1], dtype=acc_t, device=rows.device)
    src = rows.to(acc_t)
    deg = end - beg
    for k in range(int(deg.max()) if deg.numel() else 0):
        live = (deg > k).nonzero().reshape(-1)
        acc[live] = acc[live] + src[beg[live] + k]
    return acc.to(dtype).to(prec) if round_points else acc.to(prec)


def node_chain_ref(x, agg, wa, ba, wb, bb, wc, bc, ln_w, ln_b, eps=EPS, wt=None, bt=None, seg_ptr=None, *, prec=F64, round_points=True,
                   mutate=None):
    """x' [N, C], or (x', t [N, T]) with ``wt`` [T, C], in ``prec``.  agg [N, C], or with ``seg_ptr`` [N + 1] the edge rows [M, C]
    sorted by destination.  wa [C, 2 C]: K columns [0, C) meet x, [C, 2 C) meet agg."""
    _check(mutate, {"drop_b0", "drop_b1", "drop_b2", "drop_ln_b", "residual_from_next_row", "swap_wa_halves", "swap_adjacent_rows"}
           | ({"drop_bt"} if bt is not None else set()) | ({"drop_last_edge", "add_next_edge"} if seg_ptr is not None else set()))
    ev = _Eval(x.dtype, prec, round_points)
    xx = ev.up(x)
    if seg_ptr is not None:
        a = segment_sum_ref(agg, seg_ptr, x.dtype, prec=prec, round_points=round_points, mutate=mutate if mutate in ("drop_last_edge", "add_next_edge") else None)
    else:
        a = ev.up(agg)
    res = xx.roll(-1, 0) if mutate == "residual_from_next_row" else xx
    if mutate == "swap_adjacent_rows":
        xx = _swap_adjacent(xx)
    C = xx.shape[1]
    w = torch.cat([wa[:, C:], wa[:, :C]], 1) if mutate == "swap_wa_halves" else wa
    h1 = ev.hidden(torch.cat([xx, a], 1), w, ba, mutate == "drop_b0")
    h2 = ev.hidden(h1, wb, bb, mutate == "drop_b1")
    y = ev.rnd(ev.linear(h2, wc, bc, mutate == "drop_b2"))
    x_new = ev.ln_res(y, ln_w, ln_b, eps, res, mutate == "drop_ln_b")
    if wt is None:
        return x_new
    return x_new, ev.rnd(ev.linear(x_new, wt, bt, mutate == "drop_bt"))


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def params(dtype, k0=D, t_out=2 * D):
    """The parameters every test of a dtype shares (CPU, rounded to ``dtype``; treat as read-only).  Biases are 0.3 N(0, 1): with the
    0.1 of tests/test_chain_gpu.py a dropped b0 moves a bf16 row by 18 units of the bound - too little to be told from 2 K
    (tests/test_chain_refs_cpu.py asserts what these give)."""
    gen = torch.Generator().manual_seed(1234 + k0)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    p = dict(w0=r(D, k0) / math.sqrt(k0), b0=0.3 * r(D), w1=r(D, D) / 22, b1=0.3 * r(D), w2=r(D, D) / 22, b2=0.3 * r(D),
             g=1 + 0.2 * r(D), be=0.3 * r(D), wa=r(D, 2 * D) / 32, ba=0.3 * r(D), wt=r(t_out, D) / 22, bt=0.3 * r(t_out))
    return {k: v.to(dtype) for k, v in p.items()}


def edge_case(n, dtype):
    """(e [n, D], g12 [nodes, 2 D], dst [n] sorted, src [n]) on the CPU: g1 = g12[:, :D] by dst, g2 = g12[:, D:] by src."""
    gen = torch.Generator().manual_seed(10_000 + n)
    nodes = max(2, n // 6 + 3)
    e = torch.randn(n, D, generator=gen).to(dtype)
    g12 = torch.randn(nodes, 2 * D, generator=gen).to(dtype)
    dst = torch.sort(torch.randint(0, nodes, (n,), generator=gen)).values.to(torch.int32)
    src = torch.randint(0, nodes, (n,), generator=gen).to(torch.int32)
    return e, g12, dst, src


def mlp_case(n, k0, dtype):
    """(x [n, k0], residual [n, D])"""
    gen = torch.Generator().manual_seed(20_000 + n + k0)
    return torch.randn(n, k0, generator=gen).to(dtype), torch.randn(n, D, generator=gen).to(dtype)


def node_case(n, dtype):
    """(x [n, D], agg [n, D]): agg at the scale of a sum over nine edge rows"""
    gen = torch.Generator().manual_seed(30_000 + n)
    return torch.randn(n, D, generator=gen).to(dtype), (3.0 * torch.randn(n, D, generator=gen)).to(dtype)


def segsum_case(n, dtype, last="ladder"):
    """(x [n, D], edge rows [M, D], seg_ptr int32 [n + 1]): in-degrees DEGREE_LADDER by row index modulo its length - inside the first
    batch of 8 loads, exactly 8, the four-row loop with 1, 3 and 4 of its rows live, one batch more, and a hub -; ``last``: the
    in-degree of row n - 1, "hub" (41), "empty" (0) or what the ladder gives."""
    gen = torch.Generator().manual_seed(40_000 + n)
    deg = torch.tensor(DEGREE_LADDER)[torch.arange(n) % len(DEGREE_LADDER)]
    if last != "ladder":
        deg[n - 1] = {"hub": 41, "empty": 0}[last]
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = deg.cumsum(0).to(torch.int32)
    x = torch.randn(n, D, generator=gen).to(dtype)
    rows = torch.randn(int(ptr[-1]), D, generator=gen).to(dtype)
    return x, rows, ptr
