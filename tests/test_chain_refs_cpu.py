"""The restatements, the bound and the split mirror of tests/chain_refs.py are themselves checked, on the CPU: the restatements
against ``oracle.gt_oracle`` (fp32 operands, no rounding points, 1e-5), ``panel_split`` against the splits the row ladders were
chosen for, and the bound against what it has to tell apart: at the K recorded in tests/test_gnn_chain_kernels_gpu.py every named
mutation (chain_refs.MUTATIONS) must break 2 x bound in EVERY row it touches, on the operands the GPU tests use, per dtype - so
a kernel with that error in ONE row cannot pass - and the bound must be nowhere looser than the 2.5e-2 rule it replaces."""
import pytest
import torch
import torch.nn.functional as F

from oracle import gt_oracle as O
from tests import chain_refs as R
from tests.chain_refs import BF16, D, F16, F32, NAME
from tests.test_gnn_chain_kernels_gpu import K

DTYPES = [BF16, F16]
N_SENS = 256 * 4 - 3  # 256 tiles of 4 rows and one of 1: the smallest rung of the r ladder (odd: the last row has no partner to swap with)


# ---------------------------------------------------------------------------------------------------------------- the oracle pins
def _close_to_oracle(got, want, what):
    err = (got - want.double()).abs() / (1.0 + want.double().abs())
    assert float(err.max()) <= 1e-5, f"{what}: {float(err.max()):.3e}"


def _block(C=64, n=50, m=333, seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    p = {}
    for name, k in (("conv.edge_mlp", 3 * C), ("node_mlp", 2 * C)):
        for i, kk in ((0, k), (2, C), (4, C)):
            p[f"b.{name}.mlp.{i}.weight"], p[f"b.{name}.mlp.{i}.bias"] = r(C, kk) / kk ** 0.5, 0.3 * r(C)
        p[f"b.{name}.layer_norm.weight"], p[f"b.{name}.layer_norm.bias"] = 1 + 0.2 * r(C), 0.3 * r(C)
    x, e = r(n, C), r(m, C)
    dst = torch.sort(torch.randint(0, n, (m,), generator=gen)).values
    dst[dst == 7] = 8  # a destination without in-edges
    src = torch.randint(0, n, (m,), generator=gen)
    return p, x, e, src, dst


def test_restatements_reproduce_the_oracles_graphconv_block():
    """edge_chain_ref on the gather-add form of the edge MLP (first weight split into its K blocks [x_i | x_j | e], the node-level
    terms x W_i^T, x W_j^T gathered by dst, src) == edges_new, and node_chain_ref on cat[x, scatter-sum] - agg as a table and as
    ``seg_ptr`` over the dst-sorted edge rows - == nodes_new of oracle.gt_oracle.gconv_processor_block; t == its plain projection."""
    C = 64
    p, x, e, src, dst = _block(C)
    nodes_want, edges_want = O.gconv_processor_block(p, "b", x, e, torch.stack([src, dst]))
    w = p["b.conv.edge_mlp.mlp.0.weight"]
    g1, g2 = x.double() @ w[:, :C].double().t(), x.double() @ w[:, C:2 * C].double().t()
    em = [p[f"b.conv.edge_mlp.mlp.{i}.{k}"] for i in (2, 4) for k in ("weight", "bias")]
    edges = R.edge_chain_ref(e, g1, dst, g2, src, w[:, 2 * C:], p["b.conv.edge_mlp.mlp.0.bias"], *em, p["b.conv.edge_mlp.layer_norm.weight"],
                             p["b.conv.edge_mlp.layer_norm.bias"], round_points=False)
    _close_to_oracle(edges, edges_want, "edges_new")
    nm = [p[f"b.node_mlp.mlp.{i}.{k}"] for i in (0, 2, 4) for k in ("weight", "bias")] + [p["b.node_mlp.layer_norm.weight"], p["b.node_mlp.layer_norm.bias"]]
    ptr = torch.zeros(x.shape[0] + 1, dtype=torch.int32)
    ptr[1:] = torch.bincount(dst, minlength=x.shape[0]).cumsum(0)
    assert int(ptr[8] - ptr[7]) == 0
    gen = torch.Generator().manual_seed(1)
    wt, bt = torch.randn(2 * C, C, generator=gen) / 8, torch.randn(2 * C, generator=gen)
    for bias in (bt, None):
        nodes, t = R.node_chain_ref(x, edges_want, *nm, wt=wt, bt=bias, seg_ptr=ptr, round_points=False)
        _close_to_oracle(nodes, nodes_want, "nodes_new (seg_ptr)")
        _close_to_oracle(t, F.linear(nodes_want, wt, bias), "t")
    agg = torch.zeros_like(x).index_add_(0, dst, edges_want)
    _close_to_oracle(R.node_chain_ref(x, agg, *nm, round_points=False), nodes_want, "nodes_new (table)")
    # the optional operands are optional: no LayerNorm bias == a zero bias
    zero = torch.zeros(C)
    assert torch.equal(R.node_chain_ref(x, agg, *nm[:-1], None, round_points=False), R.node_chain_ref(x, agg, *nm[:-1], zero, round_points=False))


def test_mlp_restatement_reproduces_the_oracles_embedding_mlp():
    """mlp_chain_ref on the input zero-padded to a multiple of 128 columns (the weight's K padded alike) == oracle.gt_oracle.mlp"""
    C, raw, pad, n = 64, 11, 128, 77
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    p = {"m.mlp.0.weight": r(C, raw) / raw ** 0.5, "m.mlp.0.bias": 0.3 * r(C), "m.mlp.2.weight": r(C, C) / 8, "m.mlp.2.bias": 0.3 * r(C),
         "m.mlp.4.weight": r(C, C) / 8, "m.mlp.4.bias": 0.3 * r(C), "m.layer_norm.weight": 1 + 0.2 * r(C), "m.layer_norm.bias": 0.3 * r(C)}
    x, res = r(n, raw), r(n, C)
    want = O.mlp(p, "m", x)
    xp, wp = torch.zeros(n, pad), torch.zeros(C, pad)
    xp[:, :raw], wp[:, :raw] = x, p["m.mlp.0.weight"]
    rest = [p[k] for k in ("m.mlp.0.bias", "m.mlp.2.weight", "m.mlp.2.bias", "m.mlp.4.weight", "m.mlp.4.bias", "m.layer_norm.weight", "m.layer_norm.bias")]
    _close_to_oracle(R.mlp_chain_ref(xp, wp, *rest, round_points=False), want, "embedding MLP")
    _close_to_oracle(R.mlp_chain_ref(xp, wp, *rest, residual=res, round_points=False), want + res, "embedding MLP + residual")


def test_rounding_points_round_and_mutations_are_refused_where_they_do_not_apply():
    x, res = R.mlp_case(9, 128, BF16)
    p = R.params(BF16, 128)
    args = (x, p["w0"], p["b0"], p["w1"], p["b1"], p["w2"], p["b2"], p["g"], p["be"])
    y = R.mlp_chain_ref(*args)
    assert y.dtype == torch.float64 and torch.equal(y, y.to(BF16).double())  # the output is a bf16 value
    assert not torch.equal(y, R.mlp_chain_ref(*args, round_points=False))
    with pytest.raises(ValueError):
        R.mlp_chain_ref(*args, mutate="residual_from_next_row")  # no residual to take
    with pytest.raises(ValueError):
        R.mlp_chain_ref(*args, mutate="drop_bt")
    with pytest.raises(ValueError):
        R.mlp_chain_ref(*args, mutate="drop_b3")


def test_segment_sum_restatement_is_the_fp32_edge_order_sum():
    x, rows, ptr = R.segsum_case(40, BF16, "hub")
    got = R.segment_sum_ref(rows, ptr, BF16)
    for n in (0, 1, 5, 10, 39):
        acc = torch.zeros(D, dtype=F32)
        for i in range(int(ptr[n]), int(ptr[n + 1])):
            acc = acc + rows[i].float()
        assert torch.equal(got[n], acc.to(BF16).double())
    assert int(ptr[40] - ptr[39]) == 41 and not bool(got[0].any())


# ---------------------------------------------------------------------------------------------------------------- the split mirror
SPLITS_64 = {1: (1, 1, 1, 1, 1), 2: (1, 2, 1, 2, 1), 63: (1, 63, 1, 63, 1), 64: (1, 64, 1, 64, 1), 65: (1, 65, 1, 65, 1), 256: (1, 256, 1, 256, 1),
             257: (2, 129, 1, 129, 1), 16385: (33, 497, 17, 256, 2), 32763: (64, 512, 59, 256, 2), 32769: (43, 763, 3, 256, 3)}
SPLITS_48 = {1: (1, 1, 1, 1, 1), 2: (1, 2, 1, 2, 1), 47: (1, 47, 1, 47, 1), 48: (1, 48, 1, 48, 1), 49: (1, 49, 1, 49, 1), 256: (1, 256, 1, 256, 1),
             257: (2, 129, 1, 129, 1), 12289: (25, 492, 14, 256, 2), 24571: (48, 512, 43, 256, 2), 24577: (33, 745, 25, 256, 3)}


def test_panel_split_gives_the_splits_the_ladders_were_chosen_for():
    for cap, table, rs, ladder in ((64, SPLITS_64, R.R_EDGE, R.LADDER_EDGE), (48, SPLITS_48, R.R_NODE, R.LADDER_NODE)):
        want = dict(table)
        want.update({256 * r - 3: (r, 256, r - 3, 256, 1) for r in rs})
        assert sorted(want) == sorted(ladder)
        for n in ladder:
            assert R.panel_split(n, cap) == want[n], (cap, n, R.panel_split(n, cap))
        assert max(ladder) <= 32769
    # workgroups that take the extra panel, next to workgroups that do not, in ONE launch
    assert [R.panel_split(n, 64)[1] - 256 * (R.panel_split(n, 64)[4] - 1) for n in R.MULTI_EDGE] == [241, 256, 251]
    assert [R.panel_split(n, 48)[1] - 256 * (R.panel_split(n, 48)[4] - 1) for n in R.MULTI_NODE] == [236, 256, 233]
    assert R.panel_split(81840, 64)[:3] == (64, 1279, 48) and R.panel_split(40962, 48)[:3] == (41, 1000, 3)  # the sizes of tests/test_chain_gpu.py
    assert set(R.SUBSET_EDGE) <= set(R.LADDER_EDGE) and set(R.SUBSET_NODE) <= set(R.LADDER_NODE)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _edge_args(dtype):
    p = R.params(dtype)
    e, g12, dst, src = R.edge_case(N_SENS, dtype)
    return (e, g12[:, :D], dst, g12[:, D:], src, p["w0"], p["b0"], p["w1"], p["b1"], p["w2"], p["b2"], p["g"], p["be"])


def _node_args(dtype, x, agg):
    p = R.params(dtype)
    return (x, agg, p["wa"], p["ba"], p["w1"], p["b1"], p["w2"], p["b2"], p["g"], p["be"])


def _every_touched_row_breaks_twice_the_bound(what, mutated, want, dtype, k, touched):
    """at least one element beyond 2 x bound in every touched row; untouched rows unchanged"""
    worst = R.units(mutated, want, dtype).amax(1)
    assert int(touched.sum()) >= 0.75 * touched.numel(), f"{what}: touches only {int(touched.sum())} of {touched.numel()} rows"
    assert bool((worst[touched] > 2 * k).all()), (f"{what} {NAME[dtype]}: {int((worst[touched] <= 2 * k).sum())} touched rows stay inside 2 x bound "
                                                  f"(K = {k}); the mildest moves by {float(worst[touched].min()):.1f} units")
    assert not bool(worst[~touched].any()), f"{what}: rows it should not touch moved"


def _all(n):
    return torch.ones(n, dtype=torch.bool)


def _paired(n):
    return torch.arange(n) < n // 2 * 2


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_every_edge_chain_mutation_breaks_twice_the_bound_in_every_row(dtype):
    args = _edge_args(dtype)
    dst, src = args[2].long(), args[4].long()
    want = R.edge_chain_ref(*args)
    touched = {"drop_b0": _all(N_SENS), "drop_b1": _all(N_SENS), "drop_b2": _all(N_SENS), "drop_ln_b": _all(N_SENS),
               "swap_gather_indices": dst != src, "residual_from_next_row": _all(N_SENS),
               "gather_from_next_edge": (dst != dst.roll(-1)) | (src != src.roll(-1)), "swap_adjacent_rows": _paired(N_SENS)}
    for m, rows in touched.items():
        _every_touched_row_breaks_twice_the_bound("edge " + m, R.edge_chain_ref(*args, mutate=m), want, dtype, K["edge"][dtype], rows)


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("k0", [128, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_every_mlp_chain_mutation_breaks_twice_the_bound_in_every_row(dtype, k0, with_res):
    p = R.params(dtype, k0)
    x, res = R.mlp_case(N_SENS, k0, dtype)
    args = (x, p["w0"], p["b0"], p["w1"], p["b1"], p["w2"], p["b2"], p["g"], p["be"])
    kw = dict(residual=res if with_res else None)
    want = R.mlp_chain_ref(*args, **kw)
    touched = {"drop_b0": _all(N_SENS), "drop_b1": _all(N_SENS), "drop_b2": _all(N_SENS), "drop_ln_b": _all(N_SENS), "swap_adjacent_rows": _paired(N_SENS)}
    if with_res:
        touched["residual_from_next_row"] = _all(N_SENS)
    for m, rows in touched.items():
        _every_touched_row_breaks_twice_the_bound(f"mlp K={k0} {m}", R.mlp_chain_ref(*args, mutate=m, **kw), want, dtype, K["mlp_res" if with_res else "mlp"][dtype], rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_every_node_chain_mutation_breaks_twice_the_bound_in_every_row(dtype):
    p = R.params(dtype)
    args = _node_args(dtype, *R.node_case(N_SENS, dtype))
    kw = dict(wt=p["wt"], bt=p["bt"])
    want_x, want_t = R.node_chain_ref(*args, **kw)
    touched = {"drop_b0": _all(N_SENS), "drop_b1": _all(N_SENS), "drop_b2": _all(N_SENS), "drop_ln_b": _all(N_SENS), "residual_from_next_row": _all(N_SENS),
               "swap_wa_halves": _all(N_SENS), "swap_adjacent_rows": _paired(N_SENS)}
    for m, rows in touched.items():
        got_x, got_t = R.node_chain_ref(*args, mutate=m, **kw)
        _every_touched_row_breaks_twice_the_bound("node x' " + m, got_x, want_x, dtype, K["node"][dtype], rows)
        _every_touched_row_breaks_twice_the_bound("node t " + m, got_t, want_t, dtype, K["node_t"][dtype], rows)  # t carries every error of x'
    got_x, got_t = R.node_chain_ref(*args, mutate="drop_bt", **kw)
    assert torch.equal(got_x, want_x)
    _every_touched_row_breaks_twice_the_bound("node t drop_bt", got_t, want_t, dtype, K["node_t"][dtype], _all(N_SENS))


@pytest.mark.parametrize("last", ["hub", "empty"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_a_lost_or_a_foreign_edge_breaks_twice_the_bound_in_every_segment(dtype, last):
    """on the degree ladder of the GPU test: every non-empty segment notices the loss of its last edge - the hub of 41 too - and
    every segment with an edge behind it notices taking that edge in"""
    x, rows, ptr = R.segsum_case(N_SENS, dtype, last)
    args = _node_args(dtype, x, rows)
    want = R.node_chain_ref(*args, seg_ptr=ptr)
    deg = (ptr[1:] - ptr[:-1]).long()
    assert sorted(set(deg.tolist())) == sorted(R.DEGREE_LADDER) and int(deg[-1]) == {"hub": 41, "empty": 0}[last]
    for m, touched in (("drop_last_edge", deg > 0), ("add_next_edge", ptr[1:].long() < rows.shape[0])):
        _every_touched_row_breaks_twice_the_bound("node " + m, R.node_chain_ref(*args, seg_ptr=ptr, mutate=m), want, dtype, K["node"][dtype], touched)


# ---------------------------------------------------------------------------------------------------------------- against the present rule
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_the_bound_is_nowhere_looser_than_the_present_rule(dtype):
    """chain_refs.bound <= 2.5e-2 max|want| + 2.5e-2 |want| (tests/test_chain_gpu.py's _close), element by element, for every output
    of the test operands.  bound() takes the smaller of K u (1 + |want|) and that rule, so this holds by construction; what is
    asserted beside it is that the construction is no disguise: the measured term is the smaller one on more than 99.9 % of the
    elements (all of them in fp16), and where it is not - the largest elements of a bf16 tensor - the rule is within 6 % of it."""
    p = R.params(dtype)
    outs = {"edge": [R.edge_chain_ref(*_edge_args(dtype))], "mlp": [], "mlp_res": []}
    for k0 in (128, 256, 384, 512):
        pk = R.params(dtype, k0)
        x, res = R.mlp_case(N_SENS, k0, dtype)
        for fam, r in (("mlp", None), ("mlp_res", res)):
            outs[fam].append(R.mlp_chain_ref(x, pk["w0"], pk["b0"], pk["w1"], pk["b1"], pk["w2"], pk["b2"], pk["g"], pk["be"], residual=r))
    nx, nt = R.node_chain_ref(*_node_args(dtype, *R.node_case(N_SENS, dtype)), wt=p["wt"], bt=p["bt"])
    x, rows, ptr = R.segsum_case(N_SENS, dtype)
    outs["node"], outs["node_t"] = [nx, R.node_chain_ref(*_node_args(dtype, x, rows), seg_ptr=ptr)], [nt]
    for family, wants in outs.items():
        for want in wants:
            k = K[family][dtype]
            assert bool((R.bound(want, dtype, k) <= R.present_rule(want)).all())
            room = R.present_rule(want) / (k * R.U[dtype] * (1.0 + want.abs()))
            print(f"BOUND {family} {NAME[dtype]} K = {k}: the 2.5e-2 rule is {float(room.min()):.3f} .. {float(room.median()):.1f} (median) x the measured term; "
                  f"it binds on {int((room < 1).sum())} of {room.numel()} elements")
            assert float((room < 1).double().mean()) < 1e-3 and float(room.min()) > 0.94 and (dtype == BF16 or float(room.min()) > 1.0)
