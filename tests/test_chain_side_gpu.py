"""A block-tail launch that carries a side job (ops.gt_layer_chain2(..., side=...), anemoi_gt_chain2_side_fwd): the tail's workgroups and the
riders run the code of the two separate launches, so every comparison here is bit for bit - no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 512
SENTINEL = 777.0


def _tail_operands(ops, dtype, n, q_out, hidden=2048, extra=False, seed=0):
    """(positional operands, keywords) of a gt_layer_chain2 call on random weights"""
    gen = torch.Generator().manual_seed(seed + n + q_out)
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)  # noqa: E731
    attn, x = r(n, D).to(dtype), r(n, D).to(dtype)
    wp, bp = (r(D, D) / 22).to(dtype), 0.1 * r(D)
    w1, b1 = (r(hidden, D) / 22).to(dtype), (0.1 * r(hidden)).to(dtype)
    w2, b2 = (r(D, hidden) / 45).to(dtype), 0.1 * r(D)
    w1g, d1 = ops.fold_layer_norm(w1, b1, (1 + 0.2 * r(D)).to(dtype), (0.1 * r(D)).to(dtype))
    parts, kw = [bp, d1, b2], {}
    if q_out:
        wq, bq = (r(q_out, D) / 22).to(dtype), (0.1 * r(q_out)).to(dtype)
        wqg, dq = ops.fold_layer_norm(wq, bq, (1 + 0.2 * r(D)).to(dtype), (0.1 * r(D)).to(dtype))
        parts.append(dq)
        kw = dict(wqg=ops.pack_weight_frag(wqg), q_out_features=q_out)
    if extra:
        kw["extra"] = r(n, D).to(dtype)
    vec = torch.cat(parts).to(dtype).contiguous()
    return (attn, x, ops.pack_weight_frag(wp), ops.pack_weight_frag(w1g), ops.pack_weight_frag(w2), vec, hidden, 1e-5), kw


def _side_operands(ops, dtype, n, k_in, q_out=1024, seed=1):
    """gt_row_chain's positional operands on random weights"""
    gen = torch.Generator().manual_seed(seed + n + k_in)
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)  # noqa: E731
    x = r(n, k_in).to(dtype)
    we, be = (r(D, k_in) / max(k_in, 16) ** 0.5).to(dtype), 0.1 * r(D)
    wq, bq = (r(q_out, D) / 22).to(dtype), (0.1 * r(q_out)).to(dtype)
    wqg, dq = ops.fold_layer_norm(wq, bq, (1 + 0.2 * r(D)).to(dtype), (0.1 * r(D)).to(dtype))
    return x, ops.pack_embedding_frag(we), ops.pack_weight_frag(wqg), torch.cat([be, dq]).to(dtype).contiguous(), q_out, 1e-5


def _as_list(res):
    return [t for t in (res if isinstance(res, tuple) else (res,)) if t is not None]


def _check(ops, dtype, host, host_kw, side_args, want_y, first, count, riders):
    """one hosted launch against the two separate launches, twice"""
    n = side_args[0].shape[0]
    ref_host = _as_list(ops.gt_layer_chain2(*host, **host_kw))
    ref_y, ref_q = ops.gt_row_chain(*side_args, want_x_out=want_y)
    r0, r1 = first * 48, n if count is None else min(n, (first + count) * 48)
    for _ in range(2):  # (a second call reproduces both)
        y = torch.full((n, D), SENTINEL, dtype=dtype, device=DEV) if want_y else None
        q = torch.full((n, side_args[4]), SENTINEL, dtype=dtype, device=DEV)
        side = ops.ChainSide(*side_args, y=y, q=q, first_panel=first, panels=count, max_riders=riders)
        got_host = _as_list(ops.gt_layer_chain2(*host, **host_kw, side=side))
        torch.cuda.synchronize()
        assert len(got_host) == len(ref_host) and all(torch.equal(a, b) for a, b in zip(got_host, ref_host)), "host rows differ"
        for got, ref in ((y, ref_y), (q, ref_q)):
            if got is None:
                continue
            assert torch.equal(got[r0:r1], ref[r0:r1]), "side rows differ from gt_row_chain"
            assert bool((got[:r0] == SENTINEL).all()) and bool((got[r1:] == SENTINEL).all()), "rows outside the panel range were written"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k_in,want_y", [(64, True), (192, False), (192, True), (64, False)])
@pytest.mark.parametrize("riders", [1, 2, 0])
def test_side_job_beside_a_small_tail(dtype, k_in, want_y, riders):
    """149 host rows (4 panels, the last ragged) carry all 8 panels of a 347-row side job (the last ragged): one rider walking all of them,
    two riders walking four each, every idle compute unit (more than there are panels)"""
    from anemoi_core_amd import ops

    host, kw = _tail_operands(ops, dtype, 149, 2048)
    _check(ops, dtype, host, kw, _side_operands(ops, dtype, 347, k_in), want_y, 0, None, riders)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("riders", [1, 2, 0])
def test_side_job_panel_subrange(dtype, riders):
    """panels 3 .. 6 of 8: the rows of the other panels keep their sentinel"""
    from anemoi_core_amd import ops

    host, kw = _tail_operands(ops, dtype, 149, 2048)
    _check(ops, dtype, host, kw, _side_operands(ops, dtype, 347, 64), True, 3, 4, riders)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("q_out,extra,want_x", [(0, False, True), (2048, False, True), (128, False, False), (1024, True, True), (0, True, True)])
def test_side_job_beside_every_kind_of_tail(dtype, q_out, extra, want_x):
    """the tail with and without its trailing projection: four chunks, a narrow one (x2 not written), the latent skip with and without one"""
    from anemoi_core_amd import ops

    host, kw = _tail_operands(ops, dtype, 149, q_out, extra=extra)
    if not want_x:
        kw["want_x_out"] = False
    _check(ops, dtype, host, kw, _side_operands(ops, dtype, 347, 192), True, 0, None, 2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_side_job_beside_a_multi_round_tail(dtype):
    """12 336 host rows = 257 panels = two rounds of 129 workgroups: the tail's workgroups stride by 129, not by the grid, and 127 compute units
    are idle - more riders than the side job's 8 panels, and a cap of 3"""
    from anemoi_core_amd import ops

    assert ops.chain_idle_cus(12336) == 127
    host, kw = _tail_operands(ops, dtype, 12336, 2048)
    side = _side_operands(ops, dtype, 347, 192)
    _check(ops, dtype, host, kw, side, True, 0, None, 0)
    _check(ops, dtype, host, kw, side, False, 1, 6, 3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k_in,riders", [(192, 2), (192, 0), (64, 1), (320, 2)])
def test_riders_run_the_schedule_of_the_whole_side_job(dtype, k_in, riders):
    """A side job of 12 300 rows (257 panels: more than one round) is gt_rowchain_pipe_kernel when launched whole (in_features <= 256), whose
    rounding is not the single-panel schedule's: its riders run the pipelined schedule too (several panels per rider, one, as many riders as
    panels; the job's ragged last panel), and the single-panel one at 320 input columns - bit-equal to the whole launch either way."""
    from anemoi_core_amd import ops

    host, kw = _tail_operands(ops, dtype, 149, 2048)
    side = _side_operands(ops, dtype, 12300, k_in)
    _check(ops, dtype, host, kw, side, True, 250, 7, riders)
    _check(ops, dtype, host, kw, side, False, 3, 5, riders)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,k_in,first,count", [(347, 64, 3, 4), (347, 192, 0, 8), (12300, 192, 100, 157), (12300, 192, 0, 3), (12300, 320, 200, 57),
                                                (30000, 64, 10, 600)])
def test_row_chain_panels_equal_the_whole_launch(dtype, n, k_in, first, count):
    """ops.gt_row_chain_panels (the launch of the panels no tail hosted): a panel range of a single-panel job and of a pipelined one (one round
    and several rounds of the range itself), bit-equal to gt_row_chain on all rows; rows outside the range untouched"""
    from anemoi_core_amd import ops

    args = _side_operands(ops, dtype, n, k_in)
    ref_y, ref_q = ops.gt_row_chain(*args)
    y = torch.full((n, D), SENTINEL, dtype=dtype, device=DEV)
    q = torch.full((n, args[4]), SENTINEL, dtype=dtype, device=DEV)
    ops.gt_row_chain_panels(*args, y, q, first, count)
    torch.cuda.synchronize()
    r0, r1 = first * 48, min(n, (first + count) * 48)
    for got, ref in ((y, ref_y), (q, ref_q)):
        assert torch.equal(got[r0:r1], ref[r0:r1])
        assert bool((got[:r0] == SENTINEL).all()) and bool((got[r1:] == SENTINEL).all())


def test_full_tail_hosts_nothing():
    """256 panels leave no compute unit idle: unsupported, and nothing of either job is launched"""
    from anemoi_core_amd import ops

    dtype = torch.bfloat16
    assert ops.chain_idle_cus(256 * 48) == 0 and ops.chain_idle_cus(255 * 48) == 1
    host, kw = _tail_operands(ops, dtype, 256 * 48, 0)
    side_args = _side_operands(ops, dtype, 347, 64)
    y = torch.full((347, D), SENTINEL, dtype=dtype, device=DEV)
    q = torch.full((347, 1024), SENTINEL, dtype=dtype, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.gt_layer_chain2(*host, **kw, side=ops.ChainSide(*side_args, y=y, q=q))
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((q == SENTINEL).all())


@pytest.fixture(scope="module")
def model_forwards():
    """The benchmark model with two layers (built as bench.build does), one forward per path: the side job on; off with the row chain forced
    for the decoder's destination side; off (the default path: the GEMM pair).  ({path: output}, {path: (hosted, left-over panels) or None})"""
    import argparse

    import bench
    import anemoi_core_amd.models.encoder_processor_decoder as E

    args = argparse.Namespace(data_grid="o96", hidden_res=5, kind="gt", channels=512, layers=2, heads=16, vars=84, dtype="bf16")
    _, model, x = bench.build(args, torch.device(DEV))
    model = model.to(DEV).to(torch.bfloat16)
    x = {"data": x.to(DEV).to(torch.bfloat16)}
    outs, hosted = {}, {}
    dec = model.decoder["data"]
    gate, saved = dec._row_chain_ok, E._SIDE_JOB
    for name, side_job, forced in (("side", True, False), ("row_chain", False, True), ("default", False, False)):
        E._SIDE_JOB = side_job
        if forced:  # the row chain for the decoder's destination side (its only side with an embedding) whatever the row band says
            dec._row_chain_ok = lambda x, lin, ln, projs, band=True: gate(x, lin, ln, projs, False)
        try:
            with torch.no_grad():
                outs[name] = model(x)["data"].float().cpu()
            hosted[name] = E.LAST_SIDE_JOB_PANELS
        finally:
            E._SIDE_JOB = saved
            if forced:
                del dec._row_chain_ok
    return outs, hosted


def test_model_side_job_against_the_default_path(model_forwards):
    """the decoder's destination side riding on the block tails against the default path, the GEMM pair: inside the bound of
    test_mapper_with_row_chain_equals_mapper_without (3e-2 max / 4e-3 mean of the output scale).  With two layers three launches host
    (encoder tail, two processor tails: 504 panels) and 336 panels are left over: the leftover launch runs too."""
    outs, hosted = model_forwards
    print("panels (hosted, left over):", hosted)
    assert hosted["side"] == (504, 336), hosted
    assert hosted["row_chain"] is None and hosted["default"] is None
    a, b = outs["side"], outs["default"]
    scale = float(b.abs().max())
    print(f"side job vs GEMM pair: max {float((a - b).abs().max()) / scale:.3e}, mean {float((a - b).abs().mean()) / scale:.3e} of the output scale {scale:.3f}")
    assert not torch.equal(a, b)  # two different paths really ran
    assert float((a - b).abs().max()) <= 3e-2 * scale and float((a - b).abs().mean()) <= 4e-3 * scale, (float((a - b).abs().max()), scale)


def test_model_side_job_equals_the_row_chain_launch(model_forwards):
    """the side job on against the side job off with the row chain forced for that side: bit-equal.  (Forced at 40 320 rows the row chain is the
    pipelined kernel, whose rounding is not the single-panel schedule's: riders and the leftover launch run the schedule of the whole job.)"""
    outs, _ = model_forwards
    a, b = outs["side"], outs["row_chain"]
    scale = float(b.abs().max())
    print(f"side job vs one row-chain launch: {int((a != b).sum())} of {a.numel()} elements differ, max {float((a - b).abs().max()) / scale:.3e} of the output scale")
    assert torch.equal(a, b)
