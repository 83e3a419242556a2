"""The restatements of tests/model_edge_refs.py are themselves checked, on the CPU: against the reference's own recorded outputs
(tests/golden/edges.pt: preprocessing/normalizer.py; tests/golden/variants.pt: layers/bounding.py) and against this package's
torch evaluation of the column program.  tests/test_model_edge_kernels_gpu.py then holds the HIP kernels to the restatements.

``tests.cpu_ops_shim`` implements none of assemble_input / assemble_output / affine_columns / bound_columns_ (asserted below), so
the assemble restatements are checked against the reference's op sequence written with torch's own permute / cat / index_add_."""
import pytest
import torch

from tests import model_edge_refs as R
from tests.model_edge_refs import BF16, F16, F32


def test_normaliser_restatement_reproduces_the_reference_outputs_bitwise(golden):
    """affine_ref / assemble_input_ref on the reference's recorded buffers (_norm_mul, _norm_add, _input_idx, _output_idx) and
    inputs == the reference's t_in, t_all, i_out, i_all, t_idx, i_idx, bit for bit."""
    c = golden("edges.pt")["normalizer"]
    mul, add = c["buffers"]["_norm_mul"], c["buffers"]["_norm_add"]
    i_in, i_out, idx = c["buffers"]["_input_idx"].long(), c["buffers"]["_output_idx"].long(), torch.tensor(c["data_index"])
    sub = c["x_all"][..., c["data_index"]].contiguous()
    for what, x, sel, inverse, want in (("t_all", c["x_all"], slice(None), False, c["t_all"]), ("i_all", c["x_all"], slice(None), True, c["i_all"]),
                                        ("t_in", c["x_in"], i_in, False, c["t_in"]), ("i_out", c["x_out"], i_out, True, c["i_out"]),
                                        ("t_idx", sub, idx, False, c["t_idx"]), ("i_idx", sub, idx, True, c["i_idx"])):
        R.assert_bits_equal(R.affine_ref(x, mul[sel], add[sel], inverse), want, what)
    # the assembly restatement's normaliser columns are the same two roundings: [3, 5, V] as T = 3 time slices of 5 nodes
    got = R.assemble_input_ref(c["x_in"], None, 3 * c["x_in"].shape[-1] + 2, mul[i_in], add[i_in])
    V = c["x_in"].shape[-1]
    for t in range(3):
        R.assert_bits_equal(got[:, t * V:(t + 1) * V], c["t_in"][t], f"assemble_input_ref time slice {t}")
    assert not bool(got[:, 3 * V:].any())


def test_bounding_restatement_reproduces_the_reference_output_within_the_fp32_bound(golden):
    """bounding_ref on the program of the reference's eight configured boundings == the reference's recorded fp32 output within
    the bound the kernel is held to (U[fp32] * s per op)."""
    from anemoi_core_amd.layers.bounding import build_boundings_for

    c = golden("variants.pt")["bounding"]
    cfgs = [dict(_target_=f"anemoi.models.layers.bounding.{cls}", **kw) for cls, kw in c["specs"]]
    prog = [op for m in build_boundings_for(cfgs, c["name_to_index"], c["statistics"], c["name_to_index_stats"]) for op in m.program()]
    assert sorted({op[0] for op in prog}) == [1, 2, 3, 4, 5, 6, 7, 8]
    want, bound = R.bounding_ref(c["x"], prog)
    R.check_bounding(c["out"], want, bound, "reference output")
    assert float(bound.max()) < 4 * R.U[F32] * float(c["x"].abs().max() + 1)  # the bound is a few fp32 ulps, not a tolerance in disguise


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: R.NAME[d])
@pytest.mark.parametrize("kind", range(1, 9))
def test_bounding_restatement_agrees_with_the_torch_program_at_the_bounds(kind, dtype):
    """On the NaN / +-inf / at-the-bound input set of every dtype (the T-rounded values, evaluated with torch's fp32 ops as
    apply_program_torch runs them) bounding_ref and apply_program_torch agree: NaN at the same places, the same infinities, the
    finite rest within the fp32 bound.  (torch on a 16-bit tensor rounds to T after EVERY op - relu(v - m) + m twice - which is
    not what the bound describes; the kernel rounds a result once.)"""
    from anemoi_core_amd.layers.bounding import apply_program_torch

    for k, (p0, p1) in enumerate(R.BOUND_PAIRS):
        v = R.bounding_inputs(p0, p1, dtype, seed=k)
        x = torch.stack([v, R.total_column(v.numel(), dtype, seed=k), torch.ones_like(v)], -1)
        prog = [(kind, 0, 1, p0, p1)]
        want, _ = R.bounding_ref(x, prog)
        assert float(want[want.isfinite()].abs().max()) < 0.9 * torch.finfo(dtype).max  # the input set overflows in no kind
        want32, bound32 = R.bounding_ref(x.float(), prog)
        assert torch.equal(want32.nan_to_num(1.5), want.nan_to_num(1.5))
        R.check_bounding(apply_program_torch(x.float(), prog), want32, bound32, f"kind {kind} p=({p0}, {p1})")
        assert bool(want[..., 0].isnan().any()) and bool(want[..., 0].isfinite().any())


def test_bounding_restatement_kind_9_is_the_normalisers_inverse():
    """Kind 9 of bounding_ref == affine_ref(inverse) (float64 against torch's fp32 in-place sequence), within the fp32 bound."""
    mul, add, mean, stdev = R.column_stats(7)
    x = R.raw_data((300, 7), F32, mean, stdev)
    x = affine = R.affine_ref(x, mul, add)  # normalised values, O(1)
    want, bound = R.bounding_ref(x, [(9, c, 0, float(add[c]), float(mul[c])) for c in range(7)])
    R.check_bounding(R.affine_ref(affine, mul, add, inverse=True), want, bound, "kind 9")


def test_bounding_bound_accumulates_over_a_chain_and_is_exact_for_one_op():
    x = torch.tensor([[0.25, 2.0, -1.0]])
    want, bound = R.bounding_ref(x, [(5, 0, 0, 0.0, 1.0)])
    assert want.tolist() == [[0.25, 2.0, -1.0]] and bound.tolist() == [[R.U[F32] * 1.0, 0.0, 0.0]]
    want, bound = R.bounding_ref(x, [(1, 1, 0, 0.0, 0.0), (7, 0, 1, 0.0, 1.0), (9, 0, 0, 0.5, 0.25)])
    assert want.tolist() == [[(0.25 * 2.0 - 0.5) / 0.25, 2.0, -1.0]]
    e1, e0 = R.U[F32] * 2.0, 0.25 * R.U[F32] * 2.0 + R.U[F32] * 2.0
    assert bound.tolist() == [[e0 / 0.25 + R.U[F32] * 0.5, e1, 0.0]]


@pytest.mark.parametrize("pair", [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)], ids=lambda p: f"{R.NAME[p[0]]}-{R.NAME[p[1]]}")
def test_assemble_restatements_equal_the_references_op_sequence(pair):
    """assemble_input_ref == normalise in fp32, cast, "b t e g v -> (b e g) (t v)", cat (encoder_processor_decoder.py:98-143);
    assemble_output_ref == x_out.to(dtype) followed by index_add_ of the (normalised) skip columns (:145-158) - written with
    torch's own permute / cat / index_add_ on the data the GPU tests use; and that data does tell x * mul + add in two fp32
    roundings from the fused result."""
    from tests import cpu_ops_shim

    assert not any(hasattr(cpu_ops_shim, n) for n in ("assemble_input", "assemble_output", "affine_columns", "bound_columns_"))
    ti, to = pair
    T, N, V, A, W = 2, 257, 7, 5, 24
    mul, add, mean, stdev = R.column_stats(V, ti)
    x = R.raw_data((T, N, V), ti, mean, stdev)
    attrs = torch.randn(N, A, generator=torch.Generator().manual_seed(1)).to(to)
    batch = x.float().reshape(1, T, 1, N, V).mul(mul).add(add).to(to)  # InputNormalizer.transform, then the model dtype
    want = torch.cat([batch.permute(0, 2, 3, 1, 4).reshape(N, T * V), attrs, torch.zeros(N, W - T * V - A, dtype=to)], -1)
    R.assert_bits_equal(R.assemble_input_ref(x, attrs, W, mul, add, to), want, "assemble_input_ref")
    R.assert_bits_equal(R.assemble_input_ref(x, attrs, W, None, None, to)[:, :T * V], x.to(to).permute(1, 0, 2).reshape(N, T * V), "no normaliser")
    two = x.float().mul(mul).add(add)
    fused = (x.double() * mul.double() + add.double()).float()
    differ = (two != fused) & two.isfinite()
    assert int(differ.sum()) > two.numel() // 20, "the data does not tell two fp32 roundings from a fused multiply-add"
    # output: TM = to (the model dtype), TS = ti (the data dtype)
    V_out = 5
    col_map = torch.tensor([3, -1, 6, 3, 0], dtype=torch.int32)
    x_out = torch.randn(N, V_out, generator=torch.Generator().manual_seed(2)).to(to)
    skip = x[-1]
    for m, a in ((None, None), (mul, add)):
        sk = skip if m is None else skip.float().mul(m).add(a).to(ti)
        want = x_out.to(ti).clone()
        for v, src in enumerate(col_map.tolist()):  # distinct output columns: index_add_ column by column
            if src >= 0:
                want[:, v] = (want[:, v].float() + sk[:, src].float()).to(ti)
        before = x_out.clone()
        R.assert_bits_equal(R.assemble_output_ref(x_out, skip, col_map, m, a), want, "assemble_output_ref")
        assert torch.equal(x_out, before)  # the restatement leaves its inputs alone
