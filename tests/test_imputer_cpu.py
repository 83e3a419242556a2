"""The imputers on CPU tensors against the reference's recorded behaviour (tests/golden/imputer.pt, written by
tests/golden/make_golden_imputer.py from preprocessing/imputer.py), the plain-torch restatements of the imputer kernels
(tests/imputer_refs.py) against the same records, and the chains ``predict_step`` fuses."""
import pytest
import torch

from anemoi_core_amd.models import AnemoiModelEncProcDec
from anemoi_core_amd.preprocessing import BaseImputer, ConstantImputer, CopyImputer, InputImputer, InputNormalizer, Processors
from anemoi_core_amd.preprocessing.imputer import COPY
from anemoi_core_amd.utils.config import DotDict
from tests.helpers import indices_from_fixture
from tests.imputer_helpers import CLASSES, KEYS, build
from tests.imputer_refs import impute_ref, restore_nan_ref
from tests.model_edge_refs import assert_bits_equal



@pytest.fixture(scope="module")
def fx(golden):
    return golden("imputer.pt")


def same(got, want, what=""):
    """Bit-equal, NaN at the same places."""
    assert_bits_equal(got, want, what)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", list(CLASSES))
def test_transform_and_inverse_equal_the_reference(fx, name, key):
    want = fx["cases"][name][key]
    imp = build(fx, name)
    x = fx["inputs"][key].clone()
    y = imp.transform(x, in_place=False)
    same(y, want["transform"], "transform")
    same(x, fx["inputs"][key], "the input of in_place=False")
    assert imp.nan_locations.dtype == torch.bool and torch.equal(imp.nan_locations, want["nan_locations"])
    if want["loss_mask_training"] is None:
        assert imp.loss_mask_training is None
    else:
        assert imp.loss_mask_training.dtype == want["loss_mask_training"].dtype
        assert torch.equal(imp.loss_mask_training, want["loss_mask_training"])
    out = fx["outputs"][key]
    same(imp.inverse_transform(out, in_place=False), want["inverse"], "inverse")
    if "inverse_ens2" in want:  # the stored mask is broadcast over every dimension between batch and grid
        same(imp.inverse_transform(fx["outputs"][key + "_ens2"], in_place=False), want["inverse_ens2"], "inverse, two members")
    # in place: the same tensor comes back, changed
    x2, o2 = fx["inputs"][key].clone(), out.clone()
    assert imp.transform(x2) is x2 and imp.inverse_transform(o2) is o2
    same(x2, want["transform"], "in-place transform")
    same(o2, want["inverse"], "in-place inverse")


@pytest.mark.parametrize("name", list(CLASSES))
def test_attributes_and_empty_state_dict(fx, name):
    want = fx["cases"][name]["training"]
    imp = build(fx, name)
    assert isinstance(imp, BaseImputer) and imp.supports_skip_imputation
    for attr in ("index_training_input", "index_inference_input", "index_training_output", "index_inference_output"):
        assert getattr(imp, attr) == want["attributes"][attr], attr
    assert [float(r) if name != "CopyImputer" else r for r in imp.replacement] == \
           [float(r) if name != "CopyImputer" else r for r in want["attributes"]["replacement"]]
    idx = fx["indices"]
    assert (imp.num_training_input_vars, imp.num_inference_input_vars, imp.num_training_output_vars, imp.num_inference_output_vars) == \
           (len(idx["data_input_name_to_index"]), len(idx["model_input_name_to_index"]), len(idx["data_output_name_to_index"]),
            len(idx["model_output_name_to_index"]))
    assert imp.nan_locations is None and imp.loss_mask_training is None
    assert list(imp.state_dict().keys()) == want["state_dict_keys"] == []
    imp.load_state_dict({}, strict=True)


def test_config_as_mapping_or_attribute_dict(fx):
    a = build(fx, "ConstantImputer")
    b = build(fx, "ConstantImputer", DotDict({str(k): v for k, v in fx["configs"]["ConstantImputer"].items()}))
    assert a.replacement == b.replacement and a.index_training_input == b.index_training_input


@pytest.mark.parametrize("name", list(CLASSES))
def test_member_zero_decides_for_every_member(fx, name):
    """Two members (the reference's own boolean-mask assignment raises there - recorded - while its ``get_nans`` states the rule): NaN of
    member 0 is imputed in both members, NaN of member 1 alone stays; member 0 equals the recorded one-member run of the same rows."""
    assert "IndexError" in fx["cases"][name]["inference_ens2"]["error"]
    imp = build(fx, name)
    x = fx["inputs"]["inference_ens2"]
    y = imp.transform(x, in_place=False)
    want, mask = impute_ref(x, imp.program(x.shape[-1]))
    same(y, want, "two members")
    assert torch.equal(imp.nan_locations, mask)
    d = fx["indices"]["model_input_name_to_index"]["d"]
    if name != "CopyImputer":
        assert bool(y[1, 0, 1, 4, d].isnan()) and not bool(y[1, 0, 0, 4, d].isnan())  # planted in member 1 only: stays
        assert not bool(y[0, :, :, 3, d].isnan().any())  # planted in both members: imputed in both


def test_errors(fx):
    imp = build(fx, "InputImputer")
    with pytest.raises(ValueError, match="does not match the training"):
        imp.transform(torch.zeros(1, 1, 3, 5))
    with pytest.raises(RuntimeError, match="Cannot inverse-transform before"):
        imp.inverse_transform(fx["outputs"]["inference"].clone())
    with pytest.raises(ValueError, match="does not match the training"):
        imp.inverse_transform(torch.zeros(1, 1, 3, 9))
    imp.transform(fx["inputs"]["inference"].clone())
    with pytest.raises(AssertionError, match="Batch dimension"):
        imp.inverse_transform(fx["outputs"]["inference"][:1].clone())
    stats = {k: v.numpy() for k, v in fx["statistics"].items()}
    with pytest.raises(AssertionError, match="median is not a method in the statistics"):
        InputImputer({"default": "none", "median": ["a"]}, indices_from_fixture(fx["indices"]), stats)
    with pytest.raises(TypeError):
        InputImputer({"default": "none", "mean": ["a"]}, indices_from_fixture(fx["indices"]), [1.0])


def test_copy_imputer_source_column_follows_the_data_index(fx):
    """The copy source is the DATA-input column of the named variable at either width (docstring of CopyImputer): at the inference width
    column 3 is ``e``, not ``d`` - what the recorded output shows; a NaN in the copied value trips the assertion on host tensors."""
    imp = build(fx, "CopyImputer")
    n2i = fx["indices"]["data_input_name_to_index"]
    kinds, _, sources = imp.program(6)
    m = fx["indices"]["model_input_name_to_index"]
    assert kinds[m["f"]] == COPY and sources[m["f"]] == n2i["d"] == m["e"] != m["d"]
    x = fx["inputs"]["inference"].clone()
    x[0, 0, 2, n2i["d"]] = float("nan")  # where ``f`` is NaN
    with pytest.raises(AssertionError, match="NaNs found in variable d to be copied"):
        imp.transform(x)
    far = CopyImputer({"default": "none", "g": ["a"]}, indices_from_fixture(fx["indices"]))  # data column 6 does not exist at width 6
    with pytest.raises(IndexError):
        far.transform(fx["inputs"]["inference"].clone())


def test_skip_imputation(fx):
    imp = build(fx, "InputImputer")
    x = fx["inputs"]["inference"]
    y = imp.transform(x, in_place=False, skip_imputation=True)
    same(y, x)
    assert y is not x and imp.nan_locations is None
    assert imp(x, in_place=True, skip_imputation=True) is x
    o = fx["outputs"]["inference"]
    same(imp.inverse_transform(o, in_place=False, skip_imputation=True), o)


def _pair(fx):
    di = indices_from_fixture(fx["indices"])
    stats = {k: v.numpy().copy() for k, v in fx["statistics"].items()}
    imp = InputImputer(fx["configs"]["InputImputer"], di, stats)
    with pytest.warns(UserWarning):
        nm = InputNormalizer(fx["configs"]["normalizer"], di, stats)
    return imp, nm


def test_processors_chain_both_directions(fx):
    c = fx["chain"]
    imp, nm = _pair(fx)
    pre, post = Processors([["imputer", imp], ["normalizer", nm]]), Processors([["imputer", imp], ["normalizer", nm]], inverse=True)
    same(pre(c["x"], in_place=False), c["forward"], "forward chain")
    assert torch.equal(imp.nan_locations, c["nan_locations"])
    same(post(c["y"], in_place=False), c["inverse"], "inverse chain")
    skip = Processors([["imputer", imp], ["normalizer", nm]])
    skip._awaiting_first_batch = False
    same(skip(c["x"], in_place=False, skip_imputation=True), c["forward_skip"], "skip_imputation through the chain")


def test_chains_predict_step_fuses(fx):
    imp, nm = _pair(fx)
    other = build(fx, "ConstantImputer")
    chain = AnemoiModelEncProcDec._edge_chain
    fwd = Processors([["imputer", imp], ["normalizer", nm]])
    inv = Processors([["imputer", imp], ["normalizer", nm]], inverse=True)
    assert chain(fwd, False) == (imp, nm) and chain(inv, True) == (imp, nm)
    assert chain(fwd, True) is None and chain(inv, False) is None  # a chain in the wrong direction
    assert chain(Processors([["normalizer", nm]]), False) == (None, nm) and chain(nm, False) == (None, nm)
    assert chain(Processors([["normalizer", nm], ["imputer", imp]]), False) is None
    assert chain(Processors([["imputer", imp], ["imputer2", other], ["normalizer", nm]]), False) is None
    assert chain(Processors([["imputer", imp], ["imputer2", other]]), False) is None
    assert chain(Processors([["imputer", imp], ["other", torch.nn.Identity()]]), False) is None
    assert chain(torch.nn.Identity(), False) is None


# ------------------------------------------------------------------------------- the kernels' restatements against the same records
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", list(CLASSES))
def test_kernel_restatements_equal_the_reference(fx, name, key):
    want = fx["cases"][name][key]
    imp = build(fx, name)
    x = fx["inputs"][key]
    y, mask = impute_ref(x, imp.program(x.shape[-1]))
    same(y, want["transform"], "impute_ref")
    if key.startswith("inference"):
        assert torch.equal(mask, want["nan_locations"])
    else:
        assert torch.equal(mask[..., fx["indices"]["data_input_full"].long()], want["nan_locations"])
    out = fx["outputs"][key]
    same(restore_nan_ref(out, want["nan_locations"], imp.restore_pairs(out.shape[-1])), want["inverse"], "restore_nan_ref")


def test_programs(fx):
    """The imputation program of each class at the inference width, and op 10 of the output column program."""
    m = fx["indices"]["model_input_name_to_index"]
    stats = fx["statistics"]
    d = fx["indices"]["data_input_name_to_index"]
    kinds, values, _ = build(fx, "InputImputer").program(6)
    assert kinds == [1 if n in ("a", "d", "e") else 0 for n in m]
    assert values[m["d"]] == float(stats["maximum"][d["d"]].float()) and values[m["a"]] == float(stats["mean"][d["a"]].float())
    assert build(fx, "InputImputer").program(6, torch.bfloat16)[1][m["d"]] == float(stats["maximum"][d["d"]].to(torch.bfloat16))
    kinds, values, _ = build(fx, "ConstantImputer").program(6, torch.float16)
    assert values[m["d"]] == float(torch.tensor(3.14, dtype=torch.float64).to(torch.float16)) and values[m["a"]] == 1.0
    mo = fx["indices"]["model_output_name_to_index"]
    assert build(fx, "InputImputer").inverse_program(len(mo)) == [(10, mo[n], m[n], 0.0, 0.0) for n in ("a", "d")]


def test_loss_mask_is_optional_and_tables_count_their_nan_ops(fx):
    """``record_nan_locations(loss_mask=False)`` - the fused predict_step - leaves nan_locations as ``transform`` does and builds no loss
    mask; the unmasked program tables refuse an op 10, the masked ones carry the count of them."""
    from anemoi_core_amd.layers.bounding import masked_program_tables, program_tables

    imp = build(fx, "InputImputer")
    x = fx["inputs"]["training"]
    imp.transform(x, in_place=False)
    want = imp.nan_locations.clone()
    assert imp.loss_mask_training is not None
    imp.record_nan_locations(x[:, 0].isnan(), x.shape[-1], loss_mask=False)
    assert torch.equal(imp.nan_locations, want) and imp.loss_mask_training is None
    prog = [(9, 0, 0, 1.0, 2.0)] + imp.inverse_program(len(fx["indices"]["model_output_name_to_index"]))
    with pytest.raises(ValueError, match="need a mask"):
        program_tables(prog, "cpu")
    t = masked_program_tables(prog, "cpu")
    assert t.n_nan_ops == 2 and t.ops.shape == (3, 4) and t.ops[1:, 0].tolist() == [10, 10]
    assert len(program_tables(prog[:1], "cpu")) == 2
