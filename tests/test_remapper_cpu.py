"""The remapper and the post-processors on CPU tensors against the reference's recorded behaviour (tests/golden/remapper.pt, written by
tests/golden/make_golden_remapper.py from preprocessing/remapper.py, mappings.py and postprocessor.py), the plain-torch restatements
(tests/remapper_refs.py) against the same records, the chains ``predict_step`` fuses and the extended column program.

Comparison rule.  The modules and the restatements run the same torch ops, so they are BIT-equal to each other on any host.  Against the
RECORDED outputs, everything exactly rounded - untouched columns, ``none``, ``affine``, the displaced atoms and their clamp, every
post-processor - is bit-equal as well.  The maps that call libm (log1p / expm1, pow - which is also how ``sqrt`` is taken -, log / exp, atanh,
tanh, asinh, sinh) are bit-equal only where torch dispatches to the recording host's vector ISA: another host's pow differs in the last bit on
a few elements.  Both implementations are within one ulp of the true value, so two results differ by at most 2 ulp at the libm step, 3 after
its rounding; the steps that follow scale that by at most 4 (the division by lambd = 0.25) or leave it relative.  Bound for those columns:
|got - want| <= 4 ulp * |want| + 2^-20 (rtol 2^-21, atol 2^-20), NaN and infinities at exactly the recorded places."""
import pytest
import torch

from anemoi_core_amd.layers.bounding import apply_program_torch, extended_program_tables
from anemoi_core_amd.models import AnemoiModelEncProcDec
from anemoi_core_amd.preprocessing import (ConditionalZeroPostprocessor, InputImputer, NormalizedReluPostprocessor, Postprocessor, Processors,
                                           Remapper)
from tests import remapper_refs as R
from tests.helpers import indices_from_fixture
from tests.model_edge_refs import assert_bits_equal
from tests.remapper_helpers import (KEYS, POST_CONFIGS, REMAP_CONFIGS, chain_members, input_columns, output_columns, post, remapper,
                                    statistics)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("remapper.pt")


EXACT = ("none", "affine", "displace_boundary_atoms")
RTOL, ATOL = 2.0 ** -21, 2.0 ** -20


def matches_record(got, want, columns, what, atol=ATOL):
    """got against a recorded output under the comparison rule of the module text; columns = {column: (method, kwargs)} of the remapped ones."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    for col in range(got.shape[-1]):
        g, w = got[..., col], want[..., col]
        if col not in columns or columns[col][0] in EXACT:
            assert_bits_equal(g, w, f"{what}, column {col}")
            continue
        assert torch.equal(g.isnan(), w.isnan()) and torch.equal(g.isinf(), w.isinf()), f"{what}, column {col}: NaN / inf elsewhere"
        torch.testing.assert_close(g, w, rtol=RTOL, atol=atol, equal_nan=True, msg=f"{what}, column {col} ({columns[col][0]})")


def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001 - the type and the text are what is compared
        return f"{type(e).__name__}: {e}"
    return None


# ------------------------------------------------------------------------------------------------ Remapper
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("config", REMAP_CONFIGS)
def test_remapper_equals_the_reference(fx, config, key):
    want = fx["remapper"][config][key]
    rm = remapper(fx, config)
    x, y = fx["inputs"][key], fx["outputs"][key]
    cols_in = R.columns_of(fx["remap_configs"][config], input_columns(fx, key))
    cols_out = R.columns_of(fx["remap_configs"][config], output_columns(fx, key))
    fwd, inv = rm.transform(x.clone(), in_place=False), rm.inverse_transform(y.clone(), in_place=False)
    matches_record(fwd, want["transform"], cols_in, "transform")
    matches_record(inv, want["inverse"], cols_out, "inverse")
    assert_bits_equal(rm(x, in_place=False), fwd, "forward()")
    assert_bits_equal(rm(y, in_place=False, inverse=True), inv, "forward(inverse=True)")
    x2, y2 = x.clone(), y.clone()
    assert rm.transform(x2) is x2 and rm.inverse_transform(y2) is y2  # in place: the same tensor comes back, changed
    assert_bits_equal(x2, fwd, "in-place transform")
    assert_bits_equal(y2, inv, "in-place inverse")
    if "transform_nan" in want:  # a NaN in every variable, every map clipping: NaN passes through
        matches_record(rm.transform(fx["inputs_nan"][key], in_place=False), want["transform_nan"], cols_in, "transform, NaN everywhere")
    # the restatements: the module's bits, hence the records under the same rule
    assert_bits_equal(R.remap(x, cols_in), fwd, "restated transform")
    assert_bits_equal(R.remap(y, cols_out, inverse=True), inv, "restated inverse")


@pytest.mark.parametrize("config", REMAP_CONFIGS)
def test_remapper_attributes_and_empty_state_dict(fx, config):
    want = fx["remapper"][config]["attributes"]
    rm = remapper(fx, config)
    strip = lambda names: [n.replace("_converter", "").replace("_transform", "").replace("inverse_", "").replace("noop", "none") for n in names]  # noqa: E731
    back = {"expm1": "log1p"}
    assert rm.remappers == strip(want["remappers"])  # the reference holds functions, here their method names
    assert rm.backmappers == [back.get(n, n) for n in strip(want["backmappers"])]
    for attr in ("index_training_input", "index_training_out", "index_inference_input", "index_inference_output", "remapper_kwargs",
                 "num_training_input_vars", "num_inference_input_vars", "num_training_output_vars", "num_inference_output_vars"):
        assert getattr(rm, attr) == want[attr], attr
    assert list(rm.state_dict().keys()) == fx["remapper"][config]["state_dict_keys"] == []
    rm.load_state_dict({}, strict=True)


def test_the_program_leaves_identities_out(fx):
    rm = remapper(fx, "lam0")  # atanh with rho = 0 is the identity going forward and a clamp coming back; `a` is listed under none
    cols = input_columns(fx, "inference")
    assert [c for c, _ in rm.entries(8)] == sorted(cols[n] for n in "bdie")
    assert [c for c, _ in rm.entries(8, inverse=True)] == sorted(output_columns(fx, "inference")[n] for n in "bdfi")  # e is a forcing
    assert len(rm.program(9)) == 9 and sum(e[0] != 0 for e in rm.program(9)) == 4


# ------------------------------------------------------------------------------------------------ post-processors
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", POST_CONFIGS)
def test_postprocessors_equal_the_reference(fx, name, key):
    want = fx["post"][name][key]
    pp = post(fx, name)
    y = fx["outputs"][key]
    assert_bits_equal(pp.transform(y, in_place=False), want["transform"], "transform")
    assert pp.transform(y) is y
    assert_bits_equal(pp.inverse_transform(y, in_place=False), want["inverse"], "inverse")
    assert_bits_equal(pp(y, in_place=False, inverse=True), want["inverse"], "forward(inverse=True)")
    y2 = y.clone()
    assert pp.inverse_transform(y2) is y2
    assert_bits_equal(y2, want["inverse"], "in-place inverse")
    # the same program through the column-program evaluator (what the autograd path runs)
    assert_bits_equal(apply_program_torch(y, pp.inverse_program(y.shape[-1])), want["inverse"], "apply_program_torch")


@pytest.mark.parametrize("name", POST_CONFIGS)
def test_postprocessor_attributes_and_empty_state_dict(fx, name):
    want = fx["post"][name]["attributes"]
    pp = post(fx, name)
    assert isinstance(pp, Postprocessor)
    for attr in ("index_training_output", "index_inference_output", "num_training_output_vars", "num_inference_output_vars"):
        assert getattr(pp, attr) == want[attr], attr
    for attr in ("masking_variable", "masking_variable_training_output", "masking_variable_inference_output"):
        if attr in want:
            assert getattr(pp, attr) == want[attr], attr
    assert len(pp.postprocessorfunctions) == len(want["functions"])
    for f, w in zip(pp.postprocessorfunctions, want["functions"]):
        if isinstance(w, float):  # a threshold or a fill value
            got = float(getattr(f, "threshold", f))
            assert got == w or (got != got and w != w)
        else:
            assert callable(f)
    assert list(pp.state_dict().keys()) == fx["post"][name]["state_dict_keys"] == []


def test_the_mask_is_taken_before_any_fill(fx):
    """ConditionalZero fills the masking variable itself (5.0 where f == 0): the fills of the other variables must still see the zeros."""
    pp = post(fx, "ConditionalZeroPostprocessor")
    prog = pp.inverse_program(8)
    f = output_columns(fx, "inference")["f"]
    assert [op[1] for op in prog][-1] == f and all(op[2] == f and op[0] == 11 for op in prog)
    y = fx["outputs"]["inference"]
    fills = [(op[1], op[3]) for op in prog]
    assert_bits_equal(R.conditional_fill(y, fills, f, "zero"), fx["post"]["ConditionalZeroPostprocessor"]["inference"]["inverse"], "restated fill")
    nan = post(fx, "ConditionalNaNPostprocessor")
    fills = [(op[1], float("nan")) for op in nan.inverse_program(8)]
    assert_bits_equal(R.conditional_fill(y, fills, f, "nan"), fx["post"]["ConditionalNaNPostprocessor"]["inference"]["inverse"], "restated NaN fill")


def test_masking_variable_must_be_an_output(fx):
    """Deviation: the reference indexes with None there, which is an accident."""
    idx, st = indices_from_fixture(fx["indices"]), statistics(fx)
    with pytest.raises(ValueError, match="masking variable 'e' is not an output variable"):
        ConditionalZeroPostprocessor({"default": "none", "remap": "e", 0: ["a"]}, idx, st)
    with pytest.raises(ValueError, match="masking variable None"):
        ConditionalZeroPostprocessor({"default": "none", 0: ["a"]}, idx, st)


# ------------------------------------------------------------------------------------------------ what the reference raises
def test_errors_equal_the_reference(fx):
    idx, st = indices_from_fixture(fx["indices"]), statistics(fx)
    n2i = fx["indices"]["data_input_name_to_index"]
    x_tr, y_tr = fx["inputs"]["training"], fx["outputs"]["training"]
    main = remapper(fx, "main")

    def remap_error(cfg, x=x_tr, inverse=False):
        def run():
            rm = Remapper(cfg, idx, st)
            return (rm.inverse_transform if inverse else rm.transform)(x, in_place=False)
        return run

    neg = x_tr.clone()
    neg[0, 1, 2, n2i["h"]] = -0.5
    zero = x_tr.clone()
    zero[1, 0, 3, n2i["d"]] = 0.0
    cases = {
        "remapper_transform_width": lambda: main.transform(torch.zeros(2, 2, 6, 5)),
        "remapper_inverse_width": lambda: main.inverse_transform(torch.zeros(2, 2, 6, 5)),
        "remapper_unknown_method": remap_error({"default": "none", "cbrt": ["a"]}),
        "remapper_unknown_default": remap_error({"default": "mean-std", "log1p": ["a"]}),
        "sqrt_negative": remap_error({"default": "none", "sqrt": ["h"]}, neg),
        "sqrt_nan": remap_error({"default": "none", "sqrt": ["b"]}, fx["inputs_nan"]["training"]),
        "power_negative": remap_error({"default": "none", "power": ["h"]}, neg),
        "boxcox_negative": remap_error({"default": "none", "boxcox": ["h"]}, neg),
        "boxcox_log_zero": remap_error({"default": "none", "boxcox": ["d"], "method_kwargs": {"boxcox": {"lambd": 0.0}}}, zero),
        "power_lambda": remap_error({"default": "none", "power": ["b"], "method_kwargs": {"power": {"lambd": 0.0}}}),
        "power_lambda_inverse": remap_error({"default": "none", "power": ["b"], "method_kwargs": {"power": {"lambd": -1.0}}}, y_tr, inverse=True),
        "atanh_rho": remap_error({"default": "none", "atanh": ["f"], "method_kwargs": {"atanh": {"rho": -1.0}}}),
        "atoms_target_side": remap_error({"default": "none", "displace_boundary_atoms": ["i"],
                                          "method_kwargs": {"displace_boundary_atoms": {"lower_atom": 0.0, "lower_target": 0.5}}}),
        "atoms_upper_target_side": remap_error({"default": "none", "displace_boundary_atoms": ["i"],
                                                "method_kwargs": {"displace_boundary_atoms": {"upper_atom": 1.0, "upper_target": 1.0}}}),
        "atoms_target_missing": remap_error({"default": "none", "displace_boundary_atoms": ["i"],
                                             "method_kwargs": {"displace_boundary_atoms": {"upper_atom": 1.0}}}),
        "affine_scale": remap_error({"default": "none", "affine": ["a"], "method_kwargs": {"affine": {"scale": 0.0}}}),
        "affine_scale_inverse": remap_error({"default": "none", "affine": ["a"], "method_kwargs": {"affine": {"scale": 0.0}}}, y_tr, inverse=True),
        "post_forcing": lambda: Postprocessor({"default": "none", "relu": ["e"]}, idx, st),
        "post_unknown_method": lambda: Postprocessor({"default": "none", "tanh": ["a"]}, idx, st),
        "post_width": lambda: post(fx, "Postprocessor").inverse_transform(torch.zeros(2, 2, 6, 5)),
        "conditional_width": lambda: post(fx, "ConditionalZeroPostprocessor").inverse_transform(torch.zeros(2, 2, 6, 5)),
        "normalized_relu_normalizer": lambda: NormalizedReluPostprocessor({"default": "none", "normalizer": "robust", 1.0: ["a"]}, idx, st),
    }
    assert set(cases) == set(fx["errors"])
    for name, fn in cases.items():
        assert raised(fn) == fx["errors"][name], name


# ------------------------------------------------------------------------------------------------ chains
def _members(fx):
    c = fx["chain"]
    return chain_members(indices_from_fixture(fx["indices"]), statistics(fx), fx["remap_configs"]["main"], fx["normalizer_config"], c["relu_config"],
                         c["zero_config"])


def test_processors_chain_equals_the_reference(fx):
    c = fx["chain"]
    members = _members(fx)
    every = lambda cols: {col: ("libm", {}) for col in cols.values()}  # noqa: E731 - the remapper touches every column of this chain
    fwd, inv = Processors(members)(c["x"], in_place=False), Processors(members, inverse=True)(c["y"], in_place=False)
    # (the normaliser multiplies a remapped value of up to 4 by up to 1 / stdev = 2 and may cancel it against its offset: 3 ulp of 8 = 2^-18)
    matches_record(fwd, c["forward"], every(fx["indices"]["model_input_name_to_index"]), "forward chain", atol=2.0 ** -18)
    matches_record(inv, c["inverse"], every(fx["indices"]["model_output_name_to_index"]), "inverse chain")
    assert int((inv[..., fx["indices"]["model_output_name_to_index"]["h"]] == 5.0).sum()) == 8  # the fills the reference made
    # the chain's output column program (every member's inverse ops, last member first) through the evaluator: the modules' bits
    prog = [op for _, m in reversed(members) for op in m.inverse_program(c["y"].shape[-1])]
    got = apply_program_torch(c["y"], prog)
    assert_bits_equal(got, inv, "the output column program")
    ops_t, par_t = extended_program_tables(prog, c["y"].shape[-1], "cpu")
    assert ops_t.shape == (len(prog), 4) and par_t.shape == (len(prog), 2) and ops_t.dtype == torch.int32
    with pytest.raises(ValueError, match="outside"):
        extended_program_tables([(11, 0, 8, 0.0, 0.0)], 8, "cpu")
    with pytest.raises(ValueError, match="outside"):
        extended_program_tables([(1, 8, 0, 0.0, 0.0)], 8, "cpu")


def test_chains_predict_step_fuses(fx):
    idx, st = indices_from_fixture(fx["indices"]), statistics(fx)
    (_, zero), (_, rm), (_, nm), (_, relu) = members = _members(fx)
    imp = InputImputer({"default": "none", "mean": ["a"]}, idx, st)
    other = Remapper(fx["remap_configs"]["clip"], idx, st)
    chain = AnemoiModelEncProcDec._edge_chain
    P = lambda *ms, inverse=False: Processors([[f"m{i}", m] for i, m in enumerate(ms)], inverse=inverse)  # noqa: E731
    assert chain(Processors(members), False) == (None, nm, rm, [zero, rm, nm, relu])
    assert chain(Processors(members, inverse=True), True) == (None, nm, rm, [zero, rm, nm, relu])
    assert chain(Processors(members), True) is None  # a chain in the wrong direction
    assert chain(P(rm, nm), False) == (None, nm, rm, [rm, nm])
    assert chain(P(imp, rm, nm), False) == (imp, nm, rm, [imp, rm, nm])
    assert chain(P(imp, zero, rm, relu, nm), False) == (imp, nm, rm, [imp, zero, rm, relu, nm])
    assert chain(P(nm, relu), False) == (None, nm, None, [nm, relu])  # post-processors alone fuse too
    assert chain(P(imp, nm), False) == (imp, nm) and chain(P(nm), False) == (None, nm)  # as before
    assert chain(P(nm, rm), False) is None  # a Remapper after the normaliser
    assert chain(P(rm, imp, nm), False) is None  # an imputer after the Remapper
    assert chain(P(rm, other, nm), False) is None  # two Remappers
    assert chain(P(zero, imp, rm, nm), False) is None  # a post-processor that would have to follow the NaN restoration
    assert chain(P(rm, relu), False) is None  # no normaliser
    assert chain(P(rm, torch.nn.Identity(), nm), False) is None  # a member of another type
