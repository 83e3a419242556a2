"""CPU checks of the spherical-harmonic transforms and the spectral Ornstein residual: this package's Legendre tables and the float64
restatement (tests/sht_refs.py) against what the reference recorded (tests/golden/sht.pt), the launch plan (csrc/sht_plan.h through
ops.sht_plan), the ABI-25 entries, the modules' mirror of the reference's attributes, and the model wiring."""
import os
import re

import numpy as np
import pytest
import torch

from anemoi_core_amd import _lib, ops
from tests import sht_refs as R
from tests.test_abi_cpu import HEADER, header_functions

NEW_ENTRIES = ("anemoi_sht_plan", "anemoi_sht_fwd", "anemoi_sht_inv", "anemoi_ornstein_combine_fwd")
GRIDS = {"o8": R.octahedral(16), "o96": R.octahedral(192), "o1280": R.octahedral(2560), "regular": [64] * 32, "odd": [5, 9, 9, 5]}


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


# ---------------------------------------------------------------------------------------------- tables and restatement
def test_fixture_holds_the_cases_and_stays_small(fx):
    assert os.path.getsize(os.path.join(R.GOLDEN, "sht.pt")) < 1 << 20
    assert set(fx["sht"]) == {"o8_t7", "o8_t2", "o16_t10", "o16_t15", "o32_t12", "o32_t31", "reg8x16_t7", "reg8x16_t3", "odd_t3", "odd_t2"}
    e = fx["sht"]["o16_t10"]
    assert e["truncation"] + 1 == min(e["lons_per_lat"]) // 2 + 1  # the Nyquist mode of the polar rings
    e = fx["sht"]["o16_t15"]
    assert e["truncation"] + 1 > min(e["lons_per_lat"]) // 2 + 1  # clipped modes on the short rings


def test_legendre_tables_equal_the_references(fx):
    seen = 0
    for name, e in fx["sht"].items():
        if "weight" not in e:
            continue
        W, P = R.tables(e["lons_per_lat"], e["truncation"])
        assert W.shape == tuple(e["weight"].shape) and W.dtype == np.float64
        assert R.rel_err(W, e["weight"].numpy()) <= 1e-12, name
        assert R.rel_err(P, e["pct"].numpy()) <= 1e-12, name
        L = e["truncation"] + 1
        assert all(float(np.abs(W[m, :m]).max(initial=0.0)) == 0.0 for m in range(L))  # exact zeros where l < m
        seen += 1
    assert seen >= 6


def test_gauss_legendre_rule_integrates_polynomials_exactly():
    from anemoi_core_amd.layers.spectral_helpers import gauss_legendre

    for n in (1, 2, 5, 16, 192):
        x, w = gauss_legendre(n)
        assert np.all(np.diff(x) > 0) and abs(w.sum() - 2.0) < 1e-13
        for p in (min(2, 2 * n - 2), 2 * n - 2):  # an n-point rule is exact up to degree 2 n - 1
            assert abs((w * x**p).sum() - 2.0 / (p + 1)) < 1e-13


def test_restatement_reproduces_every_fixture_case(fx):
    for name, e in fx["sht"].items():
        lons, t = e["lons_per_lat"], e["truncation"]
        assert R.rel_err(R.forward64(e["x"].numpy(), lons, t), e["fwd64"].numpy()) <= 1e-11, name
        assert R.rel_err(R.inverse64(e["c"].numpy(), lons, t), e["inv64"].numpy()) <= 1e-11, name
        fwd = R.forward64(e["x"].numpy(), lons, t)
        L = t + 1
        assert all(float(np.abs(fwd[:, l, l + 1:]).max(initial=0.0)) == 0.0 for l in range(L)), name


def test_restatement_lscale_is_a_per_degree_factor(fx):
    e = fx["sht"]["o8_t7"]
    lons, t = e["lons_per_lat"], e["truncation"]
    s = np.linspace(0.25, 1.5, 2 * (t + 1)).reshape(2, t + 1)
    c = e["c"].numpy()
    a = R.inverse64(c, lons, t, lscale=s)
    b = R.inverse64(c * s[:, :, None], lons, t)
    assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()


def test_restated_residual_reproduces_the_reference(fx):
    from tests.sht_refs import build_layer, layer_input

    for key, e in fx["ornstein"].items():
        if key == "init":
            continue
        layer, grid, lmax, variant = build_layer(key, e)
        assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == e["keys"], key
        assert list(layer.state_dict().keys()) == list(e["keys"].keys()), key
        sd = {k: v.double().numpy() for k, v in layer.state_dict().items()}
        x = layer_input(layer, e)
        out = R.ornstein64(sd, x[:, -1, 0].double().numpy(), grid, lmax, layer._internal_input_idx, layer._regressors_input_idx,
                           getattr(layer, "_truncation_input_idx", []), R.ORN_THETA["theta_buff"], variant["truncate"],
                           variant.get("anti_aliasing", True))
        assert R.rel_err(out, e["out64"][:, 0].numpy()) <= 1e-11, key


def test_residual_initialisation_equals_the_references(fx):
    from tests.sht_refs import make_layer

    init = fx["ornstein"]["init"]
    stats = {k: v.numpy() for k, v in init["statistics"].items()}
    for name, kw in (("stats", dict(theta_init=0.0, theta_buff=0.0, statistics=stats)), ("fixed", dict(theta_init=0.3, theta_buff=0.1)),
                     ("no_mean", dict(theta_init=0.3, theta_buff=0.1, use_mean=False))):
        layer = make_layer("octahedral", 3, R.ORN_VARIANTS["trunc_aa"], **kw)
        sd = layer.state_dict()
        assert list(sd.keys()) == list(init["state"][name].keys())
        for k, v in sd.items():
            assert torch.equal(v, init["state"][name][k]), (name, k)
    with pytest.raises(ValueError, match="Unsupported grid type"):
        make_layer("healpix", 2, R.ORN_VARIANTS["plain"])


# ---------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("grid", ["o8", "o96", "o1280", "regular"])
@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_plan_lds_bound_holds_whatever_the_ring_length(grid, direction):
    lons = GRIDS[grid]
    for trunc in (1, len(lons) // 2 - 1, len(lons) - 1, len(lons)):
        for F in (1, 3, 17, 65, 80):
            p = ops.sht_plan(direction, F, lons, trunc)
            elem = 4 if direction == "forward" else 8
            assert p["lds_bound"] == 8 * 1024
            assert p["lds_bytes"] == p["field_tile"] * p["chunk"] * elem <= p["lds_bound"], (grid, trunc, F)
            assert p["chunk"] >= 1 and p["field_tile"] in (1, 2, 4, 8)
            assert p["workspace_bytes"] == F * len(lons) * (trunc + 1) * 8
    big = ops.sht_plan(direction, 80, GRIDS["o1280"], 1279)
    small = ops.sht_plan(direction, 80, GRIDS["o8"], 15)
    assert big["lds_bytes"] == big["lds_bound"] and small["lds_bytes"] < big["lds_bytes"]  # O1280's rings take more passes, not more LDS


@pytest.mark.parametrize("F", R.FIELDS)
@pytest.mark.parametrize("grid,trunc", [("o8", 15), ("o8", 5), ("odd", 3), ("regular", 31), ("o96", 95)])
def test_plan_covers_every_field_ring_and_mode_exactly_once(F, grid, trunc):
    lons = GRIDS[grid]
    K, M = len(lons), trunc + 1
    for direction in ("forward", "inverse"):
        p = ops.sht_plan(direction, F, lons, trunc)
        ft, T, rows = p["field_tile"], p["ring_threads"], p["leg_rows"]
        fields = np.zeros(F, dtype=np.int64)
        for z in range(p["ring_grid"][2]):
            fields[z * ft:min(F, (z + 1) * ft)] += 1
        assert np.all(fields == 1) and p["ring_grid"][2] == p["leg_grid"][2]
        assert p["ring_grid"][0] == K
        # ring launch: outputs of ring k are M modes (forward) or n_k points (inverse), tiled by ring_threads
        for k, n in enumerate(lons):
            items = M if direction == "forward" else n
            hit = np.zeros(items, dtype=np.int64)
            for y in range(p["ring_grid"][1]):
                hit[y * T:min(items, (y + 1) * T)] += 1
            assert np.all(hit == 1), (direction, k)
        # Legendre launch: (row, mode) with rows = degrees (forward) or rings (inverse)
        n_rows = M if direction == "forward" else K
        hit = np.zeros((n_rows, M), dtype=np.int64)
        for bx in range(p["leg_grid"][0]):
            for by in range(p["leg_grid"][1]):
                hit[by * rows:min(n_rows, (by + 1) * rows), bx * 64:min(M, (bx + 1) * 64)] += 1
        assert np.all(hit == 1), direction
        # the ring kernel walks a ring's points / modes in whole chunks
        extent = max(lons) if direction == "forward" else min(M, max(lons) // 2 + 1)
        assert p["chunk"] == min(extent, p["lds_bound"] // (ft * (4 if direction == "forward" else 8)))


def test_plan_refuses_bad_shapes():
    lons = GRIDS["o8"]
    for trunc in (0, -1, len(lons) + 1):
        with pytest.raises(ValueError, match="truncation"):
            ops.sht_plan("forward", 3, lons, trunc)
    with pytest.raises(ValueError, match="ring 1 has 0 points"):
        ops.sht_plan("inverse", 3, [4, 0, 4], 2)
    with pytest.raises(ValueError, match="0 rings"):
        ops.sht_plan("forward", 3, [], 1)
    assert ops.sht_plan("forward", 3, lons, len(lons))["field_tile"] == 4  # truncation = nlat is the reference's upper end


# ---------------------------------------------------------------------------------------------- ABI 25
def test_abi_25_entries_are_declared_bound_built_and_cited():
    assert _lib.ABI_VERSION >= 25  # the entries came with ABI 25; later versions keep them
    decl = header_functions()
    lib = _lib.load()
    assert lib.anemoi_hip_abi_version() == _lib.ABI_VERSION
    text = open(HEADER).read()
    assert f"#define ANEMOI_HIP_ABI_VERSION {_lib.ABI_VERSION}" in text
    for name in NEW_ENTRIES:
        assert name in decl and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][0]) == decl[name], name
        assert hasattr(lib, name), name
        # the comment block in front of the declaration names what the entry replaces in the reference
        head = text[:re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M).start()]
        comment = head[head.rindex("/*"):]
        assert "Replaces:" in comment and comment.count("*/") == 1, name
        assert re.search(r"layers/\w+\.py:\d+", comment), name


# ---------------------------------------------------------------------------------------------- modules
def test_modules_mirror_the_references_attributes(fx):
    from anemoi_core_amd.layers.spectral_helpers import InverseSphericalHarmonicTransform, SphericalHarmonicTransform

    e = fx["sht"]["o8_t7"]
    lons, t = e["lons_per_lat"], e["truncation"]
    for name, mod in (("forward", SphericalHarmonicTransform(lons, t, use_graphed_rfft=True)),
                      ("inverse", InverseSphericalHarmonicTransform(lons, t, use_graphed_irfft=True))):
        rec = fx["modules"][name]
        for attr, want in rec["attributes"].items():
            got = getattr(mod, attr)
            assert (list(got) if isinstance(got, (list, tuple)) else got) == want, (name, attr)
        assert {k: (tuple(v.shape), str(v.dtype)) for k, v in mod.named_buffers()} == rec["buffers"], name
        assert list(mod.state_dict().keys()) == rec["state_dict_keys"] == [], name  # non-persistent: the state_dict gains nothing
    with pytest.raises(AssertionError, match="Truncation"):
        SphericalHarmonicTransform(lons, len(lons) + 1)
    with pytest.raises(AssertionError, match="Truncation"):
        SphericalHarmonicTransform(lons, 0)


def test_transform_wrappers_and_cpu_refusal():
    from anemoi_core_amd.layers.spectral_transforms import InverseOctahedralSHT, InverseRegularSHT, OctahedralSHT, RegularSHT

    o, r = OctahedralSHT(16), RegularSHT(8, truncation=5)
    assert o.lons_per_lat == R.octahedral(16) and o._sht.truncation == 7 and r.lons_per_lat == [16] * 8 and r.nlon == 16 and r._sht.truncation == 5
    assert InverseOctahedralSHT(16, truncation=4)._isht.truncation == 4 and InverseRegularSHT(8)._isht.n_grid_points == 128
    with pytest.raises(RuntimeError, match="MI355X"):
        o(torch.zeros(1, 1, 1, 544, 2))
    with pytest.raises(RuntimeError, match="MI355X"):
        InverseRegularSHT(8)(torch.zeros(2, 4, 4, dtype=torch.complex64))
    c = torch.complex(torch.arange(24.0).reshape(1, 1, 1, 3, 4, 2), torch.ones(1, 1, 1, 3, 4, 2))
    assert torch.equal(o.power_spectral_density(c), (c.real**2 + c.imag**2).sum(-2))
    assert torch.equal(o.cross_spectral_density(c, 2 * c), 2 * o.power_spectral_density(c))


def test_twiddles_are_rounded_from_float64():
    tw = ops.sht_twiddles([5, 8])
    assert tw.dtype == np.float64 and tw.shape == (13, 2)
    assert tw[0].tolist() == [1.0, -0.0] and abs(tw[5 + 2][0]) < 1e-16 and tw[5 + 2][1] == -1.0  # e^{-i pi / 2}
    t = np.arange(5)
    assert np.allclose(tw[:5, 0] + 1j * tw[:5, 1], np.exp(-2j * np.pi * t / 5), atol=1e-16)


# ---------------------------------------------------------------------------------------------- the model
def test_model_accepts_the_spectral_residual(fx):
    from tests.sht_refs import build_model

    model, x = build_model(fx)
    from anemoi_core_amd.layers.residual import SpectralOrnsteinConnection

    assert isinstance(model.residual["data"], SpectralOrnsteinConnection)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == fx["model"]["keys"]
    assert model._truncated["data"] and model._ornstein["data"]
    with pytest.raises(RuntimeError, match="MI355X"):
        model.residual["data"](x)
