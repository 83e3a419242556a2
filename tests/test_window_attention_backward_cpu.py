"""The window attention's backward on the host: the C ABI of the new entry point (header, ctypes signatures, built library) and the
refusals that need no GPU.  Nothing is launched."""
import ctypes as C
import re

import pytest
import torch

from anemoi_core_amd import _lib, ops
from tests.test_abi_cpu import HEADER, header_functions


def test_header_signatures_and_library_agree_on_the_backward_symbol():
    name = "anemoi_window_attention_bwd"
    decl = header_functions()
    assert name in decl and name in _lib.SIGNATURES
    argtypes, restype = _lib.SIGNATURES[name]
    assert len(argtypes) == decl[name] and restype is C.c_int
    # the header's parameter list, type by type
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    params = re.search(name + r"\s*\((.*?)\);", text, flags=re.S).group(1).split(",")
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "anemoi_dtype_t": C.c_int}
    want = [C.c_void_p if "*" in p else kinds[p.split()[-2]] for p in params]
    assert argtypes == want
    lib = _lib.load()
    assert hasattr(lib, name) and lib.anemoi_hip_abi_version() == _lib.ABI_VERSION >= 22
    assert (ops.WINDOW_BWD_QUERY_PASS, ops.WINDOW_BWD_KEY_PASS) == tuple(
        int(re.search(rf"#define ANEMOI_WINDOW_BWD_{n}_PASS (\d+)", text).group(1)) for n in ("QUERY", "KEY"))


def test_backward_entry_point_checks_its_arguments_before_any_launch():
    """Argument errors return before a pointer is touched: zero rows are OK, an unsupported head dimension is ANEMOI_E_UNSUPPORTED."""
    fn = _lib.load().anemoi_window_attention_bwd

    def call(batch, seq, H, d, passes=3):
        return fn(0, 64, 0, 64, 0, 64, 0, 64, 0, 64, 0, 0, 64, 0, 64, 0, 64, 0, batch, seq, H, d, 8, 0.125, 0.0, 0, passes, _lib.BF16, 0)

    assert call(0, 100, 2, 32) == 0 and call(3, 0, 2, 32) == 0
    assert call(1, 100, 2, 48) == -2
    assert "head dimension 48 not supported; supported: 32, 64, 128" in _lib.load().anemoi_hip_last_error().decode()
    assert call(1, 100, 2, 32) == -1  # null pointers
    assert call(4096, 100, 16, 32) == -1  # batch * H >= 65536
    assert call(0, 100, 2, 32, passes=4) == -1


def test_cpu_tensors_that_require_grad_raise_the_device_error():
    x = torch.zeros(16, 64, requires_grad=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.window_attention(x, x, x, 2, 4)
    with pytest.raises(ValueError, match="supported"):
        y = torch.zeros(16, 96, requires_grad=True)  # d = 48
        ops.window_attention(y, y, y, 2, 4)
    z = torch.zeros(16, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.window_attention_bwd(z, z, z, z, z, torch.zeros(16, 2), 2, 4)


def test_forbid_autograd_keeps_three_refusals():
    from anemoi_core_amd.layers.attention import forbid_autograd

    lin = torch.nn.Linear(4, 4)
    x = torch.zeros(2, 4)
    with pytest.raises(NotImplementedError, match="backward kernel.*GPU"):
        forbid_autograd(lin, x)
    with pytest.raises(NotImplementedError, match="dropout.*backward kernel"):
        forbid_autograd(lin.train(), x, dropout_p=0.1)
    with torch.no_grad():
        forbid_autograd(lin, x)  # inference: nothing to refuse
    forbid_autograd(lin.eval().requires_grad_(False), x, dropout_p=0.1)
