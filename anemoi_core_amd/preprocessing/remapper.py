"""The remapper - mirror of the reference's ``anemoi.models.preprocessing.remapper.Remapper`` (with the maps of its ``mappings`` module),
written from its behaviour: same constructor arguments, same public attributes (``remappers``, ``backmappers``, ``index_training_input``,
``index_training_out``, ``index_inference_input``, ``index_inference_output``, ``remapper_kwargs`` and the four ``num_*_vars``), an empty
state_dict.

``transform(x [..., vars])`` maps single variables through ``log1p``, ``sqrt``, ``boxcox``, ``atanh``, ``asinh``, ``power``,
``displace_boundary_atoms``, ``affine`` or ``none``; ``inverse_transform`` maps the output variables back.  ``method_kwargs[method]`` is
shared by all variables of a method.  Every map is a sequence of element-wise steps, each of which rounds to the data dtype (the reference
runs them as in-place torch ops); NaN passes through all of them.

A map in one direction with its keyword arguments becomes an ENTRY ``(op, flags, p0, p1, p2, p3)`` of the remap program
(include/anemoi_hip.h); entries are built when a direction is first used, so what the reference raises at call time (a negative rho, a
target on the wrong side of its atom, lambd <= 0, a zero scale) is raised at call time here too.  CPU tensors evaluate the entries with plain
torch (``apply_entry_torch``: a division by a scalar is a division there; torch's device kernels multiply by the scalar's fp32 reciprocal, and
``device_entry`` gives the kernels that reciprocal); MI355X tensors take ONE launch of ``ops.remap_columns`` for all variables, which in place touches the
remapped columns only.  The forward domain assertions (``power`` / ``sqrt`` / ``boxcox`` without ``clip_negative``) are counted per column by
that kernel and read back after the launch - one synchronisation, as the reference's own ``.all()`` costs; ``check_domain = False`` drops
the read (a forward captured in a hipGraph), and a negative under the power is then a NaN, as in torch without the assertion.  Thresholds
and bounds reach the kernel as fp32, as torch's ROCm kernels take their scalars; on CPU tensors torch rounds them to a 16-bit data dtype."""
from __future__ import annotations

import logging
import math
from typing import Optional

import torch
from torch import Tensor

from . import BasePreprocessor

LOGGER = logging.getLogger(__name__)

# the remap ops and flags of include/anemoi_hip.h
(NONE, LOG1P, EXPM1, POWER, POWER_INV, BOXCOX, BOXCOX_INV, LOG, EXP, ATANH, ATANH_INV, ASINH, ASINH_INV, DISPLACE, CLAMP, AFFINE,
 AFFINE_INV) = range(17)
CLIP, TANGENT, LOWER, UPPER = 1, 2, 4, 8
_IDENTITY = (NONE, 0, 0.0, 0.0, 0.0, 0.0)

ASSERTIONS = {
    POWER: "Power transform input x must satisfy x >= 0, or use with clip_negative=True to clip negative values to 0.",
    BOXCOX: "input x must me greater or equal to 0, or use with clip_negative=True to clip negative values to 0",
    LOG: "input x must be strictly positive for parameter lambd == 0",
}


def _pow_flags(exponent: float) -> int:
    """How torch's scalar pow takes this exponent: 0.5 as sqrt, 2 as x * x, 3 as x * x * x, 1 as a copy, anything else as pow."""
    return {0.5: 1, 2.0: 2, 3.0: 3, 1.0: 4}.get(float(exponent), 0) << 4


def _entry(op: int, flags: int = 0, p0=0.0, p1=0.0, p2=0.0, p3=0.0) -> tuple:
    return (op, flags, float(p0), float(p1), float(p2), float(p3))


# ---- one builder per method: (inverse?) -> entry; the signatures are those of the reference's maps, so a misspelt keyword is a TypeError
def _none(inverse):
    return _IDENTITY


def _log1p(inverse):
    return _entry(EXPM1 if inverse else LOG1P)


def _power(inverse, lambd=0.33, clip_negative=False, tangent_linear_above_one=False):
    if inverse:
        assert lambd > 0, f"For inverse power transform, parameter lambd {lambd} must satisfy lambd > 0."
        return _entry(POWER_INV, (TANGENT if tangent_linear_above_one else 0) | _pow_flags(1 / lambd), 1 / lambd, 1.0 - lambd, lambd)
    assert lambd > 0, f"For power transform, parameter lambd {lambd} must satisfy lambd > 0."
    flags = (CLIP if clip_negative else 0) | (TANGENT if tangent_linear_above_one else 0) | _pow_flags(lambd)
    return _entry(POWER, flags, lambd, 1.0 - lambd)


def _sqrt(inverse):
    return _power(inverse, lambd=0.5)


def _boxcox(inverse, lambd=0.5, clip_negative=False):
    if lambd == 0:
        return _entry(EXP if inverse else LOG)
    if inverse:
        return _entry(BOXCOX_INV, _pow_flags(1 / lambd), lambd, 1 / lambd)
    return _entry(BOXCOX, (CLIP if clip_negative else 0) | _pow_flags(lambd), lambd, lambd)


def _atanh(inverse, rho=2.0):
    if rho == 0:
        return _entry(CLAMP, LOWER | UPPER, 0.0, 1.0) if inverse else _IDENTITY
    if not inverse and not (0 <= rho):
        raise ValueError(f"rho must satisfy 0 < rho , got {rho}")
    return _entry(ATANH_INV if inverse else ATANH, 0, math.tanh(rho), rho)


def _asinh(inverse, c=1.0):
    return _entry(ASINH_INV if inverse else ASINH, 0, c)


def _displace_boundary_atoms(inverse, lower_atom=None, upper_atom=None, lower_target=None, upper_target=None, eps=0.0):
    flags = (LOWER if lower_atom is not None else 0) | (UPPER if upper_atom is not None else 0)
    if inverse:
        if not flags:
            raise RuntimeError("torch.clamp: At least one of 'min' or 'max' must not be None")
        return _entry(CLAMP, flags, lower_atom or 0.0, upper_atom or 0.0)
    p = [0.0, 0.0, 0.0, 0.0]
    if lower_atom is not None:
        assert lower_target is not None, "To displace lower boundary atom, lower_target must be specified"
        assert lower_target < lower_atom, "lower_target must be less than lower_atom"
        p[0], p[1] = lower_atom + eps, lower_target
    if upper_atom is not None:
        assert upper_target is not None, "To displace upper boundary atom, upper_target must be specified"
        assert upper_target > upper_atom, "upper_target must be greater than upper_atom"
        p[2], p[3] = upper_atom - eps, upper_target
    return _entry(DISPLACE, flags, *p) if flags else _IDENTITY


def _affine(inverse, scale=1.0, shift=0.0):
    assert scale != 0, "scale must be non-zero for a reversible affine transform"
    return _entry(AFFINE_INV if inverse else AFFINE, 0, scale, shift)


# where an entry holds a scalar DIVISOR (index into the entry): torch's device kernels multiply by its fp32 reciprocal, and so do the kernels
_DIVISOR = {POWER_INV: 4, BOXCOX: 3, ATANH: 3, ATANH_INV: 2, ASINH_INV: 2, AFFINE_INV: 2}


def device_entry(entry: tuple) -> tuple:
    """The entry as the device tables hold it: a scalar divisor replaced by its fp32 reciprocal, 1.f / float(divisor) (remap_core.h)."""
    slot = _DIVISOR.get(entry[0])
    if slot is None:
        return entry
    rcp = float(torch.ones((), dtype=torch.float32) / torch.tensor(entry[slot], dtype=torch.float32))
    return entry[:slot] + (rcp,) + entry[slot + 1:]


METHODS = {"log1p": _log1p, "sqrt": _sqrt, "boxcox": _boxcox, "atanh": _atanh, "asinh": _asinh, "power": _power,
           "displace_boundary_atoms": _displace_boundary_atoms, "affine": _affine, "none": _none}


def _pow(v: Tensor, exponent: float) -> Tensor:
    return torch.pow(v, exponent)


def apply_entry_torch(v: Tensor, entry: tuple, check: bool = False) -> Tensor:
    """One entry on a tensor, out of place and differentiable: the same steps in the same order as the kernels (remap_core.h), each a
    torch op in v's dtype.  ``check``: raise the reference's AssertionError where the input leaves the map's domain."""
    op, flags, p0, p1, p2, p3 = entry
    if op in (POWER, BOXCOX):
        if flags & CLIP:
            v = torch.clamp(v, min=0.0)
        elif check:
            assert bool(v.ge(0.0).all()), ASSERTIONS[op]
    if op == NONE:
        return v
    if op == LOG1P:
        return torch.log1p(v)
    if op == EXPM1:
        return torch.expm1(v)
    if op == POWER:
        pw = _pow(v, p0)
        return torch.where(pw > 1.0, v.mul(p0).add(p1), pw) if flags & TANGENT else pw
    if op == POWER_INV:
        pw = _pow(torch.clamp(v, min=0.0), p0)
        return torch.where(pw > 1.0, v.sub(p1).div(p2), pw) if flags & TANGENT else pw
    if op == BOXCOX:
        return _pow(v, p0).sub(1.0).div(p1)
    if op == BOXCOX_INV:
        return _pow(torch.clamp(v.mul(p0).add(1.0), min=0.0), p1)
    if op == LOG:
        if check:
            assert bool(v.gt(0.0).all()), ASSERTIONS[op]
        return torch.log(v)
    if op == EXP:
        return torch.exp(v)
    if op == ATANH:
        return torch.atanh(v.mul(2.0).sub(1.0).mul(p0)).div(p1)
    if op == ATANH_INV:
        return torch.clamp(torch.tanh(v.mul(p1)).div(p0).add(1.0).mul(0.5), min=0.0, max=1.0)
    if op == ASINH:
        return torch.asinh(v.mul(p0))
    if op == ASINH_INV:
        return torch.sinh(v).div(p0)
    if op == DISPLACE:
        if flags & LOWER:
            v = v.masked_fill(v <= p0, p1)
        if flags & UPPER:
            v = v.masked_fill(v >= p2, p3)
        return v
    if op == CLAMP:
        return torch.clamp(v, p0 if flags & LOWER else None, p1 if flags & UPPER else None)
    if op == AFFINE:
        return v.mul(p0).add(p1)
    if op == AFFINE_INV:
        return v.sub(p1).div(p0)
    raise ValueError(f"unknown remap op {op}")


class Remapper(BasePreprocessor):
    """Remap and convert single variables (see the module text)."""

    supported_methods = {name: [name, name] for name in METHODS}  # method -> [forward, inverse], by name: the maps live in METHODS

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self.check_domain = True
        self._device_cache: dict = {}
        self._create_remapping_indices(statistics)
        n = len(self.remappers)
        assert len(self.index_training_input) == len(self.index_inference_input) == len(self.index_inference_output) == \
            len(self.index_training_out) == n, "Error creating conversion indices"

    def _create_remapping_indices(self, statistics=None) -> None:
        """One entry per data-input variable (those on ``none`` included), in their order: the column at each of the four widths (None
        where the variable is absent there), the names of its maps and the keyword arguments of its method."""
        d, m = self.data_indices.data, self.data_indices.model
        tr_in, inf_in = d.input.name_to_index, m.input.name_to_index
        tr_out, inf_out = d.output.name_to_index, m.output.name_to_index
        self.num_training_input_vars, self.num_inference_input_vars = len(tr_in), len(inf_in)
        self.num_training_output_vars, self.num_inference_output_vars = len(tr_out), len(inf_out)
        self.remappers, self.backmappers, self.remapper_kwargs = [], [], []
        self.index_training_input, self.index_training_out = [], []
        self.index_inference_input, self.index_inference_output = [], []
        method_of, kwargs = self.methods, self.method_kwargs
        for name in tr_in:
            method = method_of.get(name, self.default)
            if method not in METHODS:
                raise KeyError(f"Unknown remapping method for {name}: {method}")
            self.remappers.append(method)
            self.backmappers.append(method)
            self.index_training_input.append(tr_in[name])
            self.index_training_out.append(tr_out.get(name))
            self.index_inference_input.append(inf_in.get(name))
            self.index_inference_output.append(inf_out.get(name))
            self.remapper_kwargs.append(dict(kwargs[method]) if method in kwargs else {})

    # ---------------------------------------------------------------------------------- the remap program
    def _index(self, width: int, inverse: bool) -> list:
        if inverse:
            tr, inf, lists = self.num_training_output_vars, self.num_inference_output_vars, (self.index_training_out, self.index_inference_output)
        else:
            tr, inf, lists = self.num_training_input_vars, self.num_inference_input_vars, (self.index_training_input, self.index_inference_input)
        if width == tr:
            return lists[0]
        if width == inf:
            return lists[1]
        raise ValueError(f"Input tensor ({width}) does not match the training ({tr}) or inference shape ({inf})")

    def entries(self, width: int, inverse: bool = False) -> list:
        """[(column, entry)] of one direction at one width, in the order of the variables; identities are left out."""
        out = []
        for col, method, kwargs in zip(self._index(width, inverse), self.remappers, self.remapper_kwargs):
            if col is None:
                continue
            entry = METHODS[method](inverse, **kwargs)
            if entry[0] != NONE:
                out.append((col, entry))
        return out

    def program(self, width: int, inverse: bool = False) -> list:
        """One entry per column of a tensor of ``width`` variables."""
        table = [_IDENTITY] * width
        for col, entry in self.entries(width, inverse):
            table[col] = entry
        return table

    def device_program(self, width: int, inverse: bool, device):
        """The program as device tables (``ops.RemapProgram``) with its violation counters, built once per (width, direction, device).
        The tables do not depend on the dtype: every step rounds in the kernel."""
        key = (width, bool(inverse), str(device))
        hit = self._device_cache.get(key)
        if hit is None:
            from .. import ops

            table = self.program(width, inverse)
            asserting = [c for c, e in enumerate(table) if e[0] == LOG or (e[0] in (POWER, BOXCOX) and not e[1] & CLIP)]
            counters = torch.zeros(width, dtype=torch.int32, device=device) if asserting else None
            hit = self._device_cache[key] = (ops.remap_program([device_entry(e) for e in table], device), counters, {c: table[c][0] for c in asserting})
        return hit

    def inverse_program(self, width: int) -> list:
        """``inverse_transform`` as ops of the output column program (``layers.bounding``: kind 16 + remap op), in the order of the variables."""
        from ..layers.bounding import REMAP_BASE

        return [(REMAP_BASE + e[0], col, 0, e[2], e[3], e[1], e[4]) for col, e in self.entries(width, inverse=True)]

    # ---------------------------------------------------------------------------------- reference API
    def _run(self, x: Tensor, in_place: bool, inverse: bool, check_domain: Optional[bool] = None) -> Tensor:
        width = x.shape[-1]
        index = self._index(width, inverse)  # (the width is checked before anything is cloned or built)
        del index
        if x.is_cuda:
            if x.dim() not in (4, 5) or x.stride(-1) != 1:
                raise NotImplementedError(f"{type(self).__name__}: on the GPU the tensor is [batch, time, (ensemble,) grid, vars] with contiguous "
                                          f"variables; got shape {tuple(x.shape)}, strides {x.stride()}")
            from .. import ops

            program, counters, asserting = self.device_program(width, inverse, x.device)
            check = counters is not None and (self.check_domain if check_domain is None else check_domain) and not torch.cuda.is_current_stream_capturing()
            if check:
                counters.zero_()
            y = ops.remap_columns(x, program, out=x if in_place else None, violations=counters if check else None)
            if check:
                for col, count in enumerate(counters.tolist()):
                    assert count == 0, ASSERTIONS[asserting[col]]
            return y
        if not in_place:
            x = x.clone()
        for col, entry in self.entries(width, inverse):
            x[..., col] = apply_entry_torch(x[..., col], entry, check=True)
        return x

    def transform(self, x: Tensor, in_place: bool = True, check_domain: Optional[bool] = None, **_kwargs) -> Tensor:
        return self._run(x, in_place, inverse=False, check_domain=check_domain)

    def inverse_transform(self, x: Tensor, in_place: bool = True, **_kwargs) -> Tensor:
        return self._run(x, in_place, inverse=True)
