"""The post-processors - mirrors of the reference's ``anemoi.models.preprocessing.postprocessor`` classes (Postprocessor,
NormalizedReluPostprocessor, ConditionalZeroPostprocessor, ConditionalNaNPostprocessor), written from their behaviour: same constructor
arguments, same public attributes (``index_training_output``, ``index_inference_output``, ``postprocessorfunctions``, the two
``num_*_output_vars`` and, on the conditional ones, ``masking_variable`` / ``masking_variable_training_output`` /
``masking_variable_inference_output``), an empty state_dict.

``transform`` is the identity; ``inverse_transform(x [..., vars])`` clamps output variables (relu, hardtanh, a relu above a normalised
threshold) or fills them where a masking variable is zero / NaN.  Each class describes itself as ops of the ordered output column program
(``layers.bounding``): kinds 1 / 5 / 3 for the clamps, 11 / 12 for the conditional fills.  The reference takes the mask ONCE, before any
fill; the program reads the masking column as the ops before left it, so a fill of the masking variable itself is ordered after the fills
it masks.  CPU tensors evaluate the program with plain torch; MI355X tensors take one in-place launch (``ops.bound_columns_`` for the clamps,
``ops.column_program_`` for the fills).

One deviation: a conditional post-processor whose masking variable is not an output variable raises ``ValueError`` when it is built; the
reference indexes its tensor with ``None`` there, which adds a dimension and fills by accident."""
from __future__ import annotations

import logging
from typing import Optional

import torch
from torch import Tensor

from . import BasePreprocessor
from .imputer import _as_mapping, _number

LOGGER = logging.getLogger(__name__)

RELU, NORM_RELU, HARDTANH, FILL_WHERE_ZERO, NAN_WHERE_NAN = 1, 3, 5, 11, 12  # kinds of the output column program (layers/bounding.py)


class _Clamp:
    """What ``postprocessorfunctions`` holds for a clamped variable: callable, and one op of the column program."""

    def __init__(self, kind: int, p0: float = 0.0, p1: float = 0.0) -> None:
        self.kind, self.p0, self.p1 = kind, float(p0), float(p1)

    @property
    def threshold(self) -> float:
        return self.p0

    def __call__(self, v: Tensor) -> Tensor:
        if self.kind == RELU:
            return torch.relu(v)
        if self.kind == HARDTANH:
            return torch.nn.functional.hardtanh(v, self.p0, self.p1)
        return torch.relu(v - self.p0) + self.p0


class Postprocessor(BasePreprocessor):
    """relu / hardtanh (-1, 1) / hardtanh_0_1 on output variables; ``none`` variables are skipped."""

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self._device_cache: dict = {}
        self._prepare_postprocessing_indices_list()
        self._create_postprocessing_indices()
        assert len(self.index_training_output) == len(self.index_inference_output) <= len(self.postprocessorfunctions), (
            f"Error creating postprocessing indices {len(self.index_training_output)}, {len(self.index_inference_output)}, "
            f"{len(self.postprocessorfunctions)}")

    def _prepare_postprocessing_indices_list(self) -> None:
        self.num_training_output_vars = len(self.data_indices.data.output.name_to_index)
        self.num_inference_output_vars = len(self.data_indices.model.output.name_to_index)
        self.index_training_output, self.index_inference_output, self.postprocessorfunctions = [], [], []

    def _create_postprocessing_indices(self) -> None:
        tr_out, inf_out = self.data_indices.data.output.name_to_index, self.data_indices.model.output.name_to_index
        method_of = self.methods
        for name in tr_out:
            method = method_of.get(name, self.default)
            if method == "none":
                continue
            assert name in inf_out, (f"Postprocessor: {name} not found in inference output indices. "
                                     f"Postprocessors cannot be applied to forcing variables.")
            self.index_training_output.append(tr_out.get(name))
            self.index_inference_output.append(inf_out.get(name))
            self.postprocessorfunctions.append(self._get_postprocessor_function(method, name))

    def _get_postprocessor_function(self, method, name):
        if method == "relu":
            return _Clamp(RELU)
        if method == "hardtanh":
            return _Clamp(HARDTANH, -1, 1)
        if method == "hardtanh_0_1":
            return _Clamp(HARDTANH, 0, 1)
        raise ValueError(f"Unknown postprocessing method: {method}")

    # ---------------------------------------------------------------------------------- the column program
    _width_error = "Input"

    def _index(self, width: int) -> list:
        if width == self.num_training_output_vars:
            return self.index_training_output
        if width == self.num_inference_output_vars:
            return self.index_inference_output
        raise ValueError(f"{self._width_error} tensor ({width}) does not match the training ({self.num_training_output_vars}) or inference shape "
                         f"({self.num_inference_output_vars})")

    def inverse_program(self, width: int) -> list:
        """``inverse_transform`` as ops (kind, column, total column, p0, p1) of the output column program, in application order."""
        return [(f.kind, col, 0, f.p0, f.p1) for f, col in zip(self.postprocessorfunctions, self._index(width)) if col is not None]

    def _apply_torch(self, x: Tensor, program: list) -> Tensor:
        """In place on a host tensor, op by op."""
        for kind, col, tot, p0, p1 in program:
            v = x[..., col]
            if kind == FILL_WHERE_ZERO:
                x[..., col] = torch.where(x[..., tot] == 0, torch.full((), p0, dtype=x.dtype), v)
            elif kind == NAN_WHERE_NAN:
                x[..., col] = torch.where(torch.isnan(x[..., tot]), torch.full((), float("nan"), dtype=x.dtype), v)
            else:
                x[..., col] = _Clamp(kind, p0, p1)(v)
        return x

    def inverse_transform(self, x: Tensor, in_place: bool = True, **_kwargs) -> Tensor:
        width = x.shape[-1]
        program = self.inverse_program(width)
        if not in_place:
            x = x.clone()
        if not x.is_cuda:
            return self._apply_torch(x, program)
        if not x.is_contiguous():  # (a permuted output of several steps: the program runs on a contiguous copy)
            return x.copy_(self.inverse_transform(x.contiguous(), in_place=True))
        from .. import ops
        from ..layers.bounding import extended_program_tables

        key = (width, str(x.device))
        tables = self._device_cache.get(key)
        if tables is None:
            tables = self._device_cache[key] = extended_program_tables(program, width, x.device)
        if not program:
            return x
        if any(op[0] > 10 for op in program):
            return ops.column_program_(x, *tables)
        return ops.bound_columns_(x, *tables)


class NormalizedReluPostprocessor(Postprocessor):
    """relu above a threshold: the config's method keys ARE the thresholds in physical units (``271.15: [x1]``), normalised with the
    statistics at the variable's data-input index as ``normalizer`` says; the op is relu(x - t) + t."""

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        self.statistics = _as_mapping(statistics)
        super().__init__(config, data_indices, statistics)
        if self.normalizer not in {"none", "mean-std", "min-max", "max", "std"}:
            raise ValueError("Normalizer must be one of: 'none', 'mean-std', 'min-max', 'max', 'std' in NormalizedReluBounding.")

    def _get_postprocessor_function(self, method, name):
        value, s = _number(method), self.statistics
        i = self.data_indices.data.input.name_to_index[name]
        if self.normalizer == "mean-std":
            value = (value - s["mean"][i]) / s["stdev"][i]
        elif self.normalizer == "min-max":
            value = (value - s["minimum"][i]) / (s["maximum"][i] - s["minimum"][i])
        elif self.normalizer == "max":
            value = value / s["maximum"][i]
        elif self.normalizer == "std":
            value = value / s["stdev"][i]
        return _Clamp(NORM_RELU, float(value))


class ConditionalPostprocessor(Postprocessor):
    """Base of the fills that depend on another output variable: ``remap`` names the masking variable, the config's method keys are the
    fill values."""

    kind = 0
    _width_error = "Output"

    def _prepare_postprocessing_indices_list(self) -> None:
        super()._prepare_postprocessing_indices_list()
        self.masking_variable = self.remap if isinstance(self.remap, str) else None
        self.masking_variable_training_output = self.data_indices.data.output.name_to_index.get(self.masking_variable, None)
        self.masking_variable_inference_output = self.data_indices.model.output.name_to_index.get(self.masking_variable, None)
        if self.masking_variable_training_output is None or self.masking_variable_inference_output is None:
            raise ValueError(f"{type(self).__name__}: the masking variable {self.masking_variable!r} is not an output variable")

    def inverse_program(self, width: int) -> list:
        index = self._index(width)
        mask = self.masking_variable_training_output if index is self.index_training_output else self.masking_variable_inference_output
        fills = [(self.kind, col, mask, float(value), 0.0) for value, col in zip(self.postprocessorfunctions, index) if col is not None]
        return [f for f in fills if f[1] != mask] + [f for f in fills if f[1] == mask]  # the mask is taken before any fill


class ConditionalZeroPostprocessor(ConditionalPostprocessor):
    """Sets variables to their configured value where the masking variable is zero (``0: [y]``, ``5.0: [x]`` with ``remap: x``)."""

    kind = FILL_WHERE_ZERO

    def _get_postprocessor_function(self, method, name):
        return _number(method)


class ConditionalNaNPostprocessor(ConditionalPostprocessor):
    """Sets variables to NaN where the masking variable is NaN (``nan: [y]`` with ``remap: x``)."""

    kind = NAN_WHERE_NAN

    def _get_postprocessor_function(self, method, name):
        return torch.nan
