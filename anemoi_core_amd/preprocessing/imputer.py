"""The imputers - mirrors of the reference's ``anemoi.models.preprocessing.imputer`` classes (BaseImputer, InputImputer,
ConstantImputer, CopyImputer), written from their behaviour: same constructor arguments (processor config, data indices, statistics),
same public attributes (``index_training_input``, ``index_inference_input``, ``index_training_output``, ``index_inference_output``,
``replacement``, ``nan_locations``, ``loss_mask_training`` and the four ``num_*_vars``), an empty state_dict.

``transform(x [batch, time, (ensemble,) grid, vars])`` replaces NaN in the configured variables - by a statistic (InputImputer), by a
constant (ConstantImputer), by another variable's value at the same position (CopyImputer) - and remembers where the first time step had
NaN; ``inverse_transform`` puts NaN back into the output variables there.  The NaN test is that of ensemble member 0 and applies to every
member (the reference's ``get_nans`` states the rule; its own boolean-mask assignment raises on more than one member, here the rule simply
holds); each time step has its own NaN locations.

CPU tensors take plain torch (``torch.where``: no boolean-mask assignment, so nothing goes through ``nonzero``); MI355X tensors take one HIP
kernel per call (``ops.impute_columns`` / ``ops.restore_nan_columns``) and never synchronise with the host, so a forward that contains an
imputer can be captured in a hipGraph.  Inside ``AnemoiModelEncProcDec.predict_step`` the chain [imputer, InputNormalizer] runs none of these
stand-alone kernels: ``device_program`` / ``inverse_program`` below feed the model-edge kernels, which also write the NaN mask; at most one
``index_select`` follows (the mask restricted to ``data.input.full``, when the width is the training width and a diagnostic variable exists),
and ``loss_mask_training`` is not built there."""
from __future__ import annotations

import logging
from typing import Optional

import torch
from torch import Tensor

from . import BasePreprocessor

LOGGER = logging.getLogger(__name__)

NONE, CONSTANT, COPY = 0, 1, 2  # the kinds of the imputation program (include/anemoi_hip.h)


def _as_mapping(statistics):
    """A plain dict from a dict or an omegaconf DictConfig (resolved), None as it is."""
    if statistics is None or isinstance(statistics, dict):
        return statistics
    try:
        from omegaconf import DictConfig, OmegaConf
    except ImportError:
        DictConfig = ()
    if DictConfig and isinstance(statistics, DictConfig):
        return OmegaConf.to_container(statistics, resolve=True)
    raise TypeError(f"Statistics {type(statistics)} is optional and not a dictionary")


class BaseImputer(BasePreprocessor):
    """Base of the imputers: the index bookkeeping, ``transform`` / ``inverse_transform`` and the imputation program."""

    supports_skip_imputation = True

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        # these masks describe the current batch (or the rank's shard of it)
        self.nan_locations: Optional[Tensor] = None
        self.loss_mask_training: Optional[Tensor] = None
        self._device_cache: dict = {}

    # ---------------------------------------------------------------------------------- indices
    def _replacement_for(self, name: str, method: str, statistics):
        """What ``replacement`` holds for a variable imputed by ``method``."""
        raise NotImplementedError

    def _create_imputation_indices(self, statistics=None) -> None:
        """One entry per imputed variable, in the order of the data-input variables: its column in the training input / output
        (all data variables) and in the inference input / output (the model's variables; None where the variable is absent)."""
        d, m = self.data_indices.data, self.data_indices.model
        tr_in, inf_in = d.input.name_to_index, m.input.name_to_index
        tr_out, inf_out = d.output.name_to_index, m.output.name_to_index
        self.num_training_input_vars, self.num_inference_input_vars = len(tr_in), len(inf_in)
        self.num_training_output_vars, self.num_inference_output_vars = len(tr_out), len(inf_out)
        self.index_training_input, self.index_inference_input = [], []
        self.index_training_output, self.index_inference_output = [], []
        self.replacement = []
        method_of = self.methods
        for name in tr_in:
            method = method_of.get(name, self.default)
            if method == "none":
                continue
            if inf_in.get(name) is None and method != self.default:
                LOGGER.warning("If placement of NaNs for diagnostic variables in inference output is desired, this needs to be handled by "
                               "postprocessors: %s", name)
            self.index_training_input.append(tr_in[name])
            self.index_training_output.append(tr_out.get(name))
            self.index_inference_input.append(inf_in.get(name))
            self.index_inference_output.append(inf_out.get(name))
            self.replacement.append(self._replacement_for(name, method, statistics))
            LOGGER.info("Imputer: replacing NaNs in %s with %s", name, self.replacement[-1])
        n = len(self.replacement)
        assert len(self.index_training_input) == len(self.index_inference_input) <= n, "Error creating imputation indices"
        assert len(self.index_training_output) == len(self.index_inference_output) <= n, "Error creating imputation indices"

    # ---------------------------------------------------------------------------------- the imputation program
    def _input_index(self, width: int) -> list:
        if width == self.num_training_input_vars:
            return self.index_training_input
        if width == self.num_inference_input_vars:
            return self.index_inference_input
        raise ValueError(f"Input tensor ({width}) does not match the training ({self.num_training_input_vars}) or inference shape "
                         f"({self.num_inference_input_vars})")

    def _entry(self, replacement, dtype) -> tuple:
        """(kind, value, source column) of one imputed column; the value is rounded ONCE, from what ``replacement`` holds to ``dtype``."""
        return CONSTANT, float(torch.tensor(float(replacement), dtype=torch.float64).to(dtype)), 0

    def program(self, width: int, dtype=torch.float32) -> tuple[list, list, list]:
        """Per column of an input of ``width`` variables: (kinds, values, source columns), kind 0 none / 1 constant / 2 copy."""
        kinds, values, sources = [NONE] * width, [0.0] * width, [0] * width
        for col, rep in zip(self._input_index(width), self.replacement):
            if col is not None:
                kinds[col], values[col], sources[col] = self._entry(rep, dtype)
        return kinds, values, sources

    def _cached(self, key, build):
        hit = self._device_cache.get(key)
        if hit is None:
            hit = self._device_cache[key] = build()
        return hit

    def device_program(self, width: int, dtype, device):
        """The program as device tables (``ops.ImputeProgram``), built once per (width, dtype, device)."""
        from .. import ops

        return self._cached(("program", width, dtype, str(device)), lambda: ops.impute_program(*self.program(width, dtype), device))

    def restore_pairs(self, width: int) -> list:
        """[(output column, mask column)] of ``inverse_transform`` for an output of ``width`` variables; the mask column is the imputed
        variable's column in the INFERENCE input, which is also its column in the training-width mask (restricted to data.input.full)."""
        if width == self.num_training_output_vars:
            index = self.index_training_output
        elif width == self.num_inference_output_vars:
            index = self.index_inference_output
        else:
            raise ValueError(f"Input tensor ({width}) does not match the training ({self.num_training_output_vars}) or inference shape "
                             f"({self.num_inference_output_vars})")
        return [(dst, src) for src, dst in zip(self.index_inference_input, index) if src is not None and dst is not None]

    def inverse_program(self, width: int) -> list:
        """``inverse_transform`` as ops of the output column program (kind 10: NaN where mask[n, src]), one per restored column."""
        return [(10, dst, src, 0.0, 0.0) for dst, src in self.restore_pairs(width)]

    # ---------------------------------------------------------------------------------- reference API
    def get_nans(self, x: Tensor) -> Tensor:
        """isnan of the first element of every dimension between time and grid: [batch, time, grid, vars]."""
        return torch.isnan(x[(slice(None), slice(None)) + (0,) * (x.ndim - 4)])

    def record_nan_locations(self, nan0: Tensor, width: int, loss_mask: bool = True) -> None:
        """Keep what the loss and ``inverse_transform`` need of nan0 [batch, grid, vars], the NaN locations of time step 0.
        ``loss_mask=False`` (the fused ``predict_step``, where nothing reads it): ``loss_mask_training`` is not built and left None even at
        the training width - a departure from ``transform``, which costs five launches and a [batch, grid, outputs] fp32 tensor there."""
        if width != self.num_training_input_vars:  # (the training width is tried first, as everywhere: the two may coincide)
            self.nan_locations, self.loss_mask_training = nan0, None
            return
        dev = nan0.device
        full = torch.as_tensor(self.data_indices.data.input.full).long().reshape(-1)
        if full.tolist() == list(range(width)):  # no diagnostic among the data variables: the restriction is the identity
            self.nan_locations = nan0
        else:
            self.nan_locations = nan0.index_select(-1, self._cached(("full", str(dev)), lambda: full.to(dev)))
        if not loss_mask:
            self.loss_mask_training = None
            return
        n_out = len(self.data_indices.model.output.name_to_index)
        pairs = [(s, d) for s, d in zip(self.index_training_input, self.index_inference_output) if s is not None and d is not None]
        src, dst = self._cached(("loss", str(dev)), lambda: tuple(torch.tensor(c, dtype=torch.long, device=dev) for c in zip(*pairs)) or (None, None))
        loss = torch.ones((nan0.shape[0], nan0.shape[1], n_out), device=dev)
        if src is not None:
            loss.index_copy_(-1, dst, (~nan0.index_select(-1, src)).to(loss.dtype))
        self.loss_mask_training = loss

    def _fill_torch(self, x: Tensor, index: list, nan: Tensor) -> Tensor:
        """In place on a host tensor: column by column, in the order of the imputed variables."""
        for col, rep in zip(index, self.replacement):
            if col is not None:
                mask = nan[..., col].reshape(nan.shape[:2] + (1,) * (x.ndim - 4) + nan.shape[2:3])
                kind, value, _ = self._entry(rep, x.dtype)
                x[..., col] = torch.where(mask, torch.full((), value, dtype=x.dtype), x[..., col])
        return x

    def transform(self, x: Tensor, in_place: bool = True, skip_imputation: bool = False, **_kwargs) -> Tensor:
        """x [batch, time, (ensemble,) grid, vars]: NaN of the configured variables replaced; ``nan_locations`` (and, at the training
        width, ``loss_mask_training``) describe time step 0 afterwards."""
        if skip_imputation:
            return x if in_place else x.clone()
        width = x.shape[-1]
        index = self._input_index(width)
        if x.is_cuda and x.dim() in (4, 5) and x.stride(-1) == 1:
            from .. import ops

            nan0 = torch.empty((x.shape[0], x.shape[-2], width), dtype=torch.bool, device=x.device)
            y = ops.impute_columns(x, self.device_program(width, x.dtype, x.device), out=x if in_place else None, mask=nan0)
            self.record_nan_locations(nan0, width)
            return y
        if x.is_cuda:
            raise NotImplementedError(f"{type(self).__name__}: on the GPU the input is [batch, time, (ensemble,) grid, vars] with contiguous "
                                      f"variables; got shape {tuple(x.shape)}, strides {x.stride()}")
        if not in_place:
            x = x.clone()
        nan = self.get_nans(x)
        self.record_nan_locations(nan[:, 0], width)
        return self._fill_torch(x, index, nan)

    def inverse_transform(self, x: Tensor, in_place: bool = True, skip_imputation: bool = False, **_kwargs) -> Tensor:
        """x [batch, ..., grid, vars]: NaN again in the imputed output variables where the input's first time step had it."""
        if skip_imputation:
            return x if in_place else x.clone()
        pairs = self.restore_pairs(x.shape[-1])
        if self.nan_locations is None:
            raise RuntimeError("Cannot inverse-transform before the corresponding input has been transformed.")
        assert x.shape[0] == self.nan_locations.shape[0], (
            f"Batch dimension of input tensor ({x.shape[0]}) does not match the batch dimension of nan locations ({self.nan_locations.shape[0]}). "
            "Are you using the postprocessors without running the preprocessor first?")
        if x.is_cuda:
            from .. import ops

            width, dev = x.shape[-1], x.device

            def build():
                src_of = torch.full((width,), -1, dtype=torch.int32)
                for dst, src in pairs:
                    src_of[dst] = src
                return src_of.to(dev)

            if not x.is_contiguous():
                raise NotImplementedError(f"{type(self).__name__}.inverse_transform: on the GPU the tensor must be contiguous")
            return ops.restore_nan_columns(x, self.nan_locations.contiguous(), self._cached(("restore", width, str(dev)), build),
                                           out=x if in_place else None)
        if not in_place:
            x = x.clone()
        nan = self.nan_locations.reshape(self.nan_locations.shape[:1] + (1,) * (x.ndim - 3) + self.nan_locations.shape[1:])
        for dst, src in pairs:
            x[..., dst] = torch.where(nan[..., src], torch.full((), float("nan"), dtype=x.dtype), x[..., dst])
        return x


class InputImputer(BaseImputer):
    """Replaces NaN by a statistic of the variable: the config's methods name entries of ``statistics`` (``mean: [x, y]``), and the
    replacement of a variable is ``statistics[method][its data-input index]``."""

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self._create_imputation_indices(_as_mapping(statistics))

    def _replacement_for(self, name, method, statistics):
        if statistics is None:
            return method
        assert method in statistics, f"{method} is not a method in the statistics metadata"
        return statistics[method][self.data_indices.data.input.name_to_index[name]]


def _number(key):
    """The constant a configuration key stands for: mapping keys reach the processor as text (``ProcessorSpec``)."""
    if not isinstance(key, str):
        return key
    try:
        return int(key)
    except ValueError:
        return float(key)


class ConstantImputer(BaseImputer):
    """Replaces NaN by a constant: the config's method keys ARE the values (``3.14: [x, y]``)."""

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self._create_imputation_indices()

    def _replacement_for(self, name, method, statistics):
        return _number(method)


class CopyImputer(BaseImputer):
    """Replaces NaN by the value of another variable at the same (batch, time, member, grid) position: the config's method keys name the
    variable to copy from (``variable_to_copy: [variable_missing_1, variable_missing_2]``).

    A source that is itself imputed by the same imputer (a chain ``a <- b <- c``) is filled sequentially on host tensors, as the reference
    does; on the GPU such a configuration raises ``NotImplementedError`` (``ops.impute_program``): the kernels read their sources raw.

    The source column is looked up in ``data_indices.data.input.name_to_index`` for EVERY input width, as the reference does and as the
    recorded outputs show: at the inference width, where the diagnostic variables are absent, that column belongs to whichever variable
    stands there in the model's order (and a column past the width raises IndexError, as the reference's indexing does).  On host tensors
    a NaN in the copied value trips the reference's assertion; on the GPU nothing synchronises - a NaN source propagates, and the one-off
    ``Processors.check_first_batch`` catches it on the first batch."""

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self._create_imputation_indices()

    def _replacement_for(self, name, method, statistics):
        return method

    def _entry(self, replacement, dtype) -> tuple:
        return COPY, 0.0, self.data_indices.data.input.name_to_index[replacement]

    def program(self, width: int, dtype=torch.float32) -> tuple[list, list, list]:
        kinds, values, sources = super().program(width, dtype)
        for col, kind in enumerate(kinds):
            if kind == COPY and sources[col] >= width:
                raise IndexError(f"index {sources[col]} is out of bounds for dimension {-1} with size {width}")
        return kinds, values, sources

    def _fill_torch(self, x: Tensor, index: list, nan: Tensor) -> Tensor:
        for col, rep in zip(index, self.replacement):
            if col is not None:
                mask = nan[..., col].reshape(nan.shape[:2] + (1,) * (x.ndim - 4) + nan.shape[2:3])
                source = x[..., self.data_indices.data.input.name_to_index[rep]]
                assert not bool((torch.isnan(source) & mask).any()), f"NaNs found in variable {rep} to be copied."
                x[..., col] = torch.where(mask, source, x[..., col])
        return x
