"""Plain-torch CPU restatements of the imputer kernels (csrc/rowwise.hip: impute_columns, restore_nan_columns,
assemble_input_impute[_vec8], assemble_output_impute, bound_columns_mask), beside tests/model_edge_refs.py and built on it.  Nothing here
imports ``anemoi_core_amd.ops``: tests/test_imputer_cpu.py holds THESE functions to the reference's recorded outputs
(tests/golden/imputer.pt), tests/test_imputer_kernels_gpu.py holds the kernels to them.

An imputation program is (kinds, values, sources), one entry per input column: kind 0 none, 1 constant (the value already rounded to the
data dtype), 2 copy from column ``source`` at the same position (reference preprocessing/imputer.py)."""
import torch

from tests.model_edge_refs import assemble_input_ref, assemble_output_ref, bounding_ref


def impute_ref(x, program):
    """x [batch, time, (ensemble,) grid, V] -> (imputed copy, bool [batch, grid, V]: isnan of time step 0, member 0, every column).  The
    NaN test of an element is isnan of ensemble member 0 at the same (batch, time, grid, column), applied to every member; copy sources
    are read from x as given (a program never copies from an imputed column)."""
    kinds, values, sources = program
    x5 = x.unsqueeze(2) if x.dim() == 4 else x
    nan = x5[:, :, :1].isnan()
    y = x5.clone()
    for c, (kind, value, src) in enumerate(zip(kinds, values, sources)):
        if kind == 1:
            y[..., c] = torch.where(nan[..., c], torch.full((), value, dtype=x.dtype), x5[..., c])
        elif kind == 2:
            y[..., c] = torch.where(nan[..., c], x5[..., src], x5[..., c])
    return y.reshape(x.shape), nan[:, 0, 0].clone()


def restore_nan_ref(x, mask, pairs):
    """x [batch, ..., grid, V_out], mask bool [batch, grid, V_mask], pairs [(output column, mask column)] -> NaN where the mask is set."""
    y = x.clone()
    m = mask.reshape(mask.shape[:1] + (1,) * (x.dim() - 3) + mask.shape[1:])
    for dst, src in pairs:
        y[..., dst] = torch.where(m[..., src], torch.full((), float("nan"), dtype=x.dtype), x[..., dst])
    return y


def assemble_input_impute_ref(x, attrs, width, program, mul=None, add=None, out_dtype=None):
    """x [T, N, V]: each step imputed by its own NaN test, then assemble_input_ref; also the mask of step 0, bool [N, V]."""
    y, mask = impute_ref(x.unsqueeze(0), program)
    return assemble_input_ref(y[0], attrs, width, mul, add, out_dtype), mask[0]


def assemble_output_impute_ref(x_out, x_skip, col_map, program, mul=None, add=None):
    """assemble_output_ref on the imputed skip [N, V_in] (one step: its own NaN test)."""
    return assemble_output_ref(x_out, impute_ref(x_skip[None, None], program)[0][0, 0], col_map, mul, add)


def bounding_mask_ref(x, program, mask):
    """bounding_ref for a program whose ops of kind 10, (10, dst, mask column, 0, 0), follow all others: the finite part and its bound
    from bounding_ref, then NaN (bound 0) where mask[n, src]; x [..., V], mask bool [..., V_mask]."""
    first = next((i for i, op in enumerate(program) if op[0] == 10), len(program))
    assert all(op[0] == 10 for op in program[first:]), "ops of kind 10 come last"
    if first:
        want, bound = bounding_ref(x, program[:first])
    else:
        want, bound = x.double(), torch.zeros(x.shape, dtype=torch.float64)
    want, bound = want.clone(), bound.clone()
    for _, dst, src, _, _ in program[first:]:
        want[..., dst] = torch.where(mask[..., src], torch.full((), float("nan"), dtype=torch.float64), want[..., dst])
        bound[..., dst] = torch.where(mask[..., src], torch.zeros((), dtype=torch.float64), bound[..., dst])
    return want, bound
