"""Plain-torch restatements of the remapper's maps and of the post-processors, from the table of their documented behaviour: one function
per direction, keyed by the method's name, taking the column and the method's keyword arguments.  Every step is one torch op in the column's
dtype (so a 16-bit dtype rounds after every step) and leaves NaN where it was.  Shared by the CPU tests (against the recorded reference
outputs) and the GPU tests (evaluated on the device, in the kernel's dtype, and in float64)."""
import math

import torch


def _domain(v, clip_negative, message):
    if clip_negative:
        return torch.clamp(v, min=0.0)
    assert bool(v.ge(0.0).all()), message
    return v


POWER_MESSAGE = "Power transform input x must satisfy x >= 0, or use with clip_negative=True to clip negative values to 0."
BOXCOX_MESSAGE = "input x must me greater or equal to 0, or use with clip_negative=True to clip negative values to 0"
LOG_MESSAGE = "input x must be strictly positive for parameter lambd == 0"


def power(v, lambd=0.33, clip_negative=False, tangent_linear_above_one=False, check=True):
    v = _domain(v, clip_negative, POWER_MESSAGE) if check or clip_negative else v
    pw = torch.pow(v, lambd)
    return torch.where(pw > 1.0, v.mul(lambd).add(1.0 - lambd), pw) if tangent_linear_above_one else pw


def power_inverse(v, lambd=0.33, clip_negative=False, tangent_linear_above_one=False):
    pw = torch.pow(torch.clamp(v, min=0.0), 1 / lambd)
    return torch.where(pw > 1.0, v.sub(1.0 - lambd).div(lambd), pw) if tangent_linear_above_one else pw


def boxcox(v, lambd=0.5, clip_negative=False, check=True):
    if lambd == 0:
        assert not check or bool(v.gt(0.0).all()), LOG_MESSAGE
        return torch.log(v)
    v = _domain(v, clip_negative, BOXCOX_MESSAGE) if check or clip_negative else v
    return torch.pow(v, lambd).sub(1.0).div(lambd)


def boxcox_inverse(v, lambd=0.5, clip_negative=None):
    if lambd == 0:
        return torch.exp(v)
    return torch.pow(torch.clamp(v.mul(lambd).add(1.0), min=0.0), 1 / lambd)


def atanh(v, rho=2.0):
    if rho == 0:
        return v
    if rho < 0:
        raise ValueError(f"rho must satisfy 0 < rho , got {rho}")
    return torch.atanh(v.mul(2.0).sub(1.0).mul(math.tanh(rho))).div(rho)


def atanh_inverse(v, rho=2.0):
    if rho == 0:
        return torch.clamp(v, 0.0, 1.0)
    return torch.clamp(torch.tanh(v.mul(rho)).div(math.tanh(rho)).add(1.0).mul(0.5), min=0.0, max=1.0)


def displace(v, lower_atom=None, upper_atom=None, lower_target=None, upper_target=None, eps=0.0):
    if lower_atom is not None:
        v = torch.where(v <= lower_atom + eps, torch.full((), lower_target, dtype=v.dtype, device=v.device), v)
    if upper_atom is not None:
        v = torch.where(v >= upper_atom - eps, torch.full((), upper_target, dtype=v.dtype, device=v.device), v)
    return v


FORWARD = {
    "none": lambda v: v,
    "log1p": torch.log1p,
    "sqrt": lambda v, check=True: power(v, lambd=0.5, check=check),
    "power": power,
    "boxcox": boxcox,
    "atanh": atanh,
    "asinh": lambda v, c=1.0: torch.asinh(v.mul(c)),
    "displace_boundary_atoms": displace,
    "affine": lambda v, scale=1.0, shift=0.0: v.mul(scale).add(shift),
}
INVERSE = {
    "none": lambda v: v,
    "log1p": torch.expm1,
    "sqrt": lambda v: power_inverse(v, lambd=0.5),
    "power": power_inverse,
    "boxcox": boxcox_inverse,
    "atanh": atanh_inverse,
    "asinh": lambda v, c=1.0: torch.sinh(v).div(c),
    "displace_boundary_atoms": lambda v, lower_atom=None, upper_atom=None, lower_target=None, upper_target=None, eps=None: torch.clamp(v, lower_atom, upper_atom),
    "affine": lambda v, scale=1.0, shift=0.0: v.sub(shift).div(scale),
}
EXACT = ("none", "affine", "displace_boundary_atoms", "sqrt")  # exactly rounded in both directions: the kernels must be bit-equal to eager torch


def remap(x, columns, inverse=False, **extra):
    """x [..., V] with ``columns`` = {column: (method, kwargs)}: a new tensor with those columns mapped."""
    y = x.clone()
    table = INVERSE if inverse else FORWARD
    for col, (method, kwargs) in columns.items():
        y[..., col] = table[method](x[..., col], **kwargs, **extra)
    return y


def columns_of(config, name_to_column):
    """{column: (method, kwargs)} of a remapper configuration over the variables present in ``name_to_column``."""
    kwargs = config.get("method_kwargs", {})
    out = {}
    listed = {}
    for method, names in config.items():
        if method not in ("default", "method_kwargs", "remap", "normalizer"):
            listed.update(dict.fromkeys(names, str(method)))
    for name, col in name_to_column.items():
        method = listed.get(name, config.get("default", "none"))
        if method != "none":
            out[col] = (method, dict(kwargs.get(method, {})))
    return out


# ---- post-processors: ops (what, column, masking column, value) on x [..., V]
def relu_above(v, t):
    return torch.relu(v - t) + t


def conditional_fill(x, fills, mask_col, where):
    """fills = [(column, value)]; the mask is taken ONCE from the untouched masking column."""
    mask = torch.isnan(x[..., mask_col]) if where == "nan" else x[..., mask_col] == 0
    y = x.clone()
    for col, value in fills:
        y[..., col] = torch.where(mask, torch.full((), value, dtype=x.dtype, device=x.device), x[..., col])
    return y


def same(a, b):
    """Bit-equality with NaN at the same places (every NaN counts as the same value)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))
