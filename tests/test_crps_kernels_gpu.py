"""The ensemble CRPS kernels (csrc/crps.hip) through ops.kernel_crps and losses.CRPS, against the reference's `stable` all-pairs formula and
its reduction restated below, in float64 on the CPU with autograd for the gradient.

Loss: the kernel gets 4 x the error the same restatement makes in fp32 on the CPU (a different summation order over up to B T N terms),
and never less than fp32 epsilon times the weighted magnitude reduce(w (sum_m |x_m| + |y|)), for inputs the fp32 run gets exactly.
Gradient: every element is upstream (1/B, 1/V) w_time w_grid w_var (+-1/E + coef integer), at most eight fp32 roundings:
8 2^-24 |upstream| scale w (1/E + |coef| (E - 1)) absolute, plus 2^-8 relative for a bf16 result; exactly 0 where the reference's is.
A tile is 1024 consecutive (n, v) elements; the vector width is the largest of 4, 2, 1 dividing V."""
import pytest
import torch

from anemoi_core_amd import ops
from anemoi_core_amd.losses import CRPS

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def reduce(out, squash, mode):
    """[B, T, N, V] -> [V] or a scalar: variables squashed, time and grid summed, batch averaged."""
    if squash:
        out = out.mean(-1, keepdim=True) if mode == "avg" else out.sum(-1, keepdim=True)
    out = out.sum((1, 2)).mean(0)
    return out.squeeze(-1) if squash else out


def stable_crps(x, y, alpha, ignore_nans=False):
    """x [B, T, E, N, V], y [B, T, 1, N, V] -> the all-pairs almost-fair CRPS [B, T, N, V]."""
    if ignore_nans:
        bad = torch.isnan(x).any(2, keepdim=True) | torch.isnan(y)
        x, y = x.masked_fill(bad, 0.0), y.masked_fill(bad, 0.0)
    E = x.shape[2]
    xe, err = x.movedim(2, -1), (x - y).abs().movedim(2, -1)  # [B, T, N, V, E]
    var = (xe.unsqueeze(-1) - xe.unsqueeze(-2)).abs()
    mem = err.unsqueeze(-2) * ~torch.eye(E, dtype=torch.bool)
    return (mem + mem.transpose(-1, -2) - (1 - (1 - alpha) / E) * var).sum((-1, -2)) / (2 * E * (E - 1))


# E, V, N, (B, T), alpha, pred dtype, target dtype, (squash, mode), pred a slice along time
CASES = [
    (2, 1, 1, (1, 1), 0.95, F32, F32, (True, "avg"), False),
    (3, 3, 341, (2, 3), 0.0, F32, F32, (False, "avg"), True),        # one short of a tile, strides
    (8, 5, 205, (1, 1), 1.0, BF16, BF16, (True, "sum"), False),      # V one above the widest vector, one past a tile
    (16, 1, 1025, (1, 1), 0.95, BF16, BF16, (True, "avg"), False),
    (16, 4, 257, (2, 3), 1.0, F32, F32, (False, "avg"), False),      # vectors of 4
    (8, 6, 171, (1, 1), 0.0, BF16, F32, (True, "avg"), False),       # vectors of 2, fp32 target beside a bf16 ensemble
    (3, 1, 1023, (1, 1), 1.0, BF16, BF16, (True, "sum"), False),
    (2, 3, 342, (2, 3), 0.95, BF16, BF16, (False, "avg"), False),
    (2, 257, 5, (1, 1), 1.0, F32, F32, (True, "avg"), False),        # a stage-one thread owns several variables
    (3, 1025, 1, (1, 1), 0.0, F32, F32, (False, "avg"), False),      # so does a stage-two thread
    (2, 4, 262400, (1, 1), 0.95, F32, F32, (True, "avg"), False),    # 1025 tiles: two per workgroup, the last workgroup with one
]


@pytest.mark.parametrize("E, V, N, BT, alpha, dtype, tdtype, squash, strided", CASES)
def test_loss_and_gradient_against_float64(E, V, N, BT, alpha, dtype, tdtype, squash, strided):
    (B, T), (sq, mode) = BT, squash
    g = torch.Generator().manual_seed(E * 1000 + V)
    whole = torch.randint(-2, 3, (B, T * (2 if strided else 1), E, N, V), generator=g).to(dtype)  # ties in most columns
    view = (lambda t: t[:, ::2]) if strided else (lambda t: t)
    x = view(whole)
    y = torch.randint(-2, 3, (B, T, 1, N, V), generator=g).to(tdtype)  # about every other target equals a member
    wg, wv, wt = (torch.rand(n, generator=g) + 0.5 for n in (N, V, T))
    wg = wg / N
    up = torch.rand(() if sq else (V,), generator=g) + 0.5
    w = (wt[:, None, None] * wg[:, None] * wv).double()

    def restated(real):
        xr = x.to(real).clone().requires_grad_()
        loss = reduce(stable_crps(xr, y.to(real), alpha) * w.to(real), sq, mode)
        (loss * up.to(real)).sum().backward()
        return loss.detach(), xr.grad

    want, want_grad = restated(torch.float64)
    own_error = (restated(torch.float32)[0].double() - want).abs()
    floor = reduce((x.double().abs().sum(2) + y.double().abs()[:, :, 0]) * w, sq, mode) * torch.finfo(F32).eps

    def run():
        xd = view(whole.cuda()).requires_grad_()
        assert xd.stride() == x.stride()
        loss = ops.kernel_crps(xd, y.cuda(), wg.cuda(), alpha=alpha, w_var=wv.cuda(), w_time=wt.cuda(), squash=sq, squash_mode=mode)
        (loss * up.cuda()).sum().backward()
        return loss.detach().cpu(), xd.grad.cpu()

    got, got_grad = run()
    again, again_grad = run()
    assert got.dtype == F32 and got.shape == want.shape and got_grad.dtype == dtype and got_grad.shape == x.shape
    assert torch.equal(got, again) and torch.equal(got_grad, again_grad)
    error, bound = (got.double() - want).abs(), torch.maximum(4 * own_error, floor)
    ratio = lambda e: float((e / bound.clamp_min(1e-300)).max())  # noqa: E731
    print(f"loss error / bound {ratio(error):.3f}, fp32 restatement's error / bound {ratio(own_error):.3f}")
    assert bool((error <= bound).all()), (error, bound)
    coef = alpha / (E * (E - 1)) + (1 - alpha) / E**2
    scale = up.double() / B / (V if sq and mode == "avg" else 1)
    bound = 8 * 2.0**-24 * scale * w * (1 / E + coef * (E - 1))  # [T, N, V]
    bound = bound[None, :, None] + (2.0**-8 * want_grad.abs() if dtype == BF16 else 0)
    error = (got_grad.double() - want_grad).abs()
    print(f"gradient error / bound {float((error / bound).max()):.3f}")
    assert bool((error <= bound).all())
    assert bool((got_grad[want_grad == 0] == 0).all()) and (N == 1 or bool((want_grad == 0).any()))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ignore_nans_through_the_loss_module(dtype):
    """Three columns: a NaN in the target, a NaN in one member, a clean one.  With the flag the first two count 0 and have gradient 0;
    without it the loss is NaN."""
    x = torch.tensor([[1.0, 2.0, 0.0], [2.0, float("nan"), 3.0], [4.0, -1.0, 3.0]], dtype=dtype).reshape(1, 1, 3, 3, 1)
    y = torch.tensor([float("nan"), 1.0, 2.0], dtype=dtype).reshape(1, 1, 1, 3, 1)
    wg = torch.tensor([0.25, 0.5, 1.0])
    xr = x.double().requires_grad_()
    want = reduce(stable_crps(xr, y.double(), 0.95, ignore_nans=True) * wg.double()[:, None], True, "avg")
    want.backward()
    losses = {flag: CRPS(ignore_nans=flag).cuda() for flag in (True, False)}
    for loss in losses.values():
        loss.add_scaler(3, wg.cuda())
    xd = x.cuda().requires_grad_()
    got = losses[True](xd, y.cuda())
    got.backward()
    torch.testing.assert_close(got.cpu().double(), want.detach(), rtol=4 * 2.0**-23, atol=0)
    bound = 8 * 2.0**-24 * wg.double() * (1 / 3 + 2 * (0.95 / 6 + 0.05 / 9)) + (2.0**-8 if dtype == BF16 else 0) * xr.grad.abs()[0, 0, :, :, 0]
    assert bool(((xd.grad.cpu().double() - xr.grad).abs()[0, 0, :, :, 0] <= bound).all())
    assert bool((xd.grad.cpu()[0, 0, :, :2, 0] == 0).all()) and bool((xd.grad.cpu()[0, 0, :, 2, 0] != 0).all())
    with torch.no_grad():
        assert bool(torch.isnan(losses[False](x.cuda(), y.cuda())))
