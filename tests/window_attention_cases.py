"""Cases, inputs and the float64 reference that tests/test_window_attention_cases_cpu.py (no GPU) and
tests/test_window_attention_edges_gpu.py share.  Nothing here touches a GPU.

Hot keys.  For an offset delta every query i of a sequence gets one dominant key at j = i + delta (where 0 <= j < N):
k[j, h, :] += c[h] * q[j - delta, h, :] / |q[j - delta, h, :]|, per head and per sequence, before the inputs are rounded to the test
dtype.  Query i sees the vector added to every other key as a random direction.  As i runs over 64 consecutive rows the hot key passes
every lane, every 16-row wave boundary and every position of a 64-key tile, so a kernel that loses ONE in-band key - a band edge off by
one, a tile skipped too early, a zero-filled row, a wrong MFMA k slot - loses, for some query, the key that carries most of the
softmax.  ``c`` sets the hot key's probability p_hot: ``tune_c`` finds, per head, the c at which the median p_hot over the affected
rows is the case's target (float64 scores with the case's softcap and ALiBi slope, bisection, rounded up to a multiple of 1/16 so that
the inputs do not depend on the last bits of a CPU's float64 sums).

The reference is the dense-mask restatement ``dense_reference``: one [H, N, N] score matrix per sequence, optionally with a set of
(i, j) pairs taken out of the band - the reference of a kernel that LOST those keys, which the CPU file uses to show that such a kernel
cannot pass."""
import dataclasses
import functools
import math
from typing import Optional

import torch

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
NAMES = ("out", "dq", "dk", "dv")


def alibi_slopes(num_heads: int) -> torch.Tensor:
    from tests.test_window_attention_gpu import alibi_slopes as slopes

    return slopes(num_heads)


# ------------------------------------------------------------------------------------------------------------------ the reference
def dense_reference(q, k, v, H, window, batch=1, softcap=None, slopes=None, exclude=None):
    """(out [rows, A], lse [rows, H]) in float64: softmax(q k^T / sqrt(d) [capped, - slope |i - j|], masked to |i - j| <= window) v per
    sequence of the batch, from one dense [H, N, N] score matrix.  ``exclude``: int64 [P, 2] pairs (i, j) of one sequence that are
    masked as well, in every sequence and head.  Differentiable in q, k, v."""
    q, k, v = (t.to(F64) for t in (q, k, v))
    rows, A = q.shape
    N, d = rows // batch, A // H
    w = N if window is None or window < 0 else window
    idx = torch.arange(N, device=q.device)
    dist = (idx[:, None] - idx[None, :]).abs()
    masked = dist > w
    if exclude is not None and len(exclude):
        masked = masked.clone()
        masked[exclude[:, 0], exclude[:, 1]] = True
    outs, lses = [], []
    for b in range(batch):
        qb, kb, vb = (t[b * N:(b + 1) * N].reshape(N, H, d).transpose(0, 1) for t in (q, k, v))  # [H, N, d]
        s = qb @ kb.transpose(1, 2) / math.sqrt(d)
        if softcap:
            s = softcap * torch.tanh(s / softcap)
        if slopes is not None:
            s = s - slopes.to(s)[:, None, None] * dist
        s = s.masked_fill(masked[None], float("-inf"))
        lses.append(torch.logsumexp(s, -1).transpose(0, 1))
        outs.append((torch.softmax(s, -1) @ vb).transpose(0, 1).reshape(N, A))
    return torch.cat(outs), torch.cat(lses)


def autograd_of(fn, q, k, v, do, dtype):
    """(out, dq, dk, dv) of ``fn(q, k, v) -> out`` on fresh leaves of ``dtype``."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    out = fn(*leaves)
    out.backward(do.to(dtype))
    return (out.detach(), *(t.grad for t in leaves))


def hot_pairs(N, delta):
    """The (query, key) pairs (i, i + delta) of one sequence, int64 [P, 2]."""
    i = torch.arange(max(0, -delta), min(N, N - delta))
    return torch.stack([i, i + delta], 1)


def all_rows(rows_of_one_sequence, N, batch):
    return torch.cat([rows_of_one_sequence + b * N for b in range(batch)])


# ------------------------------------------------------------------------------------------------------------------------ cases
# added to every case's seed.  The sensitivity condition of tests/test_window_attention_cases_cpu.py is about the WEAKEST of up to 400
# rows; of the offsets 0..11, 2 leaves the most room: every case's weakest row is at least 2.5x its bound, where 2x is required.
SEED = 2


@dataclasses.dataclass(frozen=True)
class Case:
    family: str
    window: Optional[int]
    delta: int
    d: int = 32
    dtype: torch.dtype = BF16
    N: int = 200
    p_target: float = 0.66
    p_range: tuple = (0.4, 0.7)
    softcap: Optional[float] = None
    alibi: bool = False
    H: int = 2
    batch: int = 2

    @property
    def id(self):
        extra = ("-cap" if self.softcap else "") + ("-alibi" if self.alibi else "")
        p = f"-p{self.p_target}" if self.family == "dominance" else ""
        return f"{self.family}-N{self.N}-w{self.window}-delta{self.delta}-d{self.d}-{NAME[self.dtype]}{extra}{p}"

    @property
    def seed(self):
        w = -1 if self.window is None else self.window
        return (SEED + w * 1009 + (self.delta + 500) * 31 + self.d + 7 * self.N + round(1e4 * self.p_target)) % (2**31)

    @property
    def boosted_d_out(self):
        """Whether d_out carries the hot value's direction (_add_hot_d_out): wherever dk is held to the 2x rule in every row."""
        return self.p_target < 0.95

    @property
    def weak_rows_allowed(self):
        """The tensors of this case for which the sensitivity condition (2x the bound in EVERY affected row) cannot hold, and is
        replaced by: at least 80 % of the affected rows at 2x the bound, and the median row at 4x.  12 (case, tensor) entries, all in
        the dominance ladder, whose p_hot the issue fixes:
          dk at p_hot 0.99 (bf16 only) and at p_hot 0.999 (bf16 and fp16): 10 entries;
          dq at p_hot 0.999, d = 32: 2 entries.
        dS of the hot pair is p (1 - p) (dP_hot - mean of the other dP).  A 16-bit evaluation rounds dP - Delta at eps |dP_hot|
        (eps = 2^-9 bf16, 2^-11 fp16) and the bound is twice eager torch's error, so a row of dk shows the lost pair only where
        (1 - p) |dP_hot - mean| is several eps |dP|: with 1 - p = 0.01 or 0.001 that fails in the rows whose dP_hot happens to lie
        near the mean (a normal variable within 0.15 of its median modulus of 0: about one row in ten), and the hot d_out direction
        does not help (it raises eps |dP_hot| as much as the signal; tried with G_HOT 4 and 16).  dq at d = 32 and p_hot 0.999 needs
        c = 13, i.e. a spread of c / sqrt(d) = 2.3 in the other keys' scores: in a few rows one of them takes over the softmax once
        the hot key is lost, and dq of a query with one dominant key is near 0 either way.  Every other tensor of these cases, and dq
        in the other ten, is held to the rule in every row."""
        if self.family != "dominance" or self.p_target < 0.95:
            return ()
        dk = self.dtype == BF16 or self.p_target > 0.995
        dq = self.d == 32 and self.p_target > 0.995
        return (("dq",) if dq else ()) + (("dk",) if dk else ())

    @property
    def slopes(self):
        return alibi_slopes(self.H) if self.alibi else None


N_LADDER = 200  # 3 * 64 + 8: the last workgroup has one partial wave and three waves past the end; sequence 2 starts at row 200
LADDER_W = [1, 15, 16, 17, 47, 48, 63, 64, 65, 100, 128]


def _deltas(w):
    return sorted({-w, -w + 1, -1, 0, 1, w - 1, w})


LADDER = [Case("ladder", w, dl) for w in LADDER_W for dl in _deltas(w)]
UNBOUNDED = [Case("unbounded", w, dl) for w in (None, N_LADDER + 3) for dl in (-(N_LADDER - 1), -64, -63, 63, 64, N_LADDER - 1)]
HEAD_DIMS = [Case("dims", w, s * w, d=d, dtype=dt, N=N) for d in (64, 128) for dt in (BF16, F16) for N in (200, 130) for w in (17, 64)
             for s in (-1, 1)]
FP32_ANCHORS = [Case("fp32", 64, dl, d=d, dtype=F32) for d, dl in ((32, 64), (64, -64), (128, 64))]
FANCY = [Case("fancy", 64, dl, d=d, softcap=cap, alibi=alibi) for d in (32, 128) for cap, alibi in ((30.0, False), (None, True), (30.0, True))
         for dl in (-64, 64)]
DOMINANCE_P = {0.58: (0.45, 0.65), 0.9: (0.85, 0.95), 0.99: (0.98, 0.995), 0.999: (0.998, 0.9995)}  # target: the range of the median
DOMINANCE = [Case("dominance", 64, dl, d=d, dtype=dt, p_target=p, p_range=r) for d, dt in ((32, BF16), (64, BF16), (128, F16))
             for p, r in DOMINANCE_P.items() for dl in (-64, 64)]
ALL_CASES = LADDER + UNBOUNDED + HEAD_DIMS + FP32_ANCHORS + FANCY + DOMINANCE

INDICATOR_KEYS = [0, 15, 16, 63, 64, 100, N_LADDER - 1]  # j* of the indicator values and i of the one-hot d_out


# ------------------------------------------------------------------------------------------------------------------------ inputs
K_SCALE = 0.5  # of the keys before the hot vectors are added: fewer rows in which an ordinary key competes with the hot one
G_HOT = 4.0


def _raw(case):
    g = torch.Generator().manual_seed(case.seed)
    q, k, v, do = (torch.randn(case.batch * case.N, case.H * case.d, generator=g, dtype=F64) for _ in range(4))
    # every q[i, h, :] scaled to the norm sqrt(d) (its expected norm; what the model's qk_norm does): the hot key's score is then
    # <q_i, k_j> / sqrt(d) + c in EVERY row, so that no row's hot key is weak because its query happens to be short
    q4 = q.view(-1, case.H, case.d)
    q = (q4 * (math.sqrt(case.d) / q4.norm(dim=-1, keepdim=True))).reshape(q.shape)
    return q, K_SCALE * k, v, do


def _add_hot(case, q, k, c):
    """k with c[h] q[j - delta, h] / |q[j - delta, h]| added to key j of every sequence."""
    N, H, d, dl = case.N, case.H, case.d, case.delta
    q4, k4 = q.view(case.batch, N, H, d), k.clone().view(case.batch, N, H, d)
    pairs = hot_pairs(N, dl)
    unit = q4[:, pairs[:, 0]] / q4[:, pairs[:, 0]].norm(dim=-1, keepdim=True)
    k4[:, pairs[:, 1]] += c.to(F64)[None, None, :, None] * unit
    return k4.view(case.batch * N, H * d)


def _add_hot_d_out(case, do, v):
    """d_out with G_HOT v[i + delta, h] / |v[i + delta, h]| added to query i: dP = <dO_i, v_j> of the hot pair is G_HOT |v_j| + N(0, d),
    four standard deviations from 0.  dS of the hot pair is p (1 - p) (dP_hot - mean of the other dP), so without this a row whose
    dP_hot happens to be near that mean has a hot pair that dk does not feel.  Not added where dk cannot feel the pair anyway
    (Case.boosted_d_out): there it would only raise eps |dP_hot|, the error every 16-bit dq carries, towards what a lost key
    does to dq."""
    if not case.boosted_d_out:
        return do
    N, H, d = case.N, case.H, case.d
    v4, g4 = v.view(case.batch, N, H, d), do.clone().view(case.batch, N, H, d)
    pairs = hot_pairs(N, case.delta)
    g4[:, pairs[:, 0]] += G_HOT * v4[:, pairs[:, 1]] / v4[:, pairs[:, 1]].norm(dim=-1, keepdim=True)
    return g4.view(case.batch * N, H * d)


def hot_probability(case, q, k):
    """p of the hot key of every affected query: float64 [batch * P, H] (rows ordered as all_rows(hot_pairs[:, 0]))."""
    N, H, d = case.N, case.H, case.d
    pairs = hot_pairs(N, case.delta)
    qi, kj = all_rows(pairs[:, 0], N, case.batch), all_rows(pairs[:, 1], N, case.batch)
    _, lse = dense_reference(q, k, torch.zeros_like(q), H, case.window, case.batch, case.softcap, case.slopes)
    s = (q.to(F64)[qi].view(-1, H, d) * k.to(F64)[kj].view(-1, H, d)).sum(-1) / math.sqrt(d)  # [batch * P, H]
    if case.softcap:
        s = case.softcap * torch.tanh(s / case.softcap)
    if case.alibi:
        s = s - case.slopes[None, :] * abs(case.delta)
    return torch.exp(s - lse[qi])


@functools.lru_cache(maxsize=None)
def tune_c(case):
    """c [H]: per head the smallest multiple of 1/16 at which the median p_hot of the affected rows reaches the case's target."""
    q, k, _, _ = _raw(case)
    lo, hi = torch.zeros(case.H, dtype=F64), torch.full((case.H,), 64.0, dtype=F64)
    for _ in range(12):  # 64 / 2^12 = 1/64
        mid = (lo + hi) / 2
        med = hot_probability(case, q, _add_hot(case, q, k, mid)).median(0).values
        lo, hi = torch.where(med < case.p_target, mid, lo), torch.where(med < case.p_target, hi, mid)
    return torch.ceil(hi * 16) / 16


@functools.lru_cache(maxsize=None)
def hot_inputs(case):
    """(q, k, v, d_out) on the CPU, rounded to the case's dtype, the hot keys in k and their v directions in d_out."""
    q, k, v, do = _raw(case)
    k, do = _add_hot(case, q, k, tune_c(case)), _add_hot_d_out(case, do, v)
    return tuple(t.to(case.dtype) for t in (q, k, v, do))


def indicator_values(N, A, keys, dtype):
    """v [len(keys) * N, A]: zeros except v[j*] = 1 for the one key j* = keys[b] of sequence b (None: that sequence is all zeros).
    Then out[i, h, :] = p[i, j*, h]: non-zero exactly for |i - j*| <= w, an exact 0 elsewhere."""
    v = torch.zeros(len(keys) * N, A, dtype=dtype)
    for b, j in enumerate(keys):
        if j is not None:
            v[b * N + j] = 1
    return v


# ------------------------------------------------------------------------------------------------------------------------ bounds
def forward_bound(want, dtype):
    """The max-error bound of tests/test_window_attention_gpu.py for ``out`` and for ``lse`` (the same rule)."""
    return (1e-5 if dtype == F32 else 2e-2) * max(1.0, float(want.abs().max()))


def backward_bound(want, eager, dtype):
    """The bound of tests/test_window_attention_backward_gpu.py for one of out / dq / dk / dv: 2 * e_eager, fp32 2e-5 max|want| + 1e-6."""
    if dtype == F32:
        return 2e-5 * float(want.abs().max()) + 1e-6
    return 2 * float((eager.double() - want).abs().max())
