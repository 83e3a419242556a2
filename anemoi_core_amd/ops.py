"""Tensor-level entry points of the MI355X kernels (thin wrappers over the C ABI, include/anemoi_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every function checks its
arguments, allocates the output with torch, and enqueues one kernel through ctypes.  All tensors must live
on a ROCm device — there is no CPU / eager fallback (a CPU tensor raises).

The op-level mirror of the reference boundary is at the bottom:
``anemoi_amd::graph_transformer_attention`` and ``graph_transformer_attention_conv`` follow
``anemoi::graph_transformer_attention`` / ``graph_transformer_attention_conv``
(reference models/src/anemoi/models/triton/gt.py:390-428, 564-576).
"""
from __future__ import annotations

from dataclasses import dataclass
import functools
from typing import NamedTuple, Optional

import os

import torch
from torch import Tensor

from . import _ext, _lib

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def _dt(t: Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {t.dtype}; supported: float32, bfloat16, float16") from None


try:  # raw handle of torch's current stream without constructing a Stream object (host launch overhead matters at N > 1)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    _raw_stream = None


def _stream() -> int:
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts: Optional[Tensor]) -> None:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "anemoi_core_amd kernels run on an MI355X (ROCm) device only; got a tensor on "
                f"'{t.device}'. There is no CPU fallback in the product path."
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    # kernels are enqueued on the CURRENT device's current stream (_stream): tensors of another GPU would be launched on the
    # wrong device / stream.  Fail loudly instead (multi-GPU processes: torch.cuda.set_device / `with torch.cuda.device(d)`).
    if dev is not None and dev.index is not None and dev.index != torch.cuda.current_device():
        raise RuntimeError(f"tensors live on {dev} but the current device is cuda:{torch.cuda.current_device()}; make {dev} current "
                           "(torch.cuda.set_device or `with torch.cuda.device(...)`) before calling anemoi_core_amd ops")


def _rows(t: Optional[Tensor], name: str, dtype=None) -> tuple[int, int]:
    """(data_ptr, leading dimension) of a 2-D row-major view whose last dim is contiguous."""
    if t is None:
        return 0, 0
    shape, stride = t.shape, t.stride()
    if len(shape) != 2:
        raise ValueError(f"{name}: expected a 2-D tensor, got shape {tuple(shape)}")
    if shape[1] > 1 and stride[1] != 1:
        raise ValueError(f"{name}: last dimension must be contiguous (strides {stride})")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype} does not match {dtype}")
    ld = stride[0] if shape[0] > 1 else max(shape[1], stride[0])
    return t.data_ptr(), ld


def _vec(t: Optional[Tensor], name: str, n: int, dtype) -> int:
    if t is None:
        return 0
    if t.dim() != 1 or t.shape[0] != n or not t.is_contiguous() or t.dtype != dtype:
        raise ValueError(f"{name}: expected contiguous [{n}] {dtype}, got {tuple(t.shape)} {t.dtype}")
    return t.data_ptr()


# ------------------------------------------------------------------------------------------ static graph structure
@dataclass(frozen=True)
class CSC:
    """dst-sorted (CSC) adjacency of a static graph, int32, built once (the reference rebuilds it on every
    call: layers/block.py:779-785, triton/utils.py:25-70)."""

    row: Tensor  # [M] int32 source node of every edge, CSC order
    dst: Tensor  # [M] int32 destination node of every edge, CSC order
    colptr: Tensor  # [n_dst + 1] int32
    n_src: int
    n_dst: int
    perm: Optional[Tensor] = None  # original -> CSC edge order when the input was not dst-sorted
    order: Optional[Tensor] = None  # [n_dst] int32: the order the fused attention WORKS on the destinations (processing_order)

    @property
    def num_edges(self) -> int:
        return self.row.shape[0]


def build_csc(edge_index: Tensor, size: tuple[int, int], edges_are_dst_sorted: bool = True, check: bool = False) -> CSC:
    """edge_index [2, M] (src, dst) any integer dtype -> CSC.  Pure index bookkeeping (torch ops; works on any
    device so that the host logic is testable without a GPU)."""
    n_src, n_dst = int(size[0]), int(size[1])
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, M], got {tuple(edge_index.shape)}")
    if max(n_src, n_dst, edge_index.shape[1]) >= 2**31:
        raise ValueError("graph too large for int32 indices")
    src, dst = edge_index[0].long(), edge_index[1].long()
    perm = None
    if not edges_are_dst_sorted:
        perm = torch.sort(dst, stable=True)[1]  # sort_edge_index_by_dst (distributed/khop_edges.py:37-40)
        src, dst = src[perm], dst[perm]
    elif check and dst.numel() > 1 and not bool((dst[1:] >= dst[:-1]).all()):
        raise ValueError("edge_index is not sorted by destination node")
    colptr = torch.zeros(n_dst + 1, dtype=torch.long, device=edge_index.device)
    if dst.numel():
        colptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n_dst), 0)
    return CSC(row=src.to(torch.int32).contiguous(), dst=dst.to(torch.int32).contiguous(),
               colptr=colptr.to(torch.int32).contiguous(), n_src=n_src, n_dst=n_dst, perm=perm)


def processing_order(csc: CSC, slices: int = 8) -> Optional[Tensor]:
    """A permutation of the destinations of a SQUARE graph that keeps mesh neighbours together inside each of the `slices`
    contiguous index ranges the fused attention hands to the XCDs (csrc/gt_attention.hip): breadth-first order over the
    SHORT edges of the range's own sub-graph.  Why: the hidden mesh is sorted by latitude, so ~768 consecutive destinations are
    a whole latitude ring whose K|V neighbourhood (three rings, 2 KiB per row) overflows an XCD's 4 MiB L2 from res 6 on
    (measured 1.65x the compulsory traffic); consecutive BFS levels of a strip form compact patches instead.  "Short": an edge
    with an endpoint of minimal in-degree - in a multi-scale icosphere every finest-level edge touches a vertex that exists at
    the finest level only (in-degree 6), while the long coarse-level edges join high-degree vertices; in a graph of uniform
    degree every edge qualifies.  Host-side index work, once per static graph; None when there is nothing to gain (bipartite
    graphs, graphs whose K|V rows fit the L2s anyway)."""
    import numpy as np

    n = csc.n_dst
    if csc.n_src != n or n < int(os.environ.get("ANEMOI_ATTN_ORDER_MIN_NODES", "16384")) or csc.num_edges == 0:
        return None
    src = csc.row.cpu().numpy().astype(np.int64)
    dst = csc.dst.cpu().numpy().astype(np.int64)
    deg = np.bincount(dst, minlength=n)
    dmin = deg[deg > 0].min()
    keep = np.minimum(deg[src], deg[dst]) == dmin
    src, dst = src[keep], dst[keep]
    per = (n + slices - 1) // slices
    same = (src // per) == (dst // per)  # edges inside one XCD's range
    src, dst = src[same], dst[same]
    o = np.argsort(dst, kind="stable")
    src, dst = src[o], dst[o]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, dst + 1, 1)
    ptr = np.cumsum(ptr)
    seen = np.zeros(n, dtype=bool)
    out = []
    for x in range(slices):
        lo, hi = x * per, min(n, (x + 1) * per)
        nxt = lo
        while nxt < hi:
            if seen[nxt]:
                nxt += 1
                continue
            frontier = np.array([nxt], dtype=np.int64)
            seen[nxt] = True
            while frontier.size:
                out.append(frontier)
                starts, ends = ptr[frontier], ptr[frontier + 1]
                cnt = ends - starts
                if cnt.sum() == 0:
                    break
                idx = np.repeat(starts - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())
                cand = np.unique(src[idx])
                cand = cand[~seen[cand]]
                seen[cand] = True
                frontier = cand
    order = np.concatenate(out) if out else np.arange(n)
    assert order.size == n and np.array_equal(np.sort(order), np.arange(n)), "processing_order: not a permutation"
    return torch.from_numpy(order.astype(np.int32)).to(csc.row.device)


# ------------------------------------------------------------------------------------------ kernels
def gt_attention(q: Tensor, k: Tensor, v: Tensor, e: Optional[Tensor], csc: CSC, num_heads: int,
                 addend: Optional[Tensor] = None, return_lse: bool = False, dropout_p: float = 0.0, dropout_seed: int = 0):
    """out[d] = softmax-attention over in-edges (+ addend).  q/out/addend [n_dst, D]; k, v [n_src, D]; e [M, D].
    ``dropout_p`` > 0: dropout on the softmax weights (conv.py:145), mask = f(dropout_seed, edge, head) (``attention_dropout_mask``)."""
    _dev(q, k, v, e, addend, csc.row)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {dropout_p}")
    D = q.shape[1]
    if D % num_heads:
        raise ValueError(f"channels {D} not divisible by heads {num_heads}")
    if q.shape[0] != csc.n_dst or k.shape[0] != csc.n_src or v.shape[0] != csc.n_src:
        raise ValueError(f"node counts {q.shape[0]}/{k.shape[0]}/{v.shape[0]} do not match the graph ({csc.n_dst}, {csc.n_src})")
    if e is not None and e.shape[0] != csc.num_edges:
        raise ValueError(f"edge tensor has {e.shape[0]} rows, graph has {csc.num_edges} edges")
    out = torch.empty((csc.n_dst, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((csc.n_dst, num_heads), dtype=torch.float32, device=q.device) if return_lse else None
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, "q"), _rows(k, "k", q.dtype), _rows(v, "v", q.dtype)
    ep, lde = _rows(e, "e", q.dtype)
    ap, lda = _rows(addend, "addend", q.dtype)
    rc = _lib.load().anemoi_gt_attention_dropout_fwd(qp, ldq, kp, ldk, vp, ldv, ep, lde, csc.row.data_ptr(), csc.colptr.data_ptr(),
                                                     ap, lda, out.data_ptr(), D, lse.data_ptr() if return_lse else 0,
                                                     csc.n_dst, csc.n_src, num_heads, D // num_heads, float(dropout_p),
                                                     int(dropout_seed) & (2**64 - 1), _dt(q), _stream())
    _lib.check(rc, "gt_attention_fwd")
    return (out, lse) if return_lse else out


def attention_dropout_mask(num_edges: int, num_heads: int, dropout_p: float, dropout_seed: int, device) -> Tensor:
    """fp32 [M, H]: 0 where ``gt_attention(dropout_p, dropout_seed)`` drops the weight of (CSC edge, head), 1 / (1 - p) where it
    keeps it - the scale the kernels derive on the fly."""
    out = torch.empty((num_edges, num_heads), dtype=torch.float32, device=device)
    _dev(out)
    _lib.check(_lib.load().anemoi_attention_dropout_mask(out.data_ptr(), num_edges, num_heads, float(dropout_p), int(dropout_seed) & (2**64 - 1),
                                                         _stream()), "attention_dropout_mask")
    return out


def build_reverse_csr(csc: CSC) -> tuple[Tensor, Tensor, Tensor]:
    """(rowptr [n_src+1], edge_ids [M], edge_dst [M]) int32: the CSC edges grouped by SOURCE, as the backward pass walks
    them (reference triton/utils.py:25-70 returns the same triple next to the CSC).  Index bookkeeping, any device."""
    order = torch.sort(csc.row.long(), stable=True)[1]
    rowptr = torch.zeros(csc.n_src + 1, dtype=torch.long, device=csc.row.device)
    if csc.num_edges:
        rowptr[1:] = torch.cumsum(torch.bincount(csc.row.long(), minlength=csc.n_src), 0)
    return rowptr.to(torch.int32).contiguous(), order.to(torch.int32).contiguous(), csc.dst


def gt_attention_backward(d_out: Tensor, q: Tensor, k: Tensor, v: Tensor, e: Tensor, out: Tensor, lse: Tensor, csc: CSC,
                          reverse: tuple[Tensor, Tensor, Tensor], num_heads: int, grads_out=None, dropout_p: float = 0.0,
                          dropout_seed: int = 0):
    """Gradients (dq, dk, dv, de) of ``gt_attention`` with a materialised edge tensor.  All node/edge tensors [rows, D];
    ``out``/``lse`` are the forward's results; ``reverse`` = build_reverse_csr(csc).  ``grads_out`` = (dq, dk, dv): write
    the node gradients into these (row-strided) views, e.g. column slabs of one fused-projection gradient buffer."""
    rowptr, edge_ids, edge_dst = reverse
    _dev(d_out, q, k, v, e, out, lse, csc.row, rowptr, edge_ids, edge_dst)
    D = q.shape[1]
    if D % num_heads:
        raise ValueError(f"channels {D} not divisible by heads {num_heads}")
    M = csc.num_edges
    if q.shape[0] != csc.n_dst or k.shape[0] != csc.n_src or v.shape[0] != csc.n_src or e.shape[0] != M:
        raise ValueError("tensor row counts do not match the graph")
    if d_out.shape != q.shape or out.shape != q.shape or tuple(lse.shape) != (csc.n_dst, num_heads) or lse.dtype != torch.float32:
        raise ValueError("d_out/out must have q's shape and lse must be fp32 [n_dst, H]")
    if rowptr.shape[0] != csc.n_src + 1 or edge_ids.shape[0] != M or edge_dst.shape[0] != M:
        raise ValueError("reverse CSR does not match the graph")
    if grads_out is None:
        dq, dk, dv = torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty((csc.n_src, D), dtype=q.dtype, device=q.device), \
            torch.empty((csc.n_src, D), dtype=q.dtype, device=q.device)
    else:
        dq, dk, dv = grads_out
        if dq.shape != q.shape or dk.shape != k.shape or dv.shape != v.shape:
            raise ValueError("grads_out shapes must equal q, k, v")
    de = torch.empty((M, D), dtype=q.dtype, device=q.device)
    (dqp, lddq), (dkp, lddk), (dvp, lddv) = _rows(dq, "dq", q.dtype), _rows(dk, "dk", q.dtype), _rows(dv, "dv", q.dtype)
    ws = torch.empty((2, M, num_heads), dtype=torch.float32, device=q.device)
    (qp, ldq), (kp, ldk), (vp, ldv), (ep, lde) = _rows(q, "q"), _rows(k, "k", q.dtype), _rows(v, "v", q.dtype), _rows(e, "e", q.dtype)
    (op, ldo), (gp, ldg) = _rows(out, "out", q.dtype), _rows(d_out, "d_out", q.dtype)
    i32 = lambda t: t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()  # noqa: E731
    rowptr, edge_ids, edge_dst = i32(rowptr), i32(edge_ids), i32(edge_dst)
    rc = _lib.load().anemoi_gt_attention_dropout_bwd(
        qp, ldq, kp, ldk, vp, ldv, ep, lde, op, ldo, lse.contiguous().data_ptr(), gp, ldg, csc.row.data_ptr(), csc.colptr.data_ptr(),
        rowptr.data_ptr(), edge_ids.data_ptr(), edge_dst.data_ptr(), dqp, lddq, dkp, lddk, dvp, lddv,
        de.data_ptr(), D, ws[0].data_ptr(), ws[1].data_ptr(), csc.n_dst, csc.n_src, M, num_heads, D // num_heads, float(dropout_p),
        int(dropout_seed) & (2**64 - 1), _dt(q), _stream())
    _lib.check(rc, "gt_attention_bwd")
    return dq, dk, dv, de


ATTENTION_OPS = ("forward", "forward_fused_edge", "backward", "backward_fused_edge")  # which entry point: AttnOp of csrc/gt_attention_plan.h
ATTENTION_ROUTES = ("unsupported", "generic", "wave")                                  # AttnRoute


class AttentionPlan(NamedTuple):
    """What an edge-attention entry point launches for a shape: ``route`` (one of ATTENTION_ROUTES), the wave kernel's lane layout
    (``vec`` channels per lane, ``lph`` lanes per head), and the launch geometry; fields as in anemoi_gt_attention_plan_t."""
    route: str
    vec: int
    lph: int
    fe_pad: int
    kv_adjacent: bool
    lds_bytes: int
    grid_dst: int
    grid_src: int
    grid_wgrad: int


def gt_attention_plan(op: str, num_heads: int, C: int, *, fe_pad: int = 0, n_dst: int = 1, n_src: int = 1, dtype: torch.dtype = torch.bfloat16,
                      rows_aligned: bool = True, kv_adjacent: bool = False) -> AttentionPlan:
    """The kernel choice of ``gt_attention`` / ``gt_attention_fused_edge`` and their backwards (``op``: one of ATTENTION_OPS) for
    ``num_heads`` heads of ``C`` channels, under ANEMOI_ATTN_BLOCKS_PER_CU of this process.  Host-only: nothing is launched and no GPU
    is needed.  ``rows_aligned`` / ``kv_adjacent``: the two facts the entry points read off their operands (contiguous tensors are
    aligned; k | v adjacent is the fused projection buffer).  ``route == "unsupported"`` where the entry point refuses the shape."""
    out = _lib.AttentionPlan()
    rc = _lib.load().anemoi_gt_attention_plan(ATTENTION_OPS.index(op), num_heads, C, fe_pad, n_dst, n_src, int(rows_aligned), int(kv_adjacent),
                                              _DT[dtype], out)
    if rc != _lib.E_UNSUPPORTED:
        _lib.check(rc, "gt_attention_plan")
    f = {name: getattr(out, name) for name, _ in out._fields_}
    return AttentionPlan(**{**f, "route": ATTENTION_ROUTES[out.route], "kv_adjacent": bool(out.kv_adjacent)})


def fused_edge_backward_supported(D: int, num_heads: int, fe: int) -> bool:
    """Whether ``gt_attention_fused_edge_backward`` takes [*, D] rows of ``num_heads`` heads with ``fe`` edge attributes (contiguous
    operands): the plan's answer, the same function the entry point launches from."""
    if D <= 0 or num_heads <= 0 or D % num_heads:
        return False
    return gt_attention_plan("backward_fused_edge", num_heads, D // num_heads, fe_pad=edge_feature_pad(fe)).route == "wave"


def gt_attention_fused_edge_backward(d_out: Tensor, q: Tensor, k: Tensor, v: Tensor, edge_feat: Tensor, w_packed: Tensor, out: Tensor,
                                     lse: Tensor, csc: CSC, reverse: tuple[Tensor, Tensor, Tensor], num_heads: int, grads_out=None,
                                     need_feat_grad: bool = False, addend: Optional[Tensor] = None, d_addend: Optional[Tensor] = None):
    """Gradients of ``gt_attention_fused_edge``: (dq, dk, dv, d_w_packed fp32 [D, fe_pad], d_edge_feat fp32 [M, fe_pad] or
    None).  E and dE are never materialised.  ``out`` / ``lse``: the forward's results; ``addend``: the forward's addend if it
    had one (``out`` includes it); ``d_addend``: a [n_dst, D] view that receives the addend's gradient (= d_out)."""
    rowptr, edge_ids, edge_dst = reverse
    _dev(d_out, q, k, v, edge_feat, w_packed, out, lse, csc.row, rowptr, edge_ids, edge_dst)
    D = q.shape[1]
    M, fe_pad = csc.num_edges, w_packed.shape[1]
    if edge_feat.dtype != torch.float32 or tuple(edge_feat.shape) != (M, fe_pad) or not edge_feat.is_contiguous():
        raise ValueError(f"edge_feat must be contiguous fp32 [{M}, {fe_pad}]")
    if w_packed.dtype != torch.float32 or tuple(w_packed.shape) != (D, fe_pad) or not w_packed.is_contiguous():
        raise ValueError(f"w_packed must be contiguous fp32 [{D}, {fe_pad}]")
    if d_out.shape != q.shape or out.shape != q.shape or tuple(lse.shape) != (csc.n_dst, num_heads) or lse.dtype != torch.float32:
        raise ValueError("d_out/out must have q's shape and lse must be fp32 [n_dst, H]")
    dev = q.device
    if grads_out is None:
        dq = torch.empty_like(q, memory_format=torch.contiguous_format)
        dk, dv = torch.empty((csc.n_src, D), dtype=q.dtype, device=dev), torch.empty((csc.n_src, D), dtype=q.dtype, device=dev)
    else:
        dq, dk, dv = grads_out
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    lib = _lib.load()
    d_wp = f32(D, fe_pad)
    d_feat = f32(M, fe_pad) if need_feat_grad else None
    ws, sf = f32(2, max(M, 1), num_heads), f32(csc.n_dst, num_heads, 2, fe_pad)
    qg = f32(csc.n_dst, num_heads, 2, fe_pad) if need_feat_grad else None
    part = f32(int(lib.anemoi_gt_attention_fused_edge_bwd_partial_floats(num_heads, D // num_heads, fe_pad)))
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, "q"), _rows(k, "k", q.dtype), _rows(v, "v", q.dtype)
    (op, ldo), (gp, ldg) = _rows(out, "out", q.dtype), _rows(d_out, "d_out", q.dtype)
    (dqp, lddq), (dkp, lddk), (dvp, lddv) = _rows(dq, "dq", q.dtype), _rows(dk, "dk", q.dtype), _rows(dv, "dv", q.dtype)
    i32 = lambda t: t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()  # noqa: E731
    rowptr, edge_ids, edge_dst = i32(rowptr), i32(edge_ids), i32(edge_dst)
    rc = lib.anemoi_gt_attention_fused_edge_bwd(
        qp, ldq, kp, ldk, vp, ldv, edge_feat.data_ptr(), fe_pad, w_packed.data_ptr(), op, ldo, lse.contiguous().data_ptr(), gp, ldg,
        csc.row.data_ptr(), csc.colptr.data_ptr(), rowptr.data_ptr(), edge_ids.data_ptr(), edge_dst.data_ptr(), dqp, lddq, dkp, lddk,
        dvp, lddv, d_wp.data_ptr(), 0 if d_feat is None else d_feat.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), sf.data_ptr(),
        0 if qg is None else qg.data_ptr(), part.data_ptr(), *_rows(addend, "addend", q.dtype), *_rows(d_addend, "d_addend", q.dtype),
        csc.n_dst, csc.n_src, M, num_heads, D // num_heads, _dt(q), _stream())
    _lib.check(rc, "gt_attention_fused_edge_bwd")
    return dq, dk, dv, d_wp, d_feat


def edge_feature_pad(fe: int) -> int:
    return 4 * ((fe + 1 + 3) // 4)


def pack_edge_features(edge_attr: Tensor) -> Tensor:
    """[M, Fe] (any float dtype) -> fp32 [M, fe_pad] = [edge_attr | 1 | 0...] for the fused-edge attention."""
    _dev(edge_attr)
    M, fe = edge_attr.shape
    fe_pad = edge_feature_pad(fe)
    out = torch.empty((M, fe_pad), dtype=torch.float32, device=edge_attr.device)
    p, ld = _rows(edge_attr, "edge_attr")
    _lib.check(_lib.load().anemoi_pack_edge_features(p, ld, out.data_ptr(), M, fe, fe_pad, _dt(edge_attr), _stream()), "pack_edge_features")
    return out


def pack_edge_weights(w_edge: Tensor, b_edge: Optional[Tensor]) -> Tensor:
    """lin_edge parameters -> fp32 [D, fe_pad] = [w_edge | b_edge | 0] for the fused-edge attention."""
    _dev(w_edge, b_edge)
    D, fe = w_edge.shape
    fe_pad = edge_feature_pad(fe)
    if not w_edge.is_contiguous():
        raise ValueError("w_edge must be contiguous [D, Fe]")
    out = torch.empty((D, fe_pad), dtype=torch.float32, device=w_edge.device)
    rc = _lib.load().anemoi_pack_edge_weights(w_edge.data_ptr(), _vec(b_edge, "b_edge", D, w_edge.dtype), out.data_ptr(), D, fe, fe_pad,
                                              _dt(w_edge), _stream())
    _lib.check(rc, "pack_edge_weights")
    return out


def gt_attention_fused_edge(q: Tensor, k: Tensor, v: Tensor, edge_feat: Tensor, w_packed: Tensor, csc: CSC, num_heads: int,
                            addend: Optional[Tensor] = None, return_lse: bool = False):
    """Attention with lin_edge fused: edge_feat = pack_edge_features(edge_attr) fp32 [M, fe_pad];
    w_packed = pack_edge_weights(lin_edge.weight, lin_edge.bias) fp32 [D, fe_pad]."""
    ext = _ext.ops()
    if ext is not None:
        out, lse = ext.gt_attention_fused_edge(q, k, v, edge_feat, w_packed, csc.row, csc.colptr, csc.order, csc.n_src, num_heads, addend, return_lse)
        return (out, lse) if return_lse else out
    _dev(q, k, v, edge_feat, w_packed, addend, csc.row)
    D = q.shape[1]
    fe_pad = w_packed.shape[1]
    if D % num_heads:
        raise ValueError(f"channels {D} not divisible by heads {num_heads}")
    if edge_feat.dtype != torch.float32 or tuple(edge_feat.shape) != (csc.num_edges, fe_pad) or not edge_feat.is_contiguous():
        raise ValueError(f"edge_feat must be contiguous fp32 [{csc.num_edges}, {fe_pad}], got {tuple(edge_feat.shape)} {edge_feat.dtype}")
    if w_packed.dtype != torch.float32 or tuple(w_packed.shape) != (D, fe_pad) or not w_packed.is_contiguous():
        raise ValueError(f"w_packed must be contiguous fp32 [{D}, {fe_pad}]")
    if q.shape[0] != csc.n_dst or k.shape[0] != csc.n_src or v.shape[0] != csc.n_src:
        raise ValueError("node counts do not match the graph")
    out = torch.empty((csc.n_dst, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((csc.n_dst, num_heads), dtype=torch.float32, device=q.device) if return_lse else None
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, "q"), _rows(k, "k", q.dtype), _rows(v, "v", q.dtype)
    ap, lda = _rows(addend, "addend", q.dtype)
    rc = _lib.load().anemoi_gt_attention_fused_edge_fwd(
        qp, ldq, kp, ldk, vp, ldv, edge_feat.data_ptr(), fe_pad, w_packed.data_ptr(),
        csc.row.data_ptr(), csc.colptr.data_ptr(), csc.order.data_ptr() if csc.order is not None else 0, ap, lda, out.data_ptr(), D,
        lse.data_ptr() if return_lse else 0,
        csc.n_dst, csc.n_src, num_heads, D // num_heads, _dt(q), _stream())
    _lib.check(rc, "gt_attention_fused_edge_fwd")
    return (out, lse) if return_lse else out


WINDOW_HEAD_DIMS = (32, 64, 128)  # the head dimensions csrc/window_attention.hip is built for


def window_attention(q: Tensor, k: Tensor, v: Tensor, num_heads: int, window: Optional[int], *, scale: Optional[float] = None,
                     softcap: Optional[float] = None, alibi_slopes: Optional[Tensor] = None, batch_size: int = 1, return_lse: bool = False):
    """Sliding-window multi-head self-attention (layers/attention.py MultiHeadSelfAttention with flash-attention semantics).  q, k, v:
    [batch * N, A] (column slices of one projection buffer are read in place), head h = columns [h d, (h+1) d), d = A / num_heads in
    WINDOW_HEAD_DIMS; query i attends keys j of its own sequence with |i - j| <= window (None or -1: all).  scale defaults to d^-1/2;
    softcap > 0 caps the scores; alibi_slopes fp32 [num_heads].  Returns out [batch * N, A] (and the fp32 LSE [batch * N, num_heads]).
    Differentiable in q, k, v: with autograd recording it runs as ``autograd.WindowAttentionFunction`` (HIP backward kernel)."""
    _window_shape("window_attention", (q, k, v), num_heads, batch_size,
                  f"q, k and v must be 2-D of one shape, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if _needs_grad(q, k, v):
        from .autograd import WindowAttentionFunction

        out, lse = WindowAttentionFunction.apply(q, k, v, num_heads, window, scale, softcap, alibi_slopes, batch_size)
        return (out, lse) if return_lse else out
    return _window_attention_fwd(q, k, v, num_heads, window, scale=scale, softcap=softcap, alibi_slopes=alibi_slopes, batch_size=batch_size,
                                 return_lse=return_lse)


def _window_shape(op: str, operands, num_heads: int, batch_size: int, one_shape: str) -> tuple[int, int, int]:
    """The shape checks ``window_attention`` and ``window_attention_bwd`` share: 2-D operands of one shape [rows, A] (``one_shape`` is the
    op's message for that), heads that divide A into a supported head dimension, a batch size that divides the rows.  -> (rows, A, d)."""
    q = operands[0]
    if q.dim() != 2 or any(t.shape != q.shape for t in operands[1:]):
        raise ValueError(one_shape)
    rows, A = q.shape
    if num_heads <= 0 or A % num_heads:
        raise ValueError(f"channels {A} not divisible by heads {num_heads}")
    d = A // num_heads
    if d not in WINDOW_HEAD_DIMS:
        raise ValueError(f"{op}: head dimension {d} not supported; supported: {set(WINDOW_HEAD_DIMS)}")
    if batch_size <= 0 or rows % batch_size:
        raise ValueError(f"rows {rows} not divisible by batch_size {batch_size}")
    return rows, A, d


def _window_scalars(d: int, window: Optional[int], scale: Optional[float], softcap: Optional[float]) -> tuple[int, float, float]:
    """(window, scale, softcap) as the C ABI takes them: -1 = unbounded, the default scale d^-1/2, 0 = no cap."""
    w = -1 if window is None or window < 0 else int(min(window, 2**31 - 1))
    return w, float(d ** -0.5 if scale is None else scale), float(softcap) if softcap is not None and softcap > 0 else 0.0


def _window_attention_fwd(q: Tensor, k: Tensor, v: Tensor, num_heads: int, window: Optional[int], *, scale: Optional[float] = None,
                          softcap: Optional[float] = None, alibi_slopes: Optional[Tensor] = None, batch_size: int = 1,
                          return_lse: bool = False):
    rows, A = q.shape
    d = A // num_heads
    w, scale, cap = _window_scalars(d, window, scale, softcap)
    ext = _ext.ops()
    if ext is not None:
        out, lse = ext.window_attention(q, k, v, num_heads, w, scale, cap, alibi_slopes, batch_size, return_lse)
        return (out, lse) if return_lse else out
    _dev(q, k, v, alibi_slopes)
    out = torch.empty((rows, A), dtype=q.dtype, device=q.device)
    lse = torch.empty((rows, num_heads), dtype=torch.float32, device=q.device) if return_lse else None
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, "q"), _rows(k, "k", q.dtype), _rows(v, "v", q.dtype)
    rc = _lib.load().anemoi_window_attention_fwd(qp, ldq, kp, ldk, vp, ldv, out.data_ptr(), A, lse.data_ptr() if return_lse else 0,
                                                 batch_size, rows // batch_size, num_heads, d, w, scale, cap,
                                                 _vec(alibi_slopes, "alibi_slopes", num_heads, torch.float32), _dt(q), _stream())
    _lib.check(rc, "window_attention_fwd")
    return (out, lse) if return_lse else out


WINDOW_BWD_QUERY_PASS, WINDOW_BWD_KEY_PASS = 1, 2  # include/anemoi_hip.h: ANEMOI_WINDOW_BWD_*


def window_attention_bwd(d_out: Tensor, q: Tensor, k: Tensor, v: Tensor, out: Tensor, lse: Tensor, num_heads: int, window: Optional[int], *,
                         scale: Optional[float] = None, softcap: Optional[float] = None, alibi_slopes: Optional[Tensor] = None,
                         batch_size: int = 1, grads_out=None, delta: Optional[Tensor] = None,
                         passes: int = WINDOW_BWD_QUERY_PASS | WINDOW_BWD_KEY_PASS):
    """Gradients (dq, dk, dv) of ``window_attention`` (csrc/window_attention_bwd.hip: a query pass and a key pass, deterministic).
    ``out`` / ``lse`` are the forward's results, the scalars the forward's.  ``grads_out`` = (dq, dk, dv): write the gradients into these
    row-strided views, e.g. the three column slices of one [rows, 3A] gradient buffer.  ``delta``: the fp32 [rows, H] workspace the query
    pass fills and the key pass reads (allocated here by default); ``passes`` runs one pass alone, for timing."""
    rows, A, d = _window_shape("window_attention_bwd", (q, k, v, out, d_out), num_heads, batch_size,
                               "q, k, v, out and d_out must be 2-D of one shape")
    if tuple(lse.shape) != (rows, num_heads) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError(f"lse must be contiguous fp32 [{rows}, {num_heads}]")
    w, scale, cap = _window_scalars(d, window, scale, softcap)
    _dev(d_out, q, k, v, out, lse, alibi_slopes, delta)
    if grads_out is None:
        dq, dk, dv = (torch.empty((rows, A), dtype=q.dtype, device=q.device) for _ in range(3))
    else:
        dq, dk, dv = grads_out
        if dq.shape != q.shape or dk.shape != q.shape or dv.shape != q.shape:
            raise ValueError("grads_out shapes must equal q's")
    if delta is None:
        delta = torch.empty((rows, num_heads), dtype=torch.float32, device=q.device)
    elif tuple(delta.shape) != (rows, num_heads) or delta.dtype != torch.float32 or not delta.is_contiguous():
        raise ValueError(f"delta must be contiguous fp32 [{rows}, {num_heads}]")
    if rows == 0:  # nothing to launch (and an empty d_out has no strides to speak of)
        return dq, dk, dv
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, "q"), _rows(k, "k", q.dtype), _rows(v, "v", q.dtype)
    (op, ldo), (gp, ldg) = _rows(out, "out", q.dtype), _rows(d_out, "d_out", q.dtype)
    (dqp, lddq), (dkp, lddk), (dvp, lddv) = _rows(dq, "dq", q.dtype), _rows(dk, "dk", q.dtype), _rows(dv, "dv", q.dtype)
    rc = _lib.load().anemoi_window_attention_bwd(qp, ldq, kp, ldk, vp, ldv, op, ldo, gp, ldg, lse.data_ptr(), dqp, lddq, dkp, lddk, dvp, lddv,
                                                 delta.data_ptr(), batch_size, rows // batch_size, num_heads, d, w, scale, cap,
                                                 _vec(alibi_slopes, "alibi_slopes", num_heads, torch.float32), int(passes), _dt(q), _stream())
    _lib.check(rc, "window_attention_bwd")
    return dq, dk, dv


WINDOW_PASSES = ("forward", "backward_query", "backward_key")  # WinPass of csrc/window_attention_core.h
WINDOW_TILE_CLASSES = ("skipped", "masked", "full")              # include/anemoi_hip.h: ANEMOI_WINDOW_TILE_*


class WindowAttentionPlan(NamedTuple):
    """What one wave of a window-attention kernel does with its sequence; fields as in anemoi_window_attention_plan_t, plus one of
    WINDOW_TILE_CLASSES per streamed tile (tile t = rows [lo + t tile_rows, + tile_rows), rows from ``hi`` on read as zeros)."""
    window: int
    rows_per_block: int
    grid_x: int
    tile_rows: int
    lo: int
    hi: int
    ntiles: int
    tiles: tuple


def window_attention_plan(op: str, seq_len: int, d: int, window: Optional[int], *, dtype: torch.dtype = torch.bfloat16, block: int = 0,
                          wave: int = 0) -> WindowAttentionPlan:
    """The band arithmetic of ``window_attention`` / ``window_attention_bwd`` (``op``: one of WINDOW_PASSES) for workgroup ``block`` and
    wave ``wave`` of a sequence of ``seq_len`` rows: the functions the kernels themselves call (csrc/window_attention_core.h).  Host-only:
    nothing is launched and no GPU is needed."""
    w = -1 if window is None or window < 0 else int(min(window, 2**31 - 1))
    capacity = max(int(seq_len), 0) // 32 + 2
    out, classes = _lib.WindowAttentionPlan(), (_lib.C.c_int32 * capacity)()
    rc = _lib.load().anemoi_window_attention_plan(WINDOW_PASSES.index(op), int(seq_len), int(d), w, _DT[dtype], int(block), int(wave), out,
                                                  classes, capacity)
    _lib.check(rc, "window_attention_plan")
    return WindowAttentionPlan(**{name: getattr(out, name) for name, _ in out._fields_},
                               tiles=tuple(WINDOW_TILE_CLASSES[c] for c in classes[:out.ntiles]))


# ------------------------------------------------------------------------------------------ sparse projection
@dataclass(frozen=True)
class SparseMatrix:
    """A constant CSR matrix [n_rows, n_cols] (rows = destination nodes, columns = source nodes): int32 ``indptr`` [n_rows + 1] and
    ``indices`` [nnz], fp32 ``values`` [nnz]; ``t``: its transpose (the matrix of the backward pass), built once on the host."""

    indptr: Tensor
    indices: Tensor
    values: Tensor
    n_rows: int
    n_cols: int
    t: Optional["SparseMatrix"] = None

    @property
    def nnz(self) -> int:
        return self.indices.shape[0]

    def to(self, device) -> "SparseMatrix":
        mv = lambda a: a.to(device)  # noqa: E731
        return SparseMatrix(mv(self.indptr), mv(self.indices), mv(self.values), self.n_rows, self.n_cols, None if self.t is None else self.t.to(device))


def build_sparse_matrix(indptr, indices, values, shape: tuple[int, int], with_transpose: bool = True) -> SparseMatrix:
    """Host-side constructor (CPU tensors or numpy arrays of a CSR matrix): checks the structure ONCE - the kernel trusts it - and builds
    the transposed copy (stable sort by column: the rows of a column stay in ascending order, the order is a function of the matrix only)."""
    indptr, indices = torch.as_tensor(indptr).long().reshape(-1), torch.as_tensor(indices).long().reshape(-1)
    values = torch.as_tensor(values).to(torch.float32).reshape(-1)
    n_rows, n_cols = int(shape[0]), int(shape[1])
    if max(n_rows, n_cols, indices.numel()) >= 2**31:
        raise ValueError("matrix too large for int32 indices")
    if indptr.numel() != n_rows + 1 or int(indptr[0]) != 0 or int(indptr[-1]) != indices.numel() or bool((indptr[1:] < indptr[:-1]).any()):
        raise ValueError(f"indptr is not a row pointer of {n_rows} rows over {indices.numel()} entries")
    if values.numel() != indices.numel():
        raise ValueError(f"{values.numel()} values for {indices.numel()} indices")
    if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= n_cols):
        raise ValueError(f"column index outside [0, {n_cols})")
    i32 = lambda a: a.to(torch.int32).contiguous()  # noqa: E731
    t = None
    if with_transpose:
        rows = torch.repeat_interleave(torch.arange(n_rows), indptr[1:] - indptr[:-1])
        order = torch.sort(indices, stable=True)[1]
        tptr = torch.zeros(n_cols + 1, dtype=torch.long)
        if indices.numel():
            tptr[1:] = torch.cumsum(torch.bincount(indices, minlength=n_cols), 0)
        t = SparseMatrix(i32(tptr), i32(rows[order]), values[order].contiguous(), n_cols, n_rows)
    return SparseMatrix(i32(indptr), i32(indices), values.contiguous(), n_rows, n_cols, t)


def sparse_project(x: Tensor, matrix: SparseMatrix, cols: Optional[Tensor] = None, mul: Optional[Tensor] = None, add: Optional[Tensor] = None,
                   out_dtype=None) -> Tensor:
    """y[..., m, c] = sum_e matrix[m, e] * (x[..., e, cols[c]] * mul[c] + add[c]): the projection of SparseProjector
    (layers/sparse_projector.py:78-104) as one launch.  x: [..., n_src, V], last dimension contiguous, row and batch strides free (a time
    step of [B, T, E, N, V] is read in place); cols: int32 [C] (default: all V columns); mul / add: fp32 [C]; the result is
    [..., n_dst, C] in ``out_dtype`` (x's dtype or float32; default x's).  fp32 accumulation in CSR order, bitwise reproducible.
    Differentiable in x (the adjoint runs the same kernel on ``matrix.t``)."""
    if _needs_grad(x):
        from .autograd import SparseProjectFunction

        return SparseProjectFunction.apply(x, matrix, cols, mul, add, out_dtype)
    return _sparse_project_fwd(x, matrix, cols, mul, add, out_dtype)


def _sparse_project_fwd(x: Tensor, matrix: SparseMatrix, cols: Optional[Tensor], mul: Optional[Tensor], add: Optional[Tensor], out_dtype) -> Tensor:
    if x.dim() < 2 or x.shape[-2] != matrix.n_cols:
        raise ValueError(f"sparse_project: x {tuple(x.shape)} does not have the matrix's {matrix.n_cols} source rows in its last but one dimension")
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in (x.dtype, torch.float32):
        raise ValueError(f"sparse_project: out_dtype must be {x.dtype} or float32, got {out_dtype}")
    lead, V = x.shape[:-2], x.shape[-1]
    if V > 1 and x.stride(-1) != 1:
        raise ValueError("sparse_project: the last dimension of x must be contiguous")
    xk = _two_leading(x)  # [outer, inner, n_src, V]: a view; a copy only if the leading dimensions need more than two strides
    C = V if cols is None else cols.shape[0]
    ext = _ext.ops()
    if ext is not None:
        y = ext.sparse_project(xk, matrix.indptr, matrix.indices, matrix.values, cols, mul, add, out_dtype == torch.float32)
        return y.view(*lead, matrix.n_rows, C)
    _dev(xk, matrix.indptr, matrix.indices, matrix.values, cols, mul, add)
    _dt(xk)
    if matrix.indptr.dtype != torch.int32 or matrix.indices.dtype != torch.int32 or matrix.values.dtype != torch.float32:
        raise ValueError("sparse_project: the matrix must be int32 / int32 / float32")
    outer, inner = xk.shape[0], xk.shape[1]
    ldx = xk.stride(2) if matrix.n_cols > 1 else max(V, xk.stride(2))
    bsx, bsx_in = (xk.stride(0) if outer > 1 else 0), (xk.stride(1) if inner > 1 else 0)
    if ldx < V or bsx < 0 or bsx_in < 0:
        raise ValueError("sparse_project: x must have non-negative batch strides and a row stride of at least its width")
    B = outer * inner
    y = torch.empty((B, matrix.n_rows, C), dtype=out_dtype, device=x.device)
    rc = _lib.load().anemoi_sparse_project_fwd(xk.data_ptr(), ldx, bsx, max(inner, 1), bsx_in, matrix.n_cols, V, matrix.indptr.data_ptr(),
                                               matrix.indices.data_ptr(), matrix.values.data_ptr(), _vec(cols, "cols", C, torch.int32),
                                               _vec(mul, "mul", C, torch.float32), _vec(add, "add", C, torch.float32), y.data_ptr(), C,
                                               matrix.n_rows * C, B, matrix.n_rows, C, _DT[xk.dtype], _DT[out_dtype], _stream())
    _lib.check(rc, "sparse_project_fwd")
    return y.view(*lead, matrix.n_rows, C)


def _two_leading(x: Tensor) -> Tensor:
    """x [..., n, V] as [outer, inner, n, V] without copying when its leading dimensions can be addressed by two strides (adjacent dimensions
    that share a stride are merged; size-1 dimensions are dropped): every [B, E] step slice of [B, T, E, N, V] qualifies.  Otherwise a
    contiguous copy."""
    n, V = x.shape[-2], x.shape[-1]
    groups: list = []  # [size, stride] of merged leading dimensions, outermost first
    for size, stride in zip(x.shape[:-2], x.stride()[:-2]):
        if size == 1:
            continue
        if groups and groups[-1][1] == size * stride:
            groups[-1] = [groups[-1][0] * size, stride]
        else:
            groups.append([size, stride])
    if len(groups) > 2 or x.numel() == 0:
        lead = 1
        for d in x.shape[:-2]:
            lead *= d
        return x.reshape(1, lead, n, V)
    while len(groups) < 2:
        groups.insert(0, [1, 0])
    return x.as_strided((groups[0][0], groups[1][0], n, V), (groups[0][1], groups[1][1], x.stride(-2), x.stride(-1)), x.storage_offset())


def cond_layer_norm(x: Tensor, scale: Tensor, shift: Tensor, eps: float = 1e-5) -> Tensor:
    """y = LayerNorm(x) * (scale + 1) + shift over the last dim, per-row scale / shift [N, D] (column slices allowed)."""
    if _needs_grad(x, scale, shift):
        from .autograd import CondLayerNormFunction

        return CondLayerNormFunction.apply(x, scale, shift, float(eps))
    return _cond_layer_norm_fwd(x, scale, shift, eps)


def _cond_layer_norm_fwd(x: Tensor, scale: Tensor, shift: Tensor, eps: float = 1e-5) -> Tensor:
    _dev(x, scale, shift)
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if tuple(scale.shape) != tuple(x2.shape) or tuple(shift.shape) != tuple(x2.shape):
        raise ValueError("scale / shift must be [rows(x), D]")
    y = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device)
    (p, ld), (sp, lds), (bp, ldb) = _rows(x2, "x"), _rows(scale, "scale", x.dtype), _rows(shift, "shift", x.dtype)
    _lib.check(_lib.load().anemoi_cond_layernorm_fwd(p, ld, sp, lds, bp, ldb, y.data_ptr(), D, x2.shape[0], D, float(eps), _dt(x), _stream()),
               "cond_layernorm_fwd")
    return y.view(x.shape)


COND_PROJ_MAX = 32  # conditioning widths the in-kernel modulation of cond_layer_norm_proj takes (csrc/rowwise.hip: kCondMax)


def cond_layer_norm_proj_weights(scale_weight: Tensor, scale_bias: Tensor, shift_weight: Tensor, shift_bias: Tensor) -> tuple[Tensor, Tensor]:
    """The prepared operands of ``cond_layer_norm_proj`` from the two Linear maps of a ConditionalLayerNorm ([D, C] weights, [D] biases):
    the C-major image [C, 2 D] (row c = column c of both weights, so that a lane's columns are contiguous) and the biases [2 D]."""
    return (torch.cat([scale_weight, shift_weight], 0).t().contiguous(), torch.cat([scale_bias, shift_bias]).contiguous())


def cond_layer_norm_proj(x: Tensor, cond: Tensor, w: Tensor, b: Tensor, eps: float = 1e-5, residual: Optional[Tensor] = None) -> Tensor:
    """y = LayerNorm(x) * (1 + cond Ws^T + bs) + (cond Wb^T + bb) [+ residual] in ONE launch: the modulation is computed in the kernel,
    in fp32, from the conditioning rows ``cond`` [rows(x), C] (C <= COND_PROJ_MAX; a column slice or unaligned rows are fine) and the
    prepared operands (w [C, 2 D], b [2 D]) of ``cond_layer_norm_proj_weights``.  Inference only (no autograd)."""
    ext = _ext.ops()
    if ext is not None:
        return ext.cond_layer_norm_proj(x, cond, w, b, float(eps), residual)
    _dev(x, cond, w, b, residual)
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if x2.shape[1] > 1 and x2.stride(1) != 1:
        x2 = x2.contiguous()
    if cond.dim() != 2 or cond.shape[0] != x2.shape[0]:
        raise ValueError(f"cond must be [rows(x), C], got {tuple(cond.shape)}")
    C = cond.shape[1]
    if tuple(w.shape) != (C, 2 * D) or not w.is_contiguous() or w.dtype != x.dtype:
        raise ValueError("w must be the contiguous [C, 2 D] image of [scale.weight ; bias.weight] in x's dtype")
    if residual is not None and residual.shape != x.shape:
        raise ValueError("residual shape does not match x")
    y = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device)
    (p, ld), (cp, ldc) = _rows(x2, "x"), _rows(cond, "cond", x.dtype)
    rp, ldr = _rows(None if residual is None else residual.reshape(-1, D), "residual", x.dtype)
    rc = _lib.load().anemoi_cond_layernorm_proj_fwd(p, ld, cp, ldc, w.data_ptr(), _vec(b, "bias", 2 * D, x.dtype), rp, ldr, y.data_ptr(), D,
                                                    x2.shape[0], D, C, float(eps), _dt(x), _stream())
    _lib.check(rc, "cond_layernorm_proj_fwd")
    return y.view(x.shape)


def cond_layer_norm_backward(d_y: Tensor, x: Tensor, scale: Tensor, eps: float = 1e-5):
    """(dx, d_scale) of cond_layer_norm, both [N, D]; d_shift is d_y itself."""
    _dev(d_y, x, scale)
    D = x.shape[-1]
    x2, g2 = x.reshape(-1, D), d_y.reshape(-1, D)
    dx = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device)
    ds = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device)
    (xp, ldx), (sp, lds), (gp, ldg) = _rows(x2, "x"), _rows(scale, "scale", x.dtype), _rows(g2, "d_y", x.dtype)
    _lib.check(_lib.load().anemoi_cond_layernorm_bwd(xp, ldx, sp, lds, gp, ldg, dx.data_ptr(), D, ds.data_ptr(), D, x2.shape[0], D, float(eps),
                                                     _dt(x), _stream()), "cond_layernorm_bwd")
    return dx.view(x.shape), ds


def _needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def layer_norm(x: Tensor, weight: Tensor, bias: Optional[Tensor], eps: float = 1e-5, residual: Optional[Tensor] = None,
               out: Optional[Tensor] = None) -> Tensor:
    """LayerNorm over the last dim of a [..., D] tensor (fp32 statistics), optionally + residual (same shape).
    Differentiable: with autograd recording it runs as ``autograd.LayerNormFunction`` (HIP backward kernel).
    ``out`` (inference only): a contiguous [rows, D] tensor that receives the result."""
    if out is not None:
        if _needs_grad(x, weight, bias, residual):
            raise ValueError("layer_norm: out= is an inference-only argument")
        return _layer_norm_fwd(x, weight, bias, eps, residual, out)
    if _needs_grad(x, weight, bias, residual):
        from .autograd import LayerNormFunction

        y = LayerNormFunction.apply(x, weight, bias, float(eps))
        return y if residual is None else y + residual
    return _layer_norm_fwd(x, weight, bias, eps, residual)


def _layer_norm_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor], eps: float = 1e-5, residual: Optional[Tensor] = None,
                    out: Optional[Tensor] = None) -> Tensor:
    """``out``: a contiguous [rows, D] tensor (e.g. the leading rows of a larger buffer) that receives the result."""
    ext = _ext.ops()
    if ext is not None:  # the same entry point through the TORCH_LIBRARY layer: checks and marshalling in C++
        if out is None:
            return ext.layer_norm(x, weight, bias, float(eps), residual)
        ext.layer_norm_out(x, weight, bias, float(eps), residual, out)
        return out.view(x.shape)
    _dev(x, weight, bias, residual, out)
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if x2.shape[1] > 1 and x2.stride(1) != 1:
        x2 = x2.contiguous()
    if out is not None and (tuple(out.shape) != (x2.shape[0], D) or out.dtype != x.dtype or not out.is_contiguous()):
        raise ValueError("layer_norm: out must be a contiguous [rows, D] tensor of x's dtype")
    y = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device) if out is None else out
    p, ld = _rows(x2, "x")
    if residual is not None and residual.shape != x.shape:
        raise ValueError("residual shape does not match x")
    rp, ldr = _rows(None if residual is None else residual.reshape(-1, D), "residual", x.dtype)
    rc = _lib.load().anemoi_layernorm_fwd(p, ld, _vec(weight, "weight", D, x.dtype), _vec(bias, "bias", D, x.dtype), rp, ldr,
                                          y.data_ptr(), D, x2.shape[0], D, float(eps), _dt(x), _stream())
    _lib.check(rc, "layernorm_fwd")
    return y.view(x.shape)


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, act: Optional[str] = None,
           residual: Optional[Tensor] = None, x2: Optional[Tensor] = None, g1: Optional[Tensor] = None,
           idx1: Optional[Tensor] = None, g2: Optional[Tensor] = None, idx2: Optional[Tensor] = None,
           out: Optional[Tensor] = None, seg1=None, seg2=None) -> Tensor:
    """y = act([x | x2] @ weight^T + bias + g1[idx1] + g2[idx2]) + residual.  x [N, K1], x2 [N, K2], weight [O, K1+K2].
    Differentiable: with autograd recording it runs as ``autograd.LinearFunction``; the gather-add terms then need
    ``seg1`` / ``seg2`` = (ptr int32 [rows(g)+1], ids int32 [N] or None): the rows of the output grouped by idx value
    (for a dst-sorted graph: (colptr, None) for idx = dst and (rowptr, edge_ids) for idx = src).
    Leading dimensions of x (and of a residual) count as rows, as in torch.nn.Linear: y gets them back."""
    if x.dim() > 2:
        if out is not None:
            raise ValueError("out= needs a 2-D x")
        res2d = None if residual is None else residual.reshape(-1, residual.shape[-1])
        y = linear(x.reshape(-1, x.shape[-1]), weight, bias, act=act, residual=res2d, x2=x2, g1=g1, idx1=idx1, g2=g2, idx2=idx2,
                   seg1=seg1, seg2=seg2)
        return y.view(*x.shape[:-1], y.shape[-1])
    if _needs_grad(x, weight, bias, residual, x2, g1, g2):
        if out is not None:
            raise ValueError("out= is not supported while autograd is recording")
        from .autograd import LinearFunction

        if x2 is not None:
            x = torch.cat([x, x2.to(x.dtype)], dim=1)
        if g1 is not None or g2 is not None:
            if (g1 is not None and seg1 is None) or (g2 is not None and seg2 is None):
                raise ValueError("the backward of the gather-add terms needs seg1 / seg2 (row groups of idx1 / idx2)")
            return LinearFunction.apply(x, weight, bias, act, residual, g1, idx1, seg1, g2, idx2, seg2)
        return LinearFunction.apply(x, weight, bias, act, residual)
    return _linear_fwd(x, weight, bias, act=act, residual=residual, x2=x2, g1=g1, idx1=idx1, g2=g2, idx2=idx2, out=out)


def _linear_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, act: Optional[str] = None,
                residual: Optional[Tensor] = None, x2: Optional[Tensor] = None, g1: Optional[Tensor] = None,
                idx1: Optional[Tensor] = None, g2: Optional[Tensor] = None, idx2: Optional[Tensor] = None,
                out: Optional[Tensor] = None, want_pre: bool = False):
    """``want_pre`` (training, act = "gelu"): returns (y, pre) with pre = the pre-activation stored by the same kernel, or
    (y, None) when the shape does not run on the DMA-ring kernels (the backward then recomputes it)."""
    if not want_pre:
        ext = _ext.ops()
        if ext is not None:  # the same entry point through the TORCH_LIBRARY layer: checks and marshalling in C++
            if act not in (None, "gelu"):
                raise ValueError(f"unsupported activation {act!r}")
            actc = _lib.ACT_GELU if act == "gelu" else _lib.ACT_NONE
            if out is None:
                return ext.linear(x, weight, bias, actc, residual, x2, g1, idx1, g2, idx2)
            ext.linear_out(x, weight, bias, actc, residual, x2, g1, idx1, g2, idx2, out)
            return out
    _dev(x, weight, bias, residual, x2, g1, idx1, g2, idx2, out)
    N, K1 = x.shape
    K2 = 0 if x2 is None else x2.shape[1]
    O = weight.shape[0]
    if weight.shape[1] != K1 + K2:
        raise ValueError(f"weight is {tuple(weight.shape)}, expected [{O}, {K1 + K2}]")
    if act not in (None, "gelu"):
        raise ValueError(f"unsupported activation {act!r}")
    for name, t in (("x2", x2), ("residual", residual)):
        if t is not None and t.shape[0] != N:
            raise ValueError(f"{name} has {t.shape[0]} rows, expected {N}")
    if residual is not None and residual.shape[1] != O:
        raise ValueError("residual width does not match the output width")
    for name, g, idx in (("g1", g1, idx1), ("g2", g2, idx2)):
        if (g is None) != (idx is None):
            raise ValueError(f"{name} and its index must be given together")
        if g is not None and (g.shape[1] != O or idx.dtype != torch.int32 or idx.shape != (N,) or not idx.is_contiguous()):
            raise ValueError(f"{name}: table must be [*, {O}] and index contiguous int32 [{N}]")
    y = out if out is not None else torch.empty((N, O), dtype=x.dtype, device=x.device)
    dt = x.dtype
    (xp, ldx), (x2p, ldx2), (wp, ldw) = _rows(x, "x"), _rows(x2, "x2", dt), _rows(weight, "weight", dt)
    (g1p, ldg1), (g2p, ldg2), (rp, ldr), (yp, ldy) = _rows(g1, "g1", dt), _rows(g2, "g2", dt), _rows(residual, "residual", dt), _rows(y, "out", dt)
    lib = _lib.load()
    i1p, i2p = idx1.data_ptr() if idx1 is not None else 0, idx2.data_ptr() if idx2 is not None else 0
    actc = _lib.ACT_GELU if act == "gelu" else _lib.ACT_NONE
    if want_pre and act == "gelu" and dt != torch.float32 and N > 0:
        pre = torch.empty((N, O), dtype=dt, device=x.device)
        rc = lib.anemoi_linear_fwd_pre(xp, ldx, K1, x2p, ldx2, K2, wp, ldw, _vec(bias, "bias", O, dt), g1p, ldg1, i1p, g2p, ldg2, i2p, rp, ldr,
                                       yp, ldy, pre.data_ptr(), O, N, O, actc, _dt(x), _stream())
        if rc == 0:
            return y, pre
        if rc != _lib.E_UNSUPPORTED:
            _lib.check(rc, "linear_fwd_pre")
    rc = lib.anemoi_linear_fwd(xp, ldx, K1, x2p, ldx2, K2, wp, ldw, _vec(bias, "bias", O, dt), g1p, ldg1, i1p, g2p, ldg2, i2p, rp, ldr, yp, ldy,
                               N, O, actc, _dt(x), _stream())
    _lib.check(rc, "linear_fwd")
    return (y, None) if want_pre else y


_REDUCE_WS: dict = {}


def _reduce_workspace(D: int, device) -> Tensor:
    """fp32 scratch for the deterministic column sums (per device and width, allocated once)."""
    key = (str(device), D)
    ws = _REDUCE_WS.get(key)
    if ws is None:
        ws = torch.empty(_lib.load().anemoi_reduce_workspace_bytes(D) // 4, dtype=torch.float32, device=device)
        _REDUCE_WS[key] = ws
    return ws


def layer_norm_backward(d_y: Tensor, x: Tensor, weight: Tensor, eps: float = 1e-5, need_param_grads: bool = True):
    """(dx, dgamma fp32 [D], dbeta fp32 [D]) of LayerNorm over the last dim; statistics recomputed from x."""
    _dev(d_y, x, weight)
    D = x.shape[-1]
    x2, g2 = x.reshape(-1, D), d_y.reshape(-1, D)
    dx = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device)
    gb = torch.empty((2, D), dtype=torch.float32, device=x.device) if need_param_grads else None  # one buffer: one cast later
    dg, db = (gb[0], gb[1]) if need_param_grads else (None, None)
    (xp, ldx), (gp, ldg) = _rows(x2, "x"), _rows(g2, "d_y", x.dtype)
    rc = _lib.load().anemoi_layernorm_bwd(xp, ldx, _vec(weight, "weight", D, x.dtype), gp, ldg, dx.data_ptr(), D,
                                          dg.data_ptr() if need_param_grads else 0, db.data_ptr() if need_param_grads else 0,
                                          _reduce_workspace(D, x.device).data_ptr() if need_param_grads else 0,
                                          x2.shape[0], D, float(eps), _dt(x), _stream())
    _lib.check(rc, "layernorm_bwd")
    return dx.view(x.shape), dg, db


def colsum(x: Tensor) -> Tensor:
    """fp32 column sums of a [N, D] tensor (bias gradient), deterministic."""
    _dev(x)
    N, D = x.shape
    out = torch.empty(D, dtype=torch.float32, device=x.device)
    p, ld = _rows(x, "x")
    _lib.check(_lib.load().anemoi_colsum(p, ld, out.data_ptr(), _reduce_workspace(D, x.device).data_ptr(), N, D, _dt(x), _stream()), "colsum")
    return out


def gelu(x: Tensor) -> Tensor:
    """Exact (erf) GELU of a [..., D] tensor as ONE stand-alone kernel (the layer_kernels ``Activation`` plug-in; the fused
    blocks apply GELU in a GEMM epilogue instead).  Differentiable (backward: ``gelu_backward``)."""
    if _needs_grad(x):
        from .autograd import GeluFunction

        return GeluFunction.apply(x)
    return _gelu_fwd(x)


def _gelu_fwd(x: Tensor) -> Tensor:
    _dev(x)
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if x2.shape[1] > 1 and x2.stride(1) != 1:
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], D), dtype=x.dtype, device=x.device)
    p, ld = _rows(x2, "x")
    _lib.check(_lib.load().anemoi_gelu_fwd(p, ld, y.data_ptr(), D, x2.shape[0], D, _dt(x), _stream()), "gelu_fwd")
    return y.view(x.shape)


def gelu_backward(pre: Tensor, d_y: Tensor) -> Tensor:
    """d_pre = d_y * gelu'(pre) (exact erf form), [N, D]."""
    _dev(pre, d_y)
    N, D = pre.shape
    out = torch.empty((N, D), dtype=pre.dtype, device=pre.device)
    (pp, ldp), (gp, ldg) = _rows(pre, "pre"), _rows(d_y, "d_y", pre.dtype)
    _lib.check(_lib.load().anemoi_gelu_bwd(pp, ldp, gp, ldg, out.data_ptr(), D, N, D, _dt(pre), _stream()), "gelu_bwd")
    return out


def edge_ln_residual_segment_sum(z: Tensor, e_old: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float,
                                 csc: CSC) -> tuple[Tensor, Tensor]:
    """e_new = LayerNorm(z) + e_old;  agg[d] = sum of e_new over the in-edges of d.  Returns (e_new, agg).  Differentiable."""
    if _needs_grad(z, e_old, gamma, beta):
        from .autograd import EdgeLnResidualSegmentSumFunction

        return EdgeLnResidualSegmentSumFunction.apply(z, e_old, gamma, beta, float(eps), csc)
    return _edge_ln_residual_segment_sum_fwd(z, e_old, gamma, beta, eps, csc)


def _edge_ln_residual_segment_sum_fwd(z: Tensor, e_old: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float,
                                      csc: CSC) -> tuple[Tensor, Tensor]:
    _dev(z, e_old, gamma, beta, csc.colptr)
    M, D = z.shape
    if M != csc.num_edges or tuple(e_old.shape) != (M, D):
        raise ValueError("edge tensors do not match the graph")
    e_new = torch.empty((M, D), dtype=z.dtype, device=z.device)
    agg = torch.empty((csc.n_dst, D), dtype=z.dtype, device=z.device)
    (zp, ldz), (ep, lde) = _rows(z, "z"), _rows(e_old, "e_old", z.dtype)
    rc = _lib.load().anemoi_edge_ln_residual_segment_sum_fwd(
        zp, ldz, ep, lde, _vec(gamma, "gamma", D, z.dtype), _vec(beta, "beta", D, z.dtype), float(eps), csc.colptr.data_ptr(),
        e_new.data_ptr(), D, agg.data_ptr(), D, csc.n_dst, D, _dt(z), _stream())
    _lib.check(rc, "edge_ln_residual_segment_sum_fwd")
    return e_new, agg


def segment_sum_rows(x: Tensor, ptr: Tensor, ids: Optional[Tensor] = None) -> Tensor:
    """out[r] = sum_{i in [ptr[r], ptr[r+1])} x[ids[i] if ids is given else i]; ptr int32 [n_out + 1], ids int32."""
    _dev(x, ptr, ids)
    for t in (ptr, ids):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
            raise ValueError("ptr / ids must be contiguous int32 vectors")
    D, n_out = x.shape[1], ptr.shape[0] - 1
    if x.shape[0] == 0:  # no rows to sum (a shard without edges): every segment is empty, and x has no data pointer to pass
        return torch.zeros((n_out, D), dtype=x.dtype, device=x.device)
    out = torch.empty((n_out, D), dtype=x.dtype, device=x.device)
    p, ld = _rows(x, "x")
    rc = _lib.load().anemoi_segment_sum_rows(p, ld, ptr.data_ptr(), ids.data_ptr() if ids is not None else 0, out.data_ptr(), D, n_out, D,
                                             _dt(x), _stream())
    _lib.check(rc, "segment_sum_rows")
    return out


def gather_add_rows(a: Tensor, b: Tensor, idx: Tensor) -> Tensor:
    """out[i] = a[i] + b[idx[i]] (idx int32 [rows(a)])."""
    _dev(a, b, idx)
    if idx.dtype != torch.int32 or idx.shape != (a.shape[0],) or not idx.is_contiguous() or a.shape[1] != b.shape[1]:
        raise ValueError("idx must be contiguous int32 [rows(a)] and a, b must have the same width")
    D = a.shape[1]
    out = torch.empty((a.shape[0], D), dtype=a.dtype, device=a.device)
    (ap, lda), (bp, ldb) = _rows(a, "a"), _rows(b, "b", a.dtype)
    _lib.check(_lib.load().anemoi_gather_add_rows(ap, lda, bp, ldb, idx.data_ptr(), out.data_ptr(), D, a.shape[0], D, _dt(a), _stream()), "gather_add_rows")
    return out


def linear_splitk(a: Tensor, b: Tensor, splits: int) -> Tensor:
    """fp32 [rows(a), rows(b)] = a @ b^T for 16-bit a [R, K], b [C, K] with the reduction split over ``splits`` groups of
    CUs (fp32 atomics): the weight-gradient GEMM.  K must be a multiple of 64 * splits."""
    _dev(a, b)
    R, K = a.shape
    Cc = b.shape[0]
    if b.shape[1] != K or a.dtype != b.dtype or a.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("linear_splitk: a [R, K] and b [C, K] must be bf16/fp16 of the same dtype")
    y = torch.zeros((R, Cc), dtype=torch.float32, device=a.device)
    (ap, lda), (bp, ldb) = _rows(a, "a"), _rows(b, "b", a.dtype)
    _lib.check(_lib.load().anemoi_linear_splitk_f32(ap, lda, bp, ldb, y.data_ptr(), Cc, R, Cc, K, int(splits), _dt(a), _stream()), "linear_splitk_f32")
    return y


def linear_wgrad_eligible(dz: Tensor, x: Tensor) -> bool:
    return (dz.dtype in (torch.bfloat16, torch.float16) and x.dtype == dz.dtype and dz.shape[1] % 8 == 0 and x.shape[1] % 8 == 0
            and dz.shape[0] > 0)


def linear_wgrad(dz: Tensor, x: Tensor, with_bias_grad: bool = False):
    """dW [O, I] = dz^T x for 16-bit dz [N, O], x [N, I] (the reduction runs over the rows; no transposes in HBM);
    ``with_bias_grad``: returns (dW, db) with db [O] = column sums of dz from the same kernel."""
    _dev(dz, x)
    N, O = dz.shape
    I = x.shape[1]
    if x.shape[0] != N or not linear_wgrad_eligible(dz, x):
        raise ValueError("linear_wgrad: dz [N, O] and x [N, I] must be bf16/fp16 of one dtype with O, I multiples of 8")
    lib = _lib.load()
    ws = torch.empty((int(lib.anemoi_linear_wgrad_workspace_bytes(N, O, I)) // 4,), dtype=torch.float32, device=dz.device)
    dw = torch.empty((O, I), dtype=dz.dtype, device=dz.device)
    (zp, ldz), (xp, ldx) = _rows(dz, "dz"), _rows(x, "x", dz.dtype)
    if ldz % 8 or ldx % 8:
        raise ValueError("linear_wgrad: row strides must be multiples of 8 elements")
    db = torch.empty((O,), dtype=dz.dtype, device=dz.device) if with_bias_grad else None
    _lib.check(lib.anemoi_linear_wgrad(zp, ldz, xp, ldx, dw.data_ptr(), I, 0 if db is None else db.data_ptr(), ws.data_ptr(), N, O, I,
                                       _dt(dz), _stream()), "linear_wgrad")
    return (dw, db) if with_bias_grad else dw


def linear_with_row_stats(x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor] = None):
    """(y, stats) with y = x W^T + bias [+ residual] and stats [N, O/64, 2] fp32 = per 64-column strip (sum, sum of squares) of
    the stored rows of y — what ``linear_ln_folded`` needs to apply the LayerNorm of y.  None if the shape is not eligible."""
    ext = _ext.ops()
    if ext is not None:
        y, stats = ext.linear_with_row_stats(x, weight, bias, residual)
        return None if y.dim() != 2 else (y, stats)
    _dev(x, weight, bias, residual)
    N, K = x.shape
    O = weight.shape[0]
    if x.dtype == torch.float32 or O % 64 or K % 64:
        return None
    y = torch.empty((N, O), dtype=x.dtype, device=x.device)
    stats = torch.empty((N, O // 64, 2), dtype=torch.float32, device=x.device)
    dt = x.dtype
    (xp, ldx), (wp, ldw), (rp, ldr) = _rows(x, "x"), _rows(weight, "weight", dt), _rows(residual, "residual", dt)
    rc = _lib.load().anemoi_linear_stats_fwd(xp, ldx, K, wp, ldw, _vec(bias, "bias", O, dt), rp, ldr, y.data_ptr(), O, stats.data_ptr(), N, O,
                                             _dt(x), _stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    _lib.check(rc, "linear_stats_fwd")
    return y, stats


def linear_ln_folded(x: Tensor, w_scaled: Tensor, c: Tensor, d: Tensor, stats: Tensor, eps: float, act: Optional[str] = None):
    """act(LayerNorm(x) W^T + b) from raw x, w_scaled = W * gamma, c = rowsum(w_scaled) (fp32), d = W beta + b (fp32) and the
    producer's row statistics of x.  None if the shape is not eligible (caller: LayerNorm + linear)."""
    ext = _ext.ops()
    if ext is not None:
        y = ext.linear_ln_folded(x, w_scaled, c, d, stats, float(eps), _lib.ACT_GELU if act == "gelu" else _lib.ACT_NONE)
        return None if y.dim() != 2 else y
    _dev(x, w_scaled, c, d, stats)
    N, K = x.shape
    O = w_scaled.shape[0]
    if tuple(stats.shape) != (N, K // 64, 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
        raise ValueError("stats must be contiguous fp32 [N, K/64, 2]")
    y = torch.empty((N, O), dtype=x.dtype, device=x.device)
    dt = x.dtype
    (xp, ldx), (wp, ldw) = _rows(x, "x"), _rows(w_scaled, "w_scaled", dt)
    rc = _lib.load().anemoi_linear_lnfold_fwd(xp, ldx, K, wp, ldw, c.data_ptr(), d.data_ptr(), stats.data_ptr(), K // 64, float(eps),
                                              _lib.ACT_GELU if act == "gelu" else _lib.ACT_NONE, y.data_ptr(), O, N, O, _dt(x), _stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    _lib.check(rc, "linear_lnfold_fwd")
    return y


GEMM_ROLES = ("plain", "plain_pre", "stats_producer", "fold_consumer", "split_k")  # which entry point: GemmRole of csrc/linear_plan.h
GEMM_KERNELS = ("generic", "mfma128", "ring", "splitwave", "bigtile")                # GemmKernel


class GemmPlan(NamedTuple):
    """What a GEMM entry point launches for a shape: ``kernel`` (one of GEMM_KERNELS) on ``tile_m`` x ``tile_n`` output tiles, rows
    [0, main_rows) on the tiles and ``tail_rows`` more on the VALU; the other fields as in anemoi_linear_plan_t (include/anemoi_hip.h)."""
    kernel: str
    tile_m: int
    tile_n: int
    pingpong: bool
    stage_k: int
    mi: int
    wr: int
    kg: int
    stages: int
    epi: int
    main_rows: int
    tail_rows: int
    ln_tail_begin: int


def linear_plan(role: str, n_rows: int, K: int, O: int, *, K2: int = 0, residual: bool = False, gather: bool = False, gelu: bool = False,
                dtype: torch.dtype = torch.bfloat16) -> Optional[GemmPlan]:
    """The kernel choice of ``linear`` / ``linear_with_row_stats`` / ``linear_ln_folded`` / the split-K GEMM (``role``: one of
    GEMM_ROLES) for contiguous operands of this shape, under the environment switches of this process.  Host-only: nothing is
    launched and no GPU is needed.  None where the entry point of the role does not take the shape."""
    out = _lib.LinearPlan()
    bits = (1 if residual else 0) | (2 if gather else 0) | (4 if gelu else 0)
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}[dtype]
    rc = _lib.load().anemoi_linear_plan(GEMM_ROLES.index(role), n_rows, O, K, K2, bits, code, out)
    if rc == _lib.E_UNSUPPORTED:
        return None
    _lib.check(rc, "linear_plan")
    f = {name: getattr(out, name) for name, _ in out._fields_}
    return GemmPlan(**{**f, "kernel": GEMM_KERNELS[out.kernel], "pingpong": bool(out.pingpong)})


# ------------------------------------------------------------------------------------------ row-resident layer chain
CHAIN_CHANNELS = 512  # the chain kernels (csrc/gt_chain2.hip, gnn_chain.hip) are built for this width: 4 waves x 128 / 8 waves x 64 columns

# which entry point: ChainKind of csrc/chain_plan.h
CHAIN_KINDS = ("block_tail", "block_tail_side", "cluster_tail", "row_chain", "row_chain_panels", "embed_fold", "gnn_edge", "gnn_mlp", "gnn_node")
# ChainKernel: the instantiation as the host code names it, its dtype argument dropped
CHAIN_KERNELS = ("none", "gt_chain2_kernel", "gt_chain2_kernel<false,true>", "gt_chain2_kernel<true>", "gt_chain2_kernel<true,true>",
                 "gt_chain2_kernel<false,true,true>", "gt_cluster_chain_kernel", "gt_rowchain_kernel", "gt_rowchain_pipe_kernel", "gt_embed_fold_kernel",
                 "gnn_edge_chain_kernel", "gnn_edge_chain_kernel<true>", "gnn_node_chain_kernel")


class ChainSideShape(NamedTuple):
    """The side job of a ``block_tail_side`` plan: a row-chain job of ``rows`` x ``in_features`` -> ``q_out``, of which ``panels`` panels from
    ``first_panel`` ride, on at most ``cap`` workgroups (0: every idle compute unit)."""
    rows: int
    in_features: int
    q_out: int
    first_panel: int = 0
    panels: int = 0
    cap: int = 0
    rows_per_tile: int = 0


class ChainPlan(NamedTuple):
    """What a chain entry point launches for a shape: ``kernel`` (one of CHAIN_KERNELS; "none": nothing to do) over ``panels`` panels of
    ``rows_per_panel`` rows on ``grid`` workgroups; the other fields as in anemoi_chain_plan_t (include/anemoi_hip.h)."""
    kernel: str
    rows_per_panel: int
    panels: int
    grid: int
    threads: int
    lds_bytes: int
    rounds: int
    idle_cus: int
    host_grid: int
    riders: int
    first: int
    end: int
    side_pipelined: bool
    job_panels: int
    pipelined: bool
    n_rows: int
    row_begin: int


@functools.lru_cache(maxsize=4096)
def chain_plan(kind: str, n_rows: int, *, in_features: int = 0, hidden: int = 0, q_out: int = 0, rows_per_tile: int = 0,
               dtype: torch.dtype = torch.bfloat16, timeline: bool = False, first_panel: int = 0, panels: int = 0,
               side: Optional[ChainSideShape] = None) -> Optional[ChainPlan]:
    """The launch of the chain entry point ``kind`` (one of CHAIN_KINDS) for operands of this shape, under the environment switches of this
    process (``ANEMOI_CHAIN_ROWS``).  Host-only: nothing is launched and no GPU is needed.  None where the entry point returns
    unsupported; ValueError where it returns invalid.  A pure function of its arguments and of process constants: memoised, so that the
    per-forward callers pay a dictionary lookup."""
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}[dtype]
    sd = side or ChainSideShape(0, 0, 0)
    if side is not None:
        first_panel, panels = sd.first_panel, sd.panels
    q = _lib.ChainProblem(CHAIN_KINDS.index(kind), n_rows, in_features, hidden, q_out, rows_per_tile, code, int(timeline), first_panel, panels,
                          sd.rows, sd.in_features, sd.q_out, sd.rows_per_tile, sd.cap)
    out = _lib.ChainPlan()
    rc = _lib.load().anemoi_chain_plan(q, out)
    if rc == _lib.E_UNSUPPORTED:
        return None
    _lib.check(rc, "chain_plan")
    f = {name: getattr(out, name) for name, _ in out._fields_}
    return ChainPlan(**{**f, "kernel": CHAIN_KERNELS[out.kernel], "side_pipelined": bool(out.side_pipelined), "pipelined": bool(out.pipelined)})


def _plans(kind: str, x: Tensor, **shape) -> bool:
    """The entry point ``kind`` takes rows like ``x`` (16-bit, on the GPU) in this shape: its plan exists."""
    if not (x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16)):
        return False
    try:
        return chain_plan(kind, x.shape[0], dtype=x.dtype, **shape) is not None
    except ValueError:
        return False


def _check_chain_images(who: str, dt: torch.dtype, images, vec: Tensor, vec_numel: int, vec_what: str) -> None:
    """The fragment-major weight images (name, tensor or None, elements) and the per-column vector of a chain launch."""
    for name, w, numel in images:
        if w is None and numel == 0:
            continue
        if w is None or w.dim() != 1 or w.numel() != numel or w.dtype != dt or not w.is_contiguous():
            raise ValueError(f"{who}: {name} must be the contiguous fragment-major image ({numel} x {dt}) made by pack_weight_frag")
    if vec.dim() != 1 or vec.numel() != vec_numel or vec.dtype != dt or not vec.is_contiguous():
        raise ValueError(f"{who}: vec must be contiguous [{vec_numel}] {dt} = {vec_what}")


def pack_weight_frag(weight: Tensor) -> Tensor:
    """Fragment-major image of a Linear weight [O, K] (O % 64 == 0, K % 32 == 0) for the chain kernels: one contiguous KiB per
    MFMA B fragment, [O/64 slabs][K/32 k-steps][4 column blocks][4 k-slots][16 rows][8] (include/anemoi_hip.h).  A pure
    re-ordering (torch view + permute), made once per parameter version."""
    O, K = weight.shape
    if O % 64 or K % 32:
        raise ValueError(f"pack_weight_frag: weight [{O}, {K}] needs O % 64 == 0 and K % 32 == 0")
    w = weight.detach().reshape(O // 64, 4, 16, K // 32, 4, 8)  # (slab, ni, row, ks, kslot, e)
    return w.permute(0, 3, 1, 4, 2, 5).contiguous().reshape(-1)


def gt_layer_chain_supported(x: Tensor, hidden: int, q_out: int = 0) -> bool:
    """The experiments build's first chain kernel (tools/experiments_ops.gt_layer_chain): it keeps no vectors in LDS, so neither width has
    a limit, and its entry point has no kind in csrc/chain_plan.h."""
    return (x.is_cuda and x.dim() == 2 and x.shape[1] == CHAIN_CHANNELS and x.dtype in (torch.bfloat16, torch.float16)
            and hidden > 0 and hidden % CHAIN_CHANNELS == 0 and q_out % CHAIN_CHANNELS == 0)


class _Chain2Args(_lib.C.Structure):
    _p, _i64, _i32, _f = _lib.C.c_void_p, _lib.C.c_int64, _lib.C.c_int32, _lib.C.c_float
    _fields_ = [("attn", _p), ("ld_attn", _i64), ("x_res", _p), ("ld_x", _i64), ("wp", _p), ("w1", _p), ("hidden", _i32), ("w2", _p),
                ("wq", _p), ("q_out_features", _i32), ("vec", _p), ("ln1_eps", _f), ("lnq_eps", _f), ("extra", _p), ("ld_extra", _i64),
                ("x_out", _p), ("ld_out", _i64), ("q_out", _p), ("ld_q", _i64), ("n_rows", _i32), ("channels", _i32),
                ("rows_per_tile", _i32), ("timeline", _p)]


def fold_layer_norm(weight: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Optional[Tensor]) -> tuple[Tensor, Tensor]:
    """``LN(x) W^T + b = ((x - mean) rstd) (W diag(gamma))^T + (W beta + b)``: the affine part of a LayerNorm folded into the Linear
    that follows it.  Returns (W diag(gamma) rounded to the weight's dtype, d = W beta + b in fp32)."""
    w = weight.detach().float()
    b = w.new_zeros(w.shape[0]) if bias is None else bias.detach().float()
    wg = (w * gamma.detach().float()).to(weight.dtype)
    d = b if beta is None else w @ beta.detach().float() + b
    return wg, d


def gt_layer_chain2_supported(x: Tensor, hidden: int, q_out: int = 0) -> bool:
    """``q_out``: a multiple of 512, or a NARROW trailing projection of 128, 256 or 384 columns (the decoder's node_data_extractor)."""
    return x.dim() == 2 and x.shape[1] == CHAIN_CHANNELS and _plans("block_tail", x, hidden=hidden, q_out=q_out)


def gt_layer_chain2(attn: Tensor, x_res: Tensor, wp: Tensor, w1g: Tensor, w2: Tensor, vec: Tensor, hidden: int, ln1_eps: float, *,
                    extra: Optional[Tensor] = None, wqg: Optional[Tensor] = None, q_out_features: int = 0, lnq_eps: float = 1e-5,
                    rows_per_tile: int = 0, timeline: Optional[Tensor] = None, want_x_out: bool = True, side: Optional["ChainSide"] = None):
    """The row-local part of a GraphTransformer block in ONE launch with role-split waves (anemoi_gt_chain2_fwd, csrc/gt_chain2.hip):

        x1 = attn Wp^T + bp + x_res;  h = GELU(LN(x1; ln1) W1^T + b1);  x_out = h W2^T + b2 + x1 [+ extra]
        q_out = LN(x_out; lnq) Wq^T + bq        (optional: the NEXT block's LayerNorm + fused q|k|v|self projection)

    with the LayerNorms' affine parts folded by the caller (``fold_layer_norm``): ``w1g`` / ``wqg`` are the fragment-major images of
    ``W diag(gamma)``, ``vec = cat[bp, d1, b2, dq]`` in the model dtype with ``d = W beta + b``.  ``q_out_features`` may also be 128, 256 or
    384 (a narrow trailing projection, e.g. the decoder's ``node_data_extractor`` zero-padded to a multiple of 128 rows); with
    ``want_x_out=False`` (needs a trailing projection) x_out is not written and returned as None.  Returns ``x_out`` or ``(x_out, q_out)``.
    ``side`` (a ``ChainSide``): panels of an independent row-chain job computed by the SAME launch on the compute units this tail leaves idle
    (anemoi_gt_chain2_side_fwd); NotImplementedError, and nothing launched, where the tail leaves none idle (``chain_idle_cus``).
    Inference only (no autograd)."""
    _dev(attn, x_res, wp, w1g, w2, vec, extra, wqg)
    N, D = attn.shape
    dt = attn.dtype
    if D != CHAIN_CHANNELS or dt not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"gt_layer_chain2: {D} channels / {dt} (built for {CHAIN_CHANNELS} channels, 16-bit dtypes)")
    if chain_plan("block_tail", N, hidden=hidden, q_out=q_out_features, rows_per_tile=int(rows_per_tile), dtype=dt, timeline=timeline is not None) is None:
        raise NotImplementedError(f"gt_layer_chain2: hidden={hidden} + q_out={q_out_features} exceed the kernel's LDS vector region")
    if tuple(x_res.shape) != (N, D) or (extra is not None and tuple(extra.shape) != (N, D)):
        raise ValueError("gt_layer_chain2: attn, x_res and extra must have the same [N, channels] shape")
    if extra is not None and not want_x_out:
        raise ValueError("gt_layer_chain2: a second residual needs x_out")
    _check_chain_images("gt_layer_chain2", dt, (("wp", wp, D * D), ("w1g", w1g, hidden * D), ("w2", w2, D * hidden), ("wqg", wqg, q_out_features * D)),
                        vec, 2 * D + hidden + q_out_features, "cat[bp, d1, b2, dq]")
    if not want_x_out and not q_out_features:
        raise ValueError("gt_layer_chain2: want_x_out=False needs a trailing projection")
    x_out = torch.empty((N, D), dtype=dt, device=attn.device) if want_x_out else None
    q_out = torch.empty((N, q_out_features), dtype=dt, device=attn.device) if q_out_features else None
    (ap, lda), (xp, ldx), (ep, lde) = _rows(attn, "attn", dt), _rows(x_res, "x_res", dt), _rows(extra, "extra", dt)
    a = _Chain2Args(ap, lda, xp, ldx, wp.data_ptr(), w1g.data_ptr(), hidden, w2.data_ptr(), 0 if wqg is None else wqg.data_ptr(), q_out_features,
                    vec.data_ptr(), float(ln1_eps), float(lnq_eps), ep, lde, 0 if x_out is None else x_out.data_ptr(), D, 0 if q_out is None else q_out.data_ptr(),
                    q_out_features, N, D, int(rows_per_tile), 0 if timeline is None else timeline.data_ptr())
    if side is None:
        _lib.check(_lib.load().anemoi_gt_chain2_fwd(_lib.C.byref(a), _dt(attn), _stream()), "gt_chain2_fwd")
    else:
        if side.x.dtype != dt or side.x.device != attn.device:
            raise ValueError("gt_layer_chain2: the side job's rows must have the tail's dtype and device")
        n_panels = side.n_panels
        count = n_panels - side.first_panel if side.panels is None else side.panels
        if not (0 <= side.first_panel and 0 <= count and side.first_panel + count <= n_panels and side.max_riders >= 0):
            raise ValueError(f"gt_layer_chain2: side panels [{side.first_panel}, +{count}) of {n_panels}, max_riders={side.max_riders}")
        b = _row_chain_args(side.x, side.we, side.wqg, side.vec, side.q_out_features, side.ln_eps, side.y, side.q, 0)
        _lib.check(_lib.load().anemoi_gt_chain2_side_fwd(_lib.C.byref(a), _lib.C.byref(b), side.first_panel, count, side.max_riders, _dt(attn),
                                                         _stream()), "gt_chain2_side_fwd")
    return x_out if q_out is None else (x_out, q_out)


def chain_idle_cus(n_rows: int) -> int:
    """Compute units a ``gt_layer_chain2`` launch over ``n_rows`` rows leaves idle in every round of panels (the plan's: one workgroup per
    panel up to the chip; beyond, as many as make the rounds even)."""
    return chain_plan("block_tail", n_rows, hidden=CHAIN_CHANNELS).idle_cus if n_rows > 0 else 0


def row_chain_panels(n_rows: int, in_features: int, q_out: int) -> int:
    """Panels of the row-chain job ``gt_row_chain(x [n_rows, in_features], ..., q_out)`` (the plan's)."""
    return chain_plan("row_chain", n_rows, in_features=in_features, q_out=q_out).panels


@dataclass
class ChainSide:
    """A row-chain job (``gt_row_chain``'s operands, outputs preallocated) whose panels ride on block-tail launches: ``gt_layer_chain2(...,
    side=...)`` computes panels [first_panel, first_panel + panels) of it (``panels=None``: to the end); ``max_riders`` caps the workgroups
    that do (0: every idle compute unit)."""
    x: Tensor
    we: Tensor
    wqg: Tensor
    vec: Tensor
    q_out_features: int
    ln_eps: float
    y: Optional[Tensor]   # [N, 512] or None
    q: Tensor             # [N, q_out_features]
    first_panel: int = 0
    panels: Optional[int] = None
    max_riders: int = 0

    @property
    def n_panels(self) -> int:
        return row_chain_panels(self.x.shape[0], self.x.shape[1], self.q_out_features)


class _ClusterChainArgs(_lib.C.Structure):
    _p, _i64, _i32, _f = _lib.C.c_void_p, _lib.C.c_int64, _lib.C.c_int32, _lib.C.c_float
    _fields_ = [("attn", _p), ("ld_attn", _i64), ("x_res", _p), ("ld_x", _i64), ("wp", _p), ("w1", _p), ("hidden", _i32), ("w2", _p),
                ("wq", _p), ("q_out_features", _i32), ("vec", _p), ("ln1_eps", _f), ("lnq_eps", _f), ("extra", _p), ("ld_extra", _i64),
                ("x_out", _p), ("ld_out", _i64), ("q_out", _p), ("ld_q", _i64), ("ln_out", _p), ("ld_ln", _i64), ("q_out2", _p), ("ld_q2", _i64), ("q_split", _i32), ("workspace", _p),
                ("workspace_bytes", _i64), ("n_rows", _i32), ("channels", _i32)]


_CLUSTER_WS: dict = {}


def _cluster_workspace(device) -> Tensor:
    """The cluster chain's exchange workspace (counters + partial-sum slots), zeroed ONCE - its counters are monotonic across launches
    (csrc/gt_cluster_chain.hip).  Launches that share a workspace must be ordered: one per (device, stream) for eager launches and one
    for launches recorded into hipGraphs (a replay is ordered like one stream).  Allocated on first eager use - run a forward eagerly
    before capturing it, as every capture needs anyway."""
    capturing = torch.cuda.is_current_stream_capturing()
    key = (str(device), "graph" if capturing else torch.cuda.current_stream(device).cuda_stream)
    ws = _CLUSTER_WS.get(key)
    if ws is None:
        if capturing:
            raise RuntimeError("gt_cluster_chain: its workspace must exist before hipGraph capture (run the forward once eagerly)")
        n = _lib.load().anemoi_gt_cluster_chain_workspace_bytes()
        ws = _CLUSTER_WS[key] = torch.zeros(n // 4, dtype=torch.int32, device=device)
        _CLUSTER_WS.setdefault((str(device), "graph"), torch.zeros(n // 4, dtype=torch.int32, device=device))
    return ws


def gt_cluster_chain_supported(x: Tensor, hidden: int, q_out: int = 0) -> bool:
    return x.dim() == 2 and x.shape[1] == CHAIN_CHANNELS and _plans("cluster_tail", x, hidden=hidden, q_out=q_out)


def gt_cluster_chain(attn: Tensor, x_res: Tensor, wp: Tensor, w1g: Tensor, w2: Tensor, vec: Tensor, hidden: int, ln1_eps: float, *,
                     extra: Optional[Tensor] = None, wqg: Optional[Tensor] = None, q_out_features: int = 0, lnq_eps: float = 1e-5,
                     ln_out: Optional[Tensor] = None, q_out2: Optional[Tensor] = None, q_split: int = 0):
    """``gt_layer_chain2`` for block tails of a few thousand rows (anemoi_gt_cluster_chain_fwd, csrc/gt_cluster_chain.hip): four CUs of one
    XCD share a 48-row panel as a tensor-parallel group over the MLP's hidden width and exchange the second Linear's partial sums once.
    Same operands (``hidden`` must be 2048); ``ln_out`` (optional, [N, 512]): receives LN'(x2) WITHOUT its affine part; ``q_out2`` (optional,
    [N, q_out_features - 512 q_split], a view with any row stride): receives the trailing projection's chunks from ``q_split`` on (the returned
    ``q_out`` then holds the first ``512 q_split`` columns).  Returns ``x_out`` or ``(x_out, q_out)``.  Inference only (no autograd)."""
    _dev(attn, x_res, wp, w1g, w2, vec, extra, wqg, ln_out, q_out2)
    N, D = attn.shape
    dt = attn.dtype
    if not gt_cluster_chain_supported(attn, hidden, q_out_features):
        raise NotImplementedError(f"gt_cluster_chain: {D} channels / {dt} / hidden={hidden} / q_out={q_out_features}")
    if tuple(x_res.shape) != (N, D) or (extra is not None and tuple(extra.shape) != (N, D)) or (ln_out is not None and tuple(ln_out.shape) != (N, D)):
        raise ValueError("gt_cluster_chain: attn, x_res, extra and ln_out must have the same [N, channels] shape")
    if extra is not None and (q_out_features or ln_out is not None):
        raise ValueError("gt_cluster_chain: a trailing projection / LayerNorm output and a second residual exclude each other")
    _check_chain_images("gt_cluster_chain", dt, (("wp", wp, D * D), ("w1g", w1g, hidden * D), ("w2", w2, D * hidden), ("wqg", wqg, q_out_features * D)),
                        vec, 2 * D + hidden + q_out_features, "cat[bp, d1, b2, dq]")
    ws = _cluster_workspace(attn.device)
    x_out = torch.empty((N, D), dtype=dt, device=attn.device)
    q_cols = q_out_features if q_out2 is None else D * q_split
    if q_out2 is not None and (q_split < 0 or D * q_split > q_out_features or tuple(q_out2.shape) != (N, q_out_features - D * q_split)):
        raise ValueError(f"gt_cluster_chain: q_out2 must be [N, {q_out_features} - 512 q_split] with 0 <= 512 q_split <= q_out_features")
    q_out = torch.empty((N, q_cols), dtype=dt, device=attn.device) if q_cols else None
    (ap, lda), (xp, ldx), (ep, lde), (lp, ldl), (q2p, ldq2) = (_rows(attn, "attn", dt), _rows(x_res, "x_res", dt), _rows(extra, "extra", dt),
                                                              _rows(ln_out, "ln_out", dt), _rows(q_out2, "q_out2", dt))
    a = _ClusterChainArgs(ap, lda, xp, ldx, wp.data_ptr(), w1g.data_ptr(), hidden, w2.data_ptr(), 0 if wqg is None else wqg.data_ptr(), q_out_features,
                          vec.data_ptr(), float(ln1_eps), float(lnq_eps), ep, lde, x_out.data_ptr(), D, 0 if q_out is None else q_out.data_ptr(),
                          max(q_cols, 8), lp, ldl, q2p, ldq2, int(q_split), ws.data_ptr(), ws.numel() * 4, N, D)
    _lib.check(_lib.load().anemoi_gt_cluster_chain_fwd(_lib.C.byref(a), _dt(attn), _stream()), "gt_cluster_chain_fwd")
    return x_out if (q_out is None and q_out2 is None) else (x_out, q_out)


class _RowChainArgs(_lib.C.Structure):
    _p, _i64, _i32, _f = _lib.C.c_void_p, _lib.C.c_int64, _lib.C.c_int32, _lib.C.c_float
    _fields_ = [("x", _p), ("ld_x", _i64), ("in_features", _i32), ("we", _p), ("wq", _p), ("q_out_features", _i32), ("vec", _p), ("ln_eps", _f),
                ("x_out", _p), ("ld_out", _i64), ("q_out", _p), ("ld_q", _i64), ("n_rows", _i32), ("channels", _i32), ("rows_per_tile", _i32)]


def pack_embedding_frag(weight: Tensor) -> Tensor:
    """Fragment-major image of an embedding weight [512, in] with its columns zero-padded to a multiple of 128 (``gt_row_chain``)."""
    O, K = weight.shape
    pad = (-K) % 128
    w = weight.detach()
    return pack_weight_frag(torch.nn.functional.pad(w, (0, pad)) if pad else w)


def gt_row_chain_supported(x: Tensor, q_out: int) -> bool:
    return x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and _plans("row_chain", x, in_features=x.shape[1], q_out=q_out)


def gt_row_chain(x: Tensor, we: Tensor, wqg: Tensor, vec: Tensor, q_out_features: int, ln_eps: float, *, want_x_out: bool = True,
                 rows_per_tile: int = 0):
    """One side of a GraphTransformer mapper in ONE launch (anemoi_gt_rowchain_fwd, csrc/gt_rowchain.hip):

        y = x We^T + be;   q_out = LN(y) Wq^T + bq

    ``we``: ``pack_embedding_frag(We)``; ``wqg``: fragment-major image of ``Wq diag(gamma)``; ``vec = cat[be, Wq beta + bq]`` in the
    model dtype (``fold_layer_norm``).  Returns ``(y or None, q_out)``.  Inference only (no autograd)."""
    N, dt, D = x.shape[0], x.dtype, CHAIN_CHANNELS
    x_out = torch.empty((N, D), dtype=dt, device=x.device) if want_x_out else None
    q_out = torch.empty((N, q_out_features), dtype=dt, device=x.device)
    a = _row_chain_args(x, we, wqg, vec, q_out_features, ln_eps, x_out, q_out, rows_per_tile)
    _lib.check(_lib.load().anemoi_gt_rowchain_fwd(_lib.C.byref(a), _dt(x), _stream()), "gt_rowchain_fwd")
    return x_out, q_out


def gt_row_chain_panels(x: Tensor, we: Tensor, wqg: Tensor, vec: Tensor, q_out_features: int, ln_eps: float, y: Optional[Tensor], q: Tensor,
                        first_panel: int, panels: int) -> None:
    """48-row panels [first_panel, first_panel + panels) of the job ``gt_row_chain(x, ...)`` into the rows of ``y`` (or None) and ``q`` they
    belong to, as one launch with the schedule the whole job's launch has (anemoi_gt_rowchain_panels_fwd): bit for bit the rows ``gt_row_chain``
    writes, whichever launch computes them."""
    a = _row_chain_args(x, we, wqg, vec, q_out_features, ln_eps, y, q, 0)
    _lib.check(_lib.load().anemoi_gt_rowchain_panels_fwd(_lib.C.byref(a), int(first_panel), int(panels), _dt(x), _stream()), "gt_rowchain_panels_fwd")


def _row_chain_args(x: Tensor, we: Tensor, wqg: Tensor, vec: Tensor, q_out_features: int, ln_eps: float, x_out: Optional[Tensor], q_out: Tensor,
                    rows_per_tile: int) -> _RowChainArgs:
    """The argument block of a row-chain job behind the operand checks (``gt_row_chain``; the side job of ``gt_layer_chain2``)."""
    _dev(x, we, wqg, vec, x_out, q_out)
    N, K = x.shape
    dt, D = x.dtype, CHAIN_CHANNELS
    if not gt_row_chain_supported(x, q_out_features):
        raise NotImplementedError(f"gt_row_chain: x {tuple(x.shape)} {dt} / q_out={q_out_features} (16-bit rows of <= {D} columns, a multiple of 8; q_out a multiple of {D})")
    kp = (K + 127) // 128 * 128
    for name, w, numel in (("we", we, D * kp), ("wqg", wqg, q_out_features * D)):
        if w.dim() != 1 or w.numel() != numel or w.dtype != dt or not w.is_contiguous():
            raise ValueError(f"gt_row_chain: {name} must be the contiguous fragment-major image ({numel} x {dt})")
    if vec.dim() != 1 or vec.numel() != D + q_out_features or vec.dtype != dt or not vec.is_contiguous():
        raise ValueError(f"gt_row_chain: vec must be contiguous [{D + q_out_features}] {dt} = cat[be, dq]")
    for name, t, cols in (("x_out", x_out, D), ("q_out", q_out, q_out_features)):
        if t is not None and (tuple(t.shape) != (N, cols) or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"gt_row_chain: {name} must be contiguous [{N}, {cols}] {dt}")
    xp, ldx = _rows(x, "x", dt)
    return _RowChainArgs(xp, ldx, K, we.data_ptr(), wqg.data_ptr(), q_out_features, vec.data_ptr(), float(ln_eps),
                         0 if x_out is None else x_out.data_ptr(), D, q_out.data_ptr(), q_out_features, N, D, int(rows_per_tile))


class _EmbedFoldArgs(_lib.C.Structure):
    _p, _i64, _i32, _f = _lib.C.c_void_p, _lib.C.c_int64, _lib.C.c_int32, _lib.C.c_float
    _fields_ = [("x", _p), ("ld_x", _i64), ("in_features", _i32), ("we", _p), ("wc", _p), ("q_out_features", _i32), ("vec", _p), ("ln_eps", _f),
                ("q_out", _p), ("ld_q", _i64), ("n_rows", _i32), ("channels", _i32)]


def compose_embedding_projection(w_emb: Tensor, b_emb: Optional[Tensor], w_proj: Tensor, b_proj: Optional[Tensor], gamma: Tensor,
                                 beta: Optional[Tensor]) -> tuple[Tensor, Tensor, Tensor]:
    """The operands of ``gt_embed_fold`` for ``Linear(w_emb, b_emb) -> LayerNorm(gamma, beta) -> Linear(w_proj, b_proj)``.  With
    ``W_g = w_proj diag(gamma)`` the chain is ``rstd (W_c x + u - mean s) + d`` with ``W_c = W_g w_emb``, ``u = W_g b_emb``,
    ``s = rowsum(W_g)``, ``d = w_proj beta + b_proj`` and (mean, rstd) the LayerNorm statistics of ``w_emb x + b_emb``.  Everything is
    composed in fp32 from the given weights; ``W_c`` is rounded ONCE to ``w_emb``'s dtype.  Returns (fragment-major image of ``w_emb``,
    fragment-major image of ``W_c``, ``vec = cat[b_emb, u, s, d]``); both images have their columns zero-padded to a multiple of 64 and
    ``vec`` stays in fp32 (the kernel reads it as fp32: the embedding bias is exact there, ``u``, ``s``, ``d`` are not rounded to the
    model dtype as the chain kernels' vectors are).  Plain torch: runs wherever the weights live."""
    dt = w_emb.dtype
    we, wp = w_emb.detach().float(), w_proj.detach().float()
    be = we.new_zeros(we.shape[0]) if b_emb is None else b_emb.detach().float()
    bp = wp.new_zeros(wp.shape[0]) if b_proj is None else b_proj.detach().float()
    wg = wp * gamma.detach().float()
    d = bp if beta is None else wp @ beta.detach().float() + bp
    pad = (-we.shape[1]) % 64
    wc = torch.nn.functional.pad((wg @ we).to(dt), (0, pad))
    we16 = torch.nn.functional.pad(w_emb.detach(), (0, pad))
    return pack_weight_frag(we16), pack_weight_frag(wc), torch.cat([be, wg @ be, wg.sum(dim=1), d]).contiguous()


def gt_embed_fold_supported(x: Tensor, q_out: int) -> bool:
    return x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and _plans("embed_fold", x, in_features=x.shape[1], q_out=q_out)


def gt_embed_fold(x: Tensor, we: Tensor, wc: Tensor, vec: Tensor, q_out_features: int, ln_eps: float) -> Optional[Tensor]:
    """``LayerNorm(x We^T + be) Wq^T + bq`` from the raw rows ``x`` in ONE launch that never stores the embedded rows
    (anemoi_gt_embed_fold_fwd, csrc/gt_embed_fold.hip); ``we, wc, vec``: ``compose_embedding_projection``.  None where the shape is
    not eligible (16-bit rows of at most 256 columns, a multiple of 8; q_out a multiple of 512 up to 2048): the caller keeps the GEMM
    pair.  Inference only (no autograd)."""
    _dev(x, we, wc, vec)
    if not gt_embed_fold_supported(x, q_out_features):
        return None
    N, K = x.shape
    dt, D = x.dtype, CHAIN_CHANNELS
    kp = (K + 63) // 64 * 64
    for name, w, numel in (("we", we, D * kp), ("wc", wc, q_out_features * kp)):
        if w.dim() != 1 or w.numel() != numel or w.dtype != dt or not w.is_contiguous():
            raise ValueError(f"gt_embed_fold: {name} must be the contiguous fragment-major image ({numel} x {dt}) made by compose_embedding_projection")
    if vec.dim() != 1 or vec.numel() != D + 3 * q_out_features or vec.dtype != torch.float32 or not vec.is_contiguous():
        raise ValueError(f"gt_embed_fold: vec must be contiguous fp32 [{D + 3 * q_out_features}] = cat[be, u, s, d]")
    q_out = torch.empty((N, q_out_features), dtype=dt, device=x.device)
    xp, ldx = _rows(x, "x", dt)
    a = _EmbedFoldArgs(xp, ldx, K, we.data_ptr(), wc.data_ptr(), q_out_features, vec.data_ptr(), float(ln_eps), q_out.data_ptr(), q_out_features, N, D)
    rc = _lib.load().anemoi_gt_embed_fold_fwd(_lib.C.byref(a), _dt(x), _stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    _lib.check(rc, "gt_embed_fold_fwd")
    return q_out


def gnn_edge_chain(e: Tensor, g1: Tensor, idx1: Tensor, g2: Tensor, idx2: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor, w2: Tensor,
                   b2: Tensor, ln_w: Tensor, ln_b: Optional[Tensor], eps: float) -> Tensor:
    """GraphConv's edge MLP (three Linears, gather-add form) + LayerNorm + residual in ONE launch (anemoi_gnn_edge_chain_fwd):
    ``LayerNorm(W2 gelu(W1 gelu(W0e e + g1[idx1] + g2[idx2] + b0) + b1) + b2) + e``.  ``w0, w1, w2``: fragment-major images
    (``pack_weight_frag``) of [512, 512] weights; ``idx1 / idx2`` int32.  Inference only."""
    _dev(e, g1, idx1, g2, idx2, w0, b0, w1, b1, w2, b2, ln_w, ln_b)
    M, D = e.shape
    dt = e.dtype
    if D != CHAIN_CHANNELS or dt not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"gnn_edge_chain: {D} channels / {dt} (built for {CHAIN_CHANNELS} channels, 16-bit dtypes)")
    for name, w in (("w0", w0), ("w1", w1), ("w2", w2)):
        if w.dim() != 1 or w.numel() != D * D or w.dtype != dt or not w.is_contiguous():
            raise ValueError(f"gnn_edge_chain: {name} must be the fragment-major image of a [{D}, {D}] weight (pack_weight_frag)")
    for name, ix in (("idx1", idx1), ("idx2", idx2)):
        if ix.dtype != torch.int32 or ix.dim() != 1 or ix.shape[0] != M or not ix.is_contiguous():
            raise ValueError(f"gnn_edge_chain: {name} must be contiguous int32 [{M}]")
    if g1.shape[1] != D or g2.shape[1] != D:
        raise ValueError("gnn_edge_chain: the gathered tables must have 512 columns")
    out = torch.empty((M, D), dtype=dt, device=e.device)
    (ep, lde), (p1, ld1), (p2, ld2) = _rows(e, "e", dt), _rows(g1, "g1", dt), _rows(g2, "g2", dt)
    _lib.check(_lib.load().anemoi_gnn_edge_chain_fwd(ep, lde, p1, ld1, idx1.data_ptr(), p2, ld2, idx2.data_ptr(), w0.data_ptr(), _vec(b0, "b0", D, dt),
                                                     w1.data_ptr(), _vec(b1, "b1", D, dt), w2.data_ptr(), _vec(b2, "b2", D, dt), _vec(ln_w, "ln_w", D, dt),
                                                     _vec(ln_b, "ln_b", D, dt), float(eps), out.data_ptr(), D, M, D, _dt(e), _stream()), "gnn_edge_chain_fwd")
    return out


def gnn_mlp_chain(x: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, ln_w: Tensor, ln_b: Optional[Tensor],
                  eps: float, residual: Optional[Tensor] = None) -> Tensor:
    """An embedding MLP in ONE launch (anemoi_gnn_mlp_chain_fwd): ``LayerNorm(W2 gelu(W1 gelu(W0 x + b0) + b1) + b2) [+ residual]``.
    x [N, K] with K in {128, 256, 384, 512} (zero-padded by the caller), w0 = pack_weight_frag of the [512, K] weight.  Inference only."""
    _dev(x, w0, b0, w1, b1, w2, b2, ln_w, ln_b, residual)
    N, K = x.shape
    D, dt = CHAIN_CHANNELS, x.dtype
    if dt not in (torch.bfloat16, torch.float16) or K % 128 or not 128 <= K <= D:
        raise NotImplementedError(f"gnn_mlp_chain: width {K} / {dt} (built for 16-bit rows of 128, 256, 384 or 512 columns)")
    for name, w, numel in (("w0", w0, D * K), ("w1", w1, D * D), ("w2", w2, D * D)):
        if w.dim() != 1 or w.numel() != numel or w.dtype != dt or not w.is_contiguous():
            raise ValueError(f"gnn_mlp_chain: {name} must be a contiguous fragment-major image of {numel} elements (pack_weight_frag)")
    if residual is not None and (tuple(residual.shape) != (N, D) or residual.dtype != dt):
        raise ValueError("gnn_mlp_chain: residual must be [N, 512] of x's dtype")
    out = torch.empty((N, D), dtype=dt, device=x.device)
    (xp, ldx), (rp, ldr) = _rows(x, "x", dt), _rows(residual, "residual", dt)
    _lib.check(_lib.load().anemoi_gnn_mlp_chain_fwd(xp, ldx, K, w0.data_ptr(), _vec(b0, "b0", D, dt), w1.data_ptr(), _vec(b1, "b1", D, dt), w2.data_ptr(),
                                                    _vec(b2, "b2", D, dt), _vec(ln_w, "ln_w", D, dt), _vec(ln_b, "ln_b", D, dt), float(eps), rp, ldr,
                                                    out.data_ptr(), D, N, D, _dt(x), _stream()), "gnn_mlp_chain_fwd")
    return out


def gnn_node_chain(x: Tensor, agg: Tensor, wa: Tensor, ba: Tensor, wb: Tensor, bb: Tensor, wc: Tensor, bc: Tensor, ln_w: Tensor,
                   ln_b: Optional[Tensor], eps: float, wt: Optional[Tensor] = None, bt: Optional[Tensor] = None, t_out_features: int = 0,
                   seg_ptr: Optional[Tensor] = None):
    """A GraphConv block's node MLP + LayerNorm + skip in ONE launch (anemoi_gnn_node_chain_fwd):
    ``x_out = LayerNorm(Wc gelu(Wb gelu(Wa [x | agg] + ba) + bb) + bc) + x`` and optionally ``t_out = x_out Wt^T [+ bt]``.
    Weights are fragment-major images (``pack_weight_frag``).  Returns ``x_out`` or ``(x_out, t_out)``.  Inference only."""
    _dev(x, agg, wa, ba, wb, bb, wc, bc, ln_w, ln_b, wt, bt)
    N, D = x.shape
    dt = x.dtype
    if D != CHAIN_CHANNELS or dt not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"gnn_node_chain: {D} channels / {dt} (built for {CHAIN_CHANNELS} channels, 16-bit dtypes)")
    if seg_ptr is not None:  # ``agg`` = the dst-sorted EDGE rows [M, 512]; the kernel forms their segmented sums (segment_sum_rows' arithmetic)
        _dev(seg_ptr)
        if agg.dim() != 2 or agg.shape[1] != D or seg_ptr.dtype != torch.int32 or tuple(seg_ptr.shape) != (N + 1,) or not seg_ptr.is_contiguous():
            raise ValueError("gnn_node_chain: with seg_ptr, agg must be the [M, 512] edge rows and seg_ptr contiguous int32 [N + 1]")
    elif tuple(agg.shape) != (N, D):
        raise ValueError("gnn_node_chain: x and agg must have the same [N, 512] shape")
    for name, w, numel in (("wa", wa, 2 * D * D), ("wb", wb, D * D), ("wc", wc, D * D)):
        if w.dim() != 1 or w.numel() != numel or w.dtype != dt or not w.is_contiguous():
            raise ValueError(f"gnn_node_chain: {name} must be a contiguous fragment-major image of {numel} elements (pack_weight_frag)")
    if wt is not None and (t_out_features % D or wt.dim() != 1 or wt.numel() != t_out_features * D or wt.dtype != dt or not wt.is_contiguous()):
        raise ValueError("gnn_node_chain: wt must be the fragment-major image of a [t_out_features, 512] weight, t_out_features % 512 == 0")
    x_out = torch.empty((N, D), dtype=dt, device=x.device)
    tf = t_out_features if wt is not None else 0
    t_out = torch.empty((N, tf), dtype=dt, device=x.device) if tf else None
    (xp, ldx), (ap, lda) = _rows(x, "x", dt), _rows(agg, "agg", dt)
    tail = (wa.data_ptr(), _vec(ba, "ba", D, dt), wb.data_ptr(), _vec(bb, "bb", D, dt), wc.data_ptr(),
            _vec(bc, "bc", D, dt), _vec(ln_w, "ln_w", D, dt), _vec(ln_b, "ln_b", D, dt), float(eps), x_out.data_ptr(), D,
            0 if wt is None else wt.data_ptr(), _vec(bt, "bt", tf, dt) if (bt is not None and tf) else 0, tf,
            0 if t_out is None else t_out.data_ptr(), tf, N, D, _dt(x), _stream())
    if seg_ptr is not None:
        _lib.check(_lib.load().anemoi_gnn_node_chain_segsum_fwd(xp, ldx, ap, lda, seg_ptr.data_ptr(), *tail), "gnn_node_chain_segsum_fwd")
    else:
        _lib.check(_lib.load().anemoi_gnn_node_chain_fwd(xp, ldx, ap, lda, *tail), "gnn_node_chain_fwd")
    return x_out if t_out is None else (x_out, t_out)


GLU_KINDS = {"glu": 0, "swiglu": 1, "geglu": 2, "reglu": 3}


def glu(gate_value: Tensor, kind: str) -> Tensor:
    """out = act(gate) * value for gate_value = [gate | value] [N, 2D]; kind in GLU_KINDS.  Differentiable."""
    if _needs_grad(gate_value):
        from .autograd import GluFunction

        return GluFunction.apply(gate_value, kind)
    return _glu_fwd(gate_value, kind)


def _glu_fwd(gate_value: Tensor, kind: str) -> Tensor:
    _dev(gate_value)
    N, D2 = gate_value.shape
    out = torch.empty((N, D2 // 2), dtype=gate_value.dtype, device=gate_value.device)
    p, ld = _rows(gate_value, "gate_value")
    _lib.check(_lib.load().anemoi_glu_fwd(p, ld, out.data_ptr(), D2 // 2, N, D2 // 2, GLU_KINDS[kind], _dt(gate_value), _stream()), "glu_fwd")
    return out


def glu_backward(gate_value: Tensor, d_out: Tensor, kind: str) -> Tensor:
    _dev(gate_value, d_out)
    N, D2 = gate_value.shape
    out = torch.empty((N, D2), dtype=gate_value.dtype, device=gate_value.device)
    (p, ld), (gp, ldg) = _rows(gate_value, "gate_value"), _rows(d_out, "d_out", gate_value.dtype)
    _lib.check(_lib.load().anemoi_glu_bwd(p, ld, gp, ldg, out.data_ptr(), D2, N, D2 // 2, GLU_KINDS[kind], _dt(gate_value), _stream()), "glu_bwd")
    return out


class ImputeProgram(NamedTuple):
    """The imputation program on the device (include/anemoi_hip.h): ``kind_src`` int32 [V, 2] = (kind, source column) with kind 0 none,
    1 constant, 2 copy; ``value`` fp32 [V], each entry already rounded to the data dtype."""
    kind_src: Tensor
    value: Tensor


def impute_program(kinds, values, sources, device) -> ImputeProgram:
    """Build the device tables from per-column host lists; a copy source that is itself imputed is refused (the kernels read sources
    raw, the reference's sequential fill would read the filled value)."""
    V = len(kinds)
    for c in range(V):
        if kinds[c] not in (0, 1, 2):
            raise ValueError(f"impute_program: column {c}: kind {kinds[c]} is not 0 (none), 1 (constant) or 2 (copy)")
        if kinds[c] == 2 and not (0 <= sources[c] < V and kinds[sources[c]] == 0):
            raise NotImplementedError(f"impute_program: column {c} copies column {sources[c]}, which is out of range or itself imputed")
    ks = torch.tensor([[int(k), int(s) if k == 2 else 0] for k, s in zip(kinds, sources)], dtype=torch.int32).reshape(V, 2)
    return ImputeProgram(ks.to(device), torch.tensor([float(v) for v in values], dtype=torch.float32).to(device))


def _impute_ptrs(impute: Optional[ImputeProgram], V: int, what: str) -> tuple[int, int]:
    if impute is None:  # a chain without this stage: the null pointer group
        return 0, 0
    ks, val = impute
    _dev(ks, val)
    if ks.shape != (V, 2) or ks.dtype != torch.int32 or not ks.is_contiguous():
        raise ValueError(f"{what}: impute.kind_src must be contiguous int32 [{V}, 2], got {tuple(ks.shape)} {ks.dtype}")
    return ks.data_ptr(), _vec(val, "impute.value", V, torch.float32)


def _bool_mask(mask: Tensor, shape: tuple, what: str) -> Tensor:
    if mask.dtype != torch.bool or tuple(mask.shape) != tuple(shape) or not mask.is_contiguous():
        raise ValueError(f"{what}: the mask must be a contiguous torch.bool tensor of shape {tuple(shape)}, got {tuple(mask.shape)} {mask.dtype}")
    return mask


def impute_columns(x: Tensor, impute: ImputeProgram, out: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> Tensor:
    """BaseImputer.transform as one kernel: x [batch, time, grid, V] or [batch, time, ensemble, grid, V] (any strides, columns contiguous);
    a NaN of ensemble member 0 is replaced, in EVERY member, by what the program says for its column; each time step has its own NaN
    locations.  ``out``: x itself (in place) or a tensor of x's shape (default: a new one).  ``mask``: bool [batch, grid, V], receives the NaN
    locations of time step 0, member 0, all columns."""
    _dev(x, impute.kind_src, impute.value, out, mask)
    if x.dim() not in (4, 5) or x.stride(-1) != 1:
        raise ValueError(f"impute_columns: x must be [batch, time, (ensemble,) grid, vars] with contiguous variables, got {tuple(x.shape)}")
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or y.stride(-1) != 1:
        raise ValueError("impute_columns: out must match x")
    x5, y5 = (x.unsqueeze(2), y.unsqueeze(2)) if x.dim() == 4 else (x, y)
    B, T, E, N, V = x5.shape
    kp, vp = _impute_ptrs(impute, V, "impute_columns")
    mp = 0 if mask is None else _bool_mask(mask, (B, N, V), "impute_columns").data_ptr()
    if x5.numel():
        _lib.check(_lib.load().anemoi_impute_columns(x5.data_ptr(), *x5.stride()[:4], y5.data_ptr(), *y5.stride()[:4], kp, vp, mp, B, T, E, N, V, _dt(x),
                                                     _stream()), "impute_columns")
    return y


def restore_nan_columns(x: Tensor, mask: Tensor, src_of: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """BaseImputer.inverse_transform as one kernel: x [batch, ..., grid, V_out] contiguous; y[b, ..., n, c] = NaN where src_of[c] >= 0 and
    mask[b, n, src_of[c]] (mask bool [batch, grid, V_mask], src_of int32 [V_out]), else x.  ``out``: x itself (in place) or like x."""
    _dev(x, mask, src_of, out)
    if x.dim() < 3 or not x.is_contiguous():
        raise ValueError("restore_nan_columns: x must be a contiguous [batch, ..., grid, vars] tensor")
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or not y.is_contiguous():
        raise ValueError("restore_nan_columns: out must match x")
    B, N, V = x.shape[0], x.shape[-2], x.shape[-1]
    if mask.dim() != 3:
        raise ValueError(f"restore_nan_columns: the mask must be [batch, grid, vars], got {tuple(mask.shape)}")
    _bool_mask(mask, (B, N, mask.shape[2]), "restore_nan_columns")
    M = x.numel() // max(1, B * N * V)
    if x.numel():
        _lib.check(_lib.load().anemoi_restore_nan_columns(x.data_ptr(), V, y.data_ptr(), V, mask.data_ptr(), mask.shape[2], mask.shape[2],
                                                          _vec(src_of, "src_of", V, torch.int32), B, M, N, V, _dt(x), _stream()), "restore_nan_columns")
    return y


def assemble_input(x: Tensor, attrs: Optional[Tensor], width: int, col_mul: Optional[Tensor] = None, col_add: Optional[Tensor] = None,
                   out_dtype: Optional[torch.dtype] = None, *, impute: Optional[ImputeProgram] = None, nan_mask: Optional[Tensor] = None,
                   remap: Optional["RemapProgram"] = None) -> Tensor:
    """x [T, N, V] (time slices of one batch / ensemble member), attrs [N, A] -> [N, width] = [x[0] | ... | x[T-1] | attrs | 0...].
    With ``col_mul`` / ``col_add`` (fp32 [V]) the time / variable columns become x * mul[v] + add[v] (the input normaliser as a
    column program); ``out_dtype``: the model dtype when x is fp32 data fed to a 16-bit model (default: x's dtype).
    ``impute`` (with ``nan_mask`` bool [N, V]): every raw element is imputed within its own time step before the normaliser, and
    nan_mask receives the NaN locations of step 0.  ``remap`` (the FORWARD program of a remapper over the V columns): every raw element
    is remapped after the imputation and before the normaliser."""
    _dev(x, attrs, col_mul, col_add)
    T, N, V = x.shape
    A = 0 if attrs is None else attrs.shape[1]
    odt = x.dtype if out_dtype is None else out_dtype
    if x.stride(2) != 1 or width < T * V + A or (attrs is not None and (attrs.shape[0] != N or attrs.dtype != odt)):
        raise ValueError("assemble_input: x must be [T, N, V] with contiguous variables, attrs [N, A] of the output dtype")
    out = torch.empty((N, width), dtype=odt, device=x.device)
    ap, lda = _rows(attrs, "attrs", odt)
    staged = impute is not None or nan_mask is not None or remap is not None
    plain_pad = T == 1 and A == 0 and odt != torch.float32 and width % 8 == 0  # cast + zero-pad of [N, V] rows: the division-free 16-byte path
    if not staged and col_mul is None and col_add is None and odt == x.dtype and not plain_pad:
        _lib.check(_lib.load().anemoi_assemble_input(x.data_ptr(), x.stride(0), x.stride(1), T, V, ap, lda, A, out.data_ptr(), width, width, N,
                                                     _dt(x), _stream()), "assemble_input")
        return out
    if (impute is None) != (nan_mask is None):
        raise ValueError("assemble_input: impute and nan_mask go together")
    if (col_mul is None) != (col_add is None):
        raise ValueError("assemble_input: col_mul and col_add go together")
    if x.dtype != odt and x.dtype != torch.float32:
        raise ValueError("assemble_input: x must be in the output dtype or fp32")
    _dev(x, nan_mask)
    mp = 0 if nan_mask is None else _bool_mask(nan_mask, (N, V), "assemble_input").data_ptr()
    _lib.check(_lib.load().anemoi_assemble_input_chain(x.data_ptr(), _dt(x), x.stride(0), x.stride(1), T, V, *_impute_ptrs(impute, V, "assemble_input"),
                                                       mp, V, *_remap_ptrs(remap, V, "assemble_input"), _vec(col_mul, "col_mul", V, torch.float32),
                                                       _vec(col_add, "col_add", V, torch.float32), ap, lda, A, out.data_ptr(), width, width, N,
                                                       _DT[odt], _stream()), "assemble_input_chain")
    return out


def assemble_output(x_out: Tensor, x_skip: Tensor, col_map: Tensor, col_mul: Optional[Tensor] = None, col_add: Optional[Tensor] = None, *,
                    impute: Optional[ImputeProgram] = None, remap: Optional["RemapProgram"] = None) -> Tensor:
    """out[n, v] = x_out[n, v] + x_skip[n, col_map[v]] (where col_map[v] >= 0); x_out [N, V_out], x_skip [N, V_in] (row
    stride allowed), col_map int32 [V_out].  With ``col_mul`` / ``col_add`` (fp32 [V_in]) the skip is the RAW input, normalised
    on the fly (x_skip * mul[m] + add[m]); the result has x_skip's dtype (the model dtype or fp32).  ``impute`` (over the V_in columns):
    the raw skip is imputed before it is normalised.  ``remap`` (the FORWARD program of a remapper over the V_in columns): the raw skip is
    remapped after the imputation and before the normaliser."""
    _dev(x_out, x_skip, col_map, col_mul, col_add)
    N, V = x_out.shape
    out = torch.empty((N, V), dtype=x_skip.dtype, device=x_out.device)
    (xp, ldx), (sp, lds) = _rows(x_out, "x_out"), _rows(x_skip, "x_skip")
    Vin = x_skip.shape[1]
    if impute is None and remap is None and col_mul is None and col_add is None and x_skip.dtype == x_out.dtype:
        _lib.check(_lib.load().anemoi_assemble_output(xp, ldx, sp, lds, col_map.data_ptr(), out.data_ptr(), V, N, V, _dt(x_out), _stream()), "assemble_output")
        return out
    if x_skip.dtype != x_out.dtype and x_skip.dtype != torch.float32:
        raise ValueError("assemble_output: x_skip must be in x_out's dtype or fp32")
    _lib.check(_lib.load().anemoi_assemble_output_chain(xp, ldx, _dt(x_out), sp, lds, _vec(col_map, "col_map", V, torch.int32),
                                                        *_impute_ptrs(impute, Vin, "assemble_output"), *_remap_ptrs(remap, Vin, "assemble_output"),
                                                        _vec(col_mul, "col_mul", Vin, torch.float32), _vec(col_add, "col_add", Vin, torch.float32),
                                                        out.data_ptr(), V, N, V, _dt(x_skip), _stream()), "assemble_output_chain")
    return out


def affine_columns(x: Tensor, col_mul: Tensor, col_add: Tensor, inverse: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Per-variable affine map over the last dimension: x * mul + add, or (x - add) / mul with ``inverse`` (InputNormalizer
    transform / inverse_transform).  ``out`` may be x itself (in place)."""
    _dev(x, col_mul, col_add, out)
    V = x.shape[-1]
    if not x.is_contiguous():
        raise ValueError("affine_columns: x must be contiguous")
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or not y.is_contiguous():
        raise ValueError("affine_columns: out must match x")
    n = x.numel() // V
    _lib.check(_lib.load().anemoi_affine_columns(x.data_ptr(), V, y.data_ptr(), V, _vec(col_mul, "col_mul", V, torch.float32),
                                                 _vec(col_add, "col_add", V, torch.float32), 1 if inverse else 0, n, V, _dt(x), _stream()),
               "affine_columns")
    return y


def bound_columns_(x: Tensor, op_table: Tensor, param_table: Tensor, *, nan_mask: Optional[Tensor] = None, n_nan_ops: int = 0) -> Tensor:
    """In place: apply the column program (int32 [n_ops, 4], fp32 [n_ops, 2]; see anemoi_column_program) to x [..., V].  ``nan_mask``
    (bool [rows of x, V_mask]) serves the ops of kind 10, (10, dst column, mask column, 0): NaN where the mask is set; ``n_nan_ops``: how
    many of them the program holds - a program with such ops and no mask is an error."""
    _dev(x, op_table, param_table, nan_mask)
    if not x.is_contiguous():
        raise ValueError("bound_columns_: x must be contiguous")
    return _column_program(x, op_table, param_table, nan_mask, int(n_nan_ops), False, "bound_columns_")


def _column_program(x: Tensor, op_table: Tensor, param_table: Tensor, nan_mask: Optional[Tensor], n_nan_ops: int, extended: bool, what: str) -> Tensor:
    """The one launch behind ``bound_columns_`` and ``column_program_``; ``extended``: the tables may hold the kinds above 10."""
    V = x.shape[-1]
    mp = vm = 0
    if nan_mask is not None:
        vm = nan_mask.shape[-1]
        mp = _bool_mask(nan_mask, nan_mask.shape, what).data_ptr()
        if nan_mask.numel() != (x.numel() // V) * vm:
            raise ValueError(f"{what}: the mask {tuple(nan_mask.shape)} does not have one row per row of x {tuple(x.shape)}")
    _lib.check(_lib.load().anemoi_column_program(x.data_ptr(), V, x.numel() // V, V, op_table.data_ptr(), param_table.data_ptr(), op_table.shape[0],
                                                 mp, vm, vm, n_nan_ops, 1 if extended else 0, _dt(x), _stream()), "column_program")
    return x


class RemapProgram(NamedTuple):
    """One direction of a remapper on the device (include/anemoi_hip.h): ``op_flags`` int32 [V, 2] = (remap op, flags), ``par`` fp32 [V, 4],
    ``active`` int32: the columns whose op is not 0 (none)."""
    op_flags: Tensor
    par: Tensor
    active: Tensor


REMAP_OPS = 16  # the remap ops are 0 (none) .. 16 (affine inverse), include/anemoi_hip.h


def remap_program(entries, device) -> RemapProgram:
    """Build the device tables from one host entry per column: ``(op, flags, p0, p1, p2, p3)``, op 0 = the column is left alone."""
    V = len(entries)
    for c, e in enumerate(entries):
        if len(e) != 6 or not 0 <= int(e[0]) <= REMAP_OPS:
            raise ValueError(f"remap_program: column {c}: expected (op in 0..{REMAP_OPS}, flags, p0, p1, p2, p3), got {e}")
    of = torch.tensor([[int(e[0]), int(e[1])] for e in entries], dtype=torch.int32).reshape(V, 2)
    par = torch.tensor([[float(p) for p in e[2:]] for e in entries], dtype=torch.float32).reshape(V, 4)
    active = torch.tensor([c for c, e in enumerate(entries) if int(e[0]) != 0], dtype=torch.int32)
    return RemapProgram(of.to(device), par.to(device), active.to(device))


def _remap_ptrs(program: Optional[RemapProgram], V: int, what: str) -> tuple[int, int]:
    if program is None:  # a chain without this stage: the null pointer group
        return 0, 0
    of, par, _ = program
    _dev(of, par)
    if of.shape != (V, 2) or of.dtype != torch.int32 or not of.is_contiguous() or par.shape != (V, 4) or par.dtype != torch.float32 or not par.is_contiguous():
        raise ValueError(f"{what}: the remap program must be contiguous int32 [{V}, 2] and fp32 [{V}, 4], got {tuple(of.shape)} {of.dtype}, "
                         f"{tuple(par.shape)} {par.dtype}")
    return of.data_ptr(), par.data_ptr()


def remap_columns(x: Tensor, program: RemapProgram, inverse: bool = False, out: Optional[Tensor] = None, violations: Optional[Tensor] = None) -> Tensor:
    """Remapper.transform / inverse_transform as one kernel: x [batch, time, grid, V] or [batch, time, ensemble, grid, V] (any strides,
    columns contiguous).  ``program``: the tables of ONE direction, or a (forward, inverse) pair from which ``inverse`` picks.  ``out``: x
    itself (in place: only the remapped columns are loaded and stored) or a tensor of x's shape (default: a new one).  ``violations``:
    int32 [V], entry c incremented per element of column c that fails the reference's forward domain assertion (x >= 0 under a power
    without clipping)."""
    if not isinstance(program, RemapProgram):
        program = program[1 if inverse else 0]
    of, par, active = program
    _dev(x, of, par, active, out, violations)
    if x.dim() not in (4, 5) or x.stride(-1) != 1:
        raise ValueError(f"remap_columns: x must be [batch, time, (ensemble,) grid, vars] with contiguous variables, got {tuple(x.shape)}")
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or y.stride(-1) != 1:
        raise ValueError("remap_columns: out must match x")
    x5, y5 = (x.unsqueeze(2), y.unsqueeze(2)) if x.dim() == 4 else (x, y)
    B, T, E, N, V = x5.shape
    _remap_ptrs(program, V, "remap_columns")
    if active.dtype != torch.int32 or active.dim() != 1 or active.shape[0] > V or not active.is_contiguous():
        raise ValueError("remap_columns: program.active must be contiguous int32 [<= V]")
    vp = 0 if violations is None else _vec(violations, "violations", V, torch.int32)
    in_place = y5.data_ptr() == x5.data_ptr() and y5.stride() == x5.stride()
    if not in_place and y5.data_ptr() == x5.data_ptr():
        raise ValueError("remap_columns: out aliases x with other strides")
    if x5.numel() and (active.shape[0] or not in_place):
        ap, na = (active.data_ptr(), active.shape[0]) if in_place else (0, V)
        _lib.check(_lib.load().anemoi_remap_columns(x5.data_ptr(), *x5.stride()[:4], y5.data_ptr(), *y5.stride()[:4], of.data_ptr(), par.data_ptr(), ap, na,
                                                    vp, B, T, E, N, V, _dt(x), _stream()), "remap_columns")
    return y


def column_program_(x: Tensor, op_table: Tensor, param_table: Tensor, *, nan_mask: Optional[Tensor] = None) -> Tensor:
    """In place: the ordered column program of ``bound_columns_`` with the kinds of the post-processors and the remapper's inverse
    (anemoi_column_program: 11 fill where the masking column is 0, 12 NaN where it is NaN, 16 + remap op) over x [..., V].  Columns are
    checked against V when the tables are built (``layers.bounding.extended_program_tables``)."""
    _dev(x, op_table, param_table, nan_mask)
    if not x.is_contiguous():
        raise ValueError("column_program_: x must be contiguous")
    if op_table.dim() != 2 or op_table.shape[1] != 4 or op_table.dtype != torch.int32 or not op_table.is_contiguous() or \
            tuple(param_table.shape) != (op_table.shape[0], 2) or param_table.dtype != torch.float32 or not param_table.is_contiguous():
        raise ValueError("column_program_: the tables must be contiguous int32 [n_ops, 4] and fp32 [n_ops, 2]")
    return _column_program(x, op_table, param_table, nan_mask, 0, True, "column_program_")


def transpose_pad(x: Tensor, mult: int = 64) -> Tensor:
    """[N, C] -> contiguous [C, N_pad] with N_pad = N rounded up to ``mult`` and zeros in the padding."""
    _dev(x)
    n, c = x.shape
    n_pad = (n + mult - 1) // mult * mult
    out = torch.empty((c, n_pad), dtype=x.dtype, device=x.device)
    p, ld = _rows(x, "x")
    _lib.check(_lib.load().anemoi_transpose_pad(p, ld, out.data_ptr(), n_pad, n, c, n_pad, _dt(x), _stream()), "transpose_pad")
    return out


def gather_rows(x: Tensor, idx: Tensor) -> Tensor:
    """out[i] = x[idx[i]] (idx int32).  Differentiable (adjoint: rows summed back by index)."""
    if _needs_grad(x):
        from .autograd import GatherRowsFunction

        return GatherRowsFunction.apply(x, idx)
    return _gather_rows_fwd(x, idx)


def _gather_rows_fwd(x: Tensor, idx: Tensor) -> Tensor:
    _dev(x, idx)
    if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError("idx must be contiguous int32 [n]")
    D = x.shape[1]
    out = torch.empty((idx.shape[0], D), dtype=x.dtype, device=x.device)
    p, ld = _rows(x, "x")
    _lib.check(_lib.load().anemoi_gather_rows(p, ld, idx.data_ptr(), out.data_ptr(), D, idx.shape[0], D, _dt(x), _stream()), "gather_rows")
    return out


# ------------------------------------------------------------------------------------------ reference op mirror
@torch.library.custom_op("anemoi_amd::graph_transformer_attention", mutates_args=(), device_types="cuda")
def graph_transformer_attention(q: Tensor, k: Tensor, v: Tensor, e: Tensor, row: Tensor, colptr: Tensor, rowptr: Tensor,
                                edge_ids: Tensor, edge_dst: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """Same signature and outputs as the reference's ``anemoi::graph_transformer_attention``
    (triton/gt.py:390-428): q [N_dst,H,C], k,v [N_src,H,C], e [M,H,C] in CSC order, int64 row/colptr;
    returns (out in q.dtype, out_saved fp32, m = logsumexp fp32).  rowptr/edge_ids/edge_dst (reverse CSR)
    are only needed by the backward pass and ignored here."""
    N_dst, H, Cc = q.shape
    q2, k2, v2, e2 = (t.contiguous().view(t.shape[0], H * Cc) for t in (q, k, v, e))
    csc = CSC(row=row.to(torch.int32).contiguous(), dst=edge_dst.to(torch.int32).contiguous(),
              colptr=colptr.to(torch.int32).contiguous(), n_src=k.shape[0], n_dst=N_dst)
    if q.dtype != torch.float32:
        # the reference keeps the UNROUNDED fp32 accumulator as out_saved and rounds a copy for the caller (triton/gt.py:416-426): the
        # kernel's fp32 instantiation on the exactly upcast 16-bit operands produces that accumulator (same products, fp32 sums); the
        # module path (layers/block.py) does not come through here - it runs the fused-edge kernel in the model dtype
        saved, m = gt_attention(q2.float(), k2.float(), v2.float(), e2.float(), csc, H, return_lse=True)
        saved = saved.view(N_dst, H, Cc)
        return saved.to(q.dtype), saved, m
    out, m = gt_attention(q2, k2, v2, e2, csc, H, return_lse=True)
    out = out.view(N_dst, H, Cc)
    return out, out.clone(), m


@graph_transformer_attention.register_fake
def _graph_transformer_attention_fake(q, k, v, e, row, colptr, rowptr, edge_ids, edge_dst):
    N_dst, H, Cc = q.shape
    return (torch.empty((N_dst, H, Cc), device=q.device, dtype=q.dtype),
            torch.empty((N_dst, H, Cc), device=q.device, dtype=torch.float32),
            torch.empty((N_dst, H), device=q.device, dtype=torch.float32))


@torch.library.custom_op("anemoi_amd::graph_transformer_attention_backward", mutates_args=(), device_types="cuda")
def graph_transformer_attention_backward(d_out: Tensor, q: Tensor, k: Tensor, v: Tensor, e: Tensor, out_saved: Tensor, m: Tensor,
                                         row: Tensor, colptr: Tensor, rowptr: Tensor, edge_ids: Tensor,
                                         edge_dst: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """Same signature as the reference's ``anemoi::graph_transformer_attention_backward`` (triton/gt.py:447-492):
    returns (dQ, dK, dV, dE) shaped like q, k, v, e.  For 16-bit operands the kernels take ``out_saved`` ROUNDED to the model dtype (the
    reference reads the fp32 accumulator in D = <dO, O>): one rounding of O, inside the stated 16-bit tolerance of the gradient tests
    (tests/test_attention_backward_gpu.py); fp32 operands use it as it is."""
    N_dst, H, Cc = q.shape
    flat = lambda t: t.contiguous().view(t.shape[0], H * Cc)  # noqa: E731
    csc = CSC(row=row.to(torch.int32).contiguous(), dst=edge_dst.to(torch.int32).contiguous(),
              colptr=colptr.to(torch.int32).contiguous(), n_src=k.shape[0], n_dst=N_dst)
    dq, dk, dv, de = gt_attention_backward(flat(d_out).to(q.dtype), flat(q), flat(k), flat(v), flat(e), flat(out_saved).to(q.dtype), m, csc,
                                           (rowptr, edge_ids, edge_dst), H)
    return dq.view_as(q), dk.view_as(k), dv.view_as(v), de.view_as(e)


@graph_transformer_attention_backward.register_fake
def _graph_transformer_attention_backward_fake(d_out, q, k, v, e, out_saved, m, row, colptr, rowptr, edge_ids, edge_dst):
    return torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(e)


def _gta_setup_context(ctx, inputs, output):
    q, k, v, e, row, colptr, rowptr, edge_ids, edge_dst = inputs
    _out, out_saved, m = output
    ctx.save_for_backward(q, k, v, e, out_saved, m, row, colptr, rowptr, edge_ids, edge_dst)


def _gta_backward(ctx, d_out, _d_out_saved, _d_m):
    # only the gradient of the user-facing ``out`` is used (triton/gt.py:526-538)
    q, k, v, e, out_saved, m, row, colptr, rowptr, edge_ids, edge_dst = ctx.saved_tensors
    dq, dk, dv, de = graph_transformer_attention_backward(d_out, q, k, v, e, out_saved, m, row, colptr, rowptr, edge_ids, edge_dst)
    return dq, dk, dv, de, None, None, None, None, None


graph_transformer_attention.register_autograd(_gta_backward, setup_context=_gta_setup_context)


def graph_transformer_attention_conv(query: Tensor, key: Tensor, value: Tensor, edges: Tensor, csc: tuple[Tensor, Tensor],
                                     reverse: tuple[Tensor, Tensor, Tensor]) -> Tensor:
    """Drop-in for the reference's ``graph_transformer_attention_conv`` (triton/gt.py:564-576)."""
    row, colptr = csc
    rowptr, edge_ids, edge_dst = reverse
    out, _saved, _m = graph_transformer_attention(query, key, value, edges, row, colptr, rowptr, edge_ids, edge_dst)
    return out


# ------------------------------------------------------------------------------------------ spherical-harmonic transforms
@dataclass(frozen=True)
class ShtGrid:
    """A grid of latitude rings as the transform kernels want it (csrc/sht.hip): ring offsets int32 [K + 1] and the twiddle table fp32
    [grid, 2] = (cos, -sin)(2 pi t / n_k) at s_k + t, evaluated in float64 and rounded once; both on ``device``."""
    lons_per_lat: tuple
    ring_offsets: Tensor
    twiddles: Tensor

    @property
    def n_rings(self) -> int:
        return len(self.lons_per_lat)

    @property
    def n_grid(self) -> int:
        return int(sum(self.lons_per_lat))

    @property
    def max_ring(self) -> int:
        return int(max(self.lons_per_lat))


_SHT_GRIDS: dict = {}


def sht_twiddles(lons_per_lat) -> "np.ndarray":
    """float64 [grid, 2]: (cos, -sin)(2 pi t / n_k) for t < n_k, ring after ring."""
    import numpy as np

    out = []
    for n in lons_per_lat:
        ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
        out.append(np.stack([np.cos(ang), -np.sin(ang)], axis=1))
    return np.concatenate(out, axis=0)


def sht_grid(lons_per_lat, device) -> ShtGrid:
    """The ShtGrid of ``lons_per_lat`` on ``device``, built once per (grid, device)."""
    import numpy as np

    lons = tuple(int(n) for n in lons_per_lat)
    if not lons or min(lons) <= 0:
        raise ValueError(f"sht_grid: every ring needs at least one point, got {list(lons)[:8]}...")
    key = (lons, str(torch.device(device)))
    hit = _SHT_GRIDS.get(key)
    if hit is None:
        off = np.concatenate([[0], np.cumsum(lons)]).astype(np.int32)
        hit = ShtGrid(lons, torch.from_numpy(off).to(device), torch.from_numpy(sht_twiddles(lons).astype(np.float32)).to(device))
        _SHT_GRIDS[key] = hit
    return hit


def sht_plan(direction: str, n_fields: int, lons_per_lat, truncation: int) -> dict:
    """How ``sht_forward`` / ``sht_inverse`` tile a call (csrc/sht_plan.h) - host only, no GPU.  Raises ValueError where the entry points
    refuse the shape (truncation outside [1, nlat], a ring without points)."""
    lons = [int(n) for n in lons_per_lat]
    arr = (_lib.C.c_int32 * max(len(lons), 1))(*lons)
    plan = _lib.ShtPlan()
    rc = _lib.load().anemoi_sht_plan({"forward": 0, "inverse": 1}[direction], int(n_fields), arr, len(lons), int(truncation), _lib.C.byref(plan))
    _lib.check(rc, "sht_plan")
    return dict(field_tile=plan.field_tile, chunk=plan.chunk, lds_bytes=plan.lds_bytes, lds_bound=plan.lds_bound, ring_threads=plan.ring_threads,
                leg_rows=plan.leg_rows, ring_grid=tuple(plan.ring_grid), leg_grid=tuple(plan.leg_grid), workspace_bytes=plan.workspace_bytes)


def _sht_check(t: Tensor, name: str, dtype) -> None:
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype} (the transforms are fp32 / complex64 only)")


def _sht_table(table: Tensor, grid: ShtGrid, name: str) -> int:
    """L = M of a Legendre table [L, K, M] (fp32, contiguous, on the device)."""
    if table.dim() != 3 or table.shape[0] != table.shape[2] or table.shape[1] != grid.n_rings or table.dtype != torch.float32 or not table.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous fp32 table [L, {grid.n_rings}, L], got {tuple(table.shape)} {table.dtype}")
    return table.shape[0]


def _sht_grid_side(x: Tensor, grid: ShtGrid, cols: Optional[Tensor], columns: bool):
    """(tensor to address, lead shape, n_groups, n_cols, gs, ps) of the grid side of a transform."""
    if columns:
        if x.dim() < 2 or x.shape[-2] != grid.n_grid:
            raise ValueError(f"sht: expected [..., {grid.n_grid}, V], got {tuple(x.shape)}")
        if x.shape[-1] > 1 and x.stride(-1) != 1:
            raise ValueError("sht: the last dimension of x must be contiguous")
        xk = _two_leading(x)
        if xk.shape[0] > 1 and xk.shape[1] > 1:  # leading dimensions that need two strides: one copy (a [B > 1, T, E > 1, ..] step slice)
            xk = xk.contiguous().view(1, -1, *xk.shape[2:])
        G = xk.shape[0] * xk.shape[1]
        V = xk.shape[-1]
        if cols is not None:
            if cols.dtype != torch.int32 or cols.dim() != 1 or not cols.is_contiguous():
                raise ValueError("sht: cols must be a contiguous int32 vector")
        C = V if cols is None else cols.shape[0]
        gs = xk.stride(0) if xk.shape[0] > 1 else (xk.stride(1) if xk.shape[1] > 1 else 0)
        ps = xk.stride(2) if grid.n_grid > 1 else max(V, 1)
        if gs < 0 or ps < max(V, 1):
            raise ValueError("sht: x must have a non-negative group stride and a point stride of at least its width")
        return xk, x.shape[:-2], G, C, gs, ps
    if x.dim() < 1 or x.shape[-1] != grid.n_grid:
        raise ValueError(f"sht: expected [..., {grid.n_grid}], got {tuple(x.shape)}")
    if cols is not None:
        raise ValueError("sht: cols select columns of a [..., grid, V] tensor (columns=True)")
    xk = x.reshape(-1, grid.n_grid)
    xk = xk if xk.is_contiguous() else xk.contiguous()
    return xk, x.shape[:-1], xk.shape[0], 1, grid.n_grid, 1


def sht_forward(x: Tensor, grid: ShtGrid, wleg: Tensor, cols: Optional[Tensor] = None, columns: bool = False) -> Tensor:
    """Spherical-harmonic analysis, two launches (csrc/sht.hip; the reference's SphericalHarmonicTransform.forward,
    layers/spectral_helpers.py:317-340).  x fp32: ``[..., grid]`` fields, or with ``columns=True`` a ``[..., grid, V]`` tensor read IN PLACE
    (any row / leading strides; ``cols`` int32 on the device selects columns whose values the caller has checked to lie in [0, V)).
    wleg: fp32 [L, K, M] (``spectral_helpers.legendre_tables``).  Returns complex64 ``[..., L, M]`` (fields) or ``[..., C, L, M]`` (columns).
    Forward only: the adjoint kernels are not built."""
    _dev(x, grid.ring_offsets, wleg, cols)
    _sht_check(x, "sht_forward: x", torch.float32)
    if _needs_grad(x):
        raise NotImplementedError("sht_forward: the adjoint kernels of the spherical-harmonic transforms are not built; call it under "
                                  "torch.no_grad() or on tensors that do not require grad")
    L = _sht_table(wleg, grid, "sht_forward: wleg")
    xk, lead, G, C, gs, ps = _sht_grid_side(x, grid, cols, columns)
    F = G * C
    coeffs = torch.empty((F, L, L, 2), dtype=torch.float32, device=x.device)
    ws = torch.empty((max(F, 1) * grid.n_rings * L * 2,), dtype=torch.float32, device=x.device)
    rc = _lib.load().anemoi_sht_fwd(xk.data_ptr(), gs, ps, 0 if cols is None else cols.data_ptr(), G, C, grid.ring_offsets.data_ptr(), grid.n_rings,
                                    grid.max_ring, L - 1, grid.twiddles.data_ptr(), wleg.data_ptr(), coeffs.data_ptr(), ws.data_ptr(),
                                    ws.numel() * 4, _stream())
    _lib.check(rc, "sht_fwd")
    out = torch.view_as_complex(coeffs)
    return out.view(*lead, C, L, L) if columns else out.view(*lead, L, L)


def sht_inverse(coeffs: Tensor, grid: ShtGrid, pleg: Tensor, lscale: Optional[Tensor] = None, columns: bool = False,
                out: Optional[Tensor] = None, cols: Optional[Tensor] = None) -> Tensor:
    """Spherical-harmonic synthesis, two launches (the reference's InverseSphericalHarmonicTransform.forward,
    layers/spectral_helpers.py:530-553).  coeffs complex64 ``[..., L, M]``; lscale fp32 [S, L]: field f (flattened leading index) is
    multiplied by lscale[f % S, l] on the way in.  Returns fp32 ``[..., grid]``; with ``columns=True`` coeffs is ``[..., C, L, M]`` and the
    result ``[..., grid, C]`` (point-major) - or, with ``out`` [..., grid, V] (+ ``cols``), written in place into its columns."""
    _dev(coeffs, grid.ring_offsets, pleg, lscale, out, cols)
    _sht_check(coeffs, "sht_inverse: coeffs", torch.complex64)
    if _needs_grad(coeffs, lscale):
        raise NotImplementedError("sht_inverse: the adjoint kernels of the spherical-harmonic transforms are not built; call it under "
                                  "torch.no_grad() or on tensors that do not require grad")
    L = _sht_table(pleg, grid, "sht_inverse: pleg")
    if coeffs.dim() < 2 + int(columns) or tuple(coeffs.shape[-2:]) != (L, L):
        raise ValueError(f"sht_inverse: coefficients {tuple(coeffs.shape)} do not end in [{L}, {L}]")
    c = torch.view_as_real(coeffs if coeffs.is_contiguous() else coeffs.contiguous())
    if lscale is not None and (lscale.dim() != 2 or lscale.shape[1] != L or lscale.dtype != torch.float32 or not lscale.is_contiguous() or lscale.shape[0] < 1):
        raise ValueError(f"sht_inverse: lscale must be contiguous fp32 [S, {L}], got {tuple(lscale.shape)} {lscale.dtype}")
    if columns:
        lead, C = coeffs.shape[:-3], coeffs.shape[-3]
        if out is None:
            if cols is not None:
                raise ValueError("sht_inverse: cols need an out tensor")
            out = torch.empty((*lead, grid.n_grid, C), dtype=torch.float32, device=coeffs.device)
        _sht_check(out, "sht_inverse: out", torch.float32)
        yk, olead, G, Cy, gs, ps = _sht_grid_side(out, grid, cols, True)
        if yk.data_ptr() != out.data_ptr() or Cy != C or G * C != coeffs.numel() // (L * L):
            raise ValueError(f"sht_inverse: out {tuple(out.shape)} does not take the coefficients' {tuple(coeffs.shape[:-2])} fields in place")
    else:
        if out is not None or cols is not None:
            raise ValueError("sht_inverse: out / cols address a [..., grid, V] tensor (columns=True)")
        lead = coeffs.shape[:-2]
        out = torch.empty((*lead, grid.n_grid), dtype=torch.float32, device=coeffs.device)
        G, C, gs, ps = coeffs.numel() // (L * L), 1, grid.n_grid, 1
    F = G * C
    ws = torch.empty((max(F, 1) * grid.n_rings * L * 2,), dtype=torch.float32, device=coeffs.device)
    rc = _lib.load().anemoi_sht_inv(c.data_ptr(), 0 if lscale is None else lscale.data_ptr(), 1 if lscale is None else lscale.shape[0],
                                    grid.ring_offsets.data_ptr(), grid.n_rings, grid.max_ring, L - 1, grid.twiddles.data_ptr(), pleg.data_ptr(),
                                    out.data_ptr(), gs, ps, 0 if cols is None else cols.data_ptr(), G, C, ws.data_ptr(), ws.numel() * 4, _stream())
    _lib.check(rc, "sht_inv")
    return out


def ornstein_combine(x_last: Tensor, prog_cols: Tensor, fields: Tensor, reg_cols: Optional[Tensor] = None, trunc_map: Optional[Tensor] = None,
                     lowpass: Optional[Tensor] = None, walias: Optional[Tensor] = None, write_back: bool = False) -> Tensor:
    """The spectral Ornstein residual's row-wise step, one launch (anemoi_ornstein_combine_fwd; the reference's
    SpectralOrnsteinConnection._learnable, layers/residual.py:565-576):
    out[..., p, c] = gain[p, c] xt + mu[p, c] + sum_i beta_i[p, c] x[..., p, reg_cols[i]] with fields = [gain, mu, beta_0, ..] fp32
    [2 + R, grid, n_prog]; xt = x[..., p, prog_cols[c]], or for columns with trunc_map[c] = t >= 0 the low-pass field lowpass[..., p, t],
    blended with x by walias[p, t] when given.  x_last [..., grid, V] fp32 is read in place.  Returns the compact skip [..., grid, n_prog].
    The column vectors are int32 on the device; the caller has checked that they lie inside x's columns.  ``write_back``: xt is also
    written into the truncated columns of x_last itself (what the reference's residual leaves in its caller's input); the caller has
    checked that no regressor is a truncated column."""
    _dev(x_last, prog_cols, fields, reg_cols, trunc_map, lowpass, walias)
    _sht_check(x_last, "ornstein_combine: x", torch.float32)
    if _needs_grad(x_last, fields, lowpass, walias):
        raise NotImplementedError("ornstein_combine: the backward kernel is not built; call it under torch.no_grad()")
    n_grid, n_prog = x_last.shape[-2], prog_cols.shape[0]
    R = 0 if reg_cols is None else reg_cols.shape[0]
    if tuple(fields.shape) != (2 + R, n_grid, n_prog) or fields.dtype != torch.float32 or not fields.is_contiguous():
        raise ValueError(f"ornstein_combine: fields must be contiguous fp32 [{2 + R}, {n_grid}, {n_prog}], got {tuple(fields.shape)}")
    if x_last.shape[-1] > 1 and x_last.stride(-1) != 1:
        raise ValueError("ornstein_combine: the last dimension of x must be contiguous")
    xk = _two_leading(x_last)
    if xk.shape[0] > 1 and xk.shape[1] > 1:
        xk = xk.contiguous().view(1, -1, *xk.shape[2:])
    G = xk.shape[0] * xk.shape[1]
    gs = 0 if G <= 1 else (xk.stride(0) if xk.shape[0] > 1 else xk.stride(1))
    ps = xk.stride(2) if n_grid > 1 else max(xk.shape[-1], 1)
    n_trunc = 0
    if trunc_map is not None:
        if lowpass is None:
            raise ValueError("ornstein_combine: trunc_map needs the low-pass fields")
        n_trunc = lowpass.shape[-1]
        if lowpass.numel() != G * n_grid * n_trunc or lowpass.dtype != torch.float32 or not lowpass.is_contiguous():
            raise ValueError(f"ornstein_combine: lowpass must be contiguous fp32 [.., {n_grid}, T] over x's {G} leading entries, got {tuple(lowpass.shape)}")
        if walias is not None and (tuple(walias.shape) != (n_grid, n_trunc) or walias.dtype != torch.float32 or not walias.is_contiguous()):
            raise ValueError(f"ornstein_combine: walias must be contiguous fp32 [{n_grid}, {n_trunc}]")
    elif lowpass is not None or walias is not None or write_back:
        raise ValueError("ornstein_combine: lowpass / walias / write_back need a trunc_map")
    if write_back and xk.data_ptr() != x_last.data_ptr():
        raise ValueError("ornstein_combine: write_back needs an input whose leading dimensions are addressed in place")
    out = torch.empty((*x_last.shape[:-2], n_grid, n_prog), dtype=torch.float32, device=x_last.device)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    rc = _lib.load().anemoi_ornstein_combine_fwd(xk.data_ptr(), gs, ps, _vec(prog_cols, "prog_cols", n_prog, torch.int32), _vec(reg_cols, "reg_cols", R, torch.int32),
                                                 R, fields.data_ptr(), _vec(trunc_map, "trunc_map", n_prog, torch.int32), ptr(lowpass), n_trunc, ptr(walias),
                                                 xk.data_ptr() if write_back else 0, out.data_ptr(), G, n_grid, n_prog, _stream())
    _lib.check(rc, "ornstein_combine_fwd")
    return out


# ---------------------------------------------------------------------------------------------- EDM diffusion (csrc/transport.hip)
NOISE_CHANNELS_MAX, NOISE_COND_MAX = 64, 32  # widths anemoi_noise_cond_fwd takes (csrc/transport.hip)
HEUN_PREDICT, HEUN_CORRECT, HEUN_FINAL, DPMPP_FIRST, DPMPP_MULTI, DPMPP_FINAL = range(6)  # modes of edm_update_
_REAL = {torch.float32: 0, torch.float64: 1}


def _real(t: Tensor, what: str) -> int:
    try:
        return _REAL[t.dtype]
    except KeyError:
        raise ValueError(f"{what}: float32 or float64, got {t.dtype}") from None


def _state5(t: Tensor, what: str) -> tuple:
    """Element strides (batch, time, ensemble, grid) of a [B, T, E, N, V] tensor read in place; the last dimension is contiguous."""
    if t.dim() != 5 or (t.shape[-1] > 1 and t.stride(-1) != 1):
        raise ValueError(f"{what}: [batch, time, ensemble, grid, vars] with a contiguous last dimension, got {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0), t.stride(1), t.stride(2), t.stride(3)


def noise_cond(values: Tensor, frequencies: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, *, pi: Optional[Tensor] = None,
               log_quarter: bool = False, rows: tuple = (1,), out_dtype=None) -> tuple:
    """The conditioning rows of one denoiser call, one launch (anemoi_noise_cond_fwd): values [G] (fp32 / fp64, cast to fp32), optionally
    log(v) / 4 (the EDM c_noise), the sin | cos embedding over ``frequencies`` [C / 2] fp32 (times 2 pi[0] when ``pi`` is given), the
    two Linear maps with SiLU between them, and the result [G, cond_dim] repeated ``rows[k]`` times per group into up to two outputs
    [G rows[k], cond_dim] in ``out_dtype`` (default: the weights').  Returns one tensor per entry of ``rows`` (None for a 0 entry).
    Differentiable in the four parameters (``autograd.NoiseCondFunction``: anemoi_noise_cond_bwd); not in ``values``."""
    _dev(values, frequencies, w1, b1, w2, b2, pi)
    if _needs_grad(values):
        raise NotImplementedError("noise_cond: a gradient with respect to values (the noise level) is not built; detach it")
    if _needs_grad(w1, b1, w2, b2):
        from .autograd import NoiseCondFunction

        return NoiseCondFunction.apply(values, frequencies, pi, log_quarter, tuple(rows), out_dtype, w1, b1, w2, b2)
    return _noise_cond_fwd(values, frequencies, w1, b1, w2, b2, pi=pi, log_quarter=log_quarter, rows=rows, out_dtype=out_dtype)


def _noise_cond_operands(values: Tensor, frequencies: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, pi: Optional[Tensor]) -> tuple:
    """The checked, contiguous operands of the noise-conditioning kernels and (C, cond_dim, G)."""
    C, cond_dim, G = w1.shape[0], w2.shape[0], values.numel()
    if tuple(w1.shape) != (C, C) or tuple(w2.shape) != (cond_dim, C) or b1.numel() != C or b2.numel() != cond_dim or frequencies.numel() * 2 != C:
        raise ValueError(f"noise_cond: w1 [C, C], b1 [C], w2 [cond, C], b2 [cond], frequencies [C / 2]; got {tuple(w1.shape)}, {tuple(b1.shape)}, "
                         f"{tuple(w2.shape)}, {tuple(b2.shape)}, {tuple(frequencies.shape)}")
    if frequencies.dtype != torch.float32 or (pi is not None and pi.dtype != torch.float32):
        raise ValueError("noise_cond: frequencies and pi are fp32")
    if not (w1.dtype == b1.dtype == w2.dtype == b2.dtype):
        raise ValueError("noise_cond: the four parameters share one dtype")
    return (values.reshape(-1).contiguous(), frequencies.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()), (C, cond_dim, G)


def _noise_cond_fwd(values: Tensor, frequencies: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, *, pi: Optional[Tensor] = None,
                    log_quarter: bool = False, rows: tuple = (1,), out_dtype=None) -> tuple:
    (values, frequencies, w1, b1, w2, b2), (C, cond_dim, G) = _noise_cond_operands(values, frequencies, w1, b1, w2, b2, pi)
    if not 1 <= len(rows) <= 2:
        raise ValueError("noise_cond: one or two destinations")
    out_dtype = out_dtype or w1.dtype
    outs = [None if r == 0 else torch.empty((G * r, cond_dim), dtype=out_dtype, device=values.device) for r in rows]
    dst = [(0, 0, 0) if o is None else (o.data_ptr(), r, cond_dim) for o, r in zip(outs, rows)] + [(0, 0, 0)] * (2 - len(rows))
    rc = _lib.load().anemoi_noise_cond_fwd(values.data_ptr(), _real(values, "noise_cond: values"), 1 if log_quarter else 0, frequencies.data_ptr(),
                                           0 if pi is None else pi.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), _dt(w1),
                                           *dst[0], *dst[1], G, C, cond_dim, _DT[out_dtype], _stream())
    _lib.check(rc, "noise_cond_fwd")
    return tuple(outs)


def noise_cond_backward(d_outs: tuple, rows: tuple, values: Tensor, frequencies: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, *,
                        pi: Optional[Tensor] = None, log_quarter: bool = False) -> tuple:
    """(d_w1, d_b1, d_w2, d_b2) in fp32 from the gradients ``d_outs[k]`` [G rows[k], cond_dim] (row-major, any leading dimension; None: absent)
    of ``noise_cond``'s outputs, two launches (anemoi_noise_cond_bwd): deterministic - fixed-order fp32 sums, no atomics."""
    _dev(values, frequencies, w1, b1, w2, b2, pi, *d_outs)
    (values, frequencies, w1, b1, w2, b2), (C, cond_dim, G) = _noise_cond_operands(values, frequencies, w1, b1, w2, b2, pi)
    if not 1 <= len(d_outs) <= 2 or len(d_outs) != len(rows):
        raise ValueError("noise_cond_backward: one gradient (or None) per destination, one or two destinations")
    present = [d for d in d_outs if d is not None]
    dtype = present[0].dtype if present else w1.dtype
    src = []
    for d, r in zip(d_outs, rows):
        if d is None or r == 0 or G == 0:
            src.append((0, 0, 0))
            continue
        if d.dim() != 2 or tuple(d.shape) != (G * r, cond_dim) or (cond_dim > 1 and d.stride(1) != 1) or d.dtype != dtype or (
                d.shape[0] > 1 and d.stride(0) < cond_dim):
            raise ValueError(f"noise_cond_backward: gradient [{G * r}, {cond_dim}] row-major in {dtype}, got {tuple(d.shape)} strides {d.stride()} {d.dtype}")
        src.append((d.data_ptr(), r, d.stride(0) if d.shape[0] > 1 else cond_dim))
    src += [(0, 0, 0)] * (2 - len(src))
    lib = _lib.load()
    ws_bytes = lib.anemoi_noise_cond_bwd_workspace_bytes(src[0][1], src[1][1], G, cond_dim)
    ws = torch.empty((max(ws_bytes // 4, 1),), dtype=torch.float32, device=values.device)
    grads = torch.empty((C * C + C + cond_dim * C + cond_dim,), dtype=torch.float32, device=values.device)
    d_w1, d_b1, d_w2, d_b2 = grads[:C * C].view(C, C), grads[C * C:C * C + C], grads[C * C + C:C * C + C + cond_dim * C].view(cond_dim, C), grads[C * C + C + cond_dim * C:]
    rc = lib.anemoi_noise_cond_bwd(*src[0], *src[1], _DT[dtype], values.data_ptr(), _real(values, "noise_cond: values"), 1 if log_quarter else 0,
                                   frequencies.data_ptr(), 0 if pi is None else pi.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                   _dt(w1), d_w1.data_ptr(), d_b1.data_ptr(), d_w2.data_ptr(), d_b2.data_ptr(), ws.data_ptr(), ws.numel() * 4, G, C, cond_dim,
                                   _stream())
    _lib.check(rc, "noise_cond_bwd")
    return d_w1, d_b1, d_w2, d_b2


def transport_assemble_input(x: Tensor, y: Tensor, attrs: Optional[Tensor], width: int, *, sigma: Optional[Tensor] = None, sigma_data: float = 1.0,
                             out_dtype=None, out: Optional[Tensor] = None) -> Tensor:
    """The denoiser network's input rows, one launch (anemoi_transport_assemble_input):
    out[(b e n), :] = [x[b, t, e, n, :] | c_in[b, e] float(y[b, t, e, n, :]) | attrs[n, :] | zeros up to ``width``], c_in = 1 / sqrt(sigma_data^2
    + sigma^2) in fp32 from the device ``sigma`` [B E] (None: no scale).  x fp32 and y fp32 / fp64 are read in place through their strides.
    ``out``: a [B E N, >= width] row-major tensor to write into (its columns beyond ``width`` stay untouched).
    Differentiable in ``attrs`` (``autograd.TransportAssembleInputFunction``: anemoi_transport_assemble_input_bwd); not in x, y or sigma."""
    _dev(x, y, attrs, sigma, out)
    for name, t in (("x", x), ("y", y), ("sigma", sigma)):
        if _needs_grad(t):
            raise NotImplementedError(f"transport_assemble_input: a gradient with respect to {name} is not built; detach it")
    if _needs_grad(attrs):
        if out is not None:
            raise ValueError("transport_assemble_input: out= is an inference-only argument")
        from .autograd import TransportAssembleInputFunction

        return TransportAssembleInputFunction.apply(x, y, attrs, width, sigma, float(sigma_data), out_dtype)
    return _transport_assemble_input_fwd(x, y, attrs, width, sigma=sigma, sigma_data=sigma_data, out_dtype=out_dtype, out=out)


def _transport_assemble_input_fwd(x: Tensor, y: Tensor, attrs: Optional[Tensor], width: int, *, sigma: Optional[Tensor] = None, sigma_data: float = 1.0,
                                  out_dtype=None, out: Optional[Tensor] = None) -> Tensor:
    if x.dtype != torch.float32:
        raise NotImplementedError(f"transport_assemble_input: the data dtype is float32, got {x.dtype}")
    xs, ys = _state5(x, "transport_assemble_input: x"), _state5(y, "transport_assemble_input: y")
    B, T_in, E, N, V_in = x.shape
    T_out, V_out = y.shape[1], y.shape[4]
    if (y.shape[0], y.shape[2], y.shape[3]) != (B, E, N):
        raise ValueError(f"transport_assemble_input: x {tuple(x.shape)} and y {tuple(y.shape)} differ in batch, ensemble or grid")
    A = 0 if attrs is None else attrs.shape[1]
    if attrs is not None and (attrs.dim() != 2 or attrs.shape[0] != N or attrs.stride(1) != 1):
        raise ValueError(f"transport_assemble_input: attrs [{N}, A] row-major, got {tuple(attrs.shape)}")
    if sigma is not None and sigma.numel() != B * E:
        raise ValueError(f"transport_assemble_input: sigma has {sigma.numel()} values for {B * E} groups")
    if out is None:
        out = torch.empty((B * E * N, width), dtype=out_dtype or (attrs.dtype if attrs is not None else x.dtype), device=x.device)
    elif out.dim() != 2 or out.shape[0] != B * E * N or out.shape[1] < width or out.stride(1) != 1:
        raise ValueError(f"transport_assemble_input: out [{B * E * N}, >= {width}] row-major, got {tuple(out.shape)}")
    if attrs is not None and attrs.dtype != out.dtype:
        raise ValueError(f"transport_assemble_input: attrs {attrs.dtype} and out {out.dtype} are both the model dtype")
    sig = None if sigma is None else sigma.reshape(-1).contiguous()
    rc = _lib.load().anemoi_transport_assemble_input(x.data_ptr(), *xs, y.data_ptr(), _real(y, "transport_assemble_input: y"), *ys,
                                                     0 if sig is None else sig.data_ptr(), 0 if sig is None else _real(sig, "transport_assemble_input: sigma"),
                                                     float(sigma_data), 0 if sig is None else 1, 0 if attrs is None else attrs.data_ptr(),
                                                     0 if attrs is None else attrs.stride(0), A, out.data_ptr(), out.stride(0), width, B, E, N, T_in, V_in,
                                                     T_out, V_out, _dt(out), _stream())
    _lib.check(rc, "transport_assemble_input")
    return out


def transport_assemble_input_backward(d_rows: Tensor, col0: int, n_nodes: int, n_attrs: int) -> Tensor:
    """d_attrs [N, A] (d_rows' dtype) = the sum over the groups of columns col0 .. col0 + A - 1 of d_rows [G N, >= col0 + A], one launch
    (anemoi_transport_assemble_input_bwd): groups in order, fp32 accumulation."""
    _dev(d_rows)
    if d_rows.dim() != 2 or n_nodes <= 0 or d_rows.shape[0] % n_nodes or d_rows.shape[1] < col0 + n_attrs or (d_rows.shape[1] > 1 and d_rows.stride(1) != 1):
        raise ValueError(f"transport_assemble_input_backward: d_rows [G {n_nodes}, >= {col0 + n_attrs}] row-major, got {tuple(d_rows.shape)}")
    G = d_rows.shape[0] // n_nodes
    d_attrs = torch.empty((n_nodes, n_attrs), dtype=d_rows.dtype, device=d_rows.device)
    rc = _lib.load().anemoi_transport_assemble_input_bwd(d_rows.data_ptr(), d_rows.stride(0) if d_rows.shape[0] > 1 else d_rows.shape[1], col0,
                                                         d_attrs.data_ptr(), n_attrs, G, n_nodes, n_attrs, _dt(d_rows), _stream())
    _lib.check(rc, "transport_assemble_input_bwd")
    return d_attrs


def edm_output(pred: Tensor, y: Optional[Tensor], sigma: Optional[Tensor], shape: tuple, *, sigma_data: float = 1.0, out_dtype=torch.float32,
               out: Optional[Tensor] = None) -> Tensor:
    """The denoised state from the network's output rows, one launch (anemoi_edm_output): with ``shape`` = (B, T_out, E, N, V_out),
    out[b, t, e, n, v] = c_skip float(y[b, t, e, n, v]) + c_out pred[(b e n), t V_out + v] with the fp32 EDM coefficients of the device
    ``sigma`` [B E]; y and sigma None: "(batch ensemble grid) (time vars) -> batch time ensemble grid vars" and the cast alone.  The result
    is float32 or float64 (``out_dtype``, or the contiguous ``out``).
    Differentiable in ``pred`` (``autograd.EdmOutputFunction``: anemoi_edm_output_bwd); not in y or sigma."""
    _dev(pred, y, sigma, out)
    for name, t in (("y", y), ("sigma", sigma)):
        if _needs_grad(t):
            raise NotImplementedError(f"edm_output: a gradient with respect to {name} is not built; detach it")
    if _needs_grad(pred):
        if out is not None:
            raise ValueError("edm_output: out= is an inference-only argument")
        from .autograd import EdmOutputFunction

        return EdmOutputFunction.apply(pred, y, sigma, tuple(shape), float(sigma_data), out_dtype)
    return _edm_output_fwd(pred, y, sigma, shape, sigma_data=sigma_data, out_dtype=out_dtype, out=out)


def _edm_output_fwd(pred: Tensor, y: Optional[Tensor], sigma: Optional[Tensor], shape: tuple, *, sigma_data: float = 1.0, out_dtype=torch.float32,
                    out: Optional[Tensor] = None) -> Tensor:
    B, T_out, E, N, V_out = shape
    if pred.dim() != 2 or pred.shape[0] != B * E * N or pred.shape[1] < T_out * V_out or pred.stride(1) != 1:
        raise ValueError(f"edm_output: pred [{B * E * N}, >= {T_out * V_out}] row-major, got {tuple(pred.shape)}")
    if (y is None) != (sigma is None):
        raise ValueError("edm_output: y and sigma go together")
    ys = (0, 0, 0, 0)
    if y is not None:
        if tuple(y.shape) != tuple(shape) or sigma.numel() != B * E:
            raise ValueError(f"edm_output: y {tuple(y.shape)} against {tuple(shape)}, sigma {sigma.numel()} values for {B * E} groups")
        ys = _state5(y, "edm_output: y")
        sigma = sigma.reshape(-1).contiguous()
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=pred.device)
    elif tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"edm_output: out is contiguous {tuple(shape)}, got {tuple(out.shape)}")
    rc = _lib.load().anemoi_edm_output(pred.data_ptr(), pred.stride(0), _dt(pred), 0 if y is None else y.data_ptr(), 0 if y is None else _real(y, "edm_output: y"),
                                       *ys, 0 if sigma is None else sigma.data_ptr(), 0 if sigma is None else _real(sigma, "edm_output: sigma"),
                                       float(sigma_data), 0 if y is None else 1, out.data_ptr(), _real(out, "edm_output: out"), B, E, N, T_out, V_out,
                                       _stream())
    _lib.check(rc, "edm_output")
    return out


def edm_output_backward(d_out: Tensor, sigma: Optional[Tensor], pred_shape: tuple, pred_dtype, *, sigma_data: float = 1.0,
                        out: Optional[Tensor] = None) -> Tensor:
    """d_pred [B E N, P] in ``pred_dtype`` from d_out [B, T_out, E, N, V_out] (fp32 / fp64, read in place through its five strides - an
    expanded gradient has zeros among them), one launch (anemoi_edm_output_bwd): c_out d_out in the first T_out V_out columns (``sigma``
    None: d_out itself), zeros in the rest.  ``out``: a row-major [B E N, P] tensor in ``pred_dtype`` to write into."""
    _dev(d_out, sigma, out)
    if d_out.dim() != 5 or any(st < 0 for st in d_out.stride()):
        raise ValueError(f"edm_output_backward: d_out [batch, time, ensemble, grid, vars], got {tuple(d_out.shape)} strides {d_out.stride()}")
    B, T_out, E, N, V_out = d_out.shape
    rows, P = pred_shape
    if rows != B * E * N or P < T_out * V_out:
        raise ValueError(f"edm_output_backward: pred [{B * E * N}, >= {T_out * V_out}], got {tuple(pred_shape)}")
    if sigma is not None:
        if sigma.numel() != B * E:
            raise ValueError(f"edm_output_backward: sigma has {sigma.numel()} values for {B * E} groups")
        sigma = sigma.reshape(-1).contiguous()
    if out is None:
        out = torch.empty((rows, P), dtype=pred_dtype, device=d_out.device)
    elif tuple(out.shape) != (rows, P) or out.dtype != pred_dtype or (P > 1 and out.stride(1) != 1) or (rows > 1 and out.stride(0) < P):
        raise ValueError(f"edm_output_backward: out is row-major [{rows}, {P}] in {pred_dtype}, got {tuple(out.shape)} {out.dtype}")
    d_pred = out
    rc = _lib.load().anemoi_edm_output_bwd(d_out.data_ptr(), _real(d_out, "edm_output_backward: d_out"), *d_out.stride(),
                                           0 if sigma is None else sigma.data_ptr(), 0 if sigma is None else _real(sigma, "edm_output: sigma"),
                                           float(sigma_data), 0 if sigma is None else 1, d_pred.data_ptr(), d_pred.stride(0) if rows > 1 else P, P, _DT[pred_dtype],
                                           B, E, N, T_out, V_out,
                                           _stream())
    _lib.check(rc, "edm_output_bwd")
    return d_pred


def edm_update_(mode: int, params: Tensor, y: Tensor, D: Tensor, aux1: Optional[Tensor] = None, aux2: Optional[Tensor] = None) -> Tensor:
    """The solver arithmetic of one sampler step, in place, one launch (anemoi_edm_update; the modes and the layout of the 8 fp64 device
    ``params`` are those of include/anemoi_hip.h).  y, D, aux1 (d1 | D_old), aux2 (y_next): contiguous tensors of one shape in the solver
    dtype (float32 / float64).  Returns y."""
    _dev(params, y, D, aux1, aux2)
    if params.dtype != torch.float64 or params.numel() != 8 or not params.is_contiguous():
        raise ValueError("edm_update_: params is 8 contiguous float64 values on the device")
    for name, t in (("y", y), ("D", D), ("aux1", aux1), ("aux2", aux2)):
        if t is not None and (t.dtype != y.dtype or t.shape != y.shape or not t.is_contiguous()):
            raise ValueError(f"edm_update_: {name} is a contiguous {y.dtype} tensor of shape {tuple(y.shape)}, got {t.dtype} {tuple(t.shape)}")
    if _needs_grad(y, D, aux1, aux2):
        raise NotImplementedError("edm_update_: differentiating through the sampler is not built; call it under torch.no_grad()")
    rc = _lib.load().anemoi_edm_update(int(mode), params.data_ptr(), y.data_ptr(), D.data_ptr(), 0 if aux1 is None else aux1.data_ptr(),
                                       0 if aux2 is None else aux2.data_ptr(), y.numel(), _real(y, "edm_update_: y"), _stream())
    _lib.check(rc, "edm_update")
    return y
