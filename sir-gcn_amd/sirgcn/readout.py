"""Native graph readout on MI355X: drop-ins for ``dgl.nn.SumPooling`` / ``AvgPooling`` / ``MaxPooling`` and
``dgl.broadcast_nodes`` — the last step of every graph-level model of the reference
(``ogbg-molhiv/model.py:69,85``, ``zinc/model.py:41``, ``super-pixel/model.py:28``,
``hetero-edge-count/model.py:23,33``).

    self.pool = sirgcn.SumPooling()          # for dgl.nn.SumPooling()
    hg = self.pool(graph, h)                 # [V, ...] -> [B, ...]

``graph`` is a batched graph (``sirgcn.batch([...])``, a ``sirgcn.Graph`` with ``batch_num_nodes``, a DGLGraph
or anything with ``batch_num_nodes()``); graph b owns the node rows ``[off[b], off[b+1])`` with
``off = graph.node_offsets`` (cached per device, as for GraphNorm).  One native kernel per direction
(``sir_graph_pool_fwd`` / ``sir_graph_pool_bwd``): sums in node order, no atomics, no ``[V]`` index tensor,
no host synchronisation.  Semantics (DGL's ``segment_reduce``): an empty graph gives 0, the mean divides by
``max(n, 1)``, the maximum's gradient goes to the lowest node id among ties.  CUDA fp32 / bf16 / fp16 run the
kernels (fp32 accumulation, one rounding); any other CUDA dtype runs a torch composition with the same
semantics.  No CPU fallback.
"""
import math

import torch
from torch import nn

from . import _native
from .graph import node_offsets

_OPS = {"sum": _native.POOL_SUM, "mean": _native.POOL_MEAN, "max": _native.POOL_MAX}


def _rows(t, F):
    """``t`` [M, F] with unit-stride rows at least F apart (a column slice of a wider tensor stays a view)."""
    if t.stride(1) == 1 and t.stride(0) >= F:
        return t
    M = t.shape[0]
    if (F > 1 and t.stride(1) != 1) or (M > 1 and t.stride(0) < F):
        t = t.contiguous()
    if t.stride(1) != 1 or t.stride(0) < F:       # strides of size-1 dimensions are free: normalise them
        t = t.as_strided((M, F), (t.stride(0) if M > 1 else F, 1))
    return t


class GraphPoolFunction(torch.autograd.Function):
    """P = pool(X) over the graphs (``sir_graph_pool_fwd``) and its backward (``sir_graph_pool_bwd``).  Keeps
    ``off`` and, for max, the int32 ``arg`` [B, F] only (nothing of [V, F] size)."""

    # off (the graph's cached offsets) and arg (made here, never returned) ride on ctx itself: neither is
    # an output or needs a gradient, and the launch-bound step saves the saved-tensor round trip

    @staticmethod
    def forward(ctx, X, off, op):
        V, F = X.shape
        B = off.shape[0] - 1
        X = _rows(X, F)
        P = torch.empty((B, F), device=X.device, dtype=X.dtype)
        arg = torch.empty((B, F), device=X.device, dtype=torch.int32) if op == _native.POOL_MAX else None
        if B > 0:
            _native.graph_pool_fwd(off, X, op, P, arg)
        ctx.cfg = (off, arg, op, V)
        return P

    @staticmethod
    def backward(ctx, dP):
        off, arg, op, V = ctx.cfg
        F = dP.shape[1]
        dP = _rows(dP, F)
        dX = torch.empty((V, F), device=dP.device, dtype=dP.dtype)
        if V > 0:
            _native.graph_pool_bwd(off, dP, op, dX, arg)
        return dX, None, None


class BroadcastNodesFunction(torch.autograd.Function):
    """out[v] = gfeat[b(v)] (``sir_graph_pool_bwd`` of SUM); backward: the per-graph sum
    (``sir_graph_pool_fwd`` of SUM).  Keeps ``off`` only."""

    @staticmethod
    def forward(ctx, G, off, V):
        B, F = G.shape
        G = _rows(G, F)
        out = torch.empty((V, F), device=G.device, dtype=G.dtype)
        if V > 0:
            _native.graph_pool_bwd(off, G, _native.POOL_SUM, out)
        ctx.off = off
        return out

    @staticmethod
    def backward(ctx, dOut):
        off = ctx.off
        V, F = dOut.shape
        B = off.shape[0] - 1
        dOut = _rows(dOut, F)
        dG = torch.empty((B, F), device=dOut.device, dtype=dOut.dtype)
        if B > 0:
            _native.graph_pool_fwd(off, dOut, _native.POOL_SUM, dG)
        return dG, None, None


def _graph_ids(off, V):
    n = off[1:] - off[:-1]
    return torch.repeat_interleave(torch.arange(n.numel(), device=off.device), n, output_size=V), n


def _composed_pool(X, off, op):
    """The same readout from torch ops (CUDA dtypes the kernels do not take): empty graph -> 0, mean
    clamps n to 1, max routes its gradient to the lowest row among ties."""
    V, F = X.shape
    B = off.numel() - 1
    if V == 0 or B == 0:
        return X.new_zeros((B, F)) + X.sum() * 0
    ids, n = _graph_ids(off, V)
    if op != _native.POOL_MAX:
        P = X.new_zeros((B, F)).index_add_(0, ids, X)
        return P / n.clamp(min=1).to(X.dtype)[:, None] if op == _native.POOL_MEAN else P
    idx = ids[:, None].expand(V, F)
    Xd = X.detach()
    mx = Xd.new_zeros((B, F)).scatter_reduce(0, idx, Xd, "amax", include_self=False)
    rel = torch.arange(V, device=X.device) - off[ids]
    cand = torch.where(Xd == mx[ids], rel[:, None], V)
    arg = torch.full((B, F), V, device=X.device, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    some = (n > 0)[:, None]
    rows = torch.where(some, (off[:-1, None] + arg).clamp(max=V - 1), 0)
    return torch.where(some, X.gather(0, rows), 0)


def _check(graph, feat, rows, what):
    """``feat`` with ``rows`` leading rows on a ROCm GPU (the row count is checked first)."""
    if feat.dim() < 1 or feat.shape[0] != rows:
        raise ValueError(f"sirgcn.{what}: feat of shape {tuple(feat.shape)}, the graph needs {rows} leading rows")
    if not feat.is_cuda:
        raise RuntimeError(f"sirgcn.{what} needs a ROCm GPU tensor (no CPU fallback)")


def _num_nodes(graph):
    if hasattr(graph, "num_nodes"):
        return int(graph.num_nodes())
    return int(torch.as_tensor(graph.batch_num_nodes()).sum())


def _batch_size(graph):
    return int(torch.as_tensor(graph.batch_num_nodes()).numel())


def readout_nodes(graph, feat, op="sum"):
    """``dgl.readout_nodes`` on a feature tensor: ``[V, ...] -> [B, ...]`` with ``op`` 'sum', 'mean' or 'max'."""
    if op not in _OPS:
        raise ValueError(f"sirgcn.readout_nodes: op must be 'sum', 'mean' or 'max', got {op!r}")
    V = _num_nodes(graph)
    _check(graph, feat, V, "readout_nodes")
    off = node_offsets(graph, feat.device)
    pool = GraphPoolFunction.apply if feat.dtype in _native.STORAGE else _composed_pool
    if feat.dim() == 2 and feat.shape[1] > 0:
        return pool(feat, off, _OPS[op])
    B = off.shape[0] - 1
    tail = tuple(feat.shape[1:])
    F = math.prod(tail)
    if F == 0:
        return feat.new_zeros((B,) + tail)
    return pool(feat.reshape(V, F), off, _OPS[op]).reshape((B,) + tail)


def broadcast_nodes(graph, gfeat):
    """``dgl.broadcast_nodes``: ``[B, ...] -> [V, ...]``, ``out[v] = gfeat[b(v)]``."""
    B = _batch_size(graph)
    _check(graph, gfeat, B, "broadcast_nodes")
    V = _num_nodes(graph)
    off = node_offsets(graph, gfeat.device)
    tail = tuple(gfeat.shape[1:])
    F = math.prod(tail)
    if F == 0:
        return gfeat.new_zeros((V,) + tail)
    G = gfeat if gfeat.dim() == 2 else gfeat.reshape(B, F)
    if gfeat.dtype in _native.STORAGE:
        out = BroadcastNodesFunction.apply(G, off, V)
    else:
        out = G[_graph_ids(off, V)[0]]
    return out if gfeat.dim() == 2 else out.reshape((V,) + tail)


class SumPooling(nn.Module):
    """``dgl.nn.SumPooling``: ``forward(graph, feat)``, the per-graph sum of the node features."""

    def forward(self, graph, feat):
        return readout_nodes(graph, feat, "sum")


class AvgPooling(nn.Module):
    """``dgl.nn.AvgPooling``: the per-graph mean (an empty graph gives 0)."""

    def forward(self, graph, feat):
        return readout_nodes(graph, feat, "mean")


class MaxPooling(nn.Module):
    """``dgl.nn.MaxPooling``: the per-graph maximum; its gradient goes to the lowest node id among ties."""

    def forward(self, graph, feat):
        return readout_nodes(graph, feat, "max")
