"""DropEdge — the reference's per-layer edge dropout (``dgl.transforms.DropEdge`` behind the wrapper at
``models/utils.py:96-102``; ``graphs_, efeats_ = self.edge_drop(graphs, efeats)`` in ``zinc/model.py:50``,
``graph_ = self.edge_drop(graph)`` in ``ogbn-arxiv/model.py:146``) without a plan rebuild.

A dropped graph is not a new graph: both of its row CSRs are order-preserving subsequences of the parent's,
which :func:`~sirgcn.graph.get_plan` has already sorted and cached.  :func:`drop_edges` hands the parent's
plan and a keep bit per edge id to ``sir_plan_drop_edges`` (a flag, one prefix sum, a compaction and the
builder's plan stage — no sort) and returns a :class:`~sirgcn.graph.Graph` whose plan cache is already
filled: the layer that receives it builds nothing.  The semantics are ``dgl.remove_edges``': the survivors
are renumbered ``0..E'-1`` in ascending parent id, so ``efeats[kept]`` lines up with the child's edge ids.

``E'`` is data dependent, so the call synchronises once (one host transfer, of the plan's nine counts) and
cannot be captured into a HIP graph.

The random stream is the project's counter hash (``csrc/sirconv_dropout.h``): edge ``e`` is kept iff the
hash of ``(seed, e, 0)`` is at least ``round(p * 2^32)`` — the bit ``sir_dropout_apply`` gives element
``(e, 0)`` of an ``[E, 1]`` block.  It is not torch's Bernoulli stream (DGL samples on the host from its own
generator; that stream is not reproducible here either).  :func:`drop_edge_keep` restates the hash with torch
integer ops on the host: the CPU route of :class:`DropEdge` and the tests' oracle for the device bits.
"""
import math

import torch

from .graph import DEFAULT_CHUNK, Graph, GraphPlan, RowCSR, get_plan, plan_cache

_M32 = 0xFFFFFFFF


def _fmix(h):
    """murmur3's 32-bit finaliser (``drop_fmix``) on int64 tensors holding uint32 values."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def drop_threshold(p):
    """``make_drop``'s threshold: keep iff hash >= thr, thr = round(p * 2^32) in [1, 2^32]; 0 = no dropout."""
    p = float(p)
    if not p > 0.0:
        return 0
    thr = int((4294967296.0 if p >= 1.0 else p * 4294967296.0) + 0.5)
    return max(thr, 1)                  # a tiny p still drops something (never "off")


def drop_edge_keep(seed, E, p, device="cpu"):
    """bool [E]: the keep bit of every edge id under ``(seed, p)`` — ``drop_keep(d, drop_row_hash(d, e), 0)``
    with ``d = make_drop(p, seed)`` of ``csrc/sirconv_dropout.h``, restated with torch integer ops."""
    if math.isnan(float(p)):
        raise ValueError("drop_edge_keep: p is NaN")
    E = int(E)
    if E >= 2 ** 31 - 1:
        raise ValueError("int32 edge indices: E must be < 2^31")
    thr = drop_threshold(p)
    if thr == 0:
        return torch.ones(E, dtype=torch.bool, device=device)
    if thr > _M32:
        return torch.zeros(E, dtype=torch.bool, device=device)
    seed = int(seed) & (2 ** 64 - 1)
    s0 = seed & _M32
    s1 = (seed >> 32) ^ 0x6A09E667
    e = torch.arange(E, dtype=torch.int64, device=device)
    rh = _fmix(((e * 0x9E3779B1) & _M32) ^ s0)       # the row's high word is 0: E < 2^31
    return _fmix(rh ^ s1) >= thr                      # column 0: 0 * 0xCC9E2D51 + s1


def _device_of(graph, device):
    if device is None:
        src, _ = graph.edges()
        device = getattr(graph, "device", None) or torch.as_tensor(src).device
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _coo_on(graph, device):
    """The graph's int64 COO on ``device``, cached beside its plans (a host graph is uploaded once)."""
    cache = plan_cache(graph)
    key = ("coo", str(device))
    coo = cache.get(key)
    if coo is None:
        src, dst = graph.edges()
        coo = (torch.as_tensor(src).to(device, torch.int64), torch.as_tensor(dst).to(device, torch.int64))
        cache[key] = coo
    return coo


def _batch_num_nodes(graph):
    bnn = getattr(graph, "batch_num_nodes", None)
    return bnn() if callable(bnn) else None


def _child(graph, src, dst):
    return Graph(src, dst, int(graph.num_nodes()), _batch_num_nodes(graph))


def _csr(parts, n_rows, cnt, E2, perm=None):
    rowptr, col, eid, items, splits = parts
    n_items, n_splits, n_slots, max_deg = cnt
    return RowCSR(n_rows=n_rows, rowptr=rowptr, col=col[:E2], eid=eid[:E2], items=items[:n_items],
                  splits=splits[:n_splits] if n_splits else None, n_items=n_items, n_splits=n_splits,
                  n_slots=n_slots, max_degree=max_deg, perm=None if perm is None else perm[:E2])


def derive_plan(plan, chunk=DEFAULT_CHUNK, keep=None, drop=None):
    """``(child GraphPlan, kept)`` of a parent :class:`GraphPlan` on a GPU under a uint8 ``keep`` mask by edge
    id or the hash mask ``drop = (seed, p)``: ``sir_plan_drop_edges`` and ONE host transfer (the counts)."""
    from . import _native
    d, s, perm, kept, counts = _native.plan_drop_edges(plan.dst, plan.src, chunk, keep=keep, drop=drop)
    cnt = counts.cpu().tolist()
    E2 = cnt[8]
    child = GraphPlan.from_parts(_csr(d, plan.dst.n_rows, cnt[0:4], E2), _csr(s, plan.src.n_rows, cnt[4:8], E2, perm),
                                 plan.num_nodes, plan.device)
    return child, kept[:E2]


def _drop_native(graph, device, chunk, keep, drop):
    plan = get_plan(graph, device, chunk)           # built here only when the parent was never planned
    child_plan, kept = derive_plan(plan, chunk, keep=keep, drop=drop)
    src, dst = _coo_on(graph, device)
    child = _child(graph, src[kept], dst[kept])
    child._plans[(str(device), chunk)] = child_plan
    return child, kept


def drop_edges(graph, keep, efeats=None, device=None, chunk=DEFAULT_CHUNK):
    """``dgl.remove_edges(graph, ~keep)``: the graph of the edges whose ``keep`` bit (bool / uint8 ``[E]``, by
    edge id) is set, renumbered in ascending parent id.  Returns ``child``, or ``(child, efeats[kept])`` when
    ``efeats`` is given.

    ``graph``: a :class:`Graph`, a DGLGraph or an edges-object, as for :func:`get_plan`; ``device`` defaults to
    the graph's.  On a GPU the child's plan is derived from the parent's (built first if it was not cached)
    and pre-filled: a later ``get_plan(child, device, chunk)`` runs no build.  ``child`` keeps the parent's
    ``batch_num_nodes``; its COO lives on ``device``.  One host synchronisation (the plan sizes): not
    capturable into a HIP graph.  On the CPU the child is the compacted COO and plans lazily as any graph."""
    device = _device_of(graph, device)
    src, _ = graph.edges()
    E = int(torch.as_tensor(src).numel())
    keep = torch.as_tensor(keep)
    if keep.dim() != 1 or keep.numel() != E or keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"drop_edges: keep must be a bool / uint8 [{E}] mask by edge id")
    if device.type == "cuda":
        k8 = keep.to(device).view(torch.uint8) if keep.dtype == torch.bool else keep.to(device)
        child, kept = _drop_native(graph, device, chunk, k8.contiguous(), None)
    else:
        kept = torch.nonzero(keep.to(device)).flatten()
        src, dst = _coo_on(graph, device)
        child = _child(graph, src[kept], dst[kept])
    if efeats is None:
        return child
    return child, efeats[kept.to(efeats.device)]


class DropEdge:
    """``dgl.transforms.DropEdge(p)``: every edge dropped independently with probability ``p``.  A plain
    callable, not a module, and like DGL's (and the reference, which calls it whatever ``self.training`` is)
    it drops in eval mode too.

        graph_ = DropEdge(p)(graph)                      # ogbn-arxiv/model.py:146
        graphs_, efeats_ = DropEdge(p)(graphs, efeats)   # the wrapper of models/utils.py:96-102

    On a GPU graph the child's plan is derived natively from the parent's cached plan (:func:`drop_edges`);
    on a CPU graph the mask is :func:`drop_edge_keep` and the child the compacted COO.  Both routes draw the
    same bits: one 64-bit seed per call from torch's default CPU generator (reproducible under
    ``torch.manual_seed``), hashed per edge id — the project's counter hash, not torch's Bernoulli stream.
    ``last_kept`` holds the survivors' parent ids (int64, ascending, on the graph's device) of the last call
    and ``last_seed`` its seed, so ``drop_edge_keep(last_seed, E, p)`` reproduces the mask.

    ``p == 0`` returns the SAME graph object (and ``efeats``) and leaves ``last_kept`` None, so the parent's
    cached plan keeps serving; DGL's fast path returns a clone, which would lose the cache.  ``p == 1`` drops
    every edge.  The call synchronises once (``E'`` is data dependent): it does not capture into a HIP graph."""

    def __init__(self, p=0.5, chunk=DEFAULT_CHUNK):
        p = float(p)
        if math.isnan(p) or p < 0.0 or p > 1.0:
            raise ValueError(f"DropEdge: p must be in [0, 1], got {p}")
        self.p = p
        self.chunk = chunk
        self.last_kept = None
        self.last_seed = None

    def __call__(self, graph, efeats=None):
        if self.p == 0.0:
            self.last_kept = self.last_seed = None
            return graph if efeats is None else (graph, efeats)
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & (2 ** 64 - 1)
        device = _device_of(graph, None)
        if device.type == "cuda":
            child, kept = _drop_native(graph, device, self.chunk, None, (seed, self.p))
        else:
            src, dst = _coo_on(graph, device)
            kept = torch.nonzero(drop_edge_keep(seed, src.numel(), self.p, device)).flatten()
            child = _child(graph, src[kept], dst[kept])
        self.last_kept, self.last_seed = kept, seed
        if efeats is None:
            return child
        return child, efeats[kept.to(efeats.device)]

    def __repr__(self):
        return f"DropEdge(p={self.p})"
