"""Inputs and the restatement of the graph readout (sirgcn.readout) shared by the readout tests.

The reference is a short restatement of DGL's ``segment_reduce`` readout as a Python loop over the graphs and
their rows, in node order, in the dtype of its input (fp32: the reference's own arithmetic; fp64: the truth):
  sum: the rows added in node order;  mean: that sum / max(n, 1) (one division);
  max: starts from the first row, a later row wins only on a strict > (the lowest node id wins a tie);
  an empty graph gives 0 (arg -1);  the backward routes dP per graph (sum), dP / n (mean), or to the arg row.
Exact inputs: integers in [-8, 8] divided by 4 — every sum is an integer below 2^24 quarter-units, so fp32 and
fp64 agree bit for bit whatever the order, and every value is a bf16 and an fp16 number.
"""
import functools

import torch

OPS = ("sum", "mean", "max")
EXACT_WIDTH = 300          # the exact inputs of a narrower F are the first F columns (columns never mix)


def sizes(R):
    """Nodes per graph: empty graphs (first, middle, last), single nodes, around the slab R, several slabs."""
    return [0, 1, 2, 3, 25, 64, 65, 0, R - 1, R, R + 1, 7, 3 * R + 7, 0]


def offsets(ns):
    off = torch.zeros(len(ns) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(ns, dtype=torch.int64), 0)
    return off


def pool_ref(X, ns, op):
    """(P [B, F], arg int32 [B, F]) in X's dtype; rows in node order."""
    B, F = len(ns), X.shape[1]
    P = torch.zeros(B, F, dtype=X.dtype)
    arg = torch.full((B, F), -1, dtype=torch.int32)
    r0 = 0
    for b, n in enumerate(ns):
        if n > 0:
            acc = X[r0].clone()
            a = torch.zeros(F, dtype=torch.int32)
            for k in range(1, n):
                row = X[r0 + k]
                if op == "max":
                    better = row > acc
                    acc = torch.where(better, row, acc)
                    a = torch.where(better, torch.full_like(a, k), a)
                else:
                    acc = acc + row
            if op == "mean":
                acc = acc / torch.full((F,), max(n, 1), dtype=X.dtype)
            P[b] = acc
            if op == "max":
                arg[b] = a
        r0 += n
    return P, arg


def pool_bwd_ref(dP, arg, ns, op):
    """dX [V, F] in dP's dtype."""
    V, F = sum(ns), dP.shape[1]
    dX = torch.zeros(V, F, dtype=dP.dtype)
    r0 = 0
    for b, n in enumerate(ns):
        if n > 0:
            if op == "sum":
                dX[r0:r0 + n] = dP[b]
            elif op == "mean":
                dX[r0:r0 + n] = dP[b] / torch.full((F,), n, dtype=dP.dtype)
            else:
                rel = torch.arange(n, dtype=torch.int32)[:, None]
                dX[r0:r0 + n] = torch.where(rel == arg[b][None, :], dP[b][None, :], torch.zeros((), dtype=dP.dtype))
        r0 += n
    return dX


@functools.lru_cache(maxsize=None)
def exact_inputs(R):
    """(ns, X [V, EXACT_WIDTH], dP [B, EXACT_WIDTH]) fp32: integers in [-8, 8] / 4."""
    ns = sizes(R)
    g = torch.Generator().manual_seed(20240 + R)
    X = torch.randint(-8, 9, (sum(ns), EXACT_WIDTH), generator=g).float() / 4
    dP = torch.randint(-8, 9, (len(ns), EXACT_WIDTH), generator=g).float() / 4
    return ns, X, dP


@functools.lru_cache(maxsize=None)
def exact_expected(R, op, dtype=torch.float64):
    """{P, arg, dX} of the exact inputs at the full width, computed in ``dtype``."""
    ns, X, dP = exact_inputs(R)
    P, arg = pool_ref(X.to(dtype), ns, op)
    return {"P": P, "arg": arg, "dX": pool_bwd_ref(dP.to(dtype), arg, ns, op)}


def tie_share(X, ns):
    """Share of the (graph, column) pairs, over the graphs of more than one node, whose maximum is reached twice."""
    ties = pairs = 0
    r0 = 0
    for n in ns:
        if n > 1:
            seg = X[r0:r0 + n]
            ties += int(((seg == seg.max(0).values).sum(0) > 1).sum())
            pairs += X.shape[1]
        r0 += n
    return ties / pairs


@functools.lru_cache(maxsize=None)
def random_case(R, F):
    """Random inputs (per-column scale and offset, as the node-norm tests) and their fp32 / fp64 restatements:
    (ns, X, dP, {op: (ref32, ref64)}) with ref = {P, arg, dX}."""
    ns = sizes(R)
    V, B = sum(ns), len(ns)
    g = torch.Generator().manual_seed(1000 * V + F)
    std = 0.5 + 1.5 * torch.rand(F, generator=g)
    shift = 60.0 * torch.rand(F, generator=g) - 30.0
    X = torch.randn(V, F, generator=g) * std + shift
    dP = torch.randn(B, F, generator=g)
    refs = {}
    for op in OPS:
        out = []
        for dt in (torch.float32, torch.float64):
            P, arg = pool_ref(X.to(dt), ns, op)
            out.append({"P": P, "arg": arg, "dX": pool_bwd_ref(dP.to(dt), arg, ns, op)})
        refs[op] = tuple(out)
    return ns, X, dP, refs
