"""Correct & Smooth: a torch CPU restatement of the reference's ``label_spreading`` and of the correct /
smooth steps of its ``run()`` (ogbn-arxiv/correct_and_smooth.py:41-58, 80, 86-96), and the builders of the
graphs and inputs the GPU tests run (tests/test_labelprop_gpu.py).

The restatement computes in the dtype of its input: fp32 gives the reference's CPU bits (``index_add_``
adds a row's messages one after another in edge-id order; tests/test_cs_cases_cpu.py pins it to the
fixtures of tests/golden/cs_*.npz with ``torch.equal``), fp64 is its twin with the same fp32 norm values —
the truth the split-row tolerance is measured against.
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CHUNK = 256                      # sirgcn.graph.DEFAULT_CHUNK (tests/test_cs_cases_cpu.py checks it)
SPECIAL = (CHUNK, CHUNK - 1, 0, 1)                    # in-degrees every unsplit graph holds (as V allows)
SPLIT = (2 * CHUNK + 1, CHUNK + 1)                    # ... and the split rows: 3 and 2 slots


# ------------------------------------------------------------------------------------ restatement
def in_norm(dst, V):
    """fp32 ``pow(in_degrees().float().clamp(min=1), -0.5)`` [V, 1] (correct_and_smooth.py:44-45)."""
    degs = torch.bincount(dst, minlength=V).float().clamp(min=1)
    return torch.pow(degs, -0.5).unsqueeze(1)


def apply_post(y, post):
    """post: None, ("clamp", lo, hi) or ("fix", yfix, idx)."""
    if post is None:
        return y
    if post[0] == "clamp":
        return y.clamp(post[1], post[2])
    y = y.clone()
    y[post[2]] = post[1].to(y.dtype)[post[2]]
    return y


def step(src, dst, V, y, y0, alpha, agg, post=None):
    """One propagation step from ``y`` (dtype of ``y0``); agg 'sym' / 'mean' (the reference's two) or 'sum'."""
    dt = y0.dtype
    y = y.to(dt)
    if agg == "sym":
        norm = in_norm(dst, V).to(dt)
        y = y * norm
    s = torch.zeros_like(y0).index_add_(0, dst, y[src])
    if agg == "sym":
        s = s * norm
    elif agg == "mean":
        s = s / torch.bincount(dst, minlength=V).clamp(min=1).to(dt).unsqueeze(1)
    return apply_post(alpha * s + (1 - alpha) * y0, post)


def spread(src, dst, V, y0, nprop, alpha, agg, post=None):
    y = y0
    for _ in range(nprop):
        y = step(src, dst, V, y, y0, alpha, agg, post)
    return y


def correct_and_smooth(src, dst, V, predictions, labels, train_idx, alpha_c, nprop_c, alpha_s, nprop_s, use_sym):
    """run()'s smoothed_y (lines 80, 86-96) in the dtype of ``predictions``."""
    agg = "sym" if use_sym else "mean"
    C = predictions.shape[1]
    dt = predictions.dtype
    onehot = torch.nn.functional.one_hot(labels.reshape(-1)[train_idx], C).to(dt)
    y = predictions.clone()
    dy = torch.zeros(V, C, dtype=dt)
    dy[train_idx] = onehot - y[train_idx]
    y = y + alpha_c * spread(src, dst, V, dy, nprop_c, alpha_c, agg, ("fix", dy, train_idx))
    y[train_idx] = onehot
    return spread(src, dst, V, y, nprop_s, alpha_s, agg, ("clamp", 0.0, 1.0))


# ------------------------------------------------------------------------------------ graphs
def degrees_for(V, split, seed=0):
    """In-degree of every row: the special degrees first (as many as V holds), small random ones after."""
    want = (SPLIT if split else ()) + SPECIAL
    rng = np.random.default_rng(1000 + 7 * V + seed)
    deg = rng.integers(1, 9, size=V)
    deg[:min(V, len(want))] = want[:V]
    return [int(d) for d in deg]


def graph_with_degrees(V, deg, seed=0):
    """(src, dst) int64 with in-degree ``deg[v]`` at row v: uniformly random sources (so duplicate edges and
    nodes without out-edges), a self-loop first at every other row that has edges, edge ids shuffled."""
    rng = np.random.default_rng(2000 + 11 * V + seed)
    src, dst = [], []
    for v, d in enumerate(deg):
        if d == 0:
            continue
        s = rng.integers(0, V, size=d)
        if v % 2 == 0:
            s[0] = v
        src.append(s)
        dst.append(np.full(d, v))
    if not src:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(src.size)
    return torch.from_numpy(src[perm].astype(np.int64)), torch.from_numpy(dst[perm].astype(np.int64))


_GRAPHS = {}


def case_graph(V, split):
    """The graph of the GPU tests for (V, split): (src, dst, deg); built once."""
    key = (V, bool(split))
    if key not in _GRAPHS:
        deg = degrees_for(V, split)
        _GRAPHS[key] = graph_with_degrees(V, deg) + (deg,)
    return _GRAPHS[key]


def low_degree_graph(V):
    """(src, dst, deg) with in-degrees 0..8 only: 16-bit sums of so few terms stay well conditioned."""
    key = (V, "low")
    if key not in _GRAPHS:
        deg = [int(d) for d in np.random.default_rng(4000 + V).integers(0, 9, size=V)]
        _GRAPHS[key] = graph_with_degrees(V, deg, seed=1) + (deg,)
    return _GRAPHS[key]


def inputs(V, F, seed=0):
    """y0 [V, F] (normal: a clamp to [0, 1] bites), yfix [V, F], idx (about half the rows, row 0 among them)."""
    g = torch.Generator().manual_seed(3000 + 13 * V + F + seed)
    y0 = torch.randn(V, F, generator=g)
    yfix = torch.randn(V, F, generator=g)
    idx = torch.nonzero(torch.rand(V, generator=g) < 0.5).flatten()
    if V > 1:
        idx = torch.unique(torch.cat([idx, torch.tensor([0])]))       # sorted; row 0 (a special row) is fixed
        idx = idx[idx != 1]                                           # ... and row 1 (the other split row) is not
    return y0, yfix, idx


def downstream(src, dst, V, rows, hops):
    """Bool [V]: rows reachable from ``rows`` along edges in at most ``hops`` steps (``rows`` included) — where a
    tolerance-level difference at ``rows`` can show after ``hops`` further propagation steps."""
    hit = torch.zeros(V, dtype=torch.bool)
    hit[rows] = True
    for _ in range(hops):
        nxt = hit.clone()
        nxt[dst[hit[src]]] = True
        hit = nxt
    return hit


# ------------------------------------------------------------------------------------ fixtures
def cs_manifest():
    with open(os.path.join(GOLDEN, "cs_manifest.json")) as f:
        return json.load(f)["cases"]


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def fixture_post(case, fx):
    if case["post"] == "clamp":
        return ("clamp", case["lo"], case["hi"])
    if case["post"] == "fix":
        return ("fix", fx["yfix"], fx["idx"])
    return None
