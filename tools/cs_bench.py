#!/usr/bin/env python3
"""Correct & Smooth on the ogbn-arxiv-shaped graph (``synth.named_graph('arxiv')`` made bidirected, with
self-loops: the reference's ``--add-reverse-edge --add-self-loop``), C = 40 classes, the full 10 + 10 step run of
``correct_and_smooth.py`` (alpha 0.8, sym), three routes interleaved in ONE process on identical data:

  (a) fused   : ``sirgcn.correct_and_smooth`` — one ``sir_label_prop_step`` launch per step, post steps inside;
  (b) callable: the same step kernel with the reference's post steps as torch callables after each step;
  (c) torch   : what a user writes without DGL — a torch sparse CSR ``A @ (y * norm)`` plus the elementwise ops.

Each run times --steps whole C&S calls per route with HIP events (host launches included) after a warm-up and
takes the run's median; reported: the median over --runs runs of those medians and their spread (min .. max).
Beside the times: the bytes one propagation step has to move by the algorithm (gathered rows, indices, norms,
y0 read, output written), computed from the shapes.

    python tools/cs_bench.py > profiles/cs_bench.txt
"""
import argparse
import os
import statistics
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402

import sirgcn  # noqa: E402
from sirgcn import Graph, get_plan, synth  # noqa: E402


def arxiv_graph():
    g = synth.named_graph("arxiv")
    src, dst = g.edges()
    V = g.num_nodes()
    key = torch.unique(torch.cat([src * V + dst, dst * V + src]))          # bidirected, duplicates merged
    s, d = key // V, key % V
    keep = s != d
    loops = torch.arange(V)
    return Graph(torch.cat([s[keep], loops]), torch.cat([d[keep], loops]), V)


def fix_input(x, y, mask):
    x[mask] = y[mask]
    return x


def cs_with(spread, graph, predictions, onehot, train_idx, alpha, nprop, posts):
    """run()'s correct and smooth steps around a ``label_spreading`` implementation."""
    V, C = predictions.shape
    y = predictions.clone()
    dy = torch.zeros(V, C, device=predictions.device)
    dy[train_idx] = onehot - y[train_idx]
    y = y + alpha * spread(graph, dy, nprop=nprop, alpha=alpha, use_sym=True, post_step=posts[0](dy))
    y[train_idx] = onehot
    return spread(graph, y, nprop=nprop, alpha=alpha, use_sym=True, post_step=posts[1])


def torch_spreading(A, norm):
    def spread(graph, y0, nprop, alpha, use_sym, post_step):
        y = y0
        for _ in range(nprop):
            y = (A @ (y * norm)) * norm
            y = alpha * y + (1 - alpha) * y0
            y = post_step(y)
        return y
    return spread


def step_bytes(plan, C, fixed):
    """Bytes one sym step moves by the algorithm: (all rows gathered, the rows of ``fixed`` skipped)."""
    csr = plan.dst
    V, E = plan.num_nodes, plan.num_edges
    deg = plan.in_deg
    e_fix = int(deg[fixed.bool()].sum())
    n_fix = int(fixed.sum())

    def total(edges, rows_mixed):
        gather = edges * (C * 4 + 4 + 4)                  # Y[u] row, col[e], norm[u]
        rows = rows_mixed * (2 * C * 4 + 4) + (V - rows_mixed) * 2 * C * 4     # Y0 + out (+ norm[v]) | Yfix + out
        return gather + rows + csr.n_items * 16 + V
    return total(E, V), total(E - e_fix, V - n_fix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--nprop", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cs_bench needs the MI355X (no CPU timing is meaningful)")
    dev = torch.device("cuda", 0)
    C, alpha = a.classes, 0.8
    graph = arxiv_graph()
    V = graph.num_nodes()
    gen = torch.Generator().manual_seed(0)
    predictions = torch.softmax(torch.randn(V, C, generator=gen), -1).to(dev)
    labels = torch.randint(0, C, (V,), generator=gen).to(dev)
    train_idx = torch.randperm(V, generator=gen)[:int(0.537 * V)].sort().values.to(dev)     # arxiv: 90,941 of 169,343
    onehot = torch.nn.functional.one_hot(labels[train_idx], C).float()
    plan = get_plan(graph, dev)
    csr = plan.dst
    norm = plan.norms("sym")[0][:, None]
    A = torch.sparse_csr_tensor(csr.rowptr.long(), csr.col.long(), torch.ones(plan.num_edges, device=dev), size=(V, V))
    fixed = torch.zeros(V, dtype=torch.uint8, device=dev)
    fixed[train_idx] = 1
    clamp = lambda x: x.clamp(0, 1)  # noqa: E731
    routes = {
        "fused": lambda: sirgcn.correct_and_smooth(graph, predictions, labels, train_idx, alpha, a.nprop, alpha, a.nprop, True),
        "callable": lambda: cs_with(sirgcn.label_spreading, graph, predictions, onehot, train_idx, alpha, a.nprop,
                                    (lambda dy: partial(fix_input, y=dy, mask=train_idx), clamp)),
        "torch": lambda: cs_with(torch_spreading(A, norm), graph, predictions, onehot, train_idx, alpha, a.nprop,
                                 (lambda dy: partial(fix_input, y=dy, mask=train_idx), clamp)),
    }
    print(f"Correct & Smooth, fp32, {a.nprop} + {a.nprop} propagation steps, alpha {alpha}, sym: V = {V}, E = {plan.num_edges} "
          f"(bidirected + self-loops), C = {C}, {int(fixed.sum())} training rows; max in-degree {csr.max_degree}, "
          f"{csr.n_splits} split rows")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.runs} runs of {a.steps} interleaved calls per route after "
          f"{a.warmup} warm-up calls; ms per whole C&S call")
    with torch.no_grad():
        outs = {}
        for _ in range(a.warmup):
            for name, fn in routes.items():
                outs[name] = fn()
        torch.cuda.synchronize()
        rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm()).item()  # noqa: E731
        print(f"results: fused == callable bit for bit: {torch.equal(outs['fused'], outs['callable'])}; "
              f"fused vs torch relative L2 {rel(outs['fused'], outs['torch']):.2e}")
        meds = {name: [] for name in routes}
        for _ in range(a.runs):
            t = {name: [] for name in routes}
            for _ in range(a.steps):
                for name, fn in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    t[name].append(e0.elapsed_time(e1))
            for name in routes:
                meds[name].append(statistics.median(t[name]))
    med = {name: statistics.median(v) for name, v in meds.items()}
    for name in routes:
        v = meds[name]
        print(f"  {name:9s} median of run medians {med[name]:8.3f}   spread {min(v):8.3f} .. {max(v):8.3f}   "
              f"per propagation step {med[name] / (2 * a.nprop) * 1e3:8.1f} us")
    spread = max(max(v) - min(v) for v in meds.values())
    b_all, b_fix = step_bytes(plan, C, fixed)
    us = med["fused"] / (2 * a.nprop) * 1e3
    print(f"algorithmic bytes per step: {b_all / 1e6:.1f} MB (smooth: every row gathered), {b_fix / 1e6:.1f} MB (correct: the "
          f"training rows skipped); at the fused route's {us:.1f} us per step (its launches and the torch ops around the "
          f"two loops included) that is {(b_all + b_fix) / 2 / us / 1e6:.2f} TB/s on average")
    diff = med["torch"] - med["fused"]
    print(f"torch - fused = {diff:.3f} ms against a larger run-to-run spread of {spread:.3f} ms: "
          + ("fused is faster by more than the spread" if diff > spread else
             "NOT faster by more than the spread" if diff > 0 else "fused is SLOWER"))
    print(f"time ratio torch / fused {med['torch'] / med['fused']:.2f}, callable / fused {med['callable'] / med['fused']:.2f}")


if __name__ == "__main__":
    main()
