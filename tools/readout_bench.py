#!/usr/bin/env python3
"""Native graph readout (``sirgcn.SumPooling`` / ``AvgPooling``: ``sir_graph_pool_fwd`` / ``_bwd``) against the
torch composition a user writes without DGL — ``repeat_interleave`` graph ids, ``zeros().index_add_`` and,
for the mean, ``/ n`` — forward + backward, fp32, interleaved in ONE process on identical data, timed with HIP
events around each step (host launches included: the batched shapes are launch-bound): warm-up, then the
median and min of --steps steps.  ``MaxPooling`` has no one-line torch composition: its native time is
reported alone.

    python tools/readout_bench.py > profiles/readout_vs_torch.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402

import sirgcn  # noqa: E402
from sirgcn import Graph, workloads  # noqa: E402

POOLS = {"sum": sirgcn.SumPooling, "mean": sirgcn.AvgPooling, "max": sirgcn.MaxPooling}


def _uniform(num_graphs, nodes):
    e = torch.zeros(0, dtype=torch.int64)
    return sirgcn.batch([Graph(e, e, nodes) for _ in range(num_graphs)])


# (graph builder, F, label, gated: the native path is expected to be no slower)
SHAPES = (
    (lambda: workloads.molecule_batch(64, 25), 300, "cfg5 batch: molecule_batch(64, 25)", True),
    (lambda: _uniform(128, 100), 80, "128 graphs of 100 nodes", True),
    (lambda: _uniform(256, 20), 1, "256 graphs of 20 nodes", True),
    (lambda: _uniform(4, 100_000), 256, "4 graphs of 100,000 nodes (slab path; recorded only)", False),
)


def bench(graph, F, op, steps, warmup, dev="cuda"):
    V, B = graph.num_nodes(), graph.batch_size
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(V, F, generator=gen, device=dev)
    dP = torch.randn(B, F, generator=gen, device=dev)
    n = torch.as_tensor(graph.batch_num_nodes(), dtype=torch.int64).to(dev)
    pool = POOLS[op]()

    def composed(Xr):
        ids = torch.repeat_interleave(torch.arange(B, device=dev), n, output_size=V)
        P = torch.zeros(B, F, device=dev).index_add_(0, ids, Xr)
        return P / n.clamp(min=1)[:, None] if op == "mean" else P

    def step(name):
        Xr = X.detach().requires_grad_(True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        P = pool(graph, Xr) if name == "native" else composed(Xr)
        ev[1].record()
        P.backward(dP)
        ev[2].record()
        return ev, (P.detach(), Xr.grad)

    routes = ("native", "torch") if op != "max" else ("native",)
    times = {r: {"fwd": [], "bwd": [], "step": []} for r in routes}
    outs = {}
    for r in range(warmup + steps):
        for name in routes:
            ev, out = step(name)
            torch.cuda.synchronize()
            if r == warmup - 1:
                outs[name] = [t.clone() for t in out]
            if r >= warmup:
                times[name]["fwd"].append(ev[0].elapsed_time(ev[1]))
                times[name]["bwd"].append(ev[1].elapsed_time(ev[2]))
                times[name]["step"].append(ev[0].elapsed_time(ev[2]))
    med = statistics.median
    for name in routes:
        t = times[name]
        print(f"  {op:4s} {name:6s} step {med(t['step']):8.4f} ({min(t['step']):8.4f})  fwd {med(t['fwd']):8.4f} "
              f"({min(t['fwd']):8.4f})  bwd {med(t['bwd']):8.4f} ({min(t['bwd']):8.4f})")
    if op == "max":
        return None
    ratio = med(times["torch"]["step"]) / med(times["native"]["step"])
    rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm()).item()
    print(f"  {op:4s} step time ratio torch / native: {ratio:.2f}; native vs torch relative L2: "
          + ", ".join(f"{k} {rel(x, y):.2e}" for k, x, y in zip(("P", "dX"), outs["native"], outs["torch"])))
    return ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("readout_bench needs the MI355X (no CPU timing is meaningful)")
    if a.steps < 20 or a.warmup < 3:
        raise SystemExit("--steps must be >= 20 (median of at least 20 steps) and --warmup >= 3")
    print("graph readout, fp32, forward + backward: native sir_graph_pool_fwd / _bwd vs repeat_interleave + index_add_ (/ n)")
    print(f"device: {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, median (min) of {a.steps} interleaved steps, ms")
    slower = []
    for build, F, what, gated in SHAPES:
        graph = build()
        print(f"{what}: V = {graph.num_nodes()}, B = {graph.batch_size}, F = {F}")
        for op in ("sum", "mean", "max"):
            ratio = bench(graph, F, op, a.steps, a.warmup)
            if gated and ratio is not None and ratio < 1.0:
                slower.append((what, op, round(ratio, 2)))
        torch.cuda.empty_cache()
    print("native slower than the torch composition at a batched shape: " + (", ".join(map(str, slower)) if slower else "none"))


if __name__ == "__main__":
    main()
