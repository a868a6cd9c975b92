#!/usr/bin/env python3
"""DropEdge per layer: the native derivation (``sirgcn.DropEdge``: ``sir_plan_drop_edges`` on the parent's
cached plan) against what a user writes without it — mask -> ``nonzero`` -> ``src[kept]``, ``dst[kept]`` ->
``Graph`` -> ``get_plan`` (two radix sorts, the perm pass and the builder's synchronisation) — on IDENTICAL
keep bits, interleaved in ONE process, timed with HIP events around each whole call (host work and the
synchronisation included: the call ends with the child's plan ready on the host side).

Routes:
  a        DropEdge(p)(graph): seed draw, hash, derivation, counts transfer, child COO;
  b        the given mask (the same bits, computed outside the timed window) -> nonzero -> COO -> Graph ->
           get_plan;
  b-bern   as b with the mask drawn inside the window by torch.bernoulli (other bits; for the record).

Warm-up, then --runs runs of --steps interleaved steps; reported per route: the median over runs of each
run's median, and the spread (max - min) of the runs' medians.  Gate (the arxiv shape only): a is below b by
more than the larger of the two spreads.  The batched shapes are launch-bound and recorded only.

    python tools/dropedge_bench.py > profiles/dropedge_bench.txt
    rocprofv3 --kernel-trace --stats ... -- python tools/dropedge_bench.py --count-launches a --iters 20
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402

import sirgcn  # noqa: E402
from sirgcn import DropEdge, Graph, _native, drop_edge_keep, get_plan, workloads  # noqa: E402
from sirgcn.synth import molecule_batch  # noqa: E402

DEV = "cuda:0"

# (name, builder, gated)
SHAPES = (
    ("arxiv", lambda: workloads.make_graph("cfg3"), True),
    ("mol128", lambda: molecule_batch(128, 23), False),
    ("cfg5", lambda: workloads.make_graph("cfg5"), False),
)


def algorithmic_bytes(E, q, n_rows):
    """HBM bytes sir_plan_drop_edges moves by the algorithm (hash mode; q = kept fraction; both CSRs share
    n_rows): per edge position the flags (two edge ids read, one triple written), the scan (a triple read and
    written), the compaction (a triple read; per survivor 28 B of parent col / eid / perm read, three 4-B
    gathers, 36 B of child col / eid / perm / kept written); per row and side the degree (two rowptr, two
    gathered triples' words, one degree) and the plan stage (degree, RowAcc written, scanned, read twice,
    rowptr and one item written)."""
    per_edge = (16 + 12) + (12 + 12) + 12 + q * (28 + 12 + 36)
    per_row = 2 * ((8 + 8 + 4) + (4 + 16 + 32 + 32 + 4 + 16))
    return E * per_edge + n_rows * per_row


def route_a(de, g):
    return de(g)


def route_b(g, keep):
    src, dst = g.edges()
    kept = torch.nonzero(keep).flatten()
    child = Graph(src[kept], dst[kept], g.num_nodes(), g.batch_num_nodes())
    get_plan(child, DEV)
    return child


def route_b_bern(g, p):
    E = g.num_edges()
    keep = torch.bernoulli(torch.full((E,), 1.0 - p, device=DEV)).bool()
    return route_b(g, keep)


def timed(fn):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def bench(name, g, p, runs, steps, warmup):
    E, V = g.num_edges(), g.num_nodes()
    de = DropEdge(p)
    routes = ("a", "b", "b-bern")
    run_medians = {r: [] for r in routes}
    native_ms = []
    for run in range(runs):
        times = {r: [] for r in routes}
        for it in range(warmup + steps):
            torch.manual_seed(1000 * run + it)
            rec = _native.enable_timing(True)
            ta, child = timed(lambda: route_a(de, g))
            ev = rec.get("sir_plan_drop_edges", [])
            _native.enable_timing(False)
            keep = drop_edge_keep(de.last_seed, E, p, DEV)          # the same bits, outside the window
            torch.cuda.synchronize()
            tb, ref = timed(lambda: route_b(g, keep))
            tc, _ = timed(lambda: route_b_bern(g, p))
            if it == 0 and run == 0:                                # same bits -> the same child
                assert torch.equal(child.edges()[0], ref.edges()[0])
                pa, pb = get_plan(child, DEV), get_plan(ref, DEV)
                assert torch.equal(pa.dst.eid, pb.dst.eid) and torch.equal(pa.src.perm, pb.src.perm)
                assert torch.equal(pa.dst.items, pb.dst.items) and torch.equal(pa.src.rowptr, pb.src.rowptr)
            if it >= warmup:
                times["a"].append(ta)
                times["b"].append(tb)
                times["b-bern"].append(tc)
                native_ms += [s.elapsed_time(e) for s, e, _ in ev]
        for r in routes:
            run_medians[r].append(statistics.median(times[r]))
    q = de.last_kept.numel() / max(E, 1)
    res = {}
    for r in routes:
        m = run_medians[r]
        res[r] = (statistics.median(m), max(m) - min(m))
        print(f"  {name:7s} p={p:<4} {r:7s} {res[r][0]:9.4f} ms  spread {res[r][1]:7.4f} ms  (runs: "
              + " ".join(f"{x:.4f}" for x in m) + ")")
    nat = statistics.median(native_ms)
    by = algorithmic_bytes(E, q, V)
    print(f"  {name:7s} p={p:<4} sir_plan_drop_edges alone (device events around the entry): {nat:.4f} ms; "
          f"{by / max(E, 1):.1f} B/edge by the algorithm (kept {q:.3f}) -> {by / (nat * 1e-3) / 1e9:.1f} GB/s")
    print(f"  {name:7s} p={p:<4} b / a = {res['b'][0] / res['a'][0]:.2f}")
    return res


def count_launches(route, shape, p, iters):
    """For a profiler run of its own: the set-up, then ``iters`` calls of one route and nothing else."""
    g = dict((n, b) for n, b, _ in SHAPES)[shape]().to(DEV)
    get_plan(g, DEV)
    de = DropEdge(p)
    torch.manual_seed(0)
    keep = drop_edge_keep(1234, g.num_edges(), p, DEV)
    torch.cuda.synchronize()
    for _ in range(iters):
        route_a(de, g) if route == "a" else route_b(g, keep)
    torch.cuda.synchronize()
    print(f"count-launches: route {route}, shape {shape}, p {p}, {iters} calls after the set-up")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count-launches", choices=("a", "b"), default=None)
    ap.add_argument("--shape", default="mol128")
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropedge_bench needs the MI355X (no CPU timing is meaningful)")
    if a.count_launches:
        return count_launches(a.count_launches, a.shape, a.p, a.iters)
    if a.runs < 3 or a.steps < 10 or a.warmup < 2:
        raise SystemExit("--runs must be >= 3, --steps >= 10 and --warmup >= 2")
    print("DropEdge per call: a = sirgcn.DropEdge (sir_plan_drop_edges on the cached parent plan), b = mask -> nonzero "
          "-> COO -> Graph -> get_plan on the same bits, b-bern = b with a torch.bernoulli mask drawn inside the window")
    print(f"device: {torch.cuda.get_device_name(0)}; HIP events around each whole call (host work and the sync "
          f"included); warm-up {a.warmup}, then {a.runs} runs of {a.steps} interleaved steps: median over runs of each "
          "run's median, spread = max - min of the runs' medians")
    verdict = []
    for name, build, gated in SHAPES:
        g = build().to(DEV)
        get_plan(g, DEV)
        print(f"{name}: V = {g.num_nodes()}, E = {g.num_edges()}, B = {g.batch_size}" + ("" if gated else
              "  (launch-bound; recorded, not gated)"))
        for p in (0.1, 0.5):
            res = bench(name, g, p, a.runs, a.steps, a.warmup)
            if gated:
                margin = res["b"][0] - res["a"][0]
                spread = max(res["a"][1], res["b"][1])
                verdict.append((name, p, margin > spread, margin, spread))
        torch.cuda.empty_cache()
    for name, p, ok, margin, spread in verdict:
        print(f"gate {name} p={p}: b - a = {margin:.4f} ms, larger spread {spread:.4f} ms: "
              + ("a is faster beyond the spread" if ok else "NOT MET"))
    if not all(v[2] for v in verdict):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
