#!/usr/bin/env python3
"""Fused BatchNorm / LayerNorm -> LeakyReLU(0.2) -> + resid (``GraphBatchNorm.forward_act`` /
``GraphLayerNorm.forward_act``) against the torch chain ``nn.BatchNorm1d`` / ``nn.LayerNorm`` ->
``nn.LeakyReLU(0.2)`` -> ``+ resid`` — what a stack with these norms ran before — forward + backward,
training mode, interleaved in ONE process on identical data, timed with HIP events: warm-up, then the
median and min of --steps steps.

    python tools/norm_bench.py > profiles/norm_fused_vs_torch.txt

Per shape and norm: each route's step / forward / backward time, its design bytes (passes over a
V*H*4-byte tensor) over its step time against the 6.3 TB/s achievable HBM rate, the peak memory of one
step, and the relative L2 difference of the two routes' outputs and gradients.

    python tools/norm_bench.py --dropout > profiles/norm_fused_dropout.txt

The layer dropout fused into the pass (``forward_act(..., dropout=(seed, p))``), BatchNorm and LayerNorm at the
arxiv shape and GraphNorm at the cfg5 batch, forward + backward, three routes interleaved in one process:
(a) the fused pass with p = 0, (b) the fused pass with p = 0.2 (a device-resident seed word, as the stack hands
it in), (c) what a caller ran without it for p = 0.2: the fused pass without residual, then ``nn.Dropout``, then
the add.  --runs repetitions of the whole measurement give the run-to-run spread of each median."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from sirgcn import GraphBatchNorm, GraphLayerNorm, GraphNorm  # noqa: E402

ACHIEVABLE = 6.3e12        # B/s, the streaming rate the edge kernels are measured against
SHAPES = ((169_343, 256, "arxiv"), (231_000, 128, "ZINC batch, float4 columns"), (231_000, 75, "ZINC batch, scalar columns"),
          (2_000_000, 256, "S2"), (1_600, 300, "molhiv batch (launch-bound; reported, not gated)"))
# passes over a V*H*4-byte tensor, forward + backward
PASSES = {
    # stats: X | apply: X, R, out || reduce: X, D | apply: X, D, dX
    ("bn", "fused"): (4, 5),
    # stats: X | apply: X, Y | act: Y, A | add: A, R, out || act': D, Y, G | reduce: X, G | apply: X, G, dX
    ("bn", "torch"): (8, 8),
    # X, R, out || X, D, dX
    ("ln", "fused"): (3, 3),
    # norm: X, Y | act: Y, A | add: A, R, out || act': D, Y, G | dX: X, G, dX | dweight, dbias: X, G
    ("ln", "torch"): (7, 8),
}


def bench(kind, V, H, steps, warmup, dev="cuda"):
    gen = torch.Generator(device=dev).manual_seed(0)
    std = 0.5 + 1.5 * torch.rand(H, generator=gen, device=dev)
    off = 60.0 * torch.rand(H, generator=gen, device=dev) - 30.0
    X = torch.randn(V, H, generator=gen, device=dev) * std + off
    Rr = torch.randn(V, H, generator=gen, device=dev)
    dY = torch.randn(V, H, generator=gen, device=dev)
    gamma, beta = 0.5 + torch.rand(H, generator=gen, device=dev), torch.randn(H, generator=gen, device=dev)
    fused = (GraphBatchNorm if kind == "bn" else GraphLayerNorm)(H).to(dev)
    plain = (nn.BatchNorm1d if kind == "bn" else nn.LayerNorm)(H).to(dev)
    act = nn.LeakyReLU(0.2)
    with torch.no_grad():
        for m in (fused, plain):
            m.weight.copy_(gamma)
            m.bias.copy_(beta)

    def step(name):
        m = fused if name == "fused" else plain
        m.zero_grad(set_to_none=True)
        Xr, Rq = X.detach().requires_grad_(True), Rr.detach().requires_grad_(True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        Y = m.forward_act(None, Xr, act, Rq) if name == "fused" else act(m(Xr)) + Rq
        ev[1].record()
        Y.backward(dY)
        ev[2].record()
        return ev, (Y.detach(), Xr.grad, m.weight.grad, m.bias.grad)

    routes = ("fused", "torch")
    times = {n: {"fwd": [], "bwd": [], "step": []} for n in routes}
    peak, outs = {}, {}
    for r in range(warmup + steps):
        for name in routes:
            if r == warmup - 1:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
            ev, out = step(name)
            torch.cuda.synchronize()
            if r == warmup - 1:
                peak[name] = torch.cuda.max_memory_allocated() - base
                outs[name] = [t.clone() for t in out]
            if r >= warmup:
                times[name]["fwd"].append(ev[0].elapsed_time(ev[1]))
                times[name]["bwd"].append(ev[1].elapsed_time(ev[2]))
                times[name]["step"].append(ev[0].elapsed_time(ev[2]))
            del out
    med = statistics.median
    unit = V * H * 4
    for name in routes:
        t = times[name]
        pf, pb = PASSES[(kind, name)]
        rate = (pf + pb) * unit / (med(t["step"]) * 1e-3)
        print(f"  {name:6s} step {med(t['step']):8.3f} ({min(t['step']):8.3f})  fwd {med(t['fwd']):8.3f} ({min(t['fwd']):8.3f})  "
              f"bwd {med(t['bwd']):8.3f} ({min(t['bwd']):8.3f})  design {pf}+{pb} passes = {(pf + pb) * unit / 2**20:8.1f} MiB "
              f"-> {rate / 1e12:5.2f} TB/s = {rate / ACHIEVABLE:4.2f} of 6.3 TB/s  peak {peak[name] / 2**20:8.1f} MiB = "
              f"{peak[name] / unit:4.2f} x V*H*4")
    ratio = med(times["torch"]["step"]) / med(times["fused"]["step"])
    rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm()).item()
    print(f"  step time ratio torch / fused: {ratio:.2f} (fwd {med(times['torch']['fwd']) / med(times['fused']['fwd']):.2f}, "
          f"bwd {med(times['torch']['bwd']) / med(times['fused']['bwd']):.2f}); fused vs torch relative L2: "
          + ", ".join(f"{n} {rel(x, y):.2e}" for n, x, y in zip(("out", "dX", "dweight", "dbias"), outs["fused"], outs["torch"])))
    return ratio


DROP_P = 0.2
DROP_ROUTES = ("fused p=0", "fused p=0.2", "fused + nn.Dropout + add")


def bench_dropout(kind, steps, warmup, runs, dev="cuda"):
    """Median step time (ms) of the three routes of the module docstring, once per run: {route: [medians]}."""
    from sirgcn.workloads import CONFIGS, make_graph
    gen = torch.Generator(device=dev).manual_seed(0)
    if kind == "gn":
        graph = make_graph("cfg5")
        V, H = graph.num_nodes(), CONFIGS["cfg5"]["hidden"]
        mod = GraphNorm(H).to(dev)
    else:
        graph, (V, H) = None, (169_343, 256)
        mod = (GraphBatchNorm if kind == "bn" else GraphLayerNorm)(H).to(dev)
    X = torch.randn(V, H, generator=gen, device=dev) * (0.5 + 1.5 * torch.rand(H, generator=gen, device=dev))
    Rr = torch.randn(V, H, generator=gen, device=dev)
    dY = torch.randn(V, H, generator=gen, device=dev)
    with torch.no_grad():
        mod.weight.copy_(0.5 + torch.rand(H, generator=gen, device=dev))
        mod.bias.copy_(torch.randn(H, generator=gen, device=dev))
    mod.train()
    act, drop = nn.LeakyReLU(0.2), nn.Dropout(DROP_P)
    seed = torch.randint(0, 2 ** 62, (1,), device=dev, dtype=torch.int64)

    def step(route):
        mod.zero_grad(set_to_none=True)
        Xr, Rq = X.detach().requires_grad_(True), Rr.detach().requires_grad_(True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        if route == DROP_ROUTES[0]:
            Y = mod.forward_act(graph, Xr, act, Rq)
        elif route == DROP_ROUTES[1]:
            Y = mod.forward_act(graph, Xr, act, Rq, dropout=(seed, DROP_P))
        else:
            Y = drop(mod.forward_act(graph, Xr, act, None)) + Rq
        Y.backward(dY)
        ev[1].record()
        return ev

    print(f"{dict(bn='BatchNorm1d', ln='LayerNorm', gn='GraphNorm')[kind]} {V} x {H}"
          + (f" ({graph.batch_size} graphs, cfg5 batch; launch-bound)" if graph is not None else " (arxiv)"))
    meds = {r: [] for r in DROP_ROUTES}
    for _ in range(runs):
        times = {r: [] for r in DROP_ROUTES}
        for k in range(warmup + steps):
            for route in DROP_ROUTES:
                ev = step(route)
                torch.cuda.synchronize()
                if k >= warmup:
                    times[route].append(ev[0].elapsed_time(ev[1]))
        for r in DROP_ROUTES:
            meds[r].append(statistics.median(times[r]))
    for r in DROP_ROUTES:
        m = meds[r]
        print(f"  {r:26s} step median of the runs' medians {statistics.median(m):8.4f} ms   runs: "
              + " ".join(f"{x:.4f}" for x in m) + f"   spread {max(m) - min(m):.4f}")
    a, b, c = (statistics.median(meds[r]) for r in DROP_ROUTES)
    spread = max(max(meds[r]) - min(meds[r]) for r in DROP_ROUTES[1:])
    print(f"  (b) - (a), the cost of the hash: {b - a:+.4f} ms;  (c) - (b): {c - b:+.4f} ms, "
          f"{'above' if c - b > spread else 'NOT above'} the run-to-run spread of the two ({spread:.4f} ms);  (c) / (b) = {c / b:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", action="store_true", help="the fused layer dropout against nn.Dropout after the fused pass")
    ap.add_argument("--runs", type=int, default=5, help="--dropout: repetitions of the whole measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_bench needs the MI355X (no CPU timing is meaningful)")
    if a.steps < 20 or a.warmup < 3:
        raise SystemExit("--steps must be >= 20 (median of at least 20 steps) and --warmup >= 3")
    if a.dropout:
        print(f"norm -> LeakyReLU(0.2) -> Dropout({DROP_P}) -> + resid, training mode, fp32, forward + backward")
        print(f"device: {torch.cuda.get_device_name(0)}; per run: warm-up {a.warmup}, median of {a.steps} interleaved steps "
              f"(HIP events, a synchronise after every step), ms; {a.runs} runs")
        for kind in ("bn", "ln", "gn"):
            bench_dropout(kind, a.steps, a.warmup, a.runs)
            torch.cuda.empty_cache()
        return
    print("norm -> LeakyReLU(0.2) -> + resid, training mode, fp32: fused forward_act vs the torch chain")
    print(f"device: {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, median (min) of {a.steps} interleaved steps, ms")
    slower = []
    for V, H, what in SHAPES:
        for kind in ("bn", "ln"):
            print(f"{'BatchNorm1d' if kind == 'bn' else 'LayerNorm'} {V} x {H} ({what})")
            ratio = bench(kind, V, H, a.steps, a.warmup)
            if V >= 169_343 and ratio < 1.0:
                slower.append((kind, V, H, ratio))
            torch.cuda.empty_cache()
    print("gradient differences above 1e-6 between the routes are attributed (not separately measured) to LeakyReLU gates "
          "of the few elements whose y lies within the routes' rounding difference (the `out` figure) of 0")
    print("fused slower than the torch chain at a gated shape: " + (", ".join(map(str, slower)) if slower else "none"))


if __name__ == "__main__":
    main()
