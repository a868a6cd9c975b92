#!/usr/bin/env python3
"""Fused BatchNorm / LayerNorm -> LeakyReLU(0.2) -> + resid (``GraphBatchNorm.forward_act`` /
``GraphLayerNorm.forward_act``) against the torch chain ``nn.BatchNorm1d`` / ``nn.LayerNorm`` ->
``nn.LeakyReLU(0.2)`` -> ``+ resid`` — what a stack with these norms ran before — forward + backward,
training mode, interleaved in ONE process on identical data, timed with HIP events: warm-up, then the
median and min of --steps steps.

    python tools/norm_bench.py > profiles/norm_fused_vs_torch.txt

Per shape and norm: each route's step / forward / backward time, its design bytes (passes over a
V*H*4-byte tensor) over its step time against the 6.3 TB/s achievable HBM rate, the peak memory of one
step, and the relative L2 difference of the two routes' outputs and gradients."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from sirgcn import GraphBatchNorm, GraphLayerNorm  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_bench needs the MI355X (no CPU timing is meaningful)")
    if a.steps < 20 or a.warmup < 3:
        raise SystemExit("--steps must be >= 20 (median of at least 20 steps) and --warmup >= 3")
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
