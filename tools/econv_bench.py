#!/usr/bin/env python3
"""Fused vs edge-materialised SIREConv, forward + backward, interleaved in ONE process on identical data
(cdna_hip_programming.md §5.4 rule 24), timed with HIP events: warm-up, then the median of --steps steps.

    python tools/econv_bench.py                      # V = 200 000, E = 4 000 000, H = 256, de = 16, sum, LeakyReLU
    python tools/econv_bench.py > profiles/econv_fused_vs_legacy.txt

Also reports the two new kernels' own times (HIP events around the native calls), the forward kernel's
design bytes per edge (2 * H * 4 gathered K and Eh rows + the sign mask + the col / eidx indices) with the
rate they imply, and the plain SIRConv forward (sir_edge_agg_fwd, one gathered row per edge) on the same
plan and Q / K for scale."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from sirgcn import SIREConv, _native  # noqa: E402
from sirgcn.graph import Graph, get_plan  # noqa: E402
from sirgcn.synth import powerlaw_edges  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=200_000)
    ap.add_argument("--E", type=int, default=4_000_000)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--de", type=int, default=16)
    ap.add_argument("--out", type=int, default=64)
    ap.add_argument("--alpha", type=float, default=0.8, help="power-law exponent of the synthetic graph (0 = uniform)")
    ap.add_argument("--agg", default="sum", choices=["sum", "mean", "sym"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("econv_bench needs the MI355X (no CPU timing is meaningful)")
    if a.steps < 20 or a.warmup < 2:
        raise SystemExit("--steps must be >= 20 (median of at least 20 steps) and --warmup >= 2")
    dev = "cuda"
    V, E, H = a.V, a.E, a.H
    src, dst = powerlaw_edges(V, E, a.alpha, seed=0)
    g = Graph(src, dst, V)
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(V, a.d, generator=gen).to(dev)
    Ef = torch.randn(E, a.de, generator=gen).to(dev)
    dY = torch.randn(V, a.out, generator=gen).to(dev)
    torch.manual_seed(0)
    m = SIREConv(a.d, a.de, H, a.out, nn.LeakyReLU(0.2), 0, agg_type=a.agg).to(dev)
    plan = get_plan(g, torch.device(dev), m.chunk)
    unit = E * H * 4

    def step(fused):
        m.fused = fused
        m.zero_grad(set_to_none=True)
        Xr, Er = X.detach().requires_grad_(True), Ef.detach().requires_grad_(True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        Y = m(g, Xr, Er)
        ev[1].record()
        Y.backward(dY)
        ev[2].record()
        return ev, (Y.detach(), Xr.grad, Er.grad, m.linear_edge.weight.grad)

    routes = (("fused", True), ("edge-materialised", False))
    times = {n: {"fwd": [], "bwd": [], "step": []} for n, _ in routes}
    peak, outs = {}, {}
    for r in range(a.warmup + a.steps):
        for name, fused in routes:
            if r == a.warmup - 1:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
            ev, out = step(fused)
            torch.cuda.synchronize()
            if r == a.warmup - 1:
                peak[name] = torch.cuda.max_memory_allocated() - base
                outs[name] = [t.clone() for t in out]
            if r >= a.warmup:
                times[name]["fwd"].append(ev[0].elapsed_time(ev[1]))
                times[name]["bwd"].append(ev[1].elapsed_time(ev[2]))
                times[name]["step"].append(ev[0].elapsed_time(ev[2]))
            del out

    # the new kernels alone, and the plain forward on the same plan and rows
    rec = _native.enable_timing(True)
    for _ in range(a.steps):
        step(True)
    torch.cuda.synchronize()
    kern = {k: statistics.median(s.elapsed_time(e) for s, e, _ in v) for k, v in rec.items()}
    _native.enable_timing(False)
    QK = torch.randn(V, 2 * H, generator=gen).to(dev)
    S = torch.empty(V, H, device=dev)
    nw = _native.mask_words(H, _native.ACT_LEAKY)
    mask = torch.empty(E * nw, device=dev, dtype=torch.int64)
    n_slots = max(plan.dst.n_slots, plan.src.n_slots, 1)
    partial = torch.empty(n_slots * H, device=dev)
    in_norm, out_norm = plan.norms(a.agg)
    plain = []
    for r in range(a.warmup + a.steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _native.edge_agg_fwd(plan.dst, QK[:, :H], QK[:, H:], in_norm, out_norm, a.agg, _native.ACT_LEAKY, 0.2, S, partial,
                             mask)
        e.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            plain.append(s.elapsed_time(e))

    med = lambda xs: statistics.median(xs)
    print(f"SIREConv fused vs edge-materialised: V={V} E={E} H={H} d={a.d} de={a.de} out={a.out} agg={a.agg} "
          f"LeakyReLU(0.2) fp32, power-law alpha={a.alpha}, chunk={m.chunk}")
    print(f"device: {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, median (min) of {a.steps} interleaved steps, ms")
    for name, _ in routes:
        t = times[name]
        print(f"{name:18s} step {med(t['step']):9.3f} ({min(t['step']):9.3f})   fwd {med(t['fwd']):9.3f} "
              f"({min(t['fwd']):9.3f})   bwd {med(t['bwd']):9.3f} ({min(t['bwd']):9.3f})   "
              f"peak {peak[name] / 2**20:9.1f} MiB = {peak[name] / unit:5.2f} x E*H*4")
    f, l = med(times["fused"]["step"]), med(times["edge-materialised"]["step"])
    print(f"step time ratio edge-materialised / fused: {l / f:.2f}")
    rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm()).item()
    names = ("Y", "dX", "defeat", "dW_E")
    print("fused vs edge-materialised outputs, relative L2: "
          + ", ".join(f"{n} {rel(x, y):.2e}" for n, x, y in zip(names, outs["fused"], outs["edge-materialised"])))
    bytes_edge = 2 * H * 4 + nw * 8 + 8
    tf = kern["sir_edge_e_agg_fwd"]
    print(f"sir_edge_e_agg_fwd kernel: {tf:.3f} ms = {E / tf / 1e6:.2f} G edges/s; design bytes per edge "
          f"{bytes_edge} (2*H*4 rows + {nw * 8} mask + 8 indices) -> {E * bytes_edge / tf / 1e9:.3f} TB/s")
    tb = kern["sir_edge_e_bwd"]
    print(f"sir_edge_e_bwd kernel:     {tb:.3f} ms = {E / tb / 1e6:.2f} G edges/s; design bytes per edge "
          f"{H * 4 + nw * 8 + 4} (H*4 dE row + mask + eidx) -> {E * (H * 4 + nw * 8 + 4) / tb / 1e9:.3f} TB/s")
    if "sir_edge_agg_bwd" in kern:
        print(f"sir_edge_agg_bwd kernel (dQ + dK from the same mask): {kern['sir_edge_agg_bwd']:.3f} ms")
    tp = med(plain)
    print(f"plain sir_edge_agg_fwd (SIRConv, one gathered row per edge, same plan): {tp:.3f} ms = "
          f"{E / tp / 1e6:.2f} G edges/s; fused SIREConv forward runs at {tp / tf:.2f} of its edges/s")


if __name__ == "__main__":
    main()
