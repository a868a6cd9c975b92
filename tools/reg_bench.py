#!/usr/bin/env python3
"""The L1 / L2 parameter penalty per call: the native multi-tensor passes (``sirgcn.param_norms``:
``sir_param_norms_fwd`` / ``_bwd``) against the torch composition of the same two sums and their backward,
written from the formula (per tensor ``abs().sum()`` and ``pow(2).sum()``, stacked and summed), on IDENTICAL
parameters, the routes interleaved in ONE process and timed with HIP events around each whole call (forward
and ``torch.autograd.grad`` of both sums to every parameter; host work included).

Parameter sets:
  cfg2     the parameters of ``workloads.make_stack("cfg2", SIRConv, GraphBatchNorm)``;
  prenorm  a ``PreNormSIRModel`` at H = 512 with 5 layers.
Modes: eager, and the same call captured in a HIP graph and replayed.  Also: a whole cfg2 training step
(bf16 autocast forward, loss + penalty, backward) with the penalty on each route, eager.

Warm-up, then --runs runs of --steps interleaved steps; reported per route: the median over runs of each run's
median, and the spread (max - min) of the runs' medians.  For the large set the native entries' own device
time (events around each entry) is set against the bytes the algorithm moves (forward 4 B per element read,
backward 4 B read and 4 B written).  Gate (cfg2, eager): native is below torch by more than the larger of the
two spreads; the other figures are recorded only.

    python tools/reg_bench.py > profiles/reg_bench.txt
    rocprofv3 --kernel-trace --stats ... -- python tools/reg_bench.py --count-launches native --iters 20
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402

import sirgcn  # noqa: E402
from sirgcn import GraphBatchNorm, PreNormSIRModel, SIRConv, _native, workloads  # noqa: E402

DEV = "cuda:0"
ROUTES = ("native", "torch")


def composed(params):
    l1 = torch.stack([p.abs().sum() for p in params]).sum()
    l2 = torch.stack([p.pow(2).sum() for p in params]).sum()
    return l1, l2


NORMS = {"native": sirgcn.param_norms, "torch": composed}


def build_set(name):
    if name == "cfg2":
        model = workloads.make_stack("cfg2", SIRConv, GraphBatchNorm).to(DEV)
    else:
        torch.manual_seed(0)
        model = PreNormSIRModel(300, 512, 18, num_layers=5, input_dropout=0.2, dropout=0.2, norm="ln", residual=True,
                                feat_dropout=0.2, agg_type="sym").to(DEV)
    return model, [p for p in model.parameters()]


def call(route, params, g):
    """One whole call: both sums and their gradients.  The sums are returned DETACHED: a kept output would keep
    the autograd graph and with it the parameters' AccumulateGrad nodes alive on the stream that made them, and
    a later backward on another stream (the capture) would have to synchronise with that stream."""
    l = NORMS[route](params)
    grads = torch.autograd.grad(l, params, g)
    return tuple(x.detach() for x in l), grads


def eager_runner(route, params, g):
    def run():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        call(route, params, g)
        ev[1].record()
        return ev
    return run


def captured_runner(route, params, g):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call(route, params, g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        keep = call(route, params, g)

    def run():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        cg.replay()
        ev[1].record()
        return ev
    run.keep = keep
    return run


def measure(runners, steps, warmup, runs):
    """{route: [median time of each run, ms]}, the routes interleaved step by step."""
    meds = {name: [] for name in runners}
    for _ in range(runs):
        times = {name: [] for name in runners}
        for k in range(warmup + steps):
            for name, run in runners.items():
                ev = run()
                torch.cuda.synchronize()
                if k >= warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]))
        for name in runners:
            meds[name].append(statistics.median(times[name]))
    return meds


def report(label, meds):
    res = {}
    for name, m in meds.items():
        res[name] = (statistics.median(m), max(m) - min(m))
        print(f"  {label:24s} {name:7s} {res[name][0]:9.4f} ms  spread {res[name][1]:7.4f} ms  (runs: "
              + " ".join(f"{x:.4f}" for x in m) + ")")
    n, t = res["native"][0], res["torch"][0]
    spread = max(res["native"][1], res["torch"][1])
    print(f"  {label:24s} torch - native = {t - n:+.4f} ms, larger spread {spread:.4f} ms: "
          + ("native is faster beyond the spread" if t - n > spread else "NOT beyond the spread")
          + f";  torch / native = {t / n:.2f}")
    return t - n > spread


def entry_times(params, g, iters):
    """Median device time of each native entry alone (HIP events around the entry), ms."""
    rec = _native.enable_timing(True)
    for _ in range(iters):
        call("native", params, g)
    torch.cuda.synchronize()
    _native.enable_timing(False)
    return {k: statistics.median(s.elapsed_time(e) for s, e, _ in v) for k, v in rec.items()
            if k.startswith("sir_param_norms")}


def train_step_runner(route, stack, graph, X, dY, params, weights):
    def run():
        stack.zero_grad(set_to_none=True)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            Y = stack(graph, X)
        l1, l2 = NORMS[route](params)
        loss = (Y.float() * dY).mean() + (weights[0] * l1 + weights[1] * l2)
        loss.backward()
        ev[1].record()
        return ev
    return run


def count_launches(route, which, iters):
    """For a profiler run of its own: the set-up, then ``iters`` calls of one route and nothing else."""
    _, params = build_set(which)
    g = (torch.tensor(0.3, device=DEV), torch.tensor(0.7, device=DEV))
    torch.cuda.synchronize()
    for _ in range(iters):
        call(route, params, g)
    torch.cuda.synchronize()
    print(f"count-launches: route {route}, set {which}, {len(params)} tensors, {iters} calls after the set-up")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count-launches", choices=ROUTES, default=None)
    ap.add_argument("--set", default="cfg2", choices=("cfg2", "prenorm"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reg_bench needs the MI355X (no CPU timing is meaningful)")
    if a.count_launches:
        return count_launches(a.count_launches, a.set, a.iters)
    if a.runs < 3 or a.steps < 10 or a.warmup < 2:
        raise SystemExit("--runs must be >= 3, --steps >= 10 and --warmup >= 2")
    print("L1 / L2 parameter penalty per call (both sums and their gradients to every parameter): native = "
          "sirgcn.param_norms (sir_param_norms_fwd / _bwd), torch = per-tensor abs().sum() / pow(2).sum(), stacked and "
          "summed, and autograd through it")
    print(f"device: {torch.cuda.get_device_name(0)}; HIP events around each whole call (host work included, a synchronise "
          f"after every call); warm-up {a.warmup}, then {a.runs} runs of {a.steps} interleaved steps: median over runs of "
          "each run's median, spread = max - min of the runs' medians")
    g = (torch.tensor(0.3, device=DEV), torch.tensor(0.7, device=DEV))
    gate = None
    for which in ("cfg2", "prenorm"):
        model, params = build_set(which)
        n = sum(p.numel() for p in params)
        print(f"{which}: {len(params)} parameter tensors, {n} elements"
              + ("" if which == "cfg2" else "  (recorded, not gated)"))
        a_out, b_out = call("native", params, g), call("torch", params, g)       # same gradients, bit for bit
        assert sirgcn.param_norms.last_route == "native"
        assert all(torch.equal(x, y) for x, y in zip(a_out[1], b_out[1]))
        del a_out, b_out
        ok = report("fwd+bwd, eager", measure({r: eager_runner(r, params, g) for r in ROUTES}, a.steps, a.warmup, a.runs))
        if which == "cfg2":
            gate = ok
        report("fwd+bwd, captured", measure({r: captured_runner(r, params, g) for r in ROUTES}, a.steps, a.warmup, a.runs))
        ent = entry_times(params, g, a.steps)
        for k, by in (("sir_param_norms_fwd", 4 * n), ("sir_param_norms_bwd", 8 * n)):
            ms = ent[k]
            print(f"  {k} alone (device events around the entry): {ms:.4f} ms; {by / 1e6:.2f} MB by the algorithm -> "
                  f"{by / (ms * 1e-3) / 1e9:.1f} GB/s ({100 * by / (ms * 1e-3) / 6.3e12:.1f} % of the 6.3 TB/s float4 copy)")
        del model, params
        torch.cuda.empty_cache()
    train_step(a)
    print("gate cfg2 fwd+bwd eager: " + ("native is faster beyond the spread" if gate else "NOT MET"))
    if not gate:
        raise SystemExit(1)


def train_step(a):
    """The whole cfg2 training step with the penalty on each route."""
    graph = workloads.make_graph("cfg2").to(DEV)
    stack = workloads.make_stack("cfg2", SIRConv, GraphBatchNorm).to(DEV).train()
    X, dY = workloads.make_inputs("cfg2", graph.num_nodes(), DEV)
    params = list(stack.parameters())
    print(f"cfg2 training step (bf16 autocast forward, loss + 1e-7 * (l1 + l2), backward; V = {graph.num_nodes()}, "
          f"E = {graph.num_edges()}), eager  (recorded, not gated)")
    runners = {r: train_step_runner(r, stack, graph, X, dY, params, (1e-7, 1e-7)) for r in ROUTES}
    report("training step, eager", measure(runners, a.steps, a.warmup, a.runs))


if __name__ == "__main__":
    main()
