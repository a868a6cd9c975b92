#!/usr/bin/env python3
"""``sirgcn.PreNormSIRModel`` training step with its three elementwise sites on the native pass
(``fused_tail = True``: ``sirgcn.drop_act``, one launch per site and direction) against the same model with torch's
``nn.Dropout`` -> activation -> add at those sites (``fused_tail = False``), forward + backward, training mode, the
reference's dropouts (input 0.2, layer 0.2, feat 0.2), interleaved in ONE process on identical data and parameters.

    python tools/prenorm_bench.py > profiles/prenorm_bench.txt

Synthetic graphs (``sirgcn.synth.powerlaw_graph``) at about the shapes of two of the reference's heterophilous
configs; the node / edge / feature / class counts are from memory of the datasets, which are not read here.
Each shape runs in fp32 and under bf16 autocast (the reference's ``--use-amp``), eager and as a step captured in a
HIP graph.  HIP events; per run a warm-up and the median of --steps steps; --runs runs give the spread of the medians.
Launches per step of the sites are counted from the design, not measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sir-gcn_amd"))

import torch  # noqa: E402

from sirgcn import PreNormSIRModel  # noqa: E402
from sirgcn.synth import powerlaw_graph  # noqa: E402

# name: (V, directed E, alpha of the synthetic degree law, input features, classes, H, layers, agg, norm)
SHAPES = {
    "roman-empire-like": (22_700, 66_000, 0.1, 300, 18, 512, 5, "max", "ln"),
    "tolokers-like": (11_800, 1_040_000, 0.8, 10, 1, 256, 5, "sym", "ln"),
}
ROUTES = (("fused", True), ("torch", False))


def site_launches(L, residual=True):
    """Elementwise launches per training step at the 2 L + 1 sites, from the design.
    fused: one pass per site and direction, plus the one op that sets bit 62 in the sites' seed words.
    torch: dropout + GELU forward, GELU' + the mask multiply backward at the L + 1 activation sites; dropout + add
    forward and the mask multiply backward at the L residual sites (the add has no backward kernel)."""
    fused = 2 * (2 * L + 1) + 1
    plain = 4 * (L + 1) + (3 if residual else 2) * L
    return fused, plain


def build(name, dev):
    V, E, alpha, F_in, C, H, L, agg, norm = SHAPES[name]
    graph = powerlaw_graph(V, E, alpha, seed=1)
    torch.manual_seed(0)
    model = PreNormSIRModel(F_in, H, C, num_layers=L, input_dropout=0.2, dropout=0.2, norm=norm, residual=True,
                            feat_dropout=0.2, agg_type=agg).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(2)
    X = torch.randn(V, F_in, generator=gen, device=dev)
    dY = torch.randn((V, C) if C > 1 else (V,), generator=gen, device=dev)
    return model, graph, X, dY


def one_step(model, graph, X, dY, autocast):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        Y = model(graph, X)
    Y.float().backward(dY)


def eager_runner(model, graph, X, dY, autocast, fused):
    def run():
        model.fused_tail = fused
        model.zero_grad(set_to_none=True)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        one_step(model, graph, X, dY, autocast)
        ev[1].record()
        return ev
    return run


def captured_runner(model, graph, X, dY, autocast, fused):
    model.fused_tail = fused
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            model.zero_grad(set_to_none=False)
            one_step(model, graph, X, dY, autocast)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    model.zero_grad(set_to_none=False)
    with torch.cuda.graph(cg):
        one_step(model, graph, X, dY, autocast)

    def run():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        cg.replay()
        ev[1].record()
        return ev
    return run


def measure(runners, steps, warmup, runs):
    """{route: [median step time of each run, ms]}, the routes interleaved step by step."""
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


def report(meds):
    for name, m in meds.items():
        print(f"    {name:6s} step, median of the runs' medians {statistics.median(m):8.4f} ms   runs: "
              + " ".join(f"{x:.4f}" for x in m) + f"   spread {max(m) - min(m):.4f}")
    f, t = statistics.median(meds["fused"]), statistics.median(meds["torch"])
    spread = max(max(m) - min(m) for m in meds.values())
    print(f"    torch - fused: {t - f:+.4f} ms, {'above' if abs(t - f) > spread else 'NOT above'} the run-to-run spread "
          f"({spread:.4f} ms);  torch / fused = {t / f:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prenorm_bench needs the MI355X (no CPU timing is meaningful)")
    if a.steps < 20 or a.warmup < 3:
        raise SystemExit("--steps must be >= 20 (median of at least 20 steps) and --warmup >= 3")
    dev = "cuda"
    print("PreNormSIRModel training step (forward + backward; dropouts 0.2 / 0.2 / 0.2, residual): fused_tail True vs False")
    print(f"device: {torch.cuda.get_device_name(0)}; per run: warm-up {a.warmup}, median of {a.steps} interleaved steps "
          f"(HIP events, a synchronise after every step), ms; {a.runs} runs")
    print("graphs: synthetic (sirgcn.synth.powerlaw_graph); the V / E / feature / class counts are from memory of the "
          "datasets, which are not on this machine")
    for name in a.shapes:
        V, E, alpha, F_in, C, H, L, agg, norm = SHAPES[name]
        fused_n, plain_n = site_launches(L)
        print(f"{name}: V {V}, E {E}, in {F_in}, H {H}, {L} layers, {agg}, {norm}, out {C}")
        print(f"  elementwise launches per step at the {2 * L + 1} sites (from the design): fused {fused_n}, torch {plain_n}; "
              f"masks kept for the backward: fused 0, torch {2 * L + 1}")
        model, graph, X, dY = build(name, dev)
        for autocast in (False, True):
            eager = {r: eager_runner(model, graph, X, dY, autocast, f) for r, f in ROUTES}
            print(f"  {'bf16 autocast' if autocast else 'fp32'}, eager")
            report(measure(eager, a.steps, a.warmup, a.runs))
            captured = {r: captured_runner(model, graph, X, dY, autocast, f) for r, f in ROUTES}
            print(f"  {'bf16 autocast' if autocast else 'fp32'}, captured step (HIP graph replay)")
            report(measure(captured, a.steps, a.warmup, a.runs))
            del eager, captured
        del model, graph, X, dY
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
