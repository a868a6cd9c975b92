#!/usr/bin/env python3
"""Generate the pre-norm model fixtures from the REFERENCE's own ``heterophilous-datasets/model.py``.

Runs ONLY in the build container, where ``/root/reference`` (read-only) exists:

    python tests/golden/make_golden_prenorm.py     # rewrites tests/golden/prenorm_*.npz + prenorm_manifest.json

How the reference is executed
-----------------------------
* ``model.py`` is loaded with ``importlib`` from its path, unmodified, on the CPU, with ``dgl`` resolved to the
  test-only DGL-2.1.0-semantics shim of ``tests/golden/dgl_shim`` (its files stay as they are) and the reference's
  root on ``sys.path`` for its ``models`` package.  What the import needs beyond the shim is patched in at run
  time: ``dgl.transforms.DropEdge`` (``models/utils.py`` subclasses it; unused here).
* Each case builds ``SIRModel`` once in fp32 (``torch.manual_seed``; the norms' affine parameters are then moved
  off their ones / zeros), and runs one training-mode step with every dropout 0 twice from that ``state_dict``:
  in fp32 and, after ``.double()``, in fp64.  Recorded: the graph, ``X``, ``dY``, the state_dict (``s.<key>``),
  and per precision the output (``Y32`` / ``Y64``), ``dX``, every parameter gradient (``g32.<key>``) and, for
  ``bn``, the buffers after the step (``b32.<key>``).
* The ``max`` case also checks, from the per-edge messages the conv's ``linear_relation`` returns, that the fp32
  and the fp64 run choose the same arg edge for every (node, feature), and records the smallest gap between the best
  and the second-best message (``min_gap``); a seed is chosen for which that holds.

Only the produced data is committed; no reference source enters the repository.  The other manifests are not touched.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = "/root/reference"
REF = os.path.join(REF_ROOT, "benchmark-datasets", "heterophilous-datasets", "model.py")
SHIM = os.path.join(HERE, "dgl_shim")
sys.path.insert(0, HERE)
from make_golden import graph_small, graph_small_nodup  # noqa: E402  (the shared graph recipes)


def load_reference():
    sys.dont_write_bytecode = True
    for p in (REF_ROOT, SHIM):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dgl
    if not hasattr(dgl, "transforms"):
        transforms = types.ModuleType("dgl.transforms")
        transforms.DropEdge = type("DropEdge", (), {})
        dgl.transforms = transforms
        sys.modules["dgl.transforms"] = transforms
    spec = importlib.util.spec_from_file_location("ref_heterophilous_model", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, dgl


def build(ref, cfg, seed):
    torch.manual_seed(seed)
    model = ref.SIRModel(**cfg)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, q in model.named_parameters():
            if ".norm." in name or name.startswith("output_norm"):
                if name.endswith("weight"):
                    q.copy_(0.5 + torch.rand(q.shape, generator=gen))
                else:
                    q.copy_(0.5 * torch.randn(q.shape, generator=gen))
    return model.train()


def step(ref, dgl, cfg, state, src, dst, V, X, dY, dtype, trace=None):
    model = ref.SIRModel(**cfg).to(dtype)
    model.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()})
    model.train()
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=V)
    if trace is not None:
        model.convs[0].linear_relation.register_forward_hook(lambda m, a, out: trace.append(out.detach().clone()))
    x = X.to(dtype).detach().clone().requires_grad_(True)
    y = model(g, x)
    y.backward(dY.to(dtype))
    grads = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
    bufs = {k: b.detach().clone() for k, b in model.named_buffers()}
    return y.detach(), x.grad.detach(), grads, bufs


def arg_edges(msg, dst, V):
    """Per (node, feature): the arg edge of the max over in-edges (-1: no in-edge) and the gap to the second best."""
    msg = msg.double()
    arg = torch.full((V, msg.shape[1]), -1, dtype=torch.int64)
    gap = torch.full((V, msg.shape[1]), float("inf"), dtype=torch.float64)
    dst = torch.from_numpy(dst)
    for v in range(V):
        e = torch.nonzero(dst == v).flatten()
        if e.numel() == 0:
            continue
        top = msg[e].topk(min(2, e.numel()), dim=0)
        arg[v] = e[top.indices[0]]
        if e.numel() > 1:
            gap[v] = top.values[0] - top.values[1]
    return arg, gap


def case(ref, dgl, name, norm, agg, layers, residual, O, graph_fn, seed):
    V, src, dst = graph_fn()
    cfg = dict(input_dim=12, hidden_dim=32, output_dim=O, num_layers=layers, input_dropout=0, dropout=0, norm=norm,
               residual=residual, feat_dropout=0, agg_type=agg)
    meta = {"name": name, "norm": norm, "agg": agg, "num_layers": layers, "residual": residual, "V": V,
            "input_dim": 12, "hidden_dim": 32, "output_dim": O, "graph": graph_fn.__name__}
    while True:
        model = build(ref, cfg, seed)
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        gen = torch.Generator().manual_seed(seed + 2)
        X = torch.randn(V, 12, generator=gen)
        dY = torch.randn((V, O) if O > 1 else (V,), generator=gen)
        t32, t64 = ([], []) if agg == "max" else (None, None)
        r32 = step(ref, dgl, cfg, state, src, dst, V, X, dY, torch.float32, t32)
        r64 = step(ref, dgl, cfg, state, src, dst, V, X, dY, torch.float64, t64)
        if agg != "max":
            break
        a32, _ = arg_edges(t32[0], dst, V)
        a64, gap = arg_edges(t64[0], dst, V)
        if torch.equal(a32, a64):
            meta["min_gap"] = float(gap.min())
            break
        seed += 1                         # a near-tie flipped an arg edge between the precisions: another seed
    assert r32[0].shape == dY.shape
    out = {"src": src, "dst": dst, "X": X.numpy(), "dY": dY.numpy()}
    for k, v in state.items():
        out["s." + k] = v.numpy()
    for tag, r in (("32", r32), ("64", r64)):
        out["Y" + tag], out["dX" + tag] = r[0].numpy(), r[1].numpy()
        for k, v in r[2].items():
            out[f"g{tag}.{k}"] = v.numpy()
        for k, v in r[3].items():
            out[f"b{tag}.{k}"] = v.numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    meta.update(seed=seed, state_keys=list(state.keys()), param_keys=list(r32[2].keys()),
                buffer_keys=list(r32[3].keys()), keys=sorted(out.keys()))
    return meta


def main():
    ref, dgl = load_reference()
    cases = []
    seed = 7000
    for norm in ("ln", "bn", "none"):
        for agg in ("sym", "mean"):
            seed += 10
            cases.append(case(ref, dgl, f"prenorm_{norm}_{agg}_l2_res", norm, agg, 2, True, 3, graph_small, seed))
    cases.append(case(ref, dgl, "prenorm_ln_mean_l2_nores_o1", "ln", "mean", 2, False, 1, graph_small, 7100))
    cases.append(case(ref, dgl, "prenorm_ln_max_l1_res", "ln", "max", 1, True, 3, graph_small_nodup, 7200))
    with open(os.path.join(HERE, "prenorm_manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_prenorm.py",
                   "reference": "briangodwinlim/SIR-GCN benchmark-datasets/heterophilous-datasets/model.py:12-55 "
                                "(SIRModel), via DGL-2.1.0 semantics shim",
                   "torch": torch.__version__, "cases": cases}, f, indent=1)
    print(f"wrote {len(cases)} cases")


if __name__ == "__main__":
    main()
