#!/usr/bin/env python3
"""Generate the Correct & Smooth fixtures from the REFERENCE's own ``ogbn-arxiv/correct_and_smooth.py``.

Runs ONLY in the build container, where ``/root/reference`` (read-only) exists:

    python tests/golden/make_golden_cs.py        # rewrites tests/golden/cs_*.npz + cs_manifest.json

How the reference is executed
-----------------------------
* The file is loaded with ``importlib`` from its path, unmodified, on the CPU, with ``dgl`` resolved to the
  test-only DGL-2.1.0-semantics shim of ``tests/golden/dgl_shim`` (its files stay as they are).  What the
  script needs beyond the shim is patched in at run time: ``dgl.function.copy_u`` (the message ``m`` is the
  source's field ``u``), ``DGLGraph.number_of_nodes`` (DGL's alias of ``num_nodes``), and stub ``ogb`` /
  ``ogb.nodeproppred`` modules (the script imports the dataset and evaluator classes; neither is used here).
* ``label_spreading`` is called as ``run()`` calls it: ``partial(fix_input, y=..., mask=...)`` and
  ``lambda x: x.clamp(lo, hi)`` as post steps.
* ``run()`` is called with a stub evaluator and ``save_pred=True``; ``smoothed_y`` is read back from the file it
  saves (a relative ``pred_0.pt`` inside a temporary working directory: the script replaces every ``_`` of
  the path).  ``labels`` is [V, 1] and covers every class (``run()`` counts the classes with ``torch.unique``).

Only the produced data is committed; no reference source enters the repository.  ``manifest.json`` (the
fixtures of make_golden.py) is not touched.
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/benchmark-datasets/ogbn-arxiv/correct_and_smooth.py"
SHIM = os.path.join(HERE, "dgl_shim")


def load_reference():
    sys.dont_write_bytecode = True
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import dgl
    dgl.function.copy_u = lambda u, m: (lambda edges: {m: edges.src[u]})
    dgl.DGLGraph.number_of_nodes = dgl.DGLGraph.num_nodes
    ogb = types.ModuleType("ogb")
    npp = types.ModuleType("ogb.nodeproppred")
    npp.DglNodePropPredDataset = npp.Evaluator = object
    ogb.nodeproppred = npp
    sys.modules.setdefault("ogb", ogb)
    sys.modules.setdefault("ogb.nodeproppred", npp)
    spec = importlib.util.spec_from_file_location("ref_correct_and_smooth", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, dgl


def cs_graph(V, E, hub, n_hub, seed):
    """Random directed graph with self-loops, duplicate edges, node V - 1 without in-edges and ``hub`` with
    ``n_hub`` in-edges (a split row under the plan's chunk of 256) and only two out-edges, so that most rows
    are not downstream of it within a few steps."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, V, size=E)
    dst = rng.integers(0, V - 1, size=E)                         # node V - 1: no in-edge
    src, dst = list(src), list(dst)
    src += list(rng.integers(0, V, size=n_hub)); dst += [hub] * n_hub
    loops = rng.integers(0, V - 1, size=V // 6)
    src += list(loops); dst += list(loops)                       # self-loops
    dup = rng.integers(0, len(src), size=V // 4)
    src += [src[i] for i in dup]; dst += [dst[i] for i in dup]   # duplicate edges
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    keep = np.ones(src.size, bool)
    keep[np.nonzero((src == hub) & (dst != hub))[0][2:]] = False  # the hub keeps two out-edges (and its loops)
    src, dst = src[keep], dst[keep]
    perm = rng.permutation(src.size)
    return src[perm], dst[perm]


def spread_case(ref, dgl, name, V, F, agg, post, nprop, alpha, seed):
    src, dst = cs_graph(V, 3 * V, hub=5, n_hub=700, seed=seed)
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=V)
    gen = torch.Generator().manual_seed(seed + 1)
    y0 = torch.randn(V, F, generator=gen)
    out = {"src": src, "dst": dst, "y0": y0.numpy().copy()}
    meta = {"name": name, "kind": "spread", "V": V, "F": F, "agg": agg, "post": post, "nprop": nprop, "alpha": alpha,
            "seed": seed}
    post_step = None
    if post == "clamp":
        meta["lo"], meta["hi"] = -0.25, 0.5
        post_step = lambda x: x.clamp(-0.25, 0.5)  # noqa: E731
    elif post == "fix":
        yfix = torch.randn(V, F, generator=gen)
        idx = torch.nonzero(torch.rand(V, generator=gen) < 0.5).flatten()
        out["yfix"], out["idx"] = yfix.numpy().copy(), idx.numpy().copy()
        post_step = partial(ref.fix_input, y=yfix, mask=idx)
    y = ref.label_spreading(g, y0, nprop=nprop, alpha=alpha, use_sym=(agg == "sym"), post_step=post_step)
    assert torch.equal(y0, torch.from_numpy(out["y0"]))
    out["y"] = y.numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    meta["keys"] = sorted(out.keys())
    return meta


class _Evaluator:
    def eval(self, d):
        return {"acc": float((d["y_pred"] == d["y_true"]).float().mean())}


def run_case(ref, dgl, name, V, C, use_sym, alpha_c, nprop_c, alpha_s, nprop_s, seed):
    src, dst = cs_graph(V, 3 * V, hub=5, n_hub=700, seed=seed)
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=V)
    gen = torch.Generator().manual_seed(seed + 1)
    predictions = torch.softmax(torch.randn(V, C, generator=gen), dim=-1)
    labels = torch.randint(0, C, (V, 1), generator=gen)
    labels[:C, 0] = torch.arange(C)                              # every class present
    order = torch.randperm(V, generator=gen)
    masks = (order[:V // 2].sort().values, order[V // 2:3 * V // 4], order[3 * V // 4:])
    args = argparse.Namespace(alpha_c=alpha_c, nprop_c=nprop_c, alpha_s=alpha_s, nprop_s=nprop_s, use_sym=use_sym,
                              save_pred=True)
    keep = predictions.clone()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            ref.run(g, predictions, labels, masks, torch.device("cpu"), _Evaluator(), args, "pred_0.pt")
            smoothed = torch.load("pred_cs_0.pt")
        finally:
            os.chdir(cwd)
    assert torch.equal(predictions, keep)
    out = {"src": src, "dst": dst, "predictions": predictions.numpy(), "labels": labels.numpy(),
           "train_idx": masks[0].numpy(), "smoothed_y": smoothed.numpy()}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    return {"name": name, "kind": "run", "V": V, "F": C, "use_sym": use_sym, "alpha_c": alpha_c, "nprop_c": nprop_c,
            "alpha_s": alpha_s, "nprop_s": nprop_s, "seed": seed, "keys": sorted(out.keys())}


def main():
    ref, dgl = load_reference()
    cases = []
    seed = 4000
    for agg in ("sym", "mean"):
        for post in ("none", "clamp", "fix"):
            for nprop in (1, 3):
                seed += 10
                V, F = (72, 40) if nprop == 1 else (60, 10)
                cases.append(spread_case(ref, dgl, f"cs_spread_{agg}_{post}_n{nprop}", V, F, agg, post, nprop, 0.8, seed))
    cases.append(run_case(ref, dgl, "cs_run_sym_c40", 300, 40, True, 0.8, 3, 0.8, 3, 5001))
    cases.append(run_case(ref, dgl, "cs_run_mean_c10", 150, 10, False, 0.9, 2, 0.7, 4, 5002))
    with open(os.path.join(HERE, "cs_manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_cs.py",
                   "reference": "briangodwinlim/SIR-GCN ogbn-arxiv/correct_and_smooth.py:41-63,76-111, via DGL-2.1.0 "
                                "semantics shim",
                   "torch": torch.__version__, "cases": cases}, f, indent=1)
    print(f"wrote {len(cases)} cases")


if __name__ == "__main__":
    main()
