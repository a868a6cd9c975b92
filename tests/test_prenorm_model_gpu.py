"""``sirgcn.PreNormSIRModel`` — the pre-norm residual block of the reference's heterophilous configs
(``heterophilous-datasets/model.py:12-55``) on the MI355X, against fixtures produced by the reference's own model
(``tests/golden/make_golden_prenorm.py``: one training-mode step without dropout, in fp32 and in fp64).

* every fixture case: the reference's state_dict loads, and the output, dX, every parameter gradient and the
  BatchNorm buffers pass ``conftest.assert_parity`` (1e-5, or the reference's own fp32 error against fp64; envelope
  factor 4 for the 2-layer cases, as for the multi-layer stacks of tests/test_stacks_gpu.py; with ``bn`` the
  gradient of ``linears[i].bias`` is zero in exact arithmetic — the next BatchNorm removes a constant shift — so
  there the reference's fp32 and fp64 values are both rounding noise and the envelope is what compares them);
* with the dropouts on, the model equals at 1e-5 the loop composed by hand from SIRConv, GetNorm, linalg.linear
  and the explicit masks of ``model.site_seeds``, the convs handed the step's own seed words;
* autocast steps against the fixture's fp64 values, at the bars of the autocast stacks;
* a captured training step draws fresh masks on every replay.
"""
import json
import os

import pytest
import torch
from torch import nn

from conftest import GOLDEN, assert_close, assert_parity, load_case, rel_err

import sirgcn
import sirgcn.conv as sc
from sirgcn import Graph, PreNormSIRModel, _native, linalg

pytestmark = pytest.mark.gpu
DEV = "cuda"

with open(os.path.join(GOLDEN, "prenorm_manifest.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
DROP_CASE = "prenorm_ln_sym_l2_res"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _load(name, **kw):
    """(model on the GPU with the fixture's state_dict, graph, X, dY, the fixture's arrays)."""
    c, z = CASES[name], load_case(name)
    model = PreNormSIRModel(c["input_dim"], c["hidden_dim"], c["output_dim"], num_layers=c["num_layers"],
                            norm=c["norm"], residual=c["residual"], agg_type=c["agg"], **kw)
    assert list(model.state_dict().keys()) == c["state_keys"]
    model.load_state_dict({k: torch.from_numpy(z["s." + k]) for k in c["state_keys"]})
    graph = Graph(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), c["V"])
    return model.to(DEV).train(), graph, torch.from_numpy(z["X"]).to(DEV), torch.from_numpy(z["dY"]).to(DEV), z


def _step(model, fn, X, dY, autocast=None):
    model.zero_grad(set_to_none=True)
    x = X.clone().requires_grad_(True)
    if autocast is not None:
        with torch.autocast("cuda", dtype=autocast):
            y = fn(x)
    else:
        y = fn(x)
    y.float().backward(dY)
    return y.detach(), x.grad, {k: q.grad.clone() for k, q in model.named_parameters()}


def _check_fixture(name, got, model, z, what):
    c = CASES[name]
    factor = 4.0 if c["num_layers"] > 1 else 2.0
    assert got[0].shape == z["Y32"].shape                                          # squeeze(1)
    assert_parity(got[0], z["Y32"], z["Y64"], what=f"{what} Y", factor=factor)
    assert_parity(got[1], z["dX32"], z["dX64"], what=f"{what} dX", factor=factor)
    assert list(got[2].keys()) == c["param_keys"]
    for k in c["param_keys"]:
        assert_parity(got[2][k], z["g32." + k], z["g64." + k], what=f"{what} d{k}", factor=factor)
    bufs = dict(model.named_buffers())
    assert list(bufs.keys()) == c["buffer_keys"]
    for k in c["buffer_keys"]:
        assert_parity(bufs[k].double(), z["b32." + k].astype("float64"), z["b64." + k].astype("float64"),
                      what=f"{what} {k}", factor=factor)


# ------------------------------------------------------------------ the reference's own step
@pytest.mark.parametrize("name", list(CASES))
def test_fixture_parity(name, monkeypatch):
    model, graph, X, dY, z = _load(name)
    calls = []
    orig = _native.drop_act_fwd
    monkeypatch.setattr(_native, "drop_act_fwd", lambda *a, **k: calls.append(1) or orig(*a, **k))
    got = _step(model, lambda x: model(graph, x), X, dY)
    assert len(calls) == 2 * CASES[name]["num_layers"] + 1, "every site runs the native pass"
    assert model.site_seeds is None                                                # nothing to draw
    _check_fixture(name, got, model, z, name)


@pytest.mark.parametrize("name", ["prenorm_bn_mean_l2_res", "prenorm_ln_max_l1_res", "prenorm_ln_mean_l2_nores_o1"])
def test_unfused_tail_gives_the_same_values(name, monkeypatch):
    """``fused_tail = False``: torch's dropout, activation and add — the fixture's values again, and no native pass."""
    model, graph, X, dY, z = _load(name)
    fused = _step(model, lambda x: model(graph, x), X, dY)
    model2, *_ = _load(name)
    model2.fused_tail = False
    monkeypatch.setattr(_native, "drop_act_fwd", lambda *a, **k: pytest.fail("fused_tail = False ran the native pass"))
    got = _step(model2, lambda x: model2(graph, x), X, dY)
    _check_fixture(name, got, model2, z, name + " unfused")
    assert_close(got[0], fused[0], 1e-5, "unfused vs fused Y")


def test_eval_mode_gives_the_values_without_dropout():
    plain, graph, X, dY, z = _load(DROP_CASE)
    model, *_ = _load(DROP_CASE, input_dropout=0.2, dropout=0.2, feat_dropout=0.2)
    want = plain.eval()(graph, X)
    assert torch.equal(model.eval()(graph, X), want) and model.site_seeds is None
    model.fused_tail = False
    assert_close(model(graph, X), want, 1e-5, "eval, unfused")


# ------------------------------------------------------------------ dropouts on
def _mask(M, N, seed, p):
    return _native.dropout_apply(torch.ones(M, N, device=DEV), (seed, p))


def _drop(h, m):
    return torch.where(m != 0, h * m, 0.0).to(h.dtype)


def _composed(model, graph, x, masks, conv_words):
    """The reference's loop by hand: explicit masks at the three sites, the convs handed their seed words."""
    h = model.activation(_drop(linalg.linear(x, model.input_linear.weight, model.input_linear.bias), masks[0]))
    for i in range(model.num_layers):
        r = h
        h = model.norms[i](h)
        model.convs[i].step_seed = torch.tensor([conv_words[i]], dtype=torch.int64, device=DEV)
        h = model.convs[i](graph, h)
        h = model.activation(_drop(h, masks[2 * i + 1]))
        h = _drop(linalg.linear(h, model.linears[i].weight, model.linears[i].bias), masks[2 * i + 2])
        if model.residual:
            h = h + r
    h = model.output_norm(h)
    return linalg.linear(h, model.output_linear.weight, model.output_linear.bias).squeeze(1)


def _trace_seeds(monkeypatch):
    draws, conv_seeds = [], []
    orig = torch.randint
    monkeypatch.setattr(torch, "randint", lambda *a, **k: draws.append(orig(*a, **k)) or draws[-1])
    orig_drop = sc.SIRConv._drop
    monkeypatch.setattr(sc.SIRConv, "_drop", lambda self, dev: conv_seeds.append(orig_drop(self, dev)) or conv_seeds[-1])
    return draws, conv_seeds


@pytest.mark.parametrize("name", [DROP_CASE, "prenorm_none_mean_l2_res"])
def test_dropouts_on_equal_the_hand_composed_loop(name, monkeypatch):
    model, graph, X, dY, _ = _load(name, input_dropout=0.2, dropout=0.2, feat_dropout=0.2)
    V, H, L = X.shape[0], CASES[name]["hidden_dim"], model.num_layers
    draws, conv_seeds = _trace_seeds(monkeypatch)
    got = _step(model, lambda x: model(graph, x), X, dY)
    # one draw for the whole step: the convs' words, then the sites'
    assert [d.numel() for d in draws] == [L + 2 * L + 1]
    conv_words = [int(s[0].item()) for s in conv_seeds]
    site_words = model.site_seeds.tolist()
    assert len(conv_words) == L and len(site_words) == 2 * L + 1
    assert len(set(conv_words + site_words)) == 3 * L + 1
    assert all(w >> 62 == 1 for w in site_words) and all(w < 2 ** 62 for w in conv_words)
    masks = [_mask(V, H, w, 0.2) for w in site_words]
    assert all(0 < int((m == 0).sum()) < m.numel() for m in masks)
    del draws[:]
    want = _step(model, lambda x: _composed(model, graph, x, masks, conv_words), X, dY)
    assert draws == [], "a handed-in seed word needs no draw"
    assert_close(got[0], want[0], 1e-5, "Y")
    assert_close(got[1], want[1], 1e-5, "dX")
    assert got[2].keys() == want[2].keys()
    for k in want[2]:
        assert_close(got[2][k], want[2][k], 1e-5, f"d{k}")
    # the next step draws again
    y2 = model(graph, X)
    assert model.site_seeds.tolist() != site_words and not torch.equal(y2, got[0])


def test_sites_without_a_code_or_with_a_hook_run_torch(monkeypatch):
    model, graph, X, dY, _ = _load(DROP_CASE, input_dropout=0.2, dropout=0.2)
    calls = []
    orig = _native.drop_act_fwd
    monkeypatch.setattr(_native, "drop_act_fwd", lambda *a, **k: calls.append(1) or orig(*a, **k))
    model.activation = nn.Tanh()                      # not one of the five: sites 0, 1 and 3 on torch's ops
    hits = []
    model.drop.register_forward_hook(lambda mod, args, out: hits.append(1))
    model.input_drop.register_forward_hook(lambda mod, args, out: hits.append(1))
    y = model(graph, X)
    assert torch.isfinite(y).all() and calls == [] and len(hits) == 5      # a hooked nn.Dropout is called, too


# ------------------------------------------------------------------ autocast
@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 2e-2), (torch.float16, 1e-2)], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", [DROP_CASE, "prenorm_ln_max_l1_res", "prenorm_none_mean_l2_res"])
def test_autocast_step(name, dt, tol, monkeypatch):
    """Relative L2 against the reference's fp64 step within 2e-2 (bf16) / 1e-2 (fp16), or no worse than 1.25x the
    error of the ``fused_tail = False`` route under the same autocast."""
    model, graph, X, dY, z = _load(name)
    seen = []
    orig = _native.drop_act_fwd
    monkeypatch.setattr(_native, "drop_act_fwd", lambda Y, *a, **k: seen.append(Y.dtype) or orig(Y, *a, **k))
    got = _step(model, lambda x: model(graph, x), X, dY, autocast=dt)
    assert seen == [dt] * (2 * model.num_layers + 1), seen             # the feats stay 16-bit through the loop
    model.fused_tail = False
    base = _step(model, lambda x: model(graph, x), X, dY, autocast=dt)
    c = CASES[name]
    triples = [("Y", got[0], base[0], z["Y64"]), ("dX", got[1], base[1], z["dX64"])] + \
              [(k, got[2][k], base[2][k], z["g64." + k]) for k in c["param_keys"]]
    for what, a, b, t in triples:
        assert torch.isfinite(a).all(), what
        e, e_base = rel_err(a.double().cpu(), t), rel_err(b.double().cpu(), t)
        print(f"{name} {dt} {what}: {e:.3e} (unfused {e_base:.3e})")
        assert e <= max(tol, 1.25 * e_base), (what, e, e_base)


# ------------------------------------------------------------------ graph capture
def test_captured_training_step_draws_fresh_masks_per_replay():
    """The seed words are drawn on the device inside the capture: two replays use different masks, and within a
    replay the forward and the backward agree (they equal the composed step on that replay's own words)."""
    name = DROP_CASE
    model, graph, X, dY, _ = _load(name, input_dropout=0.2, dropout=0.2)
    V, H = X.shape[0], CASES[name]["hidden_dim"]
    x = X.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up (plans, packs) outside the capture
        for _ in range(2):
            model.zero_grad(set_to_none=False)
            x.grad = None
            model(graph, x).backward(dY)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    x.grad = torch.zeros_like(x)
    model.zero_grad(set_to_none=False)
    with torch.cuda.graph(cg):
        Y = model(graph, x)
        Y.backward(dY)
    words = model.site_seeds
    outs = []
    for _ in range(2):
        x.grad.zero_()
        cg.replay()
        torch.cuda.synchronize()
        outs.append((words.clone(), Y.detach().clone(), x.grad.clone()))
    assert not torch.equal(outs[0][0], outs[1][0]), "the captured seed draw must run again on replay"
    assert not torch.equal(outs[0][1], outs[1][1]), "two replays must use two different masks"
    assert all(w >> 62 == 1 for w in outs[1][0].tolist())
    masks = [_mask(V, H, w, 0.2) for w in outs[1][0].tolist()]
    x2 = X.clone().requires_grad_(True)
    Y2 = _composed(model, graph, x2, masks, [0] * model.num_layers)      # feat_dropout = 0: the convs draw nothing
    Y2.backward(dY)
    assert_close(outs[1][1], Y2.detach(), 1e-5, "replayed Y")
    assert_close(outs[1][2], x2.grad, 1e-5, "replayed dX")


def test_exported():
    assert sirgcn.PreNormSIRModel is PreNormSIRModel and PreNormSIRModel.fused_tail is True
