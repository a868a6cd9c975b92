"""Every activation code the kernels are instantiated for, launched on every kernel that takes one.

The rest of the suite is deep on ReLU / LeakyReLU (exact arithmetic, poison, sign mask); this file runs the codes
it leaves out — Identity, erf-GELU and tanh-GELU on the sum / mean / sym edge kernels at every width class (their
backward is always the two-pass recompute form), and all ten act1 x act2 forms of the fused per-edge MLP — each
against the fp64 oracle of the same operation at the suite's existing bars.  The code list comes from the
library's first and last code (tests/activation_cases.py), so a new code cannot arrive untested.  The max
forms' share of the matrix lives with their own tests (tests/test_edgemlp_gpu.py, tests/test_amp_gpu.py)."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
import torch.nn.functional as F

import activation_cases as ac
import exact_cases as xc
import oracle
from conftest import assert_parity, load_case, rel_err, tie_conditioned
from test_edgemlp_gpu import _graph, _no_generic, _oracle, _run, _tie_condition

from sirgcn import SIRConv, _native, edgemlp
from sirgcn.conv import EdgeAggregate, edge_backward
from sirgcn.edgemlp import EdgeMLPSum, _elementwise_code
from sirgcn.graph import Graph, GraphPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
NAN = float("nan")
NAME = ac.ORACLE_NAME
_PLANS = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _sweep_plan(H, agg, chunk):
    """One plan per (graph, chunk) of the sweep (the graph depends on the seed, i.e. on H and the agg's length)."""
    key = ("sweep", H, len(agg), chunk)
    if key not in _PLANS:
        src, dst, V = ac.edge_inputs(H, agg)[:3]
        _PLANS[key] = GraphPlan(src, dst, V, DEV, chunk=chunk)
    return _PLANS[key]


def _last(key, fn):
    """A one-entry cache: the cases that share a reference follow each other (chunk varies fastest)."""
    if _REF.get("key") != key:
        _REF.clear()
        _REF.update(key=key, value=fn())
    return _REF["value"]


# ----------------------------------------------------------------------------- (a) edge kernels, kernel level
def _sweep_reference(H, agg, code):
    def make():
        src, dst, V, Q, K, dS = ac.edge_inputs(H, agg)
        name, slope = NAME[code], ac.slope_of(code)
        out = []
        for f in (lambda t: t, lambda t: t.double()):
            q, k, g = f(Q), f(K), f(dS)
            out.append((oracle.edge_agg_fwd(src, dst, V, q, k, agg, name, slope),)
                       + oracle.edge_agg_bwd(src, dst, V, q, k, g, agg, name, slope))
        return out
    return _last(("f32", H, agg, code), make)


@pytest.mark.parametrize("chunk", ac.EDGE_CHUNKS)          # the topmost parameter varies fastest (see _last)
@pytest.mark.parametrize("code", ac.RECOMPUTE_CODES, ids=[NAME[c] for c in ac.RECOMPUTE_CODES])
@pytest.mark.parametrize("agg", ac.AGGS)
@pytest.mark.parametrize("H", ac.EDGE_H)
def test_edge_kernels_other_activations_vs_oracle(H, agg, code, chunk):
    """sir_edge_agg_fwd / _bwd_dst / _bwd_src with sigma = Identity, erf-GELU, tanh-GELU at every width class —
    the scalar path at one, two and four values per lane (3, 30, 70, 130), the sub-wave rows (4 .. 128), one to four
    full-wave passes (136 .. 1024, 640 with three vectors per lane; tests/width_cases.py) — on the
    width sweep's graph with split rows in both CSRs (chunk 4) and in the dst CSR (chunk 256): S, dQ, dK against
    the fp32 / fp64 oracle at 1e-5.  These codes have no sign mask, so the backward is the recompute one (with
    the Gm hand-off for mean).  The erf and tanh formulas lie >= 5e-5 apart on these inputs
    (tests/test_activations_cpu.py), so a dispatch arm that picked the other GELU fails."""
    assert _native.mask_words(H, code) == 0, "a sign-mask backward appeared for this code: revisit the cases"
    src, dst, V, Q, K, dS = ac.edge_inputs(H, agg)
    (S_ref, dQ_ref, dK_ref), (S_64, dQ_64, dK_64) = _sweep_reference(H, agg, code)
    plan = _sweep_plan(H, agg, chunk)
    assert plan.dst.n_splits > 0 and (plan.src.n_splits > 0) == (chunk == 4)
    QK = torch.cat([Q, K], 1).to(DEV).requires_grad_(True)
    S = EdgeAggregate.apply(QK, plan, H, agg, code, ac.slope_of(code))
    S.backward(dS.to(DEV))
    what = f"{NAME[code]} {agg} H={H} chunk={chunk}"
    assert_parity(S.detach().cpu(), S_ref, S_64, 1e-5, what + " S")
    assert_parity(QK.grad[:, :H].cpu(), dQ_ref, dQ_64, 1e-5, what + " dQ")
    assert_parity(QK.grad[:, H:].cpu(), dK_ref, dK_64, 1e-5, what + " dK")


def _within(got, truth, u, what):
    """tests/test_amp_gpu.py's bar for 16-bit storage: two units of the storage roundoff, elementwise and in
    relative L2."""
    g = got.double().cpu()
    t = truth.double().cpu()
    bound = 2 * u * t.abs() + 1e-5 * t.abs().max()
    bad = (g - t).abs() > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off by more than 2u (max {(g - t).abs().max():.3e})"
    assert rel_err(g, t) <= 2 * u, (what, rel_err(g, t))


@pytest.mark.parametrize("H", ac.EDGE_H_16BIT)
@pytest.mark.parametrize("agg", ac.AGGS)
@pytest.mark.parametrize("code", ac.RECOMPUTE_CODES, ids=[NAME[c] for c in ac.RECOMPUTE_CODES])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_edge_kernels_other_activations_16bit_storage(dt, code, agg, H):
    """The bf16 / fp16 compile units of the same passes: Q, K, dS rounded to the storage type, the oracle on those
    rounded values in fp64, the kernels (fp32 inside, one rounding per output) within 2u of it.  mean follows the
    kernel contract (include/sirconv.h): g = dS / deg is rounded to the storage type before both passes read it.
    These cases are here for indexing, rounding and the instantiation, not for the formula: erf and tanh GELU
    differ by less than one 16-bit ulp of most elements, so only the elements near zero could tell the two apart —
    the fp32 cases are what separates them."""
    assert _native.mask_words(H, code) == 0
    src, dst, V, Q, K, dS = ac.edge_inputs(H, agg)
    Q, K, dS = (t.to(DT[dt]) for t in (Q, K, dS))
    name, slope = NAME[code], ac.slope_of(code)
    S64 = oracle.edge_agg_fwd(src, dst, V, Q.double(), K.double(), agg, name, slope)
    if agg == "mean":
        deg = torch.bincount(dst, minlength=V).clamp(min=1).float().unsqueeze(1)
        g = (dS.float() / deg).to(DT[dt]).double()
        dQ64, dK64 = oracle.edge_agg_bwd(src, dst, V, Q.double(), K.double(), g, "sum", name, slope)
    else:
        dQ64, dK64 = oracle.edge_agg_bwd(src, dst, V, Q.double(), K.double(), dS.double(), agg, name, slope)
    for chunk in ac.EDGE_CHUNKS:
        QK = torch.cat([Q, K], 1).to(DEV).requires_grad_(True)
        S = EdgeAggregate.apply(QK, _sweep_plan(H, agg, chunk), H, agg, code, slope)
        assert S.dtype == DT[dt]
        S.backward(dS.to(DEV))
        assert QK.grad.dtype == DT[dt]
        what = f"{name} {agg} {dt} H={H} chunk={chunk}"
        _within(S, S64, U[dt], what + " S")
        _within(QK.grad[:, :H], dQ64, U[dt], what + " dQ")
        _within(QK.grad[:, H:], dK64, U[dt], what + " dK")


# ----------------------------------------------------------------------------- (b) identity is exact
def _exact_plan(graph, chunk):
    if (graph, chunk) not in _PLANS:
        src, dst, V = xc.GRAPHS[graph]
        _PLANS[graph, chunk] = GraphPlan(src, dst, V, DEV, chunk=chunk)
    return _PLANS[graph, chunk]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: "
                             f"got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}")


IDENTITY_CASES = [(d, H) for d in DT for H in xc.EDGE_H] + [("f32", H) for H in xc.EDGE_H_SCALAR]


@pytest.mark.parametrize("agg", ac.AGGS)
@pytest.mark.parametrize("dt,H", IDENTITY_CASES, ids=[f"{d}-{H}" for d, H in IDENTITY_CASES])
def test_identity_edge_kernels_exact(dt, H, agg):
    """sigma = identity on the dyadic inputs of tests/exact_cases.py: every intermediate is an integer (mean / sym
    on graph A: over a power of two), so S, dQ, dK equal the fp64 oracle bit for bit (rounded once for 16-bit
    storage) at chunk 4 / 64 / 256 — a dropped, doubled or misplaced term cannot hide.  Outputs and the
    partial-row workspace are pre-filled with NaN; identity has no sign mask, so the backward is the recompute
    one."""
    dtype = DT[dt]
    code = _native.ACT_IDENTITY
    assert _native.mask_words(H, code) == 0
    for graph in xc.graphs_of(agg):
        Q, K, G, _ = (t.to(DEV, dtype) for t in xc.edge_inputs(graph, H))
        wS, wdQ, wdK = (t.float().to(dtype).to(DEV) for t in xc.edge_expected(graph, H, agg, "identity"))
        for chunk in (4, 64, 256):
            plan = _exact_plan(graph, chunk)
            what = f"{graph} {dt} H={H} {agg} identity chunk={chunk}"
            in_norm, out_norm = plan.norms(agg)
            S = torch.full((Q.shape[0], H), NAN, device=DEV, dtype=dtype)
            part = torch.full((max(plan.dst.n_slots, plan.src.n_slots, 1) * H,), NAN, device=DEV)
            _native.edge_agg_fwd(plan.dst, Q, K, in_norm, out_norm, agg, code, 0.0, S, part, None)
            _same(S, wS, what + " S")
            dQK = torch.full((Q.shape[0], 2 * H), NAN, device=DEV, dtype=dtype)
            edge_backward(plan, H, agg, code, 0.0, G, Q, K, None, dQK)
            _same(dQK[:, :H], wdQ, what + " dQ")
            _same(dQK[:, H:], wdK, what + " dK")


# ----------------------------------------------------------------------------- (c) fused per-edge MLP, 10 forms
ACT1 = {"identity": nn.Identity, "relu": nn.ReLU, "leaky": lambda: nn.LeakyReLU(0.2), "gelu": nn.GELU,
        "gelu_tanh": lambda: nn.GELU(approximate="tanh")}
ACT2 = {"relu": nn.ReLU, "identity": nn.Identity}
# (ReLU, ReLU) stays in tests/test_edgemlp_gpu.py::test_seq_sigma_fused_vs_oracle
SEQ_PAIRS = [(a1, a2) for a1 in ACT1 for a2 in ACT2 if (a1, a2) != ("relu", "relu")]


def test_seq_pairs_cover_every_code():
    """act1 names every code of the library, act2 the two the kernels are built for."""
    assert sorted(ACT1) == sorted(NAME.values()) and len(SEQ_PAIRS) == 2 * len(ac.CODES) - 1
    for name, mk in ACT1.items():
        assert NAME[_elementwise_code(mk())[0]] == name


class _ReLUGiven(nn.Module):
    """ReLU whose DERIVATIVE on the listed (edge, feature) elements is given (0 or 1); its value is ReLU's."""

    def __init__(self, rows, cols, deriv):
        super().__init__()
        self.rows, self.cols, self.deriv = rows, cols, deriv

    def forward(self, h):
        mask = (h > 0).to(h.dtype)
        mask[self.rows, self.cols] = self.deriv.to(h.dtype)
        return torch.relu(h).detach() + (h - h.detach()) * mask


def _act2_tie_condition(m, src, dst, V, X, dY, agg, cap, got, what):
    """act2 = ReLU jumps at h = W act1(z) + b = 0, and among the E * F values of h a few always lie within the
    fp32 rounding of their own sum (at H = F = 256 about one in three cases has one below half an ulp of it), so
    ONE element whose sign the kernel's fp32 h resolves the other way moves the gradients by a whole edge's share
    (relL2 ~1e-3) — the per-edge Linear's counterpart of the sigma' near-ties of oracle.sigma_tie_flips.  Such
    elements are found in fp64 on the kernel's own Q, K: |h| <= c * 2^-24 * (|W| |a| + |b|) with
    c = 8 + sqrt(H) — 4 for the lo * lo products the split-fp16 MFMA drops (2^-22 relative), 4 for the fp32
    evaluation of act1, sqrt(H) for the fp32 accumulation of H products (rounding errors add as a random walk).
    The kernel's decision on each is read from ONE output, the inner Linear's dW / db (every result is affine in
    those 0 / 1 decisions; least squares, each must come out within 0.25 of 0 or 1), and the oracle is evaluated
    with ReLU' forced to them on those elements only: every output, dW / db included, must then agree at the usual
    bars.  An element beyond c that flipped is an error.  Returns the sigma to hand to the oracle and its qk
    condition, or (None, {}) when there is no such element or the kernel resolved each as fp64 does."""
    H = m.linear_query.out_features
    qk = cap["qk"]
    z = qk[dst, :H] + qk[src, H:]
    a = copy.deepcopy(m.activation[0]).cpu().double()(z)
    W, b = m.activation[1].weight.detach().cpu().double(), m.activation[1].bias.detach().cpu().double()
    h = a @ W.t() + b
    ratio = h.abs() / ((a.abs() @ W.abs().t() + b.abs()) * 2.0 ** -24)
    rows, cols = torch.nonzero(ratio <= 8 + H ** 0.5, as_tuple=True)
    k = rows.numel()
    if k == 0:
        return None, {}
    assert k <= 64, f"{what}: {k} elements of h within rounding of 0: the inputs are degenerate"
    own = (h[rows, cols] > 0).double()

    def run(deriv, dtype):
        sigma = nn.Sequential(m.activation[0], m.activation[1], _ReLUGiven(rows, cols, deriv))
        return _oracle(m, src, dst, V, X, dY, agg, sigma, dtype, qk=qk)

    keys = (("activation.1.weight", "act.1.weight"), ("activation.1.bias", "act.1.bias"))
    base = run(own, torch.float64)
    vec = lambda r, i: torch.cat([r[kk[i]].double().flatten() for kk in keys])
    A = []
    for i in range(k):
        d = own.clone()
        d[i] = 1 - d[i]
        A.append(vec(run(d, torch.float64), 1) - vec(base, 1))
    s = torch.linalg.lstsq(torch.stack(A, 1), (vec(got, 0) - vec(base, 1)).unsqueeze(1), driver="gelsd").solution[:, 0]
    flip = s.round()
    assert bool(((s - flip).abs() < 0.25).all()) and bool(((flip == 0) | (flip == 1)).all()), \
        f"{what}: dW / db of the inner Linear do not name a 0 / 1 decision on the near-zero h (solution {s.tolist()})"
    if not flip.any():              # the kernel resolved every near-zero h as fp64 does: the plain oracle
        return None, {}
    tie_conditioned(what + " [columns here: h within rounding of 0, worst |h| / (2^-24 mag); of them ReLU' resolved "
                    "the other way, worst]", k, float(ratio[rows, cols].max()), int(flip.sum()),
                    float(ratio[rows, cols][flip == 1].max()))
    deriv = torch.where(flip == 1, 1 - own, own)
    return nn.Sequential(m.activation[0], m.activation[1], _ReLUGiven(rows, cols, deriv)), {"qk": qk}


@pytest.mark.parametrize("H,Fo", [(16, 16), (100, 140), (256, 256)])
@pytest.mark.parametrize("agg", ac.AGGS)
@pytest.mark.parametrize("a1,a2", SEQ_PAIRS, ids=[f"{a}-{b}" for a, b in SEQ_PAIRS])
@pytest.mark.parametrize("chunk", [256, 4])
def test_seq_sigma_all_activation_pairs_vs_oracle(chunk, a1, a2, agg, H, Fo, monkeypatch):
    """sigma = Sequential(act1, Linear(H, F), act2) for the nine forms beside (ReLU, ReLU), through the layer:
    the fused forward (the edge-stream kernel at H = 256, the per-item one otherwise) and the fused backward
    against the fp32 / fp64 oracle of the reference dataflow — Y strict, dX, every weight and bias gradient and
    the inner Linear's, as test_seq_sigma_fused_vs_oracle scores them.  Near-ties are conditioned as there for
    sigma' of act1 (_tie_condition) and, for act2 = ReLU, for the sign of a near-zero h (_act2_tie_condition: 2 of
    the 72 such cases, one pair of duplicate edges with |h| at 0.3 ulp of its sum's magnitude)."""
    _no_generic(monkeypatch)
    src, dst, V, gen = _graph(H + Fo + len(agg))
    d, O = 24, 20
    X, dY = torch.randn(V, d, generator=gen), torch.randn(V, O, generator=gen)
    torch.manual_seed(H)
    sigma = nn.Sequential(ACT1[a1](), nn.Linear(H, Fo), ACT2[a2]())
    m = SIRConv(d, H, O, sigma, 0, agg_type=agg)
    m.linear_relation = nn.Linear(Fo, O)
    m = m.to(DEV)
    m.chunk = chunk
    seen = []
    real = edgemlp._fwd               # (plan, Q, K, W, b, agg, act1, slope, act2, out)
    monkeypatch.setattr(edgemlp, "_fwd", lambda *a, **k: seen.append((a[6], a[8])) or real(*a, **k))
    what = f"seq {a1}/{a2} {agg} H{H} F{Fo} c{chunk}"
    cap = {}
    got = _run(m, Graph(src, dst, V), X, dY, capture=cap)
    assert len(seen) == 1 and NAME[seen[0][0]] == a1 and NAME[seen[0][1]] == a2, (what, seen)
    assert "activation.1.weight" in got
    cond = _tie_condition(m, src, dst, V, X, None, cap, what)
    sigma = m.activation
    if a2 == "relu":
        given, cond2 = _act2_tie_condition(m, src, dst, V, X, dY, agg, cap, got, what)
        sigma = given or sigma
        cond.update(cond2)
    r32 = _oracle(m, src, dst, V, X, dY, agg, sigma, torch.float32, **cond)
    r64 = _oracle(m, src, dst, V, X, dY, agg, sigma, torch.float64, **cond)
    for k, kr in (("Y", "Y"), ("dX", "dX"), ("linear_query.weight", "dW_Q"), ("linear_query.bias", "db_Q"),
                  ("linear_key.weight", "dW_K"), ("linear_relation.weight", "dW_R"),
                  ("linear_relation.bias", "db_R"), ("activation.1.weight", "act.1.weight"),
                  ("activation.1.bias", "act.1.bias")):
        assert_parity(got[k], r32[kr], r64[kr], 1e-5, f"{what} {k}", strict=(k == "Y"))


@pytest.mark.parametrize("a1,a2", [("identity", "relu"), ("leaky", "identity"), ("gelu", "relu"),
                                   ("gelu_tanh", "identity")])
def test_seq_sigma_other_activations_under_bf16_autocast(a1, a2):
    """One bf16-autocast run per act1 beside ReLU, as tests/test_amp_gpu.py::
    test_fused_edge_mlp_forms_under_autocast runs the (ReLU, ReLU) form: outputs and gradients within the AMP bar
    (2e-2) of the fp32 layer, or no worse than 1.25x the reference's own AMP dataflow."""
    gen = torch.Generator().manual_seed(31 + len(a1))
    V, E, d, H, O = 300, 2400, 32, 64, 48
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(0, V - 10, (E,), generator=gen)
    dst[:300] = 4                                            # a split row
    X = torch.randn(V, d, generator=gen).to(DEV)
    dY = torch.randn(V, O, generator=gen).to(DEV)
    torch.manual_seed(5)
    act = nn.Sequential(ACT1[a1](), nn.Linear(H, H), ACT2[a2]())
    m = SIRConv(d, H, O, act, 0, agg_type="sum").to(DEV)
    ref = oracle.SIRConvRef(d, H, O, act, 0, agg_type="sum").to(DEV)
    ref.load_state_dict(m.state_dict())
    g = Graph(src, dst, V)

    def run(mod, amp):
        for p in mod.parameters():
            p.grad = None
        x = X.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = mod(g, x)
        y.float().backward(dY)
        out = {"Y": y.detach().float(), "dX": x.grad}
        out.update({n: p.grad for n, p in mod.named_parameters()})
        return {k: v.detach().float().cpu() for k, v in out.items()}

    got, truth, amp = run(m, True), run(ref, False), run(ref, True)
    for k in truth:
        e, e_amp = rel_err(got[k], truth[k]), rel_err(amp[k], truth[k])
        assert e <= max(2e-2, 1.25 * e_amp), f"seq {a1}/{a2} {k}: relL2 {e:.3e} (reference AMP {e_amp:.3e})"


# ----------------------------------------------------------------------------- (d) exact integers, MLP kernels
SEQ_CODE = {"identity": (_native.ACT_IDENTITY, 0.0), "relu": (_native.ACT_RELU, 0.0),
            "leaky": (_native.ACT_LEAKY, xc.SLOPE)}
GRAPH_AGG = xc.GRAPH_AGG


@pytest.mark.parametrize("a1,a2", xc.SEQ_ACT_PAIRS, ids=[f"{a}-{b}" for a, b in xc.SEQ_ACT_PAIRS])
@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
@pytest.mark.parametrize("H,Fo", xc.SEQ_SHAPES)
def test_seq_sigma_kernels_exact_other_activations(H, Fo, graph, agg, a1, a2):
    """tests/test_exact_gpu.py::test_seq_sigma_kernels_exact's comparison for (Identity, ReLU), (Identity,
    Identity), (LeakyReLU(0.25), Identity) and (ReLU, Identity): out, dQ, dK and the summed per-wave partials
    (dW, db) equal the fp64 oracle on the dyadic inputs (tests/test_exact_inputs_cpu.py holds them to that),
    sigma'(0) = slope for the LeakyReLU included."""
    Q, K, W, b, G = (t.to(DEV) for t in xc.mlp_inputs(graph, H, Fo))
    want = {k: v.float().to(DEV) for k, v in xc.seq_expected(graph, H, Fo, agg, act1=a1, act2=a2).items()}
    (c1, slope), c2 = SEQ_CODE[a1], SEQ_CODE[a2][0]
    for chunk in (4, 64, 256):
        what = f"seq {a1}/{a2} {graph} {agg} H={H} F={Fo} chunk={chunk}"
        QK = torch.cat([Q, K], 1).requires_grad_(True)
        Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        S = EdgeMLPSum.apply(QK, Wr, br, _exact_plan(graph, chunk), H, agg, c1, slope, c2)
        S.backward(G)
        _same(S.detach(), want["S"], what + " S")
        _same(QK.grad[:, :H], want["dQ"], what + " dQ")
        _same(QK.grad[:, H:], want["dK"], what + " dK")
        _same(Wr.grad, want["dW"], what + " dW")
        _same(br.grad, want["db"], what + " db")


# ----------------------------------------------------------------------------- layer level: the callable forms
CALLABLES = {"F.gelu": (F.gelu, "gelu"), "torch.relu": (torch.relu, "relu"),
             "GELU(tanh)": (nn.GELU(approximate="tanh"), "gelu_tanh"), "Identity": (nn.Identity(), "identity")}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "modular"])
@pytest.mark.parametrize("agg", ac.AGGS)
@pytest.mark.parametrize("form", list(CALLABLES))
def test_layer_callable_activation_forms_vs_oracle(form, agg, fused):
    """SIRConv(..., activation=<callable>) for the forms no fixture carries — the functional F.gelu and torch.relu,
    nn.GELU(approximate='tanh'), nn.Identity() — on the small_* graph and weights of tests/golden, through the
    whole-layer Function and through the modular route: Y (strict) and every gradient against
    oracle.layer_fwd_bwd in fp32 / fp64."""
    act, name = CALLABLES[form]
    z = load_case(f"small_{agg}_gelu_f32")
    d, H = z["W_Q"].shape[1], z["W_Q"].shape[0]
    O, V = z["W_R"].shape[0], z["X"].shape[0]
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(DEV)
    m = SIRConv(d, H, O, act, 0, agg_type=agg).to(DEV)
    m.use_fused = fused
    with torch.no_grad():
        m.linear_query.weight.copy_(t("W_Q")); m.linear_query.bias.copy_(t("b_Q"))
        m.linear_key.weight.copy_(t("W_K"))
        m.linear_relation.weight.copy_(t("W_R")); m.linear_relation.bias.copy_(t("b_R"))
    X = t("X").requires_grad_(True)
    Y = m(Graph(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), V), X)
    Y.backward(t("dY"))
    got = {"Y": Y, "dX": X.grad, "dW_Q": m.linear_query.weight.grad, "db_Q": m.linear_query.bias.grad,
           "dW_K": m.linear_key.weight.grad, "dW_R": m.linear_relation.weight.grad,
           "db_R": m.linear_relation.bias.grad}
    keys = ("X", "W_Q", "b_Q", "W_K", "W_R", "b_R", "dY")
    r32 = oracle.layer_fwd_bwd(z["src"], z["dst"], V, *[torch.from_numpy(z[k]) for k in keys], agg, name)
    r64 = oracle.layer_fwd_bwd(z["src"], z["dst"], V, *[torch.from_numpy(z[k]).double() for k in keys], agg, name)
    for k, v in got.items():
        assert_parity(v.detach().cpu(), r32[k], r64[k], 1e-5, f"{form} {agg} fused={fused} {k}", strict=(k == "Y"))
