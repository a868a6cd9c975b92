"""sirgcn.label_spreading / correct_and_smooth and sir_label_prop_step on the MI355X against the restatement of
tests/cs_cases.py (pinned to the reference's fixtures by tests/test_cs_cases_cpu.py):
1. exact: rows of at most one chunk equal the fp32 restatement bit for bit, one step and three, every mode;
2. split rows: inside the project's parity envelope step by step, unsplit rows of the same graph bit-equal;
3. routes and drivers: callable post steps equal the fused ones, correct_and_smooth equals the run() fixtures;
4. poison: pad columns, fixed rows, a NaN's reach, the clamp;  5. edge cases, layouts, other dtypes;
6. run-to-run determinism and a whole correct_and_smooth captured in a HIP graph."""
from functools import partial

import pytest
import torch

from conftest import assert_parity, rel_err

import cs_cases as cs
import width_cases as wc
import sirgcn
from sirgcn import Clamp, FixRows, Graph, _native, get_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 0.8
AGGS = ("sym", "mean", "sum")
POSTS = ("none", "clamp", "fix")
LO, HI = -0.25, 0.5
_GRAPHS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _graph(V, split):
    key = (V, split)
    if key not in _GRAPHS:
        src, dst, _ = cs.case_graph(V, split) if split != "low" else cs.low_degree_graph(V)
        _GRAPHS[key] = Graph(src, dst, V)
    return _GRAPHS[key]


def _edges(V, split):
    return (cs.case_graph(V, split) if split != "low" else cs.low_degree_graph(V))[:2]


def _post(kind, yfix, idx):
    """(restatement's post, fused descriptor, the reference's own callable)"""
    if kind == "clamp":
        return ("clamp", LO, HI), Clamp(LO, HI), (lambda x: x.clamp(LO, HI))
    if kind == "fix":
        return ("fix", yfix, idx), FixRows(yfix.to(DEV), idx.to(DEV)), partial(_fix_input, y=yfix.to(DEV), mask=idx.to(DEV))
    return None, None, None


def _fix_input(x, y, mask):          # what the reference's post step does, written as a user would
    x[mask] = y[mask]
    return x


def _kstep(V, split, y, y0, agg, alpha, kind="none", yfix=None, idx=None, out=None):
    """One sir_label_prop_step on the graph's plan; `partial` starts as NaN (stale slots must never be read)."""
    plan = get_plan(_graph(V, split), DEV)
    csr = plan.dst
    F = y0.shape[1]
    norm = plan.norms("sym")[0] if agg == "sym" else None
    out = torch.empty((V, F), device=DEV) if out is None else out
    part = torch.full((csr.n_slots * F,), float("nan"), device=DEV) if csr.n_splits else None
    post, lo, hi, fixed, Yf = _native.LP_POST_NONE, 0.0, 0.0, None, None
    if kind == "clamp":
        post, lo, hi = _native.LP_POST_CLAMP, LO, HI
    elif kind == "fix":
        post, fixed, Yf = _native.LP_POST_FIX, FixRows(yfix, idx).flag(V, torch.device(DEV, 0)), yfix
    _native.label_prop_step(csr, y, y0, norm, agg, alpha, 1.0 - alpha, out, post, lo, hi, fixed, Yf, part)
    return out


def _kspread(V, split, y0, nprop, agg, kind, yfix, idx):
    y = y0
    for _ in range(nprop):
        y = _kstep(V, split, y, y0, agg, ALPHA, kind, yfix, idx)
    return y


def _ref(V, split, F, nprop, agg, kind, dtype=torch.float32):
    """The restatement's result for the shared inputs of (V, F); computed once."""
    key = (V, split, F, nprop, agg, kind, dtype)
    if key not in _REFS:
        src, dst = _edges(V, split)
        y0, yfix, idx = cs.inputs(V, F)
        post = _post(kind, yfix, idx)[0]
        _REFS[key] = cs.spread(src, dst, V, y0.to(dtype), nprop, ALPHA, agg, post)
    return _REFS[key]


def _same(a, b):
    """Bit-level equality that lets NaN equal NaN."""
    a, b = a.cpu(), b.cpu()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("F", wc.LP_F)
def test_unsplit_rows_equal_the_reference_bit_for_bit(F):
    for V in (1, 5, 67, 300):
        y0, yfix, idx = cs.inputs(V, F)
        y0d, yfd, idd = y0.to(DEV), yfix.to(DEV), idx.to(DEV)
        g = _graph(V, False)
        for agg in AGGS:
            for kind in POSTS:
                fused = _post(kind, yfix, idx)[1]
                for nprop in (1, 3):
                    want = _ref(V, False, F, nprop, agg, kind)
                    got = _kspread(V, False, y0d, nprop, agg, kind, yfd, idd)
                    assert torch.equal(got.cpu(), want), f"step kernel V={V} F={F} {agg} {kind} nprop={nprop}"
                    if agg != "sum":
                        drv = sirgcn.label_spreading(g, y0d, nprop, ALPHA, agg == "sym", fused)
                        assert torch.equal(drv.cpu(), want), f"driver V={V} F={F} {agg} {kind} nprop={nprop}"
        assert torch.equal(y0d.cpu(), y0)


@pytest.mark.parametrize("name", [c["name"] for c in cs.cs_manifest() if c["kind"] == "spread"])
def test_label_spreading_fixtures(name):
    c = next(x for x in cs.cs_manifest() if x["name"] == name)
    fx = cs.load_fixture(name)
    V, src, dst = c["V"], fx["src"], fx["dst"]
    g = Graph(src, dst, V)
    post = None
    if c["post"] == "clamp":
        post = Clamp(c["lo"], c["hi"])
    elif c["post"] == "fix":
        post = FixRows(fx["yfix"].to(DEV), fx["idx"].to(DEV))
    y = sirgcn.label_spreading(g, fx["y0"].to(DEV), c["nprop"], c["alpha"], c["agg"] == "sym", post).cpu()
    deg = torch.bincount(dst, minlength=V)
    split_rows = torch.nonzero(deg > cs.CHUNK).flatten()
    # a split row's tolerance-level difference reaches its out-neighbours one step later: the rows it cannot have
    # reached within the remaining steps are the reference's bits
    clean = ~cs.downstream(src, dst, V, split_rows, c["nprop"] - 1)
    assert int(clean.sum()) > V // 2
    assert torch.equal(y[clean], fx["y"][clean]), name
    want64 = cs.spread(src, dst, V, fx["y0"].double(), c["nprop"], c["alpha"], c["agg"], cs.fixture_post(c, fx))
    assert_parity(y, fx["y"], want64, 1e-5, name)


# ------------------------------------------------------------------ 2. split rows
@pytest.mark.parametrize("F", wc.LP_F_SPLIT)
@pytest.mark.parametrize("V", [1, 5, 67, 300])
def test_split_rows_step_by_step(V, F):
    src, dst, deg = cs.case_graph(V, True)
    degt = torch.tensor(deg)
    unsplit = degt <= cs.CHUNK
    assert int((~unsplit).sum()) == min(V, 2)
    y0, yfix, idx = cs.inputs(V, F)
    y0d, yfd, idd = y0.to(DEV), yfix.to(DEV), idx.to(DEV)
    for agg in AGGS:
        for kind in POSTS:
            post = _post(kind, yfix, idx)[0]
            y = y0d
            for k in range(3):
                # step k + 1 from the kernel's own step-k output: a single-step check, nothing compounds
                nxt = _kstep(V, True, y, y0d, agg, ALPHA, kind, yfd, idd)
                w32 = cs.step(src, dst, V, y.cpu(), y0, ALPHA, agg, post)
                w64 = cs.step(src, dst, V, y.cpu().double(), y0.double(), ALPHA, agg, post)
                what = f"V={V} F={F} {agg} {kind} step {k + 1}"
                assert_parity(nxt, w32, w64, 1e-5, what)
                assert torch.equal(nxt.cpu()[unsplit], w32[unsplit]), what + ": unsplit rows"
                if kind == "fix":
                    assert torch.equal(nxt.cpu()[idx], yfix[idx]), what + ": fixed rows"
                y = nxt
            if agg != "sum":
                drv = sirgcn.label_spreading(_graph(V, True), y0d, 3, ALPHA, agg == "sym", _post(kind, yfix, idx)[1])
                assert torch.equal(drv, y), f"driver V={V} F={F} {agg} {kind}"


# ------------------------------------------------------------------ 3. routes and drivers
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("use_sym", [True, False])
def test_callable_post_steps_equal_the_fused_ones(use_sym, split):
    V, F = 300, 40
    y0, yfix, idx = cs.inputs(V, F)
    y0d = y0.to(DEV)
    g = _graph(V, split)
    for kind in ("clamp", "fix"):
        _, fused, call = _post(kind, yfix, idx)
        a = sirgcn.label_spreading(g, y0d, 3, ALPHA, use_sym, fused)
        b = sirgcn.label_spreading(g, y0d, 3, ALPHA, use_sym, call)
        assert torch.equal(a, b), kind
        assert torch.equal(y0d.cpu(), y0)
    # the defaults are the reference's: nprop=10, alpha=0.1, use_sym=True, no post step
    assert torch.equal(sirgcn.label_spreading(g, y0d), sirgcn.label_spreading(g, y0d, 10, 0.1, True, None))


@pytest.mark.parametrize("name", [c["name"] for c in cs.cs_manifest() if c["kind"] == "run"])
@pytest.mark.parametrize("labels_2d", [True, False])
def test_correct_and_smooth_equals_the_run_fixtures(name, labels_2d):
    c = next(x for x in cs.cs_manifest() if x["name"] == name)
    fx = cs.load_fixture(name)
    V, src, dst = c["V"], fx["src"], fx["dst"]
    g = Graph(src, dst, V)
    pred = fx["predictions"].to(DEV)
    labels = fx["labels"] if labels_2d else fx["labels"].reshape(-1)
    y = sirgcn.correct_and_smooth(g, pred, labels.to(DEV), fx["train_idx"].to(DEV), c["alpha_c"], c["nprop_c"],
                                  c["alpha_s"], c["nprop_s"], c["use_sym"]).cpu()
    assert torch.equal(pred.cpu(), fx["predictions"]), "predictions must not be modified"
    assert y.shape == fx["smoothed_y"].shape and y.dtype == torch.float32
    args = (src, dst, V, fx["predictions"].double(), fx["labels"], fx["train_idx"], c["alpha_c"], c["nprop_c"], c["alpha_s"],
            c["nprop_s"], c["use_sym"])
    assert_parity(y, fx["smoothed_y"], cs.correct_and_smooth(*args), 1e-5, name)
    split_rows = torch.nonzero(torch.bincount(dst, minlength=V) > cs.CHUNK).flatten()
    clean = ~cs.downstream(src, dst, V, split_rows, c["nprop_c"] + c["nprop_s"] - 1)
    assert torch.equal(y[clean], fx["smoothed_y"][clean])
    # without split rows the whole run is the reference's bits: the same inputs on the graph minus its hub row
    hub = int(split_rows[0])
    keep = dst != hub
    g2 = Graph(src[keep], dst[keep], V)
    y2 = sirgcn.correct_and_smooth(g2, pred, labels.to(DEV), fx["train_idx"].to(DEV), c["alpha_c"], c["nprop_c"],
                                   c["alpha_s"], c["nprop_s"], c["use_sym"], num_classes=c["F"]).cpu()
    want2 = cs.correct_and_smooth(src[keep], dst[keep], V, fx["predictions"], fx["labels"], fx["train_idx"], c["alpha_c"],
                                  c["nprop_c"], c["alpha_s"], c["nprop_s"], c["use_sym"])
    assert torch.equal(y2, want2)


# ------------------------------------------------------------------ 4. poison
def _padded(x, left, right, fill=float("nan")):
    """x as a column slice of a wider tensor full of `fill`; returns (view, wide)."""
    wide = torch.full((x.shape[0], left + x.shape[1] + right), fill, device=DEV)
    wide[:, left:left + x.shape[1]] = x
    return wide[:, left:left + x.shape[1]], wide


@pytest.mark.parametrize("left,right", [(0, 4), (1, 2)])         # 16-B rows (float4 path) / unaligned (scalar path)
@pytest.mark.parametrize("split", [False, True])
def test_pad_columns_are_neither_read_nor_written(split, left, right):
    V, F = 67, 40
    y0, yfix, idx = cs.inputs(V, F)
    for agg in AGGS:
        for kind in POSTS:
            yv, _ = _padded(y0.to(DEV), left, right)
            y0v, _ = _padded(y0.to(DEV), left, right)
            yfv, _ = _padded(yfix.to(DEV), left, right)
            ov, owide = _padded(torch.zeros(V, F, device=DEV), left, right, fill=123.0)
            assert yv.stride(0) == F + left + right and (yv.data_ptr() % 16 == 0) == (left == 0)
            before = owide.clone()
            _kstep(V, split, yv, y0v, agg, ALPHA, kind, yfv, idx.to(DEV), out=ov)
            plain = _kstep(V, split, y0.to(DEV), y0.to(DEV), agg, ALPHA, kind, yfix.to(DEV), idx.to(DEV))
            assert torch.equal(ov, plain) and not torch.isnan(ov).any(), f"{agg} {kind}"
            assert torch.equal(owide[:, :left], before[:, :left]) and torch.equal(owide[:, left + F:], before[:, left + F:])


@pytest.mark.parametrize("split", [False, True])
def test_nan_in_fixed_rows_of_y_is_overwritten(split):
    V, F = 67, 40
    src, dst = _edges(V, split)
    y0, yfix, idx = cs.inputs(V, F)
    y = y0.clone()
    y[idx] = float("nan")
    for agg in AGGS:
        out = _kstep(V, split, y.to(DEV), y.to(DEV), agg, ALPHA, "fix", yfix.to(DEV), idx.to(DEV)).cpu()
        assert torch.equal(out[idx], yfix[idx]), agg                   # Y, Y0 and the NaN partial slots are ignored
        assert _same(out, cs.step(src, dst, V, y, y, ALPHA, agg, ("fix", yfix, idx))), agg


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("split", [False, True])
def test_a_non_finite_row_reaches_exactly_its_out_neighbours(split, bad):
    V, F = 67, 40
    src, dst = _edges(V, split)
    y0, _, _ = cs.inputs(V, F)
    for u in (0, 2, 5, 66):
        y = y0.abs() if bad == float("inf") else y0.clone()            # no -Inf to cancel against
        y[u] = bad
        reach = torch.zeros(V, dtype=torch.bool)
        reach[dst[src == u]] = True
        for agg in AGGS:
            for kind in ("none", "clamp"):
                out = _kstep(V, split, y.to(DEV), y0.to(DEV), agg, ALPHA, kind).cpu()
                hit = ~torch.isfinite(out) if kind == "none" else torch.isnan(out)
                if bad != bad or kind == "none":
                    assert torch.equal(hit.all(1), reach) and torch.equal(hit.any(1), reach), f"u={u} {agg} {kind}"
                else:                                                  # clamp(+Inf) = hi: finite again, as torch.clamp
                    assert not hit.any() and bool((out[reach] == HI).all())
                post = ("clamp", LO, HI) if kind == "clamp" else None
                assert _same(out[~reach], cs.step(src, dst, V, y, y0, ALPHA, agg, post)[~reach])


def test_clamp_keeps_nan():
    V, F = 5, 4
    y0 = torch.full((V, F), float("nan"))
    y0[:, 1] = 7.0
    y0[:, 2] = -7.0
    src, dst = _edges(V, False)
    for agg in AGGS:
        out = _kstep(V, False, y0.to(DEV), y0.to(DEV), agg, ALPHA, "clamp").cpu()
        assert torch.isnan(out[:, 0]).all() and torch.isnan(out[:, 3]).all(), agg
        assert _same(out, cs.step(src, dst, V, y0, y0, ALPHA, agg, ("clamp", LO, HI))), agg


# ------------------------------------------------------------------ 5. edge cases, layouts, dtypes
def test_graph_without_edges_and_nprop_zero():
    V, F = 5, 40
    e = torch.zeros(0, dtype=torch.int64)
    g = Graph(e, e, V)
    y0 = cs.inputs(V, F)[0]
    y0d = y0.to(DEV)
    for use_sym in (True, False):
        out = sirgcn.label_spreading(g, y0d, 2, ALPHA, use_sym)
        assert torch.equal(out.cpu(), cs.spread(e, e, V, y0, 2, ALPHA, "sym" if use_sym else "mean"))
    assert sirgcn.label_spreading(g, y0d, nprop=0) is y0d
    assert sirgcn.label_spreading(_graph(67, True), cs.inputs(67, 3)[0].to(DEV), 0, post_step=Clamp(0, 1)).shape == (67, 3)


def test_one_node_with_a_self_loop():
    g = Graph(torch.tensor([0]), torch.tensor([0]), 1)
    for F in (1, 40):
        y0 = cs.inputs(1, F)[0]
        for use_sym in (True, False):
            out = sirgcn.label_spreading(g, y0.to(DEV), 3, ALPHA, use_sym, Clamp(LO, HI))
            want = cs.spread(torch.tensor([0]), torch.tensor([0]), 1, y0, 3, ALPHA, "sym" if use_sym else "mean",
                             ("clamp", LO, HI))
            assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("F", [40, 47])
def test_column_slice_and_non_contiguous_inputs(F, monkeypatch):
    V = 67
    y0, yfix, idx = cs.inputs(V, F)
    g = _graph(V, True)
    seen = []
    orig = _native.label_prop_step
    monkeypatch.setattr(_native, "label_prop_step",
                        lambda csr, Y, Y0, *a, **k: seen.append((Y0.stride(0), Y0.data_ptr())) or orig(csr, Y, Y0, *a, **k))
    plain = sirgcn.label_spreading(g, y0.to(DEV), 2, ALPHA, True, FixRows(yfix.to(DEV), idx.to(DEV)))
    view, wide = _padded(y0.to(DEV), 1, 2, fill=5.0)
    keep = wide.clone()
    seen.clear()
    sliced = sirgcn.label_spreading(g, view, 2, ALPHA, True, FixRows(_padded(yfix.to(DEV), 1, 2)[0], idx.to(DEV)))
    assert seen[0] == (F + 3, view.data_ptr()), "the slice must be passed with its leading dimension, not copied"
    assert torch.equal(sliced, plain) and torch.equal(wide, keep)
    tr = y0.t().contiguous().to(DEV).t()                          # column-major: rows are not unit-stride
    assert not tr.is_contiguous() and torch.equal(tr, y0.to(DEV))
    assert torch.equal(sirgcn.label_spreading(g, tr, 2, ALPHA, True, FixRows(yfix.to(DEV), idx.to(DEV))), plain)


@pytest.mark.parametrize("dt", ["bf16", "fp64"])
def test_other_dtypes_take_the_composed_route(dt, monkeypatch):
    """fp64: the restatement in fp64 at rtol = atol = 1e-12 (a different summation order only).  bf16: relative L2
    within 2e-2 on a graph of in-degrees <= 8 and two steps: every rounding is 2^-9 relative (0.11 % rms), a step
    makes about a dozen of them per element (8 adds, 3-4 products), so two orders of adding differ by well under
    sqrt(2 * 12) * 0.11 % * sqrt(2) = 0.8 %."""
    dtype = {"bf16": torch.bfloat16, "fp64": torch.float64}[dt]
    monkeypatch.setattr(_native, "label_prop_step", lambda *a, **k: pytest.fail(f"{dt} must not reach the kernel"))
    V, F = 67, 40
    split = "low" if dt == "bf16" else True
    src, dst = _edges(V, split)
    y0, yfix, idx = cs.inputs(V, F)
    for use_sym in (True, False):
        for kind in POSTS:
            post, fused, _ = _post(kind, yfix, idx)
            out = sirgcn.label_spreading(_graph(V, split), y0.to(DEV, dtype), 2, ALPHA, use_sym, fused)
            want = cs.spread(src, dst, V, y0.to(dtype), 2, ALPHA, "sym" if use_sym else "mean", post)
            assert out.dtype == dtype and out.shape == (V, F)
            if dt == "fp64":
                assert torch.allclose(out.cpu(), want, rtol=1e-12, atol=1e-12), f"{use_sym} {kind}"
            else:
                assert rel_err(out.cpu().float(), want.float()) <= 2e-2, f"{use_sym} {kind}"


# ------------------------------------------------------------------ 6. determinism and capture
def test_run_to_run_identical():
    V, F = 300, 40
    y0, yfix, idx = cs.inputs(V, F)
    g = _graph(V, True)
    for use_sym in (True, False):
        runs = [sirgcn.label_spreading(g, y0.to(DEV), 5, ALPHA, use_sym, FixRows(yfix.to(DEV), idx.to(DEV))) for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_correct_and_smooth_captures_and_replays():
    V, C = 300, 40
    g = _graph(V, True)
    gen = torch.Generator().manual_seed(17)
    preds = [torch.softmax(torch.randn(V, C, generator=gen), -1) for _ in range(2)]
    labels = torch.randint(0, C, (V, 1), generator=gen).to(DEV)
    train_idx = torch.randperm(V, generator=gen)[:V // 2].sort().values.to(DEV)
    static = preds[0].to(DEV)

    def run(p):
        return sirgcn.correct_and_smooth(g, p, labels, train_idx, 0.8, 4, 0.8, 4, True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (the plan, the norms)
        eager0 = run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    static.copy_(preds[1].to(DEV))                     # new contents of the static buffer, then two replays
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run(preds[1].to(DEV)))
    assert not torch.equal(out, eager0)
