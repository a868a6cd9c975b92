"""tests/cs_cases.py without a GPU: the fp32 restatement equals every fixture the reference's own
correct_and_smooth.py produced (tests/golden/cs_*.npz) bit for bit, the fixtures hold the graph features they
are there for, and the builders give the GPU tests the rows they assume."""
import pytest
import torch

import cs_cases as cs
from sirgcn import Graph, get_plan
from sirgcn.graph import DEFAULT_CHUNK

CASES = cs.cs_manifest()


def _ids(kind):
    return [c["name"] for c in CASES if c["kind"] == kind]


def _case(name):
    return next(c for c in CASES if c["name"] == name)


def test_manifest_covers_the_cases():
    spread = {(c["agg"], c["post"], c["nprop"]) for c in CASES if c["kind"] == "spread"}
    assert spread == {(a, p, n) for a in ("sym", "mean") for p in ("none", "clamp", "fix") for n in (1, 3)}
    assert len(_ids("run")) == 2
    assert {c["use_sym"] for c in CASES if c["kind"] == "run"} == {True, False}


@pytest.mark.parametrize("name", _ids("spread") + _ids("run"))
def test_fixture_graphs(name):
    c, fx = _case(name), cs.load_fixture(name)
    src, dst, V = fx["src"], fx["dst"], c["V"]
    assert V <= 300 and c["F"] <= 40
    deg = torch.bincount(dst, minlength=V)
    assert int(deg.max()) >= 700 and int(deg.min()) == 0                 # a hub (a split row), a row without in-edges
    assert bool((src == dst).any())                                       # self-loops
    assert torch.unique(torch.stack([src, dst]), dim=1).shape[1] < src.numel()      # duplicate edges
    assert int((deg > DEFAULT_CHUNK).sum()) == 1


@pytest.mark.parametrize("name", _ids("spread"))
def test_restatement_equals_label_spreading_fixture(name):
    c, fx = _case(name), cs.load_fixture(name)
    y0 = fx["y0"].clone()
    y = cs.spread(fx["src"], fx["dst"], c["V"], y0, c["nprop"], c["alpha"], c["agg"], cs.fixture_post(c, fx))
    assert y.dtype == torch.float32 and torch.equal(y, fx["y"]), name
    assert torch.equal(y0, fx["y0"])
    # the fp64 twin is the same algorithm: it agrees to fp32 rounding
    y64 = cs.spread(fx["src"], fx["dst"], c["V"], y0.double(), c["nprop"], c["alpha"], c["agg"], cs.fixture_post(c, fx))
    assert y64.dtype == torch.float64 and torch.allclose(y64.float(), y, rtol=1e-4, atol=1e-5)
    if c["post"] == "clamp":
        assert bool((y == c["lo"]).any()) and bool((y == c["hi"]).any())     # the clamp bites on both sides
    if c["post"] == "fix":
        assert torch.equal(y[fx["idx"]], fx["yfix"][fx["idx"]])


@pytest.mark.parametrize("name", _ids("run"))
def test_restatement_equals_run_fixture(name):
    c, fx = _case(name), cs.load_fixture(name)
    assert fx["labels"].shape == (c["V"], 1) and torch.unique(fx["labels"]).numel() == c["F"]
    pred = fx["predictions"].clone()
    y = cs.correct_and_smooth(fx["src"], fx["dst"], c["V"], pred, fx["labels"], fx["train_idx"], c["alpha_c"],
                              c["nprop_c"], c["alpha_s"], c["nprop_s"], c["use_sym"])
    assert torch.equal(y, fx["smoothed_y"]), name
    assert torch.equal(pred, fx["predictions"])
    assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0


def test_sum_is_the_mean_without_its_division():
    src, dst, deg = cs.case_graph(67, False)
    y0, _, _ = cs.inputs(67, 5)
    s = cs.step(src, dst, 67, y0, y0, 1.0, "sum")
    m = cs.step(src, dst, 67, y0, y0, 1.0, "mean")
    assert torch.equal(s / torch.tensor(deg).clamp(min=1).float()[:, None], m)


@pytest.mark.parametrize("V", [1, 5, 67, 300])
@pytest.mark.parametrize("split", [False, True])
def test_builders_give_the_rows_the_gpu_tests_assume(V, split):
    assert cs.CHUNK == DEFAULT_CHUNK == 256
    src, dst, deg = cs.case_graph(V, split)
    assert torch.equal(torch.bincount(dst, minlength=V), torch.tensor(deg)) if src.numel() else sum(deg) == 0
    want = ((2 * DEFAULT_CHUNK + 1, DEFAULT_CHUNK + 1) if split else ()) + (DEFAULT_CHUNK, DEFAULT_CHUNK - 1, 0, 1)
    assert tuple(deg[:len(want)]) == want[:V]
    if V >= 67:
        assert {0, 1, 255, 256} <= set(deg) and (not split or {257, 513} <= set(deg))
        assert bool((src == dst).any())
        assert torch.unique(torch.stack([src, dst]), dim=1).shape[1] < src.numel()
    plan = get_plan(Graph(src, dst, V), "cpu")
    csr = plan.dst
    if not split:
        assert max(deg) <= DEFAULT_CHUNK and csr.n_splits == 0 and csr.n_items == V
    else:
        rows = [v for v, d in enumerate(deg) if d > DEFAULT_CHUNK]
        assert csr.n_splits == len(rows) and csr.splits[:, 0].tolist() == rows
        assert csr.splits[:, 2].tolist() == [-(-deg[v] // DEFAULT_CHUNK) for v in rows]
        if V >= 2:
            assert csr.splits[:, 2].tolist() == [3, 2] and csr.n_slots == 5
    # edges of a row keep ascending edge id: the order the restatement's index_add_ adds in
    eid = csr.eid
    for v in range(min(V, 8)):
        seg = eid[int(csr.rowptr[v]):int(csr.rowptr[v + 1])]
        assert torch.equal(seg, torch.nonzero(dst == v).flatten())
    y0, yfix, idx = cs.inputs(V, 7)
    assert y0.shape == yfix.shape == (V, 7)
    if V > 1:
        assert 0 in idx.tolist() and 1 not in idx.tolist()


def test_downstream_marks_what_a_split_row_can_reach():
    src = torch.tensor([0, 1, 2, 3])
    dst = torch.tensor([1, 2, 3, 3])
    assert cs.downstream(src, dst, 5, torch.tensor([0]), 0).tolist() == [True, False, False, False, False]
    assert cs.downstream(src, dst, 5, torch.tensor([0]), 2).tolist() == [True, True, True, False, False]
