"""CPU-only checks of sirgcn.param_norms / sirgcn.regularizer: CPU tensors take the torch composition and equal
it bit for bit (gradients included), the regularizer is the reference's formula in train and eval mode, and the
host bookkeeping of the native route (chunk count, 16-byte gradient slots, the cached host arrays) agrees with a
brute-force restatement for every list of tests/paramnorm_cases.py."""
import types

import pytest
import torch
from torch import nn

import sirgcn
from sirgcn import regularize

import paramnorm_cases as pc


def _cpu_list(name, kind="normal"):
    specs = pc.lists()[name]
    vals, _ = pc.values(name, kind)
    return pc.materialise(specs, vals, "cpu")[0]


@pytest.mark.parametrize("name", ["sizes", "views", "len1"])
def test_cpu_tensors_take_the_composition_bit_for_bit(name):
    ps, qs = _cpu_list(name), _cpu_list(name)
    l1, l2 = sirgcn.param_norms(ps)
    assert sirgcn.param_norms.last_route == "torch"
    r1, r2 = pc.composition(qs)
    assert torch.equal(l1, r1) and torch.equal(l2, r2)
    g = (torch.tensor(0.3), torch.tensor(0.7))
    ga = torch.autograd.grad((l1, l2), ps, g)
    gb = torch.autograd.grad((r1, r2), qs, g)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


def test_generator_argument_and_grad_mode():
    m = nn.Linear(5, 3)
    l1, l2 = sirgcn.param_norms(m.parameters())
    assert l1.requires_grad and l1.dim() == 0 and l2.dim() == 0
    with torch.no_grad():
        n1, _ = sirgcn.param_norms(m.parameters())
    assert not n1.requires_grad and torch.equal(n1, l1.detach())
    z1, z2 = sirgcn.param_norms([])
    assert float(z1) == 0.0 and float(z2) == 0.0


@pytest.mark.parametrize("training", [True, False])
def test_regularizer_is_the_formula(training):
    torch.manual_seed(3)
    m = nn.Sequential(nn.Linear(7, 5), nn.ReLU(), nn.Linear(5, 2)).train(training)
    args = types.SimpleNamespace(l1=1e-5, l2=1e-6)
    got = sirgcn.regularizer(m, args)
    r1, r2 = pc.composition(list(m.parameters()))
    want = (args.l1 * r1 + args.l2 * r2) * int(m.training)
    assert torch.equal(got, want)
    assert (got.item() > 0) == training
    with torch.no_grad():
        m[0].weight[0, 0] = float("nan")            # int(model.training) multiplies: NaN in eval mode too
    assert torch.isnan(sirgcn.regularizer(m, args))


def test_chunk_and_slot_bookkeeping():
    CH = pc.consts()[0]
    for name, specs in pc.lists().items():
        numels = [n for n, _, _ in specs]
        assert regularize.chunk_count(numels, CH) == pc.chunks_brute(numels, CH), name
        for needs in (tuple(not f for _, _, f in specs), tuple(i % 3 != 1 for i in range(len(specs)))):
            offs, tot = regularize.slot_layout(numels, needs)
            assert (offs, tot) == pc.slots_brute(numels, needs), name
            assert all(o is None or o % 4 == 0 for o in offs) and tot % 4 == 0
            used = [(o, o + n) for o, n in zip(offs, numels) if o is not None]
            assert all(a[1] <= b[0] for a, b in zip(used, used[1:])) and (not used or used[-1][1] <= tot)


def test_plan_holds_the_list_and_is_cached_by_data_ptr():
    ps = _cpu_list("mixed", "exact")
    plan = regularize._plan(ps)
    assert regularize._plan(ps) is plan                                  # same addresses: not rebuilt
    assert plan.T == len(ps)
    assert [plan.params_arr[i] or 0 for i in range(plan.T)] == [p.data_ptr() for p in ps]
    assert list(plan.numel_arr) == [p.numel() for p in ps]
    CH = pc.consts()[0]
    assert plan.n_chunks == pc.chunks_brute([p.numel() for p in ps], CH)
    assert plan.work_floats >= 2 * plan.n_chunks
    moved = list(ps)
    moved[3] = ps[3].detach().clone().requires_grad_(True)               # one parameter moved
    assert moved[3].data_ptr() != ps[3].data_ptr()
    plan2 = regularize._plan(moved)
    assert plan2 is not plan and plan2.params_arr[3] == moved[3].data_ptr()
    assert regularize._plan(ps) is plan
