"""CPU self-check of the exact-arithmetic readout inputs (tests/readout_cases.py): the precondition under
which tests/test_readout_gpu.py may compare the kernels with ``torch.equal``.  For sum, mean and max and their
backwards: the fp32 node-order restatement equals the fp64 one bit for bit (so no summation order and no slab
partition can matter, and sum / n and dP / n round the same way from either), every sum is below 2^24
quarter-units, every input is also a bf16 and an fp16 number, and an exact tie for the maximum occurs on
>= 25 % of the (graph, column) pairs of the graphs with more than one node.  The floor is a condition on the
inputs, not a measurement of the kernels."""
import pytest
import torch

import readout_cases as rc
from sirgcn import _native

R = _native.POOL_SLAB_ROWS
TIE_FLOOR = 0.25
WIDTHS = (1, 3, 75, 260, rc.EXACT_WIDTH)


def test_batch_is_what_the_cases_need():
    ns = rc.sizes(R)
    assert ns == [0, 1, 2, 3, 25, 64, 65, 0, R - 1, R, R + 1, 7, 3 * R + 7, 0]
    assert ns[0] == 0 and ns[-1] == 0 and 0 in ns[1:-1]                   # empty graphs: first, inside, last
    assert {R - 1, R, R + 1} <= set(ns) and max(ns) > 3 * R               # one slab, exactly one, two, four
    off = rc.offsets(ns)
    assert off[-1] == sum(ns) and off.numel() == len(ns) + 1
    # slab slots: graph b owns [b + off[b] // R, b + 1 + off[b+1] // R), enough for its ceil(n / R) slabs
    for b, n in enumerate(ns):
        have = (b + 1 + int(off[b + 1]) // R) - (b + int(off[b]) // R)
        assert have >= max(1, -(-n // R))


def test_inputs_are_16_bit_numbers_and_quarter_integers():
    ns, X, dP = rc.exact_inputs(R)
    assert X.shape == (sum(ns), rc.EXACT_WIDTH) and dP.shape == (len(ns), rc.EXACT_WIDTH)
    for t in (X, dP):
        assert torch.equal((t * 4).round(), t * 4) and t.abs().max() <= 2
        assert int((t * 4).min()) == -8 and int((t * 4).max()) == 8
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(dt).float(), t)


@pytest.mark.parametrize("op", rc.OPS)
def test_fp32_restatement_equals_fp64(op):
    r32, r64 = rc.exact_expected(R, op, torch.float32), rc.exact_expected(R, op)
    ns, X, _ = rc.exact_inputs(R)
    assert torch.equal(r32["arg"], r64["arg"])
    for k in ("P", "dX"):
        a, b = r32[k], r64[k]
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(a.double(), b.float().double()), f"{op} {k}: fp32 differs from fp64 rounded to fp32"
        if op != "mean":
            assert torch.equal(a.double(), b), f"{op} {k}: not an fp32 number"
    # every (partial) sum is an integer number of quarter-units below 2^24
    assert 4 * 2 * max(ns) < 2 ** 24
    if op == "sum":
        assert (r64["P"] * 4).abs().max() < 2 ** 24 and torch.equal((r64["P"] * 4).round(), r64["P"] * 4)
    # empty graphs: zeros and arg -1
    for b, n in enumerate(ns):
        if n == 0:
            assert not r64["P"][b].any() and (op != "max" or bool((r64["arg"][b] == -1).all()))
    if op == "max":
        off = rc.offsets(ns)
        for b, n in enumerate(ns):
            if n > 0:
                assert int(r64["arg"][b].min()) >= 0 and int(r64["arg"][b].max()) < n
                # the gradient sits on one row only
                seg = r64["dX"][off[b]:off[b + 1]]
                assert int((seg != 0).sum(0).max()) <= 1


def test_mean_needs_a_division():
    """dP / n with n = 3, 7, 25, 65 is not dP * (1 / n) everywhere: a reciprocal multiply would be caught."""
    ns, _, dP = rc.exact_inputs(R)
    differ = 0
    for b, n in enumerate(ns):
        if n > 0:
            nf = torch.full((dP.shape[1],), n, dtype=torch.float32)
            differ += int((dP[b] / nf != dP[b] * (1.0 / nf)).sum())
    assert differ > 0


@pytest.mark.parametrize("F", WIDTHS)
def test_max_ties_meet_the_floor(F):
    ns, X, _ = rc.exact_inputs(R)
    share = rc.tie_share(X[:, :F], ns)
    assert share >= TIE_FLOOR, f"F={F}: exact ties on {share:.3f} of the (graph, column) pairs"
