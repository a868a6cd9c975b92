"""SIRStack(..., dropout=p) on the CPU stand-in modules (tests/cpu_stack_modules.py: the oracle's restated
SIRConv / GraphNorm, which have no fused pass): the stack applies ``self.dropout`` itself at the reference's
position — after the activation and before the residual add (ogbn-arxiv/model.py:70-73), after the activation
in zinc order (zinc/model.py:54-56) — and a stack without dropout draws nothing."""
import pytest
import torch
from torch import nn

import cpu_stack_modules as cpu
from sirgcn.stacks import SIRStack
from sirgcn.synth import molecule_batch

H, LAYERS, P = 16, 3, 0.3


def _stack(order, norm, **kw):
    torch.manual_seed(11)
    stack = SIRStack(cpu.SIRConv, H, LAYERS, nn.LeakyReLU(0.2), "sum", order=order,
                     norm_cls=cpu.GraphNorm if norm else None, **kw)
    if norm:
        with torch.no_grad():
            for n in stack.norms:
                n.weight.uniform_(0.5, 1.5)
                n.bias.normal_()
    return stack


def _inputs():
    g = molecule_batch(4, 9, seed=2)
    gen = torch.Generator().manual_seed(5)
    V = g.num_nodes()
    return g, torch.randn(V, H, generator=gen), torch.randn(V, H, generator=gen)


def _step(fn, stack, X, dY):
    stack.zero_grad(set_to_none=True)
    Xr = X.clone().requires_grad_(True)
    Y = fn(Xr)
    Y.backward(dY)
    return [Y.detach(), Xr.grad] + [p.grad.clone() for p in stack.parameters()]


def _hand_loop(stack, g, h, order, p):
    """The reference's layer loop with nn.Dropout written out at its position."""
    drop = nn.Dropout(p)
    drop.train(stack.training)
    for i, conv in enumerate(stack.convs):
        resid = h
        h = conv(g, h)
        if order == "zinc":
            h = h + resid
        if stack.norms is not None:
            h = stack.norms[i](g, h)
        h = stack.activation(h)
        h = drop(h)
        if order == "arxiv":
            h = h + resid
    return h


CASES = [("arxiv", True), ("zinc", True), ("arxiv", False), ("zinc", False)]


def test_constructor_keeps_the_reference_attribute():
    stack = _stack("arxiv", True, dropout=P)
    assert isinstance(stack.dropout, nn.Dropout) and stack.dropout.p == P
    assert _stack("arxiv", True).dropout.p == 0
    assert _stack("arxiv", True, feat_dropout=0.1, dropout=P).convs[0].dropout.p == 0.1
    # nn.Dropout has no state: the state_dict keys are those of a stack without it
    assert list(stack.state_dict()) == list(_stack("arxiv", True).state_dict())


@pytest.mark.parametrize("order,norm", CASES)
def test_eval_mode_equals_the_stack_without_dropout(order, norm):
    g, X, dY = _inputs()
    a, b = _stack(order, norm, dropout=P).eval(), _stack(order, norm).eval()
    state = torch.get_rng_state()
    ra = _step(lambda x: a(g, x), a, X, dY)
    assert torch.equal(torch.get_rng_state(), state), "eval mode must draw nothing"
    rb = _step(lambda x: b(g, x), b, X, dY)
    assert len(ra) == len(rb)
    for u, v in zip(ra, rb):
        assert torch.equal(u, v)


@pytest.mark.parametrize("order,norm", CASES)
def test_train_mode_equals_the_hand_written_loop(order, norm):
    g, X, dY = _inputs()
    stack = _stack(order, norm, dropout=P).train()
    torch.manual_seed(99)
    got = _step(lambda x: stack(g, x), stack, X, dY)
    torch.manual_seed(99)
    want = _step(lambda x: _hand_loop(stack, g, x, order, P), stack, X, dY)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    # the masks did something, and a second step draws new ones
    plain = _stack(order, norm).train()
    assert not torch.equal(got[0], plain(g, X).detach())
    assert not torch.equal(got[0], stack(g, X).detach())
    assert stack.layer_seeds is None                 # no device seed words on the CPU


@pytest.mark.parametrize("order,norm", CASES)
def test_no_dropout_leaves_the_global_rng_alone(order, norm):
    g, X, dY = _inputs()
    for stack in (_stack(order, norm), _stack(order, norm, dropout=0), _stack(order, norm, dropout=0.0)):
        stack.train()
        state = torch.get_rng_state()
        got = _step(lambda x: stack(g, x), stack, X, dY)
        assert torch.equal(torch.get_rng_state(), state), "a stack without dropout must draw nothing"
        want = _step(lambda x: _hand_loop(stack, g, x, order, 0.0), stack, X, dY)
        for u, v in zip(got, want):
            assert torch.equal(u, v)
