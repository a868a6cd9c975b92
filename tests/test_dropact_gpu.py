"""``sirgcn.drop_act`` — ``act(dropout(y)) + r`` in one native pass per direction (``sir_drop_act_fwd`` / ``_bwd``) on
the MI355X.

The mask is the one ``sir_dropout_apply`` writes for an [M, N] block at col0 = 0 (m = keep * scale), and the pass
rounds to the storage type wherever torch's separate kernels would, so for Identity / ReLU / LeakyReLU
  forward : out == act(where(m != 0, y * m, 0).to(dt)) + r
  backward: every gradient == autograd through that expression
bit for bit, in fp32, bf16 and fp16, with an fp32 or a 16-bit r.  The GELUs are held to the project's parity rule in
fp32 (``conftest.assert_parity``: 1e-5, or no worse than twice the error of torch's own fp32 composition against fp64)
and to units in the last place in 16-bit:

* one rounding (no r; the gradient without dropout): |ours - t| <= ulp(t), t the fp64 result from the same 16-bit
  inputs — a correctly rounded value plus an fp32 error that can move it across one rounding boundary — wherever
  that premise holds (the fp32 formula's own error E, derived in the test, is below a quarter ulp: nearly every
  element), and |ours - t| <= ulp(t) / 2 + 2 E everywhere (GELU's fp32 formulas cancel in the negative tail);
* two roundings (the 16-bit add of r after the rounded activation; the gradient's ``* scale`` after the rounded
  act'): the first value's budget carried through the second op plus the second's own rounding.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import assert_parity

import sirgcn
from sirgcn import _native, drop_act

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x1234_5678_9ABC

# one thread of four columns; one block; rows that end inside a block; more than one block (grid-stride over rows of
# 19 / 64 / 129 vectors)
SHAPES = [(1, 4), (2, 8), (129, 76), (257, 256), (130, 516)]
COMPOSED_SHAPES = [(3, 5), (130, 75)]              # N % 4 != 0: the torch composition on the same mask
EXACT_ACTS = {"identity": nn.Identity, "relu": nn.ReLU, "leaky": lambda: nn.LeakyReLU(0.2)}
GELUS = {"gelu": lambda: nn.GELU(), "gelu_tanh": lambda: nn.GELU(approximate="tanh")}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PS = (0.2, 0.5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _mask(M, N, seed, p):
    """m = keep * scale: the bits sir_dropout_apply writes for an [M, N] block at col0 = 0."""
    return _native.dropout_apply(torch.ones(M, N, device=DEV), (seed, p))


def _seed_with_both(M, N, p, seed=SEED):
    """The first seed from ``seed`` on whose [M, N] mask drops something and keeps something (a four-element mask
    keeps everything for many seeds)."""
    for s in range(seed, seed + 64):
        m = _mask(M, N, s, p)
        if 0 < int((m == 0).sum()) < m.numel():
            return s, m
    raise AssertionError(f"no seed in 64 gives a mixed [{M}, {N}] mask at p = {p}")


def _data(M, N, dt, seed=0):
    g = torch.Generator().manual_seed(1000 * M + N + seed)
    y = (1.5 * torch.randn(M, N, generator=g)).to(DEV).to(dt)
    dout = torch.randn(M, N, generator=g).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV)
    return y, r, dout


def _composed(y, act, r, m):
    """The expression the pass is defined by, from torch's own kernels."""
    d = y if m is None else torch.where(m != 0, y * m, 0.0).to(y.dtype)
    a = act(d)
    return a if r is None else a + r


def _step(fn, y, r, dout):
    y = y.clone().requires_grad_(True)
    r = r.clone().requires_grad_(True) if r is not None else None
    out = fn(y, r)
    out.backward(dout.to(out.dtype))
    return out.detach(), y.grad, (r.grad if r is not None else None)


def _spy(monkeypatch):
    calls = []
    for name in ("drop_act_fwd", "drop_act_bwd"):
        orig = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _o=orig, _n=name, **k: calls.append(_n) or _o(*a, **k))
    return calls


def _r_variants(r, dt):
    """No residual, an fp32 one and — for a 16-bit y — one of y's own type."""
    return [None, r] + ([r.to(dt)] if dt != torch.float32 else [])


# ------------------------------------------------------------------ Identity / ReLU / LeakyReLU: exact
@pytest.mark.parametrize("dt_name", list(DTYPES))
@pytest.mark.parametrize("act_name", list(EXACT_ACTS))
@pytest.mark.parametrize("M,N", SHAPES)
def test_forward_and_backward_are_exact(M, N, act_name, dt_name, monkeypatch):
    dt, act = DTYPES[dt_name], EXACT_ACTS[act_name]()
    y, r, dout = _data(M, N, dt)
    calls = _spy(monkeypatch)
    for p in PS:
        seed, m = _seed_with_both(M, N, p)
        for rv in _r_variants(r, dt):
            del calls[:]
            got = _step(lambda y_, r_: drop_act(y_, act, r_, (seed, p)), y, rv, dout)
            assert calls == ["drop_act_fwd", "drop_act_bwd"], calls
            want = _step(lambda y_, r_: _composed(y_, act, r_, m), y, rv, dout)
            assert got[0].dtype == want[0].dtype and got[1].dtype == dt
            what = f"p {p} r {None if rv is None else rv.dtype}"
            assert torch.equal(got[0], want[0]), f"forward ({what})"
            assert torch.equal(got[1], want[1]), f"dy ({what})"
            if rv is not None:
                assert torch.equal(got[2], want[2]) and torch.equal(got[2], dout.to(rv.dtype)), f"dr ({what})"


@pytest.mark.parametrize("M,N", COMPOSED_SHAPES)
def test_other_shapes_take_the_composition_on_the_same_mask(M, N, monkeypatch):
    calls = _spy(monkeypatch)
    for dt in DTYPES.values():
        y, r, dout = _data(M, N, dt)
        for act in (nn.LeakyReLU(0.2), nn.GELU()):
            seed, m = _seed_with_both(M, N, 0.5)
            got = _step(lambda y_, r_: drop_act(y_, act, r_, (seed, 0.5)), y, r, dout)
            want = _step(lambda y_, r_: _composed(y_, act, r_, m), y, r, dout)
            for u, v in zip(got, want):
                assert torch.equal(u, v)
    assert calls == []


def test_column_slice_of_a_wider_tensor_with_nan_padding(monkeypatch):
    """Rows with ld > N: the padding is never read and never written."""
    M, N, p = 129, 76, 0.5
    calls = _spy(monkeypatch)
    for dt in DTYPES.values():
        y, r, dout = _data(M, N, dt)

        def sliced(x):
            wide = torch.full((M, N + 8), float("nan"), device=DEV, dtype=x.dtype)
            wide[:, 4:4 + N] = x
            return wide[:, 4:4 + N]
        act = nn.LeakyReLU(0.2)
        base = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, p)), y, r.to(dt), dout)
        ys = sliced(y).detach().requires_grad_(True)
        rs = sliced(r.to(dt))
        del calls[:]
        out = drop_act(ys, act, rs, (SEED, p))
        out.backward(sliced(dout.to(out.dtype)))
        assert calls == ["drop_act_fwd", "drop_act_bwd"], calls
        assert torch.equal(out, base[0]) and torch.equal(ys.grad, base[1])


def test_empty_input(monkeypatch):
    for shape in ((0, 8), (0, 5)):
        y = torch.empty(shape, device=DEV, requires_grad=True)
        out = drop_act(y, nn.GELU(), None, (SEED, 0.5))
        assert out.shape == shape
        out.sum().backward()
        assert y.grad.shape == shape


# ------------------------------------------------------------------ GELU
def _truth(y, act, r, m, rounded):
    """The fp64 composition from the same inputs; ``rounded`` (a 16-bit type): with the storage roundings the pass
    is defined with (after the dropout, after the activation)."""
    y64 = y.detach().double().requires_grad_(True)
    d = y64 if m is None else torch.where(m != 0, y64 * m.double(), 0.0)
    if rounded is not None:
        d = d + (d.detach().to(rounded).double() - d.detach())          # round, straight-through
    a = act(d)
    return y64, d, a, (a if r is None else a + r.double())


@pytest.mark.parametrize("act_name", list(GELUS))
@pytest.mark.parametrize("M,N", [(129, 76), (130, 516)])
def test_gelu_fp32_parity(M, N, act_name, monkeypatch):
    act = GELUS[act_name]()
    y, r, dout = _data(M, N, torch.float32)
    calls = _spy(monkeypatch)
    for p in (0.0, 0.2):
        m = _mask(M, N, SEED, p) if p else None
        for rv in (None, r):
            got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, p)), y, rv, dout)
            ref = _step(lambda y_, r_: _composed(y_, act, r_, m), y, rv, dout)
            y64, _, _, t = _truth(y, act, rv, m, None)
            t.backward(dout.double())
            assert_parity(got[0], ref[0], t.detach(), what=f"{act_name} out p {p}")
            assert_parity(got[1], ref[1], y64.grad, what=f"{act_name} dy p {p}")
    assert calls == ["drop_act_fwd", "drop_act_bwd"] * 4


def _ulp(t, dt):
    """The spacing of ``dt`` at the magnitude of the fp64 values ``t`` (the subnormal spacing below the normals)."""
    fi = torch.finfo(dt)
    mant = {torch.bfloat16: 7, torch.float16: 10}[dt]
    e = torch.floor(torch.log2(t.abs().clamp_min(fi.smallest_normal)))
    return torch.pow(2.0, e - mant)


def _within(err, t, E, dt, what, carried=0.0, coverage=0.9):
    """|err| <= ulp(t) / 2 + 2 E (+ ``carried``) everywhere: the rounding of a value that carries the fp32 error E.
    Where the premise of the one-ulp budget holds — 2 E <= ulp(t) / 2, the fp32 error can move the value across one
    rounding boundary at most — that is within ONE ulp of t, asserted as such (single roundings: ``carried`` 0), and
    the premise must hold for at least ``coverage`` of the elements, so that the check is not vacuous (the data is
    1.5 * randn, times 1.25 under dropout: about 6 % of it lies below z = -2.9, where 1 + erf has lost more digits than
    fp16 keeps)."""
    ulp = _ulp(t, dt)
    bound = 0.5 * ulp + 2 * E + carried
    assert bool((err <= bound).all()), f"{what}: {(err / bound).max().item():.3f} of the bound"
    premise = 2 * E <= 0.5 * ulp
    assert premise.double().mean().item() >= coverage, f"{what}: premise holds for {premise.double().mean().item():.3f}"
    if isinstance(carried, float) and carried == 0.0:
        worst = (err / ulp)[premise].max().item()
        print(f"{what}: worst {worst:.3f} ulp where the premise holds ({premise.double().mean().item():.4f} of all)")
        assert worst <= 1.0, f"{what}: {worst:.3f} ulp"


@pytest.mark.parametrize("dt_name", ["bf16", "f16"])
@pytest.mark.parametrize("act_name", list(GELUS))
def test_gelu_16bit_is_within_an_ulp_of_fp64(act_name, dt_name):
    """The fp32 formulas' own absolute error against fp64, from their operations (ulp32 = 2^-24 at values <= 1):
    forward z * 0.5 * (1 + erf(z k)) and 0.5 z (1 + tanh(u)): the cancelling factor 1 + erf / 1 + tanh carries
    <= 2^-22 (erff / tanhf a few ulp32 at |value| <= 1, the argument's rounding through a slope <= 1.13, the add),
    the two products 2^-23 of the result: E = (|z| + |t|) 2^-21 with a margin of two.  Backward dout (cdf + z pdf) and
    the tanh form's five-term derivative: every term is <= 1 in magnitude with a few ulp32 each:
    E = |dout| 2^-20 + |t| 2^-22.  E is far below a 16-bit ulp except where the formula cancels — the negative tail
    (1 + erf -> 0: torch's own kernels lose the same digits there) and the zero of GELU' near z = -0.75 — so the
    premise covers nearly every element of this data; outside it the bound is the rounding plus E."""
    M, N = 130, 516
    dt, act = DTYPES[dt_name], GELUS[act_name]()
    y, r, dout = _data(M, N, dt)
    r, dout = r.to(dt), dout.to(dt)
    d64 = dout.double()
    for p in (0.0, 0.2):
        m = _mask(M, N, SEED, p) if p else None
        scale = m.max().item() if p else 1.0
        # one rounding forward: no residual
        got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, p)), y, None, dout)
        _, d, a, t = _truth(y, act, None, m, dt)
        assert got[0].dtype == dt
        z, t = d.detach(), t.detach()
        E = (z.abs() + t.abs()) * 2.0 ** -21
        _within((got[0].double() - t).abs(), t, E, dt, f"out p {p}")
        # the gradient: act'(d) * dout rounded once; with dropout, * scale rounded again
        g, = torch.autograd.grad(a, d, d64)
        Eg = d64.abs() * 2.0 ** -20 + g.abs() * 2.0 ** -22
        if m is None:
            _within((got[1].double() - g).abs(), g, Eg, dt, f"dy p {p}")
        else:
            tg = torch.where(m != 0, g * scale, 0.0)
            carried = torch.where(m != 0, scale * (0.5 * _ulp(g, dt) + 2 * Eg), 0.0)
            _within((got[1].double() - tg).abs(), tg, torch.zeros_like(tg), dt, f"dy p {p}", carried=carried)
            assert bool((got[1][m == 0] == 0).all())
        # two roundings forward: the 16-bit add of a 16-bit residual after the rounded activation
        got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, p)), y, r, dout)
        _, _, a, t = _truth(y, act, r, m, dt)
        a, t = a.detach(), t.detach()
        carried = 0.5 * _ulp(a, dt) + 2 * E + 0.5 * _ulp(t, dt)          # (+ half an ulp: the sum may change binade)
        _within((got[0].double() - t).abs(), t, torch.zeros_like(t), dt, f"out + r p {p}", carried=carried)
        assert torch.equal(got[2], dout)


# ------------------------------------------------------------------ identity cases, seeds, non-finite values
@pytest.mark.parametrize("dt_name", list(DTYPES))
def test_p_zero_none_and_eval_give_the_result_without_dropout(dt_name):
    dt = DTYPES[dt_name]
    M, N = 129, 76
    y, r, dout = _data(M, N, dt)
    for act in (nn.LeakyReLU(0.2), nn.GELU()):
        base = _step(lambda y_, r_: drop_act(y_, act, r_), y, r, dout)
        if isinstance(act, nn.LeakyReLU):
            want = _step(lambda y_, r_: _composed(y_, act, r_, None), y, r, dout)
            assert all(torch.equal(u, v) for u, v in zip(base, want))
        for kw in (dict(dropout=None), dict(dropout=(SEED, 0.0)), dict(dropout=(SEED, 0)),
                   dict(dropout=(SEED, 0.5), training=False)):
            got = _step(lambda y_, r_: drop_act(y_, act, r_, **kw), y, r, dout)
            assert all(torch.equal(u, v) for u, v in zip(got, base)), kw


@pytest.mark.parametrize("dt_name", list(DTYPES))
def test_p_one_drops_everything(dt_name):
    dt = DTYPES[dt_name]
    y, r, dout = _data(129, 76, dt)
    for act in (nn.LeakyReLU(0.2), nn.GELU(), nn.GELU(approximate="tanh"), nn.ReLU(), nn.Identity()):
        got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, 1.0)), y, r, dout)
        assert torch.equal(got[0], r) and torch.equal(got[2], dout)          # act(0) = 0 for all five
        assert torch.equal(got[1], torch.zeros_like(y))
        got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, 1.0)), y, None, dout)
        assert torch.equal(got[0], torch.zeros_like(y)) and not torch.signbit(got[0]).any()


def test_bad_probabilities_are_refused():
    y = torch.randn(5, 8, device=DEV)
    for p in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError, match="between 0 and 1"):
            drop_act(y, nn.ReLU(), None, (SEED, p))
    with pytest.raises(RuntimeError, match="sir_drop_act_fwd: dropout p is NaN"):
        _native.drop_act_fwd(y, None, 1, 0.0, torch.empty_like(y), (SEED, float("nan")))


def test_device_seed_equals_seed_by_value_and_words_differ():
    M, N = 129, 76
    y, r, dout = _data(M, N, torch.float32)
    act = nn.GELU()
    word = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    by_value = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, 0.2)), y, r, dout)
    by_word = _step(lambda y_, r_: drop_act(y_, act, r_, (word, 0.2)), y, r, dout)
    assert all(torch.equal(u, v) for u, v in zip(by_value, by_word))
    other = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED + 1, 0.2)), y, r, dout)
    assert not torch.equal(other[0], by_value[0]) and not torch.equal(other[1], by_value[1])
    assert not torch.equal(_mask(M, N, SEED, 0.2), _mask(M, N, SEED + 1, 0.2))


@pytest.mark.parametrize("dt_name", list(DTYPES))
def test_dropped_elements_are_zero_whatever_they_held(dt_name):
    """A dropped element is +0 before the activation (a NaN or an Inf there reaches neither the output nor the
    gradient), a kept one propagates, and a NaN of r comes through exactly where r holds it."""
    dt = DTYPES[dt_name]
    M, N, p = 9, 76, 0.5
    y, r, dout = _data(M, N, dt)
    m = _mask(M, N, SEED, p)
    bad = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    bad[:, ::3] = True
    y = torch.where(bad, torch.tensor(float("nan"), device=DEV, dtype=dt), y)
    y[:, 3::6] = float("inf")
    y[:, 6::12] = float("-inf")
    nonfinite = ~torch.isfinite(y)
    assert (nonfinite & (m == 0)).any() and (nonfinite & (m != 0)).any()
    r[4, 7] = r[4, 70] = float("nan")
    dirty = dout.clone()
    dirty[m == 0] = float("nan")                      # an incoming NaN at a dropped position is not multiplied in
    for act in (nn.Identity(), nn.ReLU(), nn.LeakyReLU(0.2), nn.GELU(), nn.GELU(approximate="tanh")):
        out, dy, _ = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, p)), y, r, dirty)
        dropped = (m == 0) & ~torch.isnan(r)
        assert torch.equal(out[dropped], r[dropped]), type(act).__name__        # act(+0) + r = r
        assert bool((dy[m == 0] == 0).all())
        kept_nan = torch.isnan(y) & (m != 0)
        assert bool(torch.isnan(out[kept_nan]).all())
        assert bool(torch.isnan(out[4, 7])) and bool(torch.isnan(out[4, 70]))
        finite_in = ~nonfinite & ~torch.isnan(r)
        assert bool(torch.isfinite(out[finite_in]).all())
        if isinstance(act, nn.Identity):
            kept_inf = torch.isinf(y) & (m != 0) & ~torch.isnan(r)
            assert torch.equal(out[kept_inf], y[kept_inf].to(out.dtype))        # +-Inf * scale + r = +-Inf


def test_activation_forms_map_to_the_same_pass(monkeypatch):
    y, r, dout = _data(129, 76, torch.float32)
    calls = _spy(monkeypatch)
    pairs = [(F.gelu, nn.GELU()), (torch.relu, nn.ReLU()), (F.relu, nn.ReLU()), (None, nn.Identity()),
             (F.leaky_relu, nn.LeakyReLU(0.01))]
    for form, module in pairs:
        a = _step(lambda y_, r_: drop_act(y_, form, r_, (SEED, 0.2)), y, r, dout)
        b = _step(lambda y_, r_: drop_act(y_, module, r_, (SEED, 0.2)), y, r, dout)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert calls == ["drop_act_fwd", "drop_act_bwd"] * (2 * len(pairs))
    # an activation without a code: the composition, on the same mask
    del calls[:]
    m = _mask(129, 76, SEED, 0.2)
    got = _step(lambda y_, r_: drop_act(y_, torch.tanh, r_, (SEED, 0.2)), y, r, dout)
    want = _step(lambda y_, r_: _composed(y_, torch.tanh, r_, m), y, r, dout)
    assert calls == [] and all(torch.equal(u, v) for u, v in zip(got, want))


def test_a_hook_on_the_activation_selects_the_composition(monkeypatch):
    y, r, dout = _data(129, 76, torch.float32)
    act = nn.GELU()
    fused = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, 0.2)), y, r, dout)
    calls = _spy(monkeypatch)
    seen = []
    handle = act.register_forward_hook(lambda mod, args, out: seen.append(args[0].detach()))
    got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, 0.2)), y, r, dout)
    handle.remove()
    assert calls == [] and len(seen) == 1
    m = _mask(129, 76, SEED, 0.2)
    assert torch.equal(seen[0], torch.where(m != 0, y * m, 0.0))           # the hook saw the dropout's output
    assert_parity(got[0], fused[0], fused[0].double(), what="hooked out")
    got = _step(lambda y_, r_: drop_act(y_, act, r_, (SEED, 0.2)), y, r, dout)
    assert calls == ["drop_act_fwd", "drop_act_bwd"]


def test_exported():
    assert sirgcn.drop_act is drop_act
