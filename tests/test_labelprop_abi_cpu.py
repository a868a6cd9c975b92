"""CPU-only checks of sir_label_prop_step (added under ABI 17) and of sirgcn.label_spreading /
correct_and_smooth: the symbol is exported and bound, every argument check is synchronous, returns EINVAL and
leaves a sir_last_error text that begins with the function name — no GPU work is issued (the pointers below
are host memory or NULL) — and the Python surface refuses what it must on the CPU."""
import ctypes

import pytest
import torch

import sirgcn
from sirgcn import Graph, _native

EINVAL = 1
SUM, MEAN, SYM = 0, 1, 2
NONE, CLAMP, FIX = 0, 1, 2
NAME = b"sir_label_prop_step: "


def _null():
    return ctypes.c_void_p(None)


def _bufs(n):
    keep = [ctypes.create_string_buffer(256) for _ in range(n)]
    return keep, [ctypes.c_void_p((ctypes.addressof(b) + 15) & ~15) for b in keep]


def _call(lib, **kw):
    """The call with valid defaults (V = 8 rows of F = 8, 8 items, no splits) and the given overrides."""
    a = dict(_DEFAULT)
    a.update(kw)
    return lib.sir_label_prop_step(a["rowptr"], a["col"], a["items"], a["n_items"], a["splits"], a["n_splits"], a["V"],
                                   a["F"], a["Y"], a["ldy"], a["Y0"], a["ldy0"], a["norm"], a["agg"], 0.8, 0.2,
                                   a["post"], 0.0, 1.0, a["fixed"], a["Yfix"], a["ldf"], a["out"], a["ldo"],
                                   a["partial"], _null())


_KEEP, (_P1, _P2, _P3) = _bufs(3)
_DEFAULT = dict(rowptr=_P1, col=_P1, items=_P1, n_items=8, splits=_null(), n_splits=0, V=8, F=8, Y=_P1, ldy=8, Y0=_P2,
                ldy0=8, norm=_P1, agg=SYM, post=NONE, fixed=_null(), Yfix=_null(), ldf=0, out=_P3, ldo=8,
                partial=_null())


def _rejected(lib, text, **kw):
    assert _call(lib, **kw) == EINVAL, kw
    err = lib.sir_last_error()
    assert err.startswith(NAME + text), (kw, err)


def test_symbol_and_version():
    lib = _native.load()
    assert _native.ABI_VERSION == 17 and lib.sir_abi_version() == 17
    assert "sir_label_prop_step" in _native.SIGNATURES and hasattr(lib, "sir_label_prop_step")
    assert len(_native.SIGNATURES["sir_label_prop_step"][1]) == 26
    assert hasattr(_native, "label_prop_step")
    assert (_native.LP_POST_NONE, _native.LP_POST_CLAMP, _native.LP_POST_FIX) == (NONE, CLAMP, FIX)
    assert (_native.AGG["sum"], _native.AGG["mean"], _native.AGG["sym"]) == (SUM, MEAN, SYM)
    for name in ("label_spreading", "correct_and_smooth", "Clamp", "FixRows"):
        assert hasattr(sirgcn, name) and name in sirgcn.__all__


def test_no_rows_is_a_no_op():
    lib = _native.load()
    n = _null()
    for agg in (SUM, MEAN, SYM):
        for post in (NONE, CLAMP, FIX):
            assert _call(lib, V=0, n_items=0, rowptr=n, col=n, items=n, Y=n, Y0=n, out=n, norm=n, agg=agg,
                         post=post, ldf=8) == 0


def test_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    for F in (0, -4, 65537):
        _rejected(lib, b"F must be in [1, 65536]", F=F, ldy=1 << 17, ldy0=1 << 17, ldo=1 << 17)
    _rejected(lib, b"V must be", V=-1)
    for k in ("ldy", "ldy0", "ldo"):
        _rejected(lib, b"leading", **{k: 7})
    _rejected(lib, b"leading", post=FIX, fixed=_P1, Yfix=_P2, ldf=7)
    for agg in (-1, 3, 16):
        _rejected(lib, b"agg must be", agg=agg)
    _rejected(lib, b"SYM needs norm", norm=n)
    assert _call(lib, V=0, norm=n) == 0
    for post in (-1, 3):
        _rejected(lib, b"post must be", post=post)
    _rejected(lib, b"FIX needs fixed and Yfix", post=FIX, fixed=n, Yfix=_P2, ldf=8)
    _rejected(lib, b"FIX needs fixed and Yfix", post=FIX, fixed=_P1, Yfix=n, ldf=8)
    for k in ("Y", "Y0", "out"):
        _rejected(lib, b"NULL", **{k: n})
    _rejected(lib, b"split rows need", n_splits=1, splits=_P1, partial=n)
    _rejected(lib, b"split rows need", n_splits=1, splits=n, partial=_P1)
    _rejected(lib, b"out must not alias Y", out=_P1)
    _rejected(lib, b"negative", n_items=-1)


def _graph():
    return Graph(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 4)


def test_python_surface_on_the_cpu():
    g = _graph()
    # the row count is checked first, before the device
    with pytest.raises(ValueError, match=r"needs \[4, C\]"):
        sirgcn.label_spreading(g, torch.zeros(3, 5))
    with pytest.raises(ValueError, match=r"needs \[4, C\]"):
        sirgcn.label_spreading(g, torch.zeros(4))
    with pytest.raises(RuntimeError, match=r"label_spreading needs a ROCm GPU tensor \(no CPU fallback\)"):
        sirgcn.label_spreading(g, torch.zeros(4, 5))
    with pytest.raises(ValueError, match=r"needs \[4, C\]"):
        sirgcn.correct_and_smooth(g, torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64), torch.tensor([0]))
    with pytest.raises(RuntimeError, match=r"correct_and_smooth needs a ROCm GPU tensor \(no CPU fallback\)"):
        sirgcn.correct_and_smooth(g, torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), torch.tensor([0]))


def test_post_step_descriptors_are_the_reference_callables():
    """Clamp and FixRows called as plain functions do what the reference's post steps do."""
    x = torch.tensor([[-1.0, 0.5], [2.0, float("nan")]])
    c = sirgcn.Clamp(0, 1)(x.clone())
    assert torch.equal(c[0], torch.tensor([0.0, 0.5])) and c[1, 0] == 1.0 and torch.isnan(c[1, 1])
    y = torch.tensor([[7.0, 8.0], [9.0, 10.0]])
    f = sirgcn.FixRows(y, torch.tensor([1]))
    out = f(x.clone())
    assert torch.equal(out[1], y[1]) and torch.equal(out[0], x[0])
    assert f.flag(2, torch.device("cpu")).tolist() == [0, 1] and f.flag(2, torch.device("cpu")) is f.flag(2, torch.device("cpu"))
    assert sirgcn.FixRows(y, torch.tensor([True, False])).flag(2, torch.device("cpu")).tolist() == [1, 0]
