"""CPU-only checks of the six layer-dropout entry points of the fused norms (added under ABI 17, new symbols
only): exported, bound, and every argument check synchronous — its code and its sir_last_error text with host
or NULL pointers and no GPU work."""
import ctypes

import pytest

from sirgcn import _native

NEW = ("sir_batch_norm_act_drop_fwd", "sir_batch_norm_act_drop_bwd", "sir_layer_norm_act_drop_fwd",
       "sir_layer_norm_act_drop_bwd", "sir_graph_norm_act_drop_fwd", "sir_graph_norm_act_drop_bwd")
EINVAL = 1


def _null():
    return ctypes.c_void_p(None)


def _buf():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def _drop(p=0.2, seed=5):
    return ctypes.byref(_native.Dropout(seed, p, None))


def _bn_fwd(lib, X, ldx, M, N, mean, invstd, w, b, act, R, ldr, Y, ldy, drop):
    return lib.sir_batch_norm_act_drop_fwd(X, ldx, M, N, mean, invstd, w, b, act, 0.2, R, ldr, Y, ldy, drop, _null())


def _bn_bwd(lib, X, ldx, D, ldg, M, N, mean, invstd, w, b, act, dX, lddx, dw, db, work, drop):
    return lib.sir_batch_norm_act_drop_bwd(X, ldx, D, ldg, M, N, mean, invstd, w, b, act, 0.2, 1, dX, lddx, dw, db,
                                           work, drop, _null())


def _ln_fwd(lib, X, ldx, M, N, w, b, act, R, ldr, Y, ldy, mean, rstd, drop):
    return lib.sir_layer_norm_act_drop_fwd(X, ldx, M, N, w, b, 1e-5, act, 0.2, R, ldr, Y, ldy, mean, rstd, drop,
                                           _null())


def _ln_bwd(lib, X, ldx, D, ldg, M, N, w, b, mean, rstd, act, dX, lddx, dwp, dbp, ldp, drop):
    return lib.sir_layer_norm_act_drop_bwd(X, ldx, D, ldg, M, N, w, b, mean, rstd, act, 0.2, dX, lddx, dwp, dbp, ldp,
                                           drop, _null())


def _gn_fwd(lib, off, B, F, X, ldx, w, b, ms, act, R, ldr, Y, ldy, mean, std, drop):
    return lib.sir_graph_norm_act_drop_fwd(off, B, F, X, ldx, w, b, ms, 1e-5, act, 0.2, R, ldr, Y, ldy, mean, std,
                                           drop, _null())


def _gn_bwd(lib, off, B, F, X, ldx, D, ldg, w, b, ms, mean, std, act, dX, lddx, dwp, dmp, dbp, drop):
    return lib.sir_graph_norm_act_drop_bwd(off, B, F, X, ldx, D, ldg, w, b, ms, mean, std, act, 0.2, dX, lddx, dwp,
                                           dmp, dbp, drop, _null())


def test_symbols_and_version():
    lib = _native.load()
    assert _native.ABI_VERSION == 17 and lib.sir_abi_version() == 17
    for name in NEW:
        assert name in _native.SIGNATURES and hasattr(lib, name)
        sibling = name.replace("_drop", "")
        # the sibling's argument list with one pointer (the sir_dropout_t*) before the stream
        res, args = _native.SIGNATURES[sibling]
        assert _native.SIGNATURES[name] == (res, args[:-1] + [ctypes.c_void_p] + args[-1:]), name
        # bound: the sibling's wrapper calls this entry when it is given the dropout, as its last parameter `drop`
        wrapper = getattr(_native, sibling[len("sir_"):])
        code = wrapper.__code__
        assert code.co_varnames[code.co_argcount - 1] == "drop" and wrapper.__defaults__ == (None,), name


def test_empty_work_is_a_no_op():
    lib = _native.load()
    n = _null()
    for drop in (n, _drop()):
        for act in (0, 1, 2):
            assert _bn_fwd(lib, n, 75, 0, 75, n, n, n, n, act, n, 0, n, 75, drop) == 0
            assert _bn_bwd(lib, n, 75, n, 75, 0, 75, n, n, n, n, act, n, 75, n, n, n, drop) == 0
            assert _ln_fwd(lib, n, 75, 0, 75, n, n, act, n, 0, n, 75, n, n, drop) == 0
            assert _ln_bwd(lib, n, 75, n, 75, 0, 75, n, n, n, n, act, n, 75, n, n, 76, drop) == 0
            assert _gn_fwd(lib, n, 0, 75, n, 75, n, n, n, act, n, 0, n, 75, n, n, drop) == 0
            assert _gn_bwd(lib, n, 0, 75, n, 75, n, 75, n, n, n, n, n, act, n, 75, n, n, n, drop) == 0


@pytest.mark.parametrize("with_drop", [False, True])
def test_batch_norm_drop_argument_checks(with_drop):
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    d = _drop() if with_drop else n
    for N in (0, -4, 65537):
        assert _bn_fwd(lib, p, 1 << 17, 4, N, p, p, p, p, 0, n, 0, p, 1 << 17, d) == EINVAL
        assert b"sir_batch_norm_act_drop_fwd: N must be in [1, 65536]" in lib.sir_last_error()
        assert _bn_bwd(lib, p, 1 << 17, p, 1 << 17, 4, N, p, p, p, p, 0, p, 1 << 17, p, p, p, d) == EINVAL
        assert b"sir_batch_norm_act_drop_bwd: N must be in [1, 65536]" in lib.sir_last_error()
    assert _bn_fwd(lib, p, 8, -1, 8, p, p, p, p, 0, n, 0, p, 8, d) == EINVAL
    assert b"M out of range" in lib.sir_last_error()
    for ldx, ldr, ldy in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _bn_fwd(lib, p, ldx, 4, 8, p, p, p, p, 2, p, ldr, p, ldy, d) == EINVAL
        assert b"sir_batch_norm_act_drop_fwd: leading" in lib.sir_last_error()
    for lds in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _bn_bwd(lib, p, lds[0], p, lds[1], 4, 8, p, p, p, p, 2, p, lds[2], p, p, p, d) == EINVAL
        assert b"sir_batch_norm_act_drop_bwd: leading" in lib.sir_last_error()
    for act in (-1, 3, 4, 9):
        assert _bn_fwd(lib, p, 8, 4, 8, p, p, p, p, act, n, 0, p, 8, d) == EINVAL
        assert b"act must be" in lib.sir_last_error()
        assert _bn_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, act, p, 8, p, p, p, d) == EINVAL
        assert b"act must be" in lib.sir_last_error()
    for a in range(6):
        args = [p] * 6
        args[a] = n
        assert _bn_fwd(lib, args[0], 8, 4, 8, args[1], args[2], args[3], args[4], 2, n, 0, args[5], 8, d) == EINVAL
        assert b"sir_batch_norm_act_drop_fwd: NULL" in lib.sir_last_error()
    for a in range(10):
        args = [p] * 10
        args[a] = n
        assert _bn_bwd(lib, args[0], 8, args[1], 8, 4, 8, args[2], args[3], args[4], args[5], 2, args[6], 8, args[7],
                       args[8], args[9], d) == EINVAL
        assert b"sir_batch_norm_act_drop_bwd: NULL" in lib.sir_last_error()
    odd = ctypes.c_void_p(p.value + 4)
    assert _bn_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, 2, p, 8, p, p, odd, d) == EINVAL
    assert b"8-B aligned" in lib.sir_last_error()
    del keep


@pytest.mark.parametrize("with_drop", [False, True])
def test_layer_norm_drop_argument_checks(with_drop):
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    d = _drop() if with_drop else n
    for N in (0, -4, 1025, 2048):
        assert _ln_fwd(lib, p, 4096, 4, N, p, p, 2, n, 0, p, 4096, p, p, d) == EINVAL
        assert b"sir_layer_norm_act_drop_fwd: N must be in [1, 1024]" in lib.sir_last_error()
        assert _ln_bwd(lib, p, 4096, p, 4096, 4, N, p, p, p, p, 2, p, 4096, p, p, 4096, d) == EINVAL
        assert b"sir_layer_norm_act_drop_bwd: N must be in [1, 1024]" in lib.sir_last_error()
    assert _ln_fwd(lib, p, 8, -1, 8, p, p, 2, n, 0, p, 8, p, p, d) == EINVAL
    assert b"M out of range" in lib.sir_last_error()
    for ldx, ldr, ldy in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _ln_fwd(lib, p, ldx, 4, 8, p, p, 2, p, ldr, p, ldy, p, p, d) == EINVAL
        assert b"sir_layer_norm_act_drop_fwd: leading" in lib.sir_last_error()
    for lds in ((7, 8, 8, 8), (8, 7, 8, 8), (8, 8, 7, 8), (8, 8, 8, 7)):
        assert _ln_bwd(lib, p, lds[0], p, lds[1], 4, 8, p, p, p, p, 2, p, lds[2], p, p, lds[3], d) == EINVAL
        assert b"sir_layer_norm_act_drop_bwd: leading" in lib.sir_last_error()
    for act in (-1, 3, 4, 9):
        assert _ln_fwd(lib, p, 8, 4, 8, p, p, act, n, 0, p, 8, p, p, d) == EINVAL
        assert b"act must be" in lib.sir_last_error()
        assert _ln_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, act, p, 8, p, p, 8, d) == EINVAL
        assert b"act must be" in lib.sir_last_error()
    for a in range(6):
        args = [p] * 6
        args[a] = n
        assert _ln_fwd(lib, args[0], 8, 4, 8, args[1], args[2], 2, n, 0, args[3], 8, args[4], args[5], d) == EINVAL
        assert b"sir_layer_norm_act_drop_fwd: NULL" in lib.sir_last_error()
    for a in range(9):
        args = [p] * 9
        args[a] = n
        assert _ln_bwd(lib, args[0], 8, args[1], 8, 4, 8, args[2], args[3], args[4], args[5], 2, args[6], 8, args[7],
                       args[8], 8, d) == EINVAL
        assert b"sir_layer_norm_act_drop_bwd: NULL" in lib.sir_last_error()
    del keep


@pytest.mark.parametrize("with_drop", [False, True])
def test_graph_norm_drop_argument_checks(with_drop):
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    d = _drop() if with_drop else n
    for F in (0, -4, 65537):
        assert _gn_fwd(lib, p, 2, F, p, 1 << 17, p, p, p, 2, n, 0, p, 1 << 17, p, p, d) == EINVAL
        assert b"sir_graph_norm_act_drop_fwd: bad shape" in lib.sir_last_error()
        assert _gn_bwd(lib, p, 2, F, p, 1 << 17, p, 1 << 17, p, p, p, p, p, 2, p, 1 << 17, p, p, p, d) == EINVAL
        assert b"sir_graph_norm_act_drop_bwd: bad shape" in lib.sir_last_error()
    assert _gn_fwd(lib, p, -1, 8, p, 8, p, p, p, 2, n, 0, p, 8, p, p, d) == EINVAL
    assert b"bad shape" in lib.sir_last_error()
    for ldx, ldr, ldy in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _gn_fwd(lib, p, 2, 8, p, ldx, p, p, p, 2, p, ldr, p, ldy, p, p, d) == EINVAL
        assert b"sir_graph_norm_act_drop_fwd: leading" in lib.sir_last_error()
    for lds in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _gn_bwd(lib, p, 2, 8, p, lds[0], p, lds[1], p, p, p, p, p, 2, p, lds[2], p, p, p, d) == EINVAL
        assert b"sir_graph_norm_act_drop_bwd: leading" in lib.sir_last_error()
    for act in (-1, 3, 4, 9):
        assert _gn_fwd(lib, p, 2, 8, p, 8, p, p, p, act, n, 0, p, 8, p, p, d) == EINVAL
        assert b"act must be" in lib.sir_last_error()
        assert _gn_bwd(lib, p, 2, 8, p, 8, p, 8, p, p, p, p, p, act, p, 8, p, p, p, d) == EINVAL
        assert b"act must be" in lib.sir_last_error()
    # required buffers (bias and mean_scale are optional): off, X, weight, Y, mean, std
    for a in range(6):
        args = [p] * 6
        args[a] = n
        assert _gn_fwd(lib, args[0], 2, 8, args[1], 8, args[2], n, n, 2, n, 0, args[3], 8, args[4], args[5], d) == EINVAL
        assert b"sir_graph_norm_act_drop_fwd: NULL" in lib.sir_last_error()
    # off, X, dY, weight, mean, std, dX, dw_part, db_part
    for a in range(9):
        args = [p] * 9
        args[a] = n
        assert _gn_bwd(lib, args[0], 2, 8, args[1], 8, args[2], 8, args[3], n, n, args[4], args[5], 2, args[6], 8,
                       args[7], n, args[8], d) == EINVAL
        assert b"sir_graph_norm_act_drop_bwd: NULL" in lib.sir_last_error()
    assert _gn_bwd(lib, p, 2, 8, p, 8, p, 8, p, p, p, p, p, 2, p, 8, p, n, p, d) == EINVAL
    assert b"dms_part needed" in lib.sir_last_error()
    del keep


def test_nan_probability_is_einval_everywhere():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    nan = _drop(p=float("nan"))
    calls = {
        "sir_batch_norm_act_drop_fwd": lambda: _bn_fwd(lib, p, 8, 4, 8, p, p, p, p, 2, n, 0, p, 8, nan),
        "sir_batch_norm_act_drop_bwd": lambda: _bn_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, 2, p, 8, p, p, p, nan),
        "sir_layer_norm_act_drop_fwd": lambda: _ln_fwd(lib, p, 8, 4, 8, p, p, 2, n, 0, p, 8, p, p, nan),
        "sir_layer_norm_act_drop_bwd": lambda: _ln_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, 2, p, 8, p, p, 8, nan),
        "sir_graph_norm_act_drop_fwd": lambda: _gn_fwd(lib, p, 2, 8, p, 8, p, p, p, 2, n, 0, p, 8, p, p, nan),
        "sir_graph_norm_act_drop_bwd": lambda: _gn_bwd(lib, p, 2, 8, p, 8, p, 8, p, p, p, p, p, 2, p, 8, p, p, p, nan),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() == EINVAL
        assert lib.sir_last_error() == (name + ": dropout p is NaN").encode()
    del keep
