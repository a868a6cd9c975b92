"""CPU-only checks of the BatchNorm / LayerNorm entry points (added under ABI 17): the symbols are
exported and bound, and every argument check is synchronous, returns its code and leaves a
sir_last_error text — no GPU work is issued (the pointers below are host memory or NULL)."""
import ctypes

from sirgcn import _native

NEW = ("sir_batch_norm_work_floats", "sir_batch_norm_stats", "sir_batch_norm_act_fwd", "sir_batch_norm_act_bwd",
       "sir_layer_norm_bwd_parts", "sir_layer_norm_act_fwd", "sir_layer_norm_act_bwd")
EINVAL = 1


def _null():
    return ctypes.c_void_p(None)


def _buf():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def _stats(lib, X, ldx, M, N, rm, rv, mean, invstd, work):
    return lib.sir_batch_norm_stats(X, ldx, M, N, 1e-5, 0.1, rm, rv, mean, invstd, work, _null())


def _bn_fwd(lib, X, ldx, M, N, mean, invstd, w, b, act, R, ldr, Y, ldy):
    return lib.sir_batch_norm_act_fwd(X, ldx, M, N, mean, invstd, w, b, act, 0.2, R, ldr, Y, ldy, _null())


def _bn_bwd(lib, X, ldx, D, ldg, M, N, mean, invstd, w, b, act, dX, lddx, dw, db, work):
    return lib.sir_batch_norm_act_bwd(X, ldx, D, ldg, M, N, mean, invstd, w, b, act, 0.2, 1, dX, lddx, dw, db, work,
                                      _null())


def _ln_fwd(lib, X, ldx, M, N, w, b, act, R, ldr, Y, ldy, mean, rstd):
    return lib.sir_layer_norm_act_fwd(X, ldx, M, N, w, b, 1e-5, act, 0.2, R, ldr, Y, ldy, mean, rstd, _null())


def _ln_bwd(lib, X, ldx, D, ldg, M, N, w, b, mean, rstd, act, dX, lddx, dwp, dbp, ldp):
    return lib.sir_layer_norm_act_bwd(X, ldx, D, ldg, M, N, w, b, mean, rstd, act, 0.2, dX, lddx, dwp, dbp, ldp, _null())


def test_symbols_and_version():
    lib = _native.load()
    assert _native.ABI_VERSION == 17 and lib.sir_abi_version() == 17
    for name in NEW:
        assert name in _native.SIGNATURES and hasattr(lib, name)
    for name in ("batch_norm_stats", "batch_norm_act_fwd", "batch_norm_act_bwd", "layer_norm_act_fwd",
                 "layer_norm_act_bwd"):
        assert hasattr(_native, name)


def test_sizing_calls():
    lib = _native.load()
    R = _native.BN_SLAB_ROWS
    assert R == 128
    # two [slabs, N] fp64 arrays of per-slab partials + [2, N] fp64; a function of (M, N) alone
    assert lib.sir_batch_norm_work_floats(0, 75) == 0
    assert lib.sir_batch_norm_work_floats(1, 75) == 8 * 75
    assert lib.sir_batch_norm_work_floats(R, 256) == 8 * 256
    assert lib.sir_batch_norm_work_floats(R + 1, 256) == 12 * 256
    assert lib.sir_batch_norm_work_floats(3 * R + 7, 1) == 4 * 4 + 4
    for M, N in ((-1, 4), (4, 0), (4, 65537)):
        assert lib.sir_batch_norm_work_floats(M, N) == -1
    # LayerNorm backward: at least 16 rows per partial row, at most 8192 partial rows
    assert lib.sir_layer_norm_bwd_parts(0, 64) == 0
    assert lib.sir_layer_norm_bwd_parts(1, 64) == 1
    assert lib.sir_layer_norm_bwd_parts(16, 64) == 1
    assert lib.sir_layer_norm_bwd_parts(17, 64) == 2
    assert lib.sir_layer_norm_bwd_parts(1000, 300) == 63
    assert lib.sir_layer_norm_bwd_parts(2_000_000, 256) == 8164        # 245 rows each
    for M, N in ((-1, 4), (4, 0), (4, 1025)):
        assert lib.sir_layer_norm_bwd_parts(M, N) == -1


def test_empty_work_is_a_no_op():
    lib = _native.load()
    n = _null()
    assert _stats(lib, n, 75, 0, 75, n, n, n, n, n) == 0
    for act in (0, 1, 2):
        assert _bn_fwd(lib, n, 75, 0, 75, n, n, n, n, act, n, 0, n, 75) == 0
        assert _bn_bwd(lib, n, 75, n, 75, 0, 75, n, n, n, n, act, n, 75, n, n, n) == 0
        assert _ln_fwd(lib, n, 75, 0, 75, n, n, act, n, 0, n, 75, n, n) == 0
        assert _ln_bwd(lib, n, 75, n, 75, 0, 75, n, n, n, n, act, n, 75, n, n, 76) == 0


def test_batch_norm_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    # N out of range
    for N in (0, -4, 65537):
        assert _stats(lib, p, 1 << 17, 4, N, n, n, p, p, p) == EINVAL
        assert b"sir_batch_norm_stats: N must be" in lib.sir_last_error()
        assert _bn_fwd(lib, p, 1 << 17, 4, N, p, p, p, p, 0, n, 0, p, 1 << 17) == EINVAL
        assert b"N must be" in lib.sir_last_error()
        assert _bn_bwd(lib, p, 1 << 17, p, 1 << 17, 4, N, p, p, p, p, 0, p, 1 << 17, p, p, p) == EINVAL
        assert b"N must be" in lib.sir_last_error()
    assert _stats(lib, p, 8, -1, 8, n, n, p, p, p) == EINVAL
    assert b"M out of range" in lib.sir_last_error()
    # leading dimensions below N (X; X, R, Y; X, dY, dX)
    assert _stats(lib, p, 7, 4, 8, n, n, p, p, p) == EINVAL
    assert b"leading" in lib.sir_last_error()
    for ldx, ldr, ldy in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _bn_fwd(lib, p, ldx, 4, 8, p, p, p, p, 2, p, ldr, p, ldy) == EINVAL
        assert b"sir_batch_norm_act_fwd: leading" in lib.sir_last_error()
    for lds in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _bn_bwd(lib, p, lds[0], p, lds[1], 4, 8, p, p, p, p, 2, p, lds[2], p, p, p) == EINVAL
        assert b"sir_batch_norm_act_bwd: leading" in lib.sir_last_error()
    # activations outside identity / relu / leaky_relu
    for act in (-1, 3, 4, 9):
        assert _bn_fwd(lib, p, 8, 4, 8, p, p, p, p, act, n, 0, p, 8) == EINVAL
        assert b"act must be" in lib.sir_last_error()
        assert _bn_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, act, p, 8, p, p, p) == EINVAL
        assert b"act must be" in lib.sir_last_error()
    # NULL buffers when there is work
    for a in range(4):
        args = [p, p, p, p]
        args[a] = n
        assert _stats(lib, args[0], 8, 4, 8, n, n, args[1], args[2], args[3]) == EINVAL
        assert b"NULL" in lib.sir_last_error()
    for a in range(6):
        args = [p] * 6
        args[a] = n
        assert _bn_fwd(lib, args[0], 8, 4, 8, args[1], args[2], args[3], args[4], 2, n, 0, args[5], 8) == EINVAL
        assert b"NULL" in lib.sir_last_error()
    for a in range(10):
        args = [p] * 10
        args[a] = n
        assert _bn_bwd(lib, args[0], 8, args[1], 8, 4, 8, args[2], args[3], args[4], args[5], 2, args[6], 8, args[7],
                       args[8], args[9]) == EINVAL
        assert b"NULL" in lib.sir_last_error()
    # the running buffers come as a pair, and their update needs two rows
    assert _stats(lib, p, 8, 4, 8, p, n, p, p, p) == EINVAL
    assert b"both or neither" in lib.sir_last_error()
    assert _stats(lib, p, 8, 1, 8, p, p, p, p, p) == EINVAL
    assert b"M >= 2" in lib.sir_last_error()
    # the fp64 partials live in `work`
    odd = ctypes.c_void_p(p.value + 4)
    assert _stats(lib, p, 8, 4, 8, n, n, p, p, odd) == EINVAL
    assert b"8-B aligned" in lib.sir_last_error()
    assert _bn_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, 2, p, 8, p, p, odd) == EINVAL
    assert b"8-B aligned" in lib.sir_last_error()
    del keep


def test_layer_norm_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    for N in (0, -4, 1025, 2048):
        assert _ln_fwd(lib, p, 4096, 4, N, p, p, 2, n, 0, p, 4096, p, p) == EINVAL
        assert b"sir_layer_norm_act_fwd: N must be in [1, 1024]" in lib.sir_last_error()
        assert _ln_bwd(lib, p, 4096, p, 4096, 4, N, p, p, p, p, 2, p, 4096, p, p, 4096) == EINVAL
        assert b"sir_layer_norm_act_bwd: N must be in [1, 1024]" in lib.sir_last_error()
    assert _ln_fwd(lib, p, 8, -1, 8, p, p, 2, n, 0, p, 8, p, p) == EINVAL
    assert b"M out of range" in lib.sir_last_error()
    for ldx, ldr, ldy in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert _ln_fwd(lib, p, ldx, 4, 8, p, p, 2, p, ldr, p, ldy, p, p) == EINVAL
        assert b"leading" in lib.sir_last_error()
    for lds in ((7, 8, 8, 8), (8, 7, 8, 8), (8, 8, 7, 8), (8, 8, 8, 7)):
        assert _ln_bwd(lib, p, lds[0], p, lds[1], 4, 8, p, p, p, p, 2, p, lds[2], p, p, lds[3]) == EINVAL
        assert b"leading" in lib.sir_last_error()
    for act in (-1, 3, 4, 9):
        assert _ln_fwd(lib, p, 8, 4, 8, p, p, act, n, 0, p, 8, p, p) == EINVAL
        assert b"act must be" in lib.sir_last_error()
        assert _ln_bwd(lib, p, 8, p, 8, 4, 8, p, p, p, p, act, p, 8, p, p, 8) == EINVAL
        assert b"act must be" in lib.sir_last_error()
    for a in range(6):
        args = [p] * 6
        args[a] = n
        assert _ln_fwd(lib, args[0], 8, 4, 8, args[1], args[2], 2, n, 0, args[3], 8, args[4], args[5]) == EINVAL
        assert b"NULL" in lib.sir_last_error()
    for a in range(9):
        args = [p] * 9
        args[a] = n
        assert _ln_bwd(lib, args[0], 8, args[1], 8, 4, 8, args[2], args[3], args[4], args[5], 2, args[6], 8, args[7],
                       args[8], 8) == EINVAL
        assert b"NULL" in lib.sir_last_error()
    del keep
