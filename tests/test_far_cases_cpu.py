"""CPU self-check of tests/far_cases.py: the layout arithmetic on the full-size numbers (pure integers, nothing
allocated), the embed / check harness on the scaled-down layout (CPU tensors), and graphs N and E from their
COO.  No GPU, no plan build."""
import pytest
import torch

import far_cases as fc
import poison_cases as pc

ITEMSIZES = (4, 2)


# ----------------------------------------------------------------------------- layout arithmetic, full size
@pytest.mark.parametrize("itemsize", ITEMSIZES)
def test_marks_lie_inside_and_the_last_row_is_far(itemsize):
    L = fc.FULL
    assert (L.ld, L.m, L.front) == (4096, 2 ** 19 + 300, 2 ** 31)
    marks = L.marks(itemsize)
    assert marks == ([2 ** 17, 2 ** 18, 2 ** 19] if itemsize == 4 else [2 ** 18, 2 ** 19])
    assert all(0 < m < L.m for m in marks)
    at = {m: L.offset(m) * itemsize for m in marks}
    if itemsize == 4:
        assert at[2 ** 17] == 2 ** 31 and at[2 ** 18] == 2 ** 32 and L.offset(2 ** 19) == 2 ** 31
        assert L.offset(L.m - 1) * 4 > 2 ** 33
    else:
        assert at[2 ** 18] == 2 ** 31 and at[2 ** 19] == 2 ** 32 and L.offset(2 ** 19) == 2 ** 31
        assert L.offset(L.m - 1) * 2 > 2 ** 32
    # the documented limits the layout stays inside: the direct GEMM route's 128 * lda < 2^29, and a 256-row
    # tile of the buffer-resource GEMMs spans 4 MiB (tile-local 32-bit offsets stay legitimate)
    assert 128 * L.ld < 2 ** 29 and 256 * L.ld * 4 == 4 * 2 ** 20
    assert abs(L.total * 4 / 2 ** 30 - 16.0) < 0.2 and abs(L.total * 2 / 2 ** 30 - 8.0) < 0.1
    assert all(c + 1024 <= L.ld for c in fc.COLS)


@pytest.mark.parametrize("itemsize", ITEMSIZES)
def test_mark_rows_cover_both_sides_of_every_mark(itemsize):
    L = fc.FULL
    rows = L.mark_rows(itemsize)
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == L.m - 1
    assert len(rows) == 64 * (2 + 2 * len(L.marks(itemsize)))
    have = set(rows)
    assert set(range(64)) <= have and set(range(L.m - 64, L.m)) <= have
    for m in L.marks(itemsize):
        assert set(range(m - 64, m + 64)) <= have


@pytest.mark.parametrize("itemsize", ITEMSIZES)
@pytest.mark.parametrize("kind,unit", fc.TRUNCATIONS)
def test_every_truncation_lands_inside_the_arena(kind, unit, itemsize):
    """For every row of MARK_ROWS and every operand column: origin + f(offset) is an element of the arena (never
    a fault), and from the truncation's own mark on it is another element than origin + offset (a wrong kernel
    cannot pass).  The uint32 truncation of the element offset has no mark below M * LD < 2^32 elements."""
    L = fc.FULL
    first = L.trunc_mark(kind, unit, itemsize)
    if (kind, unit) == ("uint32", "element"):
        assert first is None
    else:
        assert first in L.marks(itemsize)
    for row in L.mark_rows(itemsize):
        for col in fc.COLS:
            off = L.offset(row)                     # a kernel adds the truncated row offset to base = origin + col
            at = L.origin + col + L.truncate(kind, unit, off, itemsize)
            assert 0 <= at < L.total, (kind, unit, row, col)
            if first is not None and row >= first:
                assert at != L.origin + col + off
                assert L.wrapped_row(kind, unit, row, itemsize) != row
            else:
                assert at == L.origin + col + off


def test_scaled_layout_has_the_same_shape():
    S = fc.SMALL
    assert S.marks(4) == [16, 32, 64] and S.marks(2) == [32, 64]
    assert {k: S.trunc_mark(*k, 4) for k in fc.TRUNCATIONS} == \
        {("int32", "element"): 64, ("uint32", "element"): None, ("int32", "byte"): 16, ("uint32", "byte"): 32}
    for kind, unit in fc.TRUNCATIONS:
        for row in S.mark_rows(4):
            for col in fc.SMALL_COLS:
                assert 0 <= S.origin + col + S.truncate(kind, unit, S.offset(row), 4) < S.total


# ----------------------------------------------------------------------------- the harness, scaled down
def _copy_rows(arena, X, Y, wrap=None):
    """Y[r] = 2 X[r] as a kernel would compute it; ``wrap`` = (kind, unit): with that truncation of the row
    offset on the read side."""
    S, flat = arena.layout, arena.store.view(arena.dtype)
    x0, y0 = X.storage_offset(), Y.storage_offset()
    for r in range(X.shape[0]):
        off = S.offset(r) if wrap is None else S.truncate(*wrap, S.offset(r), arena.itemsize)
        Y[r] = 2 * flat[x0 + off:x0 + off + X.shape[1]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_harness_passes_a_correct_kernel_and_detects_each_fault(dtype):
    S = fc.SMALL
    arena = fc.Arena(S, dtype.itemsize)
    data = fc.ints((S.m, 2), 4, 5, dtype)

    def run(wrap=None):
        arena.open(dtype)
        X = arena.put(data, fc.SMALL_COLS[0])
        Y = arena.out(S.m, 2, fc.SMALL_COLS[2])
        _copy_rows(arena, X, Y, wrap)
        return X, Y

    X, Y = run()
    assert X.stride(0) == S.ld and X.storage_offset() == S.origin and torch.equal(X, data)
    arena.check(Y, 2 * data, "correct")
    arena.close("correct")
    assert bool((arena.store == pc.SENTINEL[dtype]).all()), "close leaves the arena filled"

    # one flipped bit outside: before the origin, between two operands' columns, in the tail guard
    for at in (3, S.origin + S.offset(40, 3), S.origin + S.offset(S.m - 1, S.ld - 1), S.total - 1):
        X, Y = run()
        arena.store[at] ^= 1
        arena.check(Y, 2 * data, "flip")
        with pytest.raises(AssertionError, match="outside the logical operands"):
            arena.close("flip")
    # one unwritten element inside
    X, Y = run()
    pc.bits(Y)[S.m - 2, 1] = pc.SENTINEL[dtype]
    with pytest.raises(AssertionError, match="never written"):
        arena.check(Y, 2 * data, "unwritten")
    # an input the call wrote to
    X, Y = run()
    X[50, 0] += 1
    with pytest.raises(AssertionError, match="input operand 0 was written"):
        arena.close("input")
    # a value taken from a wrapped row: every truncation that has a mark in this layout
    for kind, unit in fc.TRUNCATIONS:
        X, Y = run((kind, unit))
        if S.trunc_mark(kind, unit, dtype.itemsize) is None:
            arena.check(Y, 2 * data, "identity")
            continue
        with pytest.raises(AssertionError, match="never written|differ from the reference"):
            arena.check(Y, 2 * data, f"{kind} {unit}")
    # put_rows: the rows a call does not depend on hold the sentinel
    arena.open(dtype)
    rows = S.mark_rows(dtype.itemsize)
    X = arena.put_rows(rows, data[rows], S.m, 0)
    assert torch.equal(X[rows], data[rows]) and bool(torch.isnan(X[20]).all())
    with pytest.raises(AssertionError, match="overlap"):
        arena.out(S.m, 2, 1)
    arena.close("put_rows")


def test_integer_outputs_use_the_four_byte_arena():
    S = fc.SMALL
    arena = fc.Arena(S, 4).open(torch.float32)
    arg = arena.out(S.m, 2, 4, torch.int32)
    assert bool((arg == pc.SENTINEL[torch.float32]).all())
    want = torch.arange(2 * S.m, dtype=torch.int32).view(S.m, 2) - 1
    arg.copy_(want)
    arena.check(arg, want, "arg")
    arg[70, 1] = pc.SENTINEL[torch.float32]
    with pytest.raises(AssertionError, match="never written"):
        arena.check(arg, want, "arg")
    arena.close("arg")


# ----------------------------------------------------------------------------- graphs, from the COO
def _both_sides(ids, marks, what):
    for m in marks:
        assert bool(((ids >= m - 64) & (ids < m)).any()) and bool(((ids >= m) & (ids < m + 64)).any()), (what, m)


def test_graph_n_has_the_stated_degrees():
    src, dst, V, deg = fc.graph_n()
    rows = fc.mark_rows(4)
    marks = fc.FULL.marks(4)
    hubs = (5, 2 ** 19 + 7)
    assert V == fc.M and src.numel() == dst.numel() and 2000 < src.numel() < 20000
    ind = torch.bincount(dst, minlength=V)
    assert int((ind > 0).sum()) <= len(rows) and set(torch.nonzero(ind).flatten().tolist()) <= set(rows)
    for i, r in enumerate(rows):
        assert int(ind[r]) == (fc.HUB_DEGREE if r in hubs else fc.LADDER[i % 8]), r
    assert set(src.tolist()) <= set(rows)
    for ids, what in ((src, "src"), (dst, "dst")):
        _both_sides(ids, marks, what)
        assert bool((ids < 64).any()) and bool((ids >= V - 64).any())
    # gathers reach far rows from near rows and the reverse
    assert bool(((dst < 64) & (src >= 2 ** 19)).any()) and bool(((dst >= 2 ** 19) & (src < 64)).any())
    # the 16-bit marks are a subset: the same graph serves every dtype
    assert set(fc.mark_rows(2)) <= set(rows)
    again = fc.graph_n()
    assert torch.equal(again[0], src) and torch.equal(again[1], dst)


def test_graph_e_has_the_stated_degrees():
    src, dst, V, deg = fc.graph_e()
    E = src.numel()
    assert V == 4096 and E == fc.M == sum(deg) and len(deg) == V
    ind = torch.bincount(dst, minlength=V)
    assert ind.tolist() == deg
    split = [d for d in deg if d > 256]
    assert split == [fc.HUB_DEGREE, fc.HUB_DEGREE] and deg[5] == fc.HUB_DEGREE
    rowptr = torch.tensor([0] + deg).cumsum(0)
    row_of = lambda p: int(torch.searchsorted(rowptr, p, right=True)) - 1
    marks = fc.FULL.marks(4)
    hub2 = row_of(marks[-1])
    assert deg[hub2] == fc.HUB_DEGREE and rowptr[hub2] < marks[-1] < rowptr[hub2 + 1], "a split row crosses 2^31 elements"
    for m in marks[:-1]:            # ladder rows on both sides of the mark, and a row boundary near it
        lo, hi = row_of(m - 64), row_of(m + 63)
        assert hi > lo and all(deg[v] in fc.LADDER for v in range(lo, hi + 1))
    assert set(fc.LADDER) <= set(deg[row_of(marks[-1]) + 1:]) | set(deg[:64]), "ladder rows after the last mark"
    assert deg[:5] == list(fc.LADDER[:5]) and 0 in deg and bool((src < V).all()) and int(src.min()) >= 0
    assert len(set(src.tolist())) > V // 2


def test_batch_offsets_straddle_the_marks():
    off, sizes = fc.batch_offsets()
    assert int(off[-1]) == fc.M and len(sizes) == off.numel() - 1
    assert sizes[:6] == list(fc.BATCH_SIZES) and 0 in sizes[6:]
    for m in fc.FULL.marks(4):
        b = int(torch.searchsorted(off, m, right=True)) - 1
        assert off[b] <= m < off[b + 1]
        assert any(off[b + k] < m + 1100 for k in (1, 2)), "a graph boundary lies near the mark"
