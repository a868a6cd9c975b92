"""TEST INFRASTRUCTURE: the "far" embedding of tests/test_far_offsets_gpu.py and its CPU self-check,
tests/test_far_cases_cpu.py — operands whose later rows lie past every 32-bit mark of ``base + row * ld + col``
while the work stays tiny (used next to tests/poison_cases.py, whose sentinels it shares).

Layout.  A logical [M, N] operand is a column slice of one wide row-major buffer: leading dimension LD = 4096
elements, M = 2^19 + 300 rows.  With 4-byte elements row 2^17 starts at 2^31 bytes, row 2^18 at 2^32 bytes and
row 2^19 at 2^31 elements; with 2-byte elements row 2^18 is at 2^31 bytes and row 2^19 at 2^32 bytes and 2^31
elements.  MARK_ROWS (``Layout.mark_rows``) are the rows a test gives work to: the first 64, 64 on either side of
every mark, the last 64.  All float operands of one call are views into ONE arena per element size at column
offsets 0, 1024, 2048, 3072 (a call with more operands takes further multiples of 256 between them), like the
[Q|K] pair buffer of the product; integer outputs use the 4-byte arena through an integer view.

The front guard is the point of the design.  The arena holds FRONT = 2^31 sentinel elements BEFORE the origin
(row 0, column 0), then M * LD elements, then a GUARD tail.  Every classic truncation of an offset — to int32 or
to uint32, of the element offset or of the byte offset — moves an access by at most 2^31 elements backwards, so
``origin + f(offset)`` still lies inside the arena: a kernel with a missing 64-bit cast reads sentinel NaN (or
another row's distinct values) or overwrites a sentinel, and fails an assertion.  It does not fault the device.
(The uint32 truncation of the ELEMENT offset is the identity here: M * LD < 2^32 elements.  Its mark would need
an arena of twice the size; the other three truncations each have a mark inside [0, M).)

Checks (``Arena.check`` / ``Arena.close``): the logical output equals the reference, no sentinel is left inside
it, every input is bit-unchanged, and every sentinel outside the registered views is bit-unchanged — scanned on
the arena's own device in slices of at most 2^28 elements, never through an arena-sized mask.

The layout arithmetic is pure-integer and never allocates (``Layout``); ``SMALL`` is the same layout scaled down
(LD = 8, the marks at rows 16, 32 and 64) for the CPU self-check of the harness.  Nothing here touches the GPU at
import; ``Arena`` allocates on the device it is given."""
import torch

import exact_cases as xc
import poison_cases as pc

LD = 4096
M = 2 ** 19 + 300
FRONT = 2 ** 31
GUARD = LD
COLS = (0, 1024, 2048, 3072)
SLICE = 2 ** 28
LADDER = (0, 1, 2, 3, 5, 17, 64, 65)
HUB_DEGREE = 700                    # split at the 256-edge chunk
TRUNCATIONS = tuple((kind, unit) for kind in ("int32", "uint32") for unit in ("element", "byte"))
_STORE = {4: torch.int32, 2: torch.int16}


class Layout:
    """Pure-integer layout arithmetic of one arena: offsets are in elements from the arena's first element.
    ``bits`` is the width of the truncated offset (32; the scaled-down layout uses fewer)."""

    def __init__(self, ld=LD, m=M, front=FRONT, guard=GUARD, bits=32, span=64):
        self.ld, self.m, self.front, self.guard, self.bits, self.span = ld, m, front, guard, bits, span

    @property
    def origin(self):
        return self.front

    @property
    def total(self):
        return self.front + self.m * self.ld + self.guard

    def offset(self, row, col=0):
        """Element offset of (row, col) from the origin."""
        return row * self.ld + col

    def trunc_mark(self, kind, unit, itemsize):
        """The first row whose offset the truncation (kind, unit) changes, or None if it lies past M."""
        limit = 2 ** (self.bits - 1) if kind == "int32" else 2 ** self.bits
        step = self.ld * (itemsize if unit == "byte" else 1)
        row = -(-limit // step)
        return row if row < self.m else None

    def marks(self, itemsize):
        """The rows at 2^31 bytes, 2^32 bytes and 2^31 elements (those inside [0, M)), ascending."""
        rows = {self.trunc_mark(k, u, itemsize) for k, u in TRUNCATIONS}
        return sorted(r for r in rows if r is not None)

    def mark_rows(self, itemsize):
        """MARK_ROWS: rows 0 .. span-1, (mark - span) .. (mark + span - 1) for every mark, the last span rows."""
        rows = set(range(min(self.span, self.m))) | set(range(max(self.m - self.span, 0), self.m))
        for mark in self.marks(itemsize):
            rows |= set(range(max(mark - self.span, 0), min(mark + self.span, self.m)))
        return sorted(rows)

    def truncate(self, kind, unit, off, itemsize):
        """What a kernel computes for the element offset ``off`` when it holds the element (or byte) offset in a
        32-bit signed (or unsigned) register: the truncated offset, in elements."""
        x = off * itemsize if unit == "byte" else off
        x %= 2 ** self.bits
        if kind == "int32" and x >= 2 ** (self.bits - 1):
            x -= 2 ** self.bits
        return x // itemsize if unit == "byte" else x

    def wrapped_row(self, kind, unit, row, itemsize):
        """The row a truncated access to ``row`` lands in (it may be negative: inside the front guard)."""
        return self.truncate(kind, unit, self.offset(row), itemsize) // self.ld


FULL = Layout()
# the same layout scaled down: 10-bit offsets, so with 4-byte elements the marks are rows 16, 32 and 64
SMALL = Layout(ld=8, m=64 + 12, front=2 ** 9, guard=8, bits=10, span=4)
SMALL_COLS = (0, 2, 4, 6)


def mark_rows(itemsize=4):
    return FULL.mark_rows(itemsize)


class Arena:
    """One sentinel-filled allocation of ``layout.total`` elements of ``itemsize`` bytes.  ``open(dtype)`` starts a
    call (the whole arena holds ``dtype``'s sentinel), ``put`` / ``put_rows`` / ``out`` hand out the views,
    ``check`` compares an output, ``close`` runs the outside check and leaves the arena clean."""

    def __init__(self, layout, itemsize, device="cpu"):
        self.layout, self.itemsize, self.device = layout, itemsize, device
        self.store = torch.empty((layout.total,), dtype=_STORE[itemsize], device=device)
        self.dtype, self.sentinel, self.views = None, None, []

    @property
    def nbytes(self):
        return self.layout.total * self.itemsize

    def open(self, dtype):
        assert dtype.itemsize == self.itemsize and dtype.is_floating_point
        self.dtype, self.sentinel, self.views = dtype, pc.SENTINEL[dtype], []
        self.store.fill_(self.sentinel)
        return self

    def _view(self, rows, n, col, dtype):
        L = self.layout
        dtype = dtype or self.dtype
        assert dtype.itemsize == self.itemsize and 0 < rows <= L.m and n > 0 and 0 <= col and col + n <= L.ld
        assert L.origin + L.offset(rows - 1, col) + n <= L.total - L.guard
        for v, _ in self.views:             # operands of one call never share a column
            c0 = (v.storage_offset() - L.origin) % L.ld
            assert col + n <= c0 or c0 + v.shape[1] <= col, "views overlap"
        return self.store.view(dtype).as_strided((rows, n), (L.ld, 1), L.origin + col)

    def put(self, t, col):
        """The input ``t`` [rows, N] (any device) as a view at column ``col``; checked bit-unchanged by close."""
        v = self._view(t.shape[0], t.shape[1], col, t.dtype)
        v.copy_(t)
        self.views.append((v, pc.bits(v.contiguous())))
        return v

    def put_rows(self, rows, vals, n_rows, col):
        """An input of ``n_rows`` rows holding ``vals`` in the rows ``rows`` and the sentinel everywhere else (the
        rows a call must not depend on)."""
        v = self._view(n_rows, vals.shape[1], col, vals.dtype)
        v[torch.as_tensor(rows, device=self.device)] = vals.to(self.device)
        self.views.append((v, pc.bits(v.contiguous())))
        return v

    def out(self, rows, n, col, dtype=None, seed=None):
        """An output view: sentinel-filled, or holding ``seed`` (in-place and accumulating entries)."""
        v = self._view(rows, n, col, dtype)
        if seed is not None:
            v.copy_(seed)
        self.views.append((v, None))
        return v

    def check_written(self, view, what, rows=None):
        """No sentinel is left inside the logical output (``rows``: only these rows are the call's to write);
        returns the output as a contiguous tensor (of those rows)."""
        got = view.contiguous()
        if rows is not None:
            got = got[torch.as_tensor(rows, device=got.device)]
        # an integer output is an integer view of the 4-byte arena: it holds the float sentinel's bits
        left = pc.bits(got) == pc.SENTINEL[torch.float32 if got.dtype == torch.int32 else got.dtype]
        if bool(left.any()):
            i = torch.nonzero(left)[0].tolist()
            raise AssertionError(f"{what}: {int(left.sum())} elements of the logical output were never written (first "
                                 f"in row {i[0] if rows is None else int(rows[i[0]])} column {i[1]})")
        return got

    def check(self, view, want, what, rows=None):
        """The logical output (its rows ``rows``) holds no sentinel and equals ``want``."""
        got = self.check_written(view, what, rows)
        want = want.to(got.device)
        assert got.shape == want.shape and got.dtype == want.dtype, what
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got) if got.dtype.is_floating_point else got != want
            i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the reference, first "
                                 f"in row {i[0] if rows is None else int(rows[i[0]])} column {i[1]}: "
                                 f"got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}")

    def close(self, what):
        """Every input is bit-unchanged; then, with the registered views blanked, the whole arena holds the
        sentinel (scanned in slices): nothing outside the views was written.  Leaves the arena filled."""
        L = self.layout
        for k, (v, snap) in enumerate(self.views):
            if snap is not None:
                assert torch.equal(pc.bits(v.contiguous()), snap), f"{what}: input operand {k} was written"
        for v, _ in self.views:
            pc.bits(v).fill_(self.sentinel)
        self.views = []
        n_bad = torch.zeros((), dtype=torch.int64, device=self.device)
        bounds = [(s, min(s + SLICE, L.total)) for s in range(0, L.total, SLICE)]
        for s, e in bounds:
            n_bad += (self.store[s:e] != self.sentinel).sum()
        if int(n_bad):
            for s, e in bounds:
                hit = torch.nonzero(self.store[s:e] != self.sentinel)
                if hit.numel():
                    at = s + int(hit[0]) - L.origin
                    self.store.fill_(self.sentinel)
                    raise AssertionError(f"{what}: {int(n_bad)} elements outside the logical operands were written, "
                                         f"first at element {at} from the origin (row {at // L.ld}, column {at % L.ld})")


# ----------------------------------------------------------------------------- data
def ints(shape, bound, seed, dtype=torch.float32):
    """Seeded integers in [-bound, bound]: a row is its own draw, so a read from a wrapped row cannot give the
    right answer (up to the 1 in (2 bound + 1)^N chance per row, and a test compares hundreds of rows)."""
    return xc.ints(shape, bound, seed).to(dtype)


# ----------------------------------------------------------------------------- graphs
def _ladder_edges(rows, hubs, sources, gen):
    """(src, dst, degree-by-row): row ``rows[i]`` receives LADDER[i % 8] edges, a row of ``hubs`` HUB_DEGREE; the
    sources are drawn from ``sources``."""
    deg = {r: LADDER[i % len(LADDER)] for i, r in enumerate(rows)}
    for h in hubs:
        deg[h] = HUB_DEGREE
    dst = torch.tensor([r for r in sorted(deg) for _ in range(deg[r])], dtype=torch.int64)
    pool = torch.as_tensor(sources, dtype=torch.int64)
    src = pool[torch.randint(0, pool.numel(), (dst.numel(),), generator=gen)]
    return src, dst, deg


def graph_n(layout=FULL, itemsize=4, seed=31):
    """Graph N (node-far): V = M nodes; every row of MARK_ROWS receives an in-degree of the ladder (cycling), row 5
    and row (last mark + 7) are hubs of 700 in-edges; sources are drawn from MARK_ROWS (gathers reach far rows
    from near rows and the reverse); every other row has degree 0.  Returns (src, dst, V, degree-by-row), the
    edge ids shuffled."""
    gen = torch.Generator().manual_seed(seed)
    rows = layout.mark_rows(itemsize)
    hubs = (5, layout.marks(itemsize)[-1] + 7)
    src, dst, deg = _ladder_edges(rows, hubs, rows, gen)
    p = torch.randperm(dst.numel(), generator=gen)
    return src[p].contiguous(), dst[p].contiguous(), layout.m, deg


E_NODES = 4096
E_FILL = 140                        # in-degree of the filler rows between the ladder blocks (one chunk, unsplit)


def graph_e_degrees(layout=FULL, n_nodes=E_NODES, fill=E_FILL, hub=HUB_DEGREE):
    """In-degrees of graph E's nodes, ascending node id, E = M edges in all: a block of ``span`` ladder rows at
    the start (node 5 a hub of 700 in-edges) and one around every mark but the last, so that the edge positions
    on both sides of those marks belong to ladder rows; a second hub crosses the last mark (two thirds of what
    lies past the mark are its edges), with ladder rows before it and after it up to the last edge; filler rows
    of ``fill`` edges in between, zero-degree rows after the last edge."""
    E, marks = layout.m, layout.marks(4)
    block = [LADDER[i % len(LADDER)] for i in range(layout.span)]
    deg = []

    def fill_to(t):
        pos = sum(deg)
        assert t >= pos, "the ladder blocks overlap"
        deg.extend([fill] * ((t - pos) // fill) + ([(t - pos) % fill] if (t - pos) % fill else []))

    def ladder(until=None):
        for d in block:
            deg.append(d if until is None else min(d, until - sum(deg)))

    ladder()
    deg[5] = hub
    for m in marks[:-1]:
        fill_to(m - sum(block) // 2)
        ladder()
    hub_start = marks[-1] - hub + (E - marks[-1]) * 2 // 3
    fill_to(hub_start - sum(block))
    ladder()
    deg.append(hub)
    while sum(deg) < E:
        ladder(E)
    assert sum(deg) == E and len(deg) <= n_nodes, (sum(deg), len(deg))
    return deg + [0] * (n_nodes - len(deg))


def graph_e(layout=FULL, n_nodes=E_NODES, fill=E_FILL, seed=37):
    """Graph E (edge-far): V = 4096 nodes, E = M edges, so [E, *] operands are far.  Returns (src, dst, V, degrees)."""
    gen = torch.Generator().manual_seed(seed)
    deg = graph_e_degrees(layout, n_nodes, fill)
    dst = torch.repeat_interleave(torch.arange(n_nodes), torch.tensor(deg))
    src = torch.randint(0, n_nodes, (dst.numel(),), generator=gen)
    p = torch.randperm(dst.numel(), generator=gen)
    return src[p].contiguous(), dst[p].contiguous(), n_nodes, deg


BATCH_SIZES = (0, 1, 7, 64, 300, 1000)


def batch_offsets(v=M):
    """``off`` [B + 1] over ``v`` nodes with graph sizes cycling through BATCH_SIZES (the last graph takes the
    rest): graph boundaries straddle every mark.  The [B, F] side of a readout / GraphNorm stays near."""
    sizes, tot, i = [], 0, 0
    while tot < v:
        n = min(BATCH_SIZES[i % len(BATCH_SIZES)], v - tot)
        sizes.append(n)
        tot += n
        i += 1
    return torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0), sizes
