"""Parameter lists for the L1 / L2 penalty tests (sirgcn.param_norms, sir_param_norms_fwd / _bwd).

A list is a sequence of specs ``(numel, offset, frozen)``: ``offset`` is the distance in floats of the tensor's
first element from a 16-byte aligned base (0: an ordinary tensor; 1, 2, 3: a view that is only 4-byte aligned),
``frozen`` a parameter without a gradient.  Sizes are expressed in the library's chunk ``CH``, its tensors per
launch ``TM`` and the threads of its combine block ``CT``, all asked from the library, never restated.

Values: "quarter" = k / 4 with |k| <= 4 for lists of at most 2^19 elements (|p| and p^2 are multiples of 1/16 and
both sums stay below 2^20: every partial sum in every order is exact in fp32), "unit" = {-1, 0, 1} for longer
lists (sums below 2^24).  The fp64 sums of a list are computed once per (list, kind of values) and shared.
"""
import functools

import torch

from sirgcn import _native

EXACT_MAX = 1 << 19


@functools.lru_cache(maxsize=None)
def consts():
    lib = _native.load()
    return (int(lib.sir_param_norms_chunk()), int(lib.sir_param_norms_max_tensors()),
            int(lib.sir_param_norms_combine_threads()))


def tensor_sizes():
    CH = consts()[0]
    return [0, 1, 2, 3, 4, 5, 7, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 3]


def list_lengths():
    TM = consts()[1]
    return [1, TM - 1, TM, TM + 1, 2 * TM + 1]


def view_specs():
    CH = consts()[0]
    return [(n, off, False) for off in (1, 2, 3) for n in (1, 3, 6, CH + 5)]


def large_numel():
    """One tensor with more chunks than the combine block has threads, below 2^24 elements."""
    CH, _, CT = consts()
    n = (CT + 3) * CH + 5
    assert n < (1 << 24)
    return n


def lists():
    """name -> specs, every list of the issue."""
    out = {}
    for n in tensor_sizes():
        out[f"size{n}"] = [(n, 0, False)]
    out["sizes"] = [(n, 0, False) for n in tensor_sizes()]
    for L in list_lengths():
        out[f"len{L}"] = [(1 + i % 9, 0, False) for i in range(L)]
    for n, off, _ in view_specs():
        out[f"view{off}_{n}"] = [(n, off, False)]
    out["views"] = view_specs()
    out["large"] = [(large_numel(), 0, False)]
    TM = consts()[1]
    tiny = [(1 + i % 9, i % 4, False) for i in range(TM + 1)]
    sizes = [(n, 0, False) for n in tensor_sizes()]
    out["mixed"] = (sizes[:7] + view_specs()[:6] + tiny[:TM // 2] + [(large_numel(), 0, False)]
                    + [(consts()[0] + 7, 2, True)] + tiny[TM // 2:] + view_specs()[6:] + sizes[7:])
    return out


LIST_NAMES = None


def list_names():
    global LIST_NAMES
    if LIST_NAMES is None:
        LIST_NAMES = list(lists())
    return LIST_NAMES


def total(specs):
    return sum(n for n, _, _ in specs)


@functools.lru_cache(maxsize=None)
def values(name, kind):
    """The list's values as CPU fp32 1-D tensors (read-only by convention) and the fp64 sums (l1, l2).
    kind: "exact" (quarter / unit values) or "normal" (N(0, 1))."""
    specs = lists()[name]
    gen = torch.Generator().manual_seed(1234 + list_names().index(name))
    vals = []
    for n, _, _ in specs:
        if kind == "normal":
            v = torch.randn(n, generator=gen)
        elif total(specs) <= EXACT_MAX:
            v = torch.randint(-4, 5, (n,), generator=gen).float() / 4
        else:
            v = torch.randint(-1, 2, (n,), generator=gen).float()
        vals.append(v)
    l1 = sum(float(v.double().abs().sum()) for v in vals)
    l2 = sum(float(v.double().pow(2).sum()) for v in vals)
    return vals, (l1, l2)


def materialise(specs, vals, device, poison=float("nan")):
    """The list on ``device``: every tensor a leaf view [offset, offset + numel) of its own 16-byte aligned
    base whose other elements hold ``poison``; frozen tensors do not require a gradient.  Returns
    (tensors, bases)."""
    tensors, bases = [], []
    for (n, off, frozen), v in zip(specs, vals):
        base = torch.full((off + n + 5,), poison, device=device, dtype=torch.float32)
        assert base.data_ptr() % 16 == 0
        t = base[off:off + n]
        t.copy_(v)
        t = t.detach().requires_grad_(not frozen)
        assert n == 0 or t.data_ptr() == base.data_ptr() + 4 * off
        tensors.append(t)
        bases.append(base)
    return tensors, bases


def composition(params):
    """The reference's two sums from torch ops, written from the formula: per-tensor sums, stacked, summed."""
    dev = params[0].device
    l1 = torch.stack([p.abs().sum().to(dev) for p in params]).sum()
    l2 = torch.stack([p.pow(2).sum().to(dev) for p in params]).sum()
    return l1, l2


def chunks_brute(numels, CH):
    """Chunk count restated by walking every tensor in CH-element steps."""
    c = 0
    for n in numels:
        i = 0
        while i < n:
            c += 1
            i += CH
    return c


def slots_brute(numels, needs):
    """Slot offsets restated float by float: a slot starts at the next multiple of 4 floats."""
    offs, pos = [], 0
    for n, need in zip(numels, needs):
        if not need:
            offs.append(None)
            continue
        while pos % 4:
            pos += 1
        offs.append(pos)
        pos += n
    while pos % 4:
        pos += 1
    return offs, pos
