"""The census of the width classes (tests/width_cases.py): every template instantiation a dispatcher can pick
from the row width is launched by the GPU tests — by every list that is meant to sweep the family, and for the
edge, SIREConv, edge-materialised and LayerNorm kernels at the lowest width of the class (one active lane, or
one vector, in the last slot) and at the highest (all full).  The restatement of ``pick_shape`` is tied to the
built library through ``sir_mask_words``; graph C of tests/exact_cases.py is held to the row lengths the
kernels' chunk loops need.  A kernel with a new width class fails here until a width that reaches it is listed.

This is a statement about the dispatch arithmetic; no compiled kernel is inspected."""
import pytest
import torch

import exact_cases as xc
import width_cases as wc

from sirgcn import _native


def _missing(want, got, what):
    lost = sorted(want - got)
    assert not lost, f"{what}: no width reaches the class(es) {lost}"


# ----------------------------------------------------------------------------- the classes themselves
def test_the_dispatchers_return_the_classes_the_kernels_are_built_for():
    """What the enumeration finds is what the launchers switch on — a class added to a dispatcher shows up here."""
    assert wc.all_classes(wc.edge_class) == (
        {("edge", 4, lpr, 1) for lpr in (4, 8, 16, 32)} | {("edge", 4, 64, nv) for nv in (1, 2, 3, 4)}
        | {("edge", 1, 64, nv) for nv in (1, 2, 4)})
    assert wc.all_classes(wc.sire) == (
        {("sire", lpr, 1) for lpr in (4, 8, 16, 32)} | {("sire", 64, nv) for nv in (1, 2, 3, 4)})
    assert wc.all_classes(wc.generic_class) == {("generic", nv, vw) for nv in (1, 2, 4) for vw in (1, 4)}
    assert wc.all_classes(wc.ln_class) == (
        {("ln", 4, n) for n in (1, 2, 4)} | {("ln", 1, n) for n in (1, 2, 4, 8, 16)})
    assert wc.all_classes(wc.lp_class) == {("lp", L, vw) for L in (4, 8, 16, 32, 64) for vw in (1, 4)}
    item = lambda *s: [("mlp_fwd", "item") + t for t in s]
    assert wc.mlp_classes(wc.mlp_fwd_both, "max") == set(
        item((1, 1, 1), (2, 1, 1), (4, 1, 1), (4, 2, 1), (8, 2, 1), (4, 1, 2), (4, 2, 2), (8, 2, 2))
        + [("mlp_fwd", "stream"), ("mlp_fwd", "q", True), ("mlp_fwd", "q", False), ("mlp_fwd", "p", 4),
           ("mlp_fwd", "p", 8)])
    assert wc.mlp_classes(wc.mlp_st_both, "max") == (
        {("mlp_st", "item") + t for t in ((4, 1, 1), (8, 2, 1), (4, 2, 2), (8, 2, 2))} | {("mlp_st", "stream")})
    assert wc.mlp_classes(lambda H, F: (wc.mlp_bwd_class(H, F),), "seq") == {("mlp_bwd", n) for n in (2, 4, 8)}
    assert wc.mlp_classes(lambda H, O: (wc.maxb_class(H, O),), "max") == {("maxb", o) for o in (64, 128, 256)}


def test_scalar_widths_129_to_192_take_four_values_per_lane():
    """pick_shape and gshape compute nv = 3 there and remap it to 4: no scalar nv = 3 kernel exists."""
    for w in (129, 160, 191, 192):
        assert wc.edge_class(w, False) == ("edge", 1, 64, 4)
        assert wc.generic_class(w, False) == ("generic", 4, 1)
    assert wc.generic_class(516) == wc.generic_class(768) == ("generic", 4, 4)      # float4 nv = 3 -> 4
    assert wc.edge_class(516) == wc.edge_class(768) == ("edge", 4, 64, 3)           # the edge kernels have NV = 3


def test_mask_words_of_the_library_follow_pick_shape():
    """sir_mask_words(H, ReLU) for every H in 4..1024 step 4 is 4 nv past 128 columns, 2 for 68..128, 1 below;
    0 for H % 4 != 0 and for H > 1024 — the library agrees with the Python restatement of pick_shape."""
    _native.load()
    for H in range(4, 1025, 4):
        want = 4 * ((H // 4 + 63) // 64) if H > 128 else 2 if H >= 68 else 1
        assert wc.mask_words(H) == want, H
        for act in (_native.ACT_RELU, _native.ACT_LEAKY):
            assert _native.mask_words(H, act) == want, (H, act)
    for H in list(range(1, 260, 4)) + [2, 3, 6, 7, 1023, 1025, 1028, 1032, 2048]:
        if H % 4 != 0 or H > 1024:
            assert wc.mask_words(H) == 0 and _native.mask_words(H, _native.ACT_RELU) == 0, H


# ----------------------------------------------------------------------------- reached by the lists
def _spans(fn, cases, what, full=(), interior=False):
    """Every class at its lowest and its highest contiguous width (``interior``: and at a width in between, the
    last slot partly filled), the scalar classes also at their full width through unaligned rows when the
    family has such a test (``full``: its widths)."""
    widths = {w for w, a in cases if a}
    for cls in sorted(wc.all_classes(fn)):
        lo, hi = wc.span(fn, cls)
        assert lo in widths, f"{what}: {cls} is not reached at its lowest width {lo}"
        assert hi in widths, f"{what}: {cls} is not reached at its highest width {hi}"
        if interior:
            assert any(lo < w < hi and fn(w, True) == cls for w in widths), \
                f"{what}: {cls} is not reached at a width between {lo} and {hi}"
        if full and cls[1 if cls[0] != "generic" else 2] == 1:
            top = wc.full_unaligned(fn, cls)
            assert top in full, f"{what}: {cls} is not reached at its full width {top} through unaligned rows"


@pytest.mark.parametrize("name", list(wc.EDGE_LISTS))
def test_edge_lists_reach_every_class(name):
    _missing(wc.all_classes(wc.edge_class), wc.reached(wc.edge_class, wc.EDGE_LISTS[name]), name)


@pytest.mark.parametrize("name", list(wc.EDGE_VEC_LISTS))
def test_edge_lists_of_vector_widths_reach_every_vector_class(name):
    want = {c for c in wc.all_classes(wc.edge_class) if c[1] == 4}
    assert all(H % 4 == 0 for H in wc.EDGE_VEC_LISTS[name])
    _missing(want, wc.reached(wc.edge_class, wc.contiguous(wc.EDGE_VEC_LISTS[name])), name)


def test_exact_edge_widths_sit_on_the_class_edges():
    name = next(iter(wc.EDGE_LISTS))
    _spans(wc.edge_class, wc.EDGE_LISTS[name], name, full=wc.EDGE_H_UNALIGNED, interior=True)
    # the 16-bit kernels see every vw = 4 edge too: the same list without the scalar widths
    _spans(lambda w, a: wc.edge_class(w, a) if a and w % 4 == 0 else None, wc.contiguous(wc.EDGE_H), "16-bit exact",
           interior=True)


@pytest.mark.parametrize("name", list(wc.SIRE_LISTS))
def test_sire_lists_reach_every_class(name):
    _missing(wc.all_classes(wc.sire), wc.reached(wc.sire, wc.contiguous(wc.SIRE_LISTS[name])), name)


def test_exact_sire_widths_sit_on_the_class_edges():
    _spans(wc.sire, wc.contiguous(wc.SIRE_H), "exact SIREConv (xc.SIRE_H)", interior=True)


def test_helper_widths_reach_every_class_on_its_edges():
    what = "edge-materialised helpers (test_exact_gpu.py::test_edge_materialised_helpers_exact)"
    cases = wc.contiguous(wc.HELPER_F)
    _missing(wc.all_classes(wc.generic_class), wc.reached(wc.generic_class, cases), what)
    _spans(wc.generic_class, cases, what)


@pytest.mark.parametrize("name", list(wc.LN_LISTS))
def test_layer_norm_lists_reach_every_class(name):
    _missing(wc.all_classes(wc.ln_class), wc.reached(wc.ln_class, wc.LN_LISTS[name]), name)


def test_layer_norm_parity_widths_sit_on_the_class_edges():
    name = next(iter(wc.LN_LISTS))
    _spans(wc.ln_class, wc.LN_LISTS[name], name, full=wc.LN_UNALIGNED_N)


@pytest.mark.parametrize("name", list(wc.LP_LISTS))
def test_label_propagation_lists_reach_every_class(name):
    _missing(wc.all_classes(wc.lp_class), wc.reached(wc.lp_class, wc.contiguous(wc.LP_LISTS[name])), name)


def test_per_edge_linear_shapes_reach_every_class():
    got = wc.mlp_reached()
    _missing(wc.mlp_classes(wc.mlp_fwd_both, "max"), set(got["mlp_fwd"]), "per-edge Linear forward (fp32)")
    _missing(wc.mlp_classes(wc.mlp_st_both, "max"), set(got["mlp_st"]), "per-edge Linear forward (16-bit max)")
    _missing({("mlp_bwd", n) for n in (2, 4, 8)}, set(got["mlp_bwd"]), "per-edge Linear backward (k_mlp_bwd)")
    _missing({("maxb", o) for o in (64, 128, 256)}, set(got["maxb"]), "routed max backward")
    # the per-item kernels the exact lists did not reach before, now with an exact test each
    exact = {c for fam in got.values() for c, tests in fam.items() if any(t.startswith("exact") for t, _ in tests)}
    for cls in (("mlp_fwd", "item", 4, 1, 1), ("mlp_fwd", "item", 8, 2, 1), ("mlp_bwd", 4), ("maxb", 128)):
        assert cls in exact, f"{cls} has no exact test"


def test_every_shape_of_the_per_edge_linear_lists_is_legal():
    for H, F in list(wc.SEQ_SHAPES) + wc.SEQ_PARITY_SHAPES:
        assert wc._mlp_legal(H, F, "seq"), (H, F)
    for H, O in list(wc.MAX_SHAPES) + wc.MAX_PARITY_SHAPES + wc.MAX_ROUTED_SHAPES + [s[:2] for s in wc.MAX16_SHAPES]:
        assert wc._mlp_legal(H, O, "max"), (H, O)
    assert all(wc.maxb_class(H, O) is not None for H, O in wc.MAX_ROUTED_SHAPES)


def test_a_removed_width_is_noticed():
    """The census is a real condition: without its NV = 3 widths a list fails, and the failure names the class."""
    cases = [c for c in next(iter(wc.EDGE_LISTS.values())) if not 516 <= c[0] <= 768]
    with pytest.raises(AssertionError, match=r"\('edge', 4, 64, 3\)"):
        _missing(wc.all_classes(wc.edge_class), wc.reached(wc.edge_class, cases), "without 516..768")
    with pytest.raises(AssertionError, match=r"\('edge', 4, 64, 3\) is not reached at its lowest width 516"):
        _spans(wc.edge_class, [c for c in next(iter(wc.EDGE_LISTS.values())) if c[0] != 516], "without 516")
    exact = next(iter(wc.EDGE_LISTS.values()))
    for gone, where in ((640, "at a width between 516 and 768"), (768, "at its highest width 768")):
        with pytest.raises(AssertionError, match=rf"\('edge', 4, 64, 3\) is not reached {where}"):
            _spans(wc.edge_class, [c for c in exact if c[0] != gone], f"without {gone}", interior=True)
        with pytest.raises(AssertionError, match=rf"\('sire', 64, 3\) is not reached {where}"):
            _spans(wc.sire, wc.contiguous(h for h in wc.SIRE_H if h != gone), f"without {gone}", interior=True)
    with pytest.raises(AssertionError, match=r"\('sire', 64, 3\)"):
        _missing(wc.all_classes(wc.sire), wc.reached(wc.sire, wc.contiguous(h for h in wc.SIRE_H if h not in
                                                                            (516, 640, 768))), "without 516..768")


# ----------------------------------------------------------------------------- graph C: the rows of the chunk loops
def test_graph_c_has_every_row_length_the_chunk_loops_distinguish():
    """The per-item loops take 16 / 8 / 5 / 4 edges per chunk (1 / 2 / 3 / 4 vectors per lane), two chunks per
    trip, and a tail of 0 .. chunk - 1 edges.  On graph C the destination pass meets every in-degree 0..65 and
    the source pass every out-degree 0..65, each once: every tail after 0, 1, 2 and 3 full chunks (an even and
    an odd trip count, twice) at every chunk length, 63 / 64 / 65 around the plan chunk 64, and at plan chunk 4
    every residue of a split row with 1..16 slots."""
    src, dst, V = xc.GRAPHS["C"]
    L = xc.LADDER_C
    ind = torch.bincount(dst, minlength=V)[:L].tolist()
    outd = torch.bincount(src, minlength=V)[L:2 * L].tolist()
    for degs in (ind, outd):
        assert sorted(degs) == list(range(66))
        have = set(degs)
        for nv, ch in wc.CHUNK_EDGES.items():
            assert ch == (64 // (4 * nv) if nv != 1 else 16)
            for full in range(4):
                for tail in range(ch):
                    assert full * ch + tail in have, (nv, full, tail)
        assert {63, 64, 65} <= have and 2 * 2 * max(wc.CHUNK_EDGES.values()) <= max(have)
        assert {(d % 4, -(-d // 4)) for d in have if d > 4} >= {(r, n) for r in range(4) for n in range(3, 17)}
    assert wc.PLAN_CHUNKS == (4, 64, 256)
    # what graphs A and B leave out: these in-degrees occur in no other exact graph
    others = set()
    for g in ("A", "B"):
        s, d, v = xc.GRAPHS[g]
        others |= set(torch.bincount(d, minlength=v).tolist())
    for d in (2, 3, 5, 15, 17, 27, 29, 39, 41, 42, 45, 56, 59, 63):
        assert d not in others and d in set(ind)
