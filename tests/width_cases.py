"""TEST INFRASTRUCTURE: the census of the kernels' width classes (tests/test_width_classes_cpu.py).

Every kernel family picks a template instantiation from the row width — lanes per row, vectors per lane,
vector width.  This module restates each dispatcher's arithmetic in Python, one small function per C++
function (cited in its docstring), and owns the width lists the GPU tests parametrise over (or re-exports them
from tests/exact_cases.py and tests/activation_cases.py), so the census and the GPU tests read the same
objects: an instantiation no list reaches fails the census by name.  A kernel with a new width class is
registered here: add the class to its function, and a width that reaches it to the family's lists.

A case is (width, aligned): ``aligned`` False is a call whose rows are not 16-B aligned (an odd leading
dimension, a column slice), which sends an H % 4 == 0 row to the scalar kernels.  Nothing here touches the
GPU."""
import activation_cases as ac
import exact_cases as xc

# ----------------------------------------------------------------------------- the lists of the GPU tests
EDGE_H, EDGE_H_SCALAR, EDGE_H_UNALIGNED = xc.EDGE_H, xc.EDGE_H_SCALAR, xc.EDGE_H_UNALIGNED
SIRE_H, HELPER_F = xc.SIRE_H, xc.HELPER_F
SEQ_SHAPES, MAX_SHAPES = xc.SEQ_SHAPES, xc.MAX_SHAPES
ACT_EDGE_H, ACT_EDGE_H_16BIT = ac.EDGE_H, ac.EDGE_H_16BIT

# tests/test_gpu_parity.py
HIDDEN_SIZES = [1, 3, 7, 16, 60, 64, 100, 128, 256, 260, 300, 512, 1000, 1024, 24, 70, 130, 516, 640, 768]
SIGN_MASK_WIDTHS = [4, 12, 32, 60, 64, 76, 80, 96, 128, 136, 256, 512, 776, 1024, 516, 640, 768]
# tests/test_econv_gpu.py
ECONV_HS = [4, 32, 80, 128, 132, 256, 300, 512, 1024, 48, 640]
# tests/test_nodenorm_gpu.py (contiguous rows; the unaligned widths go through its column-slice wrapper)
LN_M = (1, 67, 1000)
LN_N = (1, 3, 4, 60, 75, 80, 256, 300, 512, 1024, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 260, 516)
LN_SHAPES = [(M, N) for M in LN_M for N in LN_N]
LN_UNALIGNED_N = (64, 128, 256, 512, 1024)
# tests/test_stackdrop_gpu.py (the fused / dropout LayerNorm)
STACKDROP_LN_SHAPES = [(3, 1), (130, 75), (67, 256), (5, 1024),
                       (67, 129), (3, 255), (67, 257), (5, 511), (3, 513), (67, 1023), (5, 300)]
# tests/test_labelprop_gpu.py
LP_F = [1, 3, 4, 40, 47, 64, 65, 256, 260, 300, 6, 8, 12, 24, 30, 32, 100, 128, 10]
LP_F_SPLIT = [3, 40, 260, 6, 8, 12, 24, 30, 32, 100, 128, 10, 47]
# tests/test_edgemlp_gpu.py, tests/test_amp_gpu.py: (H, F) of the Sequential sigma, (H, O) of the max form
SEQ_PARITY_SHAPES = [(64, 64), (32, 48), (16, 16), (200, 200), (128, 96), (100, 140), (256, 256),
                     (32, 100), (200, 128), (248, 64)]
MAX_PARITY_SHAPES = [(256, 40), (64, 64), (300, 24), (128, 256), (100, 200), (512, 512),
                     (32, 100), (64, 300), (200, 300), (248, 64)]
MAX_ROUTED_SHAPES = [(256, 256), (256, 40), (64, 64), (300, 24), (128, 256), (100, 200), (512, 256), (4, 1),
                     (32, 100), (200, 128)]
MAX16_SHAPES = [(256, 256, "leaky"), (256, 40, "relu"), (512, 512, "leaky"), (64, 48, "relu"), (128, 200, "leaky"),
                (256, 256, "identity"), (64, 48, "identity"), (256, 256, "gelu_tanh"),
                (32, 100, "relu"), (64, 300, "leaky"), (300, 24, "relu")]

MAX_H = 1024            # the widest row any family takes


# ----------------------------------------------------------------------------- the dispatchers, restated
def edge_class(H, aligned=True):
    """sirconv_dispatch.hip: pick_shape — ("edge", vw, lanes per row, vectors per lane), None when refused.
    launch_edge_shape / launch_mask_shape / launch_dual_shape (sirconv_edge_impl.h) switch on exactly these."""
    if H <= 0:
        return None
    if aligned and H % 4 == 0:
        hc = H // 4
        for lpr in (4, 8, 16, 32):
            if hc <= lpr:
                return ("edge", 4, lpr, 1)
        nv = (hc + 63) // 64
        return ("edge", 4, 64, nv) if nv <= 4 else None
    nv = (H + 63) // 64
    if nv == 3:
        nv = 4
    return ("edge", 1, 64, nv) if nv <= 4 else None


def mask_words(H):
    """sir_mask_words for ReLU / LeakyReLU, as the vw = 4 shape of :func:`edge_class` fixes it: 4 nv words past
    128 columns, 2 for 32 lanes per row, 1 below; 0 where there is no sign mask."""
    c = edge_class(H) if H % 4 == 0 else None
    if c is None:
        return 0
    _, _, lpr, nv = c
    return 4 * nv if lpr == 64 else max(lpr // 16, 1)


def sire_class(H):
    """sirconv_eedge.hip: eshape (launch_shape switches on it) — ("sire", lanes per row, vectors per lane)."""
    if H <= 0 or H % 4 != 0 or H > 1024:
        return None
    hc = H // 4
    for lpr in (4, 8, 16, 32):
        if hc <= lpr:
            return ("sire", lpr, 1)
    return ("sire", 64, (hc + 63) // 64)


def generic_class(F, aligned=True):
    """sirconv_generic.hip: gshape + gdispatch — ("generic", vectors per lane, vw), shared by gather_add,
    segment_sum, edge_broadcast, segment_max and segment_max_bwd."""
    if F <= 0:
        return None
    vw = 4 if aligned and F % 4 == 0 else 1
    nv = (F // vw + 63) // 64
    if nv == 3:
        nv = 4
    return ("generic", nv, vw) if 1 <= nv <= 4 else None


def ln_class(N, aligned=True):
    """sirconv_nodenorm.hip: ln_by_nch — ("ln", vw, vectors per lane); N <= 1024 (sirgcn/norm.py)."""
    if N <= 0 or N > 1024:
        return None
    if aligned and N % 4 == 0:
        return ("ln", 4, 1 if N <= 256 else 2 if N <= 512 else 4)
    return ("ln", 1, 1 if N <= 64 else 2 if N <= 128 else 4 if N <= 256 else 8 if N <= 512 else 16)


def lp_class(F, aligned=True):
    """sirconv_labelprop.hip: lp_dispatch — ("lp", lanes per row, vw)."""
    if F <= 0:
        return None
    vw = 4 if aligned and F % 4 == 0 else 1
    cols, L = F // vw, 4
    while L < 64 and L < cols:
        L *= 2
    return ("lp", L, vw)


def mlp_ng(H):
    """sirconv_edgemlp.hip: mlp_ng — 16-column groups of a."""
    return (H + 15) // 16


def _mlp_legal(H, F, form):
    """sirgcn/edgemlp.py: seq_sigma (H, F <= 256) / max_supported (H, O <= 512)."""
    lim = 256 if form == "seq" else 512
    return H > 0 and H % 4 == 0 and H <= lim and 0 < F <= lim


def mlp_fwd_class(H, F, stream=True):
    """The fp32 forward of the per-edge Linear: sirgcn/edgemlp.py: _fwd sends H = 256, F <= 256 to the stream
    kernel (``stream``: edgemlp.STREAM), sirconv_edgemlp.hip: mlp_fwd16_nt routes the rest — the resident
    kernels k_mlp_fwd16q ("q", H == 256) and k_mlp_fwd16p ("p", NG), else the per-item
    k_mlp_fwd16<NW, TPW, C4> ("item", NW, TPW, C4)."""
    if stream and H == 256 and F <= 256:
        return ("mlp_fwd", "stream")
    ng, nt = mlp_ng(H), (F + 31) // 32
    if F <= 256 and ng == 16:
        return ("mlp_fwd", "q", H == 256)
    if F <= 256 and ng in (4, 8):
        return ("mlp_fwd", "p", ng)
    if ng * 16 <= 256:
        return ("mlp_fwd", "item") + ((1, 1, 1) if nt <= 1 else (2, 1, 1) if nt <= 2 else (4, 1, 1) if nt <= 4
                                      else (4, 2, 1) if nt <= 8 else (8, 2, 1))
    return ("mlp_fwd", "item") + ((4, 1, 2) if nt <= 4 else (4, 2, 2) if nt <= 8 else (8, 2, 2))


def mlp_st_class(H, O, stream=True):
    """The 16-bit max forward: sirgcn/edgemlp.py: _fwd_st (stream at H = 256, O <= 256), else
    sirconv_edgemlp.hip: mlp_fwd16_st — k_mlp_fwd16<NW, TPW, C4, ST>."""
    if stream and H == 256 and O <= 256:
        return ("mlp_st", "stream")
    nt = (O + 31) // 32
    if mlp_ng(H) * 16 <= 256:
        return ("mlp_st", "item") + ((4, 1, 1) if nt <= 4 else (8, 2, 1))
    return ("mlp_st", "item") + ((4, 2, 2) if nt <= 8 else (8, 2, 2))


def mlp_bwd_class(H, F):
    """sirconv_edgemlp.hip: mlp_bwd_nw (mlp_bwd_launch switches on it) — waves per block of k_mlp_bwd, the
    backward of the Sequential sigma and the fused max backward; H, F <= 256."""
    if H > 256 or F > 256:
        return None
    hp = (H + 7) // 8 * 8
    t = max((F + 31) // 32, (hp + 31) // 32)
    return ("mlp_bwd", 2 if t <= 2 else 4 if t <= 4 else 8)


def maxb_class(H, O):
    """sirconv_maxbwd.hip: run_max_bwd_sparse — the padded output width of k_maxb_route<NK> / k_maxb_dz<OP>
    (the routed and the hybrid max backward: H <= 512, O <= 256, sirgcn/edgemlp.py: max_bwd_sparse)."""
    if H % 4 or not 0 < H <= 512 or not 0 < O <= 256:
        return None
    return ("maxb", 64 if O <= 64 else 128 if O <= 128 else 256)


# ----------------------------------------------------------------------------- enumeration
def _widths(fn):
    """{class: sorted contiguous widths that reach it} and {class: sorted unaligned widths} of a one-width
    dispatcher."""
    al, un = {}, {}
    for w in range(1, MAX_H + 64):
        for aligned, d in ((True, al), (False, un)):
            c = fn(w, aligned)
            if c is not None:
                d.setdefault(c, []).append(w)
    return al, un


def all_classes(fn):
    """Every class a one-width dispatcher can return."""
    al, un = _widths(fn)
    return set(al) | set(un)


def span(fn, cls):
    """(lowest, highest) width of ``cls`` among calls on contiguous rows: the lowest has one active lane, or one
    vector, in the last slot; the highest fills every slot a contiguous row can (a scalar class takes contiguous
    rows only at H % 4 != 0; its full width needs unaligned rows: :func:`full_unaligned`)."""
    w = _widths(fn)[0][cls]
    return w[0], w[-1]


def full_unaligned(fn, cls):
    """The highest width of a scalar class, all slots full: reached through unaligned rows only."""
    return _widths(fn)[1][cls][-1]


def reached(fn, cases):
    """Classes that the (width, aligned) ``cases`` launch."""
    return {fn(w, a) for w, a in cases} - {None}


def contiguous(widths):
    return [(w, True) for w in widths]


def unaligned(widths):
    return [(w, False) for w in widths]


def sire(H, aligned=True):
    """:func:`sire_class` as a (width, aligned) dispatcher: the edge-term kernels refuse unaligned rows."""
    return sire_class(H) if aligned else None


def mlp_classes(fn, form_of_legal):
    """Every class of a two-width dispatcher over the legal (H, F) of the form ("seq" / "max")."""
    out = set()
    for H in range(4, 513, 4):
        for F in list(range(1, 40)) + list(range(40, 513, 4)):
            if _mlp_legal(H, F, form_of_legal):
                for c in fn(H, F):
                    out.add(c)
    return out - {None}


def mlp_fwd_both(H, F):
    return mlp_fwd_class(H, F, True), mlp_fwd_class(H, F, False)


def mlp_st_both(H, O):
    return mlp_st_class(H, O, True), mlp_st_class(H, O, False)


# ----------------------------------------------------------------------------- which test launches what
EDGE_LISTS = {          # test list -> its (width, aligned) cases; every list must reach every class it can
    "exact (test_exact_gpu.py::test_edge_kernels_exact, test_activations_gpu.py::test_identity_edge_kernels_exact)":
        contiguous(EDGE_H + EDGE_H_SCALAR) + unaligned(EDGE_H_UNALIGNED),
    "parity (test_gpu_parity.py::test_hidden_sizes_vs_oracle)": contiguous(HIDDEN_SIZES),
    "activations (test_activations_gpu.py::test_edge_kernels_other_activations_vs_oracle)": contiguous(ACT_EDGE_H),
}
EDGE_VEC_LISTS = {      # lists of H % 4 == 0 widths: every vw = 4 class
    "16-bit exact (test_exact_gpu.py::test_edge_kernels_exact)": EDGE_H,
    "sign mask (test_gpu_parity.py::test_sign_mask_backward_bit_identical_all_widths*)": SIGN_MASK_WIDTHS,
    "16-bit activations (test_activations_gpu.py::test_edge_kernels_other_activations_16bit_storage)":
        ACT_EDGE_H_16BIT,
}
SIRE_LISTS = {"exact (test_exact_gpu.py::test_sire_kernels_exact)": SIRE_H,
              "parity (test_econv_gpu.py)": ECONV_HS}
LN_LISTS = {"parity (test_nodenorm_gpu.py::test_layer_norm_parity, ::test_layer_norm_unaligned_rows)":
                contiguous(LN_N) + unaligned(LN_UNALIGNED_N),
            "fused / dropout (test_stackdrop_gpu.py::test_layer_norm_dropout_is_exact)":
                contiguous(N for _, N in STACKDROP_LN_SHAPES)}
LP_LISTS = {"unsplit (test_labelprop_gpu.py::test_unsplit_rows_equal_the_reference_bit_for_bit)": LP_F,
            "split (test_labelprop_gpu.py::test_split_rows_step_by_step)": LP_F_SPLIT}


def mlp_reached():
    """{family: {class: [(test, shape), ...]}} of the per-edge Linear kernels over every shape list.  The
    exact max forward runs every shape with the stream off and, at H = 256, O <= 256, on; the 16-bit forward
    likewise; the other tests leave edgemlp.STREAM on."""
    out = {"mlp_fwd": {}, "mlp_st": {}, "mlp_bwd": {}, "maxb": {}}

    def add(fam, cls, test, shape):
        if cls is not None:
            out[fam].setdefault(cls, []).append((test, shape))

    for H, F in SEQ_SHAPES:
        add("mlp_fwd", mlp_fwd_class(H, F), "exact seq", (H, F))
        add("mlp_bwd", mlp_bwd_class(H, F), "exact seq", (H, F))
    for H, F in SEQ_PARITY_SHAPES:
        add("mlp_fwd", mlp_fwd_class(H, F), "parity seq", (H, F))
        add("mlp_bwd", mlp_bwd_class(H, F), "parity seq", (H, F))
    for H, O in MAX_SHAPES:
        for s in (False, True):
            add("mlp_fwd", mlp_fwd_class(H, O, s), "exact max", (H, O))
            add("mlp_st", mlp_st_class(H, O, s), "exact max", (H, O))
        add("mlp_bwd", mlp_bwd_class(H, O), "exact max routes (fused)", (H, O))
        add("maxb", maxb_class(H, O), "exact max routes (routed, hybrid)", (H, O))
    for H, O in MAX_PARITY_SHAPES:
        add("mlp_fwd", mlp_fwd_class(H, O), "parity max", (H, O))
        add("mlp_bwd", mlp_bwd_class(H, O), "parity max (fused backward)", (H, O))
    for H, O in MAX_ROUTED_SHAPES:
        add("mlp_fwd", mlp_fwd_class(H, O), "parity max routed", (H, O))
        add("maxb", maxb_class(H, O), "parity max routed", (H, O))
    for H, O, _ in MAX16_SHAPES:
        add("mlp_st", mlp_st_class(H, O), "16-bit max forward", (H, O))
    return out


# ----------------------------------------------------------------------------- the row loops of the edge kernels
# edges per chunk of the per-item loops at 1 / 2 / 3 / 4 vectors per lane (sirconv_edge_impl.h), unrolled by two
CHUNK_EDGES = {1: 16, 2: 8, 3: 5, 4: 4}
PLAN_CHUNKS = (4, 64, 256)      # GraphPlan chunk of the exact tests: longer rows are split
