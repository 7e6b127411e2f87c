"""The fp32 forward / dIn sparse convolution (csrc/spconv2.hip, csrc/spconv2_body.h) against fp64: launch plans, synthetic
gather tables, references, bounds and checkers.  No device code; every function works on the device its tensors live on
(tests/test_fwd2_ref_host.py runs all of it on the CPU, tests/test_gpu_fwd2_plans.py on the GPU).

  out[r, :] = sum_k X[nbr[k][r], :] @ WT[flip ? K-1-k : k]^T (+ bias) (+ residual[r, :])        WT [K, Cout, Cin]

Plans.  ``plan_ref`` restates plan2() and form2() of the default build (wave target 8192, at most 4 waves per item with
offset slabs and 16 without, ring depth 2, one output block per item, weights to registers); ``MATRIX`` lists the smallest
shapes that select each plan; tests/test_fwd2_ref_host.py holds plan_ref to the library's own wsis_debug_fwd2_plan.

Tables.  ``make_table`` builds a synthetic gather table with full control over the active offsets of every slice of 32 rows
in the PACKED layout (column j of the packed table is output row order[j]); the kernel makes no geometric assumption.

Bound of the product (derived, not measured).  Every product and every addition of the kernel rounds to nearest with
relative error at most u = 2^-24, so for ANY order of the additions (Higham, Accuracy and Stability, (3.5))
    |got - ref| <= gamma_n S,   gamma_n = n u / (1 - n u),   S = sum |x| |w| + |bias| + |residual|,
with n the number of terms an element's value passes through: (active offsets of the row) x Cin products, the additions
of the NW wave accumulators through LDS and of the ZS slabs (``extra``), the bias and the residual add.  On top of that:
  * a factor 2 for the matrix instruction: v_mfma_f32_32x32x2_f32 adds two products to the accumulator, and the ISA
    does not say how that inner sum is rounded.  THE FACTOR IS AN ASSUMPTION, not a derived quantity; the largest observed
    error / bound ratio of every plan is recorded in tests/test_gpu_fwd2_plans.py so that it can be judged;
  * n 2^-126 absolute, for subnormal intermediate values the matrix pipeline may flush to zero.
An element without any term (S = 0) has bound 0: it must be an exact zero.  ``check_conv`` also proves that the bound
still discriminates: the reference with ONE pair removed (the pair of median size in the least-populated active offset,
the rule of conv_ref.check_dw) must lie outside the bound of an element of that pair's row.

Bounds of the slice partials.  The partials are compared with fp64 values of the kernel's OWN fp32 output rows
(bn_ref.slice_partials: computed in fp64, rounded once to fp32 -- one more u), so only the epilogue's rounding counts.
n <= 32 rows y_i of a slice, A = sum |y_i|, m their exact mean, M2 = sum (y_i - m)^2:
  sum   31 additions in any order: |S^ - S| <= gamma_31 A; the reference's own rounding: u |S| <= u A.
            |got - want| <= (gamma_31 + u) A                          [the issue's 32 u A, with the second-order term kept]
  mean  m^ = fl(S^ / n): |m^ - m| <= gamma_31 A / n + u |m^| <= delta,  delta = 34 u A / n   (gamma_31 + u (1 + gamma_31) < 34 u)
  M2    d_i = fl(y_i - m^), fl(d_i^2), n - 1 additions (padded rows contribute exact zeros): at most 2 + 1 + 31 = 34
        roundings per term, so Q^ = (1 + theta) sum (y_i - m^)^2 with |theta| <= gamma_34, and
        sum (y_i - m^)^2 = M2 + n (m^ - m)^2 EXACTLY, because sum (y_i - m) = 0: the error of the slice mean enters at second
        order only.  With the reference's rounding u M2:
            |got - want| <= (gamma_34 + u) M2 + (1 + gamma_34) n delta^2 <= 40 u M2 + 32 delta^2
        (36 u < 40 u; (1 + gamma_34) n delta'^2 with the delta' ~ 32.000004 u A / n actually reached is below 32 delta^2).
BatchNorm-backward partials (sum dz, sum dz xhat): x, gamma, beta come from bn_ref with its margin rule (|z| >= MARGIN at
every element, taken with the very fp32 mean / var the kernel is given), so no ReLU mask can differ between fp32 and fp64 and
no element is excluded; the values are held to the bound tests/test_gpu_bn_edges.py applies to bn_bwd_partial_kernel's
sums (whose arithmetic bn_terms restates): 1e-3 |want| + 1e-4 max(1, max |want|)."""
import collections

import numpy as np
import torch

import bn_ref

U = 2.0 ** -24
MFMA_FACTOR = 2.0            # assumption: see the module docstring
TINY = 2.0 ** -126
SL = 32


# ---------------------------------------------------------------- launch plans

Plan = collections.namedtuple("Plan", "NB NW ZS DA BD TR xcd_run")


def plan_ref(M_out, K, Cin, Cout, slab_items=96, has_table=True, M_in=0):
    """plan2() + form2() of csrc/spconv2_body.h / spconv2.hip with the default build's constants"""
    target, nw_max_slab, nw_max_noslab = 8192, 4, 16
    nblk, slices = Cout // 32, (M_out + SL - 1) // SL
    items = slices * nblk
    noslab = not (K >= 16 and items <= slab_items)
    steps = K * (Cin // 32)
    nwm = nw_max_noslab if noslab else nw_max_slab
    nw = 1
    while nw < nwm and items * nw * 2 <= target and nw * 2 <= steps and (nw < 4 or items * nw * 2 <= target // 2):
        nw *= 2
    zs = 1
    if not noslab:
        while zs < 8 and items * nw * zs * 2 <= target and zs * 2 <= K and steps // (nw * zs * 2) >= 2:
            zs *= 2
        zs = min(zs, K)
    xcd = 64 if nw == 1 and items * zs >= 8 * 64 * 8 else 0
    tr = int(bool(has_table) and M_in < (1 << 24) and nw == 1)
    return Plan(1, nw, zs, 2, 1, tr, xcd)


_PLAN_FN = []


def plan_fn():
    """the library's own host-only plan query wsis_debug_fwd2_plan (csrc/spconv2.hip; not in the ABI header), loaded as
    tests/test_item_deal.py loads wsis_debug_item_of"""
    if not _PLAN_FN:
        import ctypes
        import os
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        fn = ctypes.CDLL(os.path.join(root, "3d-wsis_amd", "libwsis_hip.so")).wsis_debug_fwd2_plan
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                       ctypes.c_void_p]
        _PLAN_FN.append(fn)
    return _PLAN_FN[0]


def plan_lib(M_out, K, Cin, Cout, has_table, M_in):
    """the Plan the launch would choose, read through wsis_debug_fwd2_plan"""
    out = np.full(7, -7, dtype=np.int32)
    assert plan_fn()(M_out, K, Cin, Cout, int(has_table), M_in, out.ctypes.data) == 0
    return Plan(*out.tolist())


Shape = collections.namedtuple("Shape", "name K Cin Cout M_out NW ZS TR xcd table")


def _s(name, K, Cin, Cout, M_out, NW, ZS=1, TR=None, xcd=0, table="synthetic"):
    return Shape(name, K, Cin, Cout, M_out, NW, ZS, int(NW == 1) if TR is None else TR, xcd, table)


# the smallest shapes that select each plan of the default build (table: "synthetic" = make_table, "null" = the dense 1x1
# product without a table, "identity" = the same product with the table [0, 1, 2, ...])
MATRIX = (
    _s("nw1-tr-xcd-k27-ragged", 27, 32, 256, 16421, 1, xcd=64),
    _s("nw1-tr-xcd-k8", 8, 32, 256, 16416, 1, xcd=64),
    _s("nw1-null-table", 1, 32, 32, 300, 1, TR=0, table="null"),
    _s("nw1-tr-identity-k1", 1, 32, 32, 300, 1, table="identity"),
    _s("nw2-k27", 27, 32, 256, 8229, 2),
    _s("nw2-k2-step-cap", 2, 32, 32, 300, 2),
    _s("nw2-k1-wave1-idle", 1, 64, 32, 300, 2),
    _s("nw4-zs1", 27, 32, 64, 16417, 4),
    _s("nw8-k27", 27, 32, 32, 8211, 8),
    _s("nw8-k8-one-offset-per-wave", 8, 32, 32, 1000, 8),
    _s("nw8-k1-seven-idle", 1, 256, 128, 300, 8),
    _s("nw16-3105", 27, 32, 32, 3105, 16),
    _s("nw16-64-64", 27, 64, 64, 3100, 16),
    _s("nw16-k8-waves-8-15-idle", 8, 64, 32, 1000, 16),
    _s("nw4-zs2-k27", 27, 32, 32, 1000, 4, 2),
    _s("nw4-zs2-k16", 16, 32, 32, 1000, 4, 2),
    _s("nw8-k15-no-slabs", 15, 32, 32, 1000, 8),
    _s("nw4-zs4", 27, 64, 32, 1000, 4, 4),
    _s("nw4-zs8-128-32", 27, 128, 32, 1000, 4, 8),
    _s("nw4-zs8-96-items", 27, 96, 96, 1000, 4, 8),
    _s("nw4-zs8-70-rows", 27, 160, 160, 70, 4, 8),
    _s("slab-edge-3072", 27, 32, 32, 3072, 4, 2),
    _s("slab-edge-3073", 27, 32, 32, 3073, 16),
    _s("rows-1", 27, 32, 32, 1, 4, 2),
    _s("rows-31", 27, 32, 32, 31, 4, 2),
    _s("rows-32", 27, 32, 32, 32, 4, 2),
    _s("rows-33", 27, 32, 32, 33, 4, 2),
)
BY_NAME = {s.name: s for s in MATRIX}

# table variations at each plan: name -> (M_in as a function of M_out, events of make_table)
VARIATIONS = collections.OrderedDict([
    ("eq", (lambda m: m, ("perm",))),
    ("gt", (lambda m: 2 * m + 5, ("perm",))),
    ("up", (lambda m: max(1, m // 3), ("perm", "up"))),          # M_in < M_out, one pair per output row
    ("one", (lambda m: 1, ("perm",))),
])


def variations(shape):
    return ("eq",) if shape.table != "synthetic" else tuple(VARIATIONS)


# ---------------------------------------------------------------- synthetic gather tables

Table = collections.namedtuple("Table", "nbr order info")


def permutation(seed, M_out):
    return np.random.default_rng(seed).permutation(M_out).astype(np.int32)


def make_table(seed, M_in, M_out, K, events=()):
    """-> Table(nbr int32 [K, M_out] with -1 for no pair, order int32 [M_out] permutation or None, info).

    ``events``: "perm" -- the tile order is a seeded permutation (otherwise None: row order); "up" -- every output row
    has exactly one pair, like the up table of a strided convolution (rows of the all-empty slice have none, the one row
    of (e) has two).  Slice s of the PACKED table nbr[:, order] is its columns 32 s .. 32 s + 31.  Every table holds, and
    the builder asserts in the packed layout:
      (a) a full slice in which no row has a pair                                   [3 slices or more]
      (b) a slice whose only active offset is K - 1 (last wave, last slab)          [3 slices or more]
      (c) pairs that gather input row 0 and input row M_in - 1
      (d) M_out % 32 != 0: a ragged last slice with at least one -1 and one pair    [K >= 2 or two rows or more in it]
      (e) the same input row gathered by several offsets of one output row          [K >= 2]
      (f) a slice with a pair under every offset of every row (the longest walk)    [4 slices or more, not "up"]
    The other slices get a random non-empty set of active offsets each (a third of the offsets on average) and, inside
    an active offset, a pair in 70 % of the rows.  ``info``: rows (original numbering) of the special slices."""
    rng = np.random.default_rng(seed)
    up = "up" in events
    n_sl = (M_out + SL - 1) // SL
    P = np.full((K, n_sl * SL), -1, dtype=np.int64)          # packed, padded to whole slices
    for s in range(n_sl):
        if up:
            P[rng.integers(0, K, SL), s * SL + np.arange(SL)] = rng.integers(0, M_in, SL)
            continue
        act = np.flatnonzero(rng.random(K) < 1.0 / 3.0)
        if not len(act):
            act = rng.integers(0, K, 1)
        for k in act:
            rows = np.flatnonzero(rng.random(SL) < 0.7)
            P[k, s * SL + rows] = rng.integers(0, M_in, len(rows))
    full = M_out // SL                                       # full slices (3 slices or more: at least two of them)
    s_empty = s_last = None
    if n_sl >= 3:
        s_empty, s_last = full // 2, (full // 2 + 1) % full
        P[:, s_empty * SL:(s_empty + 1) * SL] = -1
        P[:, s_last * SL:(s_last + 1) * SL] = -1
        P[K - 1, s_last * SL:(s_last + 1) * SL] = rng.integers(0, M_in, SL)
    s_dense = next((s for s in range(full) if s not in (s_empty, s_last)), None) if n_sl >= 4 and not up else None
    if s_dense is not None:
        P[:, s_dense * SL:(s_dense + 1) * SL] = rng.integers(0, M_in, (K, SL))
    P = P[:, :M_out]
    free = [s for s in range(n_sl) if s not in (s_empty, s_last, s_dense)]
    cols = lambda s: list(range(s * SL, min(M_out, (s + 1) * SL)))
    # (c): under offset K - 1, in slice (b) where there is one (its active set stays {K - 1}), else in the first slice
    c_cols = cols(s_last if s_last is not None else free[0])[:2]
    P[:, c_cols] = -1
    P[K - 1, c_cols[0]] = 0
    if len(c_cols) > 1:
        P[K - 1, c_cols[1]] = M_in - 1
    elif M_in > 1:
        assert K >= 2 and not up
        P[0, c_cols[0]] = M_in - 1
    # (e): one row of a free slice gathers one input row under two (up) or three offsets
    e_cols = [c for s in free for c in cols(s) if c not in c_cols]
    row_e = None
    if K >= 2 and e_cols:
        row_e = e_cols[min(len(e_cols) - 1, 2)]
        P[:, row_e] = -1
        P[[0, K - 1] if up else sorted({0, K // 2, K - 1}), row_e] = int(rng.integers(0, M_in))
    # (d): a pair and a missing pair among the rows of the ragged last slice
    ragged = bool(M_out % SL) and (K >= 2 or M_out % SL >= 2)
    unpaired = None
    if ragged:
        r_cols = [c for c in cols(n_sl - 1) if c != row_e and c not in c_cols] or cols(n_sl - 1)
        if not (P[:, cols(n_sl - 1)] >= 0).any():
            P[K - 1, r_cols[-1]] = int(rng.integers(0, M_in))
        if not (P[:, cols(n_sl - 1)] < 0).any():
            P[0, r_cols[-1]] = -1                               # (K = 1 "up": this one row is left without its pair)
            unpaired = r_cols[-1]
    # ---- the promises, in the packed layout
    sl = lambda s: P[:, s * SL:min(M_out, (s + 1) * SL)]
    if n_sl >= 3:
        assert (sl(s_empty) < 0).all() and sl(s_empty).shape[1] == SL                                       # (a)
        assert (sl(s_last)[:K - 1] < 0).all() and (sl(s_last)[K - 1] >= 0).all()                             # (b)
    assert (P == 0).any() and (P == M_in - 1).any()                                                          # (c)
    if ragged:
        assert (sl(n_sl - 1) < 0).any() and (sl(n_sl - 1) >= 0).any()                                        # (d)
    assert s_dense is None or (sl(s_dense) >= 0).all()                                                       # (f)
    assert (s_dense is not None) == (n_sl >= 4 and not up)
    if row_e is not None:
        v = P[:, row_e]
        assert (v >= 0).sum() >= 2 and len(set(v[v >= 0].tolist())) == 1                                     # (e)
    else:
        assert K < 2 or M_out < 3, "(e) needs two offsets and a row besides those of (c)"
    if up:
        n_pairs = (P >= 0).sum(0)
        other = np.ones(M_out, dtype=bool)
        if s_empty is not None:
            other[s_empty * SL:(s_empty + 1) * SL] = False
        for c in (row_e, unpaired):
            if c is not None:
                other[c] = False
        assert (n_pairs[other] == 1).all() and (M_in >= M_out or (P < M_in).all())
    order = permutation(seed + 1, M_out) if "perm" in events else None
    nbr = np.empty((K, M_out), dtype=np.int32)
    if order is None:
        nbr[:] = P
    else:
        nbr[:, order.astype(np.int64)] = P                      # rulebook_ref.pack_ref(nbr, order) == P
    rows_of = lambda s: None if s is None else (np.arange(s * SL, (s + 1) * SL) if order is None
                                                 else order[s * SL:(s + 1) * SL].astype(np.int64))
    info = {"empty_rows": rows_of(s_empty), "last_k_rows": rows_of(s_last), "packed": P.astype(np.int32)}
    return Table(nbr, order, info)


def identity_table(M):
    return Table(np.arange(M, dtype=np.int32)[None, :].copy(), None, {"empty_rows": None, "last_k_rows": None})


def table_for(shape, variation="eq", seed=0):
    """(Table or None for the null table, M_in) of a MATRIX shape under one of VARIATIONS"""
    if shape.table == "null":
        return None, shape.M_out
    if shape.table == "identity":
        return identity_table(shape.M_out), shape.M_out
    m_in, events = VARIATIONS[variation]
    M_in = m_in(shape.M_out)
    return make_table(1000 * seed + 7 * shape.M_out + shape.K, M_in, shape.M_out, shape.K, events), M_in


def pack(nbr, order):
    """the packed table the kernels read (rulebook_ref.pack_ref)"""
    return nbr if order is None else np.ascontiguousarray(np.asarray(nbr)[:, np.asarray(order, dtype=np.int64)])


# ---------------------------------------------------------------- references

def _tab(nbr, M_out, dev):
    """gather table as a long tensor [K, M_out] on ``dev`` (None: the dense 1x1 product, row r gathers row r)"""
    if nbr is None:
        return torch.arange(M_out, device=dev)[None, :]
    return torch.as_tensor(np.asarray(nbr) if not torch.is_tensor(nbr) else nbr, device=dev).long()


def conv(X, WT, nbr, flip=0, bias=None, residual=None, M_out=None, ks=None, abs_=False):
    """fp64 [M_out, Cout]: sum_k X[nbr[k][r]] @ WT[flip ? K-1-k : k]^T (+ bias) (+ residual); ``ks``: only these offsets;
    ``abs_``: the same sum over absolute values (the S of the bound)"""
    dev = X.device
    K, Cout, _ = WT.shape
    M_out = int(M_out if M_out is not None else np.asarray(nbr).shape[1] if not torch.is_tensor(nbr) else nbr.shape[1])
    tab = _tab(nbr, M_out, dev)
    assert tab.shape == (K, M_out)
    Xd, Wd = X.double(), WT.double()
    if abs_:
        Xd, Wd = Xd.abs(), Wd.abs()
    out = torch.zeros(M_out, Cout, dtype=torch.float64, device=dev)
    for k in (range(K) if ks is None else ks):
        g = tab[k]
        ok = torch.nonzero(g >= 0).flatten()
        if ok.numel():
            out.index_add_(0, ok, Xd[g[ok]] @ Wd[K - 1 - k if flip else k].t())
    if bias is not None:
        out += bias.double().abs() if abs_ else bias.double()
    if residual is not None:
        out += residual.double().abs() if abs_ else residual.double()
    return out


def conv_abs(X, WT, nbr, flip=0, bias=None, residual=None, M_out=None, extra=0):
    """(S [M_out, Cout] fp64, n [M_out, 1] fp64): the sum over absolute values and the number of additions per element --
    active offsets of the row x Cin, ``extra`` (the NW wave accumulators and ZS slabs added to each other), bias, residual"""
    S = conv(X, WT, nbr, flip, bias, residual, M_out, abs_=True)
    tab = _tab(nbr, S.shape[0], X.device)
    n = (tab >= 0).sum(0).double() * WT.shape[2] + extra + (bias is not None) + (residual is not None)
    return S, n[:, None]


def bound_of(S, n):
    return MFMA_FACTOR * (n * U / (1.0 - n * U)) * S + n * TINY * (S > 0)


def _drop_pair(X, WT, nbr, flip, M_out):
    """(row, fp64 contribution [Cout]) of the pair of median size in the least-populated active offset"""
    tab = _tab(nbr, M_out, X.device)
    K = WT.shape[0]
    cnt = (tab >= 0).sum(1)
    live = torch.nonzero(cnt > 0).flatten()
    if not live.numel():
        return None
    k = int(live[torch.argmin(cnt[live])])
    rows = torch.nonzero(tab[k] >= 0).flatten()
    size = X[tab[k][rows]].abs().amax(1)
    j = int(torch.argsort(size)[rows.numel() // 2])
    r = int(rows[j])
    return r, X[tab[k][r]].double() @ WT[K - 1 - k if flip else k].double().t()


Ratios = collections.namedtuple("Ratios", "all pairs drop")


def check_conv(got, X, WT, nbr, flip=0, bias=None, residual=None, extra=0, what="", want=None, drop=True):
    """every element of ``got`` finite and inside the bound of the module docstring around the fp64 reference (``want``:
    a reference from elsewhere, e.g. oracle pair lists), and the reference without one pair OUTSIDE it at an element of
    that pair's row.  Returns Ratios(all: largest error / bound over every element -- the elements with a handful of terms,
    bias + residual alone, come closest to their bound: one rounding of 2 gamma_4; pairs: the same over the rows that have
    pairs, the figure that tests the assumption about the matrix instruction; drop: the largest dropped-pair difference /
    bound in that pair's row)."""
    M_out = got.shape[0]
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (an unwritten element, or a gather past the end of X)"
    if want is None:
        want = conv(X, WT, nbr, flip, bias, residual, M_out)
    S, n = conv_abs(X, WT, nbr, flip, bias, residual, M_out, extra)
    bound = bound_of(S, n)
    err = (got.double() - want).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).flatten()))
        r, c = divmod(i, got.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound; worst ({r}, {c}): got "
                             f"{float(got[r, c]):.9g} want {float(want[r, c]):.9g} err {float(err[r, c]):.3e} bound "
                             f"{float(bound[r, c]):.3e} (n = {int(n[r, 0])})")
    ratio = _ratio(err, bound)
    with_pairs = torch.nonzero(n[:, 0] >= WT.shape[2]).flatten()
    ratio_pairs = _ratio(err[with_pairs], bound[with_pairs]) if with_pairs.numel() else 0.0
    drop_ratio = float("inf")
    dp = _drop_pair(X, WT, nbr, flip, M_out) if drop else None
    if dp is not None:
        r, contrib = dp
        d = (got[r].double() - (want[r] - contrib)).abs()
        drop_ratio = float((d / bound[r].clamp_min(1e-300)).max())
        assert drop_ratio > 1.0, (f"{what}: the bound would not see a dropped pair (row {r}: largest difference "
                                  f"{float(d.max()):.3e}, {drop_ratio:.3f} of its bound)")
    return Ratios(ratio, ratio_pairs, drop_ratio)


# ---------------------------------------------------------------- slice partials

def slice_rows(order, M_out, zs):
    """row of every position of the slices the partials are taken over: tile order for the in-kernel epilogue (no slabs),
    row order for the slab reduce"""
    if zs > 1 or order is None:
        return torch.arange(M_out)
    return torch.as_tensor(np.asarray(order) if not torch.is_tensor(order) else order.cpu()).long()


def _fail(what, name, err, bound):
    i = int(torch.argmax((err - bound).flatten()))
    s, c = divmod(i, err.shape[1])
    raise AssertionError(f"{what}: {name} of slice {s}, channel {c}: error {float(err[s, c]):.3e} > bound "
                         f"{float(bound[s, c]):.3e}")


def _ratio(err, bound):
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def check_stats(stats, y, order, zs, what=""):
    """the [n_part, 2, C] statistics partials (sum, centred sum of squares per slice) against bn_ref.slice_partials of the
    kernel's own output ``y`` [M_out, C] taken in the order of that path.  Returns (ratio of the sums, of the squares)."""
    M_out = y.shape[0]
    st = stats.detach().cpu().double()
    assert bool(torch.isfinite(st).all()), f"{what}: a statistics partial was not written (NaN left in the buffer)"
    rows = slice_rows(order, M_out, zs)
    yo = y.detach().cpu()[rows]
    want = bn_ref.slice_partials(yo).double()
    assert st.shape == want.shape, (what, st.shape, want.shape)
    blocks, cnt = bn_ref._slices(yo.double())
    A = blocks.abs().sum(1)
    g31, g34 = 31 * U / (1 - 31 * U), 34 * U / (1 - 34 * U)
    b_sum = (g31 + U) * A
    exact_m2 = _exact_m2(blocks, cnt, M_out)
    delta = 34 * U * A / cnt[:, None]
    b_sq = 40 * U * exact_m2 + 32 * delta * delta
    assert g34 + U <= 40 * U and g31 + U * (1 + g31) <= 34 * U          # the derivation's constants
    e_sum, e_sq = (st[:, 0] - want[:, 0]).abs(), (st[:, 1] - want[:, 1]).abs()
    if bool((e_sum > b_sum).any()):
        _fail(what, "sum", e_sum, b_sum)
    if bool((e_sq > b_sq).any()):
        _fail(what, "centred sum of squares", e_sq, b_sq)
    return _ratio(e_sum, b_sum), _ratio(e_sq, b_sq)


def _exact_m2(blocks, cnt, M_out):
    live = (torch.arange(blocks.shape[0] * SL) < M_out).view(-1, SL, 1)
    mean = blocks.sum(1) / cnt[:, None]
    dev = torch.where(live, blocks - mean[:, None, :], torch.zeros_like(blocks))
    return (dev * dev).sum(1)


BnCase = collections.namedtuple("BnCase", "x mean var gamma beta eps")


def bn_case(M, C, seed):
    """input of the BatchNorm behind a dIn product: bn_ref.offset(ratio 3) with the ReLU margin taken with the fp32
    mean / var the kernel is handed (batch statistics of the first draw, rounded to fp32)"""
    first = bn_ref.offset(M, C, 3, seed)
    mean, var, _ = bn_ref.stats(first.x)
    mean, var = mean.float(), var.float().clamp_min(1e-3)
    c = bn_ref.offset(M, C, 3, seed, stats_given=(mean.double(), var.double()))
    return BnCase(c.x, mean, var, c.gamma, c.beta, bn_ref.EPS)


def check_bn_partials(part, y, bn, relu, order, zs, what=""):
    """the [n_part, 2, C] BatchNorm-backward partials (sum dz, sum dz xhat per slice) against bn_ref.bwd_slice_partials of
    the kernel's own dIn rows ``y``; bound: module docstring.  Returns the largest error / bound."""
    M_out = y.shape[0]
    pt = part.detach().cpu().double()
    assert bool(torch.isfinite(pt).all()), f"{what}: a partial was not written (NaN left in the buffer)"
    rows = slice_rows(order, M_out, zs)
    want = bn_ref.bwd_slice_partials(bn.x[rows], y.detach().cpu()[rows], bn.mean, bn.var, bn.gamma, bn.beta, bn.eps,
                                     relu).double()
    assert pt.shape == want.shape, (what, pt.shape, want.shape)
    worst = 0.0
    for j, name in ((0, "sum dz"), (1, "sum dz xhat")):
        w = want[:, j]
        bound = 1e-3 * w.abs() + 1e-4 * max(1.0, float(w.abs().max()))
        err = (pt[:, j] - w).abs()
        if bool((err > bound).any()):
            _fail(what, name, err, bound)
        worst = max(worst, _ratio(err, bound))
    return worst


# ---------------------------------------------------------------- inputs

def make_inputs(shape, M_in, seed, dev="cpu"):
    """X ~ N(0, 1) as the first M_in rows of a buffer with 64 rows of NaN behind them (a gather past the descriptor bound
    poisons the result), WT ~ 0.05 N(0, 1) [K, Cout, Cin], bias ~ 0.1 N(0, 1) + 0.5, residual ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M_in + 64, shape.Cin), float("nan"))
    buf[:M_in] = torch.randn(M_in, shape.Cin, generator=g)
    WT = torch.randn(shape.K, shape.Cout, shape.Cin, generator=g) * 0.05
    bias = torch.randn(shape.Cout, generator=g) * 0.1 + 0.5
    residual = torch.randn(shape.M_out, shape.Cout, generator=g)
    buf = buf.to(dev)
    return buf[:M_in], WT.to(dev), bias.to(dev), residual.to(dev), buf
