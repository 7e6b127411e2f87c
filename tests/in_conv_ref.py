"""The 6 -> 32 input convolution (csrc/spconv_in.hip: spconv_in_kernel, spconv_in_dw_kernel + spconv_in_dw_reduce_kernel)
against fp64: row counts, thinned synthetic gather tables, the weight-gradient reference, its bound and its checker.  No
device code; every function works on the device its tensors live on (tests/test_in_conv_ref_host.py runs all of it on the
CPU, tests/test_gpu_in_conv_edges.py on the GPU, tests/test_gpu_generic_fwd.py borrows ``thin``).  Built on fwd2_ref:
tables (make_table), the forward reference, bound and checker (conv, bound_of, check_conv) are used as they stand.

  forward   out[r, :] = sum_k X[nbr[k][r], 0:6] @ W[k] (+ bias) (+ residual[r, :])       W [27, 6, 32]
            check_conv(out, X, WT = W.transpose(1, 2), nbr, flip = 0, extra = 0): a row's value is ONE k-ordered chain of
            products in one lane pair -- no wave accumulators, no slabs are added to each other.
  dW        dW[k] = X[nbr[k][sel]]^T @ dY[sel],  sel = rows with a pair under offset k    dW [27, 6, 32]

Launch shapes the row counts are chosen for (CUs = compute units of the device):
  forward   4 waves per workgroup, one 32-row slice per wave and trip; workgroups = min(ceil(slices / 4), 2 CUs)
  dW        2 waves per workgroup;                                    workgroups P = min(ceil(slices / 2), 2 CUs);
            the reduce kernel's eight lane groups take the slabs p = g, g + 8, ... of the P workgroup slabs

Bound of dW (derived, not measured).  Element (k, c, o) is a sum of n_k products x dy, one per pair of offset k.  Every
product and every addition rounds to nearest with relative error at most u = 2^-24, so for ANY order of the additions
(Higham, Accuracy and Stability, (3.5)) |got - ref| <= gamma_{n_k + 1} S, S = sum |x| |dy|: n_k - 1 additions of the terms
plus the product's own rounding stay below n_k + 1 roundings per term.  The kernel adds MORE partial sums than that -- the
32 rows of a slice inside the matrix instruction, the slices a wave walks, the two waves of a workgroup through LDS, the P
workgroup slabs in eight lane groups, the eight groups -- but the any-order bound counts additions of TERMS: however the
n_k terms are bracketed, a sum of n_k non-zero terms passes through at most n_k - 1 additions that can round.  Every
other addition has an exact zero as one operand (the rows of a slice without a pair under k enter as a = 0, a wave or
workgroup without a pair contributes its zero accumulator, a lane group without a slab its zero) and x + 0 = x without
error; so the two waves, the P slabs and the eight lane groups need no extra terms.  On top, as in fwd2_ref:
  * MFMA_FACTOR = 2 for v_mfma_f32_32x32x2_f32, whose inner sum of two products the ISA does not specify (fwd2_ref's
    ASSUMPTION, reused, no new constant; the ratios recorded in tests/test_gpu_in_conv_edges.py let it be judged);
  * (n_k + 1) 2^-126 absolute for subnormal intermediates the matrix pipeline may flush.
An offset without pairs has S = 0: its 6 x 32 block must be exact zeros."""
import collections
import functools

import numpy as np
import torch

import fwd2_ref as F

IN_K, IN_C, IN_O = 27, 6, 32
SL = F.SL
CUS_MI355X = 256
DW_SLAB_FLOATS = IN_K * IN_C * IN_O          # 5184: one workgroup slab of the dW kernel

Case = collections.namedtuple("Case", "name M_out dw_wgs fwd_wgs thinned what")

# row count -> (dW workgroups, forward workgroups, what the count is for): the smallest counts that reach each branch
_SMALL = collections.OrderedDict([
    (1, (1, 1, "a partial slice of one row (31 lanes of each half idle); dW: the second wave owns no slice")),
    (31, (1, 1, "a partial slice, one row short; dW: the second wave owns no slice")),
    (32, (1, 1, "exactly one full slice; dW: the second wave owns no slice")),
    (33, (1, 1, "one row into a second slice; dW: one workgroup, both waves busy, the second with one row")),
    (64, (1, 1, "dW: P = 1 with both waves on full slices")),
    (65, (2, 1, "dW: P = 2, the second workgroup's second wave owns no slice")),
    (127, (2, 1, "forward: one workgroup's four waves, the last slice ragged")),
    (128, (2, 1, "forward: one workgroup's four waves, all full")),
    (129, (3, 2, "forward: a second workgroup for one row (three of its waves idle)")),
    (448, (7, 4, "dW: P = 7, fewer slabs than the reduce kernel's eight lane groups")),
    (512, (8, 4, "dW: P = 8, one slab per lane group")),
    (513, (9, 5, "dW: P = 9, lane group 0 adds two slabs")),
])


def capped_rows(cus, waves_per_wg):
    """rows above the grid cap of 2 CUs workgroups with a ragged last slice: 37 full slices and five rows more than
    one slice per wave, so that 38 waves walk two slices and the others one"""
    return SL * (2 * cus * waves_per_wg) + SL * 37 + 5


def cases(cus=CUS_MI355X):
    out = [Case(f"rows-{m}", m, d, f, False, what) for m, (d, f, what) in _SMALL.items()]
    m = capped_rows(cus, 2)
    out.append(Case("dw-capped", m, 2 * cus, min(cus + 10, 2 * cus), True,
                    "dW above the grid cap: waves walk two slices (prefetch of the next slice, LDS tile reused) or one; "
                    "forward: below its cap, hundreds of workgroups"))
    m = capped_rows(cus, 4)
    out.append(Case("fwd-capped", m, 2 * cus, 2 * cus, True,
                    "forward above the grid cap: waves walk two slices or one; dW: waves walk three slices or two"))
    return tuple(out)


CASES = cases()
NAMES = tuple(c.name for c in CASES)


def case(name, cus=CUS_MI355X):
    return next(c for c in cases(cus) if c.name == name)


def n_slices(M_out):
    return (M_out + SL - 1) // SL


def dw_workgroups(M_out, cus):
    """in_dw_wgs of csrc/spconv_in.hip"""
    return max(1, min((n_slices(M_out) + 1) // 2, 2 * cus))


def fwd_workgroups(M_out, cus):
    """the grid of spconv_in_launch"""
    return min((n_slices(M_out) + 3) // 4, 2 * cus)


def special_slices(M_out):
    """packed slices fwd2_ref.make_table gives a promised content: {"empty": (a), "last_k": (b) and (c), "dense": (f)}"""
    n, full = n_slices(M_out), M_out // SL
    if n < 3:
        return {}
    out = {"empty": full // 2, "last_k": (full // 2 + 1) % full}
    if n >= 4:
        out["dense"] = next(s for s in range(full) if s not in out.values())
    return out


PAIR_CAP = 500          # pairs per offset of a thinned case, at the most


def walk_slices(M_out, cus=CUS_MI355X):
    """packed slices of a capped case that must keep ALL their pairs: for the dW grid (4 CUs waves) and the forward grid
    (8 CUs waves) the first-, second- and third-trip slice of wave 0 and of wave 5, the last two slices (the last one
    ragged), and the slices of make_table's promises"""
    n = n_slices(M_out)
    keep = {n - 2, n - 1} | set(special_slices(M_out).values())
    for n_waves in (4 * cus, 8 * cus):
        for w in (0, 5):
            keep |= {w + t * n_waves for t in range(3)}
    return frozenset(s for s in keep if 0 <= s < n)


def keep_slices(M_out, cus=CUS_MI355X):
    """walk_slices and every 41st slice"""
    return walk_slices(M_out, cus) | frozenset(range(0, n_slices(M_out), 41))


def thin(table, M_out, keep, cap=None, spare=()):
    """-> Table: ``table`` with every packed 32-row slice outside ``keep`` all-empty (so that tens of thousands of rows
    keep hundreds of pairs per offset: bounds stay tight and one dropped pair stays visible).  Works on the packed layout
    table.info["packed"] and scatters back through table.order; info gains "kept" (sorted slices) and loses the row
    lists of promised slices that were not kept.  ``cap``: where an offset still has more pairs than this, the slices of
    ``spare`` (a subset of keep, taken from its upper end) lose their pairs under THAT offset, one slice at a time, until
    it has not; a spare slice keeps its other offsets, so it stays a slice with work."""
    P = np.array(table.info["packed"], dtype=np.int32, copy=True)
    K = P.shape[0]
    assert P.shape == (K, M_out)
    keep = sorted(int(s) for s in keep)
    assert all(0 <= s < n_slices(M_out) for s in keep) and set(spare) <= set(keep)
    live = np.zeros(n_slices(M_out) * SL, dtype=bool)
    for s in keep:
        live[s * SL:(s + 1) * SL] = True
    P[:, ~live[:M_out]] = -1
    if cap is not None:
        count = (P >= 0).sum(1)
        for k in range(K):
            for s in sorted(spare, reverse=True):
                if count[k] <= cap:
                    break
                cell = P[k, s * SL:(s + 1) * SL]
                if (P[:, s * SL:(s + 1) * SL] >= 0).any(1).sum() > 1:          # never a slice's last offset
                    count[k] -= int((cell >= 0).sum())
                    cell[:] = -1
    nbr = np.empty((K, M_out), dtype=np.int32)
    if table.order is None:
        nbr[:] = P
    else:
        nbr[:, table.order.astype(np.int64)] = P
    sp = special_slices(M_out)
    info = dict(table.info, packed=P, kept=keep)
    if sp.get("last_k") not in keep:
        info["last_k_rows"] = None
    return F.Table(nbr, table.order, info)


@functools.lru_cache(maxsize=None)
def table(M_out, variation, K=IN_K, keep=None, cap=None, spare=()):
    """(Table, M_in) at one of fwd2_ref.VARIATIONS, thinned to the packed slices ``keep`` (a frozenset) when given"""
    m_in, events = F.VARIATIONS[variation]
    M_in = m_in(M_out)
    tab = F.make_table(7 * M_out + K, M_in, M_out, K, events)
    return (tab if keep is None else thin(tab, M_out, keep, cap, spare)), M_in


def table_of(c, variation, cus=CUS_MI355X):
    """the table of a case: the capped cases keep keep_slices, at most PAIR_CAP pairs per offset (the every-41st slices
    that no named walk needs are the spare ones)"""
    if not c.thinned:
        return table(c.M_out, variation)
    keep = keep_slices(c.M_out, cus)
    return table(c.M_out, variation, IN_K, keep, PAIR_CAP, keep - walk_slices(c.M_out, cus))


def without_row_0(tab):
    """the table with every gather of input row 0 moved to row 1 (needs M_in >= 2): nothing may read X[0] any more"""
    nbr = np.where(tab.nbr == 0, 1, tab.nbr).astype(np.int32)
    return F.Table(nbr, tab.order, dict(tab.info, packed=F.pack(nbr, tab.order)))


POISON = (float("nan"), float("inf"), float("-inf"), float("nan"), 1e38, -1e38)


def rows_without_pairs(nbr):
    return np.flatnonzero((np.asarray(nbr) < 0).all(0))


Shape = collections.namedtuple("Shape", "K Cin Cout M_out")


def make_inputs(M_in, M_out, seed, dev="cpu", K=IN_K, Cin=IN_C, Cout=IN_O):
    """fwd2_ref.make_inputs (X as the first rows of a buffer that ends in 64 rows of NaN) plus W [K, Cin, Cout] and
    dY ~ N(0, 1) [M_out, Cout]; -> (X, W, WT, bias, residual, dY, buf)"""
    X, WT, bias, residual, buf = F.make_inputs(Shape(K, Cin, Cout, M_out), M_in, seed, dev)
    dY = torch.randn(M_out, Cout, generator=torch.Generator().manual_seed(seed + 77)).to(dev)
    return X, WT.transpose(1, 2).contiguous(), WT, bias, residual, dY, buf


# ---------------------------------------------------------------- weight gradient: reference, bound, checker

def dw_ref(X, dY, nbr):
    """(want [K, Cin, Cout], S [K, Cin, Cout], n [K]) in fp64: want[k] = X[nbr[k][sel]]^T @ dY[sel], S the same over
    absolute values, n[k] the number of pairs under offset k.  Rows of X no pair gathers are never read."""
    dev = X.device
    tab = F._tab(nbr, dY.shape[0], dev)
    K = tab.shape[0]
    want = torch.zeros(K, X.shape[1], dY.shape[1], dtype=torch.float64, device=dev)
    S = torch.zeros_like(want)
    Yd = dY.double()
    for k in range(K):
        sel = torch.nonzero(tab[k] >= 0).flatten()
        if sel.numel():
            xs, ys = X[tab[k][sel]].double(), Yd[sel]
            want[k] = xs.t() @ ys
            S[k] = xs.abs().t() @ ys.abs()
    return want, S, (tab >= 0).sum(1).double()


def dw_bound(S, n):
    n1 = (n + 1.0)[:, None, None]
    return F.MFMA_FACTOR * (n1 * F.U / (1.0 - n1 * F.U)) * S + n1 * F.TINY * (S > 0)


def _drop_pair(X, dY, nbr):
    """(offset, fp64 contribution [Cin, Cout]) of the pair of median size in the least-populated live offset (the rule
    of conv_ref.check_dw: size = max |x| max |dy| of the pair)"""
    tab = F._tab(nbr, dY.shape[0], X.device)
    cnt = (tab >= 0).sum(1)
    live = torch.nonzero(cnt > 0).flatten()
    if not live.numel():
        return None
    k = int(live[torch.argmin(cnt[live])])
    rows = torch.nonzero(tab[k] >= 0).flatten()
    size = X[tab[k][rows]].abs().amax(1).double() * dY[rows].abs().amax(1).double()
    r = int(rows[int(torch.argsort(size)[rows.numel() // 2])])
    return k, torch.outer(X[tab[k][r]].double(), dY[r].double())


def check_in_dw(got, X, dY, nbr, what, ref=None):
    """``got`` [K, Cin, Cout] against dw_ref (``ref``: its result, computed before): (1) every element finite; (2) every
    element inside dw_bound (module docstring); (3) an offset without pairs exactly zero; (4) the reference with one pair
    removed OUTSIDE the bound at some element of that pair's offset.  Returns (largest error / bound, largest
    dropped-pair difference / bound over that offset's elements -- the figure (4) rests on; a caller that reports over
    several cases takes the SMALLEST of them)."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite dW (an unwritten slab or element, or a gather of a NaN row)"
    want, S, n = dw_ref(X, dY, nbr) if ref is None else ref
    bound = dw_bound(S, n)
    err = (got.double() - want).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).flatten()))
        k, rest = divmod(i, got.shape[1] * got.shape[2])
        c, o = divmod(rest, got.shape[2])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound; worst ({k}, {c}, {o}): got "
                             f"{float(got[k, c, o]):.9g} want {float(want[k, c, o]):.9g} err {float(err[k, c, o]):.3e} "
                             f"bound {float(bound[k, c, o]):.3e} (pairs = {int(n[k])})")
    empty = torch.nonzero(n == 0).flatten()
    assert bool((got[empty] == 0).all()), f"{what}: an offset without pairs is not exactly zero"
    ratio = F._ratio(err, bound)
    drop_ratio = float("inf")
    dp = _drop_pair(X, dY, nbr)
    if dp is not None:
        k, contrib = dp
        d = (got[k].double() - (want[k] - contrib)).abs()
        drop_ratio = float((d / bound[k].clamp_min(1e-300)).max())
        assert drop_ratio > 1.0, (f"{what}: the bound would not see a dropped pair (offset {k}, {int(n[k])} pairs: "
                                  f"largest difference {float(d.max()):.3e}, {drop_ratio:.3f} of its bound)")
    return ratio, drop_ratio
