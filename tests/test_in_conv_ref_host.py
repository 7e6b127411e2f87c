"""CPU: the cases, tables, references and checkers of tests/in_conv_ref.py (the 6 -> 32 input convolution of
csrc/spconv_in.hip against fp64) are themselves right -- the evidence, obtained without a GPU, that a subtly wrong kernel
cannot pass tests/test_gpu_in_conv_edges.py.

  * every case at every table variation: make_table's promises hold (after thinning: for the kept slices), ``thin`` keeps
    the slices named in ``keep`` and nothing else, the thinned cases have 1 .. 500 pairs under every offset;
  * an fp32 EMULATION of both products in another summation order than the kernels' (offsets descending, the products of an
    offset by an fp32 matrix product over all rows at once, no slices, no slabs) passes check_conv and check_in_dw at every
    case and variation, with the dropped pair at least 10 bounds out;
  * the same emulation with one thing wrong fails: a dropped pair, a dropped packed slice, the second half's offsets
    (k >= 14) left out, offset 26 taken twice (in place of the zero 28th offset), the rows of the ragged last slice left out
    of dW, and a forward whose missing pairs are masked by a MULTIPLICATION while X[0] holds a NaN."""
import numpy as np
import pytest
import torch

import fwd2_ref as F
import in_conv_ref as I

VARS = tuple(F.VARIATIONS)


def emu_fwd(X, W, nbr, bias=None, residual=None, ks=None, mask_by_multiply=False):
    """fp32 forward, offsets in the order ``ks`` (default: DESCENDING; an offset may be named twice)"""
    tab = torch.as_tensor(np.asarray(nbr)).long()
    out = torch.zeros(tab.shape[1], W.shape[2], dtype=torch.float32)
    for k in (range(tab.shape[0] - 1, -1, -1) if ks is None else ks):
        g = tab[k]
        if mask_by_multiply:           # what a kernel would compute that zeroes a missing pair's row 0 by a factor
            out += ((g >= 0).float()[:, None] * X[g.clamp_min(0)]) @ W[k]
        else:
            ok = torch.nonzero(g >= 0).flatten()
            out.index_add_(0, ok, X[g[ok]] @ W[k])
    if residual is not None:
        out += residual
    if bias is not None:
        out += bias
    return out


def emu_dw(X, dY, nbr):
    """fp32 weight gradient: one matrix product per offset over all of its pairs"""
    tab = torch.as_tensor(np.asarray(nbr)).long()
    out = torch.zeros(tab.shape[0], X.shape[1], dY.shape[1], dtype=torch.float32)
    for k in range(tab.shape[0]):
        ok = torch.nonzero(tab[k] >= 0).flatten()
        if ok.numel():
            out[k] = X[tab[k][ok]].t() @ dY[ok]
    return out


def _slice(P, s, M_out):
    return P[:, s * I.SL:min(M_out, (s + 1) * I.SL)]


# ---------------------------------------------------------------- cases and tables

def test_cases_name_the_workgroup_counts_of_the_launch_rules():
    for cus in (I.CUS_MI355X, 304, 64):
        cs = I.cases(cus)
        assert [c.name for c in cs] == list(I.NAMES)
        for c in cs:
            assert c.dw_wgs == I.dw_workgroups(c.M_out, cus) and c.fwd_wgs == I.fwd_workgroups(c.M_out, cus), (cus, c)
        dwc, fwc = I.case("dw-capped", cus), I.case("fwd-capped", cus)
        assert dwc.M_out % 32 == 5 and fwc.M_out % 32 == 5
        # above the cap: 38 slices more than waves -- waves 0 .. 37 walk two slices, the last of them the ragged one
        assert I.n_slices(dwc.M_out) == 2 * dwc.dw_wgs + 38 and dwc.dw_wgs == 2 * cus
        assert I.n_slices(fwc.M_out) == 4 * fwc.fwd_wgs + 38 and fwc.fwd_wgs == 2 * cus
        assert dwc.fwd_wgs < 2 * cus                       # the forward of the dW size stays below its cap
    sizes = [c.M_out for c in I.CASES[:12]]
    assert sizes == [1, 31, 32, 33, 64, 65, 127, 128, 129, 448, 512, 513]
    assert [I.case(f"rows-{m}").dw_wgs for m in (448, 512, 513)] == [7, 8, 9]       # the reduce kernel's lane groups


@pytest.mark.parametrize("name", I.NAMES)
def test_tables_keep_their_promises_and_thin_keeps_what_it_is_told(name):
    c = I.case(name)
    n = I.n_slices(c.M_out)
    for v in VARS:
        tab, M_in = I.table_of(c, v)
        P = tab.info["packed"]
        assert np.array_equal(F.pack(tab.nbr, tab.order), P) and tab.order is not None
        assert P.min() >= -1 and P.max() < M_in
        sp = I.special_slices(c.M_out)
        if n >= 3:
            assert (_slice(P, sp["empty"], c.M_out) < 0).all()                                        # (a)
            last = _slice(P, sp["last_k"], c.M_out)
            assert (last[:-1] < 0).all() and (last[-1] >= 0).all()                                     # (b)
            assert np.array_equal(np.sort(tab.info["empty_rows"]),
                                  np.sort(tab.order[sp["empty"] * 32:sp["empty"] * 32 + 32]))
        assert (P == 0).any() and (P == M_in - 1).any()                                               # (c)
        if c.M_out % 32 and c.M_out > 1:
            rag = _slice(P, n - 1, c.M_out)
            assert (rag < 0).any() and (rag >= 0).any()                                               # (d)
        if n >= 4 and v != "up":
            assert (_slice(P, sp["dense"], c.M_out) >= 0).all()                                       # (f)
        if v == "up":
            assert ((P >= 0).sum(0) <= 2).all()
        if not c.thinned:
            continue
        keep, walk = I.keep_slices(c.M_out), I.walk_slices(c.M_out)
        full, _ = I.table(c.M_out, v)
        for s in range(n):
            got, orig = _slice(P, s, c.M_out), _slice(full.info["packed"], s, c.M_out)
            if s in walk:
                assert np.array_equal(got, orig), (name, v, s)
            elif s in keep:      # a spare slice: whole offsets of it may have gone to the pair cap, never all of them
                gone = (got < 0).all(1)
                assert np.array_equal(got[~gone], orig[~gone]) and (got >= 0).any(), (name, v, s)
            else:
                assert (got < 0).all(), (name, v, s)
        plain = I.thin(full, c.M_out, keep)               # without the cap: exactly the slices of keep
        for s in range(n):
            orig = _slice(full.info["packed"], s, c.M_out)
            assert np.array_equal(_slice(plain.info["packed"], s, c.M_out), orig if s in keep else np.full_like(orig, -1))
        assert tab.info["kept"] == sorted(keep) and len(keep) <= 64
        # the walks the case is for, at the dW grid (4 CUs waves) and the forward grid (8 CUs waves)
        for n_waves in (4 * I.CUS_MI355X, 8 * I.CUS_MI355X)[:2 if name == "fwd-capped" else 1]:
            for w in (0, 5):
                assert w + n_waves < n and {w, w + n_waves} <= keep
        assert {n - 2, n - 1} <= keep and set(range(0, n, 41)) <= keep
        per_offset = (P >= 0).sum(1)
        assert per_offset.min() >= 1 and per_offset.max() <= 500, (name, v, per_offset)


def test_thin_with_and_without_a_tile_order():
    for events in (("perm",), ()):
        tab = F.make_table(3, 200, 200, 27, events)
        t = I.thin(tab, 200, {0, 6})
        P = F.pack(t.nbr, t.order)
        assert np.array_equal(P, t.info["packed"])
        assert np.array_equal(P[:, :32], tab.info["packed"][:, :32]) and np.array_equal(P[:, 192:], tab.info["packed"][:, 192:])
        assert (P[:, 32:192] < 0).all() and (P[:, :32] >= 0).any() and (P[:, 192:] >= 0).any()


def test_without_row_0_moves_every_gather_of_row_0():
    tab, M_in = I.table(513, "eq")
    t = I.without_row_0(tab)
    assert (tab.nbr == 0).any() and not (t.nbr == 0).any()
    assert np.array_equal(t.nbr < 0, tab.nbr < 0) and np.array_equal(t.nbr[tab.nbr > 0], tab.nbr[tab.nbr > 0])
    assert np.array_equal(F.pack(t.nbr, t.order), t.info["packed"])


def test_generic_forward_plan_ref_agrees_with_the_workspace_query():
    """the launch rule tests/test_gpu_generic_fwd.py restates (fwd_nb + fwd_ksplit of csrc/spconv.hip) against the library's
    own size query -- host arithmetic -- at its cases and on a seeded sweep; and its cases reach their branches"""
    import test_gpu_generic_fwd as G
    G.test_the_cases_reach_the_branches_they_are_named_for()
    rng = np.random.default_rng(21)
    shapes = [(c.M_out, c.K, c.Cin, c.Cout) for c in G.CASES]
    for _ in range(3000):
        M_out = int(min(300000, max(1, round(float(np.exp(rng.uniform(0.0, np.log(300000.0))))))))
        shapes.append((M_out, int(rng.choice([1, 2, 8, 27, 64, 125])), int(rng.integers(1, 200)), int(rng.integers(1, 300))))
    for M_out, K, Cin, Cout in shapes:
        p = G.plan_ref(M_out, K, Cout)
        assert 1 <= p.kz <= p.ks <= K and p.NB * 32 * p.gy >= Cout > p.NB * 32 * (p.gy - 1)
        assert G.workspace_bytes(M_out, K, Cin, Cout) == (256 if p.ks == 1 else p.ks * M_out * Cout * 4 + 256), (M_out, K, Cout)


# ---------------------------------------------------------------- the emulation passes both checkers everywhere

@pytest.mark.parametrize("name", I.NAMES)
def test_the_fp32_emulation_passes_and_a_dropped_pair_stands_out(name):
    c = I.case(name)
    w_f = w_d = 0.0
    d_f = d_d = float("inf")
    for v in VARS:
        tab, M_in = I.table_of(c, v)
        X, W, WT, bias, residual, dY, _ = I.make_inputs(M_in, c.M_out, 5)
        for b, r in ((None, None), (bias, residual)):
            res = F.check_conv(emu_fwd(X, W, tab.nbr, b, r), X, WT, tab.nbr, 0, b, r, extra=0, what=f"{name} {v}")
            w_f, d_f = max(w_f, res.all), min(d_f, res.drop)
        ref = I.dw_ref(X, dY, tab.nbr)
        ratio, drop = I.check_in_dw(emu_dw(X, dY, tab.nbr), X, dY, tab.nbr, f"{name} {v}", ref=ref)
        w_d, d_d = max(w_d, ratio), min(d_d, drop)
        # the rounded reference itself: one rounding against 2 gamma_{n + 1}, n >= 1
        ratio, _ = I.check_in_dw(ref[0].float(), X, dY, tab.nbr, f"{name} {v}", ref=ref)
        assert ratio <= 0.25 + 1e-9
        # offsets without pairs (rows-1: most of them) are exact zeros in the reference
        assert bool((ref[0][ref[2] == 0] == 0).all())
    print(f"[in-conv-ref] {name}: forward error/bound {w_f:.3f} dropped pair/bound {d_f:.3e}; dW error/bound {w_d:.3f} "
          f"dropped pair/bound {d_d:.3e}")
    assert w_f <= 1.0 and w_d <= 1.0
    # the removed pair stands 10 bounds out: a kernel result anywhere inside the bound (1 of them) cannot hide it
    assert d_f > 10.0 and d_d > 10.0


# ---------------------------------------------------------------- simulated wrong kernels fail

SIMS = (("rows-33", "eq"), ("rows-513", "gt"), ("dw-capped", "eq"), ("fwd-capped", "up"))


@pytest.fixture(scope="module", params=SIMS, ids=lambda p: f"{p[0]}-{p[1]}")
def sim(request):
    name, v = request.param
    c = I.case(name)
    tab, M_in = I.table_of(c, v)
    X, W, WT, bias, residual, dY, _ = I.make_inputs(M_in, c.M_out, 6)
    return c, tab, X, W, WT, bias, residual, dY, I.dw_ref(X, dY, tab.nbr)


def _fwd_fails(sim, got, match="outside the bound"):
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    with pytest.raises(AssertionError, match=match):
        F.check_conv(got, X, WT, tab.nbr, 0, bias, residual, extra=0, what="sim")


def _dw_fails(sim, got, match="outside the bound"):
    c, tab, X, W, WT, bias, residual, dY, ref = sim
    with pytest.raises(AssertionError, match=match):
        I.check_in_dw(got, X, dY, tab.nbr, "sim", ref=ref)


def test_the_unharmed_emulation_passes(sim):
    c, tab, X, W, WT, bias, residual, dY, ref = sim
    F.check_conv(emu_fwd(X, W, tab.nbr, bias, residual), X, WT, tab.nbr, 0, bias, residual, extra=0, what="sim")
    I.check_in_dw(emu_dw(X, dY, tab.nbr), X, dY, tab.nbr, "sim", ref=ref)


def test_a_dropped_pair_fails(sim):
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    cnt = (tab.nbr >= 0).sum(1)
    for k in (int(np.argmax(cnt)), int(np.argmin(np.where(cnt > 0, cnt, 1 << 30)))):    # most / least populated offset
        rows = np.flatnonzero(tab.nbr[k] >= 0)
        nbr = tab.nbr.copy()
        nbr[k, rows[len(rows) // 2]] = -1
        _fwd_fails(sim, emu_fwd(X, W, nbr, bias, residual))
        _dw_fails(sim, emu_dw(X, dY, nbr))


def test_a_dropped_packed_slice_fails(sim):
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    P = tab.info["packed"]
    n = I.n_slices(c.M_out)
    pairs = [int((_slice(P, s, c.M_out) >= 0).sum()) for s in range(n)]
    live = [s for s in range(n) if pairs[s]]
    for s in (live[0], live[-1], min(live, key=lambda t: pairs[t])):      # first, last (ragged), the lightest
        t = I.thin(tab, c.M_out, set(range(n)) - {s})
        _fwd_fails(sim, emu_fwd(X, W, t.nbr, bias, residual))
        _dw_fails(sim, emu_dw(X, dY, t.nbr))


def test_the_second_halfs_offsets_left_out_fail(sim):
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    assert (tab.nbr[14:] >= 0).any()
    _fwd_fails(sim, emu_fwd(X, W, tab.nbr, bias, residual, ks=range(13, -1, -1)))
    got = emu_dw(X, dY, tab.nbr)
    got[14:] = 0.0
    _dw_fails(sim, got)


def test_offset_26_in_place_of_the_zero_offset_fails(sim):
    """half 1 holds the offsets 14 .. 26 and one zero offset (k < IN_K ? ... : 0); a clamp of k instead takes 26 twice"""
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    assert (tab.nbr[26] >= 0).any()
    _fwd_fails(sim, emu_fwd(X, W, tab.nbr, bias, residual, ks=[26] + list(range(26, -1, -1))))
    got = emu_dw(X, dY, tab.nbr)
    got[26] *= 2.0
    _dw_fails(sim, got)


def test_dw_without_the_rows_of_the_ragged_last_slice_fails(sim):
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    n = I.n_slices(c.M_out)
    assert c.M_out % 32 and (_slice(tab.info["packed"], n - 1, c.M_out) >= 0).any()
    t = I.thin(tab, c.M_out, range(n - 1))
    _dw_fails(sim, emu_dw(X, dY, t.nbr))


def test_a_missing_pair_masked_by_a_multiplication_fails_on_a_nan_in_row_0(sim):
    c, tab, X, W, WT, bias, residual, dY, _ = sim
    assert X.shape[0] >= 2
    t = I.without_row_0(tab)
    Xp = X.clone()
    Xp[0] = torch.tensor(I.POISON)
    # the select (the kernel's form) never sees the poisoned row: finite and inside the bound
    F.check_conv(emu_fwd(Xp, W, t.nbr, bias, residual), Xp, WT, t.nbr, 0, bias, residual, extra=0, what="sim")
    I.check_in_dw(emu_dw(Xp, dY, t.nbr), Xp, dY, t.nbr, "sim")
    got = emu_fwd(Xp, W, t.nbr, bias, residual, mask_by_multiply=True)
    assert bool(torch.isnan(got[(t.nbr < 0).any(0)]).all())
    with pytest.raises(AssertionError, match="non-finite"):
        F.check_conv(got, Xp, WT, t.nbr, 0, bias, residual, extra=0, what="sim")
