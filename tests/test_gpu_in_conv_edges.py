"""GPU, default build: the 6 -> 32 input convolution on the matrix cores (csrc/spconv_in.hip) -- spconv_in_kernel and its
weight gradient spconv_in_dw_kernel + spconv_in_dw_reduce_kernel -- against fp64 at every branch of the three kernels,
through wsis_spconv_fwd and wsis_spconv_dw directly.  tests/test_gpu_in_conv.py (real rooms, one blanket tolerance) stays.

Cases (tests/in_conv_ref.py: CASES, the smallest row counts that reach each branch, CUs = compute units of the device):
1, 31, 32, 33 rows (a partial slice -- lanes with my_row = -1 and the table index forced to -1 --, one full slice, one row
into a second; dW: one workgroup whose second wave owns no slice and still joins the slab sum); 64, 65 (dW: P = 1 with both
waves busy, P = 2 with an idle wave); 127, 128, 129 (forward: one workgroup's four waves, the last ragged, then a second
workgroup); 448, 512, 513 (dW: P = 7, 8, 9 slabs over the reduce kernel's eight lane groups); 32 (4 CUs) + 32 x 37 + 5 and
32 (8 CUs) + 32 x 37 + 5 rows: above the grid cap of dW and of the forward, 38 waves walk two slices (dW at the larger
count: three) and the others one -- the dW kernel's prefetch ``if (sn < n_slices)`` and the reuse of its LDS tile run only
there.  The two capped tables are thinned (in_conv_ref.thin) to the first / second / third-trip slices of waves 0 and 5,
the last two slices, every 41st slice and make_table's promised slices, at most 500 pairs per offset.  The workgroup count
every case is named for is asserted: dW through wsis_debug_dw_plan (kind 5, (ws_bytes - 256) / (5184 x 4)), the forward
by the launch rule min(ceil(slices / 4), 2 CUs).

Each row count runs on synthetic gather tables (fwd2_ref.make_table: an all-empty slice, a slice whose only offset is 26,
gathers of the first and the last input row, a ragged last slice, one input row under several offsets -- the half split of
the im2col vector, offsets 0 .. 13 | 14 .. 26 + one zero offset, sees pairs on both sides) at M_in == M_out, M_in = 2 M_out
+ 5, M_in = max(1, M_out // 3) with one pair per row, and M_in = 1, each with the table's own permutation as tile order and
with order = NULL.  X is followed by 64 rows of NaN inside its allocation (checked afterwards); out and dW start as NaN
and are followed by NaN that must stay NaN, the workspace starts as 0xFF.

Asserted.  Forward, bias x residual in {none, given}: fwd2_ref.check_conv with extra = 0 (finite; per-element bound
2 gamma_n S; the reference without one pair outside it); rows without a pair == bias + residual exactly; two launches the
same bits; the same table under order = NULL and two permutations gives every row the same bits (a row's value is one
k-ordered chain in one lane pair).  dW: in_conv_ref.check_in_dw (finite; bound 2 gamma_{n_k + 1} S; offsets without pairs
exactly zero; one pair removed stands outside); two launches the same bits.  Row 0 poison: no pair gathers input row 0 and
X[0] = [NaN, Inf, -Inf, NaN, 1e38, -1e38] -- the branch-free gather reads row 0 for every missing pair and must zero it by
a select: forward and dW finite and inside their bounds at 33 rows and at both capped sizes.  Alignment gate: X one float
into its storage takes the generic kernels (forward: the bits of the WSIS_IN_CONV=0 launch; dW: plan kind 6) and holds the
fp64 checks (dW: conv_ref.check_dw with the FRAC of tests/test_gpu_dw_walks.py).  Against the generic kernels: at 33 and
513 rows WSIS_IN_CONV=0 and 1 pass the same checkers.  Whole file: 6 s.

Measured on an MI355X (2026-10-21), all tests passing.  Largest error / bound ("all": every element, "pairs": rows with
pairs -- the figure that tests the factor 2 assumed for the matrix instruction) and the SMALLEST ratio by which the
one-pair-removed reference stood outside the bound ("drop"), over every table variation, tile order and operand combination:
  kernel, case group                                 all     pairs   drop
  forward, 1 .. 64 rows (one workgroup, one trip)    0.189   0.189   1.7e4
  forward, 65 .. 513 rows (1 .. 5 workgroups)        0.250   0.236   1.7e3
  forward, capped sizes (266 | 512 workgroups)       0.250 | 0.256   0.227 | 0.256   2.5e3
  forward, row 0 poisoned (33 rows | capped)         0.074 | 0.250
  dW, 1 .. 129 rows (P = 1 .. 3, idle waves)         0.311           2.4e4
  dW, 448 | 512 | 513 rows (P = 7 | 8 | 9)           0.120 | 0.098 | 0.067   7.3e3
  dW, capped sizes (P = 512: two | three trips)      0.047 | 0.014   1.7e3 | 2.9e2
  dW, row 0 poisoned (33 rows | capped)              0.270 | 0.036
  generic kernels behind the alignment gate / WSIS_IN_CONV=0: forward 0.025, dW 0.261 of check_in_dw's bound
No ratio is near 1 -- nothing here questions the factor 2 -- and a dropped pair stands at least 280 bounds out.  The 0.25
of the forward are elements of one or two terms (bias + residual alone, or one rounding of a short chain against
2 gamma_n with n = 2 .. 6); the dW figures fall with the number of pairs because the bound grows with n_k while the
error of a sum of random signs grows with its square root.
These are observations for judging the factor 2, not thresholds."""
import numpy as np
import pytest
import torch

import conv_ref
import dw_plan_ref
import fwd2_ref as F
import in_conv_ref as I
import wsis_native as _n
from test_gpu_generic_fwd import bits, dev_table, launch_fwd, one_float_in, plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = tuple(F.VARIATIONS)
FRAC = 1e-5                    # the dW bound of tests/test_gpu_dw_walks.py (fraction of max |dW_fp64|), for the generic kernel
KIND_IN_CONV, KIND_GENERIC = 5, 6


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in ("WSIS_IN_CONV", "WSIS_CONV_MATH"):
        monkeypatch.delenv(k, raising=False)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(name):
    cus = _cus()
    c = I.case(name, cus)
    assert c.dw_wgs == I.dw_workgroups(c.M_out, cus) and c.fwd_wgs == I.fwd_workgroups(c.M_out, cus), (c, cus)
    return c, cus


def _dw_plan(X, dY, dW, ws, M_out, has_order):
    """wsis_debug_dw_plan of the launch these pointers make"""
    _n.hip()
    al = lambda t, a: t.data_ptr() % a == 0
    align = (dw_plan_ref.X16 * al(X, 16) | dw_plan_ref.X8 * al(X, 8) | dw_plan_ref.DY16 * al(dY, 16)
             | dw_plan_ref.DW16 * al(dW, 16) | dw_plan_ref.WS16 * al(ws, 16))
    table = dw_plan_ref.TABLE if has_order else dw_plan_ref.TABLE_NO_ORDER
    p = dw_plan_ref.plan_lib(dw_plan_ref.Case("in", X.shape[0], M_out, I.IN_K, I.IN_C, I.IN_O, table, align, 0, 1, ""))
    assert p is not None
    return p


def launch_dw(X, nbr_p, order, dY):
    """wsis_spconv_dw with dW full of NaN and the workspace full of 0xFF; -> (dW, plan of this launch).  dW is followed by
    256 floats of NaN inside its allocation, which must still be NaN afterwards (the im2col matrix has 168 columns in
    LDS and 192 in the accumulators: the guard m < IN_K IN_C keeps the thirty padding columns 162 .. 191 out of dW)."""
    lib = _n.hip()
    M_out = dY.shape[0]
    wsb = int(lib.wsis_spconv_dw_workspace_bytes(M_out, I.IN_K, I.IN_C, I.IN_O))
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    guard = torch.full((I.DW_SLAB_FLOATS + 256,), float("nan"), device=DEV)
    dW = guard[:I.DW_SLAB_FLOATS].view(I.IN_K, I.IN_C, I.IN_O)
    plan = _dw_plan(X, dY, dW, ws, M_out, order is not None)
    assert plan["ws_bytes"] <= wsb
    _n.check(lib.wsis_spconv_dw(_n.ptr(X), _n.ptr(nbr_p), _n.ptr(order), _n.ptr(dY), _n.ptr(dW), X.shape[0], M_out,
                                I.IN_K, I.IN_C, I.IN_O, _n.ptr(ws), wsb, _n.stream_ptr()), "spconv_dw")
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard[I.DW_SLAB_FLOATS:]).all()), "spconv_dw wrote behind dW"
    return dW, plan


def _slabs(plan):
    q, rem = divmod(plan["ws_bytes"] - 256, I.DW_SLAB_FLOATS * 4)
    assert rem == 0
    return q


def _tail_is_nan(buf, M_in):
    return bool(torch.isnan(buf[M_in:]).all()) and buf[M_in:].shape[0] == 64


def _exact_rows(out, rows, b, r, what):
    if rows.numel():
        exact = torch.zeros(rows.numel(), out.shape[1], device=DEV)
        exact = exact if b is None else exact + b
        exact = exact if r is None else exact + r[rows]
        assert torch.equal(out[rows], exact), f"{what}: rows without a pair (all-empty slices among them)"


# ---------------------------------------------------------------- forward

@pytest.mark.parametrize("name", I.NAMES)
def test_forward_against_fp64(name):
    c, cus = _case(name)
    # the grid of spconv_in_launch: four waves a workgroup, one slice a wave and trip, two workgroups a CU at the most
    assert min(-(-I.n_slices(c.M_out) // 4), 2 * cus) == c.fwd_wgs
    if name == "fwd-capped":
        assert I.n_slices(c.M_out) == 4 * c.fwd_wgs + 38
    worst, worst_pairs, worst_drop = 0.0, 0.0, float("inf")
    for v in VARS:
        tab, M_in = I.table_of(c, v, cus)
        X, W, WT, bias, residual, dY, buf = I.make_inputs(M_in, c.M_out, 5, DEV)
        assert X.data_ptr() % 8 == 0
        core = F.conv(X, WT, tab.nbr, 0, M_out=c.M_out)
        bare = torch.from_numpy(I.rows_without_pairs(tab.nbr)).to(DEV)
        assert I.n_slices(c.M_out) < 3 or bare.numel() >= 32
        for own in ("own", None):
            nbr_p, order = dev_table(tab, own)
            for b in (None, bias):
                for r in (None, residual):
                    what = f"{name} {v} order={own} bias={b is not None} residual={r is not None}"
                    out = launch_fwd(X, nbr_p, order, W, b, r, c.M_out)
                    again = launch_fwd(X, nbr_p, order, W, b, r, c.M_out)
                    assert torch.equal(bits(out), bits(again)), f"{what}: two launches differ"
                    want = core if b is None else core + b.double()
                    want = want if r is None else want + r.double()
                    res = F.check_conv(out, X, WT, tab.nbr, 0, b, r, extra=0, what=what, want=want)
                    worst, worst_pairs, worst_drop = max(worst, res.all), max(worst_pairs, res.pairs), min(worst_drop, res.drop)
                    _exact_rows(out, bare, b, r, what)
        assert _tail_is_nan(buf, M_in) and bool(torch.isfinite(buf[:M_in]).all())
    print(f"[in-conv-edges] forward {name}: rows={c.M_out} workgroups={c.fwd_wgs}  error/bound {worst:.3e}  rows with pairs "
          f"{worst_pairs:.3e}  dropped pair/bound {worst_drop:.3e}")


@pytest.mark.parametrize("name", I.NAMES)
def test_tile_order_does_not_change_a_row(name):
    """spconv_in_kernel: a row's 162 products are one k-ordered chain in the two lanes of the row -- which slice, wave or
    workgroup the tile order puts the row into cannot enter its value"""
    c, cus = _case(name)
    for v in VARS:
        tab, M_in = I.table_of(c, v, cus)
        X, W, WT, bias, residual, dY, buf = I.make_inputs(M_in, c.M_out, 6, DEV)
        outs = []
        for o in (None, tab.order, F.permutation(977 + c.M_out, c.M_out)):
            nbr_p, order = dev_table(tab, o)
            outs.append(launch_fwd(X, nbr_p, order, W, bias, residual, c.M_out))
        assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(outs[0]), bits(outs[2])), (name, v)


# ---------------------------------------------------------------- weight gradient

@pytest.mark.parametrize("name", I.NAMES)
def test_weight_gradient_against_fp64(name):
    c, cus = _case(name)
    worst, worst_drop = 0.0, float("inf")
    for v in VARS:
        tab, M_in = I.table_of(c, v, cus)
        X, W, WT, bias, residual, dY, buf = I.make_inputs(M_in, c.M_out, 7, DEV)
        ref = I.dw_ref(X, dY, tab.nbr)
        for own in ("own", None):
            what = f"{name} {v} order={own}"
            nbr_p, order = dev_table(tab, own)
            dW, plan = launch_dw(X, nbr_p, order, dY)
            assert plan["kind"] == KIND_IN_CONV and _slabs(plan) == c.dw_wgs, (what, plan)
            again, _ = launch_dw(X, nbr_p, order, dY)
            assert torch.equal(bits(dW), bits(again)), f"{what}: two launches differ"
            ratio, drop = I.check_in_dw(dW, X, dY, tab.nbr, what, ref=ref)
            worst, worst_drop = max(worst, ratio), min(worst_drop, drop)
        assert _tail_is_nan(buf, M_in) and bool(torch.isfinite(buf[:M_in]).all())
    print(f"[in-conv-edges] dW {name}: rows={c.M_out} slabs={c.dw_wgs}  error/bound {worst:.3e}  dropped pair/bound "
          f"{worst_drop:.3e}")


# ---------------------------------------------------------------- a non-finite row 0 that no pair gathers

@pytest.mark.parametrize("name", ["rows-33", "dw-capped", "fwd-capped"])
def test_row_0_poison_does_not_leak_through_missing_pairs(name):
    c, cus = _case(name)
    worst_f = worst_d = 0.0
    for v in ("eq", "gt", "up"):
        full, M_in = I.table_of(c, v, cus)
        assert M_in >= 2
        tab = I.without_row_0(full)
        assert not (tab.nbr == 0).any() and (tab.nbr < 0).any()
        X, W, WT, bias, residual, dY, buf = I.make_inputs(M_in, c.M_out, 8, DEV)
        X[0] = torch.tensor(I.POISON, device=DEV)
        for own in ("own", None):
            what = f"poison {name} {v} order={own}"
            nbr_p, order = dev_table(tab, own)
            out = launch_fwd(X, nbr_p, order, W, bias, residual, c.M_out)
            res = F.check_conv(out, X, WT, tab.nbr, 0, bias, residual, extra=0, what=what)
            dW, plan = launch_dw(X, nbr_p, order, dY)
            assert plan["kind"] == KIND_IN_CONV
            ratio, _ = I.check_in_dw(dW, X, dY, tab.nbr, what)
            worst_f, worst_d = max(worst_f, res.all), max(worst_d, ratio)
        assert bool(torch.isnan(X[0, 0])) and _tail_is_nan(buf, M_in)
    print(f"[in-conv-edges] poison {name}: forward error/bound {worst_f:.3e}  dW error/bound {worst_d:.3e}")


# ---------------------------------------------------------------- the 8-byte alignment gate

def _pairs_of(nbr):
    out = []
    for k in range(nbr.shape[0]):
        po = np.flatnonzero(nbr[k] >= 0)
        out.append((nbr[k][po].astype(np.int64), po))
    return conv_ref.device_pairs(out, DEV)


@pytest.mark.parametrize("rows", [33, 513])
def test_a_4_byte_aligned_x_takes_the_generic_kernels(rows, monkeypatch):
    c, cus = _case(f"rows-{rows}")
    kz = plan_ref(rows, I.IN_K, I.IN_O).kz
    for v in ("eq", "gt"):
        tab, M_in = I.table_of(c, v, cus)
        Xa, W, WT, bias, residual, dY, _ = I.make_inputs(M_in, rows, 9, DEV)
        X, store = one_float_in(Xa)
        nbr_p, order = dev_table(tab)
        what = f"unaligned {rows} {v}"
        out = launch_fwd(X, nbr_p, order, W, bias, residual, rows)
        res = F.check_conv(out, X, WT, tab.nbr, 0, bias, residual, extra=kz, what=what)
        monkeypatch.setenv("WSIS_IN_CONV", "0")
        generic = launch_fwd(Xa, nbr_p, order, W, bias, residual, rows)
        monkeypatch.delenv("WSIS_IN_CONV")
        assert torch.equal(bits(out), bits(generic)), f"{what}: not the generic forward's bits"
        dW, plan = launch_dw(X, nbr_p, order, dY)
        assert plan["kind"] == KIND_GENERIC, plan
        err, bound, err_drop = conv_ref.check_dw(dW, X, dY, _pairs_of(tab.nbr), FRAC, what)
        assert bool(torch.isnan(store[-64 * I.IN_C:]).all()) and bool(torch.isnan(store[0]))
        print(f"[in-conv-edges] {what}: forward error/bound {res.all:.3e} dropped pair/bound {res.drop:.3e}; dW err "
              f"{err:.2e} <= {bound:.2e}, one pair removed {err_drop:.2e}")


# ---------------------------------------------------------------- both kernels under the same fp64 checks

@pytest.mark.parametrize("rows", [33, 513])
def test_the_generic_kernels_and_the_input_conv_pass_the_same_checks(rows, monkeypatch):
    """(their summation orders differ: no bit equality between the two is asserted)"""
    c, cus = _case(f"rows-{rows}")
    kz = plan_ref(rows, I.IN_K, I.IN_O).kz
    for v in VARS:
        tab, M_in = I.table_of(c, v, cus)
        X, W, WT, bias, residual, dY, buf = I.make_inputs(M_in, rows, 10, DEV)
        nbr_p, order = dev_table(tab)
        ref = I.dw_ref(X, dY, tab.nbr)
        line = []
        for env, kind, extra in (("0", KIND_GENERIC, kz), ("1", KIND_IN_CONV, 0)):
            monkeypatch.setenv("WSIS_IN_CONV", env)
            what = f"WSIS_IN_CONV={env} {rows} {v}"
            out = launch_fwd(X, nbr_p, order, W, bias, residual, rows)
            res = F.check_conv(out, X, WT, tab.nbr, 0, bias, residual, extra=extra, what=what)
            dW, plan = launch_dw(X, nbr_p, order, dY)
            assert plan["kind"] == kind, (what, plan)
            ratio, drop = I.check_in_dw(dW, X, dY, tab.nbr, what, ref=ref)
            line.append(f"={env}: forward {res.all:.3e} dW {ratio:.3e}")
        assert _tail_is_nan(buf, M_in)
        print(f"[in-conv-edges] both kernels {rows} {v}: error/bound WSIS_IN_CONV" + "  WSIS_IN_CONV".join(line))
