"""GPU, default build: the fp32 forward / dIn sparse convolution -- spconv_fwd2_kernel / fwd2_body and the slab sums
spconv2_reduce_kernel / spconv2_reduce_stats_kernel (csrc/spconv2.hip, csrc/spconv2_body.h) -- against fp64 at EVERY launch
plan of the default build, through wsis_spconv_fwd_t and wsis_spconv_fwd_t_bn directly.

Cases (tests/fwd2_ref.py: MATRIX, the smallest shapes that select each plan; the plan of every case is read back through
wsis_debug_fwd2_plan and asserted): one wave per item with the table entries in registers and the XCD runs (K = 27 ragged,
K = 8), one wave without a table (dense 1x1) and with the identity table, 2 / 4 / 8 / 16 waves (with waves that own no offset:
K = 1 at 2 and 8 waves, K = 8 at 16), 2 / 4 / 8 offset slabs behind 4 waves (owner pattern P = ZS NW = 32 only there), the
two sides of the slab threshold (3072 / 3073 rows, K = 16 / 15) and 1, 31, 32, 33 rows.  Each on synthetic gather tables
(fwd2_ref.make_table: an all-empty slice, a slice whose only offset is K - 1, gathers of the first and the last input row,
a ragged last slice, one input row under several offsets) with M_in == M_out, M_in > M_out, M_in < M_out with one pair per
row, and M_in = 1; X is followed by 64 rows of NaN, and the output, the slab workspace (0xFF) and the partials start as NaN.

Asserted per case: the named plan; fwd2_ref.check_conv (per-element bound 2 gamma_n S, derived in fwd2_ref; finite; the
reference without one pair lies outside the bound) for flip x bias x residual; rows of the all-empty slice == bias +
residual exactly; two launches, and the same table under no tile order and two permutations, give the same bits; with
statistics: output bit-equal, no NaN left, both partial rows of every slice inside the derived bounds against the slice's own
rows (tile order in the kernel's epilogue, row order in the slab reduce).  All of this runs at ALL FOUR table variations of
every case (the M_in = 1 table makes slices of equal rows, where the 32 delta^2 term of the squares bound decides), the
statistics also under each of the three tile orders; whole file: 15 s.  wsis_spconv_fwd_t_bn at three 1-wave, a 4-wave, a
16-wave, a slab and the 33-row case, again at every table variation: output bit-equal, partials held with ReLU on and off.  One real-geometry case per table kind
(submanifold 25,575 rows: NW 4; strided down to 6,290 rows: NW 8; strided up with flip: NW 4 -- asserted) is held to the
oracle's pair lists.

Measured on an MI355X, all 89 tests passing.  Largest error / bound per plan over every case, table variation and operand
combination: "all" over every element, "pairs" over the rows that have pairs (the figure that tests the factor 2 assumed
for the matrix instruction), "drop" the SMALLEST ratio by which the one-pair-removed reference stood outside the bound;
then the statistics partials (sum | centred squares; every variation, every tile order):
  plan                          product: all    pairs   drop      statistics: sum | squares
  NW 1, TR, XCD runs                     0.125   0.082   4.1e3                0.151 | 0.197
  NW 1, null / identity table            0.044   0.044   6.2e4                0.071 | 0.083
  NW 2                                   0.100   0.087   1.8e3                0.116 | 0.109
  NW 4                                   0.074   0.074   1.8e3                0.110 | 0.118
  NW 8                                   0.057   0.057   1.2e3                0.142 | 0.159
  NW 16                                  0.062   0.062   1.4e3                0.263 | 0.232
  NW 4, ZS 2 (and 1 .. 33 rows)          0.062   0.062   1.9e2                0.169 | 0.186
  NW 4, ZS 4                             0.050   0.037   6.8e1                0.152 | 0.142
  NW 4, ZS 8 (P = 32)                    0.036   0.023   2.7e1                0.191 | 0.260
  real geometry (subm | down | up)       0.004 | 0.020 | 0.034, drop >= 8.2e2 0.108 | 0.143
No ratio is near 1 -- nothing here questions the factor 2 -- and none is below 1e-3: the bounds themselves discriminate
(a dropped pair stands 27 to 60,000 bounds out).  The 0.125 and 0.100 of "all" are elements with bias + residual alone:
one rounding against 2 gamma_4.  The BatchNorm-backward partials reach 5e-4 .. 1.0e-3 of the bound borrowed from
tests/test_gpu_bn_edges.py (1e-3 relative + 1e-4 absolute, made for whole-column sums): THAT bound is loose for a 32-row
sum; what discriminates there is the slice order (tests/test_fwd2_ref_host.py: partials of the other order, or with the
ReLU mask ignored, fail it) and the bit-equality of the output.

Out of scope: the resident deep-level kernel (deep.hip) runs the same fwd2_body under its own phase loop, its equality
test stays ``experimental``; WSIS_FWD2_NB=2 is read once per process and stays opt-in; the EXPERIMENTAL-only forms (ring,
persistent, register-gather, fused input BatchNorm)."""
import numpy as np
import pytest
import torch

import conv_ref
import fwd2_ref as F
import wsis_native as _n

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = [s.name for s in F.MATRIX]
REAL_PLANS = {"subm": (4, 1, 0, 0), "down": (8, 1, 0, 0), "up-flip": (4, 1, 0, 0)}      # (NW, ZS, TR, xcd_run)
BN_CASES = ("nw1-null-table", "nw1-tr-identity-k1", "nw1-tr-xcd-k8", "nw4-zs1", "nw16-3105", "nw4-zs8-96-items", "rows-33")


@pytest.fixture(autouse=True)
def _no_plan_switches(monkeypatch):
    for k in ("WSIS_FWD2_SLAB_ITEMS", "WSIS_FWD2_NB", "WSIS_FWD2_DA", "WSIS_FWD2"):
        monkeypatch.delenv(k, raising=False)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(X, nbr_p, order, WT, flip, bias, residual, M_out, stats=False, bn=None, relu=0):
    """wsis_spconv_fwd_t (bn: wsis_spconv_fwd_t_bn) with the output, the slab workspace and the partials prefilled with
    NaN; -> (out, partials or None)"""
    lib = _n.hip()
    K, Cout, Cin = WT.shape
    M_in = X.shape[0]
    out = torch.full((M_out, Cout), float("nan"), device=DEV)
    wsb = int(lib.wsis_spconv_fwd_t_workspace_bytes(M_out, K, Cin, Cout))
    assert wsb >= 256
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    part = torch.full(((M_out + 31) // 32, 2, Cout), float("nan"), device=DEV) if (stats or bn is not None) else None
    if bn is None:
        _n.check(lib.wsis_spconv_fwd_t(_n.ptr(X), _n.ptr(nbr_p), _n.ptr(order), _n.ptr(WT), int(flip), _n.ptr(bias),
                                       _n.ptr(residual), _n.ptr(out), _n.ptr(part), M_in, M_out, K, Cin, Cout, _n.ptr(ws),
                                       wsb, _n.ptr(_n.sync_block()), _n.stream_ptr()), "spconv_fwd_t")
    else:
        assert bias is None and residual is None
        x, mean, var, gamma, beta, eps = bn
        _n.check(lib.wsis_spconv_fwd_t_bn(_n.ptr(X), _n.ptr(nbr_p), _n.ptr(order), _n.ptr(WT), int(flip), _n.ptr(out),
                                          _n.ptr(part), _n.ptr(x), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta),
                                          eps, int(relu), M_in, M_out, K, Cin, Cout, _n.ptr(ws), wsb,
                                          _n.ptr(_n.sync_block()), _n.stream_ptr()), "spconv_fwd_t_bn")
    torch.cuda.synchronize()
    return out, part


def _dev_table(tab, order="own"):
    """(packed table, tile order) on the device; ``order``: "own" = the table's, None, or a permutation"""
    if tab is None:
        return None, None
    o = tab.order if isinstance(order, str) else order
    return (torch.from_numpy(F.pack(tab.nbr, o)).to(DEV).contiguous(),
            None if o is None else torch.from_numpy(np.ascontiguousarray(o)).to(DEV))


def _setup(name, variation, seed=5):
    s = F.BY_NAME[name]
    tab, M_in = F.table_for(s, variation)
    X, WT, bias, residual, buf = F.make_inputs(s, M_in, seed, DEV)
    plan = F.plan_lib(s.M_out, s.K, s.Cin, s.Cout, tab is not None, M_in)
    assert (plan.NW, plan.ZS, plan.TR, plan.xcd_run) == (s.NW, s.ZS, s.TR, s.xcd), (name, variation, plan)
    return s, tab, M_in, X, WT, bias, residual, buf, plan


# ---------------------------------------------------------------- the product

@pytest.mark.parametrize("name", NAMES)
def test_product_against_fp64(name):
    worst, worst_pairs, worst_drop = 0.0, 0.0, float("inf")
    for v in F.variations(F.BY_NAME[name]):
        s, tab, M_in, X, WT, bias, residual, buf, plan = _setup(name, v)
        nbr = None if tab is None else tab.nbr
        nbr_p, order = _dev_table(tab)
        empty = None if tab is None or tab.info["empty_rows"] is None else torch.as_tensor(tab.info["empty_rows"]).to(DEV)
        for flip in (0, 1):
            core = F.conv(X, WT, nbr, flip, M_out=s.M_out)
            for b in (None, bias):
                for r in (None, residual):
                    what = f"{name} {v} flip={flip} bias={b is not None} residual={r is not None}"
                    out, _ = _launch(X, nbr_p, order, WT, flip, b, r, s.M_out)
                    again, _ = _launch(X, nbr_p, order, WT, flip, b, r, s.M_out)
                    assert torch.equal(_bits(out), _bits(again)), f"{what}: two launches differ"
                    want = core if b is None else core + b.double()
                    want = want if r is None else want + r.double()
                    res = F.check_conv(out, X, WT, nbr, flip, b, r, extra=plan.NW + plan.ZS, what=what, want=want)
                    worst, worst_pairs, worst_drop = max(worst, res.all), max(worst_pairs, res.pairs), min(worst_drop, res.drop)
                    if empty is not None:
                        exact = torch.zeros(len(empty), s.Cout, device=DEV)
                        exact = exact if b is None else exact + b
                        exact = exact if r is None else exact + r[empty]
                        assert torch.equal(out[empty], exact), f"{what}: rows of the all-empty slice"
        assert bool(torch.isnan(buf[M_in:]).all()) and bool(torch.isfinite(buf[:M_in]).all())
    print(f"[fwd2-plans] conv {name}: NW={plan.NW} ZS={plan.ZS} TR={plan.TR} xcd={plan.xcd_run}  error/bound {worst:.3e}  "
          f"rows with pairs {worst_pairs:.3e}  dropped pair/bound {worst_drop:.3e}")


@pytest.mark.parametrize("name", [n for n in NAMES if F.BY_NAME[n].table == "synthetic"])
def test_tile_order_does_not_change_a_row(name):
    """fwd2_body: the order of additions of an output row depends on the offset index alone -- the same table under no
    tile order and under two permutations gives every row the same bits (a leak between the rows of a slice would not).
    The statistics partials of every one of these launches are held to their bounds over the slices of ITS order."""
    w_sum = w_sq = 0.0
    for v in F.variations(F.BY_NAME[name]):
        s, tab, M_in, X, WT, bias, residual, buf, plan = _setup(name, v)
        outs = []
        for o in (None, tab.order, F.permutation(977 + s.M_out, s.M_out)):
            nbr_p, order = _dev_table(tab, o)
            plain, _ = _launch(X, nbr_p, order, WT, 1, bias, residual, s.M_out)
            out, part = _launch(X, nbr_p, order, WT, 1, bias, residual, s.M_out, stats=True)
            assert torch.equal(_bits(out), _bits(plain)), (name, v, "the statistics epilogue changed the output")
            a, q = F.check_stats(part, out, o, plan.ZS, f"{name} {v} order={'none' if o is None else 'perm'}")
            w_sum, w_sq = max(w_sum, a), max(w_sq, q)
            outs.append(out)
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2])), (name, v)
    print(f"[fwd2-plans] orders {name}: NW={plan.NW} ZS={plan.ZS}  sum error/bound {w_sum:.3e}  squares error/bound {w_sq:.3e}")


# ---------------------------------------------------------------- statistics partials

@pytest.mark.parametrize("name", NAMES)
def test_statistics_partials(name):
    w_sum = w_sq = 0.0
    for v in F.variations(F.BY_NAME[name]):
        s, tab, M_in, X, WT, bias, residual, buf, plan = _setup(name, v, seed=8)
        nbr_p, order = _dev_table(tab)
        for b, r in ((None, None), (bias, residual)):
            what = f"{name} {v} bias/residual={b is not None}"
            plain, _ = _launch(X, nbr_p, order, WT, 0, b, r, s.M_out)
            out, part = _launch(X, nbr_p, order, WT, 0, b, r, s.M_out, stats=True)
            assert torch.equal(_bits(out), _bits(plain)), f"{what}: the statistics epilogue changed the output"
            again, part2 = _launch(X, nbr_p, order, WT, 0, b, r, s.M_out, stats=True)
            assert torch.equal(_bits(part), _bits(part2)), f"{what}: two launches differ"
            a, q = F.check_stats(part, out, None if tab is None else tab.order, plan.ZS, what)
            w_sum, w_sq = max(w_sum, a), max(w_sq, q)
    print(f"[fwd2-plans] stats {name}: NW={plan.NW} ZS={plan.ZS}  sum error/bound {w_sum:.3e}  squares error/bound {w_sq:.3e}")


@pytest.mark.parametrize("name", BN_CASES)
def test_batchnorm_backward_partials(name):
    shape = F.BY_NAME[name]
    bn = F.bn_case(shape.M_out, shape.Cout, 11)
    bn_dev = tuple(t.to(DEV).contiguous() for t in bn[:5]) + (bn.eps,)
    worst = 0.0
    for v in F.variations(shape):
        s, tab, M_in, X, WT, bias, residual, buf, plan = _setup(name, v, seed=9)
        nbr_p, order = _dev_table(tab)
        for flip in (1, 0):
            plain, _ = _launch(X, nbr_p, order, WT, flip, None, None, s.M_out)
            for relu in (1, 0):
                what = f"{name} {v} flip={flip} relu={relu}"
                out, part = _launch(X, nbr_p, order, WT, flip, None, None, s.M_out, bn=bn_dev, relu=relu)
                assert torch.equal(_bits(out), _bits(plain)), f"{what}: the BatchNorm epilogue changed the output"
                worst = max(worst, F.check_bn_partials(part, out, bn, relu, None if tab is None else tab.order, plan.ZS, what))
    print(f"[fwd2-plans] bn-partials {name}: NW={plan.NW} ZS={plan.ZS}  error/bound {worst:.3e}")


# ---------------------------------------------------------------- real geometry, the tile order the rulebook schedules

@pytest.fixture(scope="module")
def room():
    import harness
    from oracle import spconv_ref as ref
    from spconv import ops
    b = harness.collate([harness.make_scene(41, room=(1.6, 1.3, 1.0), n_box=2)])
    idx = b["voxel_locs"].int().contiguous()
    shape = [int(v) for v in b["spatial_shape"]]
    idx_d = idx.to(DEV)
    rb = ops.build_subm_rulebook(idx_d, shape, [3] * 3, [1] * 3)
    rd = ops.build_down_rulebook(idx_d, shape, [2] * 3, [2] * 3, [0] * 3)
    subm = ref.subm_pairs_fast(idx.numpy(), shape, 3, 1)
    out_idx, _, down = ref.down_pairs_fast(idx.numpy(), shape, 2, 2, 0)
    assert np.array_equal(rd.out_indices.cpu().numpy(), np.asarray(out_idx, dtype=np.int32))
    return rb, rd, subm, down, int(idx.shape[0]), int(len(out_idx))


@pytest.mark.parametrize("kind", ["subm", "down", "up-flip"])
def test_real_geometry_against_the_oracle_pairs(room, kind):
    rb, rd, subm, down, M, Mo = room
    g = torch.Generator().manual_seed(13)
    if kind == "subm":
        K, Cin, Cout, M_in, M_out, flip = 27, 32, 64, M, M, 0
        nbr, nbr_p, order, pairs = rb.nbr, rb.nbr_p, rb.order, subm
    elif kind == "down":
        K, Cin, Cout, M_in, M_out, flip = 8, 32, 64, M, Mo, 0
        nbr, nbr_p, order, pairs = rd.nbr, rd.nbr_p, rd.order, down
    else:
        K, Cin, Cout, M_in, M_out, flip = 8, 64, 32, Mo, M, 1
        nbr, nbr_p, order, pairs = rd.nbr_up, rd.nbr_up_p, rd.order_up, conv_ref.swap(down)
    X = torch.randn(M_in, Cin, generator=g).to(DEV)
    WT = (torch.randn(K, Cout, Cin, generator=g) * 0.05).to(DEV)
    bias = (torch.randn(Cout, generator=g) * 0.1).to(DEV)
    plan = F.plan_lib(M_out, K, Cin, Cout, 1, M_in)
    # the plans the small room's tables select (25,575 and 6,290 rows): a change of the scene that moves them shows here
    assert (plan.NW, plan.ZS, plan.TR, plan.xcd_run) == REAL_PLANS[kind], (kind, M_in, M_out, plan)
    # weight of offset k as the pair lists use it: [Cin, Cout] = WT[flip ? K-1-k : k]^T
    W = (WT.flip(0) if flip else WT).transpose(1, 2).contiguous()
    want = conv_ref.rows(X, W, conv_ref.device_pairs(pairs, DEV), M_out, torch.arange(M_out, device=DEV)) + bias.double()
    out, part = _launch(X, nbr_p, order, WT, flip, bias, None, M_out, stats=True)
    what = f"{kind} {M_in}->{M_out} rows {Cin}->{Cout}"
    res = F.check_conv(out, X, WT, nbr, flip, bias, None, extra=plan.NW + plan.ZS, what=what, want=want)
    a, q = F.check_stats(part, out, order, plan.ZS, what)
    print(f"[fwd2-plans] real {what}: NW={plan.NW} ZS={plan.ZS} TR={plan.TR}  error/bound {res.all:.3e}  rows with pairs "
          f"{res.pairs:.3e}  dropped pair/bound {res.drop:.3e}  stats {a:.3e} / {q:.3e}")
