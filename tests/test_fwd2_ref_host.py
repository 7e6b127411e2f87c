"""CPU: the reference, the cases and the checkers of tests/fwd2_ref.py (the fp32 forward / dIn convolution of
csrc/spconv2.hip against fp64) are themselves right.

  * plan_ref equals the library's own plan query wsis_debug_fwd2_plan (plan2() + form2(): what the launch calls) at every
    shape of the matrix and on a seeded sweep of 4,000 shapes; every matrix shape selects the plan its name claims; every
    plan key of the default build (NW 1 .. 16, ZS 1 .. 8, table in registers on / off, XCD runs) is reached by a case;
  * fwd2_ref.conv equals oracle.spconv_ref.pairs_conv on a real submanifold and a real strided table;
  * the fp64 reference rounded to fp32 passes check_conv at every matrix case (the data scales let the dropped-pair check
    discriminate everywhere), and SIMULATED wrong kernels fail: this is the evidence, obtained without any GPU run, that a
    subtly wrong kernel cannot pass tests/test_gpu_fwd2_plans.py."""
import numpy as np
import pytest
import torch

import bn_ref
import fwd2_ref as F
from oracle import spconv_ref as ref


@pytest.fixture(autouse=True)
def _no_plan_switches(monkeypatch):
    for k in ("WSIS_FWD2_SLAB_ITEMS", "WSIS_FWD2_NB", "WSIS_FWD2_DA"):      # the switches the default build reads
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- plans

def test_plan_ref_agrees_with_the_library():
    for s in F.MATRIX:
        for has_table in (0, 1):
            if has_table or s.K == 1:
                assert F.plan_ref(s.M_out, s.K, s.Cin, s.Cout, has_table=has_table, M_in=s.M_out) == \
                    F.plan_lib(s.M_out, s.K, s.Cin, s.Cout, has_table, s.M_out), s.name
    rng = np.random.default_rng(20)
    chans = np.arange(32, 257, 32)
    for i in range(4000):
        K = int(rng.choice([1, 2, 8, 15, 16, 27, 32]))
        Cin, Cout = int(rng.choice(chans)), int(rng.choice(chans))
        # row counts on a log scale, so that the few-item plans (slabs, 8 and 16 waves) get their share of the sweep
        M_out = int(min(200000, max(1, round(float(np.exp(rng.uniform(0.0, np.log(200000.0))))))))
        M_in = int(rng.choice([1, M_out, 2 * M_out + 5, (1 << 24) - 1, 1 << 24]))
        has_table = int(rng.random() < 0.8)
        assert F.plan_ref(M_out, K, Cin, Cout, has_table=has_table, M_in=M_in) == \
            F.plan_lib(M_out, K, Cin, Cout, has_table, M_in), (M_out, K, Cin, Cout, has_table, M_in)


def test_plan_query_rejects_bad_arguments():
    fn = F.plan_fn()
    out = np.zeros(7, dtype=np.int32)
    assert fn(100, 27, 32, 32, 1, 100, None) == -1
    assert fn(0, 27, 32, 32, 1, 100, out.ctypes.data) == -1
    assert fn(100, 33, 32, 32, 1, 100, out.ctypes.data) == -1
    assert fn(100, 27, 48, 32, 1, 100, out.ctypes.data) == -1
    assert fn(100, 27, 32, 32, 1, -1, out.ctypes.data) == -1


def test_matrix_plans_are_the_named_ones_and_reach_every_plan_key():
    seen = set()
    for s in F.MATRIX:
        p = F.plan_lib(s.M_out, s.K, s.Cin, s.Cout, s.table != "null", s.M_out)
        assert (p.NW, p.ZS, p.TR, p.xcd_run) == (s.NW, s.ZS, s.TR, s.xcd), (s.name, p)
        assert (p.NB, p.DA, p.BD) == (1, 2, 1), (s.name, p)
        seen |= {("NW", p.NW), ("ZS", p.ZS), ("TR", p.TR), ("xcd", p.xcd_run > 0), ("P", p.NW * p.ZS)}
        for v in F.variations(s):       # the table variations keep the plan (TR: M_in stays below 2^24)
            M_in = F.VARIATIONS[v][0](s.M_out)
            assert F.plan_lib(s.M_out, s.K, s.Cin, s.Cout, s.table != "null", M_in) == p
    want = {("NW", n) for n in (1, 2, 4, 8, 16)} | {("ZS", z) for z in (1, 2, 4, 8)} | \
           {("TR", 0), ("TR", 1), ("xcd", True), ("xcd", False), ("P", 32)}      # P = 32: the owner pattern of ZS 8 x NW 4
    assert want <= seen, sorted(want - seen)
    # the neighbours the matrix names: 15 offsets take no slabs, 3072 / 3073 rows sit on the two sides of 96 items
    assert F.BY_NAME["nw8-k15-no-slabs"].ZS == 1 and F.BY_NAME["nw4-zs2-k16"].ZS == 2
    assert (3072 // 32, (3073 + 31) // 32) == (96, 97)
    # idle waves: offsets k with k mod (ZS NW) == z + ZS wave; K = 8 at 16 waves and K = 1 at 8 and 2 leave waves empty
    for name, idle in (("nw16-k8-waves-8-15-idle", 8), ("nw8-k1-seven-idle", 7), ("nw2-k1-wave1-idle", 1),
                       ("nw8-k8-one-offset-per-wave", 0)):
        s = F.BY_NAME[name]
        owners = {k % s.NW for k in range(s.K)}
        assert s.NW - len(owners) == idle, name


# ---------------------------------------------------------------- reference against the oracle

def test_conv_equals_the_oracle_on_real_tables():
    rng = np.random.default_rng(3)
    shape = (12, 10, 8)
    occ = np.argwhere(rng.random(shape) < 0.25)
    idx = np.concatenate([np.zeros((len(occ), 1), np.int64), occ], 1)
    M = len(idx)
    g = torch.Generator().manual_seed(4)
    X = torch.randn(M, 32, generator=g, dtype=torch.float64)
    # submanifold 3x3x3
    W = torch.randn(3, 3, 3, 32, 64, generator=g, dtype=torch.float64) * 0.05
    pairs = ref.subm_pairs(idx, shape, 3, 1)
    nbr = ref.pairs_to_table(pairs, M)
    WT = W.reshape(27, 32, 64).transpose(1, 2).contiguous()
    want = ref.pairs_conv(X, W, pairs, M)
    assert float((F.conv(X, WT, nbr) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    Wf = W.reshape(27, 32, 64).flip(0).transpose(1, 2).contiguous()          # flip: offset k uses slice K - 1 - k
    assert float((F.conv(X, Wf, nbr, flip=1) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # strided 2x2x2
    W2 = torch.randn(2, 2, 2, 32, 32, generator=g, dtype=torch.float64) * 0.05
    out_idx, _, dpairs = ref.down_pairs(idx, shape, 2, 2, 0)
    Mo = len(out_idx)
    nbr_d = ref.pairs_to_table(dpairs, Mo)
    bias = torch.randn(32, generator=g, dtype=torch.float64)
    want = ref.pairs_conv(X, W2, dpairs, Mo, bias=bias)
    got = F.conv(X, W2.reshape(8, 32, 32).transpose(1, 2).contiguous(), nbr_d, bias=bias)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # ... and its up table (the inverse convolution: the pairs swapped)
    Y = torch.randn(Mo, 32, generator=g, dtype=torch.float64)
    up = ref.inverse_pairs(dpairs)
    want = ref.pairs_conv(Y, W2, up, M)
    got = F.conv(Y, W2.reshape(8, 32, 32).transpose(1, 2).contiguous(), ref.pairs_to_table(up, M))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---------------------------------------------------------------- the checker passes the rounded reference everywhere

@pytest.mark.parametrize("name", [s.name for s in F.MATRIX])
def test_rounded_reference_passes_and_a_dropped_pair_fails(name):
    s = F.BY_NAME[name]
    for v in F.variations(s):
        tab, M_in = F.table_for(s, v)
        nbr = None if tab is None else tab.nbr
        X, WT, bias, residual, _ = F.make_inputs(s, M_in, 5)
        for flip, b, r in ((0, None, None), (1, bias, residual)):
            want = F.conv(X, WT, nbr, flip, b, r, s.M_out)
            res = F.check_conv(want.float(), X, WT, nbr, flip, b, r, extra=s.NW + s.ZS, what=f"{name} {v}", want=want)
            assert res.pairs <= res.all <= 0.125 + 1e-9          # one rounding against 2 gamma_n, n >= 4
            # the removed pair stands 10 bounds out: a kernel result anywhere inside the bound (1 of them) cannot hide it
            assert res.drop > 10.0
            if tab is not None and tab.info["empty_rows"] is not None:
                e = torch.as_tensor(tab.info["empty_rows"])
                zero = torch.zeros_like(want[e])
                assert torch.equal(want[e], (zero if b is None else zero + b.double()) + (zero if r is None else r[e].double()))


# ---------------------------------------------------------------- simulated wrong kernels fail

@pytest.fixture(scope="module")
def sim():
    s = F.BY_NAME["nw4-zs2-k27"]                       # 27 offsets, 4 waves x 2 slabs, 1000 rows (ragged last slice)
    tab, M_in = F.table_for(s, "eq")
    X, WT, bias, residual, buf = F.make_inputs(s, M_in, 6)
    want = F.conv(X, WT, tab.nbr, 1, bias, residual)
    return s, tab, X, WT, bias, residual, buf, want


def _conv_fails(sim, got, match):
    s, tab, X, WT, bias, residual, _, want = sim
    with pytest.raises(AssertionError, match=match):
        F.check_conv(got.float(), X, WT, tab.nbr, 1, bias, residual, extra=s.NW + s.ZS, what="sim", want=want)


def test_the_unharmed_reference_passes(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    F.check_conv(want.float(), X, WT, tab.nbr, 1, bias, residual, extra=s.NW + s.ZS, what="sim", want=want)


def test_a_dropped_pair_fails(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    nbr = tab.nbr.copy()
    k = 13
    r = int(np.flatnonzero(nbr[k] >= 0)[3])            # some pair of a well-populated offset
    nbr[k, r] = -1
    _conv_fails(sim, F.conv(X, WT, nbr, 1, bias, residual), "outside the bound")


def test_offsets_mirrored_with_flip_ignored_fail(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    _conv_fails(sim, F.conv(X, WT, tab.nbr, 0, bias, residual), "outside the bound")


def test_one_waves_offsets_counted_twice_fail(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    P = s.NW * s.ZS
    for wave, z in ((1, 0), (s.NW - 1, s.ZS - 1)):      # k mod (ZS NW) == z + ZS wave
        ks = [k for k in range(s.K) if k % P == z + s.ZS * wave]
        assert ks
        _conv_fails(sim, want + F.conv(X, WT, tab.nbr, 1, ks=ks), "outside the bound")


def test_a_slab_left_out_of_the_sum_fails(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    for z in range(s.ZS):
        ks = [k for k in range(s.K) if k % s.ZS == z]
        _conv_fails(sim, want - F.conv(X, WT, tab.nbr, 1, ks=ks), "outside the bound")


def test_an_unwritten_row_of_the_empty_slice_fails(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    got = want.clone()
    got[int(tab.info["empty_rows"][5])] = float("nan")
    _conv_fails(sim, got, "non-finite")


def test_a_gather_past_the_end_of_x_fails(sim):
    """a missing pair that reads the row behind the last one (instead of the descriptor's zeros) pulls in the NaN rows"""
    s, tab, X, WT, bias, residual, buf, want = sim
    nbr = tab.nbr.copy()
    k, r = np.argwhere(nbr < 0)[17]
    nbr[k, r] = X.shape[0]
    _conv_fails(sim, F.conv(buf, WT, nbr, 1, bias, residual), "non-finite")


def test_statistics_checker_passes_right_and_fails_wrong_partials(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    y = want.float()
    M = s.M_out
    assert M % 32 and tab.order is not None
    for zs in (1, s.ZS):                                # tile order (in-kernel epilogue) / row order (slab reduce)
        rows = F.slice_rows(tab.order, M, zs)
        good = bn_ref.slice_partials(y[rows])
        F.check_stats(good, y, tab.order, zs, "sim")
        # the other path's order
        other = bn_ref.slice_partials(y[F.slice_rows(tab.order, M, 1 if zs > 1 else 2)])
        with pytest.raises(AssertionError, match="sum"):
            F.check_stats(other, y, tab.order, zs, "sim")
        # the ragged slice's squares centred on sum / 32 instead of sum / rows
        blocks, cnt = bn_ref._slices(y[rows].double())
        assert cnt[-1] == M % 32
        live = torch.arange(32) < cnt[-1]
        d = torch.where(live[:, None], blocks[-1] - blocks[-1].sum(0) / 32.0, torch.zeros(()).double())
        bad = good.clone()
        bad[-1, 1] = (d * d).sum(0).float()
        with pytest.raises(AssertionError, match="centred sum of squares"):
            F.check_stats(bad, y, tab.order, zs, "sim")
        # ... and the padded rows counted as rows of value zero
        d = blocks[-1] - blocks[-1].sum(0) / 32.0
        bad[-1, 1] = (d * d).sum(0).float()
        with pytest.raises(AssertionError, match="centred sum of squares"):
            F.check_stats(bad, y, tab.order, zs, "sim")
        # an unwritten partial
        bad = good.clone()
        bad[3, 0, 7] = float("nan")
        with pytest.raises(AssertionError, match="not written"):
            F.check_stats(bad, y, tab.order, zs, "sim")
        # one ulp-scale slip is inside, a slip of 1e-5 of the sum of magnitudes is outside
        bad = good.clone()
        bad[2, 0] += 1e-5 * y[rows][64:96].abs().sum(0)
        with pytest.raises(AssertionError, match="sum"):
            F.check_stats(bad, y, tab.order, zs, "sim")


def test_bn_partials_checker_passes_right_and_fails_the_wrong_order(sim):
    s, tab, X, WT, bias, residual, _, want = sim
    y = want.float()
    bn = F.bn_case(s.M_out, s.Cout, 9)
    z = bn_ref.pre_activation(bn.x, bn.mean, bn.var, bn.gamma, bn.beta, bn.eps)
    assert float(z.abs().min()) >= bn_ref.MARGIN * (1 - 1e-9) and bool((z > 0).any()) and bool((z < 0).any())
    for relu in (1, 0):
        for zs in (1, s.ZS):
            rows = F.slice_rows(tab.order, s.M_out, zs)
            good = bn_ref.bwd_slice_partials(bn.x[rows], y[rows], bn.mean, bn.var, bn.gamma, bn.beta, bn.eps, relu)
            assert F.check_bn_partials(good, y, bn, relu, tab.order, zs, "sim") <= 1e-3
            with pytest.raises(AssertionError, match="sum dz"):
                F.check_bn_partials(good, y, bn, relu, tab.order, 1 if zs > 1 else 2, "sim")
            if relu:                                                 # the ReLU mask ignored
                open_mask = bn_ref.bwd_slice_partials(bn.x[rows], y[rows], bn.mean, bn.var, bn.gamma, bn.beta, bn.eps, 0)
                with pytest.raises(AssertionError, match="sum dz"):
                    F.check_bn_partials(open_mask, y, bn, 1, tab.order, zs, "sim")
