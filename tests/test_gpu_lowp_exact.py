"""GPU: the 16-bit sparse convolutions (csrc/spconv_lp.hip) bit-exactly at every launch branch.

Operands are integers times powers of two, sized so that every fp32 partial sum is exact (tests/lowp_exact.py): the
forward / dIn output must equal the round-to-nearest-even of the fp64 reference and dW its fp32 cast, on all elements.
Each case asserts the launch plan it reaches through wsis_spconv_lp_plan (forward NT = 1 / 2; dW chunks 1, 2, 64 and
workspace-capped, 1-4 waves, more than one tile group, LDS above 64 KiB).  Every call runs on poisoned buffers: outputs,
dW and the workspace prefilled with NaN, X rows that no pair reads and dY rows of outputs without pairs set to NaN, X and
dY passed as views into buffers with NaN rows after the last valid one.  Each case runs twice and must repeat its bits."""
import numpy as np
import pytest
import torch

import harness
import spconv
import wsis_native as _n
from oracle import spconv_ref as ref
from spconv import ops
from util import random_sparse_coords

import conv_ref
import lowp_exact as lx
from lowp_exact import lp_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
CODE = {torch.bfloat16: 0, torch.float16: 1}
NAN = float("nan")
PAD_ROWS = 37           # NaN rows after the last valid row of X and dY
XE, WE = -4, -5         # operand grains 2^-4 and 2^-5: outputs stay below 2^24 * 2^-9 = 32768 (fp16 range)
GRAIN = 2.0 ** (XE + WE)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _range(budget, terms, cap=64):
    """largest R with terms * R^2 <= budget (two operands in [-R, R]), at most cap"""
    return max(1, min(cap, int((budget / max(terms, 1)) ** 0.5)))


def _padded(vals, dt, nan_rows=None):
    """``vals`` (fp32) as a dt view of the first rows of a buffer with PAD_ROWS NaN rows after them; rows ``nan_rows``
    of the view set to NaN too"""
    buf = torch.full((vals.shape[0] + PAD_ROWS, vals.shape[1]), NAN, dtype=dt, device=DEV)
    buf[:vals.shape[0]] = vals.to(dt)
    view = buf[:vals.shape[0]]
    if nan_rows is not None:
        view[nan_rows] = NAN
    return view


def _table(M_in, M_out, K, gen, live=None):
    """[K, M_out] packed table (rows = tile positions, -1 = no pair) whose 32-row tiles follow six patterns: all
    offsets dense, one offset missing, the last offset missing, only the last offset, no offset at all (bias-only
    output), all offsets sparse.  ``live``: offsets that may carry pairs (the others are empty)."""
    t = torch.arange(M_out)
    tile = t // 32
    pat = tile % 6
    dens = torch.where(pat == 5, 0.1, 0.7)
    src = torch.randint(0, M_in, (K, M_out), generator=gen)
    take = torch.rand(K, M_out, generator=gen) < dens
    k = torch.arange(K)[:, None]
    take &= ~((pat == 1) & (k == (tile // 6) % K))
    take &= ~((pat == 2) & (k == K - 1))
    take &= ~((pat == 3) & (k != K - 1))
    take &= pat != 4
    if live is not None:
        take &= torch.isin(k, torch.as_tensor(live)).expand(K, M_out)
    return torch.where(take, src, torch.full_like(src, -1)).int()


def _pairs(nbr, order, M_out):
    """device pair lists (pi, po) of a packed table (po through ``order`` when given)"""
    pairs = []
    for k in range(nbr.shape[0]):
        t = torch.nonzero(nbr[k] >= 0).flatten()
        po = order.long()[t] if order is not None else t
        pairs.append((nbr[k, t].long(), po))
    return pairs


def _ws(nbytes):
    return torch.full((max(nbytes, 256) // 4 + 1,), NAN, dtype=torch.float32, device=DEV)


def _fwd(X, nbr, order, WT, flip, bias, M_out, dt):
    K, Cout, Cin = WT.shape
    out = torch.full((M_out, Cout), NAN, dtype=dt, device=DEV)
    lib = _n.hip()
    wsb = lib.wsis_spconv_fwd_lp_workspace_bytes(M_out, K, Cin, Cout)
    ws = _ws(wsb)
    _n.check(lib.wsis_spconv_fwd_lp(_n.ptr(X), _n.ptr(nbr), _n.ptr(order), _n.ptr(WT), flip, _n.ptr(bias), _n.ptr(out),
                                    X.shape[0], M_out, K, Cin, Cout, CODE[dt], _n.ptr(ws), wsb, _n.stream_ptr()),
             "spconv_fwd_lp")
    torch.cuda.synchronize()
    return out


def _dw(X, nbr, order, dY, K, dt):
    M_out, Cout = dY.shape
    Cin = X.shape[1]
    dW = torch.full((K, Cin, Cout), NAN, dtype=torch.float32, device=DEV)
    lib = _n.hip()
    wsb = lib.wsis_spconv_dw_lp_workspace_bytes(M_out, K, Cin, Cout)
    ws = _ws(wsb)
    _n.check(lib.wsis_spconv_dw_lp(_n.ptr(X), _n.ptr(nbr), _n.ptr(order), _n.ptr(dY), _n.ptr(dW), X.shape[0], M_out, K,
                                   Cin, Cout, CODE[dt], _n.ptr(ws), wsb, _n.stream_ptr()), "spconv_dw_lp")
    torch.cuda.synchronize()
    return dW


# ---- forward / dIn through the C ABI -------------------------------------------------------------------------------

# id: (M_out, K, Cin, Cout, flip, table (False: nbr = NULL, the dense 1x1 form), order, bias, NT)
FWD = {
    "nt1_m131040_c64": (131040, 8, 32, 64, 0, True, True, True, 1),
    "nt2_m131041_c64": (131041, 8, 32, 64, 1, True, False, True, 2),
    "nt1_m65504_c128": (65504, 1, 96, 128, 0, True, True, False, 1),
    "nt2_m65505_c128_dense": (65505, 1, 64, 128, 0, False, False, True, 2),
    "nt1_m16352_c512": (16352, 27, 32, 512, 1, True, True, True, 1),
    "nt2_m16353_cin480_c512": (16353, 27, 480, 512, 0, True, True, True, 2),
    "nt2_m50017_cin512_c512": (50017, 8, 512, 512, 1, True, False, True, 2),
    "m1_k27_flip": (1, 27, 32, 32, 1, True, True, True, 1),
    "m31_k8": (31, 8, 64, 96, 0, True, False, False, 1),
    "m33_dense_order": (33, 1, 96, 64, 0, False, True, True, 1),
    "m127_cin512": (127, 27, 512, 32, 0, True, True, True, 1),
    "m129_cin480_flip": (129, 8, 480, 160, 1, True, False, True, 1),
    "m4001_k27_flip": (4001, 27, 96, 96, 1, True, True, True, 1),
    "m3001_k1_table": (3001, 1, 64, 32, 0, True, True, True, 1),
}


def _fwd_case(name, dt, seed):
    M_out, K, Cin, Cout, flip, table, use_order, use_bias, nt = FWD[name]
    p = lp_plan(M_out, K, Cin, Cout)
    assert p["nt"] == nt, (name, p)
    gen = torch.Generator().manual_seed(seed)
    gd = torch.Generator(device=DEV).manual_seed(seed)
    M_in = M_out if not table else M_out + M_out // 3 + 7
    order = torch.randperm(M_out, generator=gen).int().to(DEV) if use_order else None
    R = _range(2.0 ** 23, K * Cin)
    xv = lx.ints((M_in, Cin), R, XE, gd)
    WT = lx.ints((K, Cout, Cin), R, WE, gd).to(dt)
    bias = lx.ints((Cout,), 1 << 15, XE + WE, gd) if use_bias else None
    if table:
        nbr = _table(M_in, M_out, K, gen).to(DEV)
        used = torch.zeros(M_in, dtype=torch.bool, device=DEV)
        used[nbr[nbr >= 0].long()] = True
        X = _padded(xv, dt, ~used)
        pairs = _pairs(nbr, order, M_out)
    else:
        nbr = None
        X = _padded(xv, dt)
        t = torch.arange(M_out, device=DEV)
        pairs = [(t, order.long() if order is not None else t)]
    Wref = (WT.flip(0) if flip else WT).transpose(1, 2)       # offset k pairs with slice K-1-k when flip
    big = M_out >= 1000
    exp = lx.expect_rows(X, Wref, pairs, M_out, dt, GRAIN, bias=bias, min_round=0.1 if big else 0.0,
                         min_ties=1 if big else 0, what=f"{name} {dt}")
    got = _fwd(X, nbr, order, WT, flip, bias, M_out, dt)
    assert torch.equal(got, exp), _mismatch(got, exp, f"{name} {dt}")
    again = _fwd(X, nbr, order, WT, flip, bias, M_out, dt)
    assert _same_bits(got, again), f"{name} {dt}: a rerun changed bits"
    if table:
        # outputs of tiles without any pair: exactly the rounded bias (or zero)
        rows = torch.nonzero((nbr < 0).all(0)).flatten()
        assert rows.numel() > 0 or M_out < 5 * 32
        orow = order.long()[rows] if order is not None else rows
        want = (bias.to(dt) if bias is not None else torch.zeros(Cout, dtype=dt, device=DEV)).expand(len(rows), Cout)
        assert torch.equal(got[orow], want), f"{name} {dt}: pair-less rows are not the rounded bias"


def _mismatch(got, exp, what):
    bad = torch.nonzero(got != exp)
    n = bad.shape[0]
    if n == 0:
        return f"{what}: NaN in the output"
    r, c = (int(v) for v in bad[0])
    return f"{what}: {n} elements differ, first [{r}, {c}] got {float(got[r, c])!r} want {float(exp[r, c])!r}"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(FWD))
def test_fwd_exact(name, dt):
    _fwd_case(name, dt, seed=sorted(FWD).index(name))


# ---- weight gradient through the C ABI ---------------------------------------------------------------------------

# id: (M_out, K, Cin, Cout, live offsets (None: all), table (False: nbr = NULL), order, expected plan values)
DW = {
    "chunks1_m2048": (2048, 8, 32, 32, None, True, True, dict(chunks=1, nw=1, groups=1)),
    "chunks2_m2049": (2049, 8, 64, 32, None, True, False, dict(chunks=2, nw=2, groups=1)),
    "chunks64_tail1": (129025, 2, 96, 32, None, True, True, dict(chunks=64, rows_per_chunk=2048, nw=3)),
    "chunks64_cap_dense": (200_000, 1, 160, 96, None, False, False, dict(chunks=64, nw=4, groups=1)),
    "groups2_partial": (3000, 27, 160, 128, None, True, True, dict(chunks=2, nw=4, groups=2)),
    "wscap_k27_c512": (20_000, 27, 512, 512, (0, 13, 26), True, True, dict(chunks=9, groups=16, lds=81920)),
    "wscap_k125_c512": (5000, 125, 512, 512, (0, 62, 124), True, False, dict(chunks=2, groups=16, lds=81920)),
    "lds_512x320": (700, 8, 512, 320, None, True, True, dict(chunks=1, groups=10, lds=66560)),
}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(DW))
def test_dw_exact(name, dt):
    M_out, K, Cin, Cout, live, table, use_order, plan = DW[name]
    p = lp_plan(M_out, K, Cin, Cout)
    assert {k: p[k] for k in plan} == plan, (name, p)
    seed = 100 + sorted(DW).index(name)
    gen = torch.Generator().manual_seed(seed)
    gd = torch.Generator(device=DEV).manual_seed(seed)
    M_in = M_out if not table else M_out + M_out // 5 + 3
    order = torch.randperm(M_out, generator=gen).int().to(DEV) if use_order else None
    if table:
        nbr = _table(M_in, M_out, K, gen, live).to(DEV)
        pairs = _pairs(nbr, order, M_out)
        used = torch.zeros(M_in, dtype=torch.bool, device=DEV)
        used[nbr[nbr >= 0].long()] = True
        paired = torch.zeros(M_out, dtype=torch.bool, device=DEV)
        paired[torch.cat([po for _, po in pairs])] = True
    else:
        nbr = None
        t = torch.arange(M_out, device=DEV)
        pairs = [(t, t)]
        used = paired = torch.ones(M_out, dtype=torch.bool, device=DEV)
    most = max(len(pi) for pi, _ in pairs)
    R = _range(2.0 ** 23, most)
    X = _padded(lx.ints((M_in, Cin), R, XE, gd), dt, ~used)
    dY = _padded(lx.ints((M_out, Cout), R, WE, gd), dt, ~paired)
    exp = lx.expect_dw(X, dY, pairs, GRAIN, what=f"{name} {dt}")
    got = _dw(X, nbr, order, dY, K, dt)
    assert torch.equal(got, exp), f"{name} {dt}: {int((got != exp).sum())} of {got.numel()} dW elements differ"
    if live is not None:
        dead = [k for k in range(K) if k not in live]
        assert int((got[dead] != 0).sum()) == 0, f"{name} {dt}: offsets without pairs are not exact zeros"
    again = _dw(X, nbr, order, dY, K, dt)
    assert _same_bits(got, again), f"{name} {dt}: a rerun changed bits"


# ---- weight cast ---------------------------------------------------------------------------------------------------

def _special_weights(K, Cin, Cout, gen):
    """fp32 weights with bf16 / fp16 ties of both parities, fp16 overflow and subnormals, +-0, +-inf and NaN"""
    n = K * Cin * Cout
    w = torch.randn(n, generator=gen)
    hi = torch.randint(0, 1 << 15, (64,), generator=gen, dtype=torch.int32)
    bf_ties = ((hi << 16) | 0x8000).view(torch.float32)                 # 64 bf16 ties, random parities
    bf_ties = torch.cat([bf_ties, ((hi & ~1) << 16 | 0x8000).view(torch.float32),
                         ((hi | 1) << 16 | 0x8000).view(torch.float32)])
    e = torch.randint(-14, 15, (64,), generator=gen).float()
    m = torch.randint(0, 1 << 10, (64,), generator=gen).float()
    f16_tie = (1 + (m + 0.5) / 1024) * torch.pow(2.0, e)                # halfway between two fp16 normals
    f16_sub = torch.randint(1, 1 << 11, (64,), generator=gen).float() * 2.0 ** -25     # subnormal grid / 2: ties too
    edges = torch.tensor([65504.0, 65519.99, 65520.0, 65536.0, 1e5, 3e38, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                          2.0 ** -26, 1e-8, 6e-5, 0.0, float("inf"), NAN, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    edges = torch.cat([edges, -edges])
    special = torch.cat([bf_ties, f16_tie, -f16_tie, f16_sub, -f16_sub, edges])
    pos = torch.randperm(n, generator=gen)[:special.numel()]
    w[pos] = special
    return w.view(K, Cin, Cout)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", (1, 8, 27))
def test_weight_cast_exact(K, dt):
    Cin, Cout = 48, 40
    W = _special_weights(K, Cin, Cout, torch.Generator().manual_seed(K)).to(DEV)
    for transpose in (0, 1):
        for flip in (0, 1):
            out = torch.full((K, Cout, Cin) if transpose else (K, Cin, Cout), NAN, dtype=dt, device=DEV)
            _n.check(_n.hip().wsis_weight_cast_lp(_n.ptr(W), _n.ptr(out), K, Cin, Cout, transpose, flip, CODE[dt],
                                                  _n.stream_ptr()), "weight_cast_lp")
            want = W.flip(0) if flip else W
            want = (want.permute(0, 2, 1) if transpose else want).contiguous().to(dt)
            what = f"K={K} transpose={transpose} flip={flip} {dt}"
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(out), nan), what + ": NaN positions"
            assert torch.equal(_bits(out)[~nan], _bits(want)[~nan]), what + ": bit patterns"
    if dt == torch.float16:
        assert bool(torch.isinf(out).any()) and bool(((out != 0) & (out.abs() < 2.0 ** -14)).any())


# ---- fp16 overflow and subnormal outputs -------------------------------------------------------------------------

def test_fp16_overflow_and_subnormal_outputs():
    dt = torch.float16
    M, Cin, Cout = 64, 32, 32
    # overflow: out[r, c] = s_r (65504 + t_r delta_c), s_r = +-1, t_r = +-1
    delta = torch.tensor([0, 0.5, 1, 7.5, 15.5, 15.75, 15.875, 15.9375, 16, 16.5, 17, 32, 100, 1000, 2.0 ** 15, 65504]
                         * 2)[:Cout]
    s = torch.tensor([1.0, -1.0]).repeat(M // 2)
    t = torch.tensor([1.0, 1.0, -1.0, -1.0]).repeat(M // 4)
    X = torch.zeros(M, Cin)
    X[:, 0], X[:, 1] = 65504 * s, s * t
    W = torch.zeros(1, Cin, Cout)
    W[0, 0], W[0, 1] = 1.0, delta
    want = X.double() @ W[0].double()
    exp = want.float().to(dt)
    assert bool((exp == 65504).any()) and bool((exp == -65504).any())
    assert bool((exp == float("inf")).any()) and bool((exp == float("-inf")).any())
    assert bool(((want.abs() >= 65504) & (want.abs() < 65520) & (want.abs() > 65504)).any())
    got = _fwd(_padded(X.to(DEV), dt), None, None, W.transpose(1, 2).contiguous().to(DEV).to(dt), 0, None, M, dt)
    assert torch.equal(got, exp.to(DEV)), _mismatch(got.cpu(), exp, "fp16 overflow")
    # subnormals: out = 2^-25 odd_r odd_c + 2^-24 m, an odd multiple of 2^-25: every value a tie between two subnormals
    g = torch.Generator().manual_seed(9)
    X = torch.zeros(M, Cin)
    W = torch.zeros(1, Cin, Cout)
    X[:, 0] = (2 * torch.randint(0, 23, (M,), generator=g) + 1).float() * 2.0 ** -12
    W[0, 0] = (2 * torch.randint(0, 23, (Cout,), generator=g) + 1).float() * 2.0 ** -13
    X[:, 1] = torch.randint(-3, 4, (M,), generator=g).float() * 2.0 ** -12
    W[0, 1] = torch.randint(-3, 4, (Cout,), generator=g).float() * 2.0 ** -12
    want = X.double() @ W[0].double()
    assert float(want.abs().max()) < 2.0 ** -14
    exp = want.float().to(dt)
    _, tie = lx.rounding(want, dt)
    assert int(tie.sum()) > M * Cout // 4 and bool(((exp != 0) & (exp.abs() < 2.0 ** -14)).any())
    got = _fwd(_padded(X.to(DEV), dt), None, None, W.transpose(1, 2).contiguous().to(DEV).to(dt), 0, None, M, dt)
    assert torch.equal(got, exp.to(DEV)), _mismatch(got.cpu(), exp, "fp16 subnormals")


# ---- real tables: a batch whose level 1 takes NT = 2 -----------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_levels():
    """levels 0 and 1 of a five-scene batch with the rulebooks of the C2 fixture (subm k3, down k2 s2)"""
    b = harness.collate([harness.make_scene(s) for s in (1, 2, 3, 4, 5)])
    idx0 = b["voxel_locs"].int().to(DEV).contiguous()
    shape0 = [int(s) for s in b["spatial_shape"]]
    down = ops.build_down_rulebook(idx0, shape0, [2] * 3, [2] * 3, [0] * 3)
    _, _, down_pairs = ref.down_pairs_fast(idx0.cpu().numpy(), shape0, 2, 2, 0)
    idx1, shape1 = down.out_indices, down.out_shape
    subm = ops.build_subm_rulebook(idx1, shape1, [3] * 3, [1] * 3)
    subm_pairs = ref.subm_pairs_fast(idx1.cpu().numpy(), shape1, 3, 1)
    return dict(M0=idx0.shape[0], M1=idx1.shape[0], down=down, subm=subm,
                down_pairs=conv_ref.device_pairs(down_pairs, DEV), subm_pairs=conv_ref.device_pairs(subm_pairs, DEV))


def _ops_exact(X, W, nf, of, nb, ob, flip, M_out, pairs, dt, seed, what):
    """forward, dIn and dW of ops.sparse_conv against the exact oracle, and a bit-identical rerun"""
    K, Cin, Cout = W.shape
    gd = torch.Generator(device=DEV).manual_seed(seed)
    dY = lx.ints((M_out, Cout), 6, XE, gd).to(dt)
    res = []
    for _ in range(2):
        xg = X.clone().requires_grad_(True)
        w = W.view(K, 1, 1, Cin, Cout).clone().requires_grad_(True)
        out = ops.sparse_conv(xg, w, None, nf, of, nb, ob, flip, M_out)
        out.backward(dY)
        res.append((out.detach(), xg.grad, w.grad.view(K, Cin, Cout)))
    out, dX, dW = res[0]
    for a, b in zip(res[0], res[1]):
        assert _same_bits(a, b), what + ": a rerun changed bits"
    exp = lx.expect_rows(X, W, pairs, M_out, dt, GRAIN, what=what + " forward")
    assert torch.equal(out, exp), _mismatch(out, exp, what + " forward")
    exp = lx.expect_rows(dY, W.transpose(1, 2), conv_ref.swap(pairs), X.shape[0], dt, 2.0 ** (XE + WE),
                         what=what + " dIn")
    assert torch.equal(dX, exp), _mismatch(dX, exp, what + " dIn")
    exp = lx.expect_dw(X, dY, pairs, 2.0 ** (2 * XE), what=what + " dW")
    assert torch.equal(dW, exp), f"{what} dW: {int((dW != exp).sum())} elements differ"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_batch_level1_subm_nt2(batch_levels, dt):
    L = batch_levels
    M1 = L["M1"]
    assert M1 >= 131041, f"level 1 has {M1} rows: too few for NT = 2 at 64 channels"
    assert lp_plan(M1, 27, 64, 64)["nt"] == 2 and lp_plan(M1, 27, 64, 64)["chunks"] == 64
    gd = torch.Generator(device=DEV).manual_seed(1)
    X = lx.ints((M1, 64), 8, XE, gd).to(dt)
    W = lx.ints((27, 64, 64), 100, WE, gd)
    s = L["subm"]
    _ops_exact(X, W, s.nbr_p, s.order, s.nbr_p, s.order, 1, M1, L["subm_pairs"], dt, 2, f"level-1 subm 64->64 {dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_batch_down_and_inverse(batch_levels, dt):
    L = batch_levels
    M0, M1, d = L["M0"], L["M1"], L["down"]
    assert lp_plan(M1, 8, 32, 64)["nt"] == 2 and lp_plan(M0, 8, 64, 32)["nt"] == 1
    gd = torch.Generator(device=DEV).manual_seed(3)
    X0 = lx.ints((M0, 32), 8, XE, gd).to(dt)
    W = lx.ints((8, 32, 64), 100, WE, gd)
    _ops_exact(X0, W, d.nbr_p, d.order, d.nbr_up_p, d.order_up, 0, M1, L["down_pairs"], dt, 4,
               f"level 0->1 down 32->64 {dt}")
    X1 = lx.ints((M1, 64), 8, XE, gd).to(dt)
    W = lx.ints((8, 64, 32), 100, WE, gd)
    _ops_exact(X1, W, d.nbr_up_p, d.order_up, d.nbr_p, d.order, 0, M0, conv_ref.swap(L["down_pairs"]), dt, 5,
               f"level 1->0 inverse 64->32 {dt}")


# ---- module level ------------------------------------------------------------------------------------------------

def test_subm_512_autocast_bf16():
    dt = torch.bfloat16
    shape = (12, 11, 10)
    coords = random_sparse_coords(21, batch=2, shape=shape, density=0.3)
    idx = np.asarray(coords)
    M = idx.shape[0]
    assert lp_plan(M, 27, 512, 512)["lds"] > 65536
    gd = torch.Generator(device=DEV).manual_seed(21)
    conv = spconv.SubMConv3d(512, 512, 3, padding=1, bias=True, indice_key="x512").to(DEV)
    with torch.no_grad():
        conv.weight.copy_(lx.ints(tuple(conv.weight.shape), 100, WE, gd))
        conv.bias.copy_(lx.ints((512,), 1 << 15, XE + WE, gd))
    x = lx.ints((M, 512), 6, XE, gd).requires_grad_(True)
    dY = lx.ints((M, 512), 6, XE, gd).to(dt)
    t = spconv.SparseConvTensor(x, torch.from_numpy(idx.astype(np.int32)).to(DEV), np.array(shape), 2)
    with torch.autocast("cuda", dtype=dt):
        out = conv(t).features
    assert out.dtype == dt
    out.backward(dY)
    pairs = conv_ref.device_pairs(ref.subm_pairs_fast(idx, shape, 3, 1), DEV)
    W = conv.weight.detach().view(27, 512, 512)
    exp = lx.expect_rows(x.detach(), W, pairs, M, dt, GRAIN, bias=conv.bias.detach(), what="SubM 512 forward")
    assert torch.equal(out.detach(), exp), _mismatch(out.detach(), exp, "SubM 512 forward")
    exp = lx.expect_rows(dY, W.transpose(1, 2), conv_ref.swap(pairs), M, dt, GRAIN, what="SubM 512 dIn")
    assert x.grad.dtype == torch.float32
    assert torch.equal(x.grad, exp.float()), _mismatch(x.grad, exp.float(), "SubM 512 dIn")
    exp = lx.expect_dw(x.detach(), dY, pairs, 2.0 ** (2 * XE), what="SubM 512 dW")
    assert torch.equal(conv.weight.grad.view(27, 512, 512), exp), "SubM 512 dW"
    assert torch.equal(conv.bias.grad.double(), dY.double().sum(0)), "SubM 512 bias gradient"


# ---- misaligned and refused inputs -------------------------------------------------------------------------------

def _misaligned(vals, dt):
    """a contiguous dt tensor equal to ``vals`` whose data_ptr is 8 bytes past a 16-byte boundary"""
    buf = torch.empty(vals.numel() + 8, dtype=dt, device=DEV)
    off = ((8 - buf.data_ptr() % 16) % 16) // 2
    t = buf[off:off + vals.numel()].view(vals.shape)
    t.copy_(vals)
    assert t.is_contiguous() and t.data_ptr() % 16 == 8
    return t


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_misaligned_features_through_ops(dt):
    shape = (12, 11, 10)
    coords = random_sparse_coords(8, batch=2, shape=shape, density=0.3)
    ind = torch.from_numpy(coords).to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(8)
    conv = spconv.SubMConv3d(32, 64, 3, padding=1, bias=True, indice_key="mis").to(DEV)
    with torch.no_grad():
        conv.weight.copy_(lx.ints(tuple(conv.weight.shape), 60, WE, gd))
    xv = lx.ints((len(coords), 32), 8, XE, gd).to(dt)
    dYv = lx.ints((len(coords), 64), 8, XE, gd).to(dt)
    res = []
    for x, dY in ((xv.clone(), dYv.clone()), (_misaligned(xv, dt), _misaligned(dYv, dt))):
        conv.zero_grad(set_to_none=True)
        x.requires_grad_(True)
        out = conv(spconv.SparseConvTensor(x, ind, np.array(shape), 2)).features
        out.backward(dY)
        res.append((out.detach(), x.grad, conv.weight.grad))
    for a, b in zip(*res):
        assert _same_bits(a, b), "a misaligned input changed the result"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_refuses_misaligned_pointer_and_short_workspace(dt):
    lib = _n.hip()
    K, Cin, Cout, M = 8, 32, 32, 4100
    gd = torch.Generator(device=DEV).manual_seed(12)
    X = lx.ints((M + 8, Cin), 8, XE, gd).to(dt)
    WT = lx.ints((K, Cout, Cin), 8, WE, gd).to(dt)
    nbr = torch.randint(-1, M, (K, M), generator=torch.Generator().manual_seed(12)).int().to(DEV)
    out = torch.full((M, Cout), NAN, dtype=dt, device=DEV)
    rc = lib.wsis_spconv_fwd_lp(X.data_ptr() + 8, _n.ptr(nbr), None, _n.ptr(WT), 0, None, _n.ptr(out), M, M, K, Cin,
                                Cout, CODE[dt], None, 256, _n.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and "align" in lib.wsis_last_error().decode()
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"
    dY = lx.ints((M, Cout), 8, XE, gd).to(dt)
    dW = torch.full((K, Cin, Cout), NAN, dtype=torch.float32, device=DEV)
    for xp, dyp in ((X.data_ptr() + 8, dY.data_ptr()), (X.data_ptr(), dY.data_ptr() + 8)):
        rc = lib.wsis_spconv_dw_lp(xp, _n.ptr(nbr), None, dyp, _n.ptr(dW), M, M, K, Cin, Cout, CODE[dt], None, 0,
                                   _n.stream_ptr())
        assert rc != 0 and "align" in lib.wsis_last_error().decode()
    wsb = lib.wsis_spconv_dw_lp_workspace_bytes(M, K, Cin, Cout)
    assert lp_plan(M, K, Cin, Cout)["chunks"] == 3 and wsb > 256
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.wsis_spconv_dw_lp(_n.ptr(X), _n.ptr(nbr), None, _n.ptr(dY), _n.ptr(dW), M, M, K, Cin, Cout, CODE[dt],
                               _n.ptr(ws), wsb - 1, _n.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and "workspace" in lib.wsis_last_error().decode()
    assert bool(torch.isnan(dW).all()), "a refused call wrote dW"
