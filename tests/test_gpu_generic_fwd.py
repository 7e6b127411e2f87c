"""GPU: the generic fp32 forward spconv_fwd_kernel and its slab sums spconv_reduce_kernel / spconv_reduce4_kernel
(csrc/spconv.hip) against fp64 at every launch branch, through wsis_spconv_fwd directly.  This kernel is the only forward
for widths that are not multiples of 32, for K > 32 and for gathered tensors of 2 GiB and more, what WSIS_FWD2=0 and
WSIS_IN_CONV=0 select, and the baseline tests/test_gpu_in_conv.py compares the input convolution with.

Launch rules (fwd_nb, fwd_ksplit and the entry point, restated in ``plan_ref`` below and held to
wsis_spconv_fwd_workspace_bytes = ks M_out Cout 4 + 256, or 256 without a split): a workgroup owns a tile of 128 rows x NB
32-column blocks; NB = blocks of Cout up to 5, else 4 (grid.y column groups), and 1 at 100 tiles or fewer; below 512
workgroups the offsets are split over grid.z: ks = min(K, ceil(1024 / workgroups)), k_per = ceil(K / ks) offsets per z
block, kz = ceil(K / k_per) blocks, each writing a partial slab the reduce kernel adds in z order; a z block walks its
offsets in table groups of 16.

Cases (CASES; ks, k_per, kz, NB, grid.y and the tile count of each are DERIVED from plan_ref and asserted -- the rule gives
every case the branch its row count was chosen for): 2 tiles at one offset per z block; k_per = 2 with a short last
block; k_per = 7 (7, 7, 7, 6); no split at K = 27 (one block walks groups of 16 + 11); K = 125 split with 16 + 5 inside a z
block; NB = 2 .. 5; NB = 4 with a second, partial column group (72 columns); the scalar loads and the scalar reduce (33 ->
70); the 6 -> 32 product under WSIS_IN_CONV=0; an X one float into its storage (VEC4 off at 32 -> 32); the dense 1x1
without a table.  Each on a synthetic table (fwd2_ref.make_table) at M_in == M_out and M_in = 2 M_out + 5; from 5,000 rows
on the table is thinned (in_conv_ref.thin) to about 40 slices with pairs, with a whole 128-row tile of them, tiles
without any pair (``if (tile_mask == 0u) continue;`` -- under a split such a tile still writes zeros to its slab) and tiles
with pairs in one of their four slices only -- asserted.  X is followed by 64 rows of NaN; the output starts as NaN and is
followed by 64 rows of NaN that must stay NaN; the workspace starts as 0xFF.

Asserted per case for bias x residual in {none, given}: fwd2_ref.check_conv with extra = kz (finite, per-element bound
2 gamma_n S, the reference without one pair outside it); rows without a pair == bias + residual exactly; two launches give
the same bits; every row has the same bits without a tile order and under two permutations (the header's "independent of
the tile order": a row's value is one offset-ordered chain per z block, the blocks added in z order).  Whole file: 5 s.

Measured on an MI355X (2026-10-21), all tests passing.  Largest error / bound over every element ("all") and over the rows
with pairs ("pairs"), smallest ratio by which the one-pair-removed reference stood outside the bound ("drop"):
  case group                                             all     pairs   drop
  full split, one offset per z block (2 tiles, 129 rows)  0.027   0.027   1.5e2
  k_per = 2 | k_per = 7 (thinned, empty tiles)           0.032 | 0.083   0.032 | 0.043   1.2e3 | 2.9e2
  no split, K = 27, groups of 16 + 11                    0.167   0.042   2.3e2
  K = 125, k_per = 21, groups of 16 + 5                  0.063   0.041   1.2e2
  NB = 2 | 3 | 4 | 5                                     0.045   0.036 | 0.040 | 0.034 | 0.037   >= 2.0e2
  NB = 4, two column groups (128 + 72)                   0.063   0.044   3.5e2
  scalar loads and scalar reduce (33 -> 70)              0.026   0.026   2.2e2
  6 -> 32 under WSIS_IN_CONV=0                           0.035   0.035   1.6e3
  X one float into its storage (32 -> 32)                0.028   0.028   2.2e2
  dense 1x1 without a table                              0.028   0.028   4.4e4
No ratio is near 1 (nothing here questions the factor 2) and a dropped pair stands more than 100 bounds out.  The larger
"all" figures (0.167 = 1 / 6 without a split, 0.083 = 1 / 12 at kz = 4, ...) are rows without a pair that hold bias +
residual alone: one rounding against 2 gamma_{2 + kz}.  The tile-order equality holds at every plan, split or not.

Out of scope: WSIS_CONV_MATH=1 / 2 (split-bf16 products; tests/test_gpu_ops.py holds their tolerance)."""
import collections

import numpy as np
import pytest
import torch

import fwd2_ref as F
import in_conv_ref as I
import wsis_native as _n

pytestmark = pytest.mark.gpu
DEV = "cuda"
TM, KG = 128, 16

Case = collections.namedtuple("Case", "name K Cin Cout M_out tiles NB gy ks k_per kz reduce note")

# the branch each case is named for: tiles, NB, grid.y, ks, k_per, kz (all re-derived by plan_ref and compared), reduce
# kernel ("4" vector, "1" scalar, None no split)
CASES = (
    Case("one-tile-full-split", 27, 32, 32, 129, 2, 1, 1, 27, 1, 27, "4", "second tile with one row; one offset per z block"),
    Case("split-kper2", 27, 32, 32, 5000, 40, 1, 1, 26, 2, 14, "4", "last z block one offset"),
    Case("split-kper7", 27, 32, 32, 38300, 300, 1, 1, 4, 7, 4, "4", "z blocks of 7, 7, 7, 6"),
    Case("no-split-k27", 27, 32, 32, 65600, 513, 1, 1, 1, 27, 1, None, "one block walks table groups of 16 + 11"),
    Case("split-two-groups", 125, 32, 32, 25500, 200, 1, 1, 6, 21, 6, "4", "groups of 16 + 5 inside a z block"),
    Case("nb2", 27, 32, 64, 12900, 101, 2, 1, 11, 3, 9, "4", "NB = 2"),
    Case("nb3", 27, 32, 96, 12900, 101, 3, 1, 11, 3, 9, "4", "NB = 3"),
    Case("nb4", 27, 32, 128, 12900, 101, 4, 1, 11, 3, 9, "4", "NB = 4"),
    Case("nb5", 27, 32, 160, 12900, 101, 5, 1, 11, 3, 9, "4", "NB = 5"),
    Case("nb4-two-groups", 27, 32, 200, 12900, 101, 4, 2, 6, 5, 6, "4", "second column group of 72 columns"),
    Case("scalar-loads", 27, 33, 70, 300, 3, 1, 3, 27, 1, 27, "1", "VEC4 off, Cin tail of 1, Cout tail of 6, scalar reduce"),
    Case("cin6-generic", 27, 6, 32, 300, 3, 1, 1, 27, 1, 27, "4", "WSIS_IN_CONV=0"),
    Case("unaligned-x", 27, 32, 32, 300, 3, 1, 1, 27, 1, 27, "4", "X one float into its storage: VEC4 off"),
    Case("null-table", 1, 64, 32, 300, 3, 1, 1, 1, 1, 1, None, "dense 1x1 without a table"),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)
THIN_FROM = 5000

Plan = collections.namedtuple("Plan", "tiles NB gy ks k_per kz")


def plan_ref(M_out, K, Cout):
    """fwd_nb + fwd_ksplit + the grid of wsis_spconv_fwd (csrc/spconv.hip) with the default build's constants: one block
    per workgroup at 100 tiles or fewer, 1024 workgroups aimed for, no split from 512 on"""
    tiles, nblk = -(-M_out // TM), -(-Cout // 32)
    NB = nblk if nblk <= 5 else 4
    if tiles <= 100 and NB > 1:
        NB = 1
    gy = -(-Cout // (NB * 32))
    wgs = tiles * gy
    ks = 1 if (wgs >= 512 or K == 1) else min(K, -(-1024 // wgs))
    k_per = -(-K // ks)
    return Plan(tiles, NB, gy, ks, k_per, -(-K // k_per))


def workspace_bytes(M_out, K, Cin, Cout):
    return int(_n.hip().wsis_spconv_fwd_workspace_bytes(M_out, K, Cin, Cout))


def launch_fwd(X, nbr_p, order, W, bias, residual, M_out):
    """wsis_spconv_fwd with the output full of NaN and the workspace full of 0xFF; W [K, Cin, Cout].  The output is
    followed by 64 rows of NaN inside its allocation, which must still be NaN afterwards (a row id past M_out)."""
    lib = _n.hip()
    K, Cin, Cout = W.shape
    guard = torch.full((M_out + 64, Cout), float("nan"), device=DEV)
    out = guard[:M_out]
    wsb = workspace_bytes(M_out, K, Cin, Cout)
    assert wsb >= 256
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    _n.check(lib.wsis_spconv_fwd(_n.ptr(X), _n.ptr(nbr_p), _n.ptr(order), _n.ptr(W), _n.ptr(bias), _n.ptr(residual),
                                 _n.ptr(out), X.shape[0], M_out, K, Cin, Cout, _n.ptr(ws), wsb, _n.stream_ptr()),
             "spconv_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard[M_out:]).all()), "spconv_fwd wrote behind the last output row"
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def dev_table(tab, order="own"):
    """(packed table, tile order) on the device; ``order``: "own" = the table's, None, or a permutation"""
    if tab is None:
        return None, None
    o = tab.order if isinstance(order, str) else order
    return (torch.from_numpy(F.pack(tab.nbr, o)).to(DEV).contiguous(),
            None if o is None else torch.from_numpy(np.ascontiguousarray(o)).to(DEV))


def one_float_in(t):
    """a copy of ``t`` one float into its own storage (4-byte aligned), followed by 64 rows of NaN"""
    store = torch.full((t.numel() + 64 * t.shape[1] + 1,), float("nan"), device=t.device)
    v = store[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 == 4
    return v, store


def keep_generic(M_out):
    """packed slices of a thinned case: the four slices of tile 0, make_table's promised slices, every 29th-or-so slice
    (alone in its tile) and the last two"""
    n = I.n_slices(M_out)
    return frozenset({0, 1, 2, 3, n - 2, n - 1} | set(I.special_slices(M_out).values()) | set(range(0, n, -(-n // 28) | 1)))


def table_for(c, variation):
    """(Table or None, M_in)"""
    if c.name == "null-table":
        return None, c.M_out
    return I.table(c.M_out, variation, c.K, keep_generic(c.M_out) if c.M_out >= THIN_FROM else None)


def variations(c):
    return ("eq",) if c.name == "null-table" else ("eq", "gt")


def _setup(name, variation, monkeypatch, seed=5):
    c = BY_NAME[name]
    monkeypatch.delenv("WSIS_CONV_MATH", raising=False)
    if name == "cin6-generic":
        monkeypatch.setenv("WSIS_IN_CONV", "0")
    else:
        monkeypatch.delenv("WSIS_IN_CONV", raising=False)
    p = plan_ref(c.M_out, c.K, c.Cout)
    assert p == Plan(c.tiles, c.NB, c.gy, c.ks, c.k_per, c.kz), (name, p)
    assert workspace_bytes(c.M_out, c.K, c.Cin, c.Cout) == (256 if p.ks == 1 else p.ks * c.M_out * c.Cout * 4 + 256), name
    tab, M_in = table_for(c, variation)
    X, W, WT, bias, residual, _, buf = I.make_inputs(M_in, c.M_out, seed, DEV, c.K, c.Cin, c.Cout)
    if name == "unaligned-x":
        X, buf = one_float_in(X)
    vec4 = c.Cin % 4 == 0 and c.Cout % 4 == 0 and X.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
    assert vec4 == (name not in ("scalar-loads", "cin6-generic", "unaligned-x")), name
    return c, p, tab, M_in, X, W, WT, bias, residual, buf


def test_the_cases_reach_the_branches_they_are_named_for():
    """host arithmetic only: the z blocks, table groups, column groups and tiles of every case, and the thinned tables"""
    for c in CASES:
        p = plan_ref(c.M_out, c.K, c.Cout)
        assert p == Plan(c.tiles, c.NB, c.gy, c.ks, c.k_per, c.kz), (c.name, p)
        blocks = [min(c.K, (z + 1) * p.k_per) - z * p.k_per for z in range(p.kz)]
        assert sum(blocks) == c.K and min(blocks) >= 1
        groups = [[min(KG, b - g) for g in range(0, b, KG)] for b in blocks]
        assert c.reduce == (None if p.kz == 1 else "4" if c.Cout % 4 == 0 else "1")
        if c.name == "one-tile-full-split":
            assert blocks == [1] * 27 and c.M_out - TM == 1
        elif c.name == "split-kper2":
            assert blocks == [2] * 13 + [1]
        elif c.name == "split-kper7":
            assert blocks == [7, 7, 7, 6]
        elif c.name == "no-split-k27":
            assert groups == [[16, 11]] and p.tiles * p.gy >= 512
        elif c.name == "split-two-groups":
            assert groups[0] == [16, 5] and all(len(g) == 2 for g in groups)
        elif c.name.startswith("nb") and c.name != "nb4-two-groups":
            assert p.NB == int(c.name[2:]) and p.gy == 1 and p.tiles == 101
        elif c.name == "nb4-two-groups":
            assert (p.NB, p.gy) == (4, 2) and c.Cout - 128 == 72 and 72 % 32
        elif c.name == "scalar-loads":
            assert c.Cin % 32 == 1 and c.Cout % 32 == 6 and c.Cout % 4
        if c.M_out < THIN_FROM:
            continue
        for v in variations(c):
            tab, _ = table_for(c, v)
            P = tab.info["packed"]
            live = np.zeros(p.tiles * 4, dtype=bool)
            n = I.n_slices(c.M_out)
            live[:n] = [(P[:, s * 32:(s + 1) * 32] >= 0).any() for s in range(n)]
            per_tile = live.reshape(p.tiles, 4).sum(1)
            assert live.sum() <= 45 and (per_tile == 0).any() and (per_tile == 1).any() and (per_tile == 4).any(), (c.name, v)
            assert ((P >= 0).sum(1) >= 1).all()                          # every offset has a pair


@pytest.mark.parametrize("name", NAMES)
def test_generic_forward_against_fp64(name, monkeypatch):
    worst, worst_pairs, worst_drop = 0.0, 0.0, float("inf")
    for v in variations(BY_NAME[name]):
        c, p, tab, M_in, X, W, WT, bias, residual, buf = _setup(name, v, monkeypatch)
        nbr = None if tab is None else tab.nbr
        nbr_p, order = dev_table(tab)
        bare = torch.arange(0) if tab is None else torch.from_numpy(I.rows_without_pairs(nbr)).to(DEV)
        assert tab is None or c.M_out < 3 * 32 or bare.numel() >= 32
        core = F.conv(X, WT, nbr, 0, M_out=c.M_out)
        for b in (None, bias):
            for r in (None, residual):
                what = f"{name} {v} bias={b is not None} residual={r is not None}"
                out = launch_fwd(X, nbr_p, order, W, b, r, c.M_out)
                again = launch_fwd(X, nbr_p, order, W, b, r, c.M_out)
                assert torch.equal(bits(out), bits(again)), f"{what}: two launches differ"
                want = core if b is None else core + b.double()
                want = want if r is None else want + r.double()
                res = F.check_conv(out, X, WT, nbr, 0, b, r, extra=p.kz, what=what, want=want)
                worst, worst_pairs, worst_drop = max(worst, res.all), max(worst_pairs, res.pairs), min(worst_drop, res.drop)
                if bare.numel():
                    exact = torch.zeros(bare.numel(), c.Cout, device=DEV)
                    exact = exact if b is None else exact + b
                    exact = exact if r is None else exact + r[bare]
                    assert torch.equal(out[bare], exact), f"{what}: rows without a pair (empty tiles and slices)"
        assert bool(torch.isnan(buf.flatten()[-64 * c.Cin:]).all()) and bool(torch.isfinite(X).all())
    print(f"[generic-fwd] conv {name}: tiles={p.tiles} NB={p.NB} gy={p.gy} ks={p.ks} k_per={p.k_per} kz={p.kz}  error/bound "
          f"{worst:.3e}  rows with pairs {worst_pairs:.3e}  dropped pair/bound {worst_drop:.3e}")


@pytest.mark.parametrize("name", NAMES)
def test_tile_order_does_not_change_a_row(name, monkeypatch):
    """csrc/spconv.hip: "the reduction order is fixed, so results are ... independent of the tile order" -- a tile walks its
    active offsets in ascending order and a row without a pair under one of them adds exact zeros, the z blocks are added
    in z order: the same table without a tile order and under two permutations gives every row the same bits"""
    for v in variations(BY_NAME[name]):
        c, p, tab, M_in, X, W, WT, bias, residual, buf = _setup(name, v, monkeypatch, seed=6)
        perms = (None, F.permutation(31 + c.M_out, c.M_out), F.permutation(977 + c.M_out, c.M_out))
        outs = []
        for o in perms:
            if tab is None:
                nbr_p, order = None, None if o is None else torch.from_numpy(o).to(DEV)
            else:
                nbr_p, order = dev_table(tab, o)
            outs.append(launch_fwd(X, nbr_p, order, W, bias, residual, c.M_out))
        assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(outs[0]), bits(outs[2])), (name, v)
