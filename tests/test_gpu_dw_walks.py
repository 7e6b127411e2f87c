"""GPU: the weight gradient of the sparse convolutions (wsis_spconv_dw; default kernel spconv_dw3_kernel,
csrc/spconv_dw2.hip) against fp64 gather-GEMMs over ORACLE pair lists (tests/conv_ref.py), where its control flow
branches.  Almost all of that control flow is slice bookkeeping -- a wave owns one (offset group, Cin chunk, Cout block)
and walks the 32-row slices first, first + stride, ... (snake: every odd round of a full round reversed, slice_at), with
the next slice's header in flight (hb / has_next), a re-issue loop for slices without pairs for its group, fix_tail for
the partial last slice and a prologue that skips empty first slices -- so the walk cases below restate the walk in
Python from the packed table, check it against the kernel's own per-wave count of slices with work
(wsis_debug_dw2_diag), and assert which of these events occurred:

  a  a wave walked >= 3 rounds with work (the snake reverses)
  b  a wave skipped a slice empty for its group between two slices with work (re-issue loop)
  c  a wave's first position was empty for its group and a later one had work (prologue loop)
  d  a wave walked >= 1 position and had no work at all (its accumulators are written as zeros)
  e  a wave reached the partial last slice (M_out % 32 != 0) by a slice advance

Every dW is computed with the workspace and the output pre-filled with NaN: an element no workgroup writes cannot pass.
Also: the edge matrix of row counts / partial output blocks / kernel volumes for both kernels (WSIS_DW3=1, 0), the
generic fallback kernel (csrc/spconv.hip), and wsis_spconv_dw_bn against fp64 relu(bn(x))."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref
import dw_plan_ref
import harness
import wsis_native as _n
from oracle import spconv_ref as ref
from spconv import ops
from test_dw_partition import _groups as _balanced_groups
from util import random_sparse_coords

pytestmark = pytest.mark.gpu
DEV = "cuda"
HINTS = (0, 625000)          # launch plans: one / two 4-wave workgroups per CU and combination (different slab counts)
FRAC = 1e-5                  # dW bound: fraction of max|dW_fp64| (fp32 sums of <= 27 * M_out products, fixed order)
EVENTS = "abcde"


def _lib():
    return _n.hip()


def _dw(X, nbr, order, dY, K, Cin, Cout):
    """wsis_spconv_dw with a workspace and an output full of NaN"""
    lib = _lib()
    M_out = dY.shape[0]
    wsb = lib.wsis_spconv_dw_workspace_bytes(M_out, K, Cin, Cout)
    ws = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)           # every float of it a NaN
    dW = torch.full((K, Cin, Cout), float("nan"), device=DEV)
    _n.check(lib.wsis_spconv_dw(_n.ptr(X), _n.ptr(nbr), _n.ptr(order), _n.ptr(dY), _n.ptr(dW), X.shape[0], M_out, K,
                                Cin, Cout, _n.ptr(ws), wsb, _n.stream_ptr()), "spconv_dw")
    torch.cuda.synchronize()
    return dW


def _diag(X, nbr, order, dY, K, Cin, Cout):
    """per-wave records of the diagnostic build of the same launch: [n_waves, 10] int64 (d[1] = loop start stamp, 0 when
    the wave had no work; d[5] = slices with work)"""
    lib = _lib()
    fn = lib.wsis_debug_dw2_diag
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_int32] * 3 + [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    M_out = dY.shape[0]
    ws = torch.empty(lib.wsis_spconv_dw_workspace_bytes(M_out, K, Cin, Cout), dtype=torch.uint8, device=DEV)
    dbg = torch.zeros(1 << 18, dtype=torch.int64, device=DEV)
    nw = ctypes.c_int64(0)
    _n.check(fn(_n.ptr(X), _n.ptr(nbr), _n.ptr(order), _n.ptr(dY), X.shape[0], M_out, K, Cin, Cout, _n.ptr(ws),
                _n.ptr(dbg), dbg.numel() * 8, ctypes.byref(nw), _n.stream_ptr()), "dw2_diag")
    torch.cuda.synchronize()
    # the diagnostic launches the grid of the plan the product itself takes (wsis_debug_dw_plan: dw_plan())
    p = dw_plan_ref.plan_lib(dw_plan_ref.Case("walk", X.shape[0], M_out, K, Cin, Cout, dw_plan_ref.TABLE,
                                              dw_plan_ref.ALIGNED, 0, 1, ""))
    assert nw.value == p["gx"] * p["gy"] * dw_plan_ref.WGW, (nw.value, p)
    return dbg[: nw.value * 10].view(-1, 10).cpu().numpy()


def _groups(K):
    """offsets of each worker's slots: the activity-balanced partition for 3 x 3 x 3, else og + j * NOG"""
    if K == 27:
        return _balanced_groups()
    nog = (K + 7) // 8
    return [[og + j * nog for j in range(8) if og + j * nog < K] for og in range(nog)]


def _walk(nbr_p, M_out, K, Cin, Cout, recs):
    """restate every wave's walk from the packed table; check it against the kernel's records; count the events"""
    n_slices = (M_out + 31) // 32
    nchunk, nblk = Cin // 32, (Cout + 31) // 32
    groups = _groups(K)
    gy = len(groups) * nchunk * nblk
    n_waves = recs.shape[0]
    assert n_waves % (4 * gy) == 0
    P = n_waves // (4 * gy)
    stride = 4 * P
    live = torch.zeros(K, n_slices * 32, dtype=torch.bool, device=nbr_p.device)
    live[:, :M_out] = nbr_p >= 0
    live = live.view(K, n_slices, 32).any(2)
    gmask = torch.stack([live[g].any(0) for g in groups]).cpu().numpy()      # [group, slice]: the group has a pair
    tail_partial = M_out % 32 != 0
    ev = dict.fromkeys(EVENTS, 0)
    rec = recs.reshape(gy, P, 4, 10)
    for by in range(gy):
        og = by // (nchunk * nblk)
        for bx in range(P):
            for w in range(4):
                first = bx * 4 + w
                R = max(0, -(-(n_slices - first) // stride))
                r = np.arange(R)
                sl = np.where((r & 1).astype(bool) & ((r + 1) * stride <= n_slices), r * stride + (stride - 1 - first),
                              first + r * stride)
                work = gmask[og, sl]
                n_work = int(work.sum())
                d = rec[by, bx, w]
                assert int(d[5]) == n_work, (by, bx, w, int(d[5]), n_work)
                assert (int(d[1]) == 0) == (n_work == 0), (by, bx, w)
                if R >= 1 and n_work == 0:
                    ev["d"] += 1
                if n_work == 0:
                    continue
                f = int(np.argmax(work))
                ev["a"] += R >= 3
                last = R - 1 - int(np.argmax(work[::-1]))
                ev["b"] += bool((~work[f + 1:last]).any())
                ev["c"] += f > 0
                ev["e"] += tail_partial and sl[-1] == n_slices - 1 and R - 1 > f
    return ev, P


# ---------------------------------------------------------------- inputs of the walk cases
@pytest.fixture(scope="module")
def c2_levels():
    b = harness.collate([harness.make_scene(1)])
    idx = b["voxel_locs"].int().to(DEV).contiguous()
    shape = [int(s) for s in b["spatial_shape"]]
    out = [(idx.cpu().numpy(), shape)]
    for _ in range(2):
        rd = ops.build_down_rulebook(idx, shape, [2] * 3, [2] * 3, [0] * 3)
        idx, shape = rd.out_indices, rd.out_shape
        out.append((idx.cpu().numpy(), [int(s) for s in shape]))
    return out


def _lines_scene(layout):
    """scenes of lines whose slices use different offset groups: x-lines ("x": offsets 4, 13, 22 -- no pair for group 1),
    xy-diagonal lines ("d": 1, 13, 25 -- none for group 3) and isolated voxels ("i": 13 only), one scene per letter.  The
    tile order puts the heavier slices first, in scene order among equals, and keeps the partial last slice last.
    "xdi": a group-1 worker starts on empty slices (c), works on the diagonals or never works (d); "dxdi": it works, skips
    the x-lines (b) and works again; the partial tail is isolated voxels in both."""
    pts = []
    for b, kind in enumerate(layout):
        if kind == "x":
            pts += [(b, x, y, z) for y in range(0, 64, 2) for z in (0, 2, 4) for x in range(64)]
        elif kind == "d":
            zs = (0, 4, 8) if b == 0 else (0, 4)
            pts += [(b, x, x - c, z) for c in range(-60, 61, 3) for z in zs for x in range(64) if 0 <= x - c < 64]
        else:
            iso = [(b, x, y, z) for x in range(0, 64, 2) for y in range(0, 64, 2) for z in range(0, 16, 2)]
            pts += iso[: len(iso) - (len(pts) + len(iso) - 7) % 32]      # M % 32 == 7
    idx = np.array(pts, dtype=np.int32)
    return idx[np.random.default_rng(8).permutation(len(idx))], [64, 64, 16]


def _case_input(name, c2_levels):
    """-> (fine indices, spatial shape, kind)"""
    if name == "c2_l0":
        return c2_levels[0] + ("subm",)
    if name == "c2_l2":
        return c2_levels[2] + ("subm",)
    if name == "c2_down0":
        return c2_levels[0] + ("down",)
    if name == "sheet120":
        return random_sparse_coords(41, 4, (120, 120, 8), 0.2, surface=True), [120, 120, 8], "subm"
    if name == "sheet120_sparse":
        return random_sparse_coords(42, 3, (120, 120, 8), 0.1, surface=True), [120, 120, 8], "subm"
    if name == "sheet40":
        return random_sparse_coords(43, 6, (40, 40, 6), 0.3, surface=True), [40, 40, 6], "subm"
    if name in ("lines", "bands"):
        idx, shape = _lines_scene("xdi" if name == "lines" else "dxdi")
        return idx, shape, "subm"
    raise ValueError(name)


# (case, Cin, Cout): the UNet's widths, the strided K = 8 form (128 -> 160: the widths of its deepest strided conv, on
# the level-0 table -- 8 slabs, 26 rounds a wave), thin low-density surfaces, and the line scenes
WALKS = [("c2_l0", 32, 32), ("c2_l2", 96, 96), ("c2_down0", 32, 64), ("c2_down0", 128, 160), ("sheet120", 64, 64),
         ("sheet120_sparse", 96, 96), ("sheet40", 160, 160), ("lines", 64, 64), ("bands", 64, 64)]


@pytest.mark.parametrize("name,cin,cout", WALKS)
def test_weight_gradient_walks_against_fp64(c2_levels, name, cin, cout):
    lib = _lib()
    idx, shape, kind = _case_input(name, c2_levels)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx)).to(DEV)
    if kind == "subm":
        rb = ops.build_subm_rulebook(idx_d, shape, [3] * 3, [1] * 3)
        pairs = ref.subm_pairs_fast(idx, shape, 3, 1)
        M_in = M_out = idx.shape[0]
    else:
        rb = ops.build_down_rulebook(idx_d, shape, [2] * 3, [2] * 3, [0] * 3)
        out_idx, _, pairs = ref.down_pairs_fast(idx, shape, 2, 2, 0)
        assert np.array_equal(rb.out_indices.cpu().numpy(), np.asarray(out_idx, dtype=np.int32))
        M_in, M_out = idx.shape[0], out_idx.shape[0]
    K = len(pairs)
    pairs_d = conv_ref.device_pairs(pairs, DEV)
    g = torch.Generator(device=DEV).manual_seed(cin + cout + M_out)
    X = torch.randn(M_in, cin, device=DEV, generator=g)
    dY = torch.randn(M_out, cout, device=DEV, generator=g)
    want = conv_ref.dw(X, dY, pairs_d)
    seen = dict.fromkeys(EVENTS, 0)
    try:
        for hint in HINTS:
            _n.check(lib.wsis_hint_batch_rows(hint), "hint")
            ev, P = _walk(rb.nbr_p, M_out, K, cin, cout, _diag(X, rb.nbr_p, rb.order, dY, K, cin, cout))
            for e in EVENTS:
                seen[e] += ev[e]
            got = _dw(X, rb.nbr_p, rb.order, dY, K, cin, cout)
            err, bound, err_drop = conv_ref.check_dw(got, X, dY, pairs_d, FRAC, f"{name} hint={hint}", want=want)
            print(f"walk {name} {kind} {cin}->{cout} M_out={M_out} hint={hint} slabs={P}: events "
                  + " ".join(f"{e}={ev[e]}" for e in EVENTS)
                  + f"; dW err {err:.2e} <= {bound:.2e}, one pair removed {err_drop:.2e}")
    finally:
        _n.check(lib.wsis_hint_batch_rows(0), "hint")
    missing = [e for e in WALK_EVENTS[(name, cin)] if seen[e] == 0]
    assert not missing, f"{name}: events {missing} did not occur ({seen})"


# the events each walk case must produce (checked above); together they cover all five
WALK_EVENTS = {("c2_l0", 32): "ae", ("c2_l2", 96): "ae", ("c2_down0", 32): "e", ("c2_down0", 128): "ae",
               ("sheet120", 64): "ae", ("sheet120_sparse", 96): "ae", ("sheet40", 160): "ae", ("lines", 64): "acde",
               ("bands", 64): "abce"}


def test_the_walk_cases_cover_every_event():
    assert set("".join(WALK_EVENTS.values())) == set(EVENTS)
    assert set(WALK_EVENTS) == {w[:2] for w in WALKS}


# ---------------------------------------------------------------- edge matrix (small, both kernels)
def _random_table(rng, M_in, M_out, K):
    """oracle-form pairs: offset 0 pairs every output row, the others a random 60 % of them; random input rows"""
    pairs = []
    for k in range(K):
        po = np.arange(M_out) if k == 0 else np.nonzero(rng.random(M_out) < 0.6)[0]
        pairs.append((rng.integers(0, M_in, len(po)), po))
    return pairs


@pytest.mark.parametrize("dw3", ["1", "0"])
@pytest.mark.parametrize("table", ["dense", "k1", "k8", "k27"])
def test_weight_gradient_edge_matrix(monkeypatch, dw3, table):
    """M_out of 1 / 31 / 32 / 33 / 95 rows (one partial slice, exactly one, one row into a second, three), Cout of 4 / 20 /
    36 / 100 / 160 (partial output blocks: pieces of the dY rows past Cout read as zero), Cin of 32 / 96 / 256, K = 1
    without a table (nbr = NULL) and with one, K = 8 and 27; WSIS_DW3=1 (spconv_dw3_kernel) and 0 (spconv_dw2_kernel)"""
    monkeypatch.setenv("WSIS_DW3", dw3)
    K = {"dense": 1, "k1": 1, "k8": 8, "k27": 27}[table]
    rng = np.random.default_rng(K * 7 + int(dw3))
    g = torch.Generator(device=DEV).manual_seed(K + int(dw3))
    worst = 0.0
    for M_out in (1, 31, 32, 33, 95):
        M_in = M_out if table == "dense" else 47
        if table == "dense":
            pairs, nbr_p, order = [(np.arange(M_out), np.arange(M_out))], None, None
        else:
            pairs = _random_table(rng, M_in, M_out, K)
            order = torch.from_numpy(rng.permutation(M_out).astype(np.int32)).to(DEV)
            nbr_p = torch.from_numpy(ref.pairs_to_table(pairs, M_out)).to(DEV)[:, order.long()].contiguous()
        pairs_d = conv_ref.device_pairs(pairs, DEV)
        for cout in (4, 20, 36, 100, 160):
            for cin in (32, 96, 256):
                X = torch.randn(M_in, cin, device=DEV, generator=g)
                dY = torch.randn(M_out, cout, device=DEV, generator=g)
                got = _dw(X, nbr_p, order, dY, K, cin, cout)
                err, bound, _ = conv_ref.check_dw(got, X, dY, pairs_d, FRAC, f"{table} M_out={M_out} {cin}->{cout}")
                worst = max(worst, err / bound if bound else 0.0)
    print(f"edge matrix {table} WSIS_DW3={dw3}: worst error {worst:.3f} of the bound")


# ---------------------------------------------------------------- the generic fallback of wsis_spconv_dw
@pytest.mark.parametrize("case", ["unaligned", "cin33_cout200", "k125"])
def test_generic_weight_gradient_kernel(case):
    """csrc/spconv.hip spconv_dw_kernel: an X that is not 16-byte aligned (a view one float into its storage), Cin not a
    multiple of 32 with more than 5 output blocks (two trips of the block-group loop), 125 offsets"""
    shape = (30, 30, 8)
    idx = random_sparse_coords(51, 2, shape, 0.4, surface=True)
    idx_d = torch.from_numpy(idx).to(DEV)
    if case == "k125":
        rb = ops.build_subm_rulebook(idx_d, list(shape), [5] * 3, [2] * 3)
        pairs = ref.subm_pairs_fast(idx, shape, 5, 2)
        cin, cout = 32, 32
    else:
        rb = ops.build_subm_rulebook(idx_d, list(shape), [3] * 3, [1] * 3)
        pairs = ref.subm_pairs_fast(idx, shape, 3, 1)
        cin, cout = (32, 32) if case == "unaligned" else (33, 200)
    K, M = len(pairs), idx.shape[0]
    g = torch.Generator(device=DEV).manual_seed(K + cin)
    store = torch.randn(M * cin + 1, device=DEV, generator=g)
    X = store[1:].view(M, cin) if case == "unaligned" else store[:-1].view(M, cin)
    assert (X.data_ptr() % 16 != 0) == (case == "unaligned")
    dY = torch.randn(M, cout, device=DEV, generator=g)
    pairs_d = conv_ref.device_pairs(pairs, DEV)
    got = _dw(X, rb.nbr_p, rb.order, dY, K, cin, cout)
    err, bound, err_drop = conv_ref.check_dw(got, X, dY, pairs_d, FRAC, case)
    print(f"generic {case} K={K} {cin}->{cout} M={M}: dW err {err:.2e} <= {bound:.2e}, one pair removed {err_drop:.2e}")


# ---------------------------------------------------------------- wsis_spconv_dw_bn against fp64 relu(bn(x))
@pytest.mark.parametrize("kind,cin,cout", [("subm", 64, 64), ("subm", 96, 32), ("down", 32, 64), ("inverse", 64, 32)])
def test_weight_gradient_with_batchnorm_on_the_fly_against_fp64(kind, cin, cout):
    """the own-rows form (spconv_dw2_kernel SWAP: slices over the convolution's INPUT rows, conv dY gathered through the
    dIn table) with and without the BatchNorm + ReLU, on a multi-scene surface: dW = sum relu(bn(x))[pi]^T dY[po] over the
    oracle's forward pairs, in fp64.  Workspace and output full of NaN."""
    lib = _lib()
    shape = [120, 120, 8]
    idx = random_sparse_coords(61, 3, tuple(shape), 0.25, surface=True)
    idx_d = torch.from_numpy(idx).to(DEV)
    if kind == "subm":
        rb = ops.build_subm_rulebook(idx_d, shape, [3] * 3, [1] * 3)
        pairs = ref.subm_pairs_fast(idx, shape, 3, 1)
        nbr_b, order_b, flip, M_in, M_out = rb.nbr_p, rb.order, 1, idx.shape[0], idx.shape[0]
    else:
        rb = ops.build_down_rulebook(idx_d, shape, [2] * 3, [2] * 3, [0] * 3)
        coarse, _, down = ref.down_pairs_fast(idx, shape, 2, 2, 0)
        if kind == "down":
            pairs = down
            nbr_b, order_b, flip, M_in, M_out = rb.nbr_up_p, rb.order_up, 0, idx.shape[0], coarse.shape[0]
        else:
            pairs = ref.inverse_pairs(down)
            nbr_b, order_b, flip, M_in, M_out = rb.nbr_p, rb.order, 0, coarse.shape[0], idx.shape[0]
    K = len(pairs)
    pairs_d = conv_ref.device_pairs(pairs, DEV)
    g = torch.Generator(device=DEV).manual_seed(cin * 3 + cout)
    x = torch.randn(M_in, cin, device=DEV, generator=g) * 1.5 + 0.4
    dY = torch.randn(M_out, cout, device=DEV, generator=g)
    gamma = torch.rand(cin, device=DEV, generator=g) + 0.5
    gamma[::5] *= -1.0
    beta = torch.randn(cin, device=DEV, generator=g)
    mean, var = x.mean(0).contiguous(), x.var(0, unbiased=False).contiguous()
    eps = 1e-4
    a = ((x.double() - mean.double()) / torch.sqrt(var.double() + eps) * gamma.double() + beta.double()).clamp_min(0.0)
    assert lib.wsis_spconv_dw_bn_supported(K, cin, cout)
    wsb = lib.wsis_spconv_dw_bn_workspace_bytes(M_in, K, cin, cout)
    for bn_on in (True, False):
        ws = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)
        dW = torch.full((K, cin, cout), float("nan"), device=DEV)
        src = x if bn_on else a.float()
        _n.check(lib.wsis_spconv_dw_bn(_n.ptr(src), _n.ptr(mean) if bn_on else None, _n.ptr(var) if bn_on else None,
                                       _n.ptr(gamma) if bn_on else None, _n.ptr(beta) if bn_on else None, eps, 1,
                                       _n.ptr(nbr_b), _n.ptr(order_b), flip, _n.ptr(dY), _n.ptr(dW), M_in, M_out, K, cin,
                                       cout, _n.ptr(ws), wsb, _n.stream_ptr()), "dw_bn")
        torch.cuda.synchronize()
        ref_in = a if bn_on else a.float()
        err, bound, err_drop = conv_ref.check_dw(dW, ref_in, dY, pairs_d, FRAC, f"dw_bn {kind} bn={bn_on}")
        print(f"dw_bn {kind} {cin}->{cout} bn={bn_on}: dW err {err:.2e} <= {bound:.2e}, one pair removed {err_drop:.2e}")
