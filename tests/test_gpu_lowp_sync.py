"""GPU, one process: the pieces of the synced 16-bit native training pass (WSIS_NATIVE_LP_TRAIN=1 + WSIS_NATIVE_LP_SYNC=1).

(a) wsis_bn_bwd_apply_lp is the apply pass of wsis_bn_bwd_lp: fed the dgamma / dbeta that wsis_bn_bwd_lp(d_dx = NULL) wrote,
    dx equals wsis_bn_bwd_lp's own bit for bit; with other sums it is wsis_bn_bwd_apply on the widened inputs, stored as
    fp32 or rounded once.
(b) the four helper kernels of the statistics exchange (wsis_bn_sync_*) equal a numpy restatement of their expressions in
    the same order: every operation is an IEEE fp64 + - * / or a round-to-nearest cast on both sides, so mean, var, count
    and the scaled sums are compared with array_equal.  Running statistics against fp64 torch BatchNorm1d over all rows.
(c) a world of one: with a gloo group of this single process the synced pass equals the unsynced 16-bit pass bit for bit
    (m n / n = m in fp64 for fp32 m and n < 2^24, the centred term is 0, M / N = 1): output, input gradient, every
    parameter gradient.  running_mean to rounding; running_var has another update expression and is left out.
"""
import os

import numpy as np
import pytest
import torch

import harness
import spconv
import unet_native as un
import wsis_native as _n
import wsis_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
CODE = {torch.bfloat16: 0, torch.float16: 1}
NAN = float("nan")
EPS = 1e-4
SMALL_ROWS = int(os.environ.get("WSIS_BN_SMALL_ROWS", "4096"))      # bn_small_rows(): one-launch reduction up to here


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- (a) the apply pass from reduced sums ----------------------------------------------------------------------------

def _bwd_lp(x, dy, mean, var, gamma, beta, relu, addend, out_dtype):
    """wsis_bn_bwd_lp in training mode; out_dtype None: d_dx == NULL"""
    M, C = x.shape
    dx = torch.full((M, C), NAN, dtype=out_dtype, device=DEV) if out_dtype is not None else None
    dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    wsb = _n.hip().wsis_bn_workspace_bytes(M, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _n.check(_n.hip().wsis_bn_bwd_lp(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta), EPS, relu,
                                     1, _n.ptr(dx), int(out_dtype == torch.float32), _n.ptr(dg), _n.ptr(db), _n.ptr(addend),
                                     M, C, CODE[x.dtype], _n.ptr(ws), wsb, _n.stream_ptr()), "bn_bwd_lp")
    return dx, dg, db


def _apply_lp(x, dy, mean, var, gamma, beta, s_xhat, s_dz, relu, addend, out_dtype):
    M, C = x.shape
    dx = torch.full((M, C), NAN, dtype=out_dtype, device=DEV)
    _n.check(_n.hip().wsis_bn_bwd_apply_lp(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta),
                                           _n.ptr(s_xhat), _n.ptr(s_dz), EPS, relu, _n.ptr(dx),
                                           int(out_dtype == torch.float32), _n.ptr(addend), M, C, CODE[x.dtype],
                                           _n.stream_ptr()), "bn_bwd_apply_lp")
    return dx


def _apply32(x, dy, mean, var, gamma, beta, s_xhat, s_dz, relu, addend):
    M, C = x.shape
    dx = torch.full((M, C), NAN, device=DEV)
    _n.check(_n.hip().wsis_bn_bwd_apply(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta),
                                        _n.ptr(s_xhat), _n.ptr(s_dz), EPS, relu, _n.ptr(dx), _n.ptr(addend), M, C,
                                        _n.stream_ptr()), "bn_bwd_apply")
    return dx


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", (8, 32, 160))
def test_bwd_apply_lp_is_the_apply_pass_of_bwd_lp(C, dt):
    g = torch.Generator(device=DEV).manual_seed(300 + C)
    rounded_somewhere = False
    for M in (1, 33, 257, SMALL_ROWS + 1):      # one row; ragged quads and workgroups; the two-launch reduction
        x = (torch.randn(M, C, device=DEV, generator=g) * 2 + 0.3).to(dt)
        dy = torch.randn(M, C, device=DEV, generator=g).to(dt)
        add = (torch.randn(M, C, device=DEV, generator=g) * 0.5).to(dt)
        mean = x.float().mean(0)
        var = x.float().var(0, unbiased=False) if M > 1 else torch.zeros(C, device=DEV)
        gamma = torch.randn(C, device=DEV, generator=g)
        beta = torch.randn(C, device=DEV, generator=g) * 0.3
        for relu in (0, 1):
            for addend in (None, add):
                what = f"M {M} C {C} relu {relu} addend {addend is not None} {dt}"
                _, dg, db = _bwd_lp(x, dy, mean, var, gamma, beta, relu, None, None)      # d_dx = NULL: the sums alone
                assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all()), what
                # arbitrary sums: the local ones as a rank holding 700 of 2000 rows would get them back
                s_g, s_b = (dg.double() * (700.0 / 2000.0)).float(), (db.double() * (700.0 / 2000.0)).float()
                a32 = None if addend is None else addend.float()
                ref32 = _apply32(x.float(), dy.float(), mean, var, gamma, beta, s_g, s_b, relu, a32)
                assert bool(torch.isfinite(ref32).all()), what
                for out_dtype in (dt, torch.float32):
                    own, dg2, db2 = _bwd_lp(x, dy, mean, var, gamma, beta, relu, addend, out_dtype)
                    assert _same(dg2, dg) and _same(db2, db), what
                    got = _apply_lp(x, dy, mean, var, gamma, beta, dg, db, relu, addend, out_dtype)
                    assert _same(got, own), what + f": out {out_dtype}: dx of the sums wsis_bn_bwd_lp wrote"
                    got = _apply_lp(x, dy, mean, var, gamma, beta, s_g, s_b, relu, addend, out_dtype)
                    want = ref32 if out_dtype == torch.float32 else ref32.to(dt)
                    assert _same(got, want), what + f": out {out_dtype}: arbitrary sums"
                    if out_dtype != torch.float32:
                        rounded_somewhere |= not torch.equal(got.float(), ref32)
    assert rounded_somewhere, "the 16-bit dx never differed from the fp32 one: the comparison shows nothing"


# ---- (b) the helper kernels of the exchange --------------------------------------------------------------------------

def _combine_ref(g, C):
    """mean, var, count of wsis_bn_sync_combine restated: fp64, ranks in ascending order, the first term starts every sum"""
    R = g.shape[0]
    n = g[:, 2 * C]
    N = n[0]
    for r in range(1, R):
        N = N + n[r]
    if not N > 0:
        return np.zeros(C, np.float32), np.zeros(C, np.float32), N
    s = g[0, :C] * n[0]
    for r in range(1, R):
        s = s + g[r, :C] * n[r]
    mean64 = s / N
    q = None
    for r in range(R):
        dm = g[r, :C] - mean64
        sq = dm * dm
        t = (g[r, C:2 * C] + sq) * n[r]
        q = t if r == 0 else q + t
    var64 = q / N
    return mean64.astype(np.float32), var64.astype(np.float32), N


def _rank_rows(counts, C, kind, seed):
    """fp32 rows of every rank (CPU); "offset": |mean| = 1000 sigma with rank means that differ"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r, n in enumerate(counts):
        if kind == "offset":
            rows.append(torch.randn(n, C, generator=g) * 0.05 + 50.0 + 0.004 * r)
        else:
            rows.append(torch.randn(n, C, generator=g) * (1.0 + 0.5 * r) + 0.3 * r - 0.5)
    return rows


CASES = [((5,), "plain"), ((1,), "plain"), ((0,), "plain"), ((700, 1300), "plain"), ((0, 9), "plain"), ((1, 1), "plain"),
         ((4, 0, 1), "plain"), ((3, 1, 0, 250, 17, 2, 1, 64), "plain"), ((700, 1300), "offset"), ((300, 1, 500), "offset")]


@pytest.mark.parametrize("C", (8, 160))
@pytest.mark.parametrize("counts,kind", CASES, ids=["-".join(map(str, c)) + "_" + k for c, k in CASES])
def test_exchange_helpers_equal_their_numpy_restatement(counts, kind, C):
    lib, st = _n.hip(), _n.stream_ptr()
    R, mom = len(counts), 0.1
    rows = _rank_rows(counts, C, kind, 7 * R + C)
    gathered = torch.full((R, 2 * C + 1), NAN, dtype=torch.float64, device=DEV)
    want_g = np.zeros((R, 2 * C + 1), np.float64)
    for r, x in enumerate(rows):
        n = x.shape[0]
        if n > 0:      # a rank's local statistics: fp32 values (how they were computed does not matter here)
            m32 = x.double().mean(0).float()
            v32 = x.double().var(0, unbiased=False).float()
            want_g[r, :C], want_g[r, C:2 * C] = m32.double().numpy(), v32.double().numpy()
            mean, var = m32.to(DEV), v32.to(DEV)
        else:          # zero rows: neither pointer is read
            mean = var = None
        want_g[r, 2 * C] = float(n)
        _n.check(lib.wsis_bn_sync_pack(_n.ptr(mean), _n.ptr(var), n, C, _n.ptr(gathered[r]), st), "bn_sync_pack")
    assert np.array_equal(gathered.cpu().numpy(), want_g), "pack"
    gt = torch.Generator().manual_seed(3)
    rm0, rv0 = torch.randn(C, generator=gt) * 0.2, torch.rand(C, generator=gt) + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    mean, var = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    count = torch.full((1,), NAN, dtype=torch.float64, device=DEV)
    _n.check(lib.wsis_bn_sync_combine(_n.ptr(gathered), R, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm), _n.ptr(rv), mom,
                                      _n.ptr(count), st), "bn_sync_combine")
    w_mean, w_var, w_N = _combine_ref(want_g, C)
    N = sum(counts)
    assert float(count) == w_N == float(N), "count"
    assert np.array_equal(mean.cpu().numpy(), w_mean), "mean"
    assert np.array_equal(var.cpu().numpy(), w_var), "var"
    # without the running pair: the same mean / var, nothing else written
    mean_b, var_b = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    _n.check(lib.wsis_bn_sync_combine(_n.ptr(gathered), R, C, _n.ptr(mean_b), _n.ptr(var_b), None, None, mom, _n.ptr(count),
                                      st), "bn_sync_combine")
    assert _same(mean_b, mean) and _same(var_b, var)
    if N == 0:
        assert _same(rm.cpu(), rm0) and _same(rv.cpu(), rv0), "no rows anywhere: the running statistics stay"
        return
    if kind == "offset":      # the ranks' means differ, and by far less than their size
        assert len({float(v) for v in want_g[:, 0] if v != 0}) > 1 and float(mean.abs().min()) > 900 * float(var.max()) ** 0.5
    if N >= 2:      # (torch's BatchNorm1d wants two rows)
        bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=mom).double()
        with torch.no_grad():
            bn.running_mean.copy_(rm0.double())
            bn.running_var.copy_(rv0.double())
        bn(torch.cat(rows).double())
        assert torch.allclose(rm.cpu().double(), bn.running_mean, rtol=1e-5, atol=1e-6), "running_mean"
        assert torch.allclose(rv.cpu().double(), bn.running_var, rtol=1e-5, atol=1e-6), "running_var"
    # backward side: widen the local sums, scale what the all-reduce returned by M / N
    dg, db = torch.randn(C, generator=gt) * 30, torch.randn(C, generator=gt) * 30
    dg_d, db_d = dg.to(DEV), db.to(DEV)
    sums = torch.full((2 * C,), NAN, dtype=torch.float64, device=DEV)
    _n.check(lib.wsis_bn_sync_sums_pack(_n.ptr(dg_d), _n.ptr(db_d), C, _n.ptr(sums), st), "bn_sync_sums_pack")
    want_s = np.concatenate([dg.double().numpy(), db.double().numpy()])
    assert np.array_equal(sums.cpu().numpy(), want_s), "sums_pack"
    _n.check(lib.wsis_bn_sync_sums_pack(None, None, C, _n.ptr(sums), st), "bn_sync_sums_pack")
    assert np.array_equal(sums.cpu().numpy(), np.zeros(2 * C)), "sums_pack of a rank without rows"
    total = torch.from_numpy(want_s * 1.75 + 0.125).to(DEV)      # (stands for the sum over the ranks)
    for M in sorted(set(c for c in counts if c > 0)):
        a, b = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
        _n.check(lib.wsis_bn_sync_sums_scale(_n.ptr(total), M, _n.ptr(count), C, _n.ptr(a), _n.ptr(b), st), "bn_sync_sums_scale")
        want = (total.cpu().numpy() * (np.float64(M) / w_N)).astype(np.float32)
        assert np.array_equal(a.cpu().numpy(), want[:C]) and np.array_equal(b.cpu().numpy(), want[C:]), f"sums_scale M {M}"


# ---- (c) a world of one ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world_of_one(tmp_path_factory):
    import torch.distributed as dist
    assert not dist.is_initialized()
    store = tmp_path_factory.mktemp("pg") / "store"
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=0, world_size=1)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def _input(batch, cfg):
    import pointgroup_ops
    feats = batch["feats"]
    if cfg.model.use_coords:
        feats = torch.cat((feats, batch["locs_float"]), 1)
    vf = pointgroup_ops.voxelization(feats, batch["v2p_map"], cfg.mode)
    return spconv.SparseConvTensor(vf, batch["voxel_coords_int"], batch["spatial_shape"], max(int(cfg.batch_size), 1))


def _bns(model):
    return [m for mod in (model.unet, model.output_layer) for m in mod.modules() if isinstance(m, torch.nn.BatchNorm1d)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_world_of_one_equals_the_unsynced_pass(dt, world_of_one):
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([harness.make_scene(0, room=(1.2, 1.0, 0.8), n_box=1)]), DEV)
    model, _, _ = harness.build_model(cfg, DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        for m in _bns(model):
            m.running_mean.copy_(torch.randn(m.num_features, device=DEV, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, device=DEV, generator=g) + 0.5)
            m.weight.copy_(torch.rand(m.num_features, device=DEV, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.num_features, device=DEV, generator=g) * 0.1)
    model.train()
    wsis_ops.flush_bn_counters(model)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    d_out = None
    res = []
    for group in (None, world_of_one):
        wsis_ops.flush_bn_counters(model)
        model.load_state_dict(state)
        for p in model.parameters():
            p.grad = None
        inp = _input(batch, cfg)
        inp.features.requires_grad_(True)
        out = un.run_unet_lp_train(model, inp, dt, dt, sync_group=group)
        prog = model._native_prog
        assert (prog.bn_sync is not None) == (group is not None)
        if d_out is None:
            d_out = (torch.randn(out.shape, device=DEV, generator=g) * 0.01).to(dt)
        out.backward(d_out)
        torch.cuda.synchronize()
        res.append((out.detach().clone(), inp.features.grad.clone(), [p.grad.clone() for p in prog.params],
                    [m.running_mean.clone() for m in _bns(model)]))
    (o_a, dx_a, g_a, rm_a), (o_b, dx_b, g_b, rm_b) = res
    assert bool(torch.isfinite(o_a.float()).all()) and float(o_a.float().abs().max()) > 0
    assert _same(o_b, o_a), f"output: {int((o_a != o_b).sum())} of {o_a.numel()} elements differ"
    assert _same(dx_b, dx_a), "input gradient"
    assert len(g_a) == len(g_b) > 100
    for i, (a, b) in enumerate(zip(g_a, g_b)):
        assert bool(torch.isfinite(a).all()) and _same(b, a), f"gradient of parameter {i} {tuple(a.shape)}"
    for i, (a, b, m) in enumerate(zip(rm_a, rm_b, _bns(model))):
        assert torch.allclose(b, a, rtol=1e-5, atol=1e-6), f"running_mean of BatchNorm {i}"
        assert not torch.equal(b, state_of(state, model, m)), f"BatchNorm {i}: running mean not updated"


def state_of(state, model, module):
    return state[next(k for k, m in model.named_modules() if m is module) + ".running_mean"]
