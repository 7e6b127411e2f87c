"""GPU: the 16-bit native TRAINING pass of the UNet (WSIS_NATIVE_LP_TRAIN=1) and the kernels it adds.

1. wsis_bn_stats_lp equals wsis_bn_stats of the widened x bit for bit (mean, var, both running statistics) on both sides
   of the one-launch / two-launch threshold, at ragged workgroups and at |mean| >> sigma.
2. wsis_bn_bwd_lp: dgamma / dbeta equal wsis_bn_bwd of the widened inputs bit for bit; dx is that call's fp32 dx rounded once
   (or unrounded with out_fp32).
3. The executor's forward + backward pass equals, bit for bit, the same sequence of single-op calls (output, every saved
   mean / var, every running statistic, every parameter gradient, the input gradient).
4. Network.forward takes the pass only when the switch, the dtype, gradient mode, training-mode BatchNorm, fp32
   parameters and the absence of a SyncBatchNorm group allow; a frozen parameter gets no gradient.
5. Two runs of three optimizer steps from one seed give identical bytes.
6. Accuracy against the fp32 native pass, with the module walk under autocast as the yardstick.

   Measured on one MI355X (small scene, model after three fp32 steps, one fixed gradient of the UNet output; error of the
   output = relative Frobenius error, of a gradient = 1 - cosine per parameter, both against the fp32 native pass;
   native / walk and their ratio):
     bf16  output 3.61e-3 / 4.31e-3 (0.84); gradient median 7.06e-4 / 9.70e-4 (0.73), worst 6.32e-3 / 6.77e-3 (0.93)
     fp16  output 4.17e-4 / 4.70e-4 (0.89); gradient median 2.52e-4 / 2.88e-4 (0.87), worst 1.74e-1 / 1.69e-1 (1.03)
   The largest ratio is 1.03: the bound is the first step of the 1.25 / 1.5 / 2 ladder.
"""
import numpy as np
import pytest
import torch

import harness
import spconv
import unet_native as un
import wsis_native as _n
import wsis_ops
import wsis_parallel
from spconv import ops as sp_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
CODE = {torch.bfloat16: 0, torch.float16: 1}
NAN = float("nan")
EPS = 1e-4
# the one-launch form up to 4096 rows and its boundary; one full + one ragged workgroup of the partial kernel at every C
# (a workgroup takes 256 / (C / 4) * 8 rows: 256 at C = 32, 64 at C = 256); many workgroups
ROWS = (1, 2, 255, 4096, 4097, 4353, 9001)
CHANNELS = (32, 96, 160, 256)
WALK_FACTOR = 1.25      # see the module docstring


def _ws(M, C):
    wsb = _n.hip().wsis_bn_workspace_bytes(M, C)
    return torch.full((wsb // 4 + 1,), NAN, device=DEV), wsb


def _inputs(M, C, kind, dt, g):
    if kind == "offset":      # |mean| = 500 sigma: the shifted sums matter
        x = 50.0 + 0.1 * torch.randn(M, C, device=DEV, generator=g)
    else:                     # one channel with all rows equal (variance exactly 0), the rest plain
        x = torch.randn(M, C, device=DEV, generator=g) * 2 + 0.3
        x[:, C // 2] = 1.375
    return x.to(dt)


# ---- 1. statistics -------------------------------------------------------------------------------------------------

def _stats32(x, rm, rv, mom):
    M, C = x.shape
    mean, var = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    ws, wsb = _ws(M, C)
    _n.check(_n.hip().wsis_bn_stats(_n.ptr(x), M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm), _n.ptr(rv), mom, _n.ptr(ws), wsb,
                                    _n.stream_ptr()), "bn_stats")
    return mean, var


def _stats_lp(x, rm, rv, mom):
    M, C = x.shape
    mean, var = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    ws, wsb = _ws(M, C)
    _n.check(_n.hip().wsis_bn_stats_lp(_n.ptr(x), M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm), _n.ptr(rv), mom, _n.ptr(ws),
                                       wsb, CODE[x.dtype], _n.stream_ptr()), "bn_stats_lp")
    return mean, var


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", CHANNELS)
def test_bn_stats_lp_equals_fp32_kernel_on_widened_input(C, dt):
    g = torch.Generator(device=DEV).manual_seed(C)
    for M in ROWS:
        for kind in ("offset", "flat_channel"):
            x = _inputs(M, C, kind, dt, g)
            rm0 = torch.randn(C, device=DEV, generator=g)
            rv0 = torch.rand(C, device=DEV, generator=g) + 0.5
            rm_a, rv_a, rm_b, rv_b = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
            mean_a, var_a = _stats32(x.float(), rm_a, rv_a, 0.1)
            mean_b, var_b = _stats_lp(x, rm_b, rv_b, 0.1)
            what = f"M {M} C {C} {kind} {dt}"
            assert bool(torch.isfinite(mean_b).all()) and bool(torch.isfinite(var_b).all()), what
            assert _same(mean_b, mean_a), what + ": mean"
            assert _same(var_b, var_a), what + ": var"
            assert _same(rm_b, rm_a) and _same(rv_b, rv_a), what + ": running statistics"
            assert not _same(rm_b, rm0) or M == 0, what + ": running statistics untouched"
            if kind == "flat_channel" and M > 1:
                assert float(var_b[C // 2]) == 0.0 and float(mean_b[C // 2]) == 1.375, what
            # without running statistics: same mean / var
            mean_c, var_c = _stats_lp(x, None, None, 0.1)
            assert _same(mean_c, mean_a) and _same(var_c, var_a), what + ": no running statistics"


# ---- 2. backward ---------------------------------------------------------------------------------------------------

def _bwd32(x, dy, mean, var, gamma, beta, relu, training, addend, want_dx=True):
    M, C = x.shape
    dx = torch.full((M, C), NAN, device=DEV) if want_dx else None
    dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    ws, wsb = _ws(M, C)
    _n.check(_n.hip().wsis_bn_bwd(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta), EPS, relu,
                                  training, _n.ptr(dx), _n.ptr(dg), _n.ptr(db), _n.ptr(addend), M, C, _n.ptr(ws), wsb,
                                  _n.stream_ptr()), "bn_bwd")
    return dx, dg, db


def _bwd_lp(x, dy, mean, var, gamma, beta, relu, training, addend, out_dtype):
    """out_dtype None: d_dx == NULL"""
    M, C = x.shape
    dx = torch.full((M, C), NAN, dtype=out_dtype, device=DEV) if out_dtype is not None else None
    dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    ws, wsb = _ws(M, C)
    _n.check(_n.hip().wsis_bn_bwd_lp(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta), EPS, relu,
                                     training, _n.ptr(dx), int(out_dtype == torch.float32), _n.ptr(dg), _n.ptr(db),
                                     _n.ptr(addend), M, C, CODE[x.dtype], _n.ptr(ws), wsb, _n.stream_ptr()), "bn_bwd_lp")
    return dx, dg, db


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", CHANNELS)
def test_bn_bwd_lp_equals_fp32_kernel_on_widened_inputs(C, dt):
    g = torch.Generator(device=DEV).manual_seed(100 + C)
    rounded_somewhere = False
    for M in ROWS:
        for kind in ("offset", "flat_channel"):
            x = _inputs(M, C, kind, dt, g)
            dy = torch.randn(M, C, device=DEV, generator=g).to(dt)
            add = (torch.randn(M, C, device=DEV, generator=g) * 0.5).to(dt)
            mean, var = _stats_lp(x, None, None, 0.1)
            gamma = torch.randn(C, device=DEV, generator=g)
            beta = torch.randn(C, device=DEV, generator=g) * 0.3
            for relu in (0, 1):
                for training in (0, 1):
                    for addend in (None, add):
                        ref_dx, ref_dg, ref_db = _bwd32(x.float(), dy.float(), mean, var, gamma, beta, relu, training,
                                                        None if addend is None else addend.float())
                        what = f"M {M} C {C} {kind} relu {relu} training {training} addend {addend is not None} {dt}"
                        dx16, dg, db = _bwd_lp(x, dy, mean, var, gamma, beta, relu, training, addend, dt)
                        assert _same(dg, ref_dg) and _same(db, ref_db), what + ": dgamma / dbeta"
                        assert torch.equal(dx16.view(torch.int16), ref_dx.to(dt).view(torch.int16)), what + ": 16-bit dx"
                        dx32, dg, db = _bwd_lp(x, dy, mean, var, gamma, beta, relu, training, addend, torch.float32)
                        assert _same(dg, ref_dg) and _same(db, ref_db), what + ": dgamma / dbeta (fp32 dx)"
                        assert _same(dx32, ref_dx), what + ": fp32 dx"
                        rounded_somewhere |= not torch.equal(dx16.float(), dx32)
            # d_dx == NULL, affine parameters absent: the reductions alone
            ref = _bwd32(x.float(), dy.float(), mean, var, None, None, 1, 1, None, want_dx=False)
            got = _bwd_lp(x, dy, mean, var, None, None, 1, 1, None, None)
            assert _same(got[1], ref[1]) and _same(got[2], ref[2]), f"M {M} C {C} {kind} {dt}: reductions without dx"
    assert rounded_somewhere, "the 16-bit dx never differed from the fp32 one: the comparison shows nothing"


# ---- shared scenes and models ----------------------------------------------------------------------------------------

def _scene(kind):
    if kind == "small":
        return harness.make_scene(0, room=(3.0, 3.0, 2.4), n_box=2, max_points=10000)
    return harness.bench_scene(1)


def _input(batch, cfg, dtype=None):
    import pointgroup_ops
    feats = batch["feats"]
    if cfg.model.use_coords:
        feats = torch.cat((feats, batch["locs_float"]), 1)
    vf = pointgroup_ops.voxelization(feats, batch["v2p_map"], cfg.mode)
    if dtype is not None:
        vf = vf.to(dtype)
    return spconv.SparseConvTensor(vf, batch["voxel_coords_int"], batch["spatial_shape"], max(int(cfg.batch_size), 1))


def _unet_modules(model):
    return [m for mod in (model.input_conv, model.unet, model.output_layer) for m in mod.modules()]


def _bns(model):
    return [m for m in _unet_modules(model) if isinstance(m, torch.nn.BatchNorm1d)]


def _snapshot(model):
    wsis_ops.flush_bn_counters(model)
    return {k: v.clone() for k, v in model.state_dict().items()}


def _restore(model, state):
    wsis_ops.flush_bn_counters(model)
    model.load_state_dict(state)
    for p in model.parameters():
        p.grad = None


_CACHE = {}


def _trained(steps=3):
    """(model, criterion, batch, cfg, state): the small scene and a model after a few fp32 training steps (running
    statistics and affine parameters that are not the initial ones), in training mode; made once, every user restores
    ``state`` when it is done"""
    if "trained" not in _CACHE:
        cfg = harness.default_cfg()
        batch = harness.to_device(harness.collate([_scene("small")]), DEV)
        model, crit, opt = harness.build_model(cfg, DEV)
        for _ in range(steps):
            harness.train_step(model, crit, opt, batch, cfg)
        model.train()
        _CACHE["trained"] = (model, crit, batch, cfg, _snapshot(model))
    return _CACHE["trained"]


# ---- 3. executor = single-op replay ----------------------------------------------------------------------------------

class _Replay(object):
    """an emitter for the recorder's own walk (unet_native._ublock) that RUNS every step with the single-op entry points:
    handles are tensors, the closures run the backward calls.  Same order of calls as the recorded lists."""

    def __init__(self, prog, dt):
        self.tt, self.Mv, self.dt, self.code = prog.table_tensors, prog.Mvec, dt, CODE[dt]
        self.lib, self.st = _n.hip(), _n.stream_ptr()
        self.grads, self.stats, self.first = {}, [], None

    def _t(self, slot):
        return self.tt[slot & un._ID_MASK] if slot else None

    def conv(self, x, m, table, lvl_in, lvl_out, residual=0, stats=True):
        K, Cin, Cout = int(np.prod(m.kernel_size)), m.in_channels, m.out_channels
        W = m.weight.detach().view(K, Cin, Cout)
        t = table if table is not None else un._Table()
        nbr_f, order_f, nbr_b, order_b = (self._t(s) for s in t[:4])
        M_out = int(self.Mv[lvl_out])
        y = torch.full((M_out, Cout), NAN, dtype=self.dt, device=DEV)
        WT = sp_ops._weight_lp(W, self.dt, 1, 0)
        _n.check(self.lib.wsis_spconv_fwd_lp_res(_n.ptr(x), _n.ptr(nbr_f), _n.ptr(order_f), _n.ptr(WT), 0, None,
                                                 _n.ptr(residual if torch.is_tensor(residual) else None), _n.ptr(y),
                                                 x.shape[0], M_out, K, Cin, Cout, self.code, None, 256, self.st), "fwd_lp_res")

        def bwd(dy):
            dx = sp_ops._conv_lp(dy, nbr_b, order_b, sp_ops._weight_lp(W, self.dt, 0, 0), t.flip, None, x.shape[0])
            self.grads[m.weight] = sp_ops._dw_lp(x, nbr_f, order_f, dy, K, Cin, Cout).view(m.weight.shape)
            return dx
        return y, bwd

    def bn_relu(self, x, bn, lvl, relu=True, fuse=False, out_dtype=None):
        M, C = x.shape
        mean, var = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
        ws, wsb = _ws(M, C)
        _n.check(self.lib.wsis_bn_stats_lp(_n.ptr(x), M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(bn.running_mean),
                                           _n.ptr(bn.running_var), bn.momentum, _n.ptr(ws), wsb, self.code, self.st), "stats")
        y = torch.full((M, C), NAN, dtype=out_dtype or self.dt, device=DEV)
        _n.check(self.lib.wsis_bn_apply_lp(_n.ptr(x), _n.ptr(mean), _n.ptr(var), _n.ptr(bn.weight), _n.ptr(bn.bias), bn.eps,
                                           int(relu), _n.ptr(y), int(y.dtype == torch.float32), M, C, self.code, self.st),
                 "apply")
        self.stats.append((mean, var))

        def bwd(dy, addend=0):
            f32 = x is self.first
            dx = torch.full((M, C), NAN, dtype=torch.float32 if f32 else self.dt, device=DEV)
            dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
            _n.check(self.lib.wsis_bn_bwd_lp(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(bn.weight),
                                             _n.ptr(bn.bias), bn.eps, int(relu), 1, _n.ptr(dx), int(f32), _n.ptr(dg), _n.ptr(db),
                                             _n.ptr(addend if torch.is_tensor(addend) else None), M, C, self.code, _n.ptr(ws),
                                             wsb, self.st), "bn_bwd_lp")
            self.grads[bn.weight], self.grads[bn.bias] = dg, db
            return dx
        return y, bwd

    def cat(self, a, b, lvl, C0):
        return torch.cat((a, b), 1), lambda d: (d[:, :C0].contiguous(), d[:, C0:].contiguous())


def _replay(model, inp, dt, out_dtype, d_out, need_dx):
    prog = model._native_prog
    em = _Replay(prog, dt)
    c0 = model.input_conv[0]
    rb = inp.indice_dict["subm1"]
    W0 = c0.weight.detach().contiguous().view(-1, c0.in_channels, c0.out_channels)
    x32 = inp.features.detach().to(dt).float().contiguous()
    y = em.first = sp_ops._fwd_fp32(x32, rb.nbr_p, rb.order, W0, None, int(prog.Mvec[0])).to(dt)
    u, b_u = un._ublock(em, y, model.unet, 0)
    out, b_out = em.bn_relu(u, model.output_layer[0], 0, out_dtype=out_dtype)
    d32 = b_u(b_out(d_out.to(dt).contiguous()))
    assert d32.dtype == torch.float32
    K0 = W0.shape[0]
    em.grads[c0.weight] = sp_ops._dw(x32, rb.nbr_p, rb.order, d32, K0, c0.in_channels, c0.out_channels).view(c0.weight.shape)
    dx = sp_ops._din_fp32(d32, rb.nbr_p, rb.order, W0, 1, x32.shape[0]) if need_dx else None
    return out, em.stats, em.grads, dx


def _saved_stats(out):
    """(mean, var) of every BatchNorm op of the pass that produced ``out``, from the arena its backward node keeps"""
    node = out.grad_fn
    ops = node.c.fwd.instantiate(node.Mvec, un._luts(node.fwd_lut, node.table_lut, 0, 0))
    base = node.arena.data_ptr()
    res = []
    for o in ops[ops["kind"] == un.OP_BN_RELU]:
        C = int(o["Cin"])
        res.append(tuple(node.arena[int(p) - base:int(p) - base + 4 * C].view(torch.float32).clone() for p in o["out"][1:3]))
    return res


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("scene", ["small", "c2"])
def test_executor_equals_single_op_replay(scene, dt):
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene(scene)]), DEV)
    model, _, _ = harness.build_model(cfg, DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        for m in _bns(model):
            m.running_mean.copy_(torch.randn(m.num_features, device=DEV, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, device=DEV, generator=g) + 0.5)
            m.weight.copy_(torch.rand(m.num_features, device=DEV, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.num_features, device=DEV, generator=g) * 0.1)
    model.train()
    state = _snapshot(model)
    out_dtype = torch.float32 if dt == torch.bfloat16 else dt      # both forms of the output layer over the two dtypes
    inp = _input(batch, cfg)
    # (both scenes have BatchNorm layers on either side of the one-launch threshold: level 0 above 4096 rows, the deep
    # levels below; c2 adds levels of many workgroups)
    assert inp.features.shape[0] > 4096
    inp.features.requires_grad_(True)
    got = un.run_unet_lp_train(model, inp, dt, out_dtype)
    assert got.dtype == out_dtype and bool(torch.isfinite(got).all())
    d_out = torch.randn(got.shape, device=DEV, generator=g) * 0.01
    stats = _saved_stats(got)
    got.backward(d_out.to(got.dtype))
    torch.cuda.synchronize()
    params = model._native_prog.params
    grads = [p.grad.clone() for p in params]
    dx = inp.features.grad.clone()
    running = [(m.running_mean.clone(), m.running_var.clone()) for m in _bns(model)]
    assert all(bool(torch.isfinite(t).all()) for t in grads + [dx])
    _restore(model, state)
    with torch.no_grad():
        want, w_stats, w_grads, w_dx = _replay(model, inp, dt, out_dtype, d_out.to(got.dtype), True)
    torch.cuda.synchronize()
    assert torch.equal(got.detach().view(torch.uint8), want.view(torch.uint8)), \
        f"output: {int((got != want).sum())} of {got.numel()} elements differ"
    assert len(stats) == len(w_stats) == len(_bns(model))
    for i, ((m_a, v_a), (m_b, v_b)) in enumerate(zip(stats, w_stats)):
        assert _same(m_a, m_b) and _same(v_a, v_b), f"saved statistics of BatchNorm op {i}"
    for i, (m, (rm, rv)) in enumerate(zip(_bns(model), running)):
        assert _same(m.running_mean, rm) and _same(m.running_var, rv), f"running statistics of BatchNorm {i}"
        assert not _same(rm, state_of(state, model, m, "running_mean")), f"BatchNorm {i}: running mean not updated"
    assert len(w_grads) == len(params)
    for i, (p, gr) in enumerate(zip(params, grads)):
        assert gr.dtype == torch.float32 and _same(gr, w_grads[p]), f"gradient of parameter {i} {tuple(p.shape)}"
    assert _same(dx, w_dx), "input gradient"


def state_of(state, model, module, name):
    key = next(k for k, m in model.named_modules() if m is module) + "." + name
    return state[key]


# ---- 4. dispatch ---------------------------------------------------------------------------------------------------

class _Stop(Exception):
    pass


def _extra(batch):
    from torch_scatter import scatter
    centre = scatter(batch["locs_float"], batch["superpoint"], dim=0, reduce="mean", csr=batch.get("superpoint_csr"))
    return {"superpoint": batch["superpoint"], "GIs": batch["GIs"], "edge_u_list": batch["edge_u_list"],
            "edge_v_list": batch["edge_v_list"], "superpoint_cenetr_xyz": centre,
            "superpoint_csr": batch.get("superpoint_csr"), "edge_graph": batch.get("edge_graph"),
            "p2v_csr": batch.get("p2v_csr"), "edge_src_rows": batch.get("edge_src_rows")}


def _chosen(model, batch, cfg, monkeypatch, feat_dtype=None):
    """the pass Network.forward chooses -- stopped before any of the three UNet paths runs"""
    def stop(*a, **k):
        raise _Stop()
    with monkeypatch.context() as mp:
        for name in ("run_unet", "run_unet_lp", "run_unet_lp_train"):
            mp.setattr(un, name, stop)
        mp.setattr(model.input_conv, "forward", stop, raising=False)
        with pytest.raises(_Stop):
            model(_input(batch, cfg, feat_dtype), batch["p2v_map"], _extra(batch))
    return model.last_pass


def test_dispatch(monkeypatch):
    model, crit, batch, cfg, state = _trained()
    for k in ("WSIS_NATIVE_LP", "WSIS_NATIVE_LP_TRAIN", "WSIS_NATIVE_UNET"):
        monkeypatch.delenv(k, raising=False)
    try:
        for dt in DTYPES:
            for mode in ("autocast", "features"):
                def run():
                    with torch.autocast("cuda", dtype=dt, enabled=mode == "autocast"):
                        return _chosen(model, batch, cfg, monkeypatch, dt if mode == "features" else None)
                monkeypatch.delenv("WSIS_NATIVE_LP_TRAIN", raising=False)
                assert run() == "modules", (dt, mode, "switch unset")
                monkeypatch.setenv("WSIS_NATIVE_LP", "1")
                assert run() == "modules", (dt, mode, "the inference switch does not select the training pass")
                monkeypatch.delenv("WSIS_NATIVE_LP")
                monkeypatch.setenv("WSIS_NATIVE_LP_TRAIN", "1")
                assert run() == "native_lp_train", (dt, mode)
                monkeypatch.setenv("WSIS_NATIVE_UNET", "0")
                assert run() == "modules", "WSIS_NATIVE_UNET=0 walks the modules"
                monkeypatch.delenv("WSIS_NATIVE_UNET")
                with torch.no_grad():
                    assert run() == "modules", (dt, mode, "no_grad")
        monkeypatch.setenv("WSIS_NATIVE_LP_TRAIN", "1")
        bf = torch.autocast("cuda", dtype=torch.bfloat16)
        # fp32 features outside autocast: the fp32 native pass as before
        assert _chosen(model, batch, cfg, monkeypatch) == "native"
        # one BatchNorm layer in evaluation mode
        model.unet.u.blocks.block1.conv_branch[3].eval()
        with bf:
            assert _chosen(model, batch, cfg, monkeypatch) == "modules"
        model.train()
        # a SyncBatchNorm group
        with monkeypatch.context() as mp, bf:
            mp.setattr(wsis_parallel, "sync_batchnorm_active", lambda m: True)
            assert _chosen(model, batch, cfg, monkeypatch) == "modules"
        # evaluation mode with gradients: the walk; without: the inference pass's business
        model.eval()
        with bf:
            assert _chosen(model, batch, cfg, monkeypatch) == "modules"
        model.train()
        with bf:
            assert _chosen(model, batch, cfg, monkeypatch) == "native_lp_train"
        # a model with 16-bit parameters
        m16, _, _ = harness.build_model(cfg, DEV)
        m16 = m16.to(torch.bfloat16).train()
        assert _chosen(m16, batch, cfg, monkeypatch, torch.bfloat16) == "modules"
    finally:
        model.train()
        _restore(model, state)


def _fwd_bwd(model, crit, batch, cfg, dt):
    with torch.autocast("cuda", dtype=dt):
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
    for p in model.parameters():
        p.grad = None
    loss.backward()
    return loss.detach()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_whole_step_and_frozen_parameter(dt, monkeypatch):
    model, crit, batch, cfg, state = _trained()
    monkeypatch.delenv("WSIS_NATIVE_UNET", raising=False)
    try:
        monkeypatch.delenv("WSIS_NATIVE_LP_TRAIN", raising=False)
        loss_walk = _fwd_bwd(model, crit, batch, cfg, dt)
        assert model.last_pass == "modules"
        _restore(model, state)
        monkeypatch.setenv("WSIS_NATIVE_LP_TRAIN", "1")
        loss = _fwd_bwd(model, crit, batch, cfg, dt)
        assert model.last_pass == "native_lp_train"
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(loss_walk))
        print(f"{dt}: loss of the step: walk {float(loss_walk):.6f}, native_lp_train {float(loss):.6f}")
        named = dict(model.named_parameters())
        grads = {k: p.grad.clone() for k, p in named.items() if p.grad is not None}
        unet = {k for k in named if k.startswith(("input_conv.", "unet.", "output_layer."))}
        assert unet <= set(grads), "every UNet parameter has a gradient"
        assert all(grads[k].dtype == torch.float32 and bool(torch.isfinite(grads[k]).all()) for k in unet)
        # num_batches_tracked follows (deferred on the host, written when the state is read)
        before = {k: int(v) for k, v in state.items() if k.endswith("num_batches_tracked") and k.split(".")[0] in ("unet", "output_layer")}
        after = _snapshot(model)
        assert before and all(int(after[k]) == v + 1 for k, v in before.items())
        # frozen: one convolution weight and one BatchNorm's affine pair
        _restore(model, state)
        frozen = ["unet.u.blocks.block0.conv_branch.2.weight", "unet.blocks.block1.conv_branch.0.weight",
                  "unet.blocks.block1.conv_branch.0.bias"]
        for k in frozen:
            named[k].requires_grad_(False)
        loss2 = _fwd_bwd(model, crit, batch, cfg, dt)
        assert model.last_pass == "native_lp_train"
        assert torch.equal(loss2, loss)
        for k, p in named.items():
            if k in frozen:
                assert p.grad is None, k
            elif k in grads:
                assert p.grad is not None and torch.equal(p.grad, grads[k]), k
    finally:
        for p in model.parameters():
            p.requires_grad_(True)
        _restore(model, state)


# ---- 5. reproducibility --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_three_steps_twice_identical_bytes(dt, monkeypatch):
    monkeypatch.setenv("WSIS_NATIVE_LP_TRAIN", "1")
    monkeypatch.delenv("WSIS_NATIVE_UNET", raising=False)
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene("small")]), DEV)
    runs = []
    for _ in range(2):
        model, crit, opt = harness.build_model(cfg, DEV)
        model.train()
        losses = []
        for _ in range(3):
            with torch.autocast("cuda", dtype=dt):
                loss, _ = harness.forward_loss(model, crit, batch, cfg)
            assert model.last_pass == "native_lp_train"
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        runs.append((torch.stack(losses), _snapshot(model)))
    (l_a, s_a), (l_b, s_b) = runs
    assert bool(torch.isfinite(l_a).all())
    assert torch.equal(l_a.view(torch.int32), l_b.view(torch.int32)), (l_a.tolist(), l_b.tolist())
    for k in s_a:
        assert torch.equal(s_a[k].reshape(-1).view(torch.uint8), s_b[k].reshape(-1).view(torch.uint8)), k
    tracked = [k for k in s_a if k.endswith("num_batches_tracked") and k.split(".")[0] in ("unet", "output_layer")]
    assert tracked and all(int(s_a[k]) == 3 for k in tracked)
    fresh, _, _ = harness.build_model(cfg, DEV)
    assert not torch.equal(s_a["unet.blocks.block0.conv_branch.2.weight"], fresh.state_dict()["unet.blocks.block0.conv_branch.2.weight"])


# ---- 6. accuracy against the fp32 native pass ----------------------------------------------------------------------

def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def _one_minus_cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(1.0 - (a @ b) / (a.norm() * b.norm()))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_accuracy_against_fp32_native_pass(dt):
    model, crit, batch, cfg, state = _trained()
    params = un._program(model).params
    G = torch.randn((int(_input(batch, cfg).features.shape[0]), model.output_layer[0].num_features), device=DEV,
                    generator=torch.Generator(device=DEV).manual_seed(11)) * 0.01

    def run(kind):
        _restore(model, state)
        inp = _input(batch, cfg)
        if kind == "fp32":
            out = un.run_unet(model, inp)
        elif kind == "native":
            out = un.run_unet_lp_train(model, inp, dt, dt)
        else:
            with torch.autocast("cuda", dtype=dt):
                out = model.output_layer(model.unet(model.input_conv(inp))).features
            sp_ops.verify_pending_counts()
        out.backward(G.to(out.dtype))
        return out.detach().clone(), [p.grad.detach().clone().float() for p in params]
    try:
        o32, g32 = run("fp32")
        o_n, g_n = run("native")
        o_w, g_w = run("walk")
    finally:
        _restore(model, state)
    e_n, e_w = _rel(o_n, o32), _rel(o_w, o32)
    c_n = np.array([_one_minus_cos(a, b) for a, b in zip(g_n, g32)])
    c_w = np.array([_one_minus_cos(a, b) for a, b in zip(g_w, g32)])
    print(f"{dt}: UNet output rel. Frobenius error native {e_n:.3e}, walk {e_w:.3e}, ratio {e_n / e_w:.3f}")
    print(f"{dt}: 1 - cos of {len(params)} parameter gradients: median native {np.median(c_n):.3e}, walk {np.median(c_w):.3e}, "
          f"ratio {np.median(c_n) / np.median(c_w):.3f}; worst native {c_n.max():.3e}, walk {c_w.max():.3e}, "
          f"ratio {c_n.max() / c_w.max():.3f}")
    assert e_w > 0 and np.median(c_w) > 0, "the walk is as exact as fp32: the yardstick shows nothing"
    assert e_n <= WALK_FACTOR * e_w, (e_n, e_w)
    assert np.median(c_n) <= WALK_FACTOR * np.median(c_w), (np.median(c_n), np.median(c_w))
    assert c_n.max() <= WALK_FACTOR * c_w.max(), (c_n.max(), c_w.max())
