"""GPU: the 16-bit evaluation-mode native UNet pass (WSIS_NATIVE_LP=1) and the kernels it adds.

1. wsis_spconv_fwd_lp_res: the residual joins acc + bias before the ONE rounding (exact integer-grain operands of
   tests/lowp_exact.py, torch.equal against round-to-nearest-even of the fp64 sum).  (wsis_spconv_fwd_lp forwards to it
   with a NULL residual; its unchanged bits are pinned by tests/test_gpu_lowp_exact.py.)
2. wsis_bn_apply_lp: the fp32 arithmetic of wsis_bn_apply on the widened input, rounded once (or stored as fp32).
3. A 16-bit CAT op copies bits (torch.cat).
4. The executor's pass equals, bit for bit, the same sequence of single-op calls made from the module tree.
5. Network.forward takes the pass only when the switch, the dtype, no-gradient mode and evaluation-mode BatchNorm allow,
   and returns the dtype the module walk returns.
6. Accuracy against the fp32 native pass after a few fp32 training steps, and reproducibility."""
import numpy as np
import pytest
import torch

import harness
import spconv
import unet_native as un
import wsis_native as _n
from spconv import ops as sp_ops

import conv_ref
import lowp_exact as lx
from lowp_exact import lp_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
CODE = {torch.bfloat16: 0, torch.float16: 1}
NAN = float("nan")
XE, WE = -4, -5
GRAIN = 2.0 ** (XE + WE)


# ---- 1. residual epilogue ------------------------------------------------------------------------------------------

def _fwd_res(X, nbr, order, WT, flip, bias, res, M_out, dt):
    K, Cout, Cin = WT.shape
    out = torch.full((M_out, Cout), NAN, dtype=dt, device=DEV)
    lib = _n.hip()
    wsb = lib.wsis_spconv_fwd_lp_workspace_bytes(M_out, K, Cin, Cout)
    ws = torch.full((max(wsb, 256) // 4 + 1,), NAN, device=DEV)
    _n.check(lib.wsis_spconv_fwd_lp_res(_n.ptr(X), _n.ptr(nbr), _n.ptr(order), _n.ptr(WT), flip, _n.ptr(bias),
                                        _n.ptr(res), _n.ptr(out), X.shape[0], M_out, K, Cin, Cout, CODE[dt], _n.ptr(ws),
                                        wsb, _n.stream_ptr()), "spconv_fwd_lp_res")
    return out


def _fwd_plain(X, nbr, order, WT, flip, bias, M_out, dt):
    K, Cout, Cin = WT.shape
    out = torch.full((M_out, Cout), NAN, dtype=dt, device=DEV)
    lib = _n.hip()
    wsb = lib.wsis_spconv_fwd_lp_workspace_bytes(M_out, K, Cin, Cout)
    _n.check(lib.wsis_spconv_fwd_lp(_n.ptr(X), _n.ptr(nbr), _n.ptr(order), _n.ptr(WT), flip, _n.ptr(bias), _n.ptr(out),
                                    X.shape[0], M_out, K, Cin, Cout, CODE[dt], None, wsb, _n.stream_ptr()),
             "spconv_fwd_lp")
    return out


# id: (M_out, K, Cin, Cout, flip, table (False: the dense 1x1 shortcut, nbr = NULL), order, bias, NT)
RES = {
    "k1_dense_nt1": (3001, 1, 64, 32, 0, False, False, True, 1),
    "k1_dense_nt2": (131041, 1, 32, 64, 0, False, True, False, 2),
    "k8_flip_nt1": (4001, 8, 96, 96, 1, True, True, True, 1),
    "k8_flip_nt2": (131041, 8, 32, 64, 1, True, False, True, 2),
    "k27_nt1": (4001, 27, 64, 96, 0, True, True, False, 1),
    "k27_nt2": (65600, 27, 32, 128, 0, True, True, True, 2),
}


def _table(M_in, M_out, K, gen):
    """[K, M_out] packed table; every 5th tile of 32 rows has no pair at all (bias + residual only)"""
    src = torch.randint(0, M_in, (K, M_out), generator=gen)
    take = torch.rand(K, M_out, generator=gen) < 0.6
    take &= ((torch.arange(M_out) // 32) % 5 != 4)[None, :]
    return torch.where(take, src, torch.full_like(src, -1)).int()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(RES))
def test_residual_epilogue_exact(name, dt):
    M_out, K, Cin, Cout, flip, table, use_order, use_bias, nt = RES[name]
    assert lp_plan(M_out, K, Cin, Cout)["nt"] == nt
    seed = sorted(RES).index(name)
    gen = torch.Generator().manual_seed(seed)
    gd = torch.Generator(device=DEV).manual_seed(seed)
    M_in = M_out if not table else M_out + M_out // 3 + 7
    order = torch.randperm(M_out, generator=gen).int().to(DEV) if use_order else None
    R = max(1, min(64, int((2.0 ** 22 / (K * Cin)) ** 0.5)))
    X = lx.ints((M_in, Cin), R, XE, gd).to(dt)
    WT = lx.ints((K, Cout, Cin), R, WE, gd).to(dt)
    bias = lx.ints((Cout,), 1 << 15, XE + WE, gd) if use_bias else None
    # residual: 16-bit values on the grain (rounding a grain multiple to 16 bits keeps it on the grain), up to 2^20 grains
    res = lx.ints((M_out, Cout), 1 << 20, XE + WE, gd).to(dt)
    if table:
        nbr = _table(M_in, M_out, K, gen).to(DEV)
        pairs = []
        for k in range(K):
            t = torch.nonzero(nbr[k] >= 0).flatten()
            pairs.append((nbr[k, t].long(), order.long()[t] if order is not None else t))
    else:
        nbr = None
        t = torch.arange(M_out, device=DEV)
        pairs = [(t, order.long() if order is not None else t)]
    Wref = (WT.flip(0) if flip else WT).transpose(1, 2)
    sel = torch.arange(M_out, device=DEV)
    want = conv_ref.rows(X, Wref, pairs, M_out, sel)
    absref = conv_ref.rows(X.abs(), Wref.abs(), pairs, M_out, sel)
    if bias is not None:
        want, absref = want + bias.double(), absref + bias.double().abs()
    acc_b = want.clone()
    want, absref = want + res.double(), absref + res.double().abs()
    what = f"{name} {dt}"
    exp = lx._round(want, GRAIN, absref, dt, 0.1, 1, what)
    # not vacuous: the walk's order (round acc + bias first, then add the residual and round again) differs somewhere
    early = (acc_b.float().to(dt).float() + res.float()).to(dt)
    assert not torch.equal(early, exp), f"{what}: a residual added after a first rounding would pass"
    got = _fwd_res(X, nbr, order, WT, flip, bias, res, M_out, dt)
    torch.cuda.synchronize()
    bad = int((got != exp).sum())
    assert torch.equal(got, exp), f"{what}: {bad} elements differ"
    assert torch.equal(_fwd_res(X, nbr, order, WT, flip, bias, res, M_out, dt), got), f"{what}: a rerun changed bits"
    # NULL residual: the plain entry point's form (which forwards here -- the independent pin of its bits is
    # tests/test_gpu_lowp_exact.py); the residual changed the result
    a = _fwd_res(X, nbr, order, WT, flip, bias, None, M_out, dt)
    b = _fwd_plain(X, nbr, order, WT, flip, bias, M_out, dt)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: NULL residual differs from wsis_spconv_fwd_lp"
    assert not torch.equal(a, got)


# ---- 2. BatchNorm apply ----------------------------------------------------------------------------------------------

def _bn32(x, mean, var, gamma, beta, eps, relu):
    y = torch.full(x.shape, NAN, device=DEV)
    _n.check(_n.hip().wsis_bn_apply(_n.ptr(x), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta), eps, relu,
                                    _n.ptr(y), x.shape[0], x.shape[1], _n.stream_ptr()), "bn_apply")
    return y


def _bn_lp(x, mean, var, gamma, beta, eps, relu, out_dtype):
    y = torch.full(x.shape, NAN, dtype=out_dtype, device=DEV)
    _n.check(_n.hip().wsis_bn_apply_lp(_n.ptr(x), _n.ptr(mean), _n.ptr(var), _n.ptr(gamma), _n.ptr(beta), eps, relu,
                                       _n.ptr(y), int(out_dtype == torch.float32), x.shape[0], x.shape[1],
                                       CODE[x.dtype], _n.stream_ptr()), "bn_apply_lp")
    return y


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [32, 64, 96, 128, 160, 192, 256])
def test_bn_apply_lp_exact(C, dt):
    g = torch.Generator(device=DEV).manual_seed(C)
    for M in (1, 1000, 4097, 150_001):
        x = (torch.randn(M, C, device=DEV, generator=g) * 3 + 0.5).to(dt)
        mean = torch.randn(C, device=DEV, generator=g) * 0.5
        var = torch.rand(C, device=DEV, generator=g) * 4 + 0.05
        gamma = torch.randn(C, device=DEV, generator=g)
        beta = torch.randn(C, device=DEV, generator=g) * 0.3
        for relu in (0, 1):
            for ga, be in ((gamma, beta), (None, None)):
                ref = _bn32(x.float(), mean, var, ga, be, 1e-4, relu)
                y16 = _bn_lp(x, mean, var, ga, be, 1e-4, relu, dt)
                y32 = _bn_lp(x, mean, var, ga, be, 1e-4, relu, torch.float32)
                what = f"M {M} C {C} relu {relu} affine {ga is not None} {dt}"
                assert torch.equal(y16, ref.to(dt)), what + ": 16-bit output"
                assert torch.equal(y32.view(torch.int32), ref.view(torch.int32)), what + ": fp32 output"


# ---- 3. 16-bit concatenation ---------------------------------------------------------------------------------------

def _op_array(rows):
    a = np.zeros(len(rows), dtype=un.OP_DTYPE)
    for i, (kind, flags, M, K, Cin, Cout, code, inp, out) in enumerate(rows):
        a[i]["kind"], a[i]["flags"], a[i]["M_in"], a[i]["M_out"] = kind, flags, M, M
        a[i]["K"], a[i]["Cin"], a[i]["Cout"], a[i]["reserved"] = K, Cin, Cout, code
        a[i]["inp"][:len(inp)] = inp
        a[i]["out"][:len(out)] = out
    return a


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("ca,cb", [(32, 32), (64, 64), (160, 160), (32, 96), (2, 6), (6, 2)])
def test_cat_op_copies_bits(ca, cb, dt):
    for M in (1, 777, 65537):
        a = torch.randn(M, ca, device=DEV).to(dt)
        b = torch.randn(M, cb, device=DEV).to(dt)
        a[0, 0] = NAN
        out = torch.full((M, ca + cb), NAN, dtype=dt, device=DEV)
        ops = _op_array([(un.OP_CAT, un.F_LP, M, 0, ca, cb, CODE[dt], (a.data_ptr(), b.data_ptr()), (out.data_ptr(),))])
        un._run(_n.hip(), ops, a.device)
        assert torch.equal(out.view(torch.int16), torch.cat((a, b), 1).view(torch.int16)), (M, ca, cb)


# ---- shared scenes and models ----------------------------------------------------------------------------------------

def _scene(kind):
    if kind == "small":
        return harness.make_scene(0, room=(3.0, 3.0, 2.4), n_box=2, max_points=10000)
    if kind == "c2":
        return harness.bench_scene(1)
    return harness.bench_scene(5, room=(13.0, 10.0, 3.0), n_box=36)


def _input(batch, cfg, dtype=None):
    """the SparseConvTensor Network.forward receives (harness.forward_loss), features in ``dtype``"""
    import pointgroup_ops
    feats = batch["feats"]
    if cfg.model.use_coords:
        feats = torch.cat((feats, batch["locs_float"]), 1)
    vf = pointgroup_ops.voxelization(feats, batch["v2p_map"], cfg.mode)
    if dtype is not None:
        vf = vf.to(dtype)
    return spconv.SparseConvTensor(vf, batch["voxel_coords_int"], batch["spatial_shape"], max(int(cfg.batch_size), 1))


def _trained(scene="small", steps=3):
    """model + batch after a few fp32 training steps (running statistics that are not the initial ones), in eval mode"""
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene(scene)]), DEV)
    model, crit, opt = harness.build_model(cfg, DEV)
    for _ in range(steps):
        harness.train_step(model, crit, opt, batch, cfg)
    model.eval()
    return model, crit, batch, cfg


def _walk(model, inp):
    out = model.output_layer(model.unet(model.input_conv(inp))).features
    sp_ops.verify_pending_counts()
    return out


# ---- 4. executor = single-op replay ----------------------------------------------------------------------------------

def _replay(model, inp, dt):
    """the module tree walked with the single-op entry points in the order the program records them"""
    lib, st = _n.hip(), _n.stream_ptr()
    code = CODE[dt]
    d = inp.indice_dict
    Mv = model._native_prog.Mvec

    def tables(kind, lvl):
        if kind == "subm":
            rb = d["subm%d" % (lvl + 1)]
            return rb.nbr_p, rb.order
        rd = d["spconv%d" % (lvl + 1)]
        return (rd.nbr_p, rd.order) if kind == "down" else (rd.nbr_up_p, rd.order_up)

    def conv(x, m, kind, lvl_in, lvl_out, res=None):
        K = int(np.prod(m.kernel_size))
        W = m.weight.detach().contiguous().view(K, m.in_channels, m.out_channels)
        nbr, order = tables(kind, lvl_in if kind != "up" else lvl_out) if kind else (None, None)
        M_out = int(Mv[lvl_out])
        out = torch.full((M_out, m.out_channels), NAN, dtype=dt, device=DEV)
        WT = sp_ops._weight_lp(W, dt, 1, 0)
        _n.check(lib.wsis_spconv_fwd_lp_res(_n.ptr(x), _n.ptr(nbr), _n.ptr(order), _n.ptr(WT), 0, None, _n.ptr(res),
                                            _n.ptr(out), x.shape[0], M_out, K, m.in_channels, m.out_channels, code,
                                            None, 256, st), "fwd_lp_res")
        return out

    def bn(x, m, out_dtype=None):
        out_dtype = out_dtype or dt
        y = torch.full(x.shape, NAN, dtype=out_dtype, device=DEV)
        _n.check(lib.wsis_bn_apply_lp(_n.ptr(x), _n.ptr(m.running_mean), _n.ptr(m.running_var), _n.ptr(m.weight),
                                      _n.ptr(m.bias), m.eps, 1, _n.ptr(y), int(out_dtype == torch.float32), x.shape[0],
                                      x.shape[1], code, st), "bn_apply_lp")
        return y

    def block(x, blk, lvl):
        s = blk.conv_branch
        z = conv(bn(x, s[0]), s[2], "subm", lvl, lvl)
        a2 = bn(z, s[3])
        first = blk.i_branch[0]
        r = x if isinstance(first, torch.nn.Identity) else conv(x, first, None, lvl, lvl)
        return conv(a2, s[5], "subm", lvl, lvl, res=r)

    def ublock(x, ub, lvl):
        for blk in ub.blocks:
            x = block(x, blk, lvl)
        if len(ub.nPlanes) == 1:
            return x
        dn = conv(bn(x, ub.conv[0]), ub.conv[2], "down", lvl, lvl + 1)
        u = ublock(dn, ub.u, lvl + 1)
        up = conv(bn(u, ub.deconv[0]), ub.deconv[2], "up", lvl + 1, lvl)
        x = torch.cat((x, up), 1)
        for blk in ub.blocks_tail:
            x = block(x, blk, lvl)
        return x

    c0 = model.input_conv[0]
    rb = d["subm1"]
    W0 = c0.weight.detach().contiguous().view(-1, c0.in_channels, c0.out_channels)
    x = sp_ops._fwd_fp32(inp.features.to(dt).float().contiguous(), rb.nbr_p, rb.order, W0, None, int(Mv[0])).to(dt)
    return bn(ublock(x, model.unet, 0), model.output_layer[0])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("scene", ["small", "c2"])
def test_executor_equals_single_op_replay(scene, dt):
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene(scene)]), DEV)
    model, _, _ = harness.build_model(cfg, DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, device=DEV, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, device=DEV, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, device=DEV, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, device=DEV, generator=g) * 0.1)
    model.eval()
    inp = _input(batch, cfg)
    with torch.no_grad():
        got = un.run_unet_lp(model, inp, dt, dt)
        want = _replay(model, inp, dt)
    torch.cuda.synchronize()
    assert got.dtype == want.dtype == dt
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        f"{int((got != want).sum())} of {got.numel()} elements differ"
    with torch.no_grad():
        g32 = un.run_unet_lp(model, inp, dt, torch.float32)
    assert g32.dtype == torch.float32 and torch.equal(g32.to(dt), got)


# ---- 5. dispatch ---------------------------------------------------------------------------------------------------

class _Stop(Exception):
    pass


def _extra(batch):
    from torch_scatter import scatter
    centre = scatter(batch["locs_float"], batch["superpoint"], dim=0, reduce="mean", csr=batch.get("superpoint_csr"))
    return {"superpoint": batch["superpoint"], "GIs": batch["GIs"], "edge_u_list": batch["edge_u_list"],
            "edge_v_list": batch["edge_v_list"], "superpoint_cenetr_xyz": centre,
            "superpoint_csr": batch.get("superpoint_csr"), "edge_graph": batch.get("edge_graph"),
            "p2v_csr": batch.get("p2v_csr"), "edge_src_rows": batch.get("edge_src_rows")}


def _unet_out(model, batch, cfg, feat_dtype=None):
    """Network.forward up to the UNet's output: (last_pass, output) -- stopped there (16-bit features do not go on
    through the fp32 heads)"""
    seen = {}
    real = un.run_unet_lp

    def lp(*a, **k):
        seen["out"] = real(*a, **k)
        raise _Stop()

    def walk_out(inp):
        seen["out"] = type(model.output_layer).forward(model.output_layer, inp).features
        raise _Stop()
    un.run_unet_lp = lp
    model.output_layer.forward = walk_out
    try:
        model(_input(batch, cfg, feat_dtype), batch["p2v_map"], _extra(batch))
    except _Stop:
        pass
    finally:
        un.run_unet_lp = real
        del model.output_layer.forward
    return model.last_pass, seen.get("out")


def test_dispatch(monkeypatch):
    model, _, batch, cfg = _trained("small", steps=1)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    monkeypatch.delenv("WSIS_NATIVE_LP", raising=False)
    monkeypatch.delenv("WSIS_NATIVE_UNET", raising=False)
    cases = []
    for dt in DTYPES:
        for mode in ("autocast", "features"):
            for grad in ("no_grad", "inference_mode"):
                cases.append((dt, mode, grad))

    def run(dt, mode, grad, feat=True):
        ctx = torch.no_grad() if grad == "no_grad" else (torch.inference_mode() if grad == "inference_mode"
                                                          else torch.enable_grad())
        with ctx, torch.autocast("cuda", dtype=dt, enabled=mode == "autocast"):
            return _unet_out(model, batch, cfg, dt if mode == "features" else None)

    for dt, mode, grad in cases:
        monkeypatch.delenv("WSIS_NATIVE_LP", raising=False)
        p_walk, walk = run(dt, mode, grad)
        assert p_walk == "modules", (dt, mode, grad, "switch unset")
        monkeypatch.setenv("WSIS_NATIVE_LP", "1")
        p_lp, lp = run(dt, mode, grad)
        assert p_lp == "native_lp", (dt, mode, grad)
        assert lp.dtype == walk.dtype, (dt, mode, grad, lp.dtype, walk.dtype)
        print(f"{dt} {mode} {grad}: output dtype {lp.dtype}")
        monkeypatch.setenv("WSIS_NATIVE_UNET", "0")
        assert run(dt, mode, grad)[0] == "modules", "WSIS_NATIVE_UNET=0 walks the modules"
        monkeypatch.delenv("WSIS_NATIVE_UNET")
    monkeypatch.setenv("WSIS_NATIVE_LP", "1")
    # gradients enabled: the walk (the training pass is fp32 only)
    assert run(torch.bfloat16, "autocast", "grad")[0] == "modules"
    # fp32 features outside autocast: the fp32 native pass as before
    with torch.no_grad():
        model(_input(batch, cfg), batch["p2v_map"], _extra(batch))
    assert model.last_pass == "native"
    # one BatchNorm layer in training mode: the walk (it updates that layer's running statistics: restored below)
    model.unet.u.blocks.block1.conv_branch[3].train()
    assert run(torch.bfloat16, "autocast", "no_grad")[0] == "modules"
    model.eval()
    model.load_state_dict(state)
    assert run(torch.bfloat16, "autocast", "no_grad")[0] == "native_lp"


def test_dispatch_walks_a_16bit_parameter_model(monkeypatch):
    """model.to(bfloat16): the executor would read its 2-byte parameters as fp32 -- the dispatch must walk the modules,
    and the result is the walk's"""
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene("small")]), DEV)
    model, _, _ = harness.build_model(cfg, DEV)
    model = model.to(torch.bfloat16).eval()
    monkeypatch.setenv("WSIS_NATIVE_LP", "1")
    monkeypatch.delenv("WSIS_NATIVE_UNET", raising=False)
    with torch.no_grad():
        p, out = _unet_out(model, batch, cfg, torch.bfloat16)
    assert p == "modules", p
    assert out is not None and out.dtype == torch.bfloat16 and bool(torch.isfinite(out).all())
    with torch.no_grad():
        want = _walk(model, _input(batch, cfg, torch.bfloat16))
    assert _rel(out, want) <= 1e-2
    # one BatchNorm buffer in 16 bits is enough to refuse; back in fp32 the pass is taken
    m2, _, _ = harness.build_model(cfg, DEV)
    m2.eval()
    bn = m2.unet.u.blocks.block0.conv_branch[3]
    bn.running_var = bn.running_var.to(torch.bfloat16)
    assert not un.lp_params_fp32(m2, batch["feats"].device)
    bn.running_var = bn.running_var.float()
    with torch.no_grad():
        assert _unet_out(m2, batch, cfg, torch.bfloat16)[0] == "native_lp"


# ---- 6. accuracy and reproducibility ------------------------------------------------------------------------------

def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_accuracy_against_fp32(dt, monkeypatch):
    model, crit, batch, cfg = _trained("small", steps=3)
    inp = _input(batch, cfg)
    with torch.no_grad():
        out32 = un.run_unet(model, inp)
        lp1 = un.run_unet_lp(model, inp, dt, dt)
        lp2 = un.run_unet_lp(model, inp, dt, dt)
        walk = _walk(model, _input(batch, cfg, dt))
    assert torch.equal(lp1.view(torch.int16), lp2.view(torch.int16)), "two calls differ"
    assert walk.dtype == lp1.dtype == dt
    e_lp, e_walk = _rel(lp1, out32), _rel(walk, out32)
    print(f"{dt}: UNet output rel. Frobenius error native_lp {e_lp:.3e}, walk {e_walk:.3e}")
    assert e_lp <= 1.25 * e_walk + 1e-3, (e_lp, e_walk)
    # measured 3.55e-3 (bf16) and 4.49e-4 (fp16), the walk's errors to three digits
    assert e_lp <= (1e-2 if dt == torch.bfloat16 else 1.5e-3), e_lp
    # the whole forward + loss under autocast (the output dtype is the walk's, everything behind the UNet as before)
    monkeypatch.setenv("WSIS_NATIVE_LP", "1")
    with torch.no_grad():
        loss32, _ = harness.forward_loss(model, crit, batch, cfg)
        assert model.last_pass == "native"
        with torch.autocast("cuda", dtype=dt):
            loss_lp, _ = harness.forward_loss(model, crit, batch, cfg)
            assert model.last_pass == "native_lp"
        monkeypatch.delenv("WSIS_NATIVE_LP")
        with torch.autocast("cuda", dtype=dt):
            loss_walk, _ = harness.forward_loss(model, crit, batch, cfg)
            assert model.last_pass == "modules"
    r_lp = abs(float(loss_lp) - float(loss32)) / abs(float(loss32))
    r_walk = abs(float(loss_walk) - float(loss32)) / abs(float(loss32))
    print(f"{dt}: loss fp32 {float(loss32):.6f}, native_lp {float(loss_lp):.6f} ({r_lp:.3e}), "
          f"walk {float(loss_walk):.6f} ({r_walk:.3e})")
    assert r_lp <= 1.25 * r_walk + 1e-3, (r_lp, r_walk)
    # measured 4.9e-5 (bf16; walk 8.0e-5) and 1.1e-5 (fp16; walk 1.5e-5)
    assert r_lp <= 1e-3, r_lp


def test_c4_room_bf16():
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene("c4")]), DEV)
    model, crit, opt = harness.build_model(cfg, DEV)
    small = harness.to_device(harness.collate([_scene("small")]), DEV)
    for _ in range(2):
        harness.train_step(model, crit, opt, small, cfg)
    model.eval()
    inp = _input(batch, cfg)
    with torch.no_grad():
        out32 = un.run_unet(model, inp)
        lp = un.run_unet_lp(model, inp, torch.bfloat16, torch.bfloat16)
    assert lp.shape == out32.shape and lp.shape[0] > 500_000
    assert bool(torch.isfinite(lp).all())
    e = _rel(lp, out32)
    print(f"C4 room ({lp.shape[0]} voxels) bf16: UNet output rel. Frobenius error {e:.3e}")
    # measured 4.75e-3 (778,302 voxels)
    assert e <= 1.5e-2, e
