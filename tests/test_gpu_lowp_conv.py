"""GPU: the 16-bit sparse convolutions (bf16 / fp16 operands, fp32 accumulation; csrc/spconv_lp.hip) through the public
modules, against fp64 over the ORACLE pair lists (oracle/spconv_ref, tests/conv_ref.py).

The reference takes the 16-bit-rounded X, W and dY, which are exact in fp64, so what is left is the fp32 accumulation
and the one final rounding of each output element:

  forward / dIn   |got - ref| <= 2u |ref| + 2^-18 (|X| @ |W|)     u = 2^-8 (bf16), 2^-11 (fp16)
  dW (fp32)       conv_ref.check_dw at 1e-5 of max |dW|

and the bound is shown tight: the same check against the reference with one offset's pairs removed fails."""
import numpy as np
import pytest
import torch

import harness
import spconv
from oracle import spconv_ref as ref
from spconv import ops
from sparse_unet3d import UBlock
from util import random_sparse_coords

import conv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CHANNELS = ((32, 32), (32, 64), (64, 96), (96, 128), (128, 160), (160, 160), (64, 32))
KINDS = ("subm", "subm1", "down", "inv", "subm133", "down3", "subm5")
SHAPE = (12, 11, 10)


def _bound_ok(got, want, absref, dt):
    """elementwise |got - want| <= 2u |want| + 2^-18 absref (all fp64)"""
    tol = 2 * UNIT[dt] * want.abs() + 2.0 ** -18 * absref
    return bool(((got.double() - want).abs() <= tol).all())


def _check_rows(got, X, W, pairs, M_out, sel, dt, what, bias=None):
    """rows ``sel`` of ``got`` against sum_k X[pi] @ W[k] (+ bias) in fp64, and against its one-offset-removed form"""
    b = bias.double() if bias is not None else 0.0
    want = conv_ref.rows(X, W, pairs, M_out, sel) + b
    absref = conv_ref.rows(X.abs(), W.abs(), pairs, M_out, sel) + (bias.double().abs() if bias is not None else 0.0)
    g = got[sel].double()
    err = float((g - want).abs().max()) if want.numel() else 0.0
    assert _bound_ok(g, want, absref, dt), f"{what}: max abs error {err:.3e} outside 2u|ref| + 2^-18 (|X| @ |W|)"
    live = [k for k, (pi, po) in enumerate(pairs) if len(pi)]
    if not live or want.numel() == 0:
        return
    k = max(live, key=lambda j: len(pairs[j][0]))
    dropped = [p if j != k else (p[0][:0], p[1][:0]) for j, p in enumerate(pairs)]
    want_d = conv_ref.rows(X, W, dropped, M_out, sel) + b
    assert not _bound_ok(g, want_d, absref, dt), f"{what}: the bound would not see offset {k} missing"


def _module_case(kind, cin, cout, coords, shape, batch):
    """(conv module, input SparseConvTensor builder, fp64 oracle pairs, M_out) of one kind"""
    idx = np.asarray(coords)
    M = idx.shape[0]
    if kind in ("subm", "subm1", "subm133", "subm5"):
        ks, pad = {"subm": (3, 1), "subm1": (1, 0), "subm133": ((1, 3, 3), (0, 1, 1)), "subm5": (5, 2)}[kind]
        conv = spconv.SubMConv3d(cin, cout, ks, padding=pad, bias=True, indice_key="k_" + kind)
        if kind == "subm1":
            pairs = [(np.arange(M), np.arange(M))]
        else:
            pairs = ref.subm_pairs_fast(idx, shape, ks, pad)
        return conv, idx, shape, pairs, M, None
    if kind in ("down", "down3"):
        ks, st, pad = (2, 2, 0) if kind == "down" else (3, 2, 1)
        conv = spconv.SparseConv3d(cin, cout, ks, stride=st, padding=pad, bias=True, indice_key="k_" + kind)
        out_idx, _, pairs = ref.down_pairs_fast(idx, shape, ks, st, pad)
        return conv, idx, shape, pairs, out_idx.shape[0], None
    assert kind == "inv"
    # SparseInverseConv3d k2 over the tables of a SparseConv3d k2 s2: input = the coarse rows, output = the fine rows
    down = spconv.SparseConv3d(cin, cin, 2, stride=2, bias=False, indice_key="k_inv")
    conv = spconv.SparseInverseConv3d(cin, cout, 2, indice_key="k_inv", bias=True)
    out_idx, _, pairs = ref.down_pairs_fast(idx, shape, 2, 2, 0)
    return conv, idx, shape, conv_ref.swap(pairs), M, down


def _run(kind, cin, cout, dt, coords, batch=2, shape=SHAPE, seed=0, check=True):
    torch.manual_seed(seed)
    conv, idx, shape, pairs, M_out, down = _module_case(kind, cin, cout, coords, shape, batch)
    conv = conv.to(DEV)
    with torch.no_grad():                   # parameters exactly representable in 16 bits: the fp64 reference is exact
        conv.weight.copy_(conv.weight.to(dt).float())
        conv.bias.copy_(conv.bias.to(dt).float())
    ind = torch.from_numpy(idx.astype(np.int32)).to(DEV)
    t = spconv.SparseConvTensor(torch.zeros(len(idx), cin, device=DEV), ind, np.array(shape), batch)
    if down is not None:
        t = down.to(DEV)(t)                 # builds the coupled tables; its output rows are the inverse conv's input
    M_in = t.features.shape[0]
    X = torch.randn(M_in, cin, device=DEV).to(dt)
    dY = torch.randn(M_out, cout, device=DEV).to(dt)
    xg = X.clone().requires_grad_(True)
    t.features = xg
    out = conv(t)
    assert out.features.dtype == dt and out.features.shape == (M_out, cout)
    out.features.backward(dY)
    assert xg.grad.dtype == dt and conv.weight.grad.dtype == torch.float32
    K = conv.weight[..., 0, 0].numel()
    W = conv.weight.detach().view(K, cin, cout)
    dp = conv_ref.device_pairs(pairs, DEV)
    res = dict(out=out.features.detach(), dX=xg.grad, dW=conv.weight.grad.view(K, cin, cout), X=X, dY=dY, W=W, dp=dp,
               M_in=M_in, M_out=M_out, bias=conv.bias.detach())
    if check:
        what = f"{kind} {cin}->{cout} {dt}"
        sel_o = torch.arange(M_out, device=DEV)
        sel_i = torch.arange(M_in, device=DEV)
        _check_rows(res["out"], X, W, dp, M_out, sel_o, dt, what + " forward", bias=conv.bias.detach())
        _check_rows(res["dX"], dY, W.transpose(1, 2), conv_ref.swap(dp), M_in, sel_i, dt, what + " dIn")
        conv_ref.check_dw(res["dW"], X, dY, dp, 1e-5, what + " dW")
    return res


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("surface", (False, True), ids=["dense", "surface"])
@pytest.mark.parametrize("kind", KINDS)
def test_lowp_kinds_against_fp64(kind, surface, dt):
    coords = random_sparse_coords(KINDS.index(kind) + 10 * surface, batch=2, shape=SHAPE,
                                  density=0.12 if surface else 0.3, surface=surface)
    cin, cout = CHANNELS[(KINDS.index(kind) + 3 * surface) % len(CHANNELS)]
    before = ops.LOWP_FALLBACKS
    _run(kind, cin, cout, dt, coords)
    assert ops.LOWP_FALLBACKS == before, "a supported shape fell back to fp32"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("kind", ("subm", "down"))
def test_lowp_channels_against_fp64(kind, cin, cout, dt):
    coords = random_sparse_coords(100 + cin + cout, batch=2, shape=SHAPE, density=0.25)
    _run(kind, cin, cout, dt, coords)


def test_lowp_dtype_contract():
    coords = random_sparse_coords(7, batch=2, shape=SHAPE, density=0.3)
    ind = torch.from_numpy(coords).to(DEV)
    torch.manual_seed(1)
    conv = spconv.SubMConv3d(32, 64, 3, padding=1, bias=True, indice_key="c").to(DEV)
    # bf16 features + bf16 parameters (model.to(torch.bfloat16)): bf16 out, dX bf16, weight.grad bf16
    conv16 = spconv.SubMConv3d(32, 64, 3, padding=1, bias=True, indice_key="c").to(DEV).to(torch.bfloat16)
    x = torch.randn(len(coords), 32, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    out = conv16(spconv.SparseConvTensor(x, ind, np.array(SHAPE), 2)).features
    assert out.dtype == torch.bfloat16
    out.float().square().sum().backward()
    assert x.grad.dtype == torch.bfloat16 and conv16.weight.grad.dtype == torch.bfloat16
    assert conv16.bias.grad.dtype == torch.bfloat16
    # bf16 features + fp32 parameters: bf16 out, fp32 parameter gradients
    x = torch.randn(len(coords), 32, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    out = conv(spconv.SparseConvTensor(x, ind, np.array(SHAPE), 2)).features
    assert out.dtype == torch.bfloat16
    out.float().sum().backward()
    assert x.grad.dtype == torch.bfloat16 and conv.weight.grad.dtype == torch.float32
    # autocast: fp32 features and parameters -> 16-bit output, fp32 gradients (features and parameters)
    for dt in DTYPES:
        conv.zero_grad()
        x = torch.randn(len(coords), 32, device=DEV, requires_grad=True)
        with torch.autocast("cuda", dtype=dt):
            out = conv(spconv.SparseConvTensor(x, ind, np.array(SHAPE), 2)).features
        assert out.dtype == dt
        out.float().sum().backward()
        assert x.grad.dtype == torch.float32 and conv.weight.grad.dtype == torch.float32
        assert conv.bias.grad.dtype == torch.float32
    # fp32 outside autocast: fp32 as before
    x = torch.randn(len(coords), 32, device=DEV)
    assert conv(spconv.SparseConvTensor(x, ind, np.array(SHAPE), 2)).features.dtype == torch.float32


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_lowp_bit_reproducible(dt):
    coords = random_sparse_coords(3, batch=2, shape=SHAPE, density=0.3)
    a = _run("subm", 64, 96, dt, coords, seed=5, check=False)
    b = _run("subm", 64, 96, dt, coords, seed=5, check=False)
    for key in ("out", "dX", "dW"):
        assert torch.equal(a[key], b[key]), key
    a = _run("down", 32, 64, dt, coords, seed=6, check=False)
    b = _run("down", 32, 64, dt, coords, seed=6, check=False)
    for key in ("out", "dX", "dW"):
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_lowp_input_conv_falls_back_within_bound(dt):
    coords = random_sparse_coords(4, batch=2, shape=SHAPE, density=0.3)
    before = ops.LOWP_FALLBACKS
    _run("subm", 6, 32, dt, coords)
    assert ops.LOWP_FALLBACKS >= before + 3, "forward, dIn and dW of 6 -> 32 count as fallbacks"


def test_lowp_unet_shapes_never_fall_back():
    planes = (32, 64, 96, 128, 160)
    for l, c in enumerate(planes):
        shapes = [(27, c, c), (27, 2 * c, c), (1, 2 * c, c)]
        if l + 1 < len(planes):
            shapes += [(8, c, planes[l + 1])]
        for K, ci, co in shapes:
            assert ops.lp_supported(K, ci, co, 10 ** 6) and ops.lp_supported(K, co, ci, 10 ** 6), (K, ci, co)
    assert not ops.lp_supported(27, 6, 32, 100)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_lowp_edges(dt):
    torch.manual_seed(2)
    # M_out = 0 (dense 1x1 form): empty output, zero dW
    w = torch.randn(1, 1, 1, 32, 64, device=DEV, requires_grad=True)
    x = torch.zeros(0, 32, device=DEV, dtype=dt, requires_grad=True)
    out = ops.sparse_conv(x, w, None, None, None, None, None, 0, 0)
    assert out.shape == (0, 64) and out.dtype == dt
    out.float().sum().backward()
    assert w.grad is not None and int((w.grad != 0).sum()) == 0
    # hand-made plain tables, M = 50 / 77 rows (not multiples of 32): rows 0..9 of the output have no pair at all
    K, M_in, M_out, cin, cout = 3, 77, 50, 32, 64
    nbr_f = torch.full((K, M_out), -1, dtype=torch.int32)
    nbr_b = torch.full((K, M_in), -1, dtype=torch.int32)
    g = torch.Generator().manual_seed(3)
    pairs = []
    for k in range(K):
        po = 10 + torch.randperm(M_out - 10, generator=g)[:30]
        pi = torch.randperm(M_in, generator=g)[:30]
        nbr_f[k, po] = pi.int()
        nbr_b[k, pi] = po.int()
        pairs.append((pi.numpy(), po.numpy()))
    W = torch.randn(K, 1, 1, cin, cout, device=DEV).to(dt).float().requires_grad_(True)
    b = torch.randn(cout, device=DEV).to(dt).float().requires_grad_(True)
    X = torch.randn(M_in, cin, device=DEV).to(dt)
    dY = torch.randn(M_out, cout, device=DEV).to(dt)
    xg = X.clone().requires_grad_(True)
    out = ops.sparse_conv(xg, W, b, nbr_f.to(DEV), None, nbr_b.to(DEV), None, 0, M_out)
    out.backward(dY)
    assert torch.equal(out[:10].float(), b.detach().to(dt).float().expand(10, cout)), "bias-only rows"
    dp = conv_ref.device_pairs(pairs, DEV)
    Wk = W.detach().view(K, cin, cout)
    _check_rows(out.detach(), X, Wk, dp, M_out, torch.arange(M_out, device=DEV), dt, "edges forward", bias=b.detach())
    _check_rows(xg.grad, dY, Wk.transpose(1, 2), conv_ref.swap(dp), M_in, torch.arange(M_in, device=DEV), dt,
                "edges dIn")
    conv_ref.check_dw(W.grad.view(K, cin, cout), X, dY, dp, 1e-5, "edges dW")
    assert torch.allclose(b.grad.double(), dY.double().sum(0), rtol=1e-5, atol=1e-4)


@pytest.fixture(scope="module")
def c2_levels():
    b = harness.collate([harness.make_scene(1)])
    idx = b["voxel_locs"].int().to(DEV).contiguous()
    shape = [int(s) for s in b["spatial_shape"]]
    levels = []
    for l in range(5):
        subm = ops.build_subm_rulebook(idx, shape, [3] * 3, [1] * 3)
        ent = {"idx": idx, "shape": shape, "subm": subm,
               "subm_pairs": ref.subm_pairs_fast(idx.cpu().numpy(), shape, 3, 1)}
        if l < 4:
            down = ops.build_down_rulebook(idx, shape, [2] * 3, [2] * 3, [0] * 3)
            out_idx, _, pairs = ref.down_pairs_fast(idx.cpu().numpy(), shape, 2, 2, 0)
            assert np.array_equal(out_idx, down.out_indices.cpu().numpy())
            ent["down"], ent["down_pairs"] = down, pairs
            idx, shape = down.out_indices, down.out_shape
        levels.append(ent)
    return levels


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("level", range(5))
def test_lowp_full_size_c2(c2_levels, level, dt):
    planes = (32, 64, 96, 128, 160)
    ent = c2_levels[level]
    C = planes[level]
    g = torch.Generator(device=DEV).manual_seed(level)
    jobs = [("subm", C, C, ent["subm"].nbr_p, ent["subm"].order, ent["subm"].nbr_p, ent["subm"].order, 1,
             ent["idx"].shape[0], ent["subm_pairs"])]
    if "down" in ent:
        d = ent["down"]
        jobs.append(("down", C, planes[level + 1], d.nbr_p, d.order, d.nbr_up_p, d.order_up, 0, d.out_indices.shape[0],
                     ent["down_pairs"]))
    for name, cin, cout, nf, of, nb, ob, flip, M_out, pairs in jobs:
        K = len(pairs)
        M_in = ent["idx"].shape[0]
        W = (torch.randn(K, 1, 1, cin, cout, device=DEV, generator=g) / np.sqrt(K * cin)).to(dt).float()
        W.requires_grad_(True)
        X = torch.randn(M_in, cin, device=DEV, generator=g).to(dt)
        dY = torch.randn(M_out, cout, device=DEV, generator=g).to(dt)
        xg = X.clone().requires_grad_(True)
        out = ops.sparse_conv(xg, W, None, nf, of, nb, ob, flip, M_out)
        assert out.dtype == dt
        out.backward(dY)
        dp = conv_ref.device_pairs(pairs, DEV)
        Wk = W.detach().view(K, cin, cout)
        sel_o = torch.randperm(M_out, device=DEV, generator=g)[:4096]
        sel_i = torch.randperm(M_in, device=DEV, generator=g)[:4096]
        what = f"C2 level {level} {name} {cin}->{cout} {dt}"
        _check_rows(out.detach(), X, Wk, dp, M_out, sel_o, dt, what + " forward")
        _check_rows(xg.grad, dY, Wk.transpose(1, 2), conv_ref.swap(dp), M_in, sel_i, dt, what + " dIn")
        conv_ref.check_dw(W.grad.view(K, cin, cout), X, dY, dp, 1e-5, what + " dW")


def _ublock_walk(ublock, x, ind, shape, dY, autocast):
    ublock.zero_grad(set_to_none=True)
    t = spconv.SparseConvTensor(x, ind, np.array(shape), 1)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = ublock(t).features
    out.float().backward(dY)
    grads = torch.cat([p.grad.float().flatten() for p in ublock.parameters() if p.grad is not None])
    return out.detach().float(), grads


def test_lowp_ublock_walk_autocast():
    sc = harness.make_scene(2, room=(2.4, 2.0, 1.4), n_box=3)
    b = harness.collate([sc])
    ind = b["voxel_locs"].int().to(DEV).contiguous()
    shape = [int(s) for s in b["spatial_shape"]]
    torch.manual_seed(11)
    ublock = UBlock([32, 64, 96, 128, 160], block_reps=2).to(DEV)
    x = torch.randn(ind.shape[0], 32, device=DEV)
    dY = torch.randn(ind.shape[0], 32, device=DEV)
    out32, g32 = _ublock_walk(ublock, x, ind, shape, dY, False)
    before = ops.LOWP_FALLBACKS
    out16, g16 = _ublock_walk(ublock, x, ind, shape, dY, True)
    assert ops.LOWP_FALLBACKS == before, "a UNet layer fell back to fp32"
    assert bool(torch.isfinite(out16).all()) and bool(torch.isfinite(g16).all())
    rel = float((out16 - out32).norm() / out32.norm())
    cos = float(torch.nn.functional.cosine_similarity(g16.double(), g32.double(), dim=0))
    print(f"UBlock walk under autocast(bf16): output rel. Frobenius error {rel:.3e}, gradient cosine {cos:.6f}")
    # measured 1.81e-2 (this scene) and 1.83e-2 (a C2-sized room)
    assert rel <= 2.5e-2, rel
    # measured 0.891 (this scene) and 0.872 (a C2-sized room), not the 0.99 first guessed: the parameter gradients of this
    # randomly initialised five-level block amplify any difference of the forward pass about 10^4-fold -- two fp32 walks
    # whose only difference is the BatchNorm implementation (fused operator against torch, outputs 1.5e-6 apart) already
    # give a gradient cosine of 0.99995 -- and the cosine falls level by level with depth (0.99 at level 0, 0.85-0.9 at
    # level 4).  The kernels themselves are held to fp64 bounds by the tests above.
    assert cos >= 0.8, cos


def test_lowp_network_autocast_step():
    cfg = harness.default_cfg()
    sc = harness.make_scene(0, room=(3.0, 3.0, 2.4), n_box=2, max_points=10000)
    batch = harness.to_device(harness.collate([sc]), DEV)
    model, crit, opt = harness.build_model(cfg, DEV)
    loss32, _ = harness.forward_loss(model, crit, batch, cfg)
    assert model.last_pass == "native"
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss16, ret = harness.forward_loss(model, crit, batch, cfg)
    assert model.last_pass == "modules", "autocast must walk the modules"
    assert bool(torch.isfinite(loss16))
    rel = abs(float(loss16.detach()) - float(loss32)) / abs(float(loss32))
    print(f"Network loss fp32 {float(loss32):.6f}, autocast(bf16) {float(loss16.detach()):.6f}, rel. difference {rel:.3e}")
    assert rel <= 5e-2, rel
    opt.zero_grad(set_to_none=True)
    loss16.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads)
    opt.step()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
