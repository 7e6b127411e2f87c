"""GPU: the superpoint-graph kernels against fp64 where they branch on node degree, feature width, row count or pointer
alignment (tests/graph_ref.py builds the graphs and the references).

  edge attention   csrc/affinity.hip   D == 64 and out-degree <= AF_MAXDEG (32): the batched path; otherwise the three
                                       per-edge passes, with more than one 64-wide d0 pass for D > 64; targets without
                                       in-edge and with ~300; sources without out-edge inside [0, Su); no d_aff
  ECC messages     csrc/ecc.hip        C == 32 with 16-byte aligned w / dout / dw: ecc_msg_bwd32_kernel, whose edge
                                       metadata comes in chunks of 64 (in-degree 64, 65, 130, 300); else the generic kernel
  ECC contraction  csrc/ecc.hip        in-degree 0 (dU row zeroed), 8k +- 1 around EBATCH, 65; accumulate over 7 steps;
                   + csrc/gru.hip      under the fused loop, the per-op path and the torch GEMM path; gru_fwd_kernel<true>
                                       segments with 0 and >= 16 messages
  GRU cell         csrc/gru.hip        workgroups capped at 256 (S > 3,072), >= 128 slabs (the 16-slab unrolled reduce)
  ecc_u_fwd        csrc/ecc.hip        S not a multiple of 32, S < 32, a 4-scene batch
  batch scale      four bench scenes collated: affinity, position encoding and recurrence on a real 4-scene batch

Outputs the caller owns are pre-filled with NaN (the C ABI is called directly): a row no kernel writes cannot pass.
Every bound is a fraction of the reference's max-abs and is proven tight by the reference with one edge of the
largest hub removed (graph_ref.check) -- except the one gradient whose true value is zero (the bias in front of the filter
net's BatchNorm), which has nothing to be tight to.  Every case runs twice and must be bit-identical (fixed order of additions)."""
import copy

import numpy as np
import pytest
import torch

import graph_ref
import harness
import wsis_native as _n
import wsis_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
AF_MAXDEG = 32                                      # csrc/affinity.hip: the batched D == 64 path up to this out-degree
HUBS = (31, 32, 33, 63, 64, 65, 129, 300)
GNN_DEG = (7, 8, 9, 16, 17, 65)                     # EBATCH = 8 edges per trip of the contraction: 8k +- 1, and > 64


def _lib():
    return _n.hip()


def _csr(index, n):
    """host CSR (stable argsort, offsets) of an int64 numpy index: independent of the segment_csr kernel"""
    perm = np.argsort(index, kind="stable").astype(np.int32)
    off = np.searchsorted(index[perm], np.arange(n + 1)).astype(np.int32)
    return torch.from_numpy(perm).to(DEV), torch.from_numpy(off).to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _same(a, b, what):
    for name in a:
        assert bool(torch.isfinite(a[name]).all()), f"{what} {name}: non-finite values (an unwritten row or element)"
        assert torch.equal(a[name], b[name]), f"{what} {name}: two runs differ (the order of additions is not fixed)"


# ---------------------------------------------------------------- edge attention
def _affinity_run(q, k, v, pos, eu, ev, S, Su, ga, gr):
    """wsis_edge_affinity_fwd / _bwd on NaN-filled outputs; CSRs built on the host"""
    lib = _lib()
    E, D = eu.numel(), q.shape[1]
    pu, ou = _csr(eu.cpu().numpy(), Su)
    pv, ov = _csr(ev.cpu().numpy(), S)
    scale = 1.0 / np.sqrt(D)
    aff, res = _nan(E), _nan(Su, D)
    _n.check(lib.wsis_edge_affinity_fwd(_n.ptr(q), _n.ptr(k), _n.ptr(v), _n.ptr(pos), _n.ptr(eu), _n.ptr(ev), _n.ptr(pu),
                                        _n.ptr(ou), scale, _n.ptr(aff), _n.ptr(res), E, Su, D, _n.stream_ptr()),
             "edge_affinity_fwd")
    dq, dk, dv, dpos, tmp = _nan(S, D), _nan(S, D), _nan(S, D), _nan(E), _nan(2 * E)
    _n.check(lib.wsis_edge_affinity_bwd(_n.ptr(q), _n.ptr(k), _n.ptr(v), _n.ptr(pos), _n.ptr(aff), _n.ptr(eu), _n.ptr(ev),
                                        _n.ptr(pu), _n.ptr(ou), _n.ptr(pv), _n.ptr(ov), scale, _n.ptr(ga), _n.ptr(gr),
                                        _n.ptr(dq), _n.ptr(dk), _n.ptr(dv), _n.ptr(dpos), _n.ptr(tmp), E, S, Su, D,
                                        _n.stream_ptr()), "edge_affinity_bwd")
    torch.cuda.synchronize()
    return {"aff": aff, "res": res, "dq": dq, "dk": dk, "dv": dv, "dpos": dpos}


def _affinity_case(eu_np, ev_np, S, q, k, v, pos, with_daff, frac, drop_pick="median", seed=0):
    eu, ev = torch.from_numpy(eu_np).to(DEV), torch.from_numpy(ev_np).to(DEV)
    E, D, Su = len(eu_np), q.shape[1], int(eu_np.max()) + 1
    g = torch.Generator(device=DEV).manual_seed(seed)
    ga = torch.randn(E, device=DEV, generator=g) if with_daff else None
    gr = torch.randn(Su, D, device=DEV, generator=g)
    got = _affinity_run(q, k, v, pos, eu, ev, S, Su, ga, gr)
    _same(got, _affinity_run(q, k, v, pos, eu, ev, S, Su, ga, gr), f"affinity D={D}")
    want = graph_ref.affinity(q, k, v, pos, eu, ev, ga, gr)
    # one in-edge of the target with the most in-edges removed: of median (or largest) affinity among them.  (An edge of a
    # 300-edge source carries ~1/300 of its softmax: dropping it moves dv by ~1e-5 of max|dv|, below fp32 noise.)
    hub = int(np.bincount(ev_np).argmax())
    a = want["aff"].cpu().numpy()
    e = graph_ref.median_edge(ev_np, a, hub) if drop_pick == "median" else int(
        np.flatnonzero(ev_np == hub)[np.argmax(a[ev_np == hub])])
    keep = graph_ref.without_edge(E, e, DEV)
    drop = graph_ref.affinity(q, k, v, pos[keep], eu[keep], ev[keep], None if ga is None else ga[keep], gr)
    for name in ("aff", "dpos"):
        drop[name] = graph_ref.reinsert(drop[name], e)
    return graph_ref.check(got, want, drop, frac, f"affinity D={D} daff={with_daff}")


def _hub_affinity_graph():
    eu, ev, roles = graph_ref.hub_graph(7, 1500, out_hubs=HUBS, in_hubs=HUBS, no_out=5, no_in=5, isolated=3)
    return eu, ev, roles


@pytest.mark.parametrize("with_daff", [True, False])
@pytest.mark.parametrize("D", [32, 40, 64, 96, 128])
def test_edge_affinity_at_hub_degrees(D, with_daff):
    eu, ev, roles = _hub_affinity_graph()
    S, Su = 1500, int(eu.max()) + 1
    out_deg, in_deg = np.bincount(eu, minlength=S), np.bincount(ev, minlength=S)
    assert set(HUBS) <= set(out_deg.tolist()) and set(HUBS) <= set(in_deg.tolist())
    assert all(x < Su for x in roles["no_out"]) and (out_deg[:Su] == 0).sum() >= 5   # res / dq rows must be written 0
    assert (in_deg == 0).sum() >= 8 and in_deg.max() == 300                          # dk / dv rows 0, and ~300 terms
    if D == 64:      # both sides of the batched path's limit, exactly at it and one past it
        assert {AF_MAXDEG, AF_MAXDEG + 1} <= set(out_deg.tolist())
        assert ((out_deg > 0) & (out_deg <= AF_MAXDEG)).any() and (out_deg > AF_MAXDEG).any()
    if D > 64:       # the per-edge path's d0 loop takes more than one 64-wide pass
        assert (D + 63) // 64 >= 2
    g = torch.Generator(device=DEV).manual_seed(D)
    q, k, v = (torch.randn(S, D, device=DEV, generator=g) for _ in range(3))
    pos = torch.randn(len(eu), device=DEV, generator=g)
    _affinity_case(eu, ev, S, q, k, v, pos, with_daff, 2e-5, seed=D)


@pytest.mark.parametrize("D", [64, 128])
def test_edge_affinity_logits_beyond_expf_range(D):
    """every logit of a source near +95 or -95 (one large channel of q and k), spread by O(1) within the source: an
    unshifted expf overflows (> 88.7) or underflows to 0 there, the softmax must subtract the per-source max"""
    eu, ev, _ = _hub_affinity_graph()
    S = 1500
    g = torch.Generator(device=DEV).manual_seed(3)
    q, k, v = (torch.randn(S, D, device=DEV, generator=g) for _ in range(3))
    big = float(np.sqrt(95.0 * np.sqrt(D)))
    q[:, 0] = big * (1 - 2 * (torch.arange(S, device=DEV) % 2))
    k[:, 0] = big
    pos = 1 + 0.01 * torch.randn(len(eu), device=DEV, generator=g)
    lg = (q.double()[eu] * k.double()[ev]).sum(1) / np.sqrt(D) * pos.double()
    assert float(lg.max()) > 88.8 and float(lg.min()) < -88.8 and float(lg.abs().min()) > 80
    _affinity_case(eu, ev, S, q, k, v, pos, True, 2e-4, seed=5)


# ---------------------------------------------------------------- ECC messages with materialised filters
def _ecc_run(x, w, gout, src, dst, S, C, dw_skew):
    lib = _lib()
    E = src.numel()
    ps, os_ = _csr(src.cpu().numpy(), S)
    pd, od = _csr(dst.cpu().numpy(), S)
    out = _nan(S, C)
    _n.check(lib.wsis_ecc_message_fwd(_n.ptr(x), _n.ptr(w), _n.ptr(dst), _n.ptr(ps), _n.ptr(os_), _n.ptr(out), S, E, C,
                                      _n.stream_ptr()), "ecc_message_fwd")
    dx = _nan(S, C)
    dw = _nan(E * C * C + dw_skew)[dw_skew:].view(E, C, C)
    _n.check(lib.wsis_ecc_message_bwd(_n.ptr(x), _n.ptr(w), _n.ptr(gout), _n.ptr(src), _n.ptr(pd), _n.ptr(od),
                                      _n.ptr(os_), _n.ptr(dx), _n.ptr(dw), S, E, C, _n.stream_ptr()), "ecc_message_bwd")
    torch.cuda.synchronize()
    return {"out": out, "dx": dx, "dw": dw}


def _skewed(t, skew):
    """a copy of ``t`` whose data pointer is ``skew`` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + skew, device=DEV)
    out = buf[skew:].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize("C,skew", [(8, None), (17, None), (31, None), (32, None), (32, "w"), (32, "dout"), (32, "dw")])
def test_ecc_message_at_hub_in_degrees(C, skew):
    S = 1200
    eu, ev, roles = graph_ref.hub_graph(13, S, out_hubs=(33, 65), in_hubs=(63, 64, 65, 130, 300), no_out=4, no_in=4,
                                        isolated=2)
    _, (src_np, dst_np) = graph_ref.edge_orders(eu, ev)       # GraphConvInfo order: sorted by target
    in_deg = np.bincount(dst_np, minlength=S)
    assert {64, 65, 130, 300} <= set(in_deg.tolist()) and (in_deg == 0).any()   # 1, 2, 3 and 5 chunks of 64 edges
    src, dst = torch.from_numpy(src_np).to(DEV), torch.from_numpy(dst_np).to(DEV)
    E = len(src_np)
    g = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randn(S, C, device=DEV, generator=g)
    w = torch.randn(E, C, C, device=DEV, generator=g) * 0.2
    gout = torch.randn(S, C, device=DEV, generator=g)
    if skew == "w":
        w = _skewed(w, 1)
    if skew == "dout":
        gout = _skewed(gout, 1)
    dw_skew = 1 if skew == "dw" else 0
    got = _ecc_run(x, w, gout, src, dst, S, C, dw_skew)
    fast = C == 32 and all(p % 16 == 0 for p in (w.data_ptr(), gout.data_ptr(), got["dw"].data_ptr()))
    assert fast == (C == 32 and skew is None)           # which backward kernel ran (csrc/ecc.hip, wsis_ecc_message_bwd)
    _same(got, _ecc_run(x, w, gout, src, dst, S, C, dw_skew), f"ecc_message C={C}")
    want = graph_ref.ecc_message(x, w, src, dst, S, gout)
    hub = int(in_deg.argmax())
    e = graph_ref.median_edge(dst_np, w.double().abs().sum((1, 2)).cpu().numpy(), hub)
    keep = graph_ref.without_edge(E, e, DEV)
    drop = graph_ref.ecc_message(x, w[keep], src[keep], dst[keep], S, gout)
    drop["dw"] = graph_ref.reinsert(drop["dw"], e)
    graph_ref.check(got, want, drop, 2e-5, f"ecc_message C={C} skew={skew}")


# ---------------------------------------------------------------- ECC contraction, kernel by kernel
def _contract_run(h, U, gms, t_np, S, mean=None):
    """wsis_ecc_contract_fwd, then the backward once per upstream gradient of ``gms``: the first call writes dh, the
    others accumulate into it (wsis_ecc_contract_bwd_acc, or _bwd_mean with ``mean`` = (src, dinps)), each dU of its
    own.  Every output NaN-filled."""
    lib = _lib()
    E = h.shape[0]
    perm, off = _csr(t_np, S)
    m = _nan(E, 32)
    _n.check(lib.wsis_ecc_contract_fwd(_n.ptr(h), _n.ptr(U), _n.ptr(perm), _n.ptr(off), _n.ptr(m), S, E, _n.stream_ptr()),
             "ecc_contract_fwd")
    out = {"m": m, "dh": _nan(E, 64)}
    if mean is not None:
        src_np = mean
        src = torch.from_numpy(src_np).to(DEV)
        _, off_src = _csr(src_np, S)
    for i, gm in enumerate(gms):
        dU = _nan(S, 65 * 32)
        if mean is None:
            _n.check(lib.wsis_ecc_contract_bwd_acc(_n.ptr(h), _n.ptr(U), _n.ptr(gm), _n.ptr(perm), _n.ptr(off), _n.ptr(dU),
                                                   _n.ptr(out["dh"]), S, E, 1 if i else 0, _n.stream_ptr()),
                     "ecc_contract_bwd_acc")
        else:
            _n.check(lib.wsis_ecc_contract_bwd_mean(_n.ptr(h), _n.ptr(U), _n.ptr(gm), _n.ptr(src), _n.ptr(off_src),
                                                    _n.ptr(perm), _n.ptr(off), _n.ptr(dU), _n.ptr(out["dh"]), S, E,
                                                    1 if i else 0, _n.stream_ptr()), "ecc_contract_bwd_mean")
        out[f"dU{i}"] = dU
    torch.cuda.synchronize()
    return out


def _contract_ref(h, U, t, gms, src=None, S=None):
    """fp64: m, dU of every step, dh summed over the steps (gms are dm [E,32], or d_inp [S,32] with ``src``: dm[e] =
    d_inp[src_e] / out-degree(src_e), the backward of the mean)"""
    out = {}
    dh = 0
    for i, gm in enumerate(gms):
        if src is not None:
            cnt = torch.bincount(src, minlength=S).clamp(min=1).double()
            gm = gm.double()[src] / cnt[src].unsqueeze(1)
        r = graph_ref.contract(h, U, t, gm)
        out["m"], out[f"dU{i}"] = r["m"], r["dU"]
        dh = dh + r["dh"]
    out["dh"] = dh
    return out


@pytest.mark.parametrize("mean", [False, True])
def test_ecc_contraction_kernels_at_hub_degrees(mean):
    """ecc_contract_fwd / bwd kernels on a CSR with nodes of 0 (their dU rows must be written as zeros), 7, 8, 9, 16,
    17 and 65 edges (EBATCH = 8 per trip), the backward accumulating into dh over 7 calls"""
    S = 1600
    eu, ev, _ = graph_ref.hub_graph(19, S, out_hubs=GNN_DEG, in_hubs=GNN_DEG, no_out=4, no_in=4, isolated=2)
    _, (t_np, s_np) = graph_ref.edge_orders(eu, ev)    # the module's contraction CSR: edge_indexes[0]
    deg = np.bincount(t_np, minlength=S)
    assert {0, *GNN_DEG} <= set(deg.tolist())
    E = len(t_np)
    g = torch.Generator(device=DEV).manual_seed(19)
    h = torch.randn(E, 64, device=DEV, generator=g)
    U = torch.randn(S, 65 * 32, device=DEV, generator=g) * 0.2
    gms = [torch.randn(S if mean else E, 32, device=DEV, generator=g) for _ in range(7)]
    t = torch.from_numpy(t_np).to(DEV)
    src = torch.from_numpy(s_np).to(DEV) if mean else None
    got = _contract_run(h, U, gms, t_np, S, s_np if mean else None)
    _same(got, _contract_run(h, U, gms, t_np, S, s_np if mean else None), "contraction")
    want = _contract_ref(h, U, t, gms, src, S)
    hub = int(deg.argmax())
    e = int(np.flatnonzero(t_np == hub)[deg[hub] // 2])
    keep = graph_ref.without_edge(E, e, DEV)
    drop = _contract_ref(h[keep], U, t[keep], [gm if mean else gm[keep] for gm in gms], None if src is None else src[keep], S)
    for name in ("m", "dh"):
        drop[name] = graph_ref.reinsert(drop[name], e)
    graph_ref.check(got, want, drop, 2e-5, f"contraction mean={mean}")


# ---------------------------------------------------------------- ECC contraction + GRU recurrence
def _gnn(S, seed):
    import graphnet
    from oracle import network_ref
    torch.manual_seed(seed)
    ref = network_ref.RefRNNGraphConv(32, 7).double().train().to(DEV)
    net = graphnet.GraphNetwork("gru_7_0", 32, [13, 32, 128, 64], fnet_orthoinit=True, fnet_llbias=True, fnet_bnidx=2)
    mod = net.gconvs[0]
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref, mod.to(DEV).train()


def _gnn_run(mod, x, ei, feats, S, go):
    import graphnet
    mod.zero_grad(set_to_none=True)
    mod.set_info(graphnet.GraphConvInfo(ei, feats, S))
    assert mod._contract_ok(x)
    xg = x.clone().requires_grad_(True)
    out = mod(xg)
    out.backward(go)
    torch.cuda.synchronize()
    got = {"out": out.detach(), "dx": xg.grad}
    got.update({n: p.grad.clone() for n, p in mod.named_parameters()})
    return got


def _gnn_ref(ref, x, ei, feats, go):
    ref.zero_grad(set_to_none=True)
    xr = x.double().requires_grad_(True)
    want = ref(xr, ei, feats.double())
    want.backward(go.double())
    out = {"out": want.detach(), "dx": xr.grad}
    out.update({n: p.grad.clone() for n, p in ref.named_parameters()})
    return out


def _gnn_case(ei, feats, S, seed, what):
    """the module and the fp64 oracle on the ECC graph ``ei`` (GraphConvInfo order) with edge features ``feats``; the
    tightness check drops the middle in-edge of the node with the most in-edges (the mean side)"""
    E = ei.shape[1]
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(S, 32, device=DEV, generator=g)
    go = torch.randn(S, 32 * 8, device=DEV, generator=g)
    ref, mod = _gnn(S, seed)
    got = _gnn_run(mod, x, ei, feats, S, go)
    _same(got, _gnn_run(mod, x, ei, feats, S, go), what)
    want = _gnn_ref(ref, x, ei, feats, go)
    dst_np = ei[1].cpu().numpy()
    hub = int(np.bincount(dst_np).argmax())
    e = int(np.flatnonzero(dst_np == hub)[int((dst_np == hub).sum()) // 2])
    drop = _gnn_ref(ref, x, ei[:, graph_ref.without_edge(E, e, DEV)], feats[graph_ref.without_edge(E, e, DEV)], go)
    gmax = max(float(t.abs().max()) for n, t in want.items() if n not in ("out", "dx"))
    # the bias in front of the filter net's BatchNorm has a true gradient of zero (its fp64 reference is rounding noise,
    # ~1e-15 of gmax): measured against 5 % of the largest parameter gradient, as in test_gpu_ops.py, at 1e-3 of that
    # (the fp32 cancellation over E edge rows leaves ~1e-5 of gmax at E = 84 k); every other output and gradient at 1e-4
    # of its own max-abs, with the dropped-edge check
    floor = {n: 5e-2 * gmax for n, t in want.items() if n not in ("out", "dx") and float(t.abs().max()) < 1e-9 * gmax}
    assert list(floor) == ["_fnet.4.bias"], floor
    frac = {n: 1e-3 if n in floor else 1e-4 for n in want}
    return graph_ref.check(got, want, drop, frac, what, floor=floor)


@pytest.mark.parametrize("setting", ["loop", "per_op", "torch_gemm"])
def test_ecc_recurrence_at_hub_degrees(setting, monkeypatch):
    """graphnet.RNNGraphConvModule (7 steps of U = x W', m_e = [h_e, 1] . U_t, mean, GRUCellEx) against the oracle's
    RefRNNGraphConv in fp64 on a graph whose contraction CSR (edge_indexes[0]) and mean CSR (edge_indexes[1]) both hold
    nodes of degree 0, 7, 8, 9, 16, 17 and 65.  loop: the fused recurrence (ecc_u_fwd, gru_fwd_kernel<true>,
    ecc_contract_bwd_kernel<true> accumulating over 7 steps); per_op: WSIS_GNN_LOOP=0 (ecc_contract fwd / bwd<false>,
    scatter-mean, the cell); torch_gemm: WSIS_ECC_OWN_GEMM=0 (torch products, segment reduce, bwd_acc)."""
    env = {"loop": {}, "per_op": {"WSIS_GNN_LOOP": "0"}, "torch_gemm": {"WSIS_ECC_OWN_GEMM": "0"}}[setting]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    S = 1600
    eu, ev, roles = graph_ref.hub_graph(17, S, out_hubs=GNN_DEG, in_hubs=GNN_DEG, no_out=4, no_in=4, isolated=2)
    out_deg, in_deg = np.bincount(eu, minlength=S), np.bincount(ev, minlength=S)
    for deg in (out_deg, in_deg):
        assert {0, *GNN_DEG} <= set(deg.tolist())
    assert (in_deg >= 16).sum() >= 3          # gru_seg_mean: segments that take the unrolled 8 x 2 loop
    _, (src, dst) = graph_ref.edge_orders(eu, ev)
    ei = torch.from_numpy(np.stack([src, dst])).to(DEV)
    feats = torch.randn(ei.shape[1], 13, device=DEV, generator=torch.Generator(device=DEV).manual_seed(18))
    _gnn_case(ei, feats, S, 17, f"recurrence {setting}")


# ---------------------------------------------------------------- GRU cell
def _gru_blocks(S, waves=4, rows_per_wave=3):
    """csrc/gru.hip gru_blocks, restated"""
    return int(min(256, max(1, -(-S // (waves * rows_per_wave)))))


def _gru_run(x, h, p, gy):
    lib = _lib()
    S = x.shape[0]
    hy = _nan(S, 32)
    args = [_n.ptr(t) for t in (x, h, p["ig.weight"], p["ig.bias"], p["weight_ih"], p["weight_hh"], p["bias_ih"],
                                 p["bias_hh"])]
    _n.check(lib.wsis_gru_cell_fwd(*args, _n.ptr(hy), S, 32, _n.stream_ptr()), "gru_cell_fwd")
    out = {"hy": hy, "dx": _nan(S, 32), "dh": _nan(S, 32)}
    out.update({n: torch.full_like(t, NAN) for n, t in p.items()})
    wsb = lib.wsis_gru_cell_workspace_bytes(S)
    ws = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)
    _n.check(lib.wsis_gru_cell_bwd(*args, _n.ptr(gy), _n.ptr(out["dx"]), _n.ptr(out["dh"]), _n.ptr(out["ig.weight"]),
                                   _n.ptr(out["ig.bias"]), _n.ptr(out["weight_ih"]), _n.ptr(out["weight_hh"]),
                                   _n.ptr(out["bias_ih"]), _n.ptr(out["bias_hh"]), S, 32, _n.ptr(ws), wsb,
                                   _n.stream_ptr()), "gru_cell_bwd")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S", [1190, 1536, 2000, 3072, 3073, 9200])
def test_gru_cell_at_slab_counts(S):
    import graphnet
    nb = _gru_blocks(S)
    if S >= 1536:
        assert nb >= 128                   # every slab lane of gru_reduce_kernel takes the 16-slab unrolled loop
    if S > 3072:
        assert nb == 256 and -(-S // (nb * 4)) > 3      # the cap: waves walk more than three rows
    if S == 2000:
        assert 128 < nb < 256 and nb % 128     # the unrolled loop, then the tail loop with slabs left to add
    torch.manual_seed(S)
    cell = graphnet.GRUCellEx(32, 32, bias=True, layernorm=True, ingate=True)
    ref = copy.deepcopy(cell).double().to(DEV)
    p = {n: t.detach().float().to(DEV).contiguous() for n, t in cell.named_parameters()}
    g = torch.Generator(device=DEV).manual_seed(S + 1)
    x, h, gy = (torch.randn(S, 32, device=DEV, generator=g) for _ in range(3))
    got = _gru_run(x, h, p, gy)
    _same(got, _gru_run(x, h, p, gy), f"gru S={S}")
    want = graph_ref.gru(ref, x, h, gy)
    # the last row dropped: its gradient out of every parameter sum, its own rows 0
    gy_drop = gy.clone()
    gy_drop[-1] = 0
    drop = graph_ref.gru(ref, x, h, gy_drop)
    drop["hy"] = want["hy"].clone()
    drop["hy"][-1] = 0
    graph_ref.check(got, want, drop, 2e-5, f"gru S={S}")


# ---------------------------------------------------------------- U = hx @ W'
def _u_run(hx, W):
    U = _nan(hx.shape[0], 65 * 32)
    _n.check(_lib().wsis_ecc_u_fwd(_n.ptr(hx), _n.ptr(W), _n.ptr(U), hx.shape[0], _n.stream_ptr()), "ecc_u_fwd")
    torch.cuda.synchronize()
    return {"U": U}


@pytest.mark.parametrize("S", [1, 31, 33, 129, 9200])
def test_ecc_u_fwd_row_counts(S):
    g = torch.Generator(device=DEV).manual_seed(S)
    hx = torch.randn(S, 32, device=DEV, generator=g)
    W = torch.randn(32, 65 * 32, device=DEV, generator=g)
    got = _u_run(hx, W)
    _same(got, _u_run(hx, W), f"ecc_u_fwd S={S}")
    want = {"U": hx.double() @ W.double()}
    drop = {"U": hx.double()[:, 1:] @ W.double()[1:]}        # one term of the K = 32 sum removed
    graph_ref.check(got, want, drop, 1e-5, f"ecc_u_fwd S={S}")


# ---------------------------------------------------------------- a collated 4-scene batch
@pytest.fixture(scope="module")
def batch4():
    scenes = [harness.bench_scene(seed) for seed in range(1, 5)]
    return harness.collate(scenes)


def test_batch_of_four_scenes(batch4):
    b = batch4
    S = int(b["sp_batch_offsets"][-1])
    eu_np, ev_np = b["edge_u_list"].numpy(), b["edge_v_list"].numpy()
    E = len(eu_np)
    assert S > 9000 and E > 80000
    # the fused recurrence's U product on the batch's row count
    g = torch.Generator(device=DEV).manual_seed(4)
    hx = torch.randn(S, 32, device=DEV, generator=g)
    W = torch.randn(32, 65 * 32, device=DEV, generator=g)
    got = _u_run(hx, W)
    graph_ref.check(got, {"U": hx.double() @ W.double()}, {"U": hx.double()[:, 1:] @ W.double()[1:]}, 1e-5,
                    "ecc_u_fwd batch")
    # position encoding of the affinity graph
    centre = torch.zeros(S, 3, dtype=torch.float64).index_add_(0, b["superpoint"], b["locs_float"].double())
    centre = (centre / torch.bincount(b["superpoint"], minlength=S).clamp(min=1).unsqueeze(1).double()).float().to(DEV)
    torch.manual_seed(4)
    fc = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1)).to(DEV)
    fc64 = copy.deepcopy(fc).double()
    eu, ev = torch.from_numpy(eu_np).to(DEV), torch.from_numpy(ev_np).to(DEV)
    gp = torch.randn(E, device=DEV, generator=g)

    def pe_run():
        fc.zero_grad(set_to_none=True)
        pos = wsis_ops.edge_position_encoding(fc, centre, eu, ev)
        assert pos is not None
        pos.backward(gp)
        torch.cuda.synchronize()
        out = {"pos": pos.detach()}
        out.update({n: p.grad.clone() for n, p in fc.named_parameters()})
        return out

    def pe_ref(keep):
        fc64.zero_grad(set_to_none=True)
        pos = fc64(centre.double()[eu[keep]] - centre.double()[ev[keep]]).view(-1)
        pos.backward(gp[keep].double())
        out = {"pos": pos.detach()}
        out.update({n: p.grad.clone() for n, p in fc64.named_parameters()})
        return out

    got = pe_run()
    _same(got, pe_run(), "pos_enc batch")
    all_e = torch.ones(E, dtype=torch.bool, device=DEV)
    hub = int(np.bincount(eu_np).argmax())
    e = int(np.flatnonzero(eu_np == hub)[0])
    want = pe_ref(all_e)
    drop = pe_ref(graph_ref.without_edge(E, e, DEV))
    drop["pos"] = graph_ref.reinsert(drop["pos"], e)
    graph_ref.check(got, want, drop, 2e-5, "pos_enc batch")
    # the attention on the batch's affinity graph, with the encoded positions
    q, k, v = (torch.randn(S, 64, device=DEV, generator=g) for _ in range(3))
    _affinity_case(eu_np, ev_np, S, q, k, v, got["pos"], True, 2e-5, seed=6)
    # the recurrence on the batch's ECC graph (GraphConvInfo order, the scenes' edge features)
    gi = b["GIs"][0]
    _gnn_case(gi._edge_indexes.to(DEV), gi._edgefeats.float().to(DEV), S, 4, "recurrence batch")
