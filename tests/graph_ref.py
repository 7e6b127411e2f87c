"""Graphs with exact hub degrees and fp64 references of the superpoint-graph operators for the GPU value tests
(tests/test_gpu_graph_edges.py), in the style of tests/conv_ref.py.

  hub_graph      a seeded directed graph without self-loops or duplicate edges in which chosen nodes have an exact
                 out-degree or in-degree (31, 32, 33, 63, 64, 65, 129, ~300 ...), plus nodes without out-edges, nodes
                 without in-edges and isolated nodes; edges in sorted-tuple order, as a scene stores them
  edge_orders    the reference's two edge orders, as harness.collate builds them
  affinity / ecc_message / contract / gru
                 fp64 references (oracle.affinity_ref.edge_affinity, the ECC mean message, m_e = [h_e, 1] . U_t,
                 GRUCellEx.forward_reference), evaluated on the device in float64
  check          every output and gradient within a fraction of the reference's max-abs, and proof that the fraction is
                 tight: the reference recomputed with ONE edge of the largest hub removed must fail the same bound"""
import numpy as np
import torch

from oracle import affinity_ref, scatter_ref


def hub_graph(seed, S, out_hubs=(), in_hubs=(), bg=(1, 4), no_out=0, no_in=0, isolated=0):
    """(eu, ev) int64 numpy in sorted-tuple order and the roles {out_hub: {node: degree}, in_hub: {node: degree},
    no_out, no_in, isolated: [nodes]}.  Out-hub u has exactly out_hubs[i] out-edges; in-hub t has exactly in_hubs[i]
    in-edges; every other node that may have out-edges gets bg[0]..bg[1] of them (plus the edges it gives to in-hubs).
    Node S - 1 is an ordinary source, so every no-out node lies inside [0, max(eu) + 1)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(S - 1)
    cut = np.cumsum([len(out_hubs), len(in_hubs), no_out, no_in, isolated])
    assert cut[-1] < S - 1
    ohub, ihub, nout, nin, iso = np.split(perm[:cut[-1]], cut[:-1])
    ihub_set, nout_set, nin_set, iso_set, ohub_set = set(ihub), set(nout), set(nin), set(iso), set(ohub)
    targets = np.array([t for t in range(S) if t not in ihub_set and t not in nin_set and t not in iso_set])
    givers = np.array([s for s in range(S) if s not in ohub_set and s not in nout_set and s not in iso_set])
    edges = set()

    def pick(pool, n, me):
        pool = pool[pool != me]
        assert len(pool) >= n, (len(pool), n)
        return rng.choice(pool, size=n, replace=False)

    for u, d in zip(ohub, out_hubs):
        edges.update((int(u), int(t)) for t in pick(targets, d, u))
    for u in givers:
        edges.update((int(u), int(t)) for t in pick(targets, int(rng.integers(bg[0], bg[1] + 1)), u))
    for t, d in zip(ihub, in_hubs):
        edges.update((int(s), int(t)) for s in pick(givers, d, t))
    e = np.array(sorted(edges), dtype=np.int64)
    roles = {"out_hub": dict(zip(map(int, ohub), out_hubs)), "in_hub": dict(zip(map(int, ihub), in_hubs)),
             "no_out": [int(x) for x in nout], "no_in": [int(x) for x in nin], "isolated": [int(x) for x in iso]}
    eu, ev = e[:, 0], e[:, 1]
    out_deg, in_deg = np.bincount(eu, minlength=S), np.bincount(ev, minlength=S)
    assert (eu != ev).all()
    assert all(out_deg[u] == d for u, d in roles["out_hub"].items())
    assert all(in_deg[t] == d for t, d in roles["in_hub"].items())
    assert all(out_deg[x] == 0 for x in roles["no_out"] + roles["isolated"])
    assert all(in_deg[x] == 0 for x in roles["no_in"] + roles["isolated"])
    assert eu.max() == S - 1
    return eu, ev, roles


def edge_orders(eu, ev):
    """the two edge orders of harness._assemble_host: the scene's sorted-tuple order (edge_u_list / edge_v_list, the
    affinity graph) and the stable sort by target (GraphConvInfo's edge_indexes, the ECC graph)"""
    order = np.argsort(ev, kind="stable")
    return (eu, ev), (eu[order], ev[order])


def without_edge(n_edges, e, dev):
    """index of every edge but ``e``"""
    keep = torch.ones(n_edges, dtype=torch.bool, device=dev)
    keep[e] = False
    return keep


def reinsert(t, e):
    """a per-edge tensor of the one-edge-removed reference back at full length, the removed edge's row 0 (what a
    kernel that dropped the edge would leave behind)"""
    return torch.cat([t[:e], torch.zeros_like(t[:1]), t[e:]])


def median_edge(end, weight, node):
    """the edge with ``end`` (per-edge node array: sources or targets) == ``node`` whose ``weight`` (per-edge array) is
    the median of those edges' weights"""
    es = np.flatnonzero(end == node)
    return int(es[np.argsort(weight[es], kind="stable")[len(es) // 2]])


# ---- fp64 references (device, float64) ------------------------------------------------------------------------------
def affinity(q, k, v, pos, eu, ev, ga, gr):
    """oracle edge attention in fp64 and its gradient for the upstream (ga [E] or None, gr [Su, D]):
    {aff, res, dq, dk, dv, dpos}"""
    t = [x.detach().double().requires_grad_(True) for x in (q, k, v, pos)]
    aff, res = affinity_ref.edge_affinity(*t, eu, ev)
    loss = (res * gr.double()).sum()
    if ga is not None:
        loss = loss + (aff * ga.double()).sum()
    loss.backward()
    return {"aff": aff.detach(), "res": res.detach(), "dq": t[0].grad, "dk": t[1].grad, "dv": t[2].grad,
            "dpos": t[3].grad}


def ecc_message(x, w, src, dst, S, gout):
    """out[s] = mean_{e: src_e = s} x[dst_e] @ W_e in fp64 and its gradient for ``gout``: {out, dx, dw}"""
    xr, wr = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    msg = torch.matmul(xr[dst].unsqueeze(1), wr).squeeze(1)
    out = scatter_ref.scatter(msg, src, 0, S, "mean")
    out.backward(gout.double())
    return {"out": out.detach(), "dx": xr.grad, "dw": wr.grad}


def contract(h, U, dst, gm):
    """m_e = [h_e, 1] . U[dst_e].view(65, 32) in fp64 and its gradient for ``gm``: {m, dU, dh}"""
    hr, Ur = h.detach().double().requires_grad_(True), U.detach().double().requires_grad_(True)
    haug = torch.cat([hr, torch.ones_like(hr[:, :1])], 1)
    m = torch.bmm(haug.unsqueeze(1), Ur[dst].view(-1, 65, 32)).squeeze(1)
    m.backward(gm.double())
    return {"m": m.detach(), "dU": Ur.grad, "dh": hr.grad}


def gru(cell64, x, h, gy):
    """GRUCellEx.forward_reference of a float64 copy of the cell and its gradient for ``gy``:
    {hy, dx, dh, <parameter name>: gradient}"""
    cell64.zero_grad(set_to_none=True)
    xr, hr = x.detach().double().requires_grad_(True), h.detach().double().requires_grad_(True)
    hy = cell64.forward_reference(xr, hr)
    hy.backward(gy.double())
    out = {"hy": hy.detach(), "dx": xr.grad, "dh": hr.grad}
    out.update({n: p.grad.clone() for n, p in cell64.named_parameters()})
    return out


# ---- comparison ------------------------------------------------------------------------------------------------------
def check(got, want, drop, frac, what, floor=None):
    """for every name of ``want``: ``got`` finite (a row no kernel writes stays NaN) and within frac * max|want| of it,
    and ``drop`` (the reference with one hub edge removed, per-edge rows re-inserted as 0) more than that bound away
    from ``got``.  ``frac`` a number or {name: number}; ``floor`` {name: scale}: the scale of a gradient whose true value
    is 0 (its reference is rounding noise, at most 1e-6 of the floor -- asserted); only those are not asked to see the
    dropped edge.  Returns {name: (err, bound, err_drop)}."""
    rep = {}
    for name, w in want.items():
        g = got[name].detach()
        f = frac[name] if isinstance(frac, dict) else frac
        assert g.shape == w.shape, (what, name, tuple(g.shape), tuple(w.shape))
        assert bool(torch.isfinite(g).all()), f"{what} {name}: non-finite values (an unwritten row or element)"
        scale = float(w.abs().max()) if w.numel() else 0.0
        tight = True
        if floor and name in floor:
            assert scale <= 1e-6 * floor[name], f"{what} {name}: max|ref| {scale:.3e} is no rounding noise to floor"
            scale, tight = floor[name], False
        bound = f * scale
        err = float((g.double() - w).abs().max()) if w.numel() else 0.0
        err_drop = float((g.double() - drop[name]).abs().max())
        rep[name] = (err, bound, err_drop)
        assert err <= bound, f"{what} {name}: max abs error {err:.3e} > {bound:.3e} ({f:g} of max|ref| {scale:.3e})"
        if tight:
            assert err_drop > bound, f"{what} {name}: the bound {bound:.3e} would not see a dropped edge ({err_drop:.3e})"
    return rep
