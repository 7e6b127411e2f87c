"""GPU: the device l0 cut-pursuit solver (wsis_partition.cut_pursuit, csrc/cutpursuit.hip) against the restatement
tests/cut_pursuit_ref.py (itself checked on the CPU in test_cut_pursuit_ref_host.py).

1. min cut: sink side and cut value bit for bit on hand-made and random networks;
2. quantisation: integers come through exactly, real capacities within one step, the scale is a power of two;
3. 2-means, capacities, activation, components, reduced graph, merge and relabelling, stage by stage on the restatement's
   own state, on a 24 x 24 grid and on the k-NN graph of a room of about 2,000 voxels whose features and weights are
   rounded to multiples of 2^-10 (every sum of features is then exact in fp64, so the comparison is exact);
4. the merge on a reduced graph with a hub of 100 borders, ties and gains <= 0;
5. the whole solver on a planted partition; 6. its properties on the room graph; 7. its energy against the restatement's
   seed-to-seed spread; 8. generate_superpoints with no solver argument, and every refusal.

Test 7 on the MI355X: device, seed 0: 264.79725665664057 (23 components); restatement, seeds 0..4: 264.79725665664057,
261.55037080395556, 264.4723715766014, 264.99007385598867, 281.9735039025538 (23, 34, 27, 22, 16 components); DESIGN.md 4.16.
"""
import numpy as np
import pytest
import torch

import cut_pursuit_ref as cp
import partition_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}
LAMBDA = 0.03


def wp():
    import wsis_partition
    return wsis_partition


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to("cuda")


def host(t):
    return t.cpu().numpy()


def dev_arcs(source, target, V):
    return wp().cp_arcs(dev(source, np.int32), dev(target, np.int32), V)


# ---- 1. min cut ------------------------------------------------------------------------------------------------------------

def _concat(nets):
    """disjoint sub-networks in one: node and arc ids shifted"""
    src, snk, source, target, fwd, bwd, base = [], [], [], [], [], [], 0
    for s, k, a, b, cap in nets:
        src.append(s), snk.append(k), source.append(a + base), target.append(b + base)
        fwd.append(cap[:len(a)]), bwd.append(cap[len(a):])
        base += len(s)
    return (np.concatenate(src), np.concatenate(snk), np.concatenate(source).astype(np.int32),
            np.concatenate(target).astype(np.int32), np.concatenate(fwd + bwd).astype(np.int32))


def _chain(n):
    cap = 5 + (np.arange(n - 1) % 3)
    cap[40] = 2
    src, snk = np.zeros(n, np.int32), np.zeros(n, np.int32)
    src[0], snk[n - 1] = 10, 10
    return src, snk, np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32), \
        np.concatenate([cap, np.zeros(n - 1)]).astype(np.int32)


def network(name):
    i32 = lambda *v: np.array(v, dtype=np.int32)                                            # noqa: E731
    if name == "one_node":
        return i32(3), i32(5), i32(), i32(), i32()
    if name == "one_node_source_side":
        return i32(5), i32(5), i32(), i32(), i32()
    if name == "two_nodes":
        return i32(5, 0), i32(0, 4), i32(0), i32(1), i32(3, 1)
    if name == "chain_70":                                   # one source, one sink, the bottleneck in the middle
        return _chain(70)
    if name == "star_300":
        n = 301
        src, snk = np.zeros(n, np.int32), (np.arange(n) % 7).astype(np.int32)
        src[0], snk[0] = 700, 0
        return src, snk, np.zeros(n - 1, np.int32), np.arange(1, n, dtype=np.int32), \
            np.concatenate([np.arange(n - 1) % 5, np.arange(n - 1) % 2]).astype(np.int32)
    if name == "repeated_and_self_loops":
        rng = np.random.default_rng(1)
        V = 20
        a, b = rng.integers(0, V, 60), rng.integers(0, V, 60)
        a, b = np.concatenate([a, b[:30], a[:10], np.arange(5)]), np.concatenate([b, a[:30], b[:10], np.arange(5)])
        d = rng.integers(-9, 10, V)
        return np.maximum(d, 0).astype(np.int32), np.maximum(-d, 0).astype(np.int32), a.astype(np.int32), \
            b.astype(np.int32), rng.integers(1, 4, 2 * len(a)).astype(np.int32)
    if name == "zero_capacities":
        return cp.random_network(200, 4, 10, 3, 2, 5)
    if name == "no_sink":
        s, k, a, b, c = cp.random_network(150, 4, 10, 0, 4, 6)
        return s + k, np.zeros_like(k), a, b, c
    if name == "no_source":
        s, k, a, b, c = cp.random_network(150, 2, 10, 0, 4, 7)
        k = (s + k) * (np.arange(150) % 9 == 0)
        return np.zeros_like(s), k.astype(np.int32), a, b, c
    if name == "six_disjoint":
        return _concat([cp.random_network(V, 3, 12, 4, 5, 20 + V) for V in (1, 2, 7, 40, 150, 333)])
    if name == "random_300":
        return cp.random_network(300, 6, 40, 13, 8, 11)
    if name == "random_5000":
        return cp.random_network(5000, 10, 60, 20, 8, 12)
    raise KeyError(name)


NETWORKS = ["one_node", "one_node_source_side", "two_nodes", "chain_70", "star_300", "repeated_and_self_loops",
            "zero_capacities", "no_sink", "no_source", "six_disjoint", "random_300", "random_5000"]


@pytest.mark.parametrize("name", NETWORKS)
def test_min_cut_bit_exact(name):
    w = wp()
    src, snk, source, target, cap = network(name)
    V = len(src)
    arc = cp.arcs(source, target, V)
    cap = cap[arc["arc"]] if len(cap) else cap
    want, value = cp.min_cut(src, snk, arc, cap)
    arcs = dev_arcs(source, target, V)
    assert np.array_equal(host(arcs.off), arc["off"])
    if len(source):
        for k in ("head", "rev", "edge"):
            assert np.array_equal(host(getattr(arcs, k)), arc[k]), k
    side, cut, rounds = w.cp_min_cut(dev(src), dev(snk), arcs, dev(cap))
    print(f"{name}: V = {V}, A = {len(cap)}, cut = {value}, sink side = {int(want.sum())}, rounds = {rounds}")
    assert rounds < w.FLOW_ROUND_CAP
    assert int(cut) == value
    assert np.array_equal(host(side), want)
    if name.startswith("random"):
        assert 0.1 * V <= want.sum() <= 0.9 * V
    if name == "no_sink":
        assert not want.any()
    if name == "chain_70":
        assert value == 2 and want.sum() == 29


def test_min_cut_refuses_to_go_past_its_round_cap():
    """200 nodes in a row: the excess moves one node per sweep inside a wavefront, so the 64 sweeps of one round cannot
    carry it through the second wavefront's 64 nodes -- one round is never enough, and the call must say so"""
    w = wp()
    src, snk, source, target, cap = _chain(200)
    arc = cp.arcs(source, target, 200)
    with pytest.raises(w._n.WsisError):
        w.cp_min_cut(dev(src), dev(snk), dev_arcs(source, target, 200), dev(cap[arc["arc"]]), max_rounds=1)
    side, cut, rounds = w.cp_min_cut(dev(src), dev(snk), dev_arcs(source, target, 200), dev(cap[arc["arc"]]))
    assert int(cut) == 2 and host(side).sum() == 159 and 1 < rounds < w.FLOW_ROUND_CAP


# ---- 2. quantisation --------------------------------------------------------------------------------------------------------

def _quantize(term, weight, lam):
    w = wp()
    E = len(weight)
    source, target = np.arange(E, dtype=np.int32) % len(term), (np.arange(E, dtype=np.int32) * 7 + 1) % len(term)
    arc = cp.arcs(source, target, len(term))
    arcs = dev_arcs(source, target, len(term))
    src, snk, cap, scale = w.cp_quantize(dev(term), dev(weight), None, lam, arcs)
    want = cp.quantize(term, weight, None, lam, arc["edge"])
    scale = float(scale[0])
    assert scale == want[3] and np.frexp(scale)[0] == 0.5
    for got, exp in zip((src, snk, cap), want):
        assert np.array_equal(host(got), exp)
    return host(src).astype(np.float64) - host(snk), host(cap)[np.argsort(arc["arc"])][:E].astype(np.float64), scale


def test_quantize_integers_exactly():
    rng = np.random.default_rng(3)
    term = rng.integers(-2 ** 24 + 1, 2 ** 24, 5000).astype(np.float64)
    weight = rng.integers(0, 2 ** 24, 3000).astype(np.float32)
    t, c, scale = _quantize(term, weight, 1.0)                       # largest < 2^24: scale 2^-6, an exact multiple
    assert scale == 2.0 ** -6 and np.array_equal(t * scale, term) and np.array_equal(c * scale, weight)
    term[0] = 2.0 ** 29                                                # largest in [2^29, 2^30): scale 1, the integers themselves
    t, c, scale = _quantize(term, weight, 1.0)
    assert scale == 1.0 and np.array_equal(t, term) and np.array_equal(c, weight)


def test_quantize_reals_within_one_step():
    rng = np.random.default_rng(4)
    term, weight = rng.normal(0, 3, 5000), rng.random(3000).astype(np.float32)
    t, c, scale = _quantize(term, weight, LAMBDA)
    assert np.abs(t * scale - term).max() <= scale
    assert np.abs(c * scale - LAMBDA * weight.astype(np.float64)).max() <= scale
    t, c, scale = _quantize(np.zeros(10), np.zeros(4, np.float32), LAMBDA)
    assert scale == 1.0 and not t.any() and not c.any()


# ---- the graphs of 3., 5., 6. and 7. ------------------------------------------------------------------------------------------

def grid_graph(n=24):
    idx = np.arange(n * n).reshape(n, n)
    source = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]).astype(np.int32)
    target = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]).astype(np.int32)
    return source, target


def quadrants(n=24):
    i = np.arange(n)
    return ((i[:, None] >= n // 2) * 2 + (i[None, :] >= n // 2)).ravel()


def planted_features(n=24):
    vals = np.array([[0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0]], dtype=np.float32)
    return vals[quadrants(n)]


def room_inputs():
    """``partition_inputs`` of a room of about 2,000 voxels (device), and its arrays on the host"""
    if "room" not in _CACHE:
        xyz, rgb = ref.make_room(9, n=5000, size=(0.7, 0.6, 0.5))
        inputs = wp().partition_inputs(xyz, rgb)
        f = torch.nan_to_num(inputs.features)
        inputs = inputs._replace(features=f)
        _CACHE["room"] = (inputs, host(f), host(inputs.source), host(inputs.target), host(inputs.edge_weight))
        assert 1500 <= len(host(f)) <= 3000
    return _CACHE["room"]


def dyadic(a):
    return (np.round(np.asarray(a, dtype=np.float64) * 1024) / 1024).astype(np.float32)


def stage_graph(name):
    if name == "grid":
        source, target = grid_graph()
        rng = np.random.default_rng(2)
        f = dyadic(planted_features() + rng.normal(0, 0.3, (576, 7)))
        return f, source, target, np.ones(len(source), np.float32)
    _, f, source, target, weight = room_inputs()
    return dyadic(f), source, target, dyadic(weight)


# ---- 3. the stages, on the restatement's state ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "room"])
def test_stages_follow_the_restatement(name):
    w = wp()
    f, source, target, weight = stage_graph(name)
    V, E = len(f), len(source)
    fd, sd, td, wd = dev(f), dev(source), dev(target), dev(weight)
    arc, arcs = cp.arcs(source, target, V), dev_arcs(source, target, V)
    comp, C, sat, active = np.zeros(V, np.int32), 1, np.zeros(1, np.uint8), np.zeros(E, np.uint8)
    off, nodes = cp.components_of(comp, C)
    for it in (1, 2, 3):
        offd, nodesd = w.cp_components(dev(comp), C)
        assert np.array_equal(host(offd), off) and np.array_equal(host(nodesd), nodes)
        label = cp.kmeans(f, off, nodes, sat, 0, it)
        assert np.array_equal(host(w.cp_kmeans(fd, offd, nodesd, dev(sat), 0, it)), label), f"2-means, iteration {it}"
        for step in range(cp.FLOW_STEPS):
            satd = dev(sat)
            centres, term, sat = cp.capacities(f, off, nodes, label, sat)
            centresd, termd = w.cp_capacities(fd, offd, nodesd, dev(label), satd)
            assert np.array_equal(host(satd), sat)
            assert np.array_equal(host(centresd), centres) and np.array_equal(host(termd), term), f"capacities {it}.{step}"
            src, snk, cap, scale = cp.quantize(term, weight, active, LAMBDA, arc["edge"])
            srcd, snkd, capd, scaled = w.cp_quantize(termd, wd, dev(active), LAMBDA, arcs)
            assert float(scaled[0]) == scale
            assert all(np.array_equal(host(a), b) for a, b in ((srcd, src), (snkd, snk), (capd, cap)))
            label, value = cp.min_cut(src, snk, arc, cap)
            side, cut, rounds = w.cp_min_cut(srcd, snkd, arcs, capd)
            assert rounds < w.FLOW_ROUND_CAP and int(cut) == value and np.array_equal(host(side), label), f"flow {it}.{step}"
        satd, actived = dev(sat), dev(active)
        compd, sat_newd, Cd = w.cp_activate(sd, td, dev(label), dev(comp), offd, nodesd, satd, actived)
        comp, sat_new, C, active, sat = cp.activate(source, target, label, comp, off, nodes, sat, active)
        assert Cd == C and np.array_equal(host(compd), comp) and np.array_equal(host(sat_newd), sat_new)
        assert np.array_equal(host(satd), sat) and np.array_equal(host(actived), active)
        sat = sat_new
        off, nodes = cp.components_of(comp, C)
        offd, nodesd = w.cp_components(compd, C)
        red = cp.reduce(f, source, target, weight, comp, off, nodes, LAMBDA)
        redd = w.cp_reduce(fd, sd, td, wd, compd, offd, nodesd, LAMBDA)
        assert np.array_equal(host(redd.mean), red["mean"]) and np.array_equal(host(redd.weight), red["weight"])
        assert np.array_equal(host(redd.a), red["a"]) and np.array_equal(host(redd.b), red["b"])
        assert np.array_equal(host(redd.border_weight), red["border_weight"]) and np.array_equal(host(redd.gain), red["gain"])
        taken = cp.merge_sequential(red["a"], red["b"], red["gain"], C)
        takend, cmapd, _ = w.cp_merge(redd.a, redd.b, redd.gain, C)
        assert np.array_equal(host(takend).astype(bool), taken)
        actived = dev(active)
        comp, sat, C, active = cp.relabel(red["a"], red["b"], taken, comp, sat, source, target, active)
        compd, satd, Cd = w.cp_relabel(cmapd, sd, td, compd, dev(sat_new), actived)
        assert Cd == C and np.array_equal(host(compd), comp) and np.array_equal(host(satd), sat)
        assert np.array_equal(host(actived), active)
        off, nodes = cp.components_of(comp, C)
        offd, nodesd = w.cp_components(compd, C)
        fid, pen, nsat = w.cp_energy(fd, compd, w.cp_values(fd, offd, nodesd)[0], sd, td, wd, LAMBDA, satd)
        want = cp.energy(f, source, target, weight, LAMBDA, comp)
        assert abs(fid - want[0]) <= 1e-12 * want[0] and abs(pen - want[1]) <= 1e-12 * max(want[1], 1e-300)
        assert nsat == int(np.diff(off)[sat.astype(bool)].sum())
        print(f"{name}: iteration {it}: {C} components, {nsat} nodes saturated, energy {fid + pen:.6f}")
    assert C > 1


def test_component_shapes():
    """singletons, one node beside a component of 1,500, and a chain of 1,000 nodes in shuffled id order"""
    w = wp()
    rng = np.random.default_rng(8)
    V = 1000 + 1500 + 1 + 20
    ids = rng.permutation(V)
    chain, blob, lone = ids[:1000], ids[1000:2500], ids[2500]
    source = np.concatenate([chain[:-1], blob[:-1], blob[rng.integers(0, 1500, 3000)], [lone, blob[7]], [lone]])
    target = np.concatenate([chain[1:], blob[1:], blob[rng.integers(0, 1500, 3000)], [blob[3], lone], [lone]])
    label = np.zeros(V, np.uint8)
    label[lone] = 1
    f = dyadic(rng.normal(0, 1, (V, 7)))
    comp0, sat0, active0 = np.zeros(V, np.int32), np.zeros(1, np.uint8), np.zeros(len(source), np.uint8)
    off, nodes = cp.components_of(comp0, 1)
    offd, nodesd = w.cp_components(dev(comp0), 1)
    actived = dev(active0)
    compd, satd, Cd = w.cp_activate(dev(source, np.int32), dev(target, np.int32), dev(label), dev(comp0), offd, nodesd,
                                    dev(sat0), actived)
    comp, sat, C, active, _ = cp.activate(source, target, label, comp0, off, nodes, sat0, active0)
    assert C == Cd == 23 and np.array_equal(host(compd), comp) and np.array_equal(host(actived), active)
    assert active.sum() == 2 and not host(satd).any()
    sizes = np.bincount(comp)
    assert sorted(sizes)[-2:] == [1000, 1500] and (sizes == 1).sum() == 21
    off, nodes = cp.components_of(comp, C)
    offd, nodesd = w.cp_components(compd, C)
    label = cp.kmeans(f, off, nodes, sat, 5, 2)
    assert np.array_equal(host(w.cp_kmeans(dev(f), offd, nodesd, satd, 5, 2)), label)
    assert label[chain].any() and not label[chain].all() and not label[lone]
    centres, term, sat = cp.capacities(f, off, nodes, label, sat)
    centresd, termd = w.cp_capacities(dev(f), offd, nodesd, dev(label), satd)
    assert np.array_equal(host(termd), term) and np.array_equal(host(centresd), centres) and np.array_equal(host(satd), sat)
    assert sat.sum() == 21


# ---- 4. merge ----------------------------------------------------------------------------------------------------------------

def test_merge_with_a_hub_of_100_borders():
    w = wp()
    rng = np.random.default_rng(13)
    C = 140
    a = np.concatenate([np.zeros(100, np.int64), rng.integers(1, C - 1, 260)])
    b = np.concatenate([np.arange(1, 101), np.zeros(260, np.int64)])
    b[100:] = a[100:] + 1 + rng.integers(0, C - 1 - a[100:])
    gain = rng.integers(-3, 6, len(a)).astype(np.float64) * 0.125
    order = np.lexsort((b, a))
    a, b, gain = a[order], b[order], gain[order]
    want = cp.merge_sequential(a, b, gain, C)
    taken, cmap, rounds = w.cp_merge(dev(a, np.int32), dev(b, np.int32), dev(gain), C)
    print(f"merge: {int(want.sum())} of {len(a)} borders taken in {rounds} rounds")
    assert np.array_equal(host(taken).astype(bool), want)
    assert want[:100].sum() == 1 and (gain <= 0).any() and not want[gain <= 0].any()
    exp = np.arange(C)
    exp[b[want]] = a[want]
    assert np.array_equal(host(cmap), exp)
    taken, cmap, _ = w.cp_merge(dev(a[:0], np.int32), dev(b[:0], np.int32), dev(gain[:0]), C)
    assert np.array_equal(host(cmap), np.arange(C))


# ---- 5. the whole solver, planted --------------------------------------------------------------------------------------------

def test_planted_quadrants():
    w = wp()
    source, target = grid_graph()
    f, ones = planted_features(), np.ones(len(source), np.float32)
    (comps, ids, info) = w.cut_pursuit(f, source.view(np.uint32), target.view(np.uint32), ones, LAMBDA, info=True)
    assert np.array_equal(ids, quadrants()) and ids.dtype == np.uint32
    assert info.stopped == "saturated" and info.components[-1] == 4 and info.saturated[-1] == 576
    assert len(comps) == 4 and all(np.array_equal(c, np.nonzero(quadrants() == i)[0]) for i, c in enumerate(comps))
    assert info.fidelity[-1] == 0 and abs(info.penalty[-1] - LAMBDA * 48) < 1e-12
    _, ids, info = w.cut_pursuit(f, source.view(np.uint32), target.view(np.uint32), ones, 1e6, info=True)
    assert not ids.any() and info.components == [1] and info.stopped == "saturated"
    q3 = np.nonzero((quadrants()[source] == 3) & (quadrants()[target] == 3))[0]
    source2, target2 = np.concatenate([source, source[q3], target[q3]]), np.concatenate([target, target[q3], source[q3]])
    _, ids = w.cut_pursuit(f, source2.view(np.uint32), target2.view(np.uint32), np.ones(len(source2), np.float32), LAMBDA)
    assert np.array_equal(ids, quadrants())
    _, ids = w.cut_pursuit(f, source[:0].view(np.uint32), target[:0].view(np.uint32), ones[:0], LAMBDA)      # no edges
    assert ids.max() > 0


# ---- 6. the whole solver, properties -----------------------------------------------------------------------------------------

def room_solution():
    if "solution" not in _CACHE:
        inputs = room_inputs()[0]
        _CACHE["solution"] = wp().cut_pursuit(inputs.features, inputs.source, inputs.target, inputs.edge_weight, LAMBDA,
                                              info=True)
    return _CACHE["solution"]


def test_room_partition_properties():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    w = wp()
    inputs, f, source, target, weight = room_inputs()
    (off, nodes), ids, info = room_solution()
    ids, off, nodes = host(ids), host(off), host(nodes)
    V, C = len(f), len(off) - 1
    assert ids.dtype == np.int32 and np.array_equal(np.unique(ids), np.arange(C)) and C == info.components[-1]
    assert np.array_equal(cp.canonical(ids)[0], ids)
    inner = ids[source] == ids[target]
    n, _ = connected_components(coo_matrix((np.ones(inner.sum()), (source[inner], target[inner])), shape=(V, V)), directed=False)
    assert n == C
    want_off, want_nodes = cp.components_of(ids, C)
    assert np.array_equal(off, want_off) and np.array_equal(nodes, want_nodes)
    total = np.array(info.fidelity) + np.array(info.penalty)
    one = cp.energy(f, source, target, weight, LAMBDA, np.zeros(V, np.int64))[0]
    print(f"room: V = {V}, components {info.components}, saturated {info.saturated}, energies {total.tolist()}, "
          f"one component {one}, flow rounds {info.flow_rounds}, stopped on '{info.stopped}'")
    assert (np.diff(total) <= 0).all()
    fid, pen = cp.energy(f, source, target, weight, LAMBDA, ids)
    assert abs(fid + pen - total[-1]) <= 1e-9 * total[-1]
    assert total[-1] < one and 1 < C < V
    assert max(info.flow_rounds) < w.FLOW_ROUND_CAP
    (off2, nodes2), ids2, info2 = w.cut_pursuit(inputs.features, inputs.source, inputs.target, inputs.edge_weight, LAMBDA,
                                                info=True)
    same = lambda a, b: (a[:4], a.stopped) == (b[:4], b.stopped)              # noqa: E731 (the rounds a flow takes may differ)
    assert torch.equal(ids2.cpu(), torch.from_numpy(ids)) and same(info2, info)
    assert torch.equal(off2.cpu(), torch.from_numpy(off)) and torch.equal(nodes2.cpu(), torch.from_numpy(nodes))
    comps, ids3 = w.cut_pursuit(f, source.view(np.uint32), target.view(np.uint32), weight, LAMBDA)
    assert np.array_equal(ids3, ids.astype(np.uint32))
    assert len(comps) == C and all(np.array_equal(c, nodes[off[i]:off[i + 1]]) for i, c in enumerate(comps))


# ---- 7. the whole solver against the restatement -------------------------------------------------------------------------------

def test_room_energy_within_the_restatements_spread():
    """the start of the 2-means is the only declared source of divergence, so the restatement's own seed-to-seed spread is
    the margin: E(device, seed 0) <= max_ref + (max_ref - min_ref) over the restatement's seeds 0..4"""
    _, f, source, target, weight = room_inputs()
    _, ids, info = room_solution()
    mine = sum(cp.energy(f, source, target, weight, LAMBDA, host(ids)))
    theirs, counts = [], []
    for seed in range(5):
        comp, run = cp.solve(f, source, target, weight, LAMBDA, seed)
        theirs.append(sum(cp.energy(f, source, target, weight, LAMBDA, comp)))
        counts.append(run["components"][-1])
    print(f"device seed 0: energy {mine!r}, {info.components[-1]} components; restatement seeds 0..4: energies {theirs}, "
          f"components {counts}")
    assert mine <= max(theirs) + (max(theirs) - min(theirs))


# ---- 8. generate_superpoints without a solver; the refusals ------------------------------------------------------------------

def test_generate_superpoints_with_the_device_solver():
    w = wp()
    xyz, rgb = ref.make_room(9, n=30000, size=(2.0, 1.5, 1.2))
    ids = w.generate_superpoints(xyz, rgb)
    inputs = w.partition_inputs(xyz, rgb)
    _, comp = w.cut_pursuit(inputs.features, inputs.source, inputs.target, inputs.edge_weight, LAMBDA)
    V = int(inputs.xyz.shape[0])
    assert ids.shape == (len(xyz),) and np.array_equal(ids, host(inputs.to_points(comp)))
    assert 1 < len(np.unique(ids)) < V


def test_refusals():
    w = wp()
    err = w._n.WsisError
    source, target = grid_graph()
    f, ones = planted_features(), np.ones(len(source), np.float32)
    s, t = source.view(np.uint32), target.view(np.uint32)
    with pytest.raises(err):
        w.cut_pursuit(torch.from_numpy(f), torch.from_numpy(source), torch.from_numpy(target), torch.from_numpy(ones), LAMBDA,
                      device="cpu")
    for bad in ((f.astype(np.float64), s, t, ones), (f, s.astype(np.int64), t, ones), (f, s, t, ones.astype(np.float64)),
                (f, s, t[:-1], ones), (f, s, t, ones[:-1]), (f[:0], s[:0], t[:0], ones[:0])):
        with pytest.raises(err):
            w.cut_pursuit(*bad, LAMBDA)
    far = s.copy()
    far[5] = 576
    nan, neg = ones.copy(), ones.copy()
    nan[3], neg[3] = np.nan, -1
    for bad in ((f, far, t, ones), (f, s, t, nan), (f, s, t, neg)):
        with pytest.raises(err):
            w.cut_pursuit(*bad, LAMBDA)
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(err):
            w.cut_pursuit(f, s, t, ones, lam)
    for kw in ({"cutoff": 10}, {"spatial": 1}, {"weight_decay": 0.7}):
        with pytest.raises(err):
            w.cut_pursuit(f, s, t, ones, LAMBDA, **kw)
    with pytest.raises(err):
        w.cut_pursuit(f, s, t, ones, LAMBDA, 10)
