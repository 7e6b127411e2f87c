"""numpy / scipy restatement of the device l0 cut-pursuit solver (3d-wsis_amd/wsis_partition.py ``cut_pursuit``,
csrc/cutpursuit.hip): the same hash, quantisation and stage definitions, each function citing the part of
the reference's data/S3DIS/partition/cut-pursuit it follows.

* the maximum flow is ``scipy.sparse.csgraph.maximum_flow`` on int32 capacities, the sink side a reverse breadth-first
  search from the sink over the residual graph: the set of nodes the sink can be reached from is the same for every
  maximum flow (and maximum preflow), which is what makes the device's push-relabel comparable bit for bit;
* the merge is the sequential walk over the borders sorted by (gain descending, index ascending) of CutPursuit.h merge;
  ``merge_rounds`` is the locally-dominant form the device runs;
* sums are float64.  Where the features are multiples of 2^-10 every sum of features and of squared distances to a
  feature is exact, so the order of summation does not show and the stages can be compared exactly.
"""
import numpy as np
from scipy.sparse import coo_matrix, csr_matrix
from scipy.sparse.csgraph import breadth_first_order, connected_components, maximum_flow

FLOW_STEPS, KMEANS_ITE, KMEANS_RESAMPLING, MAX_ITE_MAIN, STOPPING_RATIO = 3, 5, 10, 15, 0.05
M32 = 0xffffffff


# ---- the random stream ---------------------------------------------------------------------------------------------------

def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw(seed, iteration, restart, root, k):
    h = mix((int(seed) & M32) ^ 0x9e3779b9)
    for v in (iteration, restart, root, k):
        h = mix((h + int(v)) & M32)
    return h


# ---- arcs: API.h:959-974 --------------------------------------------------------------------------------------------------

def arcs(source, target, V):
    """-> dict off [V+1], head, rev, edge [2E]: arc a < E is source[a] -> target[a], a + E its reverse, sorted by tail"""
    source, target = np.asarray(source, dtype=np.int64), np.asarray(target, dtype=np.int64)
    E = len(source)
    tails = np.concatenate([source, target])
    heads = np.concatenate([target, source])
    perm = np.argsort(tails, kind="stable")
    inv = np.empty(2 * E, dtype=np.int64)
    inv[perm] = np.arange(2 * E)
    off = np.concatenate([[0], np.cumsum(np.bincount(tails, minlength=V))]).astype(np.int64)
    return {"off": off, "head": heads[perm], "rev": inv[(perm + E) % (2 * E)] if E else perm, "edge": perm % max(E, 1),
            "tail": tails[perm], "arc": perm}


def components_of(in_component, C):
    """(off [C+1], nodes [V]): the nodes of every component, ascending"""
    in_component = np.asarray(in_component, dtype=np.int64)
    nodes = np.argsort(in_component, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(in_component, minlength=C))])
    return off, nodes


# ---- 2-means: CutPursuit_L2.h init_labels -----------------------------------------------------------------------------------

def dist2(x, k):
    s = np.zeros(len(x), dtype=np.float64)
    for d in range(x.shape[1]):
        t = x[:, d] - k[d]
        s = s + t * t
    return s


def kmeans(features, off, nodes, sat, seed, iteration, restarts=KMEANS_RESAMPLING, kmeans_ite=KMEANS_ITE):
    f = np.asarray(features, dtype=np.float32).astype(np.float64)
    label = np.zeros(len(f), dtype=np.uint8)
    for c in range(len(off) - 1):
        idx = nodes[off[c]:off[c + 1]]
        n = len(idx)
        if sat[c] or n <= 1:
            continue
        x = f[idx]
        root = int(idx[0])
        best = np.inf
        for r in range(restarts):
            k0 = x[draw(seed, iteration, r, root, 0) % n].copy()
            e = dist2(x, k0)
            thresh = np.float64(e.sum()) * (np.float64(draw(seed, iteration, r, root, 1)) * (1.0 / 4294967296.0))
            over = np.nonzero(np.cumsum(e) > thresh)[0]
            k1 = x[over[0] if len(over) else 0].copy()
            for _ in range(kmeans_ite):
                pot = dist2(x, k0) > dist2(x, k1)
                if pot.all() or not pot.any():
                    break
                k0, k1 = x[pot].sum(0) / np.float64(pot.sum()), x[~pot].sum(0) / np.float64((~pot).sum())
            energy = np.where(pot, dist2(x, k0), dist2(x, k1)).sum()
            if energy < best:
                best = energy
                label[idx] = pot
    return label


# ---- capacities: CutPursuit_L2.h compute_center, set_capacities -----------------------------------------------------------

def capacities(features, off, nodes, label, sat):
    """-> (centres [C,2,D], term [V], sat): term = cost_B - cost_notB, 0 in saturated components"""
    f = np.asarray(features, dtype=np.float32).astype(np.float64)
    C, D = len(off) - 1, f.shape[1]
    centres, term, sat = np.zeros((C, 2, D)), np.zeros(len(f)), np.array(sat, dtype=np.uint8)
    for c in range(C):
        idx = nodes[off[c]:off[c + 1]]
        lab = label[idx].astype(bool)
        if sat[c] or lab.all() or not lab.any():
            sat[c] = 1
            continue
        x = f[idx]
        c0, c1 = x[lab].sum(0) / np.float64(lab.sum()), x[~lab].sum(0) / np.float64((~lab).sum())
        centres[c, 0], centres[c, 1] = c0, c1
        cb, cn = np.zeros(len(idx)), np.zeros(len(idx))
        for d in range(D):
            cb = cb + 0.5 * (c0[d] * c0[d] - 2.0 * (c0[d] * x[:, d]))
            cn = cn + 0.5 * (c1[d] * c1[d] - 2.0 * (c1[d] * x[:, d]))
        term[idx] = cb - cn
    return centres, term, sat


def scale_of(largest):
    """2^(e - 30) with largest in [2^(e-1), 2^e); 1 when every capacity is 0"""
    if not largest > 0:
        return 1.0
    return float(np.ldexp(1.0, int(np.frexp(largest)[1]) - 30))


def quantize(term, edge_weight, active, lam, arc_edge):
    """-> (src_cap, snk_cap int32 [V], arc_cap int32 [2E], scale)"""
    term = np.asarray(term, dtype=np.float64)
    w = np.abs(np.float64(lam) * np.asarray(edge_weight, dtype=np.float32).astype(np.float64))
    if active is not None:
        w = np.where(np.asarray(active).astype(bool), 0.0, w)
    s = scale_of(max(np.abs(term).max(initial=0.0), w.max(initial=0.0)))
    src = np.where(term > 0, np.rint(term / s), 0).astype(np.int32)
    snk = np.where(term < 0, np.rint(-term / s), 0).astype(np.int32)
    return src, snk, np.rint(w / s).astype(np.int32)[arc_edge] if len(w) else np.zeros(0, np.int32), s


# ---- min cut ----------------------------------------------------------------------------------------------------------------

def min_cut(src_cap, snk_cap, arc, arc_cap):
    """-> (sink_side uint8 [V], cut value): node V is the source, V + 1 the sink; parallel arcs add, self loops drop"""
    V = len(src_cap)
    rows = np.concatenate([np.full(V, V), np.arange(V), arc["tail"]])
    cols = np.concatenate([np.arange(V), np.full(V, V + 1), arc["head"]])
    caps = np.concatenate([src_cap, snk_cap, arc_cap]).astype(np.int64)
    keep = (rows != cols) & (caps > 0)
    cap = coo_matrix((caps[keep], (rows[keep], cols[keep])), shape=(V + 2, V + 2)).tocsr()
    assert cap.data.max(initial=0) < 2 ** 31
    cap = csr_matrix((cap.data.astype(np.int32), cap.indices, cap.indptr), shape=cap.shape)
    res = maximum_flow(cap, V, V + 1)
    residual = (cap - res.flow).tocsr()
    residual.data = (residual.data > 0).astype(np.int32)
    residual.eliminate_zeros()
    reach = breadth_first_order(residual.T.tocsr(), V + 1, directed=True, return_predecessors=False)
    side = np.zeros(V + 2, dtype=np.uint8)
    side[reach] = 1
    assert side[V] == 0
    return side[:V], int(res.flow_value)


def cut_value(src_cap, snk_cap, arc, arc_cap, side):
    """the value of the cut that puts ``side == 1`` with the sink"""
    side = np.asarray(side).astype(bool)
    cross = (~side[arc["tail"]]) & side[arc["head"]]
    return int(np.asarray(src_cap, np.int64)[side].sum() + np.asarray(snk_cap, np.int64)[~side].sum()
               + np.asarray(arc_cap, np.int64)[cross].sum())


def random_network(V, degree, spread, offset, cap_below, seed):
    """``degree`` edges from every node to random nodes, an independent capacity below ``cap_below`` on each of the two
    arcs of an edge; src - snk uniform in [-spread, spread], plus ``offset`` on the first half of the nodes and minus
    ``offset`` on the second -> (src_cap, snk_cap int32 [V], source, target int32 [E], capacity by arc id int32 [2E])"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-spread, spread + 1, V) + np.where(np.arange(V) < V // 2, offset, -offset)
    source = np.repeat(np.arange(V), degree).astype(np.int32)
    target = rng.integers(0, V, V * degree).astype(np.int32)
    cap = rng.integers(0, cap_below, 2 * V * degree).astype(np.int32)
    return np.maximum(d, 0).astype(np.int32), np.maximum(-d, 0).astype(np.int32), source, target, cap


# ---- activation and components: CutPursuit.h activate_edges, compute_connected_components -------------------------------

def canonical(labels):
    """ids 0..C-1 in order of each class's smallest node"""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.reshape(-1)].astype(np.int32), len(first)


def activate(source, target, label, in_component, off, nodes, sat, active):
    """-> (in_component', sat', C', active', sat of the old components)"""
    source, target = np.asarray(source, dtype=np.int64), np.asarray(target, dtype=np.int64)
    sat, active = np.array(sat, dtype=np.uint8), np.array(active, dtype=np.uint8)
    V = len(label)
    for c in range(len(off) - 1):
        lab = label[nodes[off[c]:off[c + 1]]].astype(bool)
        if not sat[c] and (lab.all() or not lab.any()):
            sat[c] = 1
    active[label[source] != label[target]] = 1
    keep = active == 0
    graph = coo_matrix((np.ones(keep.sum()), (source[keep], target[keep])), shape=(V, V))
    comp, C = canonical(connected_components(graph, directed=False)[1])
    first = np.full(C, V, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(V))
    return comp, sat[np.asarray(in_component)[first]], C, active, sat


# ---- reduced graph and merge: CutPursuit.h compute_reduced_graph, merge; CutPursuit_L2.h compute_merge_gain -----------------

def values(features, off, nodes):
    f = np.asarray(features, dtype=np.float32).astype(np.float64)
    C = len(off) - 1
    weight = np.diff(off).astype(np.float64)
    mean = np.stack([f[nodes[off[c]:off[c + 1]]].sum(0) / weight[c] for c in range(C)])
    return mean, weight


def merge_gain(mean, weight, a, b):
    g = np.zeros(len(a))
    w1, w2 = weight[a], weight[b]
    for d in range(mean.shape[1]):
        v1, v2 = mean[a, d], mean[b, d]
        mv = (w1 * v1 + w2 * v2) / (w1 + w2)
        g = g + 0.5 * (mv * mv * (w1 + w2) - v1 * v1 * w1 - v2 * v2 * w2)
    return g


def reduce(features, source, target, edge_weight, in_component, off, nodes, lam):
    """-> dict mean, weight, a < b, border_weight, gain; borders ascend in (a, b)"""
    comp = np.asarray(in_component, dtype=np.int64)
    C = len(off) - 1
    mean, weight = values(features, off, nodes)
    ca, cb = comp[np.asarray(source, dtype=np.int64)], comp[np.asarray(target, dtype=np.int64)]
    cross = ca != cb
    keys = np.minimum(ca, cb)[cross] * C + np.maximum(ca, cb)[cross]
    ukeys, inverse = np.unique(keys, return_inverse=True)
    bw = np.zeros(len(ukeys))
    np.add.at(bw, inverse.reshape(-1), np.asarray(edge_weight, dtype=np.float32).astype(np.float64)[cross])
    a, b = (ukeys // C).astype(np.int64), (ukeys % C).astype(np.int64)
    gain = merge_gain(mean, weight, a, b) + bw * np.float64(lam) if len(a) else np.zeros(0)
    return {"mean": mean, "weight": weight, "a": a, "b": b, "border_weight": bw, "gain": gain}


def merge_sequential(a, b, gain, C):
    """the priority-queue walk of CutPursuit.h merge -> taken bool [B]"""
    gain = np.asarray(gain, dtype=np.float64)
    merged, taken = np.zeros(C, dtype=bool), np.zeros(len(gain), dtype=bool)
    for i in sorted(range(len(gain)), key=lambda i: (-gain[i], i)):
        if not gain[i] > 0:
            break
        if merged[a[i]] or merged[b[i]]:
            continue
        merged[a[i]] = merged[b[i]] = taken[i] = True
    return taken


def merge_rounds(a, b, gain, C):
    """rounds of locally dominant borders: a live border is taken when it is the best, by (gain descending, index
    ascending), among the live borders at both its ends -> (taken bool [B], rounds)"""
    gain = np.asarray(gain, dtype=np.float64)
    matched, taken, rounds = np.zeros(C, dtype=bool), np.zeros(len(gain), dtype=bool), 0
    while True:
        live = [i for i in range(len(gain)) if gain[i] > 0 and not matched[a[i]] and not matched[b[i]]]
        if not live:
            return taken, rounds
        best = {}
        for i in live:
            for c in (a[i], b[i]):
                if c not in best or (-gain[i], i) < (-gain[best[c]], best[c]):
                    best[c] = i
        for i in live:
            if best[a[i]] == i and best[b[i]] == i:
                taken[i] = matched[a[i]] = matched[b[i]] = True
        rounds += 1


def relabel(a, b, taken, in_component, sat, source, target, active):
    """-> (in_component', sat', C', active')"""
    comp, C = np.asarray(in_component, dtype=np.int64), len(sat)
    cmap, merged = np.arange(C), np.zeros(C, dtype=bool)
    cmap[np.asarray(b)[taken]] = np.asarray(a)[taken]
    merged[np.asarray(a)[taken]] = True
    keep = cmap == np.arange(C)
    newid = np.cumsum(keep) - 1
    active = np.array(active, dtype=np.uint8)
    cu, cv = comp[np.asarray(source, dtype=np.int64)], comp[np.asarray(target, dtype=np.int64)]
    active[(cu != cv) & (cmap[cu] == cmap[cv])] = 0
    sat_new = (np.asarray(sat).astype(bool) & ~merged)[keep].astype(np.uint8)
    return newid[cmap[comp]].astype(np.int32), sat_new, int(keep.sum()), active


# ---- energy: CutPursuit_L2.h compute_energy, from the ids alone ----------------------------------------------------------------

def energy(features, source, target, edge_weight, lam, in_component):
    """-> (fidelity, penalty) in float64: 1/2 sum_v |f_v - mean of its component|^2 and lam times the weight of the input
    edges between components"""
    f = np.asarray(features, dtype=np.float32).astype(np.float64)
    comp = np.asarray(in_component, dtype=np.int64)
    C = int(comp.max()) + 1
    count = np.bincount(comp, minlength=C).astype(np.float64)
    mean = np.stack([np.bincount(comp, weights=f[:, d], minlength=C) for d in range(f.shape[1])], 1) / count[:, None]
    fid = 0.5 * float(((f - mean[comp]) ** 2).sum())
    cross = comp[np.asarray(source, dtype=np.int64)] != comp[np.asarray(target, dtype=np.int64)]
    pen = float(lam) * float(np.asarray(edge_weight, dtype=np.float32).astype(np.float64)[cross].sum())
    return fid, pen


# ---- the solver: CutPursuit.h run ---------------------------------------------------------------------------------------------

def solve(features, source, target, edge_weight, lam, seed=0):
    """-> (in_component int32 [V], dict fidelity, penalty, components, saturated, stopped)"""
    features = np.asarray(features, dtype=np.float32)
    source, target = np.asarray(source).astype(np.int64), np.asarray(target).astype(np.int64)
    V, E = len(features), len(source)
    arc = arcs(source, target, V)
    comp, C = np.zeros(V, dtype=np.int32), 1
    sat, active = np.zeros(1, dtype=np.uint8), np.zeros(E, dtype=np.uint8)
    off, nodes = components_of(comp, C)
    old = energy(features, source, target, edge_weight, lam, comp)[0]
    info = {"fidelity": [], "penalty": [], "components": [], "saturated": [], "stopped": "iterations"}
    for it in range(1, MAX_ITE_MAIN + 1):
        label = kmeans(features, off, nodes, sat, seed, it)
        for _ in range(FLOW_STEPS):
            _, term, sat = capacities(features, off, nodes, label, sat)
            src, snk, cap, _ = quantize(term, edge_weight, active, lam, arc["edge"])
            label, _ = min_cut(src, snk, arc, cap)
        comp, sat, C, active, _ = activate(source, target, label, comp, off, nodes, sat, active)
        off, nodes = components_of(comp, C)
        red = reduce(features, source, target, edge_weight, comp, off, nodes, lam)
        taken = merge_sequential(red["a"], red["b"], red["gain"], C)
        comp, sat, C, active = relabel(red["a"], red["b"], taken, comp, sat, source, target, active)
        off, nodes = components_of(comp, C)
        fid, pen = energy(features, source, target, edge_weight, lam, comp)
        nsat = int(np.diff(off)[sat.astype(bool)].sum())
        for k, v in (("fidelity", fid), ("penalty", pen), ("components", C), ("saturated", nsat)):
            info[k].append(v)
        if nsat == V:
            info["stopped"] = "saturated"
            break
        if old > 0 and (old - fid - pen) / old < STOPPING_RATIO:
            info["stopped"] = "energy"
            break
        old = fid + pen
    return comp, info
