"""numpy oracle of the superpoint-graph preparation (3d-wsis_amd/wsis_graph_prep.py, csrc/graphprep.hip), in the
reference's own shape: one ``np.where(superpoint == spID)`` mask per superpoint, one Python loop per edge
(data/ScanNetV2/prepare_data_inst_ScanNetV2.py:172-285, :340-433 and data/S3DIS/prepare_S3DIS_inst_data.py:101-224,
:268-358).

Two evaluations:

* ``wide=False`` follows the reference's dtypes operation for operation (float32 means and standard deviations of
  float32 arrays, float64 ``np.cov``): against tests/golden/graph_prep_golden.npz everything is bit-equal except the
  eigenvalue features, where the reference's ``LA.eig`` and this file's ``eigvalsh`` are two different fp64 solvers;
* ``wide=True`` takes every sum in float64 and rounds once: the value the kernels are compared with.

Neighbour lists are brute force in float64, ``d2 = (dx*dx + dy*dy) + dz*dz``, ordered by (d2, id), self excluded by id.

Tolerances.  ``gap_c`` bounds the error of a sequential float32 mean of n <= n_max values of magnitude <= max|coord|
(numpy's axis-0 mean of a float32 array): (n_max + 2) * 2^-24 * max|coord|.  ``EV_TOL`` (relative to the trace) is 8 x
the largest ``|eig - eigvalsh| / trace`` seen over every fixture and edge-case matrix (floor 2^-50): two correct fp64
solvers' disagreement is the scale of a legitimate difference (DESIGN.md 4.14 quotes the measured figure).
"""
import itertools

import numpy as np

NONE = -100
EV_MEASURED = 1.4316065011004693e-15      # largest |LA.eig - eigvalsh| / trace, see tests/test_graph_prep_host.py::test_ev_tol
EV_TOL = max(8 * EV_MEASURED, 2.0 ** -50)
EPS32 = 2.0 ** -24
SQRT3 = float(np.sqrt(3.0))
FEATURE_NAMES = ("delta_mean", "delta_std", "delta_centroid", "length_ratio", "surface_ratio", "volume_ratio",
                 "count_ratio")


def gap_c(xyz, n_max):
    return (n_max + 2) * EPS32 * float(np.abs(xyz).max())


def step32(v):
    """one float32 step at |v|"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def rows_of(superpoint):
    S = int(superpoint.max()) + 1
    return [np.where(superpoint == s)[0] for s in range(S)]


# ---- superpoint features ---------------------------------------------------------------------------------------------

def cov6(m):
    return np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])


def superpoint_features(xyz, superpoint, wide=False, eig=None):
    """-> dict: centroid fp32 [S,3], length / surface / volume fp32 [S], count uint64 [S], cov fp64 [S,6], ev fp64 [S,3]
    (zeros for n < 3).  ``eig``: the solver, eigenvalues of a symmetric 3x3 (default ``np.linalg.eigvalsh``)."""
    eig = np.linalg.eigvalsh if eig is None else eig
    rows = rows_of(superpoint)
    S = len(rows)
    out = {"centroid": np.zeros((S, 3), np.float32), "length": np.zeros(S, np.float32), "surface": np.zeros(S, np.float32),
           "volume": np.zeros(S, np.float32), "count": np.zeros(S, np.uint64), "cov": np.zeros((S, 6)), "ev": np.zeros((S, 3))}
    for s, mask in enumerate(rows):
        p = xyz[mask]
        n = len(p)
        out["count"][s] = n
        mean = p.astype(np.float64).mean(0) if wide else np.mean(p, axis=0)
        out["centroid"][s] = p[0] if n == 1 else mean
        if n == 2:
            var = np.var(p.astype(np.float64), axis=0) if wide else np.var(p, axis=0)
            out["length"][s] = np.sqrt(np.sum(var))
            out["cov"][s, :3] = var
            d = p.astype(np.float64) - p.astype(np.float64).mean(0)
            out["cov"][s, 3:] = [(d[:, 0] * d[:, 1]).mean(), (d[:, 0] * d[:, 2]).mean(), (d[:, 1] * d[:, 2]).mean()]
        elif n >= 3:
            c = np.cov(np.transpose(p), rowvar=True)
            ev = -np.sort(-np.asarray(eig(c)))
            out["cov"][s], out["ev"][s] = cov6(c), ev
            out["length"][s] = ev[0]
            out["surface"][s] = np.sqrt(ev[0] * ev[1] + 1e-10)
            out["volume"][s] = np.sqrt(ev[0] * ev[1] * ev[2] + 1e-10)
    return out


def features_array(ft):
    """the reference's float64 [S,7] ``superpoints_features``"""
    return np.concatenate([ft["centroid"], ft["length"][:, None], ft["surface"][:, None], ft["volume"][:, None],
                           ft["count"][:, None]], axis=1)


# ---- labels ----------------------------------------------------------------------------------------------------------

def label_mode(labels, superpoint):
    """stats.mode per superpoint: the most frequent value, the smallest on a tie -> float64 [S]"""
    out = []
    for mask in rows_of(superpoint):
        v, c = np.unique(labels[mask], return_counts=True)
        out.append(v[np.argmax(c)])
    return np.asarray(out, dtype=np.float64)


def superpoint_labels(xyz, superpoint, semantic_labels, instance_labels, wide=False):
    rows = rows_of(superpoint)
    S = len(rows)
    if semantic_labels is None and instance_labels is None:
        return np.full(S, -100.0), np.full(S, -100.0), np.zeros((S, 3))
    sem, ins = label_mode(semantic_labels, superpoint), label_mode(instance_labels, superpoint)
    acc = (lambda a: a.astype(np.float64).mean(0).astype(np.float32)) if wide else (lambda a: np.mean(a, axis=0))
    centre = {i: acc(xyz[instance_labels == i]) for i in np.unique(instance_labels)}
    off = np.zeros((S, 3))
    for s, mask in enumerate(rows):
        off[s] = centre[ins[s]] - acc(xyz[mask])
    return sem, ins, off


# ---- neighbours ------------------------------------------------------------------------------------------------------

def distances2(centres):
    c = np.asarray(centres).astype(np.float64)
    d = c[:, None, :] - c[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbor_lists(centres, k, radius=np.inf):
    """-> nbr int32 [S,k] (-1 padded), dist2 fp64 [S,k] (inf padded), count int32 [S]"""
    d2 = distances2(centres)
    S = len(d2)
    nbr, dist2 = np.full((S, k), -1, np.int32), np.full((S, k), np.inf)
    count = np.zeros(S, np.int32)
    r2 = float(radius) * float(radius)
    for s in range(S):
        ids = np.array([i for i in range(S) if i != s and d2[s, i] <= r2], dtype=np.int64)
        ids = ids[np.lexsort((ids, d2[s, ids]))] if len(ids) else ids
        count[s] = len(ids)
        m = min(k, len(ids))
        nbr[s, :m], dist2[s, :m] = ids[:m], d2[s, ids[:m]]
    return nbr, dist2, count


def _sorted_distances(centres):
    """[S, S-1]: every row's distances to the OTHER centres, ascending"""
    d = np.sqrt(distances2(centres))
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, :-1]


def knn_margin(centres, k):
    """the smallest of: every centre distance, and the cut d_(k+1) - d_k after the k-th neighbour of every row"""
    if len(centres) < 2:
        return np.inf
    o = _sorted_distances(centres)
    worst = float(o[:, 0].min())
    if o.shape[1] > k:
        worst = min(worst, float((o[:, k] - o[:, k - 1]).min()))
    return worst


def radius_margin(centres, radius):
    """-> (smallest |d - radius|, smallest difference of consecutive candidate distances inside the radius, the point
    itself at distance 0 included)"""
    if len(centres) < 2:
        return np.inf, np.inf
    o = _sorted_distances(centres)
    edge = float(np.abs(o - radius).min())
    step = np.diff(np.concatenate([np.zeros((len(o), 1)), o], axis=1), axis=1)[o <= radius]
    return edge, (float(step.min()) if step.size else np.inf)


def neighbours_clear(centres, k=None, radius=None, gap=0.0):
    """the condition of the fixtures: no neighbour decision within rounding of its threshold"""
    if k is not None and not knn_margin(centres, k) > 4 * SQRT3 * gap:
        return False
    if radius is not None:
        edge, step = radius_margin(centres, radius)
        if not (edge > 2 * SQRT3 * gap and step > 4 * SQRT3 * gap):
            return False
    return True


def cap_rule(centres, start_edges, radius, cap):
    """ScanNet :217-225 by brute force: the full candidate list of every s (ascending (d2, id), self excluded)"""
    S = len(centres)
    nbr, _, _ = neighbor_lists(centres, max(S - 1, 1), radius)
    edges = set(map(tuple, np.asarray(start_edges, dtype=np.int64).reshape(-1, 2).tolist()))
    for s in range(S):
        cnt = 0
        for t in nbr[s]:
            if t < 0 or cnt >= cap:
                break
            if (s, int(t)) not in edges:
                edges.add((s, int(t)))
                edges.add((int(t), s))
                cnt += 1
    return edges


def face_edges(faces, superpoint):
    edges = set()
    for face in np.asarray(faces).reshape(-1, 3):
        ids = np.unique(superpoint[face])
        for a, b in itertools.combinations(ids.tolist(), 2):
            edges.add((a, b))
            edges.add((b, a))
    return edges


# ---- edge features ---------------------------------------------------------------------------------------------------

def draw_samples(counts, edges, rng):
    off, idx = [0], []
    for s, t in edges:
        ns, nt = int(counts[s]), int(counts[t])
        if ns != nt:
            idx.extend(rng.choice(max(ns, nt), min(ns, nt), replace=False).tolist())
        off.append(len(idx))
    return np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int32)


def edge_features(xyz, superpoint, ft, edges, samples, wide=False):
    """-> fp32 [E,13]; ``samples`` = (offsets [E+1], indices) as ``draw_samples`` returns them"""
    rows = rows_of(superpoint)
    off, idx = samples
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    E = len(edges)
    f = np.zeros((E, 13), np.float32)
    for e, (s, t) in enumerate(edges):
        ps, pt = xyz[rows[s]], xyz[rows[t]]
        pick = idx[off[e]:off[e + 1]]
        if len(ps) > len(pt):
            ps = ps[pick]
        elif len(ps) < len(pt):
            pt = pt[pick]
        delta = ps - pt
        if len(delta) > 1:
            d = delta.astype(np.float64) if wide else delta
            f[e, 0:3], f[e, 3:6] = np.mean(d, axis=0), np.std(d, axis=0)
        else:
            f[e, 0:3] = delta
    es, et = edges[:, 0], edges[:, 1]
    f[:, 6:9] = ft["centroid"][es] - ft["centroid"][et]
    for j, name in enumerate(("length", "surface", "volume")):
        f[:, 9 + j] = ft[name][es] / (ft[name][et] + 1e-6)              # float32 throughout, as on (S,1) float32 arrays
    f[:, 12] = ft["count"][es] / (ft["count"][et] + 1e-6)                # uint64 / float64 -> float64, rounded on store
    return f


def standardize(f):
    """StandardScaler().fit(f) then transform(f, copy=False) on fp32 [E,13], with sklearn's own operations -> (fp32 [E,13],
    mean fp64 [13], scale fp64 [13])"""
    n = f.shape[0]
    total = np.sum(f, axis=0, dtype=np.float64)
    mean = total / n
    temp = f - mean
    corr = np.sum(temp, axis=0)
    temp **= 2
    var = (np.sum(temp, axis=0) - corr ** 2 / n) / n
    scale = np.sqrt(var)
    scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
    out = f.copy()
    out -= mean
    out /= scale
    return out, mean, scale


# ---- the two builders ------------------------------------------------------------------------------------------------

def _centres(xyz, superpoint):
    c = np.zeros((int(superpoint.max()) + 1, 3), dtype=np.float32)
    for s, mask in enumerate(rows_of(superpoint)):
        c[s] = xyz[mask].mean(0)
    return c


def _finish(xyz, superpoint, labels, edges, rng, samples, wide):
    ft = superpoint_features(xyz, superpoint, wide)
    if samples is None:
        samples = draw_samples(ft["count"], edges, rng)
    f = edge_features(xyz, superpoint, ft, edges, samples, wide)
    return {"v": np.arange(len(ft["count"])), "semantic_label": labels[0], "instance_label": labels[1],
            "superpoint_feature": features_array(ft), "superpoint_offset_vector": labels[2],
            "edges": np.asarray(edges, dtype=np.int64).reshape(-1, 2), "f": f, "samples": samples, "features": ft}


def build_graph_s3dis(xyz, superpoint, semantic_labels, instance_labels, rng=None, k=10, samples=None, wide=False):
    centres = _centres(xyz, superpoint)
    nbr, _, _ = neighbor_lists(centres, k)
    edges = set()
    for s in range(len(nbr)):
        for t in nbr[s]:
            if t >= 0:
                edges.add((s, int(t)))
                edges.add((int(t), s))
    edges = sorted(edges)
    labels = superpoint_labels(xyz, superpoint, semantic_labels, instance_labels, wide)
    g = _finish(xyz, superpoint, labels, edges, rng, samples, wide)
    sem, ins = labels[0], labels[1]
    g["is1ins"] = np.asarray([(sem[s] == sem[t]) if (ins[s] == NONE and ins[t] == NONE) else (ins[s] == ins[t])
                              for s, t in edges], dtype=np.int64)
    g["centres"] = centres
    return g


def build_graph_scannet(xyz, faces, superpoint, semantic_labels=None, instance_labels=None, rng=None, radius=0.3, cap=5,
                        samples=None, wide=False, standardized=True):
    centres = _centres(xyz, superpoint)
    edges = sorted(cap_rule(centres, sorted(face_edges(faces, superpoint)), radius, cap))
    labels = superpoint_labels(xyz, superpoint, semantic_labels, instance_labels, wide)
    g = _finish(xyz, superpoint, labels, edges, rng, samples, wide)
    g["f_raw"] = g["f"]
    if standardized:
        g["f"], g["f_mean"], g["f_scale"] = standardize(g["f_raw"])
    ins = labels[1]
    g["is1ins"] = np.asarray([0 if (ins[s] == NONE or ins[t] == NONE) else (-1 if ins[s] == ins[t] else 1)
                              for s, t in edges], dtype=np.int64)
    g["centres"] = centres
    return g


# ---- tolerances: the reference's float32 sums (gap_c) and the solver (EV_TOL) through each expression ----------------

def feature_tolerances(ft, gap):
    """|device - reference| bounds per superpoint feature, BEFORE the final float32 step: dict of [S] arrays.
    centroid: gap.  n == 2: the reference takes sqrt(sum(var)) in float32 about a float32 mean: each deviation is off by
    at most 2 * 2^-24 * max|coord| <= gap, so the length by sqrt(3) * gap, plus 8 float32 roundings of the value.
    n >= 3: an eigenvalue moves by at most EV_TOL * trace =: D; d sqrt(u) = du / (2 sqrt(u))."""
    ev, n = ft["ev"], ft["count"].astype(np.int64)
    D = EV_TOL * (ft["cov"][:, 0] + ft["cov"][:, 1] + ft["cov"][:, 2])
    a = np.abs(ev)
    sur = np.sqrt(np.maximum(ev[:, 0] * ev[:, 1] + 1e-10, 1e-300))
    vol = np.sqrt(np.maximum(ev[:, 0] * ev[:, 1] * ev[:, 2] + 1e-10, 1e-300))
    length = np.where(n == 2, SQRT3 * gap + 8 * EPS32 * ft["length"].astype(np.float64), np.where(n >= 3, D, 0.0))
    surface = np.where(n >= 3, D * (a[:, 0] + a[:, 1] + D) / (2 * sur), 0.0)
    volume = np.where(n >= 3, D * (a[:, 0] * a[:, 1] + a[:, 0] * a[:, 2] + a[:, 1] * a[:, 2] + D * a.sum(1) + D * D) / (2 * vol), 0.0)
    return {"centroid": np.full(len(n), gap), "length": length, "surface": surface, "volume": volume}


def edge_tolerances(ft, edges, f, gap):
    """|device - reference| bounds for the raw [E,13] features, the final float32 step included.
    delta_mean: a sequential float32 mean of m <= n_max deltas of magnitude <= 2 max|coord|: 2 gap.
    delta_std: about a mean off by eps <= 2 gap the variance grows by eps^2, so the deviation by at most eps; the float32
      accumulation of the squares adds (m + 4) * 2^-24 * std / 2 <= gap: 3 gap, rounded up to 4 gap for the float32
      deviations themselves.
    delta_centroid: 2 gap.
    ratio a_s / (a_t + 1e-6): (tol_s + ratio * tol_t) / (a_t + 1e-6), each tol with the float32 step of the stored
      feature; the float32 addition and division add 2 steps of the result.  count ratio: exact."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    es, et = edges[:, 0], edges[:, 1]
    tol = np.zeros(f.shape)
    tol[:, 0:3] = 2 * gap
    tol[:, 3:6] = 4 * gap
    tol[:, 6:9] = 2 * gap
    ftol = feature_tolerances(ft, gap)
    for j, name in enumerate(("length", "surface", "volume")):
        a = ft[name].astype(np.float64)
        t = ftol[name] + step32(a)
        ratio = np.abs(f[:, 9 + j].astype(np.float64))
        tol[:, 9 + j] = (t[es] + ratio * t[et]) / (a[et] + 1e-6) + 2 * step32(ratio)
    return tol + step32(f)
