"""numpy oracle of the S3DIS partition front end (3d-wsis_amd/wsis_partition.py, csrc/partition.hip): the four array
stages of ``generate_SPG_superpoint`` (data/S3DIS/partition/partition_S3DIS.py:81-115 of the reference), each function
citing the lines it follows.

* ``prune`` keeps the reference's arithmetic operation for operation: fp32 bins, ids in order of first occurrence,
  sequential fp32 sums in point order, truncated colour means (ply_c/ply_c.cpp:293-392);
* ``knn`` is a ``cKDTree`` query with spare neighbours, re-sorted by (d2, id) with d2 = (dx*dx + dy*dy) + dz*dz
  recomputed in float64 and self excluded by id (graphs.py:34-38);
* ``geof`` evaluates ply_c.cpp:406-463 in float64 with ``eigh`` and rounds once;
* ``assemble`` is partition_S3DIS.py:105-108 and graphs.py:69-74 in numpy's own dtypes.

Tolerances.  The covariance is compared within one fp64 step (2^-52, relative to the trace) per
accumulated term: ``cov_tol(k)`` = (k + 1) 2^-52.  ``EV_TOL`` (relative to the trace) is 8 x the largest
``|eig - eigvalsh| / trace`` over the 46-point neighbourhoods of tests/golden/partition_golden.npz (floor 2^-50): the
disagreement of two correct fp64 solvers is the scale of a legitimate difference.  An eigenvalue is compared within
D = EV_TOL * trace, and ``feature_tolerances`` carries D through each expression:

* r_i = sqrt(lambda_i) moves by e_i = min(sqrt(D), D / r_i) (|sqrt a - sqrt b| <= sqrt|a - b| and <= |a - b| / sqrt a);
* linearity 1 - r1 / r0, planarity (r1 - r2) / r0, scattering r2 / r0: first order in e_i / r0, doubled for the
  higher orders (e_0 << r_0 always: lambda_0 >= trace / 3);
* an eigenvector turns by at most 2 D / gap_j, gap_j its eigenvalue's distance to the nearest other one, so a component
  of u = sum_j lambda_j |v_j| moves by sum_j (D + 2 lambda_j D / gap_j), and verticality u_z / |u| by 2 sqrt(3) times
  that over |u| >= lambda_0.  With g = the smallest gap over the trace this is at most 2 sqrt(3) EV_TOL (9 + 6 / g),
  which is below one fp32 step of 1 (2^-24) for g >= ``GAP_MIN``: verticality is compared where g > GAP_MIN only.
"""
import numpy as np
from scipy.spatial import cKDTree

EV_MEASURED = 1.2663804692531014e-15      # largest |LA.eig - eigvalsh| / trace over the fixture (test_partition_ref_host.py)
EV_TOL = max(8 * EV_MEASURED, 2.0 ** -50)
K_GEOF = 45
EPS32 = 2.0 ** -24


def cov_tol(k):
    """relative to the trace: one fp64 step per accumulated term, k + 1 of them"""
    return (k + 1) * 2.0 ** -52


def gap_min():
    """the smallest relative eigen-gap at which the verticality bound stays below one fp32 step at 1"""
    return 6.0 / (EPS32 / (2 * np.sqrt(3.0) * EV_TOL) - 9.0)


GAP_MIN = gap_min()


def step32(v):
    """one float32 step at |v|"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- prune: ply_c/ply_c.cpp:293-392 ----------------------------------------------------------------------------------

def bins(xyz, voxel):
    """:311-337: floor((x - x_min) / voxel) per axis in float32, not clamped -> (int64 [N,3], float32 [3])"""
    xyz = np.asarray(xyz, dtype=np.float32)
    mn = xyz.min(0)
    b = np.floor((xyz - mn) / np.float32(voxel))
    assert b.dtype == np.float32
    return b.astype(np.int64), mn


def prune(xyz, voxel, rgb, labels=None, n_labels=0):
    """-> dict: xyz fp32 [V,3], rgb uint8 [V,3], label_hist uint32 [V, n_labels + 1] (None without labels), p2v uint32
    [N], count uint32 [V].  Voxel ids are the insertion index of the reference's std::map (:175-189): first occurrence.
    The sums of :262-268 are sequential in point order: round j adds the j-th point of every voxel, in float32."""
    xyz, rgb = np.asarray(xyz, dtype=np.float32), np.asarray(rgb, dtype=np.uint8)
    b, _ = bins(xyz, voxel)
    _, first, inverse = np.unique(b, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")              # unique row -> rank of its first occurrence
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    p2v = rank[inverse]
    V = len(first)
    count = np.bincount(p2v, minlength=V)
    by_voxel = np.argsort(p2v, kind="stable")
    start = np.concatenate([[0], np.cumsum(count)])
    acc = np.zeros((V, 3), dtype=np.float32)
    col = np.zeros((V, 3), dtype=np.uint32)
    for j in range(int(count.max())):
        rows = np.nonzero(count > j)[0]
        pts = by_voxel[start[rows] + j]
        acc[rows] = acc[rows] + xyz[pts]                  # float32 + float32
        col[rows] += rgb[pts]
    n = count.astype(np.float32)[:, None]
    out = {"xyz": acc / n, "rgb": (col.astype(np.float32) / n).astype(np.uint8), "p2v": p2v.astype(np.uint32),
           "count": count.astype(np.uint32), "label_hist": None}
    assert out["xyz"].dtype == np.float32
    if labels is not None:
        labels = np.asarray(labels).astype(np.int64)
        if labels.min() < 0 or labels.max() > n_labels:
            raise IndexError("label outside the histogram (the reference's .at() throws)")
        hist = np.zeros((V, n_labels + 1), dtype=np.uint32)
        np.add.at(hist, (p2v, labels), 1)
        out["label_hist"] = hist
    return out


# ---- k nearest neighbours: graphs.py:34-38 ---------------------------------------------------------------------------

def dist2(xyz, a, b):
    """(dx*dx + dy*dy) + dz*dz on the coordinates widened to float64; a, b index arrays that broadcast"""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    d = x[b] - x[a]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn(xyz, k, spare=8):
    """-> (nbr int32 [V,k], dist2 float64 [V,k]): every row ascending in (d2, id), self excluded by id.  The tree returns
    k + 1 + spare candidates; a row is settled when its k-th pair is strictly below the last candidate's d2 (everything
    the tree left out is at least that far), otherwise the query is repeated with more spare."""
    xyz = np.asarray(xyz, dtype=np.float32)
    V = len(xyz)
    if V < k + 1:
        raise ValueError("Expected n_neighbors <= n_samples")          # sklearn raises there too
    tree = cKDTree(xyz.astype(np.float64))
    nbr = np.empty((V, k), dtype=np.int32)
    d2o = np.empty((V, k), dtype=np.float64)
    todo = np.arange(V)
    while len(todo):
        m = min(V, k + 1 + spare)
        _, cand = tree.query(xyz[todo].astype(np.float64), k=m)
        cand = cand.reshape(len(todo), m)
        d2 = dist2(xyz, todo[:, None], cand)
        d2 = np.where(cand == todo[:, None], np.inf, d2)              # self leaves by id
        o = np.lexsort((cand, d2))                                    # along the last axis: by d2, then by id
        cand, d2 = np.take_along_axis(cand, o, 1), np.take_along_axis(d2, o, 1)
        # candidates other than self: m - 1 (self is always among the m nearest unless > m points coincide with it)
        last = np.where(np.isinf(d2[:, -1]), d2[:, -2], d2[:, -1])
        done = (m == V) | (d2[:, k - 1] < last * (1 - 1e-12))          # the tree's own d2 is rounded differently
        rows = todo[done]
        nbr[rows], d2o[rows] = cand[done, :k], d2[done, :k]
        todo, spare = todo[~done], 4 * spare + 64
    return nbr, d2o


# ---- geometric features: ply_c/ply_c.cpp:406-463 in float64 ------------------------------------------------------------

def cov_of(xyz, nbr):
    """:406-428 -> float64 [V,3,3]: self first, then the neighbours; central second moments over k + 1"""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    nbr = np.asarray(nbr).astype(np.int64)
    pos = np.concatenate([x[:, None, :], x[nbr]], 1)
    c = pos - pos.mean(1, keepdims=True)
    return np.einsum("vni,vnj->vij", c, c) / pos.shape[1]


def geof(xyz, nbr):
    """-> dict: geof fp32 [V,4] (linearity, planarity, scattering, verticality), cov float64 [V,6] = (xx, yy, zz, xy, xz,
    yz), ev float64 [V,3] descending and clamped at 0 (:433-437), gap float64 [V] = the smallest distance between two
    eigenvalues over the trace"""
    c = cov_of(xyz, nbr)
    w, vec = np.linalg.eigh(c)                               # ascending
    w, vec = w[:, ::-1], vec[:, :, ::-1]
    lam = np.maximum(w, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(lam)
        lin = (r[:, 0] - r[:, 1]) / r[:, 0]
        plan = (r[:, 1] - r[:, 2]) / r[:, 0]
        scat = r[:, 2] / r[:, 0]
        u = (lam[:, None, 0] * np.abs(vec[:, :, 0]) + lam[:, None, 1] * np.abs(vec[:, :, 1])) + lam[:, None, 2] * np.abs(vec[:, :, 2])
        norm = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        vert = u[:, 2] / norm
        trace = c[:, 0, 0] + c[:, 1, 1] + c[:, 2, 2]
        gap = np.minimum(lam[:, 0] - lam[:, 1], lam[:, 1] - lam[:, 2]) / trace
    cov6 = np.stack([c[:, 0, 0], c[:, 1, 1], c[:, 2, 2], c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]], 1)
    return {"geof": np.stack([lin, plan, scat, vert], 1).astype(np.float32), "geof64": np.stack([lin, plan, scat, vert], 1),
            "cov": cov6, "ev": lam, "gap": gap, "trace": trace}


def feature_tolerances(ev, trace, gap):
    """|device - oracle| bounds BEFORE the final float32 step -> float64 [V,4] (module docstring)"""
    D = EV_TOL * trace
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(ev)
        e = np.minimum(np.sqrt(D)[:, None], D[:, None] / r)
        e = np.where(np.isnan(e), np.sqrt(D)[:, None], e)
        r0 = r[:, 0]
        lin = 2 * (e[:, 1] + e[:, 0] * r[:, 1] / r0) / r0
        plan = 2 * (e[:, 1] + e[:, 2] + e[:, 0] * (r[:, 1] - r[:, 2]) / r0) / r0
        scat = 2 * (e[:, 2] + e[:, 0] * r[:, 2] / r0) / r0
        vert = 2 * np.sqrt(3.0) * EV_TOL * (9 + 6 / gap)
    return np.stack([lin, plan, scat, vert], 1)


# ---- assembly: partition_S3DIS.py:105-108, graphs.py:69-74 -----------------------------------------------------------

def assemble(geof32, rgb, nbr, d2, k_adj, lambda_edge_weight=1., mean=None):
    """-> dict of the arguments of libcp.cutpursuit in the reference's dtypes.  ``mean``: a float32 to use instead of
    numpy's own ``np.mean`` of the float32 distances (to evaluate the expressions with the device's mean)."""
    V = len(geof32)
    features = np.hstack((np.asarray(geof32, dtype=np.float32), np.asarray(rgb, dtype=np.uint8) / 255.)).astype('float32')
    features[:, 3] = 2. * features[:, 3]
    source = np.repeat(np.arange(V), k_adj).astype('uint32')
    target = np.asarray(nbr)[:, :k_adj].flatten().astype('uint32')
    distances = np.sqrt(np.asarray(d2, dtype=np.float64)[:, :k_adj]).flatten().astype('float32')
    m = np.mean(distances) if mean is None else np.float32(mean)
    assert np.asarray(m).dtype == np.float32
    edge_weight = np.array(1. / (lambda_edge_weight + distances / m), dtype='float32')
    return {"features": features, "source": source, "target": target, "distances": distances, "edge_weight": edge_weight,
            "mean": np.float32(m)}


def edge_weight_of(distances, mean, lambda_edge_weight=1.):
    """partition_S3DIS.py:108 on float32 distances with a given float32 mean, in numpy's float32 arithmetic"""
    return np.array(1. / (lambda_edge_weight + np.asarray(distances, dtype=np.float32) / np.float32(mean)), dtype='float32')


def edge_weight_margin(distances, mean_a, mean_b, lambda_edge_weight=1.):
    """what a difference between two means propagates into 1 / (lambda + d / mean), plus one float32 step of the value.
    The expression is a float32 one, so what a mean propagates is what the float32 expression gives for the two means
    (a one-step change of the mean can move the rounded sum lambda + d / mean by a step of its own, which near w = 1 is
    two steps of w: the derivative w^2 d / mean^2 alone does not see it); with equal means the margin is one step."""
    wa = edge_weight_of(distances, mean_a, lambda_edge_weight).astype(np.float64)
    wb = edge_weight_of(distances, mean_b, lambda_edge_weight).astype(np.float64)
    return np.abs(wa - wb) + step32(np.maximum(wa, wb))


# ---- synthetic rooms ---------------------------------------------------------------------------------------------------

def make_room(seed, n=40000, offset=(12.0, -7.0, 3.0), size=(4.0, 3.0, 2.5)):
    """floor, one wall, a thin column and a cluttered volume, offset some metres from the origin -> (xyz fp32 [n,3], rgb
    uint8 [n,3])"""
    rng = np.random.default_rng(seed)
    sx, sy, sz = size
    parts = []
    m = n // 4
    parts.append(np.stack([rng.uniform(0, sx, m), rng.uniform(0, sy, m), rng.normal(0, 0.004, m)], 1))           # floor
    parts.append(np.stack([rng.normal(0, 0.004, m), rng.uniform(0, sy, m), rng.uniform(0, sz, m)], 1))           # wall
    c = m // 4
    parts.append(np.stack([0.7 * sx + rng.normal(0, 0.02, c), 0.6 * sy + rng.normal(0, 0.02, c), rng.uniform(0, sz, c)], 1))
    rest = n - 2 * m - c
    parts.append(np.stack([rng.uniform(0.3 * sx, 0.6 * sx, rest), rng.uniform(0.2 * sy, 0.7 * sy, rest),
                           rng.uniform(0.1, 0.9, rest)], 1))                                                    # clutter
    xyz = (np.concatenate(parts) + np.asarray(offset)).astype(np.float32)
    perm = rng.permutation(len(xyz))
    rgb = rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    return xyz[perm], rgb[perm]
