"""Inputs and references of tests/test_gpu_point_ops_edges.py (the pointgroup_ops drop-in: voxelization in csrc/core.hip,
the device voxelization_idx in csrc/voxelize_idx.hip, ballquery_batch_p and the device bfs_cluster in csrc/cluster.hip),
made here so that tests/test_point_ops_cases_host.py can check on any machine that every one of them still has the
property it is named after.  Every builder asserts its own precondition; references are numpy / scipy at fp64 or integer,
or oracle/pg_ops.py.

Ball-query scenes live on the lattice of multiples of 2^-10 with |x| < 2^13, and the radius is a lattice length too: the
coordinates, their differences, r^2 and every squared distance are exact in fp32 (and the build has no fused
multiply-add), so `d2 < r2` has one right answer, ties (d2 == r2) included -- a great many of them by construction.

Not reached: the third arm of row_col (csrc/common.h), the 64-bit division for M * C >= 2^32 with C not a power of two.
It needs an output of about 17 GB and stays untested."""
import functools
from collections import namedtuple

import numpy as np

from oracle import pg_ops

GRID_THREADS = 2048 * 256            # csrc/common.h grid_for: a launch has at most this many threads
BQ_CAP = 1000                        # csrc/cluster.hip: neighbours kept per point
CELL_BITS = 18                       # csrc/cluster.hip: bits per cell coordinate in the cell key (bias 2^17)
CELL_BIAS = 1 << (CELL_BITS - 1)
UNIT = 2.0 ** -10                    # the lattice
R_UNITS = 15                         # 15^2 = 225 = 9^2 + 12^2 = 10^2 + 10^2 + 5^2 = 11^2 + 10^2 + 2^2 = 14^2 + 5^2 + 2^2: many ties
FAR_R_UNITS = 32                     # r = 2^-5; 32^2 = 4^5 is a sum of three squares only as (32, 0, 0): ties along the axes
INT32_MIN = -2 ** 31

Scene = namedtuple("Scene", "name xyz batch_idx batch_off radius")


# ===================================================================================================== ball query
def _scene(name, units, sizes, r_units):
    """a Scene from integer lattice coordinates [N, 3] and the batch item sizes"""
    units = np.asarray(units, dtype=np.int64).reshape(-1, 3)
    assert sum(sizes) == units.shape[0]
    assert units.size == 0 or np.abs(units).max() < 2 ** 23, "|x| < 2^13 on the 2^-10 lattice"
    x64 = units.astype(np.float64) * UNIT
    x32 = x64.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x64), "the fp32 coordinates are the fp64 ones"
    r = float(r_units) * UNIT
    assert float(np.float32(r)) == r and float(np.float32(r) * np.float32(r)) == r * r
    bi = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return Scene(name, np.ascontiguousarray(x32), bi, off, r)


def units_of(scene):
    return np.rint(scene.xyz.astype(np.float64) / UNIT).astype(np.int64)


def _block(n, side, seed, step=1):
    """n distinct cells of a side^3 block, every ``step`` lattice units, in random order"""
    rng = np.random.default_rng(seed)
    lin = rng.choice(side ** 3, n, replace=False)
    return np.stack(np.unravel_index(lin, (side,) * 3), 1).astype(np.int64) * step


def cells_fp32(scene):
    """the cell of every point by the kernel's own fp32 expression: floor(fl(x * fl(1 / fl(r * 1.001))))"""
    inv = np.float32(1.0) / (np.float32(scene.radius) * np.float32(1.001))
    prod = scene.xyz * inv
    assert prod.dtype == np.float32
    return np.floor(prod).astype(np.int64)


def hits_int(scene):
    """bool [N, N] on small scenes, by integer arithmetic on the lattice: same batch item and d^2 < r^2; and the ties"""
    K = units_of(scene)
    r2 = int(round(scene.radius / UNIT)) ** 2
    same = scene.batch_idx[:, None] == scene.batch_idx[None, :]
    d2 = np.zeros((len(K), len(K)), dtype=np.int64)
    for a in range(3):
        d = K[:, a][:, None] - K[:, a][None, :]
        d2 += d * d
    return same & (d2 < r2), same & (d2 == r2)


def tie_pairs(scene):
    """ordered pairs at a distance of exactly r: the strict `<` leaves every one of them out"""
    return int(hits_int(scene)[1].sum())


def true_counts(scene):
    """uncapped neighbour count of every point (itself included when r > 0)"""
    return hits_int(scene)[0].sum(1)


def kd_reference(scene, lists_of=None, cap=BQ_CAP):
    """cKDTree at fp64 per batch item with the closed radius nextafter(r, 0): on the lattice no distance lies between it
    and r, so it is the strict ball.  -> (counts int64 [N], {p: ascending global indices, first ``cap``} for the points
    ``lists_of`` (default: all))"""
    from scipy.spatial import cKDTree
    assert scene.radius > 0
    rr = np.nextafter(np.float64(scene.radius), 0.0)
    N = len(scene.xyz)
    counts = np.zeros(N, dtype=np.int64)
    lists = {}
    want = np.arange(N) if lists_of is None else np.asarray(lists_of)
    x64 = scene.xyz.astype(np.float64)
    for b in range(len(scene.batch_off) - 1):
        lo, hi = int(scene.batch_off[b]), int(scene.batch_off[b + 1])
        if lo == hi:
            continue
        tree = cKDTree(x64[lo:hi])
        counts[lo:hi] = tree.query_ball_point(x64[lo:hi], rr, return_length=True)
        mine = want[(want >= lo) & (want < hi)]
        for p, nb in zip(mine.tolist(), tree.query_ball_point(x64[mine], rr)):
            lists[p] = (np.sort(np.asarray(nb, dtype=np.int64)) + lo)[:cap]
    return counts, lists


def kd_flat(scene):
    """(idx, start_len) in the layout of the operator from kd_reference"""
    counts, lists = kd_reference(scene)
    N = len(scene.xyz)
    n = np.minimum(counts, BQ_CAP)
    start = np.concatenate([[0], np.cumsum(n)[:-1]]) if N else np.zeros(0, np.int64)
    idx = np.concatenate([lists[p] for p in range(N)]) if N else np.zeros(0, np.int64)
    return idx.astype(np.int32), np.stack([start, n], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_flat(name):
    """pg_ops.ballquery_batch_p of a named scene, computed once"""
    s = SCENES[name]()
    idx, sl = pg_ops.ballquery_batch_p(s.xyz, s.batch_idx, s.batch_off, s.radius)
    idx.setflags(write=False)
    sl.setflags(write=False)
    return idx, sl


@functools.lru_cache(maxsize=None)
def lattice_scene(name):
    """3000 distinct cells of a 64^3 block in two batch items (1400 + 1600), r = 15 * 2^-10, at three placements; and two
    placements so far out that a cell index leaves the 18-bit field of the cell key: r = 2^-5, 1500 points every 8 units
    of a 128^3 block around |coordinate| = 4101 (cell size 1.001 * 2^-5: cell index 2^17 is at 4100.1)"""
    W = 1024                                     # lattice units per world unit
    if name in ("origin", "straddle", "offset"):
        origin = {"origin": (0, 0, 0), "straddle": (-32, -32, -32), "offset": (1000 * W, -3 * W, 7 * W)}[name]
        s = _scene(name, _block(3000, 64, 11) + np.asarray(origin), (1400, 1600), R_UNITS)
        if name == "straddle":
            K = units_of(s)
            assert (K.min(0) < 0).all() and (K.max(0) > 0).all() and (cells_fp32(s).min(0) < 0).all()
    else:
        origin = {"far_z": (5 * W, -7 * W, 4101 * W), "far_y": (3 * W, -4101 * W - 128, 2 * W)}[name]
        s = _scene(name, _block(1500, 16, 13, step=8) + np.asarray(origin), (700, 800), FAR_R_UNITS)
        c = cells_fp32(s)
        if name == "far_z":
            assert (c[:, 2] + CELL_BIAS >= 1 << CELL_BITS).all(), "every z cell is past the top of its key field"
        else:
            assert (c[:, 1] + CELL_BIAS < 0).all(), "every y cell is below the bottom of its key field"
        assert np.unique(c, axis=0).shape[0] >= 27 and true_counts(s).max() * 3 < BQ_CAP
    assert tie_pairs(s) >= 1000, "at least 1000 ordered pairs at exactly r"
    return s


def _sites(counts, seed, shift=(0, 0, 0)):
    """points on a row of sites 10 units apart, jittered by -1..1 per axis: sites next to each other are within
    r = 15 (<= 12 + jitter < 15), sites two apart are not (>= 18); a point of site i has n[i-1] + n[i] + n[i+1] hits"""
    rng = np.random.default_rng(seed)
    pts = []
    for i, n in enumerate(counts):
        pts.append(rng.integers(-1, 2, (n, 3)) + np.array([10 * i, 0, 0]) + np.asarray(shift))
    pts = np.concatenate(pts)
    site = np.repeat(np.arange(len(counts)), counts)
    perm = rng.permutation(len(pts))             # hits and non-hits interleave in index order
    return pts[perm], site[perm]


@functools.lru_cache(maxsize=None)
def cap_scene():
    """two batch items at the same place, 1501 and 1488 points (neither a multiple of 64, nor is the second offset); in
    each, points with exactly 1000 hits (grid path, list full), exactly 1001 (overflow scan: the last hit is cut) and
    ~1100 / ~1150 (the cut falls inside a 64-lane ballot, with non-hits between the hits)"""
    a, sa = _sites((400, 600, 1, 500), 21)
    b, sb = _sites((300, 700, 1, 450), 22)
    far = np.arange(37)[:, None] * np.array([0, 40, 0]) + np.array([0, 500, 0])
    b = np.concatenate([b, far])
    mix = np.random.default_rng(23).permutation(len(b))
    b = b[mix]
    s = _scene("cap", np.concatenate([a, b]), (len(a), len(b)), R_UNITS)
    assert all(int(n) % 64 for n in (len(a), len(b), s.batch_off[1]))
    cnt, (hit, _) = true_counts(s), hits_int(s)
    for lo, hi in zip(s.batch_off[:-1], s.batch_off[1:]):
        c = cnt[lo:hi]
        assert (c == BQ_CAP).any() and (c == BQ_CAP + 1).any() and (c > BQ_CAP + 64).any() and (c < BQ_CAP).any()
        for p in np.flatnonzero(c > BQ_CAP) + lo:
            row = hit[p, lo:hi]
            last = np.flatnonzero(row)[BQ_CAP - 1]               # the 1000th hit, counted inside the batch item
            assert not row[:last].all(), "non-hits before the cut: the first 1000 hits are no index prefix"
        big = np.flatnonzero(c > BQ_CAP + 64) + lo
        cut = np.array([np.flatnonzero(hit[p, lo:hi])[BQ_CAP - 1] for p in big])
        assert ((cut % 64) != 63).any(), "a cut in the middle of a 64-lane ballot"
    return s


@functools.lru_cache(maxsize=None)
def empty_item_scene():
    """three batch items, the middle one empty"""
    base = lattice_scene("origin")
    return _scene("empty_item", units_of(base)[:1200], (700, 0, 500), R_UNITS)


def zero_radius_scene():
    s = lattice_scene("origin")
    return Scene("r0", s.xyz[:500].copy(), s.batch_idx[:500].copy(), np.array([0, 500], np.int32), 0.0)


def single_point_scene():
    return _scene("single", [[3, -4, 5]], (1,), R_UNITS)


def no_point_scene():
    return _scene("none", np.zeros((0, 3)), (0,), R_UNITS)


SCENES = {name: functools.partial(lattice_scene, name) for name in ("origin", "straddle", "offset", "far_z", "far_y")}
SCENES.update(cap=cap_scene, empty_item=empty_item_scene, single=single_point_scene)
FAR = ("far_z", "far_y")


@functools.lru_cache(maxsize=None)
def large_scene():
    """N = 2048 * 256 + 1 points: one more than a launch has threads, so every per-point grid-stride loop takes a second
    trip.  Random cells of a 700^3 box (repeats allowed), two batch items: a ball of 15 units holds ~14,000 cells, mean count ~11.
    -> (scene, counts of every point, {p: list} for every 64th point)"""
    N = GRID_THREADS + 1
    rng = np.random.default_rng(31)
    s = _scene("large", rng.integers(0, 700, (N, 3)) - 300, (200001, N - 200001), R_UNITS)
    sample = np.arange(0, N, 64)
    counts, lists = kd_reference(s, sample)
    assert N > GRID_THREADS and 8 < counts.mean() < 14 and counts.max() < BQ_CAP and counts.min() >= 1
    counts.setflags(write=False)
    return s, counts, lists


# ---- the grid walk of csrc/cluster.hip, replayed in numpy ---------------------------------------------------------------
def cell_key(b, cx, cy, cz, masked):
    """cell_key() of csrc/cluster.hip in Python integers; ``masked`` = with each cell field cut to CELL_BITS"""
    f = [(int(c) + CELL_BIAS) & 0xFFFFFFFF for c in (cx, cy, cz)]           # (uint64_t)(uint32_t)(c + bias)
    if masked:
        f = [v & ((1 << CELL_BITS) - 1) for v in f]
    key = ((int(b) & 0xFFFFFFFF) << (3 * CELL_BITS)) | (f[0] << (2 * CELL_BITS)) | (f[1] << CELL_BITS) | f[2]
    return key & ((1 << 64) - 1)


def neighbour_keys(b, c, masked):
    return [cell_key(b, c[0] + dx, c[1] + dy, c[2] + dz, masked)
            for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def grid_walk_counts(scene, masked):
    """counts as bq_grid_kernel<false> finds them: points bucketed by key, the 27 neighbour keys of a point visited one
    after the other (a key that comes up twice is visited twice), hits by the fp32 distance expression"""
    cells = cells_fp32(scene)
    buckets = {}
    for p, (b, c) in enumerate(zip(scene.batch_idx, cells)):
        buckets.setdefault(cell_key(b, c[0], c[1], c[2], masked), []).append(p)
    buckets = {k: np.asarray(v) for k, v in buckets.items()}
    r2 = np.float32(scene.radius) * np.float32(scene.radius)
    x = scene.xyz
    out = np.zeros(len(x), dtype=np.int64)
    for p, (b, c) in enumerate(zip(scene.batch_idx, cells)):
        for key in neighbour_keys(b, c, masked):
            ks = buckets.get(key)
            if ks is None:
                continue
            e = x[p][None, :] - x[ks]
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).astype(np.float32) + (e[:, 2] * e[:, 2]).astype(np.float32)
            out[p] += int((d2 < r2).sum())
    return out


# ===================================================================================================== bfs_cluster
BfsCase = namedtuple("BfsCase", "sem idx start_len thresholds")


def _lists(n, pairs, with_self=True):
    """symmetric ascending neighbour lists (every point lists itself, as a ball query with r > 0 does)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    parts = [p, p[:, ::-1]]
    if with_self:
        parts.append(np.stack([np.arange(n)] * 2, 1))
    both = np.unique(np.concatenate(parts), axis=0)              # sorted by (row, column): ascending lists
    counts = np.bincount(both[:, 0], minlength=n)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return both[:, 1].astype(np.int32), np.stack([start, counts], 1).astype(np.int32)


def _bfs_case(sem, pairs, thresholds, with_self=True):
    sem = np.asarray(sem, dtype=np.int32)
    idx, sl = _lists(len(sem), pairs, with_self)
    for p in (0, len(sem) // 2, len(sem) - 1):
        row = idx[sl[p, 0]:sl[p, 0] + sl[p, 1]]
        assert (np.diff(row) > 0).all()
    return BfsCase(sem, idx, sl, tuple(thresholds))


def frontier_sizes(case, threshold=1):
    """per kept cluster of pg_ops.bfs_cluster: the number of points at BFS depth 0, 1, 2, ... (read off its FIFO order)"""
    ci, co = pg_ops.bfs_cluster(case.sem, case.idx, case.start_len, threshold)
    depth = np.full(len(case.sem), -1, dtype=np.int64)
    out = []
    for c in range(len(co) - 1):
        pts = ci[co[c]:co[c + 1], 1]
        depth[pts[0]] = 0
        for p in pts.tolist():
            s, n = case.start_len[p]
            for nb in case.idx[s:s + n].tolist():
                if case.sem[nb] == case.sem[p] and depth[nb] < 0:
                    depth[nb] = depth[p] + 1
        out.append(np.bincount(depth[pts]).tolist())
    return out


STAR_LEAVES = (255, 256, 257, 511, 512, 513)     # around one and two 256-thread chunks of a frontier


def _bfs_stars():
    """centre -> L leaves -> one child per leaf: frontiers 1, L, L; the centre has the component's smallest index (the
    seed), the other indices are shuffled"""
    rng = np.random.default_rng(41)
    pairs, base = [], 0
    for L in STAR_LEAVES:
        local = np.concatenate([[0], 1 + rng.permutation(2 * L)]) + base
        leaves, kids = local[1:1 + L], local[1 + L:]
        pairs += [np.stack([np.full(L, base), leaves], 1), np.stack([leaves, kids], 1)]
        base += 1 + 2 * L
    case = _bfs_case(np.zeros(base), np.concatenate(pairs), (1, 512, 1027, 1028))
    assert frontier_sizes(case) == [[1, L, L] for L in STAR_LEAVES]
    assert max(1 + 2 * L for L in STAR_LEAVES) == 1027
    return case


def _bfs_layers():
    """seed -> 300 -> 700, every point of the last layer listed by 3 or more of the 300: the parent with the smallest
    queue position owns it"""
    rng = np.random.default_rng(42)
    mid = 1 + rng.permutation(300)
    last = 301 + rng.permutation(700)
    pairs = [np.stack([np.zeros(300, np.int64), mid], 1)]
    for t in range(4):
        pairs.append(np.stack([mid[(np.arange(700) * 7 + 11 * t) % 300], last], 1))
    case = _bfs_case(np.zeros(1001), np.concatenate(pairs), (1, 1001, 1002))
    assert frontier_sizes(case) == [[1, 300, 700]]
    parents = case.start_len[last, 1] - 1
    assert parents.min() >= 3
    return case


def _bfs_chain():
    """a path 2000 deep from the seed, indices shuffled along it"""
    order = np.concatenate([[0], 1 + np.random.default_rng(43).permutation(2000)])
    case = _bfs_case(np.zeros(2001), np.stack([order[:-1], order[1:]], 1), (1, 2001))
    assert frontier_sizes(case) == [[1] * 2001]
    return case


def _bfs_labels():
    """i lists i +- 1 and i +- 2; labels alternate between 3 and -100: two components, interleaved by index, each held
    together by the +- 2 links only"""
    n = 999
    i = np.arange(n)
    pairs = np.concatenate([np.stack([i[:-1], i[1:]], 1), np.stack([i[:-2], i[2:]], 1)])
    case = _bfs_case(np.where(i % 2, -100, 3), pairs, (1, 499, 500, 501))
    f = frontier_sizes(case)
    assert [sum(x) for x in f] == [500, 499] and (case.sem < 0).any()
    return case


def _bfs_threshold():
    """cliques of 37 and 36 points, and singletons, at threshold 37"""
    T = 37
    perm = np.random.default_rng(44).permutation(2 * T - 1 + 20)
    a, b = perm[:T], perm[T:2 * T - 1]
    pairs = [np.stack(np.meshgrid(g, g), -1).reshape(-1, 2) for g in (a, b)]
    case = _bfs_case(np.full(len(perm), 5), np.concatenate(pairs), (T - 1, T, T + 1, 1))
    sizes = sorted(sum(x) for x in frontier_sizes(case))
    assert sizes[-2:] == [T - 1, T]
    assert len(pg_ops.bfs_cluster(case.sem, case.idx, case.start_len, T)[1]) == 2
    return case


def _bfs_fallback():
    """a centre that lists 1000 points (itself and 999 leaves): a list at the cap, the host walk takes over"""
    leaves = 1 + np.arange(999)
    case = _bfs_case(np.zeros(1300), np.stack([np.zeros(999, np.int64), leaves], 1), (1, 2, 1000))
    assert case.start_len[:, 1].max() == BQ_CAP
    return case


def _bfs_singletons():
    """70,000 points that list only themselves: 70,000 kept clusters at threshold 1 (one workgroup each), none at 2"""
    n = 70000
    case = _bfs_case(np.arange(n) % 3, np.zeros((0, 2)), (1, 2))
    assert (case.start_len[:, 1] == 1).all()
    return case


def _bfs_no_lists():
    """what a ball query with r == 0 returns: no point lists even itself"""
    return _bfs_case(np.arange(300) % 2, np.zeros((0, 2)), (1, 2), with_self=False)


def _bfs_none():
    return BfsCase(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), (1,))


BFS_CASES = {"stars": _bfs_stars, "layers": _bfs_layers, "chain": _bfs_chain, "labels": _bfs_labels,
             "threshold": _bfs_threshold, "fallback": _bfs_fallback, "singletons": _bfs_singletons,
             "no_lists": _bfs_no_lists, "none": _bfs_none}


@functools.lru_cache(maxsize=None)
def bfs_case(name):
    return BFS_CASES[name]()


def components(case):
    """(root, size) by scipy on the same-label subgraph: root[i] = smallest index of i's component, size[i] = its size"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(case.sem)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    u = np.repeat(np.arange(n), case.start_len[:, 1])
    v = case.idx.astype(np.int64)
    keep = case.sem[u] == case.sem[v]
    g = csr_matrix((np.ones(int(keep.sum()), np.int8), (u[keep], v[keep])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    root = np.full(lab.max() + 1, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n))
    return root[lab].astype(np.int32), np.bincount(lab)[lab].astype(np.int32)


# ===================================================================================================== voxelization_idx
_M64 = (1 << 64) - 1
I64_MAX = 2 ** 63 - 1


def mix64(x):
    """mix64 of csrc/common.h"""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


def hash4(c):
    """hash4 of csrc/voxelize_idx.hip on a row of four Python integers"""
    h = mix64((int(c[0]) + 0x9e3779b97f4a7c15) & _M64)
    for k in (1, 2, 3):
        h = mix64(h ^ (int(c[k]) & _M64))
    return h


def table_cap(n):
    cap = 16
    while cap < 2 * n:
        cap <<= 1
    return cap


def first_occurrence(coords):
    """(voxel_locs, p2v, v2p) of voxelization_idx by np.unique: voxels in order of first occurrence, lists ascending"""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    N = coords.shape[0]
    if N == 0:
        return np.zeros((0, 4), np.int64), np.zeros(0, np.int32), np.zeros((0, 1), np.int32)
    _, first, inv = np.unique(coords, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first)
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    p2v = rank[inv]
    counts = np.bincount(p2v, minlength=len(first))
    by_voxel = np.argsort(p2v, kind="stable")
    pos = np.arange(N) - np.repeat(np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)
    v2p = np.zeros((len(first), 1 + counts.max()), dtype=np.int32)
    v2p[:, 0] = counts
    v2p[p2v[by_voxel], 1 + pos] = by_voxel
    return coords[first[order]], p2v.astype(np.int32), v2p


def _vi(rows):
    out = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 4))
    out.setflags(write=False)
    return out


def _vi_one_voxel():
    """all 4096 points in one voxel (vi_fill_kernel walks a run backwards: quadratic, so no more than this)"""
    c = _vi(np.tile([1, -5, 7, 9], (4096, 1)))
    assert len(c) <= 4096 and np.unique(c, axis=0).shape[0] == 1
    return c


def _vi_all_distinct():
    rng = np.random.default_rng(51)
    lin = rng.choice(2 * 40 ** 3, 5000, replace=False)
    c = _vi(np.stack(np.unravel_index(lin, (2, 40, 40, 40)), 1) - np.array([0, 20, 20, 20]))
    assert np.unique(c, axis=0).shape[0] == 5000
    return c


def _vi_one_column():
    """for each of the four columns a pair of voxels that differ in that column only, each voxel several times"""
    base = np.array([1, 20, -30, 40])
    rows = [base]
    for k in range(4):
        other = base.copy()
        other[k] += 1
        rows.append(other)
    rows = np.asarray(rows)
    for k in range(4):
        d = rows[0] != rows[1 + k]
        assert d.sum() == 1 and d[k]
    pick = np.random.default_rng(52).integers(0, 5, 300)
    c = _vi(rows[pick])
    assert np.unique(c, axis=0).shape[0] == 5
    return c


def _vi_extreme():
    """-1, -2^40 and +-(2^63 - 1) in every column, alone and together"""
    vals = [-1, -2 ** 40, I64_MAX, -I64_MAX, 0]
    rows = [[a, b, a, b] for a in vals for b in vals] + [[v if k == j else 0 for k in range(4)] for v in vals for j in range(4)]
    rows = np.asarray(rows, dtype=np.int64)
    pick = np.random.default_rng(53).integers(0, len(rows), 400)
    c = _vi(rows[pick])
    for v in vals:
        assert (c == v).any()
    return c


def _vi_full_table(n):
    """N distinct voxels with cap == 2 N: the table at its highest load"""
    assert table_cap(n) == 2 * n
    c = _vi([[k % 2, 3 * k, -k, k * k] for k in range(n)])
    assert np.unique(c, axis=0).shape[0] == n
    return c


def _vi_wrap():
    """N = 8 (cap 16): three distinct voxels whose first slot is the last one, 15 -- two of them are pushed on to slots 0
    and 1 -- each twice, and two other voxels; by the Python replica of hash4"""
    cap = table_cap(8)
    last = [(0, x, 0, 0) for x in range(2000) if hash4((0, x, 0, 0)) & (cap - 1) == cap - 1][:3]
    assert len(last) == 3 and len(set(last)) == 3
    rows = [last[0], last[1], (0, -1, 0, 0), last[2], last[1], last[0], last[2], (1, -1, 0, 0)]
    assert len(rows) == 8 and cap == 16
    return _vi(rows)


def _vi_large():
    """N = 2048 * 256 + 1 points in ~128,000 voxels: the per-point loops take a second trip, and the points of a voxel
    are spread over the whole launch (so which of them claims the voxel's slot first is up to the scheduler)"""
    N = GRID_THREADS + 1
    rng = np.random.default_rng(54)
    c = _vi(np.concatenate([rng.integers(0, 2, (N, 1)), rng.integers(-20, 20, (N, 3))], 1))
    assert N > GRID_THREADS
    return c


def vi_random_small(seed):
    """N = 8 with cap == 2 N, coordinates from a range small enough for repeats"""
    return _vi(np.random.default_rng(1000 + seed).integers(-2, 3, (8, 4)))


VI_CASES = {"one_voxel": _vi_one_voxel, "all_distinct": _vi_all_distinct, "one_column": _vi_one_column,
            "extreme": _vi_extreme, "full_8": functools.partial(_vi_full_table, 8),
            "full_16": functools.partial(_vi_full_table, 16), "wrap": _vi_wrap, "large": _vi_large,
            "none": lambda: _vi(np.zeros((0, 4)))}
VI_DICT_ORACLE_MAX = 5000


@functools.lru_cache(maxsize=None)
def vi_case(name):
    return VI_CASES[name]()


# ===================================================================================================== voxelization
VoxCase = namedtuple("VoxCase", "v2p n_points")


def _v2p(row_sizes, n_points, seed, unused):
    """a handwritten map: row m lists row_sizes[m] points, every point in at most one row, ``unused`` points in none;
    the padding behind a list is INT32_MIN -- an index that must never be read"""
    rng = np.random.default_rng(seed)
    row_sizes = np.asarray(row_sizes, dtype=np.int64)
    assert row_sizes.sum() + unused == n_points
    perm = rng.permutation(n_points)
    v2p = np.full((len(row_sizes), 1 + int(row_sizes.max())), INT32_MIN, dtype=np.int32)
    v2p[:, 0] = row_sizes
    at = 0
    for m, n in enumerate(row_sizes.tolist()):
        v2p[m, 1:1 + n] = perm[at:at + n]
        at += n
    listed = np.concatenate([v2p[m, 1:1 + n] for m, n in enumerate(row_sizes.tolist())])
    assert len(np.unique(listed)) == len(listed) and n_points - len(listed) == unused
    return VoxCase(v2p, n_points)


@functools.lru_cache(maxsize=None)
def vox_small():
    """rows of 0, 1, 2, 3, 300 ... points, INT32_MIN padding, 61 points in no row"""
    sizes = [0, 1, 2, 3, 300, 0, 0, 7, 64, 65] + list(np.random.default_rng(61).integers(0, 6, 400)) + [0]
    case = _v2p(sizes, int(np.sum(sizes)) + 61, 62, 61)
    n = case.v2p[:, 0]
    assert (n == 0).sum() >= 4 and n.max() == 300 and (case.v2p == INT32_MIN).any()
    return case


VOX_LARGE_M, VOX_LARGE_C = 87382, 6


@functools.lru_cache(maxsize=None)
def vox_large():
    """M * C = 524,292 > 2048 * 256 with C = 6 (the smallest such M): the grid-stride loop takes a second trip, under the
    32-bit division arm of row_col"""
    assert VOX_LARGE_M * VOX_LARGE_C > GRID_THREADS >= (VOX_LARGE_M - 1) * VOX_LARGE_C
    sizes = np.random.default_rng(63).integers(0, 4, VOX_LARGE_M)
    sizes[-1] = 3                                      # the items of the second trip belong to a row that has points
    return _v2p(sizes, int(sizes.sum()) + 1000, 64, 1000)


VOX_CHANNELS = (1, 3, 6, 8)       # row_col: powers of two shift, the others divide


def vox_feats(n, C, seed):
    return np.random.default_rng(seed).standard_normal((n, C)).astype(np.float32)


def vox_fp64(feats, v2p, mode):
    """(mean or sum at fp64, the bound (n + 2) * 2^-24 * sum |w x_i|): n sequential fp32 additions, one multiplication
    per term and one reciprocal, each within 2^-24 relative"""
    f = np.asarray(feats, dtype=np.float64)
    M, C = v2p.shape[0], f.shape[1]
    out, mag = np.zeros((M, C)), np.zeros((M, C))
    n = v2p[:, 0].astype(np.int64)
    w = np.where((mode == 4) & (n > 0), 1.0 / np.maximum(n, 1), 1.0)
    for i in range(v2p.shape[1] - 1):
        live = n > i
        out[live] += w[live, None] * f[v2p[live, 1 + i]]
        mag[live] += np.abs(w[live, None] * f[v2p[live, 1 + i]])
    return out, (n[:, None] + 2) * 2.0 ** -24 * mag


def vox_bwd_fp64(dout, v2p, n_points, mode):
    """(gradient at fp64, bound 3 * 2^-24 |w g|: a sum of one term; exactly 0 for a point in no row)"""
    g = np.asarray(dout, dtype=np.float64)
    d = np.zeros((n_points, g.shape[1]))
    n = v2p[:, 0].astype(np.int64)
    w = np.where((mode == 4) & (n > 0), 1.0 / np.maximum(n, 1), 1.0)
    for i in range(v2p.shape[1] - 1):
        live = n > i
        d[v2p[live, 1 + i]] = w[live, None] * g[live]
    return d, 3 * 2.0 ** -24 * np.abs(d)
