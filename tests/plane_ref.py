"""fp64 numpy oracle of the S3DIS wall split (utils/planeSegment.py:get_room_walls of the reference with open3d's
segment_plane restated on given triples).  No torch, no GPU.

Everything is written element-wise in the operation order of the device kernels -- dist = |((a*x + b*y) + c*z) + d|
with fp32 coordinates widened to fp64 -- without ``@`` or ``dot`` (BLAS may fuse or reorder), so ``dist < thr`` is the
same set of points here and on the device as long as no distance sits within rounding of the threshold: ``score``
reports the smallest |dist - thr| it saw and the callers assert it is above ``GAP``."""
import numpy as np

GAP = 1e-10


def make_room(seed, walls=(11000, 7000, 5000, 3000), clutter=2000, noise=0.03, size=(5.0, 4.0, 2.6)):
    """fp32 [sum(walls) + clutter, 3]: the four walls of a ``size`` room with uniform +-``noise`` across each wall
    and uniform clutter inside, shuffled"""
    rng = np.random.default_rng(seed)
    lx, ly, lz = size
    parts = []
    for k, n in enumerate(walls):
        along = rng.random(n) * (lx if k % 2 == 0 else ly)
        z = rng.random(n) * lz
        off = (rng.random(n) * 2 - 1) * noise
        if k == 0:
            p = np.stack([along, off, z], 1)                 # y = 0
        elif k == 1:
            p = np.stack([lx + off, along, z], 1)            # x = lx
        elif k == 2:
            p = np.stack([along, ly + off, z], 1)            # y = ly
        else:
            p = np.stack([off, along, z], 1)                 # x = 0
        parts.append(p)
    parts.append(rng.random((clutter, 3)) * np.array(size))
    xyz = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


def draw_triples(n, iters, rng):
    """one ``choice(n, 3, replace=False)`` per iteration"""
    return np.stack([rng.choice(n, 3, replace=False) for _ in range(iters)]).astype(np.int64)


def planes_from_triples(pts):
    """pts [H,3,3] -> (planes fp64 [H,4] = (n / |n|, -n.p0) with n = (p1-p0) x (p2-p0), valid [H]: |n| > 0 and finite)"""
    p = np.asarray(pts, dtype=np.float64)
    H = p.shape[0]
    planes = np.zeros((H, 4))
    valid = np.zeros(H, dtype=bool)
    with np.errstate(all="ignore"):
        for h in range(H):
            p0, p1, p2 = p[h]
            ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
            vx, vy, vz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
            nx = uy * vz - uz * vy
            ny = uz * vx - ux * vz
            nz = ux * vy - uy * vx
            norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
            if not norm > 0:
                continue
            a, b, c = nx / norm, ny / norm, nz / norm
            d = -((a * p0[0] + b * p0[1]) + c * p0[2])
            if np.isfinite([a, b, c, d]).all():
                planes[h] = (a, b, c, d)
                valid[h] = True
    return planes, valid


def distances(xyz, plane):
    """fp64 [N]: |((a*x + b*y) + c*z) + d|"""
    x, y, z = (np.asarray(xyz)[:, k].astype(np.float64) for k in range(3))
    a, b, c, d = (np.float64(v) for v in plane)
    with np.errstate(all="ignore"):
        return np.abs(((a * x + b * y) + c * z) + d)


def score(xyz, planes, thr):
    """-> (count int64 [H], sumsq fp64 [H], smallest |dist - thr| over all finite distances)"""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    count = np.zeros(len(planes), dtype=np.int64)
    sumsq = np.zeros(len(planes), dtype=np.float64)
    gap = np.inf
    for h, plane in enumerate(planes):
        dist = distances(xyz, plane)
        inl = dist < thr                                    # NaN and inf: False
        count[h] = int(inl.sum())
        sumsq[h] = float((dist[inl] * dist[inl]).sum())
        fin = np.isfinite(dist)
        if fin.any():
            gap = min(gap, float(np.abs(dist[fin] - thr).min()))
    return count, sumsq, gap


def mark(xyz, plane, thr):
    return distances(xyz, plane) < thr


def choose(count, sumsq):
    """most inliers, then the smaller sum of squares, then the earliest; plain loop with open3d's strict comparisons"""
    best = -1
    for h in range(len(count)):
        if best < 0 or count[h] > count[best] or (count[h] == count[best] and sumsq[h] < sumsq[best]):
            best = h
    return best


def get_room_walls_ref(xyz, wall_ind, distance=0.1, iter=200, max_num=4, seed=None, samples=None, min_points=10000):
    """-> (walls: list of bool [N], info).  ``samples[round]`` int [iter,3] into the remaining wall points, else drawn
    from default_rng(seed).  info: the triples used per round, the smallest |dist - thr| seen, whether the top count was
    ever shared, and the number of wall points left."""
    xyz = np.asarray(xyz)
    wall_ind = np.asarray(wall_ind).astype(bool)
    remain_ind = np.where(wall_ind)[0]
    remain_xyz = xyz[wall_ind]
    rng = np.random.default_rng(seed) if samples is None else None
    walls, used, gap, top_ties = [], [], np.inf, 0
    for rnd in range(max_num):
        n = len(remain_ind)
        if n < min_points or n < 3:
            break
        tri = draw_triples(n, iter, rng) if samples is None else np.asarray(samples[rnd], dtype=np.int64).reshape(-1, 3)
        used.append(tri)
        planes, valid = planes_from_triples(remain_xyz[tri.reshape(-1)].reshape(-1, 3, 3))
        planes = planes[valid]
        if len(planes) == 0:
            break
        count, sumsq, g = score(remain_xyz, planes, distance)
        gap = min(gap, g)
        best = choose(count, sumsq)
        if count[best] == 0:
            break
        top_ties += int((count == count[best]).sum() > 1)
        inl = mark(remain_xyz, planes[best], distance)
        m = np.zeros(len(xyz), dtype=bool)
        m[remain_ind[inl]] = True
        walls.append(m)
        remain_ind, remain_xyz = remain_ind[~inl], remain_xyz[~inl]
    return walls, {"samples": used, "gap": gap, "top_ties": top_ties, "remaining": len(remain_ind)}
