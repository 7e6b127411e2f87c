"""PointGroup's elastic distortion (``elastic`` of modules/datasets/scannetv2_dataset.py:222-249) restated in plain numpy
fp64, without scipy: what ``wsis_datasets.ScenePrep.elastic`` computes through ``scipy.ndimage.convolve`` and
``RegularGridInterpolator``, and what csrc/sceneprep.hip computes on the device.  Every operation is written out in the
order the result depends on, so the three agree bit for bit and are compared with ``np.array_equal``."""
import numpy as np

W = np.float64(np.float32(1) / np.float32(3))            # the blur tap: 1/3 rounded to fp32, widened


def grid_shape(xyz, gran):
    """step 1: ``bb``, int32 [3]"""
    return np.abs(np.asarray(xyz, dtype=np.float64)).max(0).astype(np.int32) // gran + 3


def draw_noise(rng, bb):
    """three grids of shape ``bb``, drawn as fp64 normals in this order and cast to fp32"""
    return [rng.randn(int(bb[0]), int(bb[1]), int(bb[2])).astype(np.float32) for _ in range(3)]


def blur_pass(grid, axis):
    """out[i] = fp32((w*in[i-1] + w*in[i]) + w*in[i+1]) along ``axis``; neighbours outside the grid are 0"""
    g = np.moveaxis(np.asarray(grid, dtype=np.float32), axis, 0).astype(np.float64)
    left, right = np.zeros_like(g), np.zeros_like(g)
    left[1:] = g[:-1]
    right[:-1] = g[1:]
    out = (W * left + W * g) + W * right
    return np.ascontiguousarray(np.moveaxis(out.astype(np.float32), 0, axis))


def blur(grid):
    """step 2: six passes, along axis 0, 1, 2, 0, 1, 2"""
    for axis in (0, 1, 2, 0, 1, 2):
        grid = blur_pass(grid, axis)
    return grid


def axes(bb, gran):
    """step 3: the nodes of the three axes, exact integers as fp64"""
    return [(-(int(b) - 1) * int(gran) + 2 * int(gran) * np.arange(int(b), dtype=np.int64)).astype(np.float64) for b in bb]


def displacement(xyz, grids, gran):
    """step 4: fp64 [N,3], column m from ``grids[m]`` (fp32, blurred); 0 in all three columns for a point with a
    coordinate outside the grid on any axis"""
    xyz = np.asarray(xyz, dtype=np.float64)
    bb = grids[0].shape
    idx, t = [], []
    inside = np.ones(len(xyz), dtype=bool)
    for j, a in enumerate(axes(bb, gran)):
        x = xyz[:, j]
        inside &= (x >= a[0]) & (x <= a[-1])
        c = (a[None, :] < x[:, None]).sum(1)                         # nodes < x
        i = np.clip(c - 1, 0, bb[j] - 2)
        idx.append(i)
        t.append((x - a[i]) / (a[i + 1] - a[i]))
    d = np.zeros((len(xyz), 3), dtype=np.float64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                wx = t[0] if cx else 1 - t[0]
                wy = t[1] if cy else 1 - t[1]
                wz = t[2] if cz else 1 - t[2]
                w = (wx * wy) * wz
                for m in range(3):
                    d[:, m] = d[:, m] + grids[m][idx[0] + cx, idx[1] + cy, idx[2] + cz].astype(np.float64) * w
    d[~inside] = 0.0
    return d


def apply(xyz, grids, gran, mag):
    """steps 3-5 on blurred grids"""
    xyz = np.asarray(xyz, dtype=np.float64)
    return xyz + displacement(xyz, grids, gran) * mag


def elastic(xyz, gran, mag, rng):
    """steps 1-5, the draws taken from ``rng`` (a ``numpy.random.RandomState``)"""
    noise = draw_noise(rng, grid_shape(xyz, gran))
    return apply(xyz, [blur(g) for g in noise], gran, mag)
