"""Elastic distortion on the host: the plain-numpy restatement (tests/elastic_ref.py) against ``ScenePrep.elastic``
(scipy), both against the reference's own method (tests/golden/elastic_golden.npz, make_elastic_golden.py), and the
``with_elastic`` switch of ``ScenePrep.__call__``.  Everything is compared with ``np.array_equal``: the
restatement performs scipy's operations in scipy's order, so no tolerance is needed.  CPU only.

``ScenePrep.elastic`` sizes its grid from the points, and that grid always reaches beyond them ((bb - 1) * gran >
max|x|): a point on the outermost node, or outside the grid, can only be handed to the operators directly.  Those cases
run ``scipy_apply`` below, the method's own two scipy lines on given grids."""
import importlib
import os

import numpy as np
import pytest
import torch

importlib.import_module("3d-wsis_amd")
import wsis_datasets as datasets  # noqa: E402
import harness  # noqa: E402
from tests import elastic_ref as ref  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "elastic_golden.npz"))
PAIRS = ((6, 40.0), (20, 160.0))
ROOM = dict(room=(1.0, 0.9, 0.8), n_box=2)
_SCENE = []


def _scene():
    if not _SCENE:
        _SCENE.append(datasets.synthetic_scene_to_reference_format(harness.make_scene(5, **ROOM)))
    return _SCENE[0]


def _both(xyz, gran, mag, seed):
    return datasets.ScenePrep(seed=seed).elastic(xyz, gran, mag), ref.elastic(xyz, gran, mag, np.random.RandomState(seed))


def scipy_apply(xyz, grids, gran, mag):
    """lines :245-249 of the method on given (blurred) grids"""
    import scipy.interpolate
    bb = grids[0].shape
    ax = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in bb]
    interp = [scipy.interpolate.RegularGridInterpolator(ax, n, bounds_error=0, fill_value=0) for n in grids]
    return xyz + np.hstack([i(xyz)[:, None] for i in interp]) * mag


def _grids(bb, seed):
    return [ref.blur(g) for g in ref.draw_noise(np.random.RandomState(seed), bb)]


# ---- the restatement against scipy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("gran,mag", PAIRS)
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_restatement_equals_the_scipy_method(gran, mag, seed):
    rs = np.random.RandomState(50 + seed)
    xyz = (rs.rand(2000, 3) - np.array([0.3, 0.5, 0.05])) * np.array([400.0, 300.0, 150.0])
    got, want = _both(xyz, gran, mag, seed)
    assert np.array_equal(want, got) and not np.array_equal(got, xyz)


@pytest.mark.parametrize("gran,mag", PAIRS)
def test_a_cloud_inside_one_cell_has_the_smallest_grid(gran, mag):
    xyz = (np.random.RandomState(3).rand(300, 3) * 2 - 1) * (gran - 0.5)
    assert list(ref.grid_shape(xyz, gran)) == [3, 3, 3]
    got, want = _both(xyz, gran, mag, 11)
    assert np.array_equal(want, got)


@pytest.mark.parametrize("gran,mag", PAIRS)
def test_negative_only_coordinates(gran, mag):
    xyz = -np.random.RandomState(4).rand(500, 3) * np.array([300.0, 200.0, 90.0]) - 0.25
    got, want = _both(xyz, gran, mag, 12)
    assert np.array_equal(want, got)


def special_points(bb, gran):
    """points on interior nodes, on the outermost node of each axis (both ends), at mid-cell, and beside them"""
    a = ref.axes(bb, gran)
    rs = np.random.RandomState(9)
    rows = []
    for _ in range(40):                                              # interior nodes, all three coordinates on a node
        rows.append([a[j][rs.randint(1, bb[j] - 1)] for j in range(3)])
    for j in range(3):                                               # the outermost nodes of axis j, the others anywhere
        for end in (0, -1):
            p = [rs.uniform(a[k][0], a[k][-1]) for k in range(3)]
            p[j] = a[j][end]
            rows.append(p)
    rows.append([a[j][0] for j in range(3)])                         # the two corners of the grid
    rows.append([a[j][-1] for j in range(3)])
    for _ in range(40):                                              # mid-cell
        rows.append([a[j][rs.randint(0, bb[j] - 1)] + gran for j in range(3)])
    for _ in range(40):                                              # one coordinate on a node, the others not
        p = [rs.uniform(a[k][0], a[k][-1]) for k in range(3)]
        j = rs.randint(3)
        p[j] = a[j][rs.randint(0, bb[j])]
        rows.append(p)
    return np.asarray(rows, dtype=np.float64)


@pytest.mark.parametrize("gran,mag", PAIRS)
def test_points_on_nodes_and_at_mid_cell(gran, mag):
    bb = (5, 4, 7)
    grids = _grids(bb, 21)
    xyz = special_points(bb, gran)
    assert np.array_equal(scipy_apply(xyz, grids, gran, mag), ref.apply(xyz, grids, gran, mag))
    # through the method itself: interior nodes and mid-cells of the grid the method will choose for these points
    big = np.array([[4.5 * gran, 3.5 * gran, 6.5 * gran]])           # fixes bb = (7, 6, 9)
    bb2 = ref.grid_shape(big, gran)
    inner = special_points(bb2, gran)
    inner = inner[(np.abs(inner) < np.abs(big)).all(1)]
    xyz2 = np.concatenate([big, -big, inner])
    assert len(inner) > 40 and list(ref.grid_shape(xyz2, gran)) == list(bb2)
    got, want = _both(xyz2, gran, mag, 13)
    assert np.array_equal(want, got)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_point_outside_the_grid_is_not_moved_on_any_column(axis):
    gran, mag, bb = 6, 40.0, (4, 5, 3)
    grids = _grids(bb, 22)
    a = ref.axes(bb, gran)
    xyz = np.array([[1.5, -2.5, 3.25]] * 4)
    xyz[0, axis] = a[axis][-1] + 0.5
    xyz[1, axis] = a[axis][0] - 1e-9
    xyz[2, axis] = np.nextafter(a[axis][-1], np.inf)
    d = ref.displacement(xyz, grids, gran)
    assert (d[:3] == 0).all() and (d[3] != 0).all()
    assert np.array_equal(ref.apply(xyz, grids, gran, mag)[:3], xyz[:3])
    assert np.array_equal(scipy_apply(xyz, grids, gran, mag), ref.apply(xyz, grids, gran, mag))


# ---- the reference's own method ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(int(G["n_cases"])))
def test_golden(k):
    gran, mag, seed = G[f"cfg_{k}"]
    gran, seed = int(gran), int(seed)
    assert (gran, float(mag)) == PAIRS[k]
    xyz = G[f"in_{k}"]
    assert (xyz < 0).any() and (xyz > 0).any()
    assert np.array_equal(ref.grid_shape(xyz, gran), G[f"bb_{k}"])
    assert np.array_equal(ref.elastic(xyz, gran, float(mag), np.random.RandomState(seed)), G[f"out_{k}"])
    assert np.array_equal(datasets.ScenePrep(seed=seed).elastic(xyz, gran, float(mag)), G[f"out_{k}"])


# ---- the switch -------------------------------------------------------------------------------------------------------
def _fields(item):
    scene, loc, loc_offset, loc_float, feat, sem, ins, sp, g, inst_num, info, pointnum = item
    return dict(loc=loc.numpy(), loc_offset=loc_offset.numpy(), loc_float=loc_float.numpy(), feat=feat.numpy(),
                sem=sem.numpy(), ins=ins.numpy(), sp=sp.numpy(), inst_num=inst_num, inst_info=info.numpy(),
                inst_pointnum=np.asarray(pointnum), g_v=g.vs["v"], g_edges=g.edges,
                g_off=g.vs["superpoint_offset_vector"])


def test_the_switch_changes_loc_and_loc_offset_only():
    tup, graph = _scene()
    on = _fields(datasets.ScenePrep(aug=True, seed=5, with_elastic=True)(tup, graph))
    off = _fields(datasets.ScenePrep(aug=True, seed=5)(tup, graph))
    assert on["loc"].shape == off["loc"].shape and not np.array_equal(on["loc"], off["loc"])
    for k in off:
        if k not in ("loc", "loc_offset"):
            assert np.array_equal(on[k], off[k]), k
    # where it should: the distorted coordinates, shifted to their own minimum, truncated
    h = datasets.ScenePrep(aug=True, seed=5)
    xyz = np.matmul(np.asarray(tup[0]), h.aug_matrix(True, True, True)) * 50
    for gran, mag in PAIRS:
        xyz = ref.elastic(xyz, gran, mag, h.rng)
    assert np.array_equal(on["loc_offset"], torch.from_numpy(xyz.min(0)).long().numpy())
    assert np.array_equal(on["loc"], torch.from_numpy(xyz - xyz.min(0)).long().numpy())
    assert on["loc"].min() == 0


@pytest.mark.parametrize("version", [1, 2])
def test_the_draw_order(version):
    """subsample choice, augmentation matrix, three grids of call 1, three grids of call 2, crop draws: the item
    re-derived by hand from a fresh RandomState, the crop rounds running"""
    tup, graph = _scene()
    seed, max_npoint = 17, 3000
    kw = dict(aug=True, seed=seed, max_npoint=max_npoint, subsample_train=True, crop_version=version)
    item = _fields(datasets.ScenePrep(with_elastic=True, **kw)(tup, graph))
    h = datasets.ScenePrep(**kw)                                     # its methods draw from h.rng, a fresh RandomState
    n = len(tup[0])
    pick = h.rng.choice(n, size=n // 4, replace=False)               # 1
    mid = np.matmul(np.asarray(tup[0])[pick], h.aug_matrix(True, True, True))      # 2
    xyz = mid * 50
    for gran, mag in PAIRS:                                          # 3, 4
        bb = ref.grid_shape(xyz, gran)
        noise = [h.rng.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
        xyz = ref.apply(xyz, [ref.blur(g) for g in noise], gran, mag)
    offset = xyz.min(0)
    xyz, valid = (h.crop if version == 1 else h.crop_v2)(xyz - offset)             # 5
    assert 0 < valid.sum() <= max_npoint < len(valid)
    assert np.array_equal(item["loc_offset"], torch.from_numpy(offset).long().numpy())
    assert np.array_equal(item["loc"], torch.from_numpy(xyz[valid]).long().numpy())
    assert np.array_equal(item["loc_float"], mid[valid])


def test_without_augmentation_the_switch_does_nothing_and_draws_nothing():
    tup, graph = _scene()
    preps = [datasets.ScenePrep(aug=False, test_mode=tm, seed=8, with_elastic=we) for tm in (False, True)
             for we in (False, True)]
    items = [_fields(p(tup, graph)) for p in preps]
    for a, b, pa, pb in ((items[0], items[1], preps[0], preps[1]), (items[2], items[3], preps[2], preps[3])):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        sa, sb = pa.rng.get_state(), pb.rng.get_state()
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    fresh = np.random.RandomState(8).get_state()
    assert np.array_equal(preps[3].rng.get_state()[1], fresh[1]) and preps[3].rng.get_state()[2] == fresh[2]


def test_test_mode_does_not_matter():
    tup, graph = _scene()
    on = _fields(datasets.ScenePrep(aug=True, test_mode=True, seed=5, with_elastic=True)(tup, graph))
    off = _fields(datasets.ScenePrep(aug=True, test_mode=True, seed=5)(tup, graph))
    assert not np.array_equal(on["loc"], off["loc"]) and np.array_equal(on["loc_float"], off["loc_float"])


@pytest.mark.parametrize("scale", [50.0, 8, 0, 12.5])
def test_a_grid_spacing_that_is_no_positive_integer_is_refused(scale):
    with pytest.raises(ValueError):
        datasets.ScenePrep(scale=scale, with_elastic=True)
    datasets.ScenePrep(scale=scale)                                  # off: as before


def test_the_smallest_scale():
    p = datasets.ScenePrep(scale=9, with_elastic=True)
    assert p.elastic_calls() == ((1, 40 * 9 / 50), (3, 160 * 9 / 50))
    assert datasets.ScenePrep(scale=np.int64(50), with_elastic=True).elastic_calls() == ((6, 40.0), (20, 160.0))
