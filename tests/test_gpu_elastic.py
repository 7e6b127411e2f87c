"""Elastic distortion on the device (``wsis_elastic_blur`` / ``wsis_elastic_apply`` of csrc/sceneprep.hip,
``DeviceScenePrep(with_elastic=True)``) against the plain-numpy restatement tests/elastic_ref.py, which
tests/test_elastic_host.py holds equal to scipy and to the reference's own method.  Everything is compared with
``np.array_equal``: the kernels perform the restatement's fp64 operations in its order (no contraction, correctly
rounded division), so there is no tolerance.  Device buffers are carved out of NaN-filled ones: a read outside a grid or
a point array would show in the result, a write outside in the margin.  The items are compared with the host class
under the rule of tests/test_gpu_scene_prep.py (its ``_compare``)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import harness
import wsis_datasets as datasets
import wsis_native as _n
from tests import elastic_ref as ref
from tests.test_elastic_host import PAIRS, special_points
from tests.test_gpu_scene_prep import _compare, _one_step, _scene, _want_of_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EL_BLOCK = 256            # csrc/sceneprep.hip: cells per workgroup of a blur pass, points per workgroup of the apply
MARGIN = 64


def test_the_launch_constant_matches_the_source():
    src = open(os.path.join(ROOT, "3d-wsis_amd", "csrc", "sceneprep.hip")).read()
    assert int(re.search(r"constexpr int EL_BLOCK = (\d+);", src).group(1)) == EL_BLOCK
    assert "ceil_div(cells, EL_BLOCK)" in src and "ceil_div(n, EL_BLOCK)" in src


def _carve(a, dtype):
    """(device view holding ``a``, the NaN-filled buffer around it)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    buf = torch.full((a.size + 2 * MARGIN,), float("nan"), dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[MARGIN:MARGIN + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view, buf


def _margin_untouched(buf):
    return bool(torch.isnan(buf[:MARGIN]).all()) and bool(torch.isnan(buf[-MARGIN:]).all())


def _bb3(bb):
    return (ctypes.c_int32 * 3)(*[int(b) for b in bb])


def _blur(noise):
    """three fp32 grids of one shape -> the device's blur, fp32 [3, bb0, bb1, bb2]"""
    grids, gbuf = _carve(np.stack(noise), np.float32)
    tmp, tbuf = _carve(np.full(grids.shape, np.nan), np.float32)
    _n.check(_n.hip().wsis_elastic_blur(_n.ptr(grids), _n.ptr(tmp), _bb3(noise[0].shape), _n.stream_ptr()),
             "elastic_blur")
    out = grids.cpu().numpy()
    assert _margin_untouched(gbuf) and _margin_untouched(tbuf)
    return out


def _apply(xyz, grids, gran, mag):
    """-> (the distorted points, decoded bounds fp64 [6], raw bound keys)"""
    n = len(xyz)
    d_xyz, xbuf = _carve(np.asarray(xyz, dtype=np.float64).reshape(n, 3), np.float64)
    d_g, gbuf = _carve(np.stack(grids), np.float32)
    bounds = torch.full((6,), 0x1234, dtype=torch.int64, device=DEV)          # the call initialises them
    _n.check(_n.hip().wsis_elastic_apply(_n.ptr(d_xyz) if n else None, n, _n.ptr(d_g), _bb3(grids[0].shape), gran,
                                         float(mag), _n.ptr(bounds), _n.stream_ptr()), "elastic_apply")
    out, keys = d_xyz.cpu().numpy(), bounds.cpu().numpy()
    assert _margin_untouched(xbuf) and _margin_untouched(gbuf)
    assert np.array_equal(d_g.cpu().numpy(), np.stack(grids))                  # the grids are read only
    return out, datasets._ordered_to_double(keys), keys


_GRIDS = {}


def _grids(bb, seed=21):
    """blurred grids of shape ``bb`` from the restatement; built once, never modified"""
    key = (tuple(int(b) for b in bb), seed)
    if key not in _GRIDS:
        _GRIDS[key] = [ref.blur(g) for g in ref.draw_noise(np.random.RandomState(seed), key[0])]
    return _GRIDS[key]


# ---- blur -------------------------------------------------------------------------------------------------------------
# (3, 9, 19): 513 cells, one more than two workgroups' share; (4, 8, 8): exactly one share
@pytest.mark.parametrize("bb", [(3, 3, 3), (3, 4, 65), (65, 3, 4), (4, 8, 8), (3, 9, 19), (28, 25, 20)])
def test_blur(bb):
    assert bb != (3, 9, 19) or bb[0] * bb[1] * bb[2] == 2 * EL_BLOCK + 1
    noise = ref.draw_noise(np.random.RandomState(sum(bb)), bb)
    want = np.stack([ref.blur(g) for g in noise])
    got = _blur(noise)
    assert got.dtype == np.float32 and not np.isnan(got).any()
    assert np.array_equal(got, want)
    assert np.array_equal(_blur(noise).view(np.uint32), got.view(np.uint32))


# ---- apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gran,mag", PAIRS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, EL_BLOCK - 1, EL_BLOCK, EL_BLOCK + 1, 3 * EL_BLOCK + 7])
def test_apply_point_counts_and_bounds(N, gran, mag):
    bb = (7, 5, 4)
    grids = _grids(bb)
    a = ref.axes(bb, gran)
    rs = np.random.RandomState(N)
    xyz = np.stack([rs.uniform(a[j][0], a[j][-1], N) for j in range(3)], 1)
    want = ref.apply(xyz, grids, gran, mag)
    got, bounds, _ = _apply(xyz, grids, gran, mag)
    assert np.array_equal(got, want) and not np.array_equal(got, xyz)
    assert np.array_equal(bounds, np.concatenate([want.min(0), want.max(0)]))
    again, _, keys = _apply(xyz, grids, gran, mag)                              # two calls: identical bytes
    assert again.tobytes() == got.tobytes()
    assert np.array_equal(datasets._ordered_to_double(keys), bounds)


@pytest.mark.parametrize("gran,mag", PAIRS)
def test_apply_special_points(gran, mag):
    bb = (5, 4, 7)
    grids = _grids(bb)
    a = ref.axes(bb, gran)
    xyz = special_points(bb, gran)                # nodes, outermost nodes, corners of the grid, mid-cells; both signs
    assert (xyz < 0).any() and (xyz > 0).any()
    outside = []
    for j in range(3):                            # outside on one axis only, the other two well inside
        for v in (a[j][-1] + 0.5, a[j][0] - 1e-9, np.nextafter(a[j][-1], np.inf), np.nextafter(a[j][0], -np.inf)):
            p = [1.5, -2.5, 3.25]
            p[j] = v
            outside.append(p)
    xyz = np.concatenate([xyz, np.asarray(outside)])
    want = ref.apply(xyz, grids, gran, mag)
    got, bounds, _ = _apply(xyz, grids, gran, mag)
    assert np.array_equal(got, want)
    assert np.array_equal(got[-len(outside):], np.asarray(outside))             # displacement 0 on all three columns
    assert (got[:40] != xyz[:40]).any()
    assert np.array_equal(bounds, np.concatenate([want.min(0), want.max(0)]))


def test_apply_on_the_golden_inputs():
    G = np.load(os.path.join(ROOT, "tests", "golden", "elastic_golden.npz"))
    for k in range(int(G["n_cases"])):
        gran, mag, seed = int(G[f"cfg_{k}"][0]), float(G[f"cfg_{k}"][1]), int(G[f"cfg_{k}"][2])
        noise = ref.draw_noise(np.random.RandomState(seed), G[f"bb_{k}"])
        grids = list(_blur(noise))
        got, _, _ = _apply(G[f"in_{k}"], grids, gran, mag)
        assert np.array_equal(got, G[f"out_{k}"])                               # the reference's own output


def test_apply_without_points_leaves_the_initial_bounds():
    _, _, keys = _apply(np.zeros((0, 3)), _grids((3, 3, 3)), 6, 40.0)
    assert list(keys.view(np.uint64)) == [2 ** 64 - 1] * 3 + [0] * 3


def test_refusals():
    lib, st = _n.hip(), _n.stream_ptr()
    g = torch.zeros(3 * 27, dtype=torch.float32, device=DEV)
    t = torch.zeros(3 * 27, dtype=torch.float32, device=DEV)
    x = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    b = torch.zeros(6, dtype=torch.int64, device=DEV)
    ok3 = _bb3((3, 3, 3))
    bad_shapes = [(2, 3, 3), (3, 3, 0), (3, -1, 3), (2048, 2048, 512), (65536, 65536, 3)]

    def blur(grids, tmp, bb):
        _n.check(lib.wsis_elastic_blur(grids, tmp, bb, st), "elastic_blur")

    def apply(xyz, n, grids, bb, gran, bounds):
        _n.check(lib.wsis_elastic_apply(xyz, n, grids, bb, gran, 40.0, bounds, st), "elastic_apply")

    blur(_n.ptr(g), _n.ptr(t), ok3)                                             # the valid calls pass
    apply(_n.ptr(x), 4, _n.ptr(g), ok3, 6, _n.ptr(b))
    for args in ((None, _n.ptr(t), ok3), (_n.ptr(g), None, ok3), (_n.ptr(g), _n.ptr(t), None)):
        with pytest.raises(_n.WsisError):
            blur(*args)
    for bb in bad_shapes:
        with pytest.raises(_n.WsisError):
            blur(_n.ptr(g), _n.ptr(t), _bb3(bb))
        with pytest.raises(_n.WsisError):
            apply(_n.ptr(x), 4, _n.ptr(g), _bb3(bb), 6, _n.ptr(b))
    for args in ((None, 4, _n.ptr(g), ok3, 6, _n.ptr(b)), (_n.ptr(x), 4, None, ok3, 6, _n.ptr(b)),
                 (_n.ptr(x), 4, _n.ptr(g), None, 6, _n.ptr(b)), (_n.ptr(x), 4, _n.ptr(g), ok3, 6, None),
                 (_n.ptr(x), 2 ** 31, _n.ptr(g), ok3, 6, _n.ptr(b)), (_n.ptr(x), -1, _n.ptr(g), ok3, 6, _n.ptr(b)),
                 (_n.ptr(x), 4, _n.ptr(g), ok3, 0, _n.ptr(b)), (_n.ptr(x), 4, _n.ptr(g), ok3, -6, _n.ptr(b)),
                 (_n.ptr(x), 4, _n.ptr(g), _bb3((3, 3, 2 ** 27)), 2 ** 31 - 1, _n.ptr(b))):     # nodes beyond 2^52
        with pytest.raises(_n.WsisError):
            apply(*args)
    torch.cuda.synchronize()
    assert not x.any()                                                          # zeros stay: no refused call ran a kernel


# ---- end to end -------------------------------------------------------------------------------------------------------
def _pair(**kw):
    return (datasets.ScenePrep(with_elastic=True, **kw), datasets.DeviceScenePrep(with_elastic=True, device=DEV, **kw))


def test_scannet_item_with_several_crop_rounds():
    tup, graph = _scene()
    host, dev = _pair(max_npoint=12000, aug=True, seed=31)
    want = _want_of_host(host(tup, graph))
    prepared = dev(dev.upload(tup, graph))
    rounds = dev.last_stats["readbacks"] - 4                  # the bounds, two elastic calls, the final counts
    print(f"scannet: {dev.last_stats}, {rounds} crop rounds, {prepared.n} points kept")
    assert rounds >= 2 and 0 < prepared.n <= 12000
    _compare(prepared.to_host(), want, "elastic scannet")
    plain = _want_of_host(datasets.ScenePrep(max_npoint=12000, aug=True, seed=31)(tup, graph))
    assert plain["loc"].shape != want["loc"].shape or not np.array_equal(plain["loc"], want["loc"])


def test_s3dis_item():
    tup, graph = _scene()
    host, dev = _pair(max_npoint=3000, aug=True, seed=32, crop_version=2, subsample_train=True)
    want = _want_of_host(host(tup, graph))
    prepared = dev(dev.upload(tup, graph))
    assert 0 < prepared.n <= 3000
    _compare(prepared.to_host(), want, "elastic s3dis")


def test_two_calls_on_one_resident_scene():
    tup, graph = _scene()
    host, dev = _pair(max_npoint=12000, aug=True, seed=41)
    res = dev.upload(tup, graph)
    xyz_before = res.xyz.clone()
    for call in range(2):
        _compare(dev(res).to_host(), _want_of_host(host(tup, graph)), f"elastic call {call}")
    assert torch.equal(res.xyz, xyz_before)


def test_an_item_without_a_crop_round_and_in_test_mode():
    tup, graph = _scene()
    for test_mode in (False, True):
        host, dev = _pair(aug=True, seed=5, test_mode=test_mode)
        _compare(dev(dev.upload(tup, graph)).to_host(), _want_of_host(host(tup, graph)), f"elastic test_mode={test_mode}")
        assert dev.last_stats["readbacks"] == 4


def test_collate_prepared_equals_the_host_collate():
    pairs = [_scene(5), _scene(6)]
    host, dev = _pair(max_npoint=11000, aug=True, seed=4)
    want = harness.to_device(datasets.collate_fn([host(t, g) for t, g in pairs]), DEV)
    got = datasets.collate_prepared([dev(dev.upload(t, g)) for t, g in pairs])
    checked = 0
    for k, w in want.items():
        if not torch.is_tensor(w):
            continue
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        if k == "instance_info":
            assert torch.equal(got[k][:, 3:9].cpu(), w[:, 3:9].cpu())
            assert _one_step(got[k][:, 0:3].cpu().numpy(), w[:, 0:3].cpu().numpy()).all()
        else:
            assert torch.equal(got[k].cpu(), w.cpu()), k
        checked += 1
    assert checked >= 23
    assert np.array_equal(got["spatial_shape"], want["spatial_shape"])
    assert list(got["level_counts"]) == list(want["level_counts"])
    for k in ("superpoint_csr", "p2v_csr"):
        assert torch.equal(got[k].perm, want[k].perm) and torch.equal(got[k].offsets, want[k].offsets), k


# ---- off means off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aug", [True, False])
def test_switched_off_the_item_and_the_read_backs_are_unchanged(aug):
    tup, graph = _scene()
    kw = dict(max_npoint=12000, aug=aug, seed=31)
    today = datasets.DeviceScenePrep(device=DEV, **kw)
    off = datasets.DeviceScenePrep(device=DEV, with_elastic=not aug, **kw)      # aug=False: the flag does nothing
    a, b = today(today.upload(tup, graph)), off(off.upload(tup, graph))
    assert off.last_stats == today.last_stats
    for k in ("loc", "loc_float", "feat", "sem", "ins", "sp", "inst_info", "inst_pointnum", "edges", "f", "is1ins"):
        ta, tb = getattr(a, k), getattr(b, k)
        assert ta.dtype == tb.dtype and torch.equal(ta, tb), k
    assert torch.equal(a.loc_offset, b.loc_offset)
    _compare(b.to_host(), _want_of_host(datasets.ScenePrep(**kw)(tup, graph)), "off")
    sa, sb = today.rng.get_state(), off.rng.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
