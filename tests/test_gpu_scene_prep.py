"""Per-scene preparation on the device (``wsis_datasets.DeviceScenePrep``, csrc/sceneprep.hip) against the reference's own
``__getitem__`` outputs (tests/golden/dataset_golden.npz, written by make_dataset_golden.py from scannetv2_dataset.py:96-190
and s3dis_dataset.py), against the host class ``ScenePrep`` beyond the fixture, and the kernels' edges against numpy.

Field rules, everywhere: integers, ``loc_float`` (after the cast to fp32 ``collate_fn`` applies), ``feat``, the graph
and ``inst_info[:, 3:9]`` (min / max) are EQUAL; ``inst_info[:, 0:3]`` (the mean) is within one fp32 step: the fp64 sum
is taken in another order than numpy's, its reordering error n * 2^-53 * sum|x| is far below half an fp32 ulp, so the two
roundings to fp32 differ by at most one step."""
import ctypes
import os

import numpy as np
import pytest
import torch

import harness
import wsis_datasets as datasets
import wsis_native as _n

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_golden.npz"))
ROOM = dict(room=(1.0, 0.9, 0.8), n_box=2)

_SCENES = {}


def _scene(seed=5):
    """the fixture scene (20,031 points for seed 5) in the reference's on-disk form; built once per seed, never modified"""
    if seed not in _SCENES:
        sc = harness.make_scene(seed, **ROOM)
        _SCENES[seed] = datasets.synthetic_scene_to_reference_format(sc)
    return _SCENES[seed]


class _CountingRng(object):
    """a RandomState that counts the ``rand(3)`` draws: one per round of ``crop``"""

    def __init__(self, rng):
        self._rng, self.rounds = rng, 0

    def rand(self, *shape):
        self.rounds += shape == (3,)
        return self._rng.rand(*shape)

    def __getattr__(self, name):
        return getattr(self._rng, name)


class _Spy(datasets.ScenePrep):
    """the host class, remembering the coordinates it truncates to ``loc`` and counting its crop rounds"""
    pre = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rng = _CountingRng(self.rng)

    def data_aug_with_graph(self, xyz, graph, *a):
        mid = super().data_aug_with_graph(xyz, graph, *a)
        s = mid * self.scale
        self.pre = s - s.min(0)
        return mid

    def crop(self, xyz):
        out, valid = super().crop(xyz)
        self.pre = out[valid]
        return out, valid

    def crop_v2(self, xyz):
        out, valid = super().crop_v2(xyz)
        self.pre = out[valid]
        return out, valid


def _one_step(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    inf = np.float32(np.inf)
    return (got == want) | (got == np.nextafter(want, inf)) | (got == np.nextafter(want, -inf))


def _want_of_host(item):
    scene, loc, loc_offset, loc_float, feat, sem, ins, sp, g, inst_num, info, pointnum = item
    return dict(loc=loc.numpy(), loc_offset=loc_offset.numpy(), loc_float=loc_float.numpy(), feat=feat.numpy(),
                sem=sem.numpy(), ins=ins.numpy(), sp=sp.numpy(), inst_num=inst_num, inst_info=info.numpy(),
                inst_pointnum=np.asarray(pointnum), g_v=g.vs["v"], g_edges=g.edges,
                g_off=g.vs["superpoint_offset_vector"], g_f=g.f, g_is1ins=g.is1ins,
                g_sem=g.vs["semantic_label"], g_ins=g.vs["instance_label"])


def _want_of_golden(tag):
    keys = ("loc", "loc_offset", "loc_float", "sem", "ins", "sp", "inst_num", "inst_info", "inst_pointnum", "g_v",
            "g_edges", "g_off")
    return {k: G[f"{tag}_{k}"] for k in keys if f"{tag}_{k}" in G.files}


def _compare(item, want, what):
    scene, loc, loc_offset, loc_float, feat, sem, ins, sp, g, inst_num, info, pointnum = item
    eq = np.testing.assert_array_equal
    eq(loc.numpy(), want["loc"], what + " loc")
    eq(loc_offset.numpy(), want["loc_offset"], what + " loc_offset")
    assert loc_float.dtype == torch.float32 and feat.dtype == torch.float32
    eq(loc_float.numpy(), np.asarray(want["loc_float"]).astype(np.float32), what + " loc_float")
    eq(sem.numpy(), np.asarray(want["sem"]).astype(np.int64), what + " sem")
    eq(ins.numpy(), np.asarray(want["ins"]).astype(np.int64), what + " ins")
    eq(sp.numpy(), want["sp"], what + " sp")
    assert inst_num == int(want["inst_num"]), what
    if "inst_pointnum" in want:
        eq(np.asarray(pointnum, dtype=np.int64), np.asarray(want["inst_pointnum"], dtype=np.int64), what + " pointnum")
    got_info, want_info = info.numpy(), np.asarray(want["inst_info"])
    assert got_info.dtype == np.float32 and got_info.shape == want_info.shape
    eq(got_info[:, 3:9], want_info[:, 3:9], what + " inst_info min/max")
    differ = int((got_info[:, 0:3] != want_info[:, 0:3]).sum())
    print(f"{what}: {differ} of {got_info[:, 0:3].size} instance-mean elements differ from the reference at all")
    assert _one_step(got_info[:, 0:3], want_info[:, 0:3]).all(), what + " inst_info mean"
    eq(g.vs["v"], want["g_v"], what + " g_v")
    eq(g.edges, want["g_edges"], what + " g_edges")
    eq(g.vs["superpoint_offset_vector"], want["g_off"], what + " g_off")
    for k, field in (("g_f", g.f), ("g_is1ins", g.is1ins), ("g_sem", g.vs["semantic_label"]),
                     ("g_ins", g.vs["instance_label"]), ("feat", feat.numpy())):
        if k in want:
            eq(field, want[k], what + " " + k)


def _no_last_bit_question(pre):
    """a coordinate within 1e-9 of an integer, but not on it, could truncate differently for a last-bit difference"""
    d = np.abs(pre - np.round(pre))
    assert not ((d > 0) & (d < 1e-9)).any()
    return float(d[d > 0].min()) if (d > 0).any() else 0.0


def _pair(cfg, **kw):
    """host spy and device class with equal constructor arguments"""
    return _Spy(**cfg, **kw), datasets.DeviceScenePrep(**cfg, device=DEV, **kw)


# ---- 1, 2: the reference's own outputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["t", "c", "e"])
def test_scannet_item_matches_reference_getitem(tag):
    aug, test_mode, max_npoint, seed = [int(x) for x in G[tag + "_cfg"]]
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=max_npoint, aug=bool(aug), test_mode=bool(test_mode), seed=seed))
    host_item = host(tup, graph)
    print(f"{tag}: smallest distance of a pre-truncation coordinate to an integer {_no_last_bit_question(host.pre):.3g}")
    res = dev.upload(tup, graph)
    item = dev(res).to_host()
    print(f"{tag}: {dev.last_stats}")
    _compare(item, _want_of_golden(tag), tag)
    np.testing.assert_array_equal(item[4].numpy(), host_item[4].numpy(), tag + " feat")
    # read-backs: the bounds, the final counts, one per crop round
    assert dev.last_stats["readbacks"] == 2 + host.rng.rounds and (host.rng.rounds >= 14) == (tag == "c")


@pytest.mark.parametrize("tag", ["s3a", "s3b", "s3c"])
def test_s3dis_item_matches_reference_getitem(tag):
    sub, max_npoint, seed = [int(x) for x in G[tag + "_cfg"]]
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=max_npoint, aug=True, test_mode=False, seed=seed, crop_version=2,
                           subsample_train=bool(sub)))
    host_item = host(tup, graph)
    _no_last_bit_question(host.pre)
    item = dev(dev.upload(tup, graph)).to_host()
    _compare(item, _want_of_golden(tag), tag)
    np.testing.assert_array_equal(item[4].numpy(), host_item[4].numpy(), tag + " feat")
    assert item[1].shape[0] <= max_npoint


# ---- 3: the host class beyond the fixture -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed,version,sub,max_npoint", [(31, 1, False, 12000), (32, 2, True, 3000), (33, 2, False, 8000)])
def test_further_seeds_equal_the_host_class(seed, version, sub, max_npoint):
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=max_npoint, aug=True, seed=seed, crop_version=version, subsample_train=sub))
    want = _want_of_host(host(tup, graph))
    _no_last_bit_question(host.pre)
    _compare(dev(dev.upload(tup, graph)).to_host(), want, f"seed {seed}")


def test_a_crop_that_loses_superpoints_and_instances():
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=9000, aug=True, seed=45))
    want = _want_of_host(host(tup, graph))
    _no_last_bit_question(host.pre)
    prepared = dev(dev.upload(tup, graph))
    ids_before = np.unique(tup[3][tup[3] >= 0])
    assert prepared.S < graph.vcount and len(want["g_v"]) < graph.vcount            # a superpoint vanished
    assert 0 < prepared.inst_num < len(ids_before)                                   # an instance id vanished
    assert 0 < prepared.n <= 9000
    _compare(prepared.to_host(), want, "lossy crop")


def test_a_crop_that_keeps_nothing():
    """the reference's crop shrinks its window until at most max_npoint points are left: that can be none"""
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=7000, aug=True, seed=40))
    want = _want_of_host(host(tup, graph))
    prepared = dev(dev.upload(tup, graph))
    assert prepared.n == 0 and prepared.S == 0 and prepared.E == 0 and prepared.inst_num == 0
    _compare(prepared.to_host(), want, "empty crop")


def test_two_calls_on_one_resident_scene_follow_the_host_streams():
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=9000, aug=True, seed=41))
    res = dev.upload(tup, graph)
    before = {k: getattr(res, k).clone() for k in ("xyz", "rgb", "sem", "ins", "sp", "edges", "f", "is1ins")}
    before_vs = {k: t.clone() for k, t in res.vs.items()}
    for call in range(2):
        want = _want_of_host(host(tup, graph))
        _compare(dev(res).to_host(), want, f"call {call}")
    for k, t in before.items():
        assert torch.equal(getattr(res, k), t), k
    for k, t in before_vs.items():
        assert torch.equal(res.vs[k], t), k


def test_update_labels_then_a_call():
    tup, graph = _scene()
    host, dev = _pair(dict(max_npoint=9000, aug=True, seed=52))
    res = dev.upload(tup, graph)
    _compare(dev(res).to_host(), _want_of_host(host(tup, graph)), "before the update")
    sem2 = (np.asarray(tup[2]) + 1) % 20
    ins2 = np.where(np.asarray(tup[3]) >= 0, np.asarray(tup[3]) * 3 + 1, -100.0)     # ids with holes
    g2 = graph.copy()
    g2.vs["semantic_label"] = (g2.vs["semantic_label"] + 1) % 20
    g2.vs["instance_label"] = np.where(g2.vs["instance_label"] >= 0, g2.vs["instance_label"] * 3 + 1, -100)
    g2.vs["superpoint_offset_vector"] = g2.vs["superpoint_offset_vector"] * 0.5
    g2.is1ins = (np.arange(len(g2.edges)) % 3 - 1).astype(np.int64)
    tup2 = (tup[0], tup[1], sem2, ins2, tup[4], tup[5])
    xyz_ptr = res.xyz.data_ptr()
    dev.update_labels(res, sem2, ins2, g2)
    assert res.xyz.data_ptr() == xyz_ptr                          # the coordinates were not uploaded again
    _compare(dev(res).to_host(), _want_of_host(host(tup2, g2)), "after the update")


# ---- 5: bit reproducibility -------------------------------------------------------------------------------------------
def test_two_runs_with_equal_seeds_are_byte_identical():
    tup, graph = _scene()
    runs = []
    for _ in range(2):
        dev = datasets.DeviceScenePrep(max_npoint=7000, aug=True, seed=45, device=DEV)
        p = dev(dev.upload(tup, graph))
        runs.append([p.loc, p.loc_float, p.feat, p.sem, p.ins, p.sp, p.inst_info, p.inst_pointnum, p.edges, p.f,
                     p.is1ins] + [p.vs[k] for k in sorted(p.vs)])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


# ---- 4: the kernels' edges against numpy ------------------------------------------------------------------------------
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _d3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _state():
    st = torch.empty(int(_n.hip().wsis_sp_state_bytes()) // 8, dtype=torch.int64, device=DEV)
    _n.check(_n.hip().wsis_sp_state_init(_n.ptr(st), _n.stream_ptr()), "sp_state_init")
    return st


def _crop_mask(scaled, mn, form, a, b, st, rnd):
    mask = torch.full((len(scaled),), 7, dtype=torch.uint8, device=DEV)
    _n.check(_n.hip().wsis_sp_crop_mask(_n.ptr(_dev(scaled, np.float64)), len(scaled), _d3(mn), form, _d3(a), _d3(b),
                                        _n.ptr(mask), _n.ptr(st), rnd, _n.stream_ptr()), "sp_crop_mask")
    w = st[16 + 4 * rnd:20 + 4 * rnd].cpu().numpy()
    return mask.cpu().numpy(), int(w[0]), datasets._ordered_to_double(w[1:])


def _emit(mask, scaled, middle, mn, off, rgb, sem, ins, sp, S, K, jitter=None, n_out=None):
    """wsis_sp_emit + wsis_sp_tables + wsis_sp_relabel on host arrays -> dict of host arrays"""
    lib, n = _n.hip(), len(scaled)
    n_out = (n if mask is None else int(np.count_nonzero(mask))) if n_out is None else n_out
    st = _state()
    d_mask = None if mask is None else _dev(mask, np.uint8)
    ins_d, sp_d, sem_d = _dev(ins, np.int64), _dev(sp, np.int64), _dev(sem, np.int64)
    scaled_d, middle_d, rgb_d = _dev(scaled, np.float64), _dev(middle, np.float64), _dev(rgb, np.float32)
    o = dict(loc=torch.empty((n_out, 3), dtype=torch.int64, device=DEV),
             loc_float=torch.empty((n_out, 3), dtype=torch.float32, device=DEV),
             middle=torch.empty((n_out, 3), dtype=torch.float64, device=DEV),
             feat=torch.empty((n_out, 3), dtype=torch.float32, device=DEV),
             sem=torch.empty(n_out, dtype=torch.int64, device=DEV), ins_raw=torch.empty(n_out, dtype=torch.int64, device=DEV),
             sp_old=torch.empty(n_out, dtype=torch.int64, device=DEV))
    flags = torch.full((S + K,), 9, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.wsis_sp_emit_workspace_bytes(n, S, K))
    assert ws_bytes >= 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    jit = None if jitter is None else (ctypes.c_float * 3)(*jitter)
    _n.check(lib.wsis_sp_emit(_n.ptr(d_mask), None, n, n, n_out, _n.ptr(scaled_d), _n.ptr(middle_d), _d3(mn), _d3(off),
                              _n.ptr(rgb_d), jit, _n.ptr(sem_d), _n.ptr(ins_d), _n.ptr(sp_d), S, K, _n.ptr(o["loc"]),
                              _n.ptr(o["loc_float"]), _n.ptr(o["middle"]), _n.ptr(o["feat"]), _n.ptr(o["sem"]),
                              _n.ptr(o["ins_raw"]), _n.ptr(o["sp_old"]), _n.ptr(flags), _n.ptr(st), _n.ptr(ws), ws_bytes,
                              _n.stream_ptr()), "sp_emit")
    sp_new = torch.empty(S, dtype=torch.int32, device=DEV)
    subset = torch.zeros(S, dtype=torch.int64, device=DEV)
    ins_map = torch.empty(K, dtype=torch.int32, device=DEV)
    scratch = torch.empty(2 * K, dtype=torch.int32, device=DEV)
    _n.check(lib.wsis_sp_tables(_n.ptr(flags), S, K, _n.ptr(sp_new), _n.ptr(subset), _n.ptr(ins_map), _n.ptr(scratch),
                                _n.ptr(st), _n.stream_ptr()), "sp_tables")
    o["sp"] = torch.empty(n_out, dtype=torch.int64, device=DEV)
    o["ins"] = torch.empty(n_out, dtype=torch.int64, device=DEV)
    o["seg"] = torch.empty(n_out, dtype=torch.int64, device=DEV)
    _n.check(lib.wsis_sp_relabel(_n.ptr(o["sp_old"]), _n.ptr(o["ins_raw"]), n_out, _n.ptr(sp_new), S, _n.ptr(ins_map), K,
                                 _n.ptr(o["sp"]), _n.ptr(o["ins"]), _n.ptr(o["seg"]), _n.stream_ptr()), "sp_relabel")
    out = {k: t.cpu().numpy() for k, t in o.items()}
    words = st.cpu().numpy()
    out.update(bad=int(words[6]), locmax=words[8:11].copy(), S_new=int(words[11]), k=int(words[12]),
               subset=subset.cpu().numpy()[:int(words[11])])
    return out


SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]


def _synthetic(N, seed):
    rng = np.random.RandomState(seed)
    scaled = rng.randint(-40, 600, size=(N, 3)) * 0.25             # quarter steps: every sum below is exact
    return rng, scaled


@pytest.mark.parametrize("N", SIZES)
def test_crop_masks_and_counts(N):
    rng, scaled = _synthetic(N, N)
    mn = np.array([-10.0, -10.0, -10.0])
    off = np.array([-3.0, -2.25, 0.0])
    full = np.array([128.0, 96.0, 128.0])
    scaled[0] = mn - off                                            # x + off == 0 in every column: inside
    if N > 1:
        scaled[1] = mn - off
        scaled[1, 0] += full[0]                                     # x + off == full_scale: outside
    if N > 2:
        scaled[2] = mn - off
        scaled[2, 1] -= 0.25                                        # just below zero: outside
    st = _state()
    x = scaled - mn
    want = ((x + off).min(1) >= 0) * (((x + off) < full).sum(1) == 3)
    mask, count, _ = _crop_mask(scaled, mn, 1, off, full, st, 0)
    np.testing.assert_array_equal(mask, want.astype(np.uint8))
    assert count == int(want.sum()) and mask[0] == 1 and (N < 2 or mask[1] == 0) and (N < 3 or mask[2] == 0)
    count1 = count
    lo, hi = np.array([20.0, 15.5, 0.0]), np.array([90.0, 70.25, 0.0])
    scaled[0, :2] = mn[:2] + lo[:2]                                 # on the lower edge: inside
    if N > 1:
        scaled[1, :2] = mn[:2] + hi[:2]                             # on the upper edge: inside
    x = scaled - mn
    want = (x[:, 0] >= lo[0]) & (x[:, 0] <= hi[0]) & (x[:, 1] >= lo[1]) & (x[:, 1] <= hi[1])
    mask, count, kmin = _crop_mask(scaled, mn, 2, lo, hi, st, 5)
    np.testing.assert_array_equal(mask, want.astype(np.uint8))
    assert count == int(want.sum()) and mask[0] == 1 and (N < 2 or mask[1] == 1)
    np.testing.assert_array_equal(kmin, x[want].min(0))
    assert int(st[16].item()) == count1                            # another round's slot is left alone


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["random", "ones", "single"])
def test_compaction_order_and_truncation(N, kind):
    rng, scaled = _synthetic(N, 100 + N)
    scaled = scaled + rng.randint(0, 4, size=(N, 3)) * 0.0625
    middle = rng.randn(N, 3)
    rgb = rng.rand(N, 3).astype(np.float32)
    sem, ins, sp = rng.randint(0, 20, N), rng.randint(-1, 5, N), rng.randint(0, 9, N)
    ins = np.where(ins < 0, -100, ins)
    mn, off = np.array([-10.0, -10.0, -10.0]), np.array([-30.5, -7.25, 0.0])       # negative results truncate up
    if kind == "random":
        mask = (rng.rand(N) < 0.4).astype(np.uint8)
    elif kind == "ones":
        mask = np.ones(N, np.uint8)
    else:
        mask = np.zeros(N, np.uint8)
        mask[N // 2] = 1
    jitter = [0.125, -0.25, 0.5]
    o = _emit(mask, scaled, middle, mn, off, rgb, sem, ins, sp, 9, 5, jitter)
    keep = mask.astype(bool)
    pre = (scaled - mn) + off
    assert (pre < 0).any() or N < 3
    np.testing.assert_array_equal(o["loc"], np.trunc(pre[keep]).astype(np.int64))
    np.testing.assert_array_equal(o["loc_float"], middle[keep].astype(np.float32))
    np.testing.assert_array_equal(o["middle"], middle[keep])
    np.testing.assert_array_equal(o["feat"], rgb[keep] + np.asarray(jitter, np.float32))
    np.testing.assert_array_equal(o["sem"], sem[keep])
    np.testing.assert_array_equal(o["ins_raw"], ins[keep])
    np.testing.assert_array_equal(o["sp_old"], sp[keep])
    assert o["bad"] == 0
    if keep.any():
        np.testing.assert_array_equal(o["locmax"], np.maximum(np.trunc(pre[keep]).max(0), 0).astype(np.int64))
        subset, inverse = np.unique(sp[keep], return_inverse=True)
        np.testing.assert_array_equal(o["subset"], subset)
        np.testing.assert_array_equal(o["sp"], inverse.reshape(-1))
        np.testing.assert_array_equal(o["ins"], datasets.ScenePrep.get_cropped_inst_label(ins.copy(), keep))
    if kind == "ones":                                               # the form without a mask: every point, same result
        p = _emit(None, scaled, middle, mn, off, rgb, sem, ins, sp, 9, 5, jitter)
        for k in ("loc", "loc_float", "feat", "sem", "ins", "sp"):
            np.testing.assert_array_equal(p[k], o[k])


def _relabel(ins, K=None):
    ins = np.asarray(ins).astype(np.int64)
    n = len(ins)
    K = max(int(ins.max()) + 1, 0) if K is None else K
    z3 = np.zeros((n, 3))
    return _emit(None, z3, z3, np.zeros(3), np.zeros(3), z3.astype(np.float32), np.zeros(n), ins, np.zeros(n), 1, K)


INST_CASES = {
    "leading holes": [3, 3, 5, 7, 7, 9, -100, 5],
    "hole below the maximum": [0, 1, 2, 4, 4, 0, -100],
    "all unlabelled": [-100] * 70,
    "single id": [4] * 5,
    "every second of 300 ids empty": list(np.repeat(np.arange(0, 600, 2), 3)),
    "dense already": [0, 1, 2, 3, 2, 1, 0],
}


@pytest.mark.parametrize("case", sorted(INST_CASES))
def test_instance_ids_are_recompacted_as_the_reference_walk_does(case):
    ins = np.asarray(INST_CASES[case], dtype=np.int64)
    if case.startswith("every second"):
        ins = ins[np.random.RandomState(1).permutation(len(ins))]
    want = datasets.ScenePrep.get_cropped_inst_label(ins.astype(np.float64), np.ones(len(ins), bool))
    o = _relabel(ins)
    np.testing.assert_array_equal(o["ins"], want.astype(np.int64))
    assert o["bad"] == 0 and o["k"] == len(np.unique(ins[ins >= 0]))


def test_recompaction_of_the_golden_crop():
    kept = G["inst_in"][G["crop_valid"].astype(bool)]
    o = _relabel(kept, K=max(int(G["inst_in"].max()) + 1, 0))
    np.testing.assert_array_equal(o["ins"], G["inst_cropped"].astype(np.int64))
    want = datasets.ScenePrep.get_cropped_inst_label(G["inst_in"].copy(), G["crop_valid"].astype(bool))
    np.testing.assert_array_equal(o["ins"], want.astype(np.int64))


def test_more_ids_than_the_table_holds_are_refused():
    lib = _n.hip()
    assert lib.wsis_sp_emit_workspace_bytes(10, 4, 65537) == -1
    st = _state()
    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc = lib.wsis_sp_tables(_n.ptr(t), 0, 65537, None, None, _n.ptr(t), _n.ptr(t), _n.ptr(st), _n.stream_ptr())
    assert rc == -3                                                # WSIS_ERR_OVERFLOW
    o = _relabel([0, 7, 2], K=4)                                   # an id outside the caller's table: counted, not written
    assert o["bad"] == 1


def test_instance_info_rows():
    from torch_scatter import SegmentCSR
    rng = np.random.RandomState(7)
    sizes = {0: 1, 1: 64, 2: 65, 3: 1000, 5: 3}                    # id 4 has no points
    K = 6
    ins = np.concatenate([np.full(c, i) for i, c in sizes.items()] + [np.full(10, -100)])
    ins = ins[rng.permutation(len(ins))]
    n = len(ins)
    mid = rng.randn(n, 3) * 3 + 1.5
    seg = _dev(np.where(ins < 0, K, ins), np.int64)
    csr = SegmentCSR(seg, K + 1)
    info = torch.full((n, 9), 7.0, dtype=torch.float32, device=DEV)
    pointnum = torch.full((K,), -1, dtype=torch.int32, device=DEV)
    _n.check(_n.hip().wsis_sp_instance_info(_n.ptr(_dev(mid, np.float64)), _n.ptr(csr.perm), _n.ptr(csr.offsets), n, K,
                                            _n.ptr(info), _n.ptr(pointnum), _n.stream_ptr()), "sp_instance_info")
    n_inst, want = datasets.ScenePrep.get_instance_info(mid, ins.astype(np.int32))
    assert n_inst == K
    got = info.cpu().numpy()
    np.testing.assert_array_equal(pointnum.cpu().numpy(), want["instance_pointnum"])
    assert pointnum[4].item() == 0
    np.testing.assert_array_equal(got[:, 3:9], want["instance_info"][:, 3:9])
    assert _one_step(got[:, 0:3], want["instance_info"][:, 0:3]).all()
    assert (got[ins < 0] == -100.0).all() and not (got == 7.0).any()
    again = torch.full((n, 9), 7.0, dtype=torch.float32, device=DEV)
    _n.check(_n.hip().wsis_sp_instance_info(_n.ptr(_dev(mid, np.float64)), _n.ptr(csr.perm), _n.ptr(csr.offsets), n, K,
                                            _n.ptr(again), _n.ptr(pointnum), _n.stream_ptr()), "sp_instance_info")
    assert torch.equal(again.view(torch.int32), info.view(torch.int32))


@pytest.mark.parametrize("S,ids", [(1, [0, 0, 0]), (10, [3, 8, 1, 3, 6, 6, 2, 8]), (2500, None)])
def test_superpoint_renumbering(S, ids):
    if ids is None:                                                # more ids than the scan takes in one round
        ids = np.random.RandomState(3).randint(1, S - 1, 4000)
    sp = np.asarray(ids, dtype=np.int64)
    n = len(sp)
    z3 = np.zeros((n, 3))
    o = _emit(None, z3, z3, np.zeros(3), np.zeros(3), z3.astype(np.float32), np.zeros(n), np.full(n, -100), sp, S, 0)
    subset, inverse = np.unique(sp, return_inverse=True)
    np.testing.assert_array_equal(o["subset"], subset)
    np.testing.assert_array_equal(o["sp"], inverse.reshape(-1))
    assert o["S_new"] == len(subset) and o["bad"] == 0 and o["k"] == 0
    if S > 1:
        assert 0 not in subset and S - 1 not in subset


# ---- 6: the batch -----------------------------------------------------------------------------------------------------
_BATCH = {}


def _batches():
    """host and device batch of the two cropped, augmented scenes; built once"""
    if not _BATCH:
        pairs = [_scene(5), _scene(6)]
        host = datasets.ScenePrep(max_npoint=11000, aug=True, seed=4)
        dev = datasets.DeviceScenePrep(max_npoint=11000, aug=True, seed=4, device=DEV)
        _BATCH["host"] = harness.to_device(datasets.collate_fn([host(t, g) for t, g in pairs]), DEV)
        _BATCH["dev"] = datasets.collate_prepared([dev(dev.upload(t, g)) for t, g in pairs])
        torch.cuda.synchronize()
    return _BATCH["host"], _BATCH["dev"]


def test_collate_prepared_equals_the_host_collate():
    host, dev = _batches()
    checked = 0
    for k, want in host.items():
        if not torch.is_tensor(want):
            continue
        got = dev[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        if k == "instance_info":
            assert torch.equal(got[:, 3:9].cpu(), want[:, 3:9].cpu())
            assert _one_step(got[:, 0:3].cpu().numpy(), want[:, 0:3].cpu().numpy()).all()
        else:
            assert torch.equal(got.cpu(), want.cpu()), k
        checked += 1
    assert checked >= 23
    for k in ("locs_float", "feats", "locs", "instance_info", "semantic_labels", "instance_labels", "superpoint"):
        assert dev[k].is_cuda, k
    assert np.array_equal(dev["spatial_shape"], host["spatial_shape"])
    assert list(dev["level_counts"]) == list(host["level_counts"])
    assert dev["edge_src_rows"] == host["edge_src_rows"] and dev["sp_instance_slots"] == host["sp_instance_slots"]
    assert dev["scene_list"] == host["scene_list"]
    gd, gh = dev["GIs"][0], host["GIs"][0]
    assert gd.num_nodes == gh.num_nodes
    assert torch.equal(gd._edge_indexes.cpu(), gh._edge_indexes.cpu()) and torch.equal(gd._edgefeats.cpu(), gh._edgefeats.cpu())
    for k in ("superpoint_csr", "p2v_csr"):
        assert torch.equal(dev[k].perm, host[k].perm) and torch.equal(dev[k].offsets, host[k].offsets), k


def test_a_step_on_the_prepared_batch_gives_the_same_loss_bits():
    host, dev = _batches()
    # the mean columns of instance_info are not an input of the step: the loss sees the same numbers on both batches
    cfg = harness.default_cfg()
    losses = []
    for batch in (host, dev):
        model, crit, opt = harness.build_model(cfg, DEV)
        loss, _ = harness.train_step(model, crit, opt, batch, cfg)
        losses.append(loss.cpu().numpy().tobytes())
    assert losses[0] == losses[1]
