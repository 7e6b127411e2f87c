"""CPU: the one layout rule behind the four collate functions (``wsis_datasets.assemble_batch``)
against its numpy restatement (tests/batch_ref.py), through each adapter that runs without the GPU: synthetic scene
dicts, packed scenes (views of the unpinned host buffer) and ``ScenePrep`` tuples."""
import numpy as np
import pytest
import torch

import harness
import wsis_datasets as datasets
from batch_ref import batch_ref

INT64 = ("locs", "semantic_labels", "instance_labels", "superpoint", "edge_u_list", "edge_v_list",
         "superpoint_semantic_labels", "superpoint_instance_labels")
FP32 = ("locs_float", "feats", "superpoint_offset_vector", "superpoint_instance_size")
_SCENES = {}


def _scenes():
    if not _SCENES:
        _SCENES["s"] = [harness.make_scene(s, room=(1.0, 0.9, 0.8), n_box=2) for s in (5, 6, 7)]
    return _SCENES["s"]


def _ref_scene(sc):
    """a ``make_scene`` dict as the restatement takes it: voxel coordinates = floor(xyz * 50) from the scene's minimum"""
    v = np.floor(sc["xyz"].astype(np.float64) * harness.SCALE).astype(np.int64)
    return dict(loc=v - v.min(0), loc_float=sc["xyz"], feat=sc["rgb"], sem=sc["sem_label"], ins=sc["ins_label"],
                sp=sc["superpoint"], S=sc["S"], n_inst=sc["n_inst"], sp_sem=sc["sp_sem"], sp_ins=sc["sp_ins"],
                sp_off=sc["sp_offset"], sp_vox=sc["sp_voxnum"], sp_size=sc["sp_size"], edges=sc["edges"],
                edge_feats=sc["edge_feats"])


def _from_scenes(scenes, shift=True):
    recs = [harness._scene_record(sc, i) for i, sc in enumerate(scenes)]
    return datasets.assemble_batch(recs, shift_sp_instances=shift, full_scale_min=harness.FULL_SCALE_MIN)


def _from_packs(scenes, shift=True):
    recs = [harness._packed_record(harness.pack_scene(sc, pin=False), torch.device("cpu"), i)
            for i, sc in enumerate(scenes)]
    return datasets.assemble_batch(recs, shift_sp_instances=shift, full_scale_min=harness.FULL_SCALE_MIN)


def _check(got, want):
    for keys, dtype in ((INT64, torch.int64), (FP32, torch.float32), (("offsets", "sp_batch_offsets"), torch.int32)):
        for k in keys:
            assert got[k].dtype == dtype and got[k].is_contiguous(), k
            assert torch.equal(got[k], torch.from_numpy(np.ascontiguousarray(want[k])).to(dtype)), k
    vox = got["superpoint_instance_voxel_num"]
    raw = torch.from_numpy(want["superpoint_instance_voxel_num_raw"]).float()
    assert vox.dtype == torch.float32 and torch.equal(vox, torch.log(raw))       # (the host's log, bit for bit)
    assert got["spatial_shape"].dtype == np.int64 and np.array_equal(got["spatial_shape"], want["spatial_shape"])
    assert got["edge_src_rows"] == want["edge_src_rows"]
    assert got["sp_instance_slots"] == want["sp_instance_slots"]
    gi = got["GIs"][0]
    assert gi.num_nodes == want["gi_num_nodes"]
    assert gi.get_pyg_buffers().dtype == torch.int64 and gi.get_pyg_buffers().is_contiguous()
    assert torch.equal(gi.get_pyg_buffers(), torch.from_numpy(np.ascontiguousarray(want["gi_edges"])))
    assert gi.get_buffers().dtype == torch.float32
    assert torch.equal(gi.get_buffers(), torch.from_numpy(want["gi_edgefeats"]))


def _same(a, b):
    assert set(a) == set(b)
    for k, x in a.items():
        if torch.is_tensor(x):
            assert x.dtype == b[k].dtype and torch.equal(x, b[k]), k
        elif k == "GIs":
            assert x[0].num_nodes == b[k][0].num_nodes
            assert torch.equal(x[0].get_pyg_buffers(), b[k][0].get_pyg_buffers())
            assert torch.equal(x[0].get_buffers(), b[k][0].get_buffers())
        elif k == "spatial_shape":
            assert np.array_equal(x, b[k])
        else:
            assert x == b[k], k


def _no_edges(sc):
    return dict(sc, edges=np.zeros((0, 2), dtype=np.int64), edge_feats=np.zeros((0, 13), dtype=np.float32))


def _no_labels(sc, n_inst=None):
    return dict(sc, ins_label=np.full_like(sc["ins_label"], -100), sp_ins=np.full_like(sc["sp_ins"], -100),
                n_inst=sc["n_inst"] if n_inst is None else n_inst)


def test_assemble_batch_equals_the_restatement():
    scenes = _scenes()
    got = _from_scenes(scenes)
    _check(got, batch_ref([_ref_scene(sc) for sc in scenes], True))
    assert got["scene_list"] == ["synthetic_0", "synthetic_1", "synthetic_2"]
    # more than one scene carries instances, so the shift shows: the ids of scene 1 start behind those of scene 0
    lab = got["superpoint_instance_labels"][int(got["sp_batch_offsets"][1]):int(got["sp_batch_offsets"][2])]
    assert int(lab[lab != -100].min()) >= scenes[0]["n_inst"]
    for k in ("locs_offset", "instance_info", "instance_pointnum", "is1ins_labels"):       # dataset ends only
        assert k not in got
    # the public function: this plus the voxel hash, without the slots (to_device reads them from the labels)
    full = harness.collate(scenes)
    assert set(full) == (set(got) - {"sp_instance_slots"}) | {"voxel_locs", "p2v_map", "v2p_map", "level_counts"}
    for k in INT64 + FP32:
        assert torch.equal(full[k], got[k]), k


def test_the_packed_adapter_equals_the_scene_adapter_on_the_host():
    scenes = _scenes()
    _same(_from_packs(scenes), _from_scenes(scenes))
    # the numbers a pack carries for the device ends = what a host record reads from its tensors
    for i, sc in enumerate(scenes + [_no_edges(scenes[0]), _no_labels(scenes[1])]):
        packed = harness._packed_record(harness.pack_scene(sc, pin=False), torch.device("cpu"), i)
        assert packed.extent is not None and packed.edge_src_max is not None and packed.sp_ins_max is not None
        extent, src_max, ins_max = harness._scene_record(sc, i).host_numbers()
        assert np.array_equal(packed.extent, extent) and packed.extent.dtype == np.int64
        assert (packed.edge_src_max, packed.sp_ins_max) == (src_max, ins_max)


def test_scene_prep_tuples_keep_the_raw_superpoint_instance_ids():
    """the dataset ends: no shift of the graph's instance ids (scannetv2_dataset.py:407), the slots follow the labels
    as they are emitted, a scene's superpoint count is its largest id + 1"""
    scenes = _scenes()
    prep = datasets.ScenePrep(aug=False, test_mode=True)
    tuples = [prep(*datasets.synthetic_scene_to_reference_format(sc)) for sc in scenes]
    got = datasets.assemble_batch([datasets._tuple_record(t) for t in tuples], shift_sp_instances=False,
                                  full_scale_min=128)
    ref_scenes = []
    for (name, loc, loc_offset, loc_float, feat, sem, ins, sp, g, inst_num, info, pointnum), sc in zip(tuples, scenes):
        ref_scenes.append(dict(loc=loc.numpy(), loc_float=loc_float.numpy(), feat=feat.numpy(), sem=sem.numpy(),
                               ins=ins.numpy(), sp=sp.numpy(), S=None, n_inst=inst_num, sp_sem=g.vs["semantic_label"],
                               sp_ins=g.vs["instance_label"], sp_off=g.vs["superpoint_offset_vector"],
                               sp_vox=g.vs["instance_voxel_num"], sp_size=g.vs["instance_size"], edges=g.edges,
                               edge_feats=g.f))
    _check(got, batch_ref(ref_scenes, False, s_from_max=True))
    raw = torch.from_numpy(np.concatenate([sc["sp_ins"] for sc in scenes])).long()
    assert torch.equal(got["superpoint_instance_labels"], raw)
    assert got["sp_instance_slots"] == [max(int(sc["sp_ins"].max()) + 1, 1) for sc in scenes]
    assert got["sp_instance_slots"] != _from_scenes(scenes)["sp_instance_slots"]           # (the shifted ends differ)
    for k in ("locs_offset", "instance_info", "instance_pointnum", "is1ins_labels"):
        assert k in got
    assert got["instance_pointnum"].dtype == torch.int32 and got["instance_info"].dtype == torch.float32
    assert got["scene_list"] == ["synthetic"] * 3
    full = datasets.collate_fn(tuples)
    assert torch.equal(full["superpoint_instance_labels"], raw) and "sp_instance_slots" not in full
    # the caller's tensors are not written to (the point ids are shifted out of place)
    assert torch.equal(tuples[1][6], prep(*datasets.synthetic_scene_to_reference_format(scenes[1]))[6])


def test_collate_fn_refuses_superpoint_ids_with_a_gap():
    prep = datasets.ScenePrep(aug=False, test_mode=True)
    t = list(prep(*datasets.synthetic_scene_to_reference_format(_scenes()[0])))
    t[7] = torch.where(t[7] == 3, t[7] - 1, t[7])
    with pytest.raises(ValueError):
        datasets.collate_fn([tuple(t)])


def _edge_cases():
    a, b, c = _scenes()
    return {"one_scene": [a], "no_edges_first": [_no_edges(a), b, c], "no_edges_middle": [a, _no_edges(b), c],
            "no_instance_on_any_superpoint": [a, _no_labels(b), c], "no_instances_then_instances": [_no_labels(a, 0), b]}


@pytest.mark.parametrize("case", ["one_scene", "no_edges_first", "no_edges_middle", "no_instance_on_any_superpoint",
                                  "no_instances_then_instances"])
@pytest.mark.parametrize("build", [_from_scenes, _from_packs])
def test_edge_cases_equal_the_restatement(case, build):
    scenes = _edge_cases()[case]
    got = build(scenes)
    _check(got, batch_ref([_ref_scene(sc) for sc in scenes], True))
    if case == "no_instance_on_any_superpoint":
        assert got["sp_instance_slots"][1] == 1
    if case.startswith("no_edges"):
        assert harness.pack_scene(scenes[case == "no_edges_middle"], pin=False)["edge_src_max"] == -1
    if case == "no_instances_then_instances":       # bias 0 behind the first scene: the ids of the second one are raw
        assert torch.equal(got["instance_labels"][len(scenes[0]["xyz"]):], torch.from_numpy(scenes[1]["ins_label"]))
    if case == "one_scene" and build is _from_scenes:
        # a host batch is a copy: editing it never reaches the scene's arrays
        assert got["locs_float"].data_ptr() != torch.from_numpy(scenes[0]["xyz"]).data_ptr()


def test_a_device_record_must_carry_the_host_known_numbers():
    """laying a batch out never reads the device back: extent, largest edge source and largest superpoint instance id
    of a record on the GPU come with it"""
    class OnDevice(object):
        is_cuda = True
    rec = harness._scene_record(_scenes()[0], 0)
    rec.loc = OnDevice()
    with pytest.raises(AssertionError):
        datasets.assemble_batch([rec], shift_sp_instances=True, full_scale_min=128)
    with pytest.raises(AssertionError):
        rec.host_numbers()
