"""What a batch IS, in numpy: the layout rule of the reference's ``collate_fn``
(modules/datasets/scannetv2_dataset.py:343-474) that ``wsis_datasets.assemble_batch`` is compared with key by key.

A scene is a dict of numpy arrays: ``loc`` [n,3], ``loc_float``, ``feat``, ``sem``, ``ins``, ``sp``, ``S``, ``n_inst``,
``sp_sem``, ``sp_ins``, ``sp_off``, ``sp_vox``, ``sp_size``, ``edges`` [E,2], ``edge_feats`` [E,13].  The two switches
are the two points in which the ends differ: ``shift_sp_instances`` (the reference leaves the graph's instance ids as
they are, :407) and ``s_from_max`` (a scene's superpoint count is its largest id + 1, :385, or the scene's own ``S``).
The voxel counts come back as they are: their log (:438) is ``torch.log`` on the host, numpy's differs in the last bit.
"""
import numpy as np


def batch_ref(scenes, shift_sp_instances, s_from_max=False, full_scale_min=128):
    cols = {k: [] for k in ("locs", "locs_float", "feats", "semantic_labels", "instance_labels", "superpoint",
                            "superpoint_semantic_labels", "superpoint_instance_labels", "superpoint_offset_vector",
                            "superpoint_instance_voxel_num_raw", "superpoint_instance_size", "edges", "gi_edges",
                            "gi_edgefeats")}
    offsets, sp_offsets, slots, inst_bias = [0], [0], [], 0
    for b, sc in enumerate(scenes):
        sp_bias = sp_offsets[-1]
        shift = lambda ids: np.where(ids != -100, ids + inst_bias, ids)                  # noqa: E731  (:389-390)
        sp_ins = shift(sc["sp_ins"]) if shift_sp_instances else sc["sp_ins"]             # :407
        cols["locs"].append(np.concatenate([np.full((len(sc["loc"]), 1), b), sc["loc"]], 1))        # :396
        for key, a in (("locs_float", sc["loc_float"]), ("feats", sc["feat"]), ("semantic_labels", sc["sem"]),
                       ("instance_labels", shift(sc["ins"])), ("superpoint", sc["sp"] + sp_bias),   # :383
                       ("superpoint_semantic_labels", sc["sp_sem"]), ("superpoint_instance_labels", sp_ins),
                       ("superpoint_offset_vector", sc["sp_off"]), ("superpoint_instance_size", sc["sp_size"]),
                       ("superpoint_instance_voxel_num_raw", sc["sp_vox"]), ("edges", sc["edges"] + sp_bias)):
            cols[key].append(a)
        order = np.argsort(sc["edges"][:, 1], kind="stable")                             # ecc/GraphConvInfo.py:54
        cols["gi_edges"].append(sc["edges"][order] + sp_bias)
        cols["gi_edgefeats"].append(sc["edge_feats"][order])
        slots.append(max(int(sp_ins.max()) + 1, 1) if len(sp_ins) else 1)
        inst_bias += sc["n_inst"]                                                        # :391
        offsets.append(offsets[-1] + len(sc["loc"]))                                     # :394
        sp_offsets.append(sp_bias + (int(sc["sp"].max()) + 1 if s_from_max else sc["S"]))    # :385-387
    out = {k: np.concatenate(v, 0) for k, v in cols.items()}
    edges = out.pop("edges")                                                             # original order, :455-457
    out.update(edge_u_list=edges[:, 0], edge_v_list=edges[:, 1], gi_edges=out["gi_edges"].T,
               edge_src_rows=int(edges[:, 0].max()) + 1 if len(edges) else 0,
               offsets=np.array(offsets, np.int32), sp_batch_offsets=np.array(sp_offsets, np.int32),
               spatial_shape=np.clip(out["locs"][:, 1:].max(0) + 1, full_scale_min, None),      # :445
               sp_instance_slots=slots, gi_num_nodes=sp_offsets[-1])
    return out
