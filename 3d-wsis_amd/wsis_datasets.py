"""Host side of the input contract: the reference's per-scene preparation and batch assembly for the hot path.

Mirrors ``modules/datasets/scannetv2_dataset.py`` -- ``__getitem__`` (:96-190), ``data_aug_with_graph`` (:194-209),
``elastic`` (:225-250), ``crop`` (:252-273), ``get_instance_info`` (:275-309), ``get_cropped_inst_label`` (:311-330)
and ``collate_fn`` (:343-474, schema in SURVEY App. C) -- on plain numpy arrays.  Pure host code, safe in DataLoader
workers (``pointgroup_ops.voxelization_idx`` runs in ``libwsis_host.so``).  The layout of the batch dict is written once
(``SceneRecord``, ``assemble_batch``, ``voxelize_and_count``: the same torch calls wherever the records live; also behind
``harness.collate*``).  The last part of the file is the same preparation on the device (``DeviceScenePrep``,
``collate_prepared``: csrc/sceneprep.hip) for scenes that stay resident in device memory; only that part
and batches of device records touch the GPU.

Two deliberate differences:

* randomness comes from an explicit ``numpy.random.RandomState`` (the reference uses numpy's global state; with
  ``RandomState(seed)`` the draws equal the reference's after ``np.random.seed(seed)``), and the colour jitter from
  a ``torch.Generator``;
* the superpoint graph is a :class:`PlainGraph` (arrays) instead of an ``igraph.Graph``: igraph is not in the
  image, so the ``*_spg.dat`` pickles cannot be opened here.  ``PlainGraph.from_igraph`` is the converter a
  maintainer runs where igraph exists.
"""
import math

import numpy as np
import torch

VERTEX_ATTRS = ("v", "semantic_label", "instance_label", "superpoint_offset_vector", "instance_voxel_num",
                "instance_size")


class PlainGraph(object):
    """Superpoint graph as arrays: per-vertex attributes (``prepare_data_inst_ScanNetV2.py:268-271``) and a directed
    edge list with 13 edge features ``f`` and the ``is1ins`` flag."""

    def __init__(self, vs, edges, f=None, is1ins=None):
        self.vs = {k: np.asarray(a) for k, a in vs.items()}
        self.edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        n_e = self.edges.shape[0]
        if f is None:
            self.f = np.zeros((n_e, 13), np.float32)
        else:
            f = np.asarray(f, dtype=np.float32)
            # (a graph without edges: reshape cannot infer the width of an empty array)
            self.f = f.reshape(n_e, -1) if n_e else f.reshape(0, f.shape[-1] if f.ndim == 2 else 13)
        self.is1ins = np.zeros(n_e, np.int64) if is1ins is None else np.asarray(is1ins, dtype=np.int64)

    @property
    def vcount(self):
        return len(next(iter(self.vs.values())))

    def copy(self):
        return PlainGraph({k: a.copy() for k, a in self.vs.items()}, self.edges.copy(), self.f.copy(),
                          self.is1ins.copy())

    def subgraph(self, subset):
        """Induced subgraph on the ascending vertex list ``subset`` (``superpoint_graph.subgraph(subset)``, :169):
        kept vertices are renumbered 0..len-1 in that order, edges with both ends kept stay in their order."""
        subset = np.asarray(subset, dtype=np.int64)
        new_id = np.full(self.vcount, -1, np.int64)
        new_id[subset] = np.arange(len(subset))
        e = new_id[self.edges] if len(self.edges) else self.edges
        keep = (e >= 0).all(1) if len(e) else np.zeros(0, bool)
        return PlainGraph({k: a[subset] for k, a in self.vs.items()}, e[keep], self.f[keep], self.is1ins[keep])

    @staticmethod
    def from_igraph(g):
        """Converter for a machine that has igraph (not this image): ``igraph.Graph.Read_Pickle(..._spg.dat)``."""
        vs = {k: np.asarray(g.vs[k]) for k in g.vs.attributes()}
        edges = np.asarray([e.tuple for e in g.es], dtype=np.int64).reshape(-1, 2)
        f = np.asarray(g.es["f"], dtype=np.float32) if "f" in g.es.attributes() else None
        one = np.asarray(g.es["is1ins"]) if "is1ins" in g.es.attributes() else None
        return PlainGraph(vs, edges, f, one)

    def save(self, path):
        np.savez_compressed(path, edges=self.edges, f=self.f, is1ins=self.is1ins,
                            **{"vs_" + k: a for k, a in self.vs.items()})

    @staticmethod
    def load(path):
        z = np.load(path)
        return PlainGraph({k[3:]: z[k] for k in z.files if k.startswith("vs_")}, z["edges"], z["f"], z["is1ins"])


class _PickledIGraph(object):
    """What ``igraph.Graph.__reduce__`` stores: the constructor arguments ``(n, edges, directed, graph_attrs,
    vertex_attrs, edge_attrs)`` (python-igraph 0.8 - 0.10: ``Graph.__reduce__`` returns ``(cls, (vcount, edgelist,
    is_directed, gattrs, vattrs, eattrs), __dict__)``; ``write_pickle`` is ``pickle.dump(graph)``).  Stands in for the
    class while a ``_spg.dat`` file is unpickled on a machine without igraph."""

    def __init__(self, n=0, edges=None, directed=False, graph_attrs=None, vertex_attrs=None, edge_attrs=None, *rest):
        self.n, self.edges, self.directed = int(n), list(edges or []), bool(directed)
        self.graph_attrs, self.vertex_attrs, self.edge_attrs = dict(graph_attrs or {}), dict(vertex_attrs or {}), dict(edge_attrs or {})

    def __setstate__(self, state):       # the instance __dict__ igraph appends (empty for a plain Graph)
        pass


class _SpgUnpickler(__import__("pickle").Unpickler):
    """resolves ``igraph.Graph`` (whatever sub-module the installed version defined it in) to the stand-in and lets exactly
    the globals a pickled graph with numpy attributes needs through -- an allow-list of (module, name) PAIRS, not of
    modules: ``builtins.eval`` / ``numpy.testing...runstring`` reachable through REDUCE would be code execution.
    Anything else in the stream raises ``UnpicklingError``."""

    _OK = frozenset(
        [(m, "_reconstruct") for m in ("numpy.core.multiarray", "numpy._core.multiarray")] +
        [(m, "scalar") for m in ("numpy.core.multiarray", "numpy._core.multiarray")] +
        [(m, "_frombuffer") for m in ("numpy.core.numeric", "numpy._core.numeric")] +      # (pickle protocol 5 arrays)
        [("numpy", "ndarray"), ("numpy", "dtype"), ("_codecs", "encode"), ("collections", "OrderedDict")] +
        [("builtins", n) for n in ("list", "dict", "tuple", "set", "frozenset", "int", "float", "complex", "str", "bytes",
                                   "bytearray", "bool", "slice", "range")])

    def find_class(self, module, name):
        if module.split(".")[0] == "igraph" and name == "Graph":
            return _PickledIGraph
        if (module, name) in self._OK:
            return super().find_class(module, name)
        raise __import__("pickle").UnpicklingError(f"_spg.dat: unexpected global {module}.{name}")


def read_spg_pickle(path):
    """``igraph.Graph.Read_Pickle(scene + '_spg.dat')`` (``scannetv2_dataset.py:79``) WITHOUT igraph -> PlainGraph.
    The file is the pickle ``graph.write_pickle`` wrote (``prepare_data_inst_ScanNetV2.py:88,163``; gzip-compressed
    streams are accepted like Read_Pickle does): vertex attributes ``v, semantic_label, instance_label,
    superpoint_feature, superpoint_offset_vector``, directed edge list in the prep's sorted-tuple order with edge
    attributes ``f`` (13 standardised features) and ``is1ins`` (``:268-280``)."""
    import gzip
    with open(path, "rb") as fh:
        head = fh.read(2)
    opener = gzip.open if head == b"\x1f\x8b" else open
    with opener(path, "rb") as fh:
        g = _SpgUnpickler(fh).load()
    if not isinstance(g, _PickledIGraph):
        raise ValueError(f"{path}: not an igraph.Graph pickle")
    vs = {k: np.asarray(v) for k, v in g.vertex_attrs.items()}
    for k, a in vs.items():
        if len(a) != g.n:
            raise ValueError(f"{path}: vertex attribute {k} has {len(a)} entries for {g.n} vertices")
    if not vs:
        vs = {"v": np.arange(g.n)}
    edges = np.asarray(g.edges, dtype=np.int64).reshape(-1, 2)
    f = np.asarray(g.edge_attrs["f"], dtype=np.float32).reshape(len(edges), -1) if "f" in g.edge_attrs else None
    one = np.asarray(g.edge_attrs["is1ins"]).astype(np.int64) if "is1ins" in g.edge_attrs else None
    return PlainGraph(vs, edges, f, one)


def _numpy_safe_globals():
    """The globals a ``torch.save`` of plain numpy arrays references, as (callable, path-in-the-file) pairs for
    ``torch.serialization.safe_globals``: the array reconstructor under both of its module names (files written with
    numpy 1.x say ``numpy.core.multiarray``, numpy 2 says ``numpy._core.multiarray``), ``ndarray``, ``dtype`` and the
    per-type dtype classes newer numpy pickles.  Nothing here can run code: ``_reconstruct`` / ``scalar`` build an
    array / a scalar from bytes (object dtypes are refused below)."""
    try:
        from numpy._core.multiarray import _reconstruct, scalar
    except ImportError:                                            # numpy 1.x
        from numpy.core.multiarray import _reconstruct, scalar
    out = [np.ndarray, np.dtype]
    for mod in ("numpy.core.multiarray", "numpy._core.multiarray"):
        out += [(_reconstruct, mod + "._reconstruct"), (scalar, mod + ".scalar")]
    for code in ("f2", "f4", "f8", "i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8", "b1"):
        cls = type(np.dtype(code))
        if cls is not np.dtype:
            out.append(cls)
    return out


def safe_torch_load(path, map_location="cpu"):
    """``torch.load(..., weights_only=True)`` with the numpy reconstructors allow-listed: tensors, numpy arrays of
    numeric dtype, containers, strings and numbers load; every other global in the stream (a ``REDUCE`` of
    ``os.system``, a pickled class) raises ``pickle.UnpicklingError`` before anything of the file runs.  The loader of
    the reference's own files: per-scene ``.pth`` (``scannetv2_dataset.py:62-73``) and checkpoints
    (``utils/checkpoint.py:105-135``) are files of somebody else's making."""
    with torch.serialization.safe_globals(_numpy_safe_globals()):
        return torch.load(path, map_location=map_location, weights_only=True)


def load_scene_file(path):
    """The reference's per-scene ``.pth``: ``(coords, colors, sem, inst, superpoint, scene_name)``
    (``prepare_data_inst_ScanNetV2.py:166``, read at ``scannetv2_dataset.py:62,72``).  Read with ``safe_torch_load``:
    nothing of the file is executed."""
    t = safe_torch_load(path)
    if not (isinstance(t, (tuple, list)) and len(t) == 6):
        raise ValueError(f"{path}: expected the 6-tuple (coords, colors, sem, inst, superpoint, scene)")
    coords, colors, sem, inst, superpoint, scene = t
    arrays = [np.asarray(a) for a in (coords, colors, sem, inst, superpoint)]
    for a in arrays:
        if a.dtype.hasobject:
            raise ValueError(f"{path}: object arrays are not scene data")
    return (*arrays, str(scene))


class ScenePrep(object):
    """Per-scene transform of ``ScanNetV2Inst_spg.__getitem__``.

    ``full_scale`` [128, 512], ``scale`` 50, ``max_npoint`` 250000 are the values of
    ``config/ScanNet_v2_3D_WSIS.yaml`` (read at ``scannetv2_dataset.py:36-38``)."""

    def __init__(self, full_scale=(128, 512), scale=50, max_npoint=250000, aug=True, test_mode=False, seed=None,
                 crop_version=1, subsample_train=False, with_elastic=False):
        """``crop_version=2`` / ``subsample_train=True``: the S3DIS variant (``s3dis_dataset.py``: block crop around a
        random point, :285-319, and a random quarter of the points per training item, :135-144).  ``with_elastic``
        (``param_dataset.with_elastic`` :39): the two ``elastic`` calls of PointGroup on the scaled coordinates of an
        augmented item; off, nothing changes."""
        self.with_elastic = bool(with_elastic)
        if self.with_elastic:
            for gran in (6 * scale // 50, 20 * scale // 50):
                if isinstance(gran, bool) or not isinstance(gran, (int, np.integer)) or gran < 1:
                    raise ValueError(f"with_elastic needs an integer scale of at least 9 (grid spacing {gran!r})")
        self.crop_version = int(crop_version)
        self.subsample_train = bool(subsample_train)
        self.full_scale = [int(full_scale[0]), int(full_scale[1])]
        self.scale = scale
        self.max_npoint = max_npoint
        self.aug_flag = aug
        self.test_mode = test_mode
        self.rng = np.random.RandomState(seed)
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))

    # -- :211-222 / :194-209 -------------------------------------------------------------------------------------
    def aug_matrix(self, jitter=False, flip=False, rot=False):
        m = np.eye(3)
        if jitter:
            m += self.rng.randn(3, 3) * 0.1
        if flip:
            m[0][0] *= self.rng.randint(0, 2) * 2 - 1
        if rot:
            theta = self.rng.rand() * 2 * math.pi
            m = np.matmul(m, [[math.cos(theta), math.sin(theta), 0], [-math.sin(theta), math.cos(theta), 0],
                              [0, 0, 1]])
        return m

    def data_aug(self, xyz, jitter=False, flip=False, rot=False):
        return np.matmul(xyz, self.aug_matrix(jitter, flip, rot))

    def data_aug_with_graph(self, xyz, graph, jitter=False, flip=False, rot=False):
        """The same matrix also rotates every superpoint's offset vector (the reference loops over ``graph.vs``)."""
        m = self.aug_matrix(jitter, flip, rot)
        graph.vs["superpoint_offset_vector"] = np.matmul(graph.vs["superpoint_offset_vector"], m)
        return np.matmul(xyz, m)

    # -- :225-250 ------------------------------------------------------------------------------------------------
    def elastic(self, xyz, gran, mag):
        import scipy.interpolate
        import scipy.ndimage
        bb = np.abs(xyz).max(0).astype(np.int32) // gran + 3
        noise = [self.rng.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
        for _ in range(2):
            for axis in range(3):
                shape = [1, 1, 1]
                shape[axis] = 3
                blur = np.ones(shape, "float32") / 3
                noise = [scipy.ndimage.convolve(n, blur, mode="constant", cval=0) for n in noise]
        ax = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in bb]
        interp = [scipy.interpolate.RegularGridInterpolator(ax, n, bounds_error=0, fill_value=0) for n in noise]
        return xyz + np.hstack([i(xyz)[:, None] for i in interp]) * mag

    def elastic_calls(self):
        """(gran, mag) of the two calls of PointGroup's ``__getitem__`` [UPSTREAM]; none unless switched on and augmenting"""
        if not (self.with_elastic and self.aug_flag):
            return ()
        return ((6 * self.scale // 50, 40 * self.scale / 50), (20 * self.scale // 50, 160 * self.scale / 50))

    # -- :252-273 ------------------------------------------------------------------------------------------------
    def crop(self, xyz):
        xyz_offset = xyz.copy()
        valid = xyz_offset.min(1) >= 0
        if valid.sum() != xyz.shape[0]:
            raise ValueError("crop expects coordinates already shifted to be non-negative (:151-152)")
        full_scale = np.array([self.full_scale[1]] * 3)
        room_range = xyz.max(0) - xyz.min(0)
        while valid.sum() > self.max_npoint:
            offset = np.clip(full_scale - room_range + 0.001, None, 0) * self.rng.rand(3)
            xyz_offset = xyz + offset
            valid = (xyz_offset.min(1) >= 0) * ((xyz_offset < full_scale).sum(1) == 3)
            full_scale[:2] -= 32
        return xyz_offset, valid

    # -- s3dis_dataset.py:285-319 ------------------------------------------------------------------------------------
    def crop_v2(self, xyz):
        """S3DIS rooms: an x/y block around a random point, its half-widths the largest of 20 scale steps (binary
        search) that keeps at most ``max_npoint`` points; coordinates are shifted to the block's minimum."""
        out = xyz.copy()
        if (out.min(1) >= 0).sum() != xyz.shape[0]:
            raise ValueError("crop_v2 expects coordinates already shifted to be non-negative")
        room_max = xyz.max(0)
        center = xyz[self.rng.choice(len(xyz))][:3]
        half_x, half_y = max(room_max[0] - center[0], center[0]), max(room_max[1] - center[1], center[1])
        scale = np.arange(0, 1, 0.05)

        def inside(s):
            dx, dy = half_x * s, half_y * s
            lo, hi = center - [dx, dy, 0], center + [dx, dy, 0]
            return (xyz[:, 0] >= lo[0]) & (xyz[:, 0] <= hi[0]) & (xyz[:, 1] >= lo[1]) & (xyz[:, 1] <= hi[1])

        low, high = 0, len(scale) - 1
        while low < high:
            mid = int(math.ceil((low + high) / 2))
            if inside(scale[mid]).sum() <= self.max_npoint:
                low = mid
            else:
                high = mid - 1
        keep = inside(scale[high])
        out -= xyz[keep].min(0)
        return out, keep

    # -- :311-330 ------------------------------------------------------------------------------------------------
    @staticmethod
    def get_cropped_inst_label(instance_label, valid_idxs):
        """Re-compacts the ids after a crop exactly as the reference does: walking j upward, an empty id j takes over
        the points of the current largest id."""
        instance_label = instance_label[valid_idxs]
        if instance_label.size == 0:
            return instance_label
        j = 0
        while j < instance_label.max():
            if not (instance_label == j).any():
                instance_label[instance_label == instance_label.max()] = j
            j += 1
        return instance_label

    # -- :275-309 ------------------------------------------------------------------------------------------------
    @staticmethod
    def get_instance_info(xyz, instance_label):
        info = np.ones((xyz.shape[0], 9), dtype=np.float32) * -100.0
        pointnum = []
        n_inst = int(instance_label.max()) + 1 if instance_label.size else 0
        for i in range(n_inst):
            idx = np.where(instance_label == i)[0]
            pointnum.append(idx.size)
            if idx.size == 0:      # the reference would take min() of an empty array here; ids are compact, see above
                continue
            p = xyz[idx]
            info[idx, 0:3] = p.mean(0)
            info[idx, 3:6] = p.min(0)
            info[idx, 6:9] = p.max(0)
        return n_inst, {"instance_info": info, "instance_pointnum": pointnum}

    # -- :96-190 -------------------------------------------------------------------------------------------------
    def __call__(self, scene_tuple, graph):
        """(coords, colors, sem, inst, superpoint, scene), PlainGraph -> the 12-tuple ``__getitem__`` returns."""
        xyz_origin, rgb, semantic_label, instance_label, superpoint, scene = scene_tuple
        if self.subsample_train:                         # s3dis_dataset.py:135-144, before any other draw
            pick = self.rng.choice(len(xyz_origin), size=len(xyz_origin) // 4, replace=False)
            xyz_origin, rgb = np.asarray(xyz_origin)[pick], np.asarray(rgb)[pick]
            semantic_label, instance_label = np.asarray(semantic_label)[pick], np.asarray(instance_label)[pick]
            superpoint = np.asarray(superpoint)[pick]
        graph = graph.copy()
        flag = bool(self.aug_flag)
        xyz_middle = self.data_aug_with_graph(np.asarray(xyz_origin), graph, flag, flag, flag)
        xyz = xyz_middle * self.scale
        for gran, mag in self.elastic_calls():           # voxel coordinates only: xyz_middle and the graph stay
            xyz = self.elastic(xyz, gran, mag)
        xyz_offset = xyz.min(0)
        xyz = xyz - xyz_offset
        valid = np.ones(len(xyz_middle), dtype=bool)
        if not self.test_mode:
            xyz, valid = self.crop(xyz) if self.crop_version == 1 else self.crop_v2(xyz)
        xyz_middle = xyz_middle[valid]
        xyz = xyz[valid]
        rgb = np.asarray(rgb)[valid]
        semantic_label = np.asarray(semantic_label)[valid]
        instance_label = self.get_cropped_inst_label(np.asarray(instance_label).copy(), valid)
        superpoint = np.asarray(superpoint)[valid]
        subset, new_superpoint = np.unique(superpoint, return_inverse=True)
        sub = graph.subgraph(subset)
        inst_num, infos = self.get_instance_info(xyz_middle, instance_label.astype(np.int32))
        feat = torch.from_numpy(np.ascontiguousarray(rgb))
        if self.aug_flag:
            feat = feat + torch.randn(3, generator=self.gen) * 0.1
        return (scene, torch.from_numpy(xyz).long(), torch.from_numpy(xyz_offset).long(),
                torch.from_numpy(xyz_middle), feat, torch.from_numpy(semantic_label),
                torch.from_numpy(instance_label), torch.from_numpy(new_superpoint.reshape(-1)), sub, inst_num,
                torch.from_numpy(infos["instance_info"]), infos["instance_pointnum"])


# ---- batch assembly: ONE layout rule behind the four collate functions ------------------------------
class SceneRecord(object):
    """What every input of a collate reduces to: one scene as torch tensors in their final dtypes, on any device.

    ``name``; points ``loc`` int64 [n,3], ``loc_float`` fp32 [n,3], ``feat`` fp32 [n,C], ``sem`` / ``ins`` / ``sp`` int64 [n]
    (``ins`` and ``sp`` scene-local, -100 = no instance); host ints ``S`` and ``n_inst``; superpoints ``sp_sem`` / ``sp_ins``
    int64 [S], ``sp_off`` fp32 [S,3], ``sp_size`` / ``sp_vox`` fp32 [S] (``sp_vox_is_log``: the log is taken already);
    graph ``edges`` int64 [E,2] scene-local in their original order, ``edge_feats`` fp32 [E,13].  The dataset ends add
    ``loc_offset``, ``inst_info``, ``inst_pointnum``, ``is1ins``.  ``extent`` (int64 [3], loc.max + 1), ``edge_src_max``
    (-1 without edges) and ``sp_ins_max`` (-100 without superpoints) are the numbers the layout needs on the host."""
    loc_offset = inst_info = inst_pointnum = is1ins = None
    extent = edge_src_max = sp_ins_max = None
    sp_vox_is_log = False

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def host_numbers(self):
        """(extent, edge_src_max, sp_ins_max) as carried, else read from the tensors -- host tensors only: a record on
        the device must carry them, so that laying a batch out never reads the device back"""
        if self.extent is not None and self.edge_src_max is not None and self.sp_ins_max is not None:
            return self.extent, self.edge_src_max, self.sp_ins_max
        assert not self.loc.is_cuda, "a scene record on the device must carry extent, edge_src_max and sp_ins_max"
        return ((self.loc.max(0)[0] + 1).numpy() if self.loc.shape[0] else np.zeros(3, dtype=np.int64),
                int(self.edges[:, 0].max()) if self.edges.shape[0] else -1,
                int(self.sp_ins.max()) if self.S else -100)


def instance_slots(label_maxima):
    """``sp_instance_slots``: per scene the bound of the superpoint instance ids AS THE BATCH EMITS THEM (largest label
    + 1, at least 1) -- lets the loss place the instances in fixed slots instead of torch.unique (a sync) or an [S, S]
    same-instance matrix"""
    return [max(int(m) + 1, 1) for m in label_maxima]


def assemble_batch(records, *, shift_sp_instances, full_scale_min):
    """The layout rule of ``collate_fn`` (:343-474), once: batch column, point / superpoint / instance offsets
    (:383-396), both edge orders (:455-457 and ecc/GraphConvInfo.py:54), the host-side numbers -- everything of the batch
    dict before the voxel hash, with the same torch calls on whatever device the records live on.

    ``shift_sp_instances``: the reference batches the graph's per-superpoint instance ids as they are (:407; the loss
    only compares them inside one scene), the dataset ends pass False; the synthetic-workload ends shift them per scene
    like the point ids and pass True.  ``sp_instance_slots`` follows the labels as emitted either way.

    The inputs are never written to.  A host batch is a copy of them; on the device a bias of 0 adds nothing and a
    one-scene batch is not concatenated."""
    from graphnet import GraphConvInfo
    cols = {k: [] for k in ("locs", "locs_float", "feats", "sem", "ins", "sps", "sp_sem", "sp_ins", "sp_off", "sp_vox",
                            "sp_size", "edge_sorted", "edge_feats_sorted", "edges_ext", "info", "pointnum", "is1ins")}
    batch_offsets, sp_batch_offsets, label_maxima = [0], [0], []
    sp_bias, inst_bias, edge_src_rows = 0, 0, 0
    extent = np.zeros(3, dtype=np.int64)
    for b, r in enumerate(records):
        r_extent, src_max, ins_max = r.host_numbers()

        def shifted(ids):                                          # :389-391, out of place
            return torch.where(ids != -100, ids + inst_bias, ids) if inst_bias else ids
        n = r.loc.shape[0]
        cols["locs"].append(torch.cat([torch.full((n, 1), b, dtype=torch.int64, device=r.loc.device), r.loc], 1))
        cols["locs_float"].append(r.loc_float)
        cols["feats"].append(r.feat)
        cols["sem"].append(r.sem)
        cols["ins"].append(shifted(r.ins))
        cols["sps"].append(r.sp + sp_bias if sp_bias else r.sp)
        cols["sp_sem"].append(r.sp_sem)
        cols["sp_ins"].append(shifted(r.sp_ins) if shift_sp_instances else r.sp_ins)
        cols["sp_off"].append(r.sp_off)
        cols["sp_vox"].append(r.sp_vox)
        cols["sp_size"].append(r.sp_size)
        order = torch.argsort(r.edges[:, 1], stable=True)          # ecc/GraphConvInfo.py:54-70 (sorted by target)
        Eb = r.edges + sp_bias if sp_bias else r.edges
        cols["edge_sorted"].append(Eb[order])
        cols["edge_feats_sorted"].append(r.edge_feats[order])
        cols["edges_ext"].append(Eb)                               # original (sorted-tuple) order, :455-457
        cols["info"].append(r.inst_info)
        cols["pointnum"].append(r.inst_pointnum)
        cols["is1ins"].append(r.is1ins)
        if src_max >= 0:
            edge_src_rows = max(edge_src_rows, src_max + sp_bias + 1)
        label_maxima.append(ins_max + inst_bias if shift_sp_instances and ins_max >= 0 else ins_max)
        extent = np.maximum(extent, r_extent)
        sp_bias += r.S
        inst_bias += r.n_inst
        batch_offsets.append(batch_offsets[-1] + n)
        sp_batch_offsets.append(sp_bias)
    first = records[0]

    def cat(k):
        c = cols[k]
        return (c[0] if len(c) == 1 and c[0].is_cuda else torch.cat(c, 0)).contiguous()
    edges = cat("edges_ext")
    vox = cat("sp_vox")
    if not first.sp_vox_is_log:
        # torch's CPU log, as :438 takes it -- never the device's: it differs in the last bit
        assert not vox.is_cuda, "a scene record on the device carries the log of its voxel counts"
        vox = torch.log(vox)
    out = {
        "locs": cat("locs"), "locs_float": cat("locs_float"), "feats": cat("feats"), "semantic_labels": cat("sem"),
        "instance_labels": cat("ins"), "offsets": torch.tensor(batch_offsets, dtype=torch.int32),
        "spatial_shape": np.clip(extent, full_scale_min, None), "superpoint": cat("sps"),
        "GIs": [GraphConvInfo(cat("edge_sorted").t().contiguous(), cat("edge_feats_sorted"), sp_bias)],
        "sp_batch_offsets": torch.tensor(sp_batch_offsets, dtype=torch.int32),
        "edge_u_list": edges[:, 0].contiguous(), "edge_v_list": edges[:, 1].contiguous(),
        # rows of scatter(..., edge_u): known here on the host, so the device step never has to read it back
        "edge_src_rows": edge_src_rows,
        "superpoint_semantic_labels": cat("sp_sem"), "superpoint_instance_labels": cat("sp_ins"),
        "superpoint_offset_vector": cat("sp_off"), "superpoint_instance_voxel_num": vox,
        "superpoint_instance_size": cat("sp_size"), "scene_list": [r.name for r in records],
        "sp_instance_slots": instance_slots(label_maxima),
    }
    if first.loc_offset is not None:
        out["locs_offset"] = torch.stack([r.loc_offset for r in records])
    for key, k in (("instance_info", "info"), ("instance_pointnum", "pointnum"), ("is1ins_labels", "is1ins")):
        if cols[k][0] is not None:
            out[key] = cat(k)
    return out


def voxelize_and_count(batch, n_scenes, mode, n_levels):
    """the voxel hash of ``batch["locs"]`` (:445-449) and the active voxels of the UNet's strided levels, on the host or
    on the device, wherever ``locs`` is; the device rulebook build sizes its tables from the counts instead of reading
    them back (spconv.ops.level_voxel_counts).  Device: one read-back, of the counts."""
    import pointgroup_ops
    import spconv
    voxel_locs, p2v_map, v2p_map = pointgroup_ops.voxelization_idx(batch["locs"], n_scenes, mode)
    if voxel_locs.is_cuda:
        counts = spconv.ops.level_voxel_counts_device(voxel_locs, batch["spatial_shape"], n_levels)
        counts = [int(c) for c in counts.tolist()]
    else:
        counts = spconv.ops.level_voxel_counts(voxel_locs.numpy(), batch["spatial_shape"], n_levels)
    batch.update(voxel_locs=voxel_locs, p2v_map=p2v_map, v2p_map=v2p_map, level_counts=counts)
    return batch


def _tuple_record(data):
    """``ScenePrep`` 12-tuple -> record; the scene has as many superpoints as its largest id says (:385)"""
    scene, loc, loc_offset, loc_float, feat, sem, ins, superpoint, graph, inst_num, inst_info, inst_pointnum = data
    vs = graph.vs
    return SceneRecord(
        name=scene, loc=loc.long(), loc_float=loc_float.to(torch.float32), feat=feat.to(torch.float32), sem=sem.long(),
        ins=ins.long(), sp=superpoint.long(), S=int(superpoint.max()) + 1, n_inst=inst_num,
        sp_sem=torch.as_tensor(vs["semantic_label"]).long(), sp_ins=torch.as_tensor(vs["instance_label"]).long(),
        sp_off=torch.as_tensor(vs["superpoint_offset_vector"]).to(torch.float32),
        sp_size=torch.as_tensor(vs["instance_size"]).to(torch.float32),
        sp_vox=torch.as_tensor(vs["instance_voxel_num"]).to(torch.float32),
        edges=torch.from_numpy(graph.edges), edge_feats=torch.from_numpy(graph.f).float(),
        loc_offset=loc_offset, inst_info=inst_info.to(torch.float32),
        inst_pointnum=torch.tensor(inst_pointnum, dtype=torch.int), is1ins=torch.from_numpy(graph.is1ins))


def collate_fn(batch, full_scale_min=128, mode=4):
    """``collate_fn`` (:343-474): list of ``ScenePrep`` 12-tuples -> batch dict."""
    out = assemble_batch([_tuple_record(data) for data in batch], shift_sp_instances=False,
                         full_scale_min=full_scale_min)
    # (a host dict may still be edited: ``harness.to_device`` takes the slots from the labels it uploads)
    del out["sp_instance_slots"]
    superpoint = out["superpoint"]
    if len(np.unique(superpoint.numpy())) != int(superpoint.max()) + 1:
        raise ValueError("superpoint ids are not dense after batching (:422)")
    return voxelize_and_count(out, len(batch), mode, 5)


def synthetic_scene_to_reference_format(sc):
    """A ``harness.make_scene`` scene as the reference's on-disk pair: the 6-tuple and the superpoint graph."""
    tup = (sc["xyz"].astype(np.float32), sc["rgb"].astype(np.float32), sc["sem_label"].astype(np.float64),
           sc["ins_label"].astype(np.float64), sc["superpoint"].astype(np.int64), "synthetic")
    g = PlainGraph({"v": np.arange(sc["S"]), "semantic_label": sc["sp_sem"], "instance_label": sc["sp_ins"],
                    "superpoint_offset_vector": sc["sp_offset"].astype(np.float64),
                    "instance_voxel_num": sc["sp_voxnum"], "instance_size": sc["sp_size"]},
                   sc["edges"], sc["edge_feats"])
    return tup, g


def _segment_mode(seg, values, n_seg):
    """per-segment mode of ``values`` (ties -> the smallest value, as ``scipy.stats.mode``)"""
    vals, inv = np.unique(values, return_inverse=True)
    pair = seg.astype(np.int64) * len(vals) + inv.reshape(-1)
    up, cnt = np.unique(pair, return_counts=True)
    s, v = up // len(vals), up % len(vals)
    order = np.lexsort((v, -cnt, s))                 # segment, then count descending, then value ascending
    first = np.ones(len(order), dtype=bool)
    first[1:] = s[order][1:] != s[order][:-1]
    out = np.full(n_seg, -100, dtype=vals.dtype)
    out[s[order][first]] = vals[v[order][first]]
    return out


def acquire_weak_label(xyz, semantic_labels, instance_labels, superpoint, graph, annotation_num=1, rng=None):
    """``ScanNetV2Inst_spg.acquire_weak_label`` (scannetv2_dataset.py:970-1036): per instance, ``annotation_num``
    superpoints are drawn with probability proportional to their point count (all of them if the instance has no
    more); the drawn ones keep their labels and get the offset to the centre of the drawn points of their instance,
    every other superpoint of ``graph`` (a PlainGraph, modified in place) is reset to label -100 / offset 0.
    ``rng``: ``numpy.random.RandomState`` (the reference draws from numpy's global state: ``RandomState(seed)``
    reproduces ``np.random.seed(seed)``).  Returns the list of annotated superpoint ids in drawing order."""
    rng = rng if rng is not None else np.random.RandomState()
    superpoint = np.asarray(superpoint).astype("int")
    sp_ids, sp_size = np.unique(superpoint, return_counts=True)
    n_sp = int(sp_ids.max()) + 1 if len(sp_ids) else 0
    sp_instance = _segment_mode(superpoint, np.asarray(instance_labels), n_sp)
    members = {}                                        # instance label -> [(superpoint, size)] in ascending id order
    for sp, size in zip(sp_ids, sp_size):
        members.setdefault(sp_instance[sp], []).append((sp, size))
    chosen_all = []
    off = np.array(graph.vs["superpoint_offset_vector"], dtype=np.float64, copy=True)
    for ins in np.unique(instance_labels):
        if ins not in members:
            continue
        ids = np.array([m[0] for m in members[ins]])
        num = np.array([m[1] for m in members[ins]])
        prob = num / num.sum()
        chosen = rng.choice(ids, size=annotation_num, p=prob, replace=False) if annotation_num < ids.shape[0] else ids
        chosen_all.extend(list(chosen))
        centre = np.mean(xyz[np.isin(superpoint, chosen)], axis=0)
        for sp in chosen:
            if graph.vs["v"][sp] != sp:
                raise ValueError("graph vertex ids must equal the superpoint ids (:1018)")
            off[sp] = centre - np.mean(xyz[superpoint == sp], axis=0)
    keep = np.zeros(graph.vcount, dtype=bool)
    keep[np.asarray(chosen_all, dtype=np.int64)] = True
    graph.vs["semantic_label"] = np.where(keep, graph.vs["semantic_label"], -100)
    graph.vs["instance_label"] = np.where(keep, graph.vs["instance_label"], -100)
    off[~keep] = 0.0
    graph.vs["superpoint_offset_vector"] = off
    return [int(c) for c in chosen_all]


# ---- the same per-scene preparation on the device ------------------------------------------------------------------
_SP_STATE_WORDS, _SP_ROUNDS, _SP_ROUND0, SP_MAX_IDS = 144, 32, 16, 65536      # include/wsis_hip.h: the state block


def _ordered_to_double(keys):
    """doubles behind the ordered uint64 keys of the state block (include/wsis_hip.h): key = ~bits for a negative
    value, bits | 2^63 otherwise"""
    u = np.ascontiguousarray(keys).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    return np.where(u & top, u ^ top, ~u).astype(np.uint64).view(np.float64)


def _cuda_device(device, what):
    from wsis_native import WsisError
    dev = torch.device(device)
    if dev.type != "cuda":
        raise WsisError(f"{what} runs on the MI355X (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _as_device(a, dtype, dev, shape=None):
    if torch.is_tensor(a):
        t = a.detach().to(device=dev, dtype=dtype)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a)).astype(_NP_OF[dtype], copy=False)).to(dev)
    return (t.reshape(shape) if shape is not None else t).contiguous()


_NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64}


class ResidentScene(object):
    """One scene in device memory, uploaded once and prepared every epoch: the per-point arrays of the reference's
    ``.pth`` 6-tuple (``xyz`` fp32 [N,3], ``rgb`` fp32 [N,3], ``sem`` / ``ins`` / ``sp`` int64 [N]) and the arrays of
    its superpoint graph (every vertex attribute in its own dtype, ``edges`` int64 [E,2], ``f`` fp32 [E,13], ``is1ins``
    int64 [E]).  ``logvox``: ``torch.log`` of ``instance_voxel_num`` as the HOST takes it (``collate_fn`` :438) -- the
    device's log differs in the last bit, and a gather commutes with it.  ``n_ids``: size of the instance-id table."""

    def __init__(self, scene, device):
        self.scene, self.device = scene, device

    def _set_point_labels(self, semantic_label, instance_label):
        from wsis_native import WsisError
        self.sem = _as_device(semantic_label, torch.int64, self.device, (-1,))
        self.ins = _as_device(instance_label, torch.int64, self.device, (-1,))
        if self.sem.numel() != self.N or self.ins.numel() != self.N:
            raise ValueError(f"{self.N} points but {self.sem.numel()} / {self.ins.numel()} labels")
        self.n_ids = max(int(self.ins.max()) + 1, 0) if self.N else 0          # (at upload time, not per item)
        if self.n_ids > SP_MAX_IDS:
            raise WsisError(f"instance id {self.n_ids - 1}: the device re-compaction takes ids below {SP_MAX_IDS}")

    def _set_graph(self, graph):
        if graph.vcount != self.S:
            raise ValueError(f"the graph has {graph.vcount} vertices, the scene {self.S} superpoints")
        dev = self.device
        self.vs = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in graph.vs.items()}
        self.vs["superpoint_offset_vector"] = _as_device(graph.vs["superpoint_offset_vector"], torch.float64, dev, (-1, 3))
        self.vs_dtype = {k: np.asarray(a).dtype for k, a in graph.vs.items()}
        self.logvox = None
        if "instance_voxel_num" in graph.vs:
            self.logvox = torch.log(torch.as_tensor(np.asarray(graph.vs["instance_voxel_num"])).to(torch.float32)).to(dev)
        self.edges = _as_device(graph.edges, torch.int64, dev, (-1, 2))
        self.f = _as_device(graph.f, torch.float32, dev)
        self.is1ins = _as_device(graph.is1ins, torch.int64, dev, (-1,))
        self.E = int(self.edges.shape[0])
        if self.E and (int(self.edges.min()) < 0 or int(self.edges.max()) >= self.S):
            raise ValueError("edge endpoint outside the graph")


class PreparedScene(object):
    """What ``DeviceScenePrep.__call__`` returns: the fields of ``ScenePrep``'s 12-tuple as device tensors in the
    dtypes ``collate_fn`` ends with (``loc`` int64 [n,3], ``loc_float`` fp32, ``feat`` fp32, ``sem`` / ``ins`` / ``sp``
    int64, ``inst_info`` fp32 [n,9], ``inst_pointnum`` int32), the restricted graph (``vs``, ``edges``, ``f``,
    ``is1ins``) and the host-side counts a collate lays a batch out with."""

    def to_host(self):
        """the 12-tuple of ``ScenePrep.__call__`` with a :class:`PlainGraph` -- for the host ``collate_fn`` and for
        comparison.  The labels are int64 and ``loc_float`` fp32 (what ``collate_fn`` casts them to)."""
        vs = {k: t.cpu().numpy().astype(self.vs_dtype[k], copy=False) for k, t in self.vs.items()}
        g = PlainGraph(vs, self.edges.cpu().numpy(), self.f.cpu().numpy(), self.is1ins.cpu().numpy())
        pointnum = self.inst_pointnum.cpu().tolist()
        return (self.scene, self.loc.cpu(), self.loc_offset.clone(), self.loc_float.cpu(), self.feat.cpu(),
                self.sem.cpu(), self.ins.cpu(), self.sp.cpu(), g, self.inst_num, self.inst_info.cpu(), pointnum)


class DeviceScenePrep(ScenePrep):
    """``ScenePrep`` on the device (csrc/sceneprep.hip): same constructor arguments, same two random streams consumed
    in the same order, the per-point work as one pass per stage on a scene that stays in device memory.

    Read-backs per item: the six bounds; one count per crop round (``crop_version=2``: with the kept-point minimum, and
    one row of three doubles for the random centre); one final vector of counts; with ``with_elastic`` on an augmented
    item, the six bounds after each of the two elastic calls (the noise grids are drawn on the host from ``self.rng``,
    as the host class draws them, and uploaded in one copy per call).  ``last_stats`` holds the launches
    of this file's native entry points (the CSR build's own launches not included) and the read-backs of the last call.

    Differences from the host class: instance ids are refused above 65,536; an id outside its table is reported with
    the final counts (``WsisError``) instead of an ``IndexError`` on the spot; a scene without points is refused;
    ``crop``'s check that the shifted coordinates are non-negative is not repeated; the labels come back as int64 and
    ``loc_float`` as fp32, what ``collate_fn`` casts them to.  There is no CPU fallback."""

    def __init__(self, *args, device="cuda", **kw):
        super().__init__(*args, **kw)
        self.device = _cuda_device(device, "DeviceScenePrep")
        self.last_stats = {}

    # -- residency -------------------------------------------------------------------------------------------------
    def upload(self, scene_tuple, graph):
        xyz, rgb, semantic_label, instance_label, superpoint, scene = scene_tuple
        dev = self.device
        R = ResidentScene(scene, dev)
        with torch.cuda.device(dev):
            R.xyz = _as_device(xyz, torch.float32, dev, (-1, 3))
            R.rgb = _as_device(rgb, torch.float32, dev, (-1, 3))
            R.N, R.S = int(R.xyz.shape[0]), int(graph.vcount)
            R.sp = _as_device(superpoint, torch.int64, dev, (-1,))
            if R.rgb.shape[0] != R.N or R.sp.numel() != R.N:
                raise ValueError(f"{R.N} points but {R.rgb.shape[0]} colours / {R.sp.numel()} superpoint ids")
            if R.N and (int(R.sp.min()) < 0 or int(R.sp.max()) >= R.S):
                raise ValueError("superpoint id outside the graph")
            R._set_point_labels(semantic_label, instance_label)
            R._set_graph(graph)
        return R

    def update_labels(self, resident, semantic_label, instance_label, graph):
        """new point labels and graph arrays after a weak-label stage; coordinates, colours and superpoint ids stay"""
        with torch.cuda.device(resident.device):
            resident._set_point_labels(semantic_label, instance_label)
            resident._set_graph(graph)
        return resident

    # -- one item ----------------------------------------------------------------------------------------------------
    def __call__(self, resident):
        import ctypes
        import wsis_native as _n
        from torch_scatter import SegmentCSR
        R, dev = resident, resident.device
        lib = _n.hip()
        stats = {"launches": 0, "readbacks": 0}
        d3 = ctypes.c_double * 3

        def host3(v):
            return d3(*[float(x) for x in v])

        with torch.cuda.device(dev):
            st = _n.stream_ptr()
            pick = None
            if self.subsample_train:                     # s3dis_dataset.py:135-144, before any other draw
                pick = torch.from_numpy(self.rng.choice(R.N, size=R.N // 4, replace=False).astype(np.int64)).to(dev)
            n = R.N if pick is None else int(pick.numel())
            flag = bool(self.aug_flag)
            m = np.ascontiguousarray(self.aug_matrix(flag, flag, flag), dtype=np.float64)
            m9 = (ctypes.c_double * 9)(*m.reshape(-1).tolist())
            state = torch.empty(_SP_STATE_WORDS, dtype=torch.int64, device=dev)
            _n.check(lib.wsis_sp_state_init(_n.ptr(state), st), "sp_state_init")
            middle = torch.empty((n, 3), dtype=torch.float64, device=dev)
            scaled = torch.empty((n, 3), dtype=torch.float64, device=dev)
            _n.check(lib.wsis_sp_affine(_n.ptr(R.xyz), 0, _n.ptr(pick), R.N, n, m9, float(self.scale), _n.ptr(middle),
                                        _n.ptr(scaled), _n.ptr(state), st), "sp_affine")
            off_vec = R.vs["superpoint_offset_vector"]
            off_rot = torch.empty_like(off_vec)
            _n.check(lib.wsis_sp_affine(_n.ptr(off_vec), 1, None, R.S, R.S, m9, 1.0, _n.ptr(off_rot), None, None, st),
                     "sp_affine")
            stats["launches"] += 3
            if n == 0:
                raise ValueError("a scene without points cannot be prepared")
            bounds = _ordered_to_double(state[:6].cpu().numpy())
            stats["readbacks"] += 1
            mn, mx = bounds[:3].copy(), bounds[3:].copy()
            for gran, mag in self.elastic_calls():       # elastic :222-249 in place on `scaled`; its bounds replace mn, mx
                bb = np.maximum(np.abs(mn), np.abs(mx)).astype(np.int32) // gran + 3
                bb3 = (ctypes.c_int32 * 3)(*[int(b) for b in bb])
                noise = np.stack([self.rng.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)])
                grids = torch.from_numpy(noise).to(dev)
                tmp, el_bounds = torch.empty_like(grids), torch.empty(6, dtype=torch.int64, device=dev)
                _n.check(lib.wsis_elastic_blur(_n.ptr(grids), _n.ptr(tmp), bb3, st), "elastic_blur")
                _n.check(lib.wsis_elastic_apply(_n.ptr(scaled), n, _n.ptr(grids), bb3, int(gran), float(mag),
                                                _n.ptr(el_bounds), st), "elastic_apply")
                bounds = _ordered_to_double(el_bounds.cpu().numpy())
                stats["launches"] += 7
                stats["readbacks"] += 1
                mn, mx = bounds[:3].copy(), bounds[3:].copy()
            mask, count, off, rnd = None, n, np.zeros(3), 0

            def crop_round(form, a, b):
                nonlocal mask, rnd
                if rnd >= _SP_ROUNDS:
                    raise _n.WsisError("more crop rounds than the state block holds")
                if mask is None:
                    mask = torch.empty(n, dtype=torch.uint8, device=dev)
                _n.check(lib.wsis_sp_crop_mask(_n.ptr(scaled), n, host3(mn), form, host3(a), host3(b), _n.ptr(mask),
                                               _n.ptr(state), rnd, st), "sp_crop_mask")
                w = state[_SP_ROUND0 + 4 * rnd:_SP_ROUND0 + 4 * rnd + 4].cpu().numpy()
                stats["launches"] += 1
                stats["readbacks"] += 1
                rnd += 1
                return int(w[0]), w[1:]

            if not self.test_mode and self.crop_version == 1:           # crop :252-273
                full_scale = np.array([self.full_scale[1]] * 3)
                room_range = (mx - mn) - (mn - mn)
                while count > self.max_npoint:
                    off = np.clip(full_scale - room_range + 0.001, None, 0) * self.rng.rand(3)
                    count, _ = crop_round(1, off, full_scale.astype(np.float64))
                    full_scale[:2] -= 32
            elif not self.test_mode:                                    # crop_v2 s3dis_dataset.py:285-319
                room_max = mx - mn
                centre = scaled[self.rng.choice(n)].cpu().numpy() - mn
                stats["readbacks"] += 1
                half_x = max(room_max[0] - centre[0], centre[0])
                half_y = max(room_max[1] - centre[1], centre[1])
                steps = np.arange(0, 1, 0.05)

                def inside(s):
                    dx, dy = half_x * s, half_y * s
                    return crop_round(2, centre - [dx, dy, 0], centre + [dx, dy, 0])

                low, high = 0, len(steps) - 1
                while low < high:
                    mid = int(math.ceil((low + high) / 2))
                    if inside(steps[mid])[0] <= self.max_npoint:
                        low = mid
                    else:
                        high = mid - 1
                count, kmin = inside(steps[high])
                if count == 0:
                    raise ValueError("crop_v2 kept no point")
                off = -_ordered_to_double(kmin)
            n_out = count
            jit = None
            if self.aug_flag:
                jit = (ctypes.c_float * 3)(*(torch.randn(3, generator=self.gen) * 0.1).tolist())
            S, K = R.S, R.n_ids
            P = PreparedScene()
            P.scene, P.device, P.vs_dtype = R.scene, dev, R.vs_dtype
            P.loc = torch.empty((n_out, 3), dtype=torch.int64, device=dev)
            P.loc_float = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
            P.feat = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
            P.sem = torch.empty(n_out, dtype=torch.int64, device=dev)
            middle_kept = torch.empty((n_out, 3), dtype=torch.float64, device=dev)
            ins_raw = torch.empty(n_out, dtype=torch.int64, device=dev)
            sp_old = torch.empty(n_out, dtype=torch.int64, device=dev)
            flags = torch.empty(S + K, dtype=torch.int32, device=dev)
            ws_bytes = int(lib.wsis_sp_emit_workspace_bytes(n, S, K))
            if ws_bytes < 0:
                raise _n.WsisError("sp_emit workspace query failed")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _n.check(lib.wsis_sp_emit(_n.ptr(mask), _n.ptr(pick), R.N, n, n_out, _n.ptr(scaled), _n.ptr(middle), host3(mn),
                                      host3(off), _n.ptr(R.rgb), jit, _n.ptr(R.sem), _n.ptr(R.ins), _n.ptr(R.sp), S, K,
                                      _n.ptr(P.loc), _n.ptr(P.loc_float), _n.ptr(middle_kept), _n.ptr(P.feat),
                                      _n.ptr(P.sem), _n.ptr(ins_raw), _n.ptr(sp_old), _n.ptr(flags), _n.ptr(state),
                                      _n.ptr(ws), ws_bytes, st), "sp_emit")
            stats["launches"] += 2 + (mask is not None)
            sp_new = torch.empty(S, dtype=torch.int32, device=dev)
            subset = torch.zeros(S, dtype=torch.int64, device=dev)
            ins_map = torch.empty(K, dtype=torch.int32, device=dev)
            scratch = torch.empty(2 * K, dtype=torch.int32, device=dev)
            _n.check(lib.wsis_sp_tables(_n.ptr(flags), S, K, _n.ptr(sp_new), _n.ptr(subset), _n.ptr(ins_map),
                                        _n.ptr(scratch), _n.ptr(state), st), "sp_tables")
            P.sp = torch.empty(n_out, dtype=torch.int64, device=dev)
            P.ins = torch.empty(n_out, dtype=torch.int64, device=dev)
            seg = torch.empty(n_out, dtype=torch.int64, device=dev)
            _n.check(lib.wsis_sp_relabel(_n.ptr(sp_old), _n.ptr(ins_raw), n_out, _n.ptr(sp_new), S, _n.ptr(ins_map), K,
                                         _n.ptr(P.sp), _n.ptr(P.ins), _n.ptr(seg), st), "sp_relabel")
            csr = SegmentCSR(seg, K + 1)
            P.inst_info = torch.empty((n_out, 9), dtype=torch.float32, device=dev)
            pointnum = torch.zeros(K, dtype=torch.int32, device=dev)
            _n.check(lib.wsis_sp_instance_info(_n.ptr(middle_kept), _n.ptr(csr.perm), _n.ptr(csr.offsets), n_out, K,
                                               _n.ptr(P.inst_info), _n.ptr(pointnum), st), "sp_instance_info")
            stats["launches"] += 3
            # ---- the graph side: a few thousand vertices, ~20 k edges (subgraph(subset) :169, PlainGraph.subgraph)
            kept_v = sp_new >= 0
            keep_e = kept_v[R.edges[:, 0]] & kept_v[R.edges[:, 1]] if R.E else torch.zeros(0, dtype=torch.bool, device=dev)
            e_order = torch.argsort(~keep_e, stable=True)                # the kept edges first, in their order
            e_new = sp_new.long()[R.edges] if R.E else R.edges
            sp_ins = R.vs["instance_label"].long() if "instance_label" in R.vs else torch.full((S,), -100, device=dev)
            neg = torch.full((1,), -100, dtype=torch.int64, device=dev)
            tail = torch.stack([
                keep_e.sum(),
                (P.ins.max() + 1) if n_out else neg[0] + 100,
                torch.where(keep_e, e_new[:, 0], -1).max() if R.E else neg[0] + 99,
                torch.where(kept_v, sp_ins, neg).max() if S else neg[0]])
            counts = torch.cat([state[6:13], tail]).cpu().tolist()      # the one final vector of counts
            stats["readbacks"] += 1
            bad, locmax, S1, k_inst, E1 = counts[0], counts[2:5], counts[5], counts[6], counts[7]
            if bad:
                raise _n.WsisError(f"{bad} ids outside their tables (superpoint id >= {S}, instance id >= {K})")
            P.inst_num, P.edge_src_max, P.sp_ins_max = int(counts[8]), int(counts[9]), int(counts[10])
            P.n, P.S, P.E = n_out, int(S1), int(E1)
            P.extent = np.asarray(locmax, dtype=np.int64) + 1
            P.loc_offset = torch.from_numpy(mn.copy()).long()           # trunc toward zero (:177)
            P.inst_pointnum = pointnum[:max(P.inst_num, 0)]
            sub = subset[:P.S]
            P.vs = {k: (off_rot if k == "superpoint_offset_vector" else t)[sub] for k, t in R.vs.items()}
            P.logvox = R.logvox[sub] if R.logvox is not None else None
            eo = e_order[:P.E]
            P.edges, P.f, P.is1ins = e_new[eo], R.f[eo], R.is1ins[eo]
        self.last_stats = stats
        return P


def _prepared_record(it):
    """:class:`PreparedScene` -> record"""
    vs = it.vs
    return SceneRecord(
        name=it.scene, loc=it.loc, loc_float=it.loc_float, feat=it.feat, sem=it.sem, ins=it.ins, sp=it.sp, S=it.S,
        n_inst=it.inst_num, sp_sem=vs["semantic_label"].long(), sp_ins=vs["instance_label"].long(),
        sp_off=vs["superpoint_offset_vector"].to(torch.float32), sp_size=vs["instance_size"].to(torch.float32),
        sp_vox=it.logvox, sp_vox_is_log=True, edges=it.edges, edge_feats=it.f.float(), loc_offset=it.loc_offset,
        inst_info=it.inst_info, inst_pointnum=it.inst_pointnum, is1ins=it.is1ins,
        extent=it.extent, edge_src_max=it.edge_src_max, sp_ins_max=it.sp_ins_max)


def collate_prepared(items, mode=4, n_levels=5):
    """``collate_fn`` (:343-474) over :class:`PreparedScene` items, on the device: returns what
    ``harness.to_device(collate_fn([...]), device)`` returns, the per-point tensors never leaving the device.  The host
    thread lays the batch out from the items' counts."""
    import wsis_native as _n
    from harness import FULL_SCALE_MIN, finish_device_batch
    if not items:
        raise ValueError("empty batch")
    dev = items[0].device
    if torch.device(dev).type != "cuda":
        raise _n.WsisError("collate_prepared runs on the MI355X (there is no CPU fallback)")
    with torch.cuda.device(dev):
        out = assemble_batch([_prepared_record(it) for it in items], shift_sp_instances=False,
                             full_scale_min=FULL_SCALE_MIN)
        return finish_device_batch(voxelize_and_count(out, len(items), mode, n_levels))
