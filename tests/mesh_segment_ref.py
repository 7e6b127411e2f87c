"""The mesh segmentation of DESIGN.md 4.17 (``wsis_graph_prep.segment_mesh``: the ScanNet "Segmentator" that
``data/ScanNetV2/prepare_data_inst_ScanNetV2.py:77`` calls, [UPSTREAM], restated from its definition) twice over:

1. ``face_normals`` .. ``segment_mesh``: steps 1-8 with plain loops, ``numpy.float32`` scalars and the operation order as
   written -- every product, sum, division and square root is one correctly rounded fp32 operation, nothing is fused.
   The device kernels and ``wsis_host_mesh_merge`` are compared with it for equality of bits and of integers.
2. ``sweeps_by_rounds``: the two sweeps without the sequential pass over the edges.  Per round an undecided edge is
   decided when no undecided edge of smaller index is admissible for either of its two components; it is accepted if it
   is admissible for both and rejected for good otherwise.  A component remembers the index of the edge that formed it:
   an edge of smaller index met an ancestor, which had refused it, so it is not admissible.  The accepted edges of a
   round touch disjoint pairs of components.  It shares no code with the sequential sweeps (labels instead of a
   union-find) and must give the same segments.
"""
import numpy as np

F32 = np.float32
K_THRESH = 0.01
SEG_MIN_VERTS = 20


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def face_normals(vertices, faces):
    """step 1 -> fp32 [F,3]; a face whose cross product has length 0 gets the normal 0"""
    p = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    out = np.zeros((len(faces), 3), F32)
    for f, (i1, i2, i3) in enumerate(faces.tolist()):
        u = [p[i2, k] - p[i1, k] for k in range(3)]
        v = [p[i3, k] - p[i1, k] for k in range(3)]
        c = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        length = np.sqrt(_dot(c, c))
        if length != 0:
            out[f] = [c[0] / length, c[1] / length, c[2] / length]
    return out


def vertex_normals(n_vertices, faces, fnormals):
    """step 2 -> fp32 [V,3]: the running mean over the incident face slots, ascending face index, then slot"""
    faces = np.asarray(faces).reshape(-1, 3)
    n = np.zeros((n_vertices, 3), F32)
    cnt = np.zeros(n_vertices, F32)
    for f, tri in enumerate(faces.tolist()):
        for v in tri:
            r = F32(1.0) / (cnt[v] + F32(1.0))
            for k in range(3):
                n[v, k] = n[v, k] + (fnormals[f, k] - n[v, k]) * r
            cnt[v] = cnt[v] + F32(1.0)
    return n


def edges_of_faces(faces):
    """step 3 -> (a, b) int32 [3F]: (i1, i2), (i1, i3), (i3, i2) at 3f, 3f + 1, 3f + 2"""
    faces = np.asarray(faces).reshape(-1, 3)
    a = np.empty(3 * len(faces), np.int32)
    b = np.empty(3 * len(faces), np.int32)
    for f, (i1, i2, i3) in enumerate(faces.tolist()):
        a[3 * f:3 * f + 3] = (i1, i1, i3)
        b[3 * f:3 * f + 3] = (i2, i3, i2)
    return a, b


def edge_weights(vertices, vnormals, a, b):
    """step 4 -> fp32 [E]"""
    p = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    w = np.empty(len(a), F32)
    for e, (va, vb) in enumerate(zip(a.tolist(), b.tolist())):
        d = [p[vb, k] - p[va, k] for k in range(3)]
        length = np.sqrt(_dot(d, d))
        d = [x / length for x in d] if length != 0 else [F32(0.0)] * 3
        dot = _dot(vnormals[va], vnormals[vb])
        dot2 = _dot(vnormals[vb], d)
        x = F32(1.0) - dot
        w[e] = x * x if dot2 > 0 else x
    return w


def sort_edges(a, b, w):
    """step 5: ascending w, ties by edge index"""
    order = np.argsort(w, kind="stable")
    return a[order], b[order], w[order]


def canonical_ids(label):
    """step 8: dense ids numbered by each segment's smallest vertex -> (int64 [V], S)"""
    ids = np.empty(len(label), np.int64)
    seen = {}
    for v, r in enumerate(np.asarray(label).tolist()):
        ids[v] = seen.setdefault(r, len(seen))
    return ids, len(seen)


def _find(parent, v):
    r = v
    while parent[r] != r:
        r = parent[r]
    while parent[v] != r:
        parent[v], v = r, parent[v]
    return r


def sweeps(a, b, w, n_vertices, k_thresh=K_THRESH, seg_min_verts=SEG_MIN_VERTS):
    """steps 6-8 over edges already in the order of step 5 -> (ids int64 [V], S)"""
    kt = F32(k_thresh)
    parent = list(range(n_vertices))
    size = [1] * n_vertices
    thr = [kt] * n_vertices
    edges = list(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    for (va, vb), we in zip(edges, np.asarray(w, dtype=F32)):
        ra, rb = _find(parent, va), _find(parent, vb)
        if ra != rb and we <= thr[ra] and we <= thr[rb]:
            parent[rb] = ra
            size[ra] += size[rb]
            thr[ra] = we + kt / F32(size[ra])
    for va, vb in edges:
        ra, rb = _find(parent, va), _find(parent, vb)
        if ra != rb and (size[ra] < seg_min_verts or size[rb] < seg_min_verts):
            parent[rb] = ra
            size[ra] += size[rb]
    return canonical_ids([_find(parent, v) for v in range(n_vertices)])


def segment_mesh(vertices, faces, k_thresh=K_THRESH, seg_min_verts=SEG_MIN_VERTS):
    """steps 1-8 -> int64 [V]"""
    vertices = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    fn = face_normals(vertices, faces)
    vn = vertex_normals(len(vertices), faces, fn)
    a, b = edges_of_faces(faces)
    return sweeps(*sort_edges(a, b, edge_weights(vertices, vn, a, b)), len(vertices), k_thresh, seg_min_verts)[0]


# ---- the second construction: rounds ---------------------------------------------------------------------------------

def _round(a, b, comp, live, admissible):
    """the edges of ``live`` decided this round -> (their positions in ``live``, accepted mask of those).  ``admissible``
    [len(live), 2]: per side of the edge"""
    ca, cb = comp[a[live]], comp[b[live]]
    big = np.iinfo(np.int64).max
    first = np.full(len(comp), big, np.int64)            # per component: its admissible undecided edge of smallest index
    np.minimum.at(first, ca[admissible[:, 0]], live[admissible[:, 0]])
    np.minimum.at(first, cb[admissible[:, 1]], live[admissible[:, 1]])
    decided = (live <= first[ca]) & (live <= first[cb])
    return decided, admissible[decided].all(1)


def sweeps_by_rounds(a, b, w, n_vertices, k_thresh=K_THRESH, seg_min_verts=SEG_MIN_VERTS):
    """steps 6-8 in rounds -> (ids int64 [V], S, rounds of sweep 1, rounds of sweep 2)"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    w = np.asarray(w, dtype=F32)
    kt = F32(k_thresh)
    comp = np.arange(n_vertices, dtype=np.int64)         # the label of a component is one of its vertices
    size = np.ones(n_vertices, np.int64)
    thr = np.full(n_vertices, kt, F32)
    formed = np.full(n_vertices, -1, np.int64)
    rounds = [0, 0]

    def join(edges):                                     # disjoint pairs of components
        keep, gone = comp[a[edges]], comp[b[edges]]
        size[keep] += size[gone]
        relabel = np.arange(n_vertices, dtype=np.int64)
        relabel[gone] = keep
        comp[:] = relabel[comp]
        return keep

    live = np.arange(len(a), dtype=np.int64)
    while len(live):
        live = live[comp[a[live]] != comp[b[live]]]      # an edge inside a component never joins anything
        if not len(live):
            break
        rounds[0] += 1
        sides = np.stack([comp[a[live]], comp[b[live]]], 1)
        admissible = (w[live][:, None] <= thr[sides]) & (live[:, None] > formed[sides])
        decided, accepted = _round(a, b, comp, live, admissible)
        edges = live[decided][accepted]
        keep = join(edges)
        thr[keep] = w[edges] + kt / size[keep].astype(F32)
        formed[keep] = edges
        live = live[~decided]

    live = np.arange(len(a), dtype=np.int64)
    while len(live):
        ca, cb = comp[a[live]], comp[b[live]]
        live = live[(ca != cb) & ((size[ca] < seg_min_verts) | (size[cb] < seg_min_verts))]     # sizes only grow
        if not len(live):
            break
        rounds[1] += 1
        decided, accepted = _round(a, b, comp, live, np.ones((len(live), 2), bool))
        assert accepted.all()
        join(live[decided])
        live = live[~decided]
    ids, S = canonical_ids(comp)
    return ids, S, rounds[0], rounds[1]


# ---- meshes of the tests ---------------------------------------------------------------------------------------------

def grid_faces(nx, ny):
    """two triangles per cell of an nx x ny vertex grid (vertex = iy * nx + ix) -> int64 [2 (nx-1) (ny-1), 3]"""
    ix, iy = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    v = (iy * nx + ix).reshape(-1)
    return np.concatenate([np.stack([v, v + 1, v + nx], 1), np.stack([v + 1, v + nx + 1, v + nx], 1)]).astype(np.int64)


def heightfield(n, seed, step=0.08, noise=0.002, cell=0.05):
    """a stepped, noisy n x n heightfield: terraces ``step`` high every n // 4 columns and a raised block in one corner
    -> (vertices fp32 [n*n,3], faces int64)"""
    rng = np.random.RandomState(seed)
    ix, iy = np.meshgrid(np.arange(n), np.arange(n))
    z = step * (ix // max(n // 4, 1)) + 3 * step * ((ix > n // 2) & (iy > n // 2))
    xyz = np.stack([ix * cell, iy * cell, z], -1).reshape(-1, 3) + rng.normal(0, noise, (n * n, 3))
    return xyz.astype(F32), grid_faces(n, n)
