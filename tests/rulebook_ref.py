"""What a tile order IS, in numpy, with no device code: the definition the device results of
csrc/rulebook.hip are compared with bit for bit.  Below it, the same for everything the build makes before the orders:
the coordinate hash's contents, the SubM and strided gather tables with their masks and output coordinates, and the
whole pyramid (``subm_table``, ``down_tables``, ``hash_contents``, ``pyramid``).

``tile_order_ref``: stable argsort of the rows by the 64-bit key

    table << 60 | (batch & batch_mask) << 56 | (morton & 0xffffff) << 32 | mask

where ``morton`` interleaves the low 8 bits of x >> block_shift, y >> block_shift, z >> block_shift (x in bit 0) and
``mask`` is the row's set of active kernel offsets (0 without one).  With a mask and at least ``SCHED_MIN`` full
32-row slices, the full slices of that locality order are then emitted by ascending 32 - popcount(OR of the slice's
masks) -- heaviest slice first, stable --, the partial last slice stays in place.  The default build has no snake band.
"""
import numpy as np

SLICE = 32
SCHED_MIN = 4


def morton24(x, y, z):
    """bit 3*i + j of the result = bit i of (x, y, z)[j], i < 8"""
    out = np.zeros(np.shape(x), dtype=np.uint64)
    for i in range(8):
        for j, v in enumerate((x, y, z)):
            out |= ((np.asarray(v, dtype=np.uint64) >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + j)
    return out


def tile_key(indices, mask, block_shift, table=0, batch_mask=0xff):
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    c = (idx[:, 1:] >> block_shift).astype(np.uint64)
    m = np.zeros(idx.shape[0], dtype=np.uint64) if mask is None else \
        (np.asarray(mask, dtype=np.int64) & 0xffffffff).astype(np.uint64)
    b = (idx[:, 0] & batch_mask).astype(np.uint64)
    return ((np.uint64(table) << np.uint64(60)) | (b << np.uint64(56)) |
            ((morton24(c[:, 0], c[:, 1], c[:, 2]) & np.uint64(0xffffff)) << np.uint64(32)) | m)


def slice_weights(order, mask):
    """32 - popcount(OR of the masks of the rows) of every full slice of ``order``"""
    n = order.shape[0] // SLICE
    m = (np.asarray(mask, dtype=np.int64) & 0xffffffff)[order[:n * SLICE]].reshape(n, SLICE)
    union = np.bitwise_or.reduce(m, axis=1)
    return np.array([32 - bin(int(u)).count("1") for u in union], dtype=np.int64)


def tile_order_ref(indices, mask, block_shift, table=0, batch_mask=0xff):
    order = np.argsort(tile_key(indices, mask, block_shift, table, batch_mask), kind="stable").astype(np.int32)
    n = order.shape[0] // SLICE
    if mask is None or n < SCHED_MIN:
        return order
    rank = np.argsort(slice_weights(order, mask), kind="stable")
    out = order.copy()
    out[:n * SLICE] = order[:n * SLICE].reshape(n, SLICE)[rank].reshape(-1)
    return out


def pack_ref(nbr, order):
    return np.asarray(nbr)[:, np.asarray(order, dtype=np.int64)]


def mask_of_nbr(nbr):
    """offset mask of every column of a gather table [K <= 32, M]: bit k = nbr[k] >= 0 (as int32, the tables' dtype)"""
    nbr = np.asarray(nbr)
    assert nbr.shape[0] <= 32
    bits = (nbr >= 0).astype(np.uint32) << np.arange(nbr.shape[0], dtype=np.uint32)[:, None]
    return np.bitwise_or.reduce(bits, axis=0).astype(np.uint32).view(np.int32) if nbr.shape[1] else \
        np.zeros(0, dtype=np.int32)


# ---- what the tables ARE (csrc/rulebook.hip, head of the file) ------------------------------------
# A pair (input row i, output row o) exists under kernel offset kappa iff, on every axis j,
#     coord_i[j] = coord_o[j] * stride[j] - pad[j] + kappa[j],   0 <= kappa[j] < k[j],   0 <= coord_o[j] < out_shape[j]
# and both rows are of the same batch item; flat offset = (kappa0 * k1 + kappa1) * k2 + kappa2.  A gather table holds,
# per flat offset and row of one side, the row of the other side or -1.  Inputs: unique coordinates inside the shape.
def _triple(v):
    return [int(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else [int(v)] * 3


def lin_keys(indices, shape):
    """linear index ((b * S0 + c0) * S1 + c1) * S2 + c2 of every row, int64"""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    return ((idx[:, 0] * int(shape[0]) + idx[:, 1]) * int(shape[1]) + idx[:, 2]) * int(shape[2]) + idx[:, 3]


def out_shape_of(shape, ksize, stride, pad):
    k, s, p = _triple(ksize), _triple(stride), _triple(pad)
    return [(int(shape[j]) + 2 * p[j] - (k[j] - 1) - 1) // s[j] + 1 for j in range(3)]


def _offsets(k):
    return [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


def _rows_of(sorted_keys, sorted_rows, query, valid):
    """row holding each queried key, -1 where ``valid`` is False or nobody holds it"""
    out = np.full(query.shape[0], -1, dtype=np.int32)
    if sorted_keys.shape[0] == 0:
        return out
    pos = np.minimum(np.searchsorted(sorted_keys, query), sorted_keys.shape[0] - 1)
    hit = valid & (sorted_keys[pos] == query)
    out[hit] = sorted_rows[pos[hit]]
    return out


def mask_bits(nbr):
    """uint32 [rows]: bit k set iff nbr[k] >= 0 and k < 32 (tables of more than 32 offsets keep the first 32)"""
    nbr = np.asarray(nbr)
    out = np.zeros(nbr.shape[1], dtype=np.uint32)
    for k in range(min(nbr.shape[0], 32)):
        out |= (nbr[k] >= 0).astype(np.uint32) << np.uint32(k)
    return out


def subm_table(indices, shape, ksize, pad):
    """SubMConv3d (stride 1, output rows = input rows) -> nbr int32 [K, M], mask uint32 [M]"""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    k, p = _triple(ksize), _triple(pad)
    S = np.asarray([int(v) for v in shape], dtype=np.int64)
    keys = lin_keys(idx, S)
    by_key = np.argsort(keys, kind="stable")
    skeys, srows = keys[by_key], by_key.astype(np.int32)
    nbr = np.full((k[0] * k[1] * k[2], idx.shape[0]), -1, dtype=np.int32)
    for kf, kappa in enumerate(_offsets(k)):
        q = idx[:, 1:] - np.asarray(p) + np.asarray(kappa)            # the INPUT voxel of output row o under kappa
        inside = np.all((q >= 0) & (q < S), axis=1)
        nbr[kf] = _rows_of(skeys, srows, lin_keys(np.concatenate([idx[:, :1], q], 1), S), inside)
    return nbr, mask_bits(nbr)


def down_tables(indices, shape, ksize, stride, pad, batch_size=None):
    """SparseConv3d -> out_indices int32 [M_out, 4] (ascending linear index), out_shape, nbr_down int32 [K, M_out]
    (input row of every output row), nbr_up int32 [K, M_in] (output row of every input row), mask_down, mask_up.
    ``batch_size``: rows whose batch index is outside [0, batch_size) are not part of the build."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    k, s, p = _triple(ksize), _triple(stride), _triple(pad)
    out_shape = out_shape_of(shape, k, s, p)
    O, sa = np.asarray(out_shape, dtype=np.int64), np.asarray(s, dtype=np.int64)
    part = np.ones(idx.shape[0], dtype=bool) if batch_size is None else (idx[:, 0] >= 0) & (idx[:, 0] < int(batch_size))
    K = k[0] * k[1] * k[2]
    cand_ok = np.zeros((K, idx.shape[0]), dtype=bool)
    cand_key = np.zeros((K, idx.shape[0]), dtype=np.int64)
    for kf, kappa in enumerate(_offsets(k)):
        t = idx[:, 1:] + np.asarray(p) - np.asarray(kappa)            # = coord_o * stride where a pair exists
        o = t // sa
        cand_ok[kf] = part & np.all((t >= 0) & (t % sa == 0) & (o < O), axis=1)
        cand_key[kf] = lin_keys(np.concatenate([idx[:, :1], o], 1), O)
    out_keys = np.unique(cand_key[cand_ok])
    M_out = out_keys.shape[0]
    out_indices = np.zeros((M_out, 4), dtype=np.int32)
    rest = out_keys.copy()
    for j in (2, 1, 0):
        out_indices[:, j + 1] = rest % O[j]
        rest = rest // O[j]
    out_indices[:, 0] = rest
    nbr_up = np.full((K, idx.shape[0]), -1, dtype=np.int32)
    nbr_down = np.full((K, M_out), -1, dtype=np.int32)
    rows = np.arange(idx.shape[0], dtype=np.int32)
    for kf in range(K):
        nbr_up[kf] = _rows_of(out_keys, np.arange(M_out, dtype=np.int32), cand_key[kf], cand_ok[kf])
        got = nbr_up[kf] >= 0
        assert np.unique(nbr_up[kf][got]).shape[0] == int(got.sum()), "duplicate input coordinates"
        nbr_down[kf, nbr_up[kf][got]] = rows[got]
    return out_indices, out_shape, nbr_down, nbr_up, mask_bits(nbr_down), mask_bits(nbr_up)


def hash_contents(indices, shape):
    """what the coordinate hash of these rows must hold: (keys ascending int64 [M], the row of each key int32 [M])"""
    keys = lin_keys(indices, shape)
    by_key = np.argsort(keys, kind="stable")
    return keys[by_key], by_key.astype(np.int32)


def pow2_cap(m):
    """slots of the hash of m rows (csrc/rulebook.hip pow2_cap, spconv.ops._pow2_cap)"""
    cap = 16
    while cap < 2 * m:
        cap <<= 1
    return cap


def pyramid(indices0, shape, n_levels, batch_size, block_shift):
    """The arena of wsis_rulebook_pyramid: SubM k3 p1 per level, k2 s2 p0 between levels.  -> list over the levels of
    dicts: ``indices`` int32 [M, 4], ``shape``, ``subm_nbr`` / ``subm_mask`` / ``subm_order`` / ``subm_nbr_p`` and, above
    the last level, ``down_*`` (rows of the level below) / ``up_*`` (rows of this level) the same way, ``count``."""
    levels = []
    idx, shp, table = np.asarray(indices0, dtype=np.int32).reshape(-1, 4), [int(v) for v in shape], 0

    def ordered(lv, name, coords, nbr, mask):
        nonlocal table
        order = tile_order_ref(coords, mask.view(np.int32), block_shift, table=table, batch_mask=0xf)
        table += 1
        lv[name + "_nbr"], lv[name + "_mask"], lv[name + "_order"], lv[name + "_nbr_p"] = nbr, mask, order, \
            pack_ref(nbr, order)

    for l in range(int(n_levels)):
        lv = {"indices": idx, "shape": list(shp)}
        ordered(lv, "subm", idx, *subm_table(idx, shp, 3, 1))
        if l + 1 < int(n_levels):
            out_idx, out_shape, nbr_down, nbr_up, mask_down, mask_up = down_tables(idx, shp, 2, 2, 0, batch_size)
            lv["count"] = out_idx.shape[0]
            ordered(lv, "down", out_idx, nbr_down, mask_down)
            ordered(lv, "up", idx, nbr_up, mask_up)
            idx, shp = out_idx, out_shape
        levels.append(lv)
    return levels


# ---- the hash function, restated ONLY to choose inputs and to show that a case reaches its branch -------------------
_M64 = (1 << 64) - 1


def mix64(x):
    x = int(x) & _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


def home_slot(key, cap):
    """first slot probed for ``key`` in a table of ``cap`` slots (a power of two); probing goes on at slot + 1 mod cap"""
    return mix64(key) & (int(cap) - 1)


def occupied_slots(keys, cap):
    """slots that hold a key after all of ``keys`` went in (open addressing with linear probing: the SET of occupied
    slots does not depend on the order of insertion, which key sits where does)"""
    taken = set()
    for key in keys:
        h = home_slot(key, cap)
        while h in taken:
            h = (h + 1) & (cap - 1)
        taken.add(h)
    return taken
