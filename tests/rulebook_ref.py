"""What a tile order IS, in numpy, with no device code: the definition the device results of
csrc/rulebook.hip are compared with bit for bit.

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
