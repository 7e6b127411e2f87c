"""Tile orders and packed tables of csrc/rulebook.hip against their numpy definition (tests/rulebook_ref.py), bit for bit:
both C entry points of the one tile-order implementation, both pack entry points, and the Python layer
(spconv.ops.finish_tile_orders) under the switches that choose between them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rulebook_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    import wsis_native as _n
    return _n, _n.hip()


@functools.lru_cache(maxsize=None)
def _table(M, with_mask, n_batch=3, seed=0):
    """host table: indices int32 [M, 4] with coordinates in [0, 60), a random 27-bit mask or None"""
    rng = np.random.RandomState(1000 * seed + M)
    idx = np.concatenate([rng.randint(0, n_batch, (M, 1)), rng.randint(0, 60, (M, 3))], 1).astype(np.int32)
    mask = rng.randint(0, 1 << 27, M).astype(np.int32) if with_mask else None
    return idx, mask


@functools.lru_cache(maxsize=None)
def _want(M, with_mask, bs):
    idx, mask = _table(M, with_mask)
    return torch.from_numpy(R.tile_order_ref(idx, mask, bs))


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _tile_order(idx, mask, bs):
    _n, lib = _lib()
    M = idx.shape[0]
    c, m = _up(idx), _up(mask)
    ws_bytes = lib.wsis_tile_order_workspace_bytes(M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    _n.check(lib.wsis_tile_order(_ptr(c), _ptr(m), M, bs, _ptr(out), ws.data_ptr(), ws_bytes, _n.stream_ptr()),
             "tile_order")
    return out.cpu()


def _tile_order_batch(tabs, bs, batch_size):
    _n, lib = _lib()
    n = len(tabs)
    dev = [(_up(i), _up(m)) for i, m in tabs]
    Ms = [int(i.shape[0]) for i, _ in tabs]
    N = sum(Ms)
    ws_bytes = lib.wsis_tile_order_batch_workspace_bytes(N)
    assert ws_bytes == lib.wsis_tile_order_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    _n.check(lib.wsis_tile_order_batch(n, (ctypes.c_void_p * n)(*[_ptr(c) for c, _ in dev]),
                                       (ctypes.c_void_p * n)(*[_ptr(m) for _, m in dev]), (ctypes.c_int64 * n)(*Ms), bs,
                                       batch_size, _ptr(out), ws.data_ptr(), ws_bytes, _n.stream_ptr()),
             "tile_order_batch")
    return out.cpu(), Ms


@pytest.mark.parametrize("bs", [0, 4])
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("M", [1, 31, 32, 127, 128, 129, 700])
def test_one_table_equals_the_reference(M, with_mask, bs):
    """wsis_tile_order and wsis_tile_order_batch with n = 1: no full slice, below / at / above the 4 full slices where
    the slice schedule starts, a partial last slice, several blocks of every launch"""
    idx, mask = _table(M, with_mask)
    want = _want(M, with_mask, bs)
    assert torch.equal(_tile_order(idx, mask, bs), want)
    got, _ = _tile_order_batch([(idx, mask)], bs, 3)
    assert torch.equal(got, want)


def test_slices_of_equal_weight_keep_the_locality_order():
    idx, _ = _table(256, False)
    mask = np.full(256, 0b10110, dtype=np.int32)
    want = torch.from_numpy(R.tile_order_ref(idx, mask, 4))
    assert torch.equal(want, torch.from_numpy(np.argsort(R.tile_key(idx, mask, 4), kind="stable").astype(np.int32)))
    assert torch.equal(_tile_order(idx, mask, 4), want)
    assert torch.equal(_tile_order_batch([(idx, mask)], 4, 3)[0], want)


def test_one_table_keeps_eight_bits_of_the_batch_index():
    """batch indices 0..16 in one table: batch 16 sorts behind batch 15 (a 4-bit field would fold it onto batch 0)"""
    idx, mask = _table(17 * 8, True)
    idx = idx.copy()
    idx[:, 0] = np.random.RandomState(7).permutation(np.repeat(np.arange(17), 8))
    got = _tile_order(idx, mask, 4)
    assert torch.equal(got, torch.from_numpy(R.tile_order_ref(idx, mask, 4, batch_mask=0xff)))
    assert not torch.equal(got, torch.from_numpy(R.tile_order_ref(idx, mask, 4, batch_mask=0xf)))
    # (the slice schedule moves whole slices only: the last 8 rows, a partial slice, are the end of the locality order)
    assert idx[got.numpy()[-8:], 0].tolist() == [16] * 8


def test_morton_code_keeps_eight_bits_per_axis():
    """coordinates up to 255 with block_shift 0: bits 4..7 of every axis enter the key"""
    rng = np.random.RandomState(21)
    idx = np.concatenate([np.zeros((200, 1)), rng.randint(0, 256, (200, 3))], 1).astype(np.int32)
    idx[:3, 1:] = [[128, 0, 0], [0, 192, 0], [0, 0, 255]]
    mask = rng.randint(0, 1 << 27, 200).astype(np.int32)
    want = torch.from_numpy(R.tile_order_ref(idx, mask, 0))
    assert torch.equal(_tile_order(idx, mask, 0), want)
    assert torch.equal(_tile_order_batch([(idx, mask)], 0, 1)[0], want)


def test_three_tables_from_one_sort_equal_the_reference():
    """an empty table among others, the last one without a mask; batch_size 3: the 4-bit batch field, table number on top"""
    tabs = [_table(700, True), _table(0, True), _table(300, False)]
    # (the order inside a table does not depend on its number -- the device counts the empty table, the reference does
    # not --; what this pins is that the table field stays clear of the batch field: device table 2 meets batches 0..2)
    got, Ms = _tile_order_batch(tabs, 4, 3)
    off = table = 0
    for (idx, mask), M in zip(tabs, Ms):
        if M == 0:
            continue
        want = torch.from_numpy(R.tile_order_ref(idx, mask, 4, table=table, batch_mask=0xf))
        assert torch.equal(got[off:off + M], want), table
        off += M
        table += 1


@pytest.mark.parametrize("K,M", [(27, 1), (8, 700), (8, 0)])
def test_pack_equals_the_reference(K, M):
    _n, lib = _lib()
    rng = np.random.RandomState(K + M)
    nbr = rng.randint(-1, max(M, 1), (K, M)).astype(np.int32)
    order = rng.permutation(M).astype(np.int32)
    want = torch.from_numpy(R.pack_ref(nbr, order))
    d_nbr, d_order = _up(nbr), _up(order)
    one = torch.full((K, M), -9, dtype=torch.int32, device=DEV)
    _n.check(lib.wsis_rulebook_pack(_ptr(d_nbr), _ptr(d_order), _ptr(one), M, K, _n.stream_ptr()), "rulebook_pack")
    assert torch.equal(one.cpu(), want)
    many = torch.full((K, M), -9, dtype=torch.int32, device=DEV)
    _n.check(lib.wsis_rulebook_pack_batch(1, (ctypes.c_void_p * 1)(_ptr(d_nbr)), (ctypes.c_void_p * 1)(_ptr(d_order)),
                                          (ctypes.c_void_p * 1)(_ptr(many)), (ctypes.c_int64 * 1)(M),
                                          (ctypes.c_int32 * 1)(K), _n.stream_ptr()), "rulebook_pack_batch")
    assert torch.equal(many.cpu(), want)


# ---- the Python layer ----------------------------------------------------------------------------------------------
SHAPE = [30, 30, 10]


@functools.lru_cache(maxsize=None)
def _surface():
    """two scenes, each a random height field over the (30, 30, 10) grid: int32 [1800, 4] (batch, x, y, z)"""
    rng = np.random.RandomState(11)
    x, y = np.meshgrid(np.arange(30), np.arange(30), indexing="ij")
    rows = []
    for b in range(2):
        z = np.clip(np.round(4.5 + 2.0 * np.sin(x / 5.0 + b) + rng.randn(30, 30)), 0, 9).astype(np.int64)
        rows.append(np.stack([np.full(900, b), x.ravel(), y.ravel(), z.ravel()], 1))
    idx = np.concatenate(rows).astype(np.int32)
    return idx[rng.permutation(idx.shape[0])]


def _check_rulebook(rb, ordered=True):
    """order / order_up / nbr_p / nbr_up_p of ``rb`` against the reference applied to its own tables"""
    for nbr, order, packed, indices in ((rb.nbr, rb.order, rb.nbr_p, rb.out_indices),
                                        (rb.nbr_up, rb.order_up, rb.nbr_up_p, rb.in_indices)):
        if nbr is None:
            assert order is None and packed is None
            continue
        if not ordered:
            assert order is None and packed is nbr
            continue
        h_nbr = nbr.cpu().numpy()
        want = R.tile_order_ref(indices.cpu().numpy(), R.mask_of_nbr(h_nbr), 4)
        assert torch.equal(order.cpu(), torch.from_numpy(want))
        assert torch.equal(packed.cpu(), torch.from_numpy(R.pack_ref(h_nbr, want)))


def _build_two(ordered=True):
    from spconv import ops
    idx = _up(_surface())
    sub = ops.build_subm_rulebook(idx, SHAPE, [3, 3, 3], [1, 1, 1])
    down = ops.build_down_rulebook(idx, SHAPE, [2, 2, 2], [2, 2, 2], [0, 0, 0])
    torch.cuda.synchronize()
    assert sub.nbr.shape == (27, 1800) and down.nbr_up.shape == (8, 1800) and down.nbr.shape[1] >= 128
    _check_rulebook(sub, ordered)
    _check_rulebook(down, ordered)


def _prebuild(batch_size, counts=False):
    import spconv
    from spconv import ops
    idx = _up(_surface())
    t = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device=DEV), idx, SHAPE, batch_size)
    if counts:
        t._level_counts = ops.level_voxel_counts(_surface(), SHAPE, 3)
    ops.prebuild_unet_rulebooks(t, 3)
    torch.cuda.synchronize()
    ops.verify_pending_counts()
    assert len(t.indice_dict) == 5
    return t


def test_python_layer_default_switches():
    _build_two()
    for rb in _prebuild(2).indice_dict.values():           # all tables from one wsis_tile_order_batch call
        _check_rulebook(rb)
    native = _prebuild(2, counts=True)                     # the one-call pyramid
    assert type(native.indice_dict).__name__ == "PyramidDict"
    for rb in native.indice_dict.values():
        _check_rulebook(rb)


def test_python_layer_one_sort_per_table(monkeypatch):
    monkeypatch.setenv("WSIS_TILE_BATCH", "0")
    _build_two()
    for rb in _prebuild(2).indice_dict.values():
        _check_rulebook(rb)


def test_python_layer_without_mask_order(monkeypatch):
    monkeypatch.setenv("WSIS_MASK_ORDER", "0")
    _build_two(ordered=False)
    for rb in _prebuild(2).indice_dict.values():
        _check_rulebook(rb, ordered=False)


def test_python_layer_more_than_16_scenes():
    """batch_size 17 does not fit the 4-bit batch field: every table alone through wsis_tile_order"""
    for rb in _prebuild(17).indice_dict.values():
        _check_rulebook(rb)
