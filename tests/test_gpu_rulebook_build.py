"""The rulebook build of csrc/rulebook.hip -- coordinate hash, SubM tables, strided tables with their output set, offset
masks, and the one-call pyramid with its orders and packed tables -- against its numpy definition
(tests/rulebook_ref.py), bit for bit, through the C entry points.  Every buffer the caller owns starts from a sentinel
(-7 in tables, orders, coordinates and counts, 0xA5A5A5A5 in masks), so a word no kernel writes cannot pass; every case
asserts that it reaches the branch it is named after (tests/rulebook_cases.py; the same assertions run on the host in
tests/test_rulebook_build_ref_host.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rulebook_cases as C
import rulebook_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASK_SENTINEL = 0xA5A5A5A5 - (1 << 32)      # as int32
BITMAP, SORT = 1, 0


def _lib():
    import wsis_native as _n
    return _n, _n.hip()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _full(shape, value, dtype=torch.int32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _hash_pairs(keys, vals):
    """(keys ascending, value of each key) of the occupied slots of a device or host hash table"""
    k = keys.cpu().numpy() if isinstance(keys, torch.Tensor) else keys
    v = vals.cpu().numpy() if isinstance(vals, torch.Tensor) else vals
    used = k != -1
    by_key = np.argsort(k[used], kind="stable")
    return k[used][by_key], v[used][by_key]


def _check_hash(keys, vals, indices, shape):
    got_k, got_v = _hash_pairs(keys, vals)
    want_k, want_v = R.hash_contents(indices, shape)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)


def _hash(d_idx, shape):
    _n, lib = _lib()
    M = d_idx.shape[0]
    cap = R.pow2_cap(M)
    keys, vals = _full((cap,), -7, torch.int64), _full((cap,), -7)
    _n.check(lib.wsis_hash_build(_ptr(d_idx), M, _n.i32x3(shape), _ptr(keys), _ptr(vals), cap, _n.stream_ptr()), "hash")
    return keys, vals, cap


def _subm(idx, shape, k, p):
    """hash + wsis_rulebook_subm -> nbr int32 [K, M], mask uint32 [M] (host), and the hash (device)"""
    _n, lib = _lib()
    k3, p3 = R._triple(k), R._triple(p)
    d_idx = _up(idx)
    M = idx.shape[0]
    keys, vals, cap = _hash(d_idx, shape)
    nbr, mask = _full((k3[0] * k3[1] * k3[2], M), -7), _full((M,), MASK_SENTINEL)
    _n.check(lib.wsis_rulebook_subm(_ptr(d_idx), M, _n.i32x3(shape), _n.i32x3(k3), _n.i32x3(p3), _ptr(keys), _ptr(vals),
                                    cap, _ptr(nbr), _ptr(mask), _n.stream_ptr()), "rulebook_subm")
    return nbr.cpu().numpy(), _u32(mask), (keys, vals)


def _check_subm(idx, shape, k=3, p=1):
    nbr, mask, (keys, vals) = _subm(idx, shape, k, p)
    want_nbr, want_mask = R.subm_table(idx, shape, k, p)
    _check_hash(keys, vals, idx, shape)
    assert np.array_equal(nbr, want_nbr)
    assert np.array_equal(mask, want_mask)
    return want_nbr, want_mask


def _down(idx, shape, k, s, p):
    """wsis_rulebook_down_keys + the count read + wsis_rulebook_down_fill, as the per-table build issues them"""
    _n, lib = _lib()
    k3, s3, p3 = _n.i32x3(R._triple(k)), _n.i32x3(R._triple(s)), _n.i32x3(R._triple(p))
    out_shape = R.out_shape_of(shape, k, s, p)
    in3, out3 = _n.i32x3(shape), _n.i32x3(out_shape)
    d_idx = _up(idx)
    M = idx.shape[0]
    K = int(np.prod(R._triple(k)))
    n_cand = lib.wsis_rulebook_down_ncand(M, k3, s3, p3)
    ws_bytes = lib.wsis_rulebook_down_workspace_bytes(n_cand)
    assert n_cand >= M and ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    cand, out_keys, count = _full((n_cand,), -7, torch.int64), _full((n_cand,), -7, torch.int64), _full((1,), -7)
    _n.check(lib.wsis_rulebook_down_keys(_ptr(d_idx), M, in3, out3, k3, s3, p3, _ptr(cand), _ptr(out_keys), _ptr(count),
                                         _ptr(ws), ws_bytes, _n.stream_ptr()), "rulebook_down_keys")
    M_out = int(count.item())
    assert 0 <= M_out <= n_cand
    cap = R.pow2_cap(M_out)
    out = {"count": M_out, "out_shape": out_shape, "out_indices": _full((M_out, 4), -7),
           "keys": _full((cap,), -7, torch.int64), "vals": _full((cap,), -7),
           "nbr_down": _full((K, M_out), -7), "nbr_up": _full((K, M), -7),
           "mask_down": _full((M_out,), MASK_SENTINEL), "mask_up": _full((M,), MASK_SENTINEL)}
    _n.check(lib.wsis_rulebook_down_fill(_ptr(d_idx), M, in3, out3, k3, s3, p3, _ptr(out_keys), M_out,
                                         _ptr(out["out_indices"]), _ptr(out["keys"]), _ptr(out["vals"]), cap,
                                         _ptr(out["nbr_down"]), _ptr(out["nbr_up"]), _ptr(out["mask_down"]),
                                         _ptr(out["mask_up"]), _n.stream_ptr()), "rulebook_down_fill")
    return out


def _check_down(idx, shape, k, s, p):
    got = _down(idx, shape, k, s, p)
    out_idx, out_shape, nbr_down, nbr_up, mask_down, mask_up = R.down_tables(idx, shape, k, s, p)
    assert got["count"] == out_idx.shape[0] and got["out_shape"] == out_shape
    assert np.array_equal(got["out_indices"].cpu().numpy(), out_idx)
    assert np.array_equal(got["nbr_down"].cpu().numpy(), nbr_down)
    assert np.array_equal(got["nbr_up"].cpu().numpy(), nbr_up)
    assert np.array_equal(_u32(got["mask_down"]), mask_down)
    assert np.array_equal(_u32(got["mask_up"]), mask_up)
    _check_hash(got["keys"], got["vals"], out_idx, out_shape)
    return out_idx, nbr_up, mask_up


# ---- hash + subm3_kernel (k3 p1) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 7, 8, 9, 33])
def test_subm3_probing_wraps_and_survives_collisions(M):
    """min(M, 3) keys whose first slot is the last one of the table (the others of them are stored at slots 0, 1), a
    lookup that finds its key behind a collision and one that runs from a taken first slot into an empty one"""
    idx = C.wrap_rows(M)
    cap = R.pow2_cap(M)
    f = C.probe_facts(idx, C.WRAP_SHAPE, cap)
    assert f["last"] >= min(M, 3) and f["miss_after_collision"] >= 1
    assert M < 2 or (f["found_later"] >= 1 and f["found_through_wrap"] >= 1)
    _check_subm(idx, C.WRAP_SHAPE)
    if M >= 2:      # the wrap in the device's own table: keys whose first slot is cap - 1 stored in slots 0 ..
        keys = _hash(_up(idx), C.WRAP_SHAPE)[0].cpu().numpy()
        wrapped = [s for s, k in enumerate(keys.tolist()) if k != -1 and R.home_slot(k, cap) == cap - 1 and s != cap - 1]
        assert keys[cap - 1] != -1 and len(wrapped) >= min(M, 3) - 1      # (probing only moves up: below = wrapped)


def test_subm3_probing_loop_steps_from_the_last_slot_to_slot_0():
    """three keys of first slot cap - 2 fill cap - 2, cap - 1 and 0; the one in slot 0 is looked up by a neighbour"""
    idx = C.wrap_in_loop_rows()
    cap = R.pow2_cap(idx.shape[0])
    _check_subm(idx, C.WRAP_SHAPE)
    keys = _hash(_up(idx), C.WRAP_SHAPE)[0].cpu().numpy()
    assert keys[0] != -1 and R.home_slot(int(keys[0]), cap) == cap - 2
    assert int(keys[0]) in C._queried_keys(idx, C.WRAP_SHAPE)


def test_subm3_dense_block_every_boundary_combination():
    """(6, 6, 6) fully occupied: interior rows have all 27 neighbours, corners / edges / faces every combination of the
    tests at coordinate 0 and shape - 1"""
    idx = C.block_rows((6, 6, 6))
    _, mask = _check_subm(idx, (6, 6, 6))
    inner = np.all((idx[:, 1:] >= 1) & (idx[:, 1:] <= 4), axis=1)
    assert np.all(mask[inner] == 0x7FFFFFF) and len(set(mask.tolist())) == 27


@pytest.mark.parametrize("shape", [(1, 5, 7), (5, 1, 7), (5, 7, 1)])
def test_subm3_axis_of_size_one(shape):
    nbr, _ = _check_subm(C.block_rows(shape), shape)
    assert int((nbr >= 0).sum(0).max()) == 9


def test_subm3_no_entry_crosses_a_batch_item():
    idx = C.block_rows((5, 5, 5), 16)
    nbr, _ = _check_subm(idx, (5, 5, 5))
    assert np.all((nbr < 0) | (idx[np.maximum(nbr, 0), 0] == idx[None, :, 0]))


def test_subm3_keys_above_32_bits():
    idx = C.big_key_rows()
    assert int(R.lin_keys(idx, C.BIG_SHAPE).max()) > 1 << 32
    _check_subm(idx, C.BIG_SHAPE)


# ---- generic subm_kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,density", [((9, 8, 7), 0.3), ((24, 20, 16), 0.05)])
@pytest.mark.parametrize("k,p", [((1, 3, 3), (0, 1, 1)), ((3, 1, 3), (1, 0, 1)), (2, 0), (3, 2), ((3, 3, 5), (1, 1, 2)),
                                 (5, 2)])
def test_generic_subm_geometries(shape, density, k, p):
    """(5, 2): 125 offsets with a mask buffer -- only the bits of the first 32 are set"""
    idx = C.random_rows(shape, 2, density, 11)
    nbr, mask = _check_subm(idx, shape, k, p)
    assert nbr.shape[0] == int(np.prod(R._triple(k))) and (nbr >= 0).any()


# ---- strided build, per-table entry points --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8, 8), (9, 7, 8), (33, 20, 17)])
@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (3, 2, 1), (3, 1, 1), ((1, 2, 2), (1, 2, 2), 0),
                                   ((2, 3, 2), (2, 2, 2), (0, 1, 0)), (3, 3, 0)])
def test_strided_tables(shape, k, s, p):
    _check_down(C.random_rows(shape, 3, 0.25, 12), shape, k, s, p)


def test_strided_level_without_output_rows():
    """every voxel on the odd plane k2 s2 drops: count 0, nbr_up all -1, mask_up all 0 (M_out == 0: the fill zeroes it)"""
    idx = C.dropped_plane_rows()
    out_idx, nbr_up, mask_up = _check_down(idx, (3, 3, 3), 2, 2, 0)
    assert out_idx.shape[0] == 0 and np.all(nbr_up == -1) and np.all(mask_up == 0)


@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (3, 2, 1), (3, 1, 1)])
def test_strided_tables_keys_above_32_bits(k, s, p):
    """the fine keys are above 2^31 and 2^32 in all three; with stride 1 the output grid is the input grid, so the
    output keys the device sorts and decodes are as well"""
    out_idx, _, _ = _check_down(C.big_key_rows(), C.BIG_SHAPE, k, s, p)
    top = int(R.lin_keys(out_idx, R.out_shape_of(C.BIG_SHAPE, k, s, p)).max())
    assert top > (1 << 32 if s == 1 else 1 << 29)


# ---- the pyramid arena ----------------------------------------------------------------------------------------------
def _ops():
    from spconv import ops
    return ops


TABLE_FIELDS = ("SUBM_NBR", "SUBM_ORDER", "SUBM_NBR_P", "DOWN_NBR", "UP_NBR", "DOWN_ORDER", "UP_ORDER", "DOWN_NBR_P",
                "UP_NBR_P", "INDICES", "COUNT")
MASK_FIELDS = ("SUBM_MASK", "DOWN_MASK", "UP_MASK")


def _form(M, shape, batch_size):
    _n, lib = _lib()
    form = lib.wsis_rulebook_down_form(M, _n.i32x3(R.out_shape_of(shape, 2, 2, 0)), _n.i32x3(2), _n.i32x3(2), _n.i32x3(0),
                                       batch_size)
    assert form in (BITMAP, SORT)
    return form


def _build_pyramid(idx, shape, n_levels, batch_size, counts, block_shift=4):
    """wsis_rulebook_pyramid into an arena whose fields start from their sentinels -> {(level, field): host array}"""
    _n, lib = _lib()
    ops = _ops()
    M0 = idx.shape[0]
    rows = [M0] + [int(c) for c in counts]
    h_counts = (ctypes.c_int64 * max(len(counts), 1))(*[int(c) for c in counts])
    layout = np.zeros((n_levels, ops.PYR_FIELDS), dtype=np.int64)
    total = lib.wsis_rulebook_pyramid_layout(M0, h_counts, n_levels, layout.ctypes.data)
    assert total > 0
    arena = torch.zeros(total + 256, dtype=torch.uint8, device=DEV)
    skip = (-arena.data_ptr()) % 256
    arena = arena[skip:skip + total]

    def span(l, name):
        """(offset, int32 words) of a field"""
        M, Mo = rows[l], rows[l + 1] if l + 1 < n_levels else 0
        words = {"SUBM_NBR": 27 * M, "SUBM_NBR_P": 27 * M, "SUBM_ORDER": M, "SUBM_MASK": M, "INDICES": 4 * M,
                 "DOWN_NBR": 8 * Mo, "DOWN_NBR_P": 8 * Mo, "DOWN_ORDER": Mo, "DOWN_MASK": Mo, "UP_NBR": 8 * M,
                 "UP_NBR_P": 8 * M, "UP_ORDER": M, "UP_MASK": M, "COUNT": 1,
                 "KEYS": 2 * int(layout[l, ops.PYR_CAP]), "VALS": int(layout[l, ops.PYR_CAP])}[name]
        return int(layout[l, getattr(ops, "PYR_" + name)]), words

    for l in range(n_levels):
        assert int(layout[l, ops.PYR_ROWS]) == rows[l] and int(layout[l, ops.PYR_CAP]) == R.pow2_cap(rows[l])
        for names, value in ((TABLE_FIELDS + ("KEYS", "VALS"), -7), (MASK_FIELDS, MASK_SENTINEL)):
            for name in names:
                off, words = span(l, name)
                if off >= 0 and words:
                    assert off % 4 == 0 and off + 4 * words <= total
                    arena[off:off + 4 * words].view(torch.int32).fill_(value)
    d_idx = _up(idx)
    _n.check(lib.wsis_rulebook_pyramid(_ptr(d_idx), M0, _n.i32x3(shape), h_counts, n_levels, batch_size, block_shift,
                                       arena.data_ptr(), total, _n.stream_ptr()), "rulebook_pyramid")
    host = arena.cpu().numpy()
    got = {}
    for l in range(n_levels):
        for name in TABLE_FIELDS + MASK_FIELDS + ("KEYS", "VALS"):
            off, words = span(l, name)
            if off >= 0:
                got[l, name] = host[off:off + 4 * words].view(np.int64 if name == "KEYS" else np.int32)
    return got


def _check_arena(got, want, n_levels):
    """every field of every level against the reference's levels"""
    for l, lv in enumerate(want):
        M = lv["indices"].shape[0]
        if l > 0:
            assert np.array_equal(got[l, "INDICES"].reshape(M, 4), lv["indices"]), l
        k, v = _hash_pairs(got[l, "KEYS"], got[l, "VALS"])
        wk, wv = R.hash_contents(lv["indices"], lv["shape"])
        assert np.array_equal(k, wk) and np.array_equal(v, wv), l
        names = [("SUBM", "subm", 27, M)]
        if l + 1 < n_levels:
            Mo = want[l + 1]["indices"].shape[0]
            assert int(got[l, "COUNT"][0]) == lv["count"] == Mo, l
            names += [("DOWN", "down", 8, Mo), ("UP", "up", 8, M)]
        else:
            assert (l, "COUNT") not in got
        for dev, ref, K, rows in names:
            assert np.array_equal(got[l, dev + "_NBR"].reshape(K, rows), lv[ref + "_nbr"]), (l, dev)
            assert np.array_equal(got[l, dev + "_MASK"].view(np.uint32), lv[ref + "_mask"]), (l, dev)
            assert np.array_equal(got[l, dev + "_ORDER"], lv[ref + "_order"]), (l, dev)
            assert np.array_equal(got[l, dev + "_NBR_P"].reshape(K, rows), lv[ref + "_nbr_p"]), (l, dev)


@functools.lru_cache(maxsize=None)
def _want(case, shape, n_levels, batch_size):
    idx = {"odd": C.odd_pyramid_rows, "block20": C.block20_rows, "box1": lambda: C.box_rows(1, 81),
           "box4": lambda: C.box_rows(4, 82), "cells45": lambda: C.cells45_rows()[0], "sheet": C.sheet_rows,
           "big": C.big_key_rows}[case]()
    return idx, R.pyramid(idx, shape, n_levels, batch_size, 4)


def _pyramid_case(case, shape, n_levels, batch_size):
    idx, want = _want(case, tuple(shape), n_levels, batch_size)
    got = _build_pyramid(idx, shape, n_levels, batch_size, [lv["count"] for lv in want[:-1]])
    _check_arena(got, want, n_levels)
    return idx, want, got


def test_pyramid_three_levels_with_odd_planes():
    idx, want, _ = _pyramid_case("odd", C.ODD_SHAPE, 3, 3)
    assert [lv["shape"] for lv in want] == [[37, 30, 23], [18, 15, 11], [9, 7, 5]]
    # (11,000 rows in 3 x 18 x 15 x 11 cells: the bitmap fits the sort workspace)
    assert _form(idx.shape[0], C.ODD_SHAPE, 3) == BITMAP


@pytest.mark.parametrize("n_levels", [5, 6])
def test_pyramid_levels_below_one_slice_and_of_one_row(n_levels):
    """a (20, 20, 20) block: 8,000 / 1,000 / 125 / 27 / 8 rows, and on a sixth level a single one"""
    idx, want, _ = _pyramid_case("block20", (64, 64, 64), n_levels, 1)
    assert [lv["indices"].shape[0] for lv in want] == [8000, 1000, 125, 27, 8, 1][:n_levels]
    assert _form(8000, (64, 64, 64), 1) == BITMAP


def test_pyramid_both_forms_on_the_same_coordinates():
    """rows of batch item 0 only, built with batch_size 1 (level 0 -> 1 by the bitmap) and 16 (by the sort): both arenas
    equal the reference and -- the batch field of every tile key being 0 -- each other"""
    idx = C.box_rows(1, 81)
    shapes = [s for s in C.FORM_SHAPES if _form(idx.shape[0], s, 1) == BITMAP and _form(idx.shape[0], s, 16) == SORT]
    assert shapes, "no shape whose level 0 takes the bitmap at batch_size 1 and the sort at 16"
    shape = shapes[0]
    _, _, a = _pyramid_case("box1", shape, 3, 1)
    _, _, b = _pyramid_case("box1", shape, 3, 16)
    assert a.keys() == b.keys()
    for key in a:
        if key[1] not in ("KEYS", "VALS"):      # (which slot holds a key depends on the order the threads arrive in)
            assert np.array_equal(a[key], b[key]), key
        else:
            assert a[key].shape == b[key].shape


def test_pyramid_bitmap_of_45_bits():
    """output grid (5, 3, 3): the last bitmap word is partial, 2 words are no multiple of the 4 a thread reads"""
    idx, shape = C.cells45_rows()
    assert _form(idx.shape[0], shape, 1) == BITMAP
    _pyramid_case("cells45", shape, 2, 1)


def test_pyramid_bitmap_of_more_than_256_chunks():
    """145,000 rows in (416, 416, 416): 275 chunk sums, the scan's carry from its first 256 into the second pass"""
    idx = C.sheet_rows()
    assert C.bitmap_chunks((208, 208, 208), 1)[2] > 256
    assert _form(idx.shape[0], C.SHEET_SHAPE, 1) == BITMAP
    _pyramid_case("sheet", C.SHEET_SHAPE, 2, 1)


def test_pyramid_more_than_2_31_output_cells_takes_the_sort():
    idx = C.big_key_rows()
    assert C.bitmap_chunks(R.out_shape_of(C.BIG_SHAPE, 2, 2, 0), 16)[0] > 1 << 31
    assert _form(idx.shape[0], C.BIG_SHAPE, 16) == SORT
    _pyramid_case("big", C.BIG_SHAPE, 2, 16)


@pytest.mark.parametrize("form", [BITMAP, SORT])
def test_pyramid_leaves_out_rows_beyond_the_batch_size(form):
    """rows of batch items 0 .. 3 built with batch_size 2: the level counts, the coarse coordinates and the up tables
    hold nothing of items 2 and 3, whichever form finds the output cells"""
    idx = C.box_rows(4, 82)
    shapes = [s for s in C.FORM_SHAPES if _form(idx.shape[0], s, 2) == form]
    assert shapes, "no shape that takes form %d" % form
    _, want, got = _pyramid_case("box4", shapes[0], 3, 2)
    beyond = idx[:, 0] >= 2
    assert beyond.any() and int(got[0, "COUNT"][0]) == want[0]["count"]
    assert got[1, "INDICES"].reshape(-1, 4)[:, 0].max() == 1
    assert np.all(got[0, "UP_NBR"].reshape(8, -1)[:, beyond] == -1)
    assert np.all(got[0, "UP_MASK"][beyond] == 0)


# ---- the Python layer -----------------------------------------------------------------------------------------------
def test_python_layer_builds_an_empty_level_table_by_table():
    """level 2 of the pyramid is empty (its hint is 0): the one-call build is refused, the per-table walk builds every
    table, the empty ones included, and the device counts agree with the hints"""
    import spconv
    ops = _ops()
    idx = C.empty_level_rows()
    shape = [6, 6, 6]
    want = R.pyramid(idx, shape, 3, 2, 4)
    t = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device=DEV), _up(idx), shape, 2)
    t._level_counts = ops.level_voxel_counts(idx, shape, 3)
    assert t._level_counts == [want[1]["indices"].shape[0], 0]
    assert not ops._pyramid_native_ok(t, 3, ["subm1", "subm2", "subm3", "spconv1", "spconv2"])
    ops.prebuild_unet_rulebooks(t, 3)
    torch.cuda.synchronize()
    ops.verify_pending_counts()
    assert not isinstance(t.indice_dict, ops.PyramidDict) and len(t.indice_dict) == 5

    def same(nbr, order, packed, ref, rows):
        assert tuple(nbr.shape) == ref["nbr"].shape and np.array_equal(nbr.cpu().numpy(), ref["nbr"])
        if rows == 0:
            assert order is None or order.numel() == 0
            return
        assert np.array_equal(order.cpu().numpy(), ref["order"])
        assert np.array_equal(packed.cpu().numpy(), ref["nbr_p"])

    for l, lv in enumerate(want):
        M = lv["indices"].shape[0]
        rb = t.indice_dict["subm%d" % (l + 1)]
        same(rb.nbr, rb.order, rb.nbr_p, {k[5:]: v for k, v in lv.items() if k.startswith("subm_")}, M)
        if l + 1 < 3:
            rb = t.indice_dict["spconv%d" % (l + 1)]
            Mo = want[l + 1]["indices"].shape[0]
            assert np.array_equal(rb.out_indices.cpu().numpy(), want[l + 1]["indices"]) and list(rb.out_shape) == \
                want[l + 1]["shape"]
            same(rb.nbr, rb.order, rb.nbr_p, {k[5:]: v for k, v in lv.items() if k.startswith("down_")}, Mo)
            same(rb.nbr_up, rb.order_up, rb.nbr_up_p, {k[3:]: v for k, v in lv.items() if k.startswith("up_")}, M)
            if Mo == 0:
                assert np.all(rb.nbr_up.cpu().numpy() == -1)


def test_level_counts_on_the_device_and_on_the_host_equal_the_reference():
    ops = _ops()
    idx = C.odd_pyramid_rows()
    want = [lv["indices"].shape[0] for lv in _want("odd", C.ODD_SHAPE, 3, 3)[1][1:]]
    assert ops.level_voxel_counts(idx, C.ODD_SHAPE, 3) == want
    assert ops.level_voxel_counts_device(_up(idx).long(), C.ODD_SHAPE, 3).tolist() == want
