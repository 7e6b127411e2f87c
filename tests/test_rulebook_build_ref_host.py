"""The numpy definition of the whole rulebook build (tests/rulebook_ref.py: subm_table, down_tables, pyramid,
hash_contents) checked on its own against the loop-written oracle (oracle/spconv_ref.py), and every input builder of
tests/test_gpu_rulebook_build.py (tests/rulebook_cases.py) checked for the branch it is named after.  No device code."""
import numpy as np
import pytest

import rulebook_cases as C
import rulebook_ref as R
from oracle import spconv_ref as ref
from spconv import ops

SUBM_GEOS = [(3, 1), ((1, 3, 3), (0, 1, 1)), ((3, 1, 3), (1, 0, 1)), (2, 0), (3, 2), ((3, 3, 5), (1, 1, 2)), (5, 2)]
DOWN_GEOS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), ((1, 2, 2), (1, 2, 2), 0), ((2, 3, 2), (2, 2, 2), (0, 1, 0)), (3, 3, 0)]


def _small(shape, n_batch, density, seed):
    return C.random_rows(tuple(shape), n_batch, density, seed)


@pytest.mark.parametrize("shape", [(5, 4, 3), (1, 5, 4), (4, 1, 5), (5, 4, 1), (9, 8, 7)])
@pytest.mark.parametrize("k,p", SUBM_GEOS)
def test_subm_table_equals_the_loop_written_oracle(shape, k, p):
    idx = _small(shape, 2, 0.4, 3)
    nbr, mask = R.subm_table(idx, shape, k, p)
    want = ref.pairs_to_table(ref.subm_pairs(idx, shape, k, p), idx.shape[0])
    assert nbr.dtype == np.int32 and np.array_equal(nbr, want)
    assert mask.dtype == np.uint32 and np.array_equal(mask, R.mask_bits(want))
    if nbr.shape[0] > 32:
        assert int(mask.max()) < 1 << 32 and np.array_equal(mask, R.mask_bits(want[:32]))
    else:
        assert np.array_equal(mask.view(np.int32), R.mask_of_nbr(want))


@pytest.mark.parametrize("shape", [(8, 8, 8), (9, 7, 8), (3, 3, 3), (11, 6, 7)])
@pytest.mark.parametrize("k,s,p", DOWN_GEOS)
def test_down_tables_equal_the_loop_written_oracle(shape, k, s, p):
    idx = _small(shape, 3, 0.3, 4)
    out_idx, out_shape, nbr_down, nbr_up, mask_down, mask_up = R.down_tables(idx, shape, k, s, p)
    o_idx, o_shape, pairs = ref.down_pairs(idx, shape, k, s, p)
    assert list(out_shape) == list(o_shape) and np.array_equal(out_idx, o_idx) and out_idx.dtype == np.int32
    assert np.array_equal(nbr_down, ref.pairs_to_table(pairs, o_idx.shape[0]))
    assert np.array_equal(nbr_up, ref.pairs_to_table(ref.inverse_pairs(pairs), idx.shape[0]))
    assert np.array_equal(mask_down, R.mask_bits(nbr_down)) and np.array_equal(mask_up, R.mask_bits(nbr_up))
    keys = R.lin_keys(out_idx, out_shape)
    assert np.all(keys[1:] > keys[:-1])


@pytest.mark.parametrize("shape", [(8, 8, 8), (9, 7, 8)])
def test_batch_limit_leaves_rows_out(shape):
    idx = _small(shape, 4, 0.3, 5)
    inside = idx[:, 0] < 2
    out_idx, _, nbr_down, nbr_up, _, mask_up = R.down_tables(idx, shape, 2, 2, 0, batch_size=2)
    o_idx, _, pairs = ref.down_pairs(idx[inside], shape, 2, 2, 0)
    assert np.array_equal(out_idx, o_idx) and out_idx[:, 0].max() == 1
    assert np.all(nbr_up[:, ~inside] == -1) and np.all(mask_up[~inside] == 0)
    rows = np.nonzero(inside)[0].astype(np.int32)          # rows of the full table that the oracle's sub-table numbers
    want_down = ref.pairs_to_table(pairs, o_idx.shape[0])
    assert np.array_equal(nbr_down, np.where(want_down >= 0, rows[np.maximum(want_down, 0)], -1))
    assert np.array_equal(nbr_up[:, inside], ref.pairs_to_table(ref.inverse_pairs(pairs), int(inside.sum())))


def test_dropped_plane_gives_an_empty_level():
    idx = C.dropped_plane_rows()
    out_idx, out_shape, nbr_down, nbr_up, mask_down, mask_up = R.down_tables(idx, (3, 3, 3), 2, 2, 0)
    assert out_shape == [1, 1, 1] and out_idx.shape == (0, 4) and nbr_down.shape == (8, 0) and mask_down.shape == (0,)
    assert np.all(nbr_up == -1) and np.all(mask_up == 0)


def test_hash_contents_and_the_restated_hash_function():
    idx = _small((9, 8, 7), 2, 0.3, 6)
    keys, rows = R.hash_contents(idx, (9, 8, 7))
    assert np.all(keys[1:] > keys[:-1]) and np.array_equal(R.lin_keys(idx[rows], (9, 8, 7)), keys)
    # MurmurHash3's 64-bit finaliser: fmix64(1), fmix64(2) and the fixed point 0
    assert R.mix64(0) == 0 and R.mix64(1) == 0xb456bcfc34c2cb2c and R.mix64(2) == 0x3abf2a20650683e7
    assert R.home_slot(1, 16) == 0xc and R.occupied_slots([1, 1 + (1 << 40)], 1 << 20).__len__() == 2
    assert [R.pow2_cap(m) for m in (0, 1, 8, 9, 33, 64, 65)] == [16, 16, 16, 32, 128, 128, 256]


@pytest.mark.parametrize("shape,n_levels", [(C.ODD_SHAPE, 3), ((9, 7, 8), 3), ((21, 13, 6), 2)])
def test_level_voxel_counts_equal_the_pyramid_rows(shape, n_levels):
    """a row dropped on an odd plane stays dropped below"""
    idx = C.odd_pyramid_rows() if shape == C.ODD_SHAPE else _small(shape, 3, 0.3, 7)
    lv = R.pyramid(idx, shape, n_levels, 3, 4)
    assert ops.level_voxel_counts(idx, shape, n_levels) == [v["indices"].shape[0] for v in lv[1:]]
    assert [v["count"] for v in lv[:-1]] == [v["indices"].shape[0] for v in lv[1:]]
    for a, b in zip(lv[:-1], lv[1:]):
        assert b["shape"] == [(s - 2) // 2 + 1 for s in a["shape"]]
        assert np.array_equal(a["down_nbr_p"], a["down_nbr"][:, a["down_order"]])
        assert a["up_nbr"].shape == (8, a["indices"].shape[0]) and a["down_nbr"].shape == (8, b["indices"].shape[0])


def test_pyramid_orders_carry_the_table_number_and_a_four_bit_batch_field():
    idx = _small((12, 10, 9), 3, 0.3, 8)
    lv = R.pyramid(idx, (12, 10, 9), 2, 3, 4)
    a, b = lv
    assert np.array_equal(a["subm_order"], R.tile_order_ref(idx, a["subm_mask"].view(np.int32), 4, 0, 0xf))
    assert np.array_equal(a["down_order"], R.tile_order_ref(b["indices"], a["down_mask"].view(np.int32), 4, 1, 0xf))
    assert np.array_equal(a["up_order"], R.tile_order_ref(idx, a["up_mask"].view(np.int32), 4, 2, 0xf))
    assert np.array_equal(b["subm_order"], R.tile_order_ref(b["indices"], b["subm_mask"].view(np.int32), 4, 3, 0xf))
    assert "down_nbr" not in b and "count" not in b


# ---- the builders reach their branches ------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 7, 8, 9, 33])
def test_wrap_rows_reach_the_probing_branches(M):
    idx = C.wrap_rows(M)
    cap = R.pow2_cap(M)
    assert idx.shape == (M, 4) and cap == {1: 16, 2: 16, 7: 16, 8: 16, 9: 32, 33: 128}[M]
    f = C.probe_facts(idx, C.WRAP_SHAPE, cap)
    assert f["last"] >= min(M, 3)                          # (a table of M rows cannot hold more than M such keys)
    assert f["miss_after_collision"] >= 1
    assert f["found_later"] >= (1 if M >= 2 else 0)
    assert f["found_through_wrap"] >= (1 if M >= 2 else 0)     # a looked-up key of the last slot that is stored at slot 0 ..
    if M >= 2:                                             # probing wraps: slots 0 .. hold the keys that found cap - 1 taken
        taken = R.occupied_slots([int(k) for k in R.lin_keys(idx, C.WRAP_SHAPE)], cap)
        assert cap - 1 in taken and 0 in taken and (M < 3 or 1 in taken)


def test_wrap_in_loop_rows_put_a_key_of_slot_cap_minus_2_into_slot_0():
    idx = C.wrap_in_loop_rows()
    cap = R.pow2_cap(idx.shape[0])
    keys = [int(k) for k in R.lin_keys(idx, C.WRAP_SHAPE)]
    mine = [k for k in keys if R.home_slot(k, cap) == cap - 2]
    assert cap == 16 and len(mine) == 3 and not any(R.home_slot(k, cap) in (cap - 1, 0) for k in keys)
    for order in (keys, keys[::-1], mine + [k for k in keys if k not in mine]):
        assert {cap - 2, cap - 1, 0} <= R.occupied_slots(order, cap)
    assert set(mine) <= C._queried_keys(idx, C.WRAP_SHAPE)


def test_dense_blocks_meet_every_boundary_combination():
    idx = C.block_rows((6, 6, 6))
    nbr, mask = R.subm_table(idx, (6, 6, 6), 3, 1)
    inner = np.all((idx[:, 1:] >= 1) & (idx[:, 1:] <= 4), axis=1)
    assert inner.sum() == 64 and np.all(mask[inner] == 0x7FFFFFF)
    corner = np.all((idx[:, 1:] == 0) | (idx[:, 1:] == 5), axis=1)
    assert corner.sum() == 8 and len(set(mask[corner].tolist())) == 8
    assert all(bin(int(m)).count("1") == 8 for m in mask[corner])
    assert len(set(mask.tolist())) == 27                   # every combination of (low edge, inside, high edge) per axis
    for shape in ((1, 5, 7), (5, 1, 7), (5, 7, 1)):
        nbr, mask = R.subm_table(C.block_rows(shape), shape, 3, 1)
        assert int((nbr >= 0).sum(0).max()) == 9 and len(set(mask.tolist())) == 9


def test_batch_isolation_case_has_adjacent_keys_in_different_batch_items():
    idx = C.block_rows((5, 5, 5), 16)
    assert idx.shape[0] == 2000 and set(idx[:, 0].tolist()) == set(range(16))
    keys, rows = R.hash_contents(idx, (5, 5, 5))
    assert np.all(np.diff(keys) == 1)                      # key + 1 of a batch item's last cell is the next item's first
    nbr, _ = R.subm_table(idx, (5, 5, 5), 3, 1)
    assert np.all((nbr < 0) | (idx[np.maximum(nbr, 0), 0] == idx[None, :, 0]))


def test_big_key_rows_exceed_31_and_32_bits():
    idx = C.big_key_rows()                                 # (asserts the key ranges itself)
    nbr, mask = R.subm_table(idx, C.BIG_SHAPE, 3, 1)
    assert (mask == 0x7FFFFFF).any() and int((nbr >= 0).sum()) > 10 * idx.shape[0]
    for k, s, p in ((2, 2, 0), (3, 2, 1)):
        out_idx, out_shape, *_ = R.down_tables(idx, C.BIG_SHAPE, k, s, p)
        assert int(R.lin_keys(out_idx, out_shape).max()) > 1 << 29 and out_idx[:, 0].max() == 1


def test_pyramid_builders():
    assert [v["indices"].shape[0] for v in R.pyramid(C.block20_rows(), (64, 64, 64), 6, 1, 4)] == \
        [8000, 1000, 125, 27, 8, 1]
    idx, shape = C.cells45_rows()
    assert R.pyramid(idx, shape, 2, 1, 4)[1]["shape"] == [5, 3, 3]
    assert C.empty_level_rows().shape[0] > 100
    lv = R.pyramid(C.odd_pyramid_rows(), C.ODD_SHAPE, 3, 3, 4)
    assert [v["shape"] for v in lv] == [[37, 30, 23], [18, 15, 11], [9, 7, 5]]
    assert min(v["indices"].shape[0] for v in lv) >= 128
    for n_batch, seed in ((1, 81), (4, 82)):
        box = C.box_rows(n_batch, seed)
        assert set(box[:, 0].tolist()) == set(range(n_batch)) and np.all(box[:, 1:].max(0) < (20, 18, 14))
    cut = R.pyramid(C.box_rows(4, 82), (20, 18, 14), 3, 2, 4)
    assert cut[1]["indices"][:, 0].max() == 1 and cut[0]["indices"].shape[0] == C.box_rows(4, 82).shape[0]


def test_sheet_rows_need_more_than_256_chunks():
    idx = C.sheet_rows()                                   # (asserts chunks == 275 and keys behind chunk 256 itself)
    assert C.bitmap_chunks((208, 208, 208), 1)[2] > 256
    # the bitmap and its chunk sums fit the sort workspace of these rows whatever the sort's own scratch takes: the
    # workspace holds the sorted keys (8 bytes a row) before anything else
    cells, words, chunks = C.bitmap_chunks((208, 208, 208), 1)
    assert (words * 4 + 255) // 256 * 256 + (chunks * 4 + 255) // 256 * 256 <= idx.shape[0] * 8
