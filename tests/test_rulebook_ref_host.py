"""The numpy definition of a tile order (tests/rulebook_ref.py) checked on its own: a case worked by hand and the
properties DESIGN.md section 4.3 states.  No device code runs here; tests/test_gpu_rulebook_order.py compares the device
with this reference."""
import numpy as np

import rulebook_ref as R

# (batch, x, y, z), mask.  Morton code with block_shift 0: x -> bit 0, y -> bit 1, z -> bit 2, x >> 1 -> bit 3, ...
HAND_ROWS = np.array([[1, 0, 0, 0],     # 0: batch 1, morton 0, mask 5
                      [0, 1, 1, 0],     # 1: morton 3, mask 3
                      [0, 0, 0, 1],     # 2: morton 4, mask 1
                      [0, 1, 1, 0],     # 3: morton 3, mask 2 -> before row 1
                      [0, 2, 0, 0],     # 4: morton 8, mask 0
                      [0, 0, 0, 1],     # 5: the key of row 2 -> behind it (stable)
                      [0, 0, 0, 0],     # 6: morton 0, mask 7 -> first
                      [1, 0, 0, 0]],    # 7: batch 1, morton 0, mask 4 -> before row 0
                     dtype=np.int32)
HAND_MASK = np.array([5, 3, 1, 2, 0, 1, 7, 4], dtype=np.int32)


def test_hand_worked_order_of_eight_rows():
    assert R.morton24(np.array([1, 0, 0, 2, 3]), np.array([0, 1, 0, 0, 1]), np.array([0, 0, 1, 0, 2])).tolist() == \
        [1, 2, 4, 8, 1 + 8 + 2 + 32]
    assert R.morton24(np.array([128, 16]), np.array([0, 64]), np.array([255, 0])).tolist() == \
        [(1 << 21) | sum(4 << (3 * i) for i in range(8)), (1 << 12) | (1 << 19)]
    key = R.tile_key(HAND_ROWS, HAND_MASK, 0)
    assert int(key[1]) == (3 << 32) | 3 and int(key[0]) == (1 << 56) | 5 and int(key[4]) == 8 << 32
    assert R.tile_order_ref(HAND_ROWS, HAND_MASK, 0).tolist() == [6, 3, 1, 2, 5, 4, 7, 0]
    # blocks of 2 voxels per side: rows 1, 2, 3, 5, 6 share block (0, 0, 0) and sort by mask, row 4 is block (1, 0, 0)
    assert R.tile_order_ref(HAND_ROWS, HAND_MASK, 1).tolist() == [2, 5, 3, 1, 6, 4, 7, 0]
    # without a mask: (batch, morton) only, ties in row order
    assert R.tile_order_ref(HAND_ROWS, None, 0).tolist() == [6, 1, 3, 2, 5, 4, 0, 7]
    # the table number sits above everything and does not change the order inside a table
    assert int(R.tile_key(HAND_ROWS, HAND_MASK, 0, table=3, batch_mask=0xf)[0]) == (3 << 60) | (1 << 56) | 5
    assert R.tile_order_ref(HAND_ROWS, HAND_MASK, 0, table=3, batch_mask=0xf).tolist() == [6, 3, 1, 2, 5, 4, 7, 0]
    # a 4-bit batch field folds batch 16 onto batch 0, the 8-bit field does not
    rows = np.array([[16, 0, 0, 0], [1, 0, 0, 0]], dtype=np.int32)
    assert R.tile_order_ref(rows, None, 0).tolist() == [1, 0]
    assert R.tile_order_ref(rows, None, 0, batch_mask=0xf).tolist() == [0, 1]


def _table(M, seed):
    rng = np.random.RandomState(seed)
    idx = np.concatenate([rng.randint(0, 2, (M, 1)), rng.randint(0, 60, (M, 3))], 1).astype(np.int32)
    # one of 12 offsets per row: the union over a slice has 8 to 12 bits, so slices of equal and of different weight occur
    mask = (1 << rng.randint(0, 12, M)).astype(np.int32)
    return idx, mask


def test_scheduled_order_of_160_rows():
    idx, mask = _table(160, 3)
    order = R.tile_order_ref(idx, mask, 4)
    assert order.dtype == np.int32
    assert np.array_equal(np.sort(order), np.arange(160))
    local = np.argsort(R.tile_key(idx, mask, 4), kind="stable")
    # every full output slice is one slice of the locality order, rows in the same sequence
    src = {tuple(local[s * 32:(s + 1) * 32]): s for s in range(5)}
    came_from = [src[tuple(order[s * 32:(s + 1) * 32])] for s in range(5)]
    assert sorted(came_from) == list(range(5))
    # slice weights (kernel offsets any row of the slice uses) do not increase, equal weights keep the locality order
    w = 32 - R.slice_weights(order, mask)
    assert np.all(w[1:] <= w[:-1])
    assert 1 < len(set(w.tolist())) < 5                    # the case has slices of different and of equal weight
    for a, b in zip(range(4), range(1, 5)):
        if w[a] == w[b]:
            assert came_from[a] < came_from[b]


def test_equal_weights_keep_the_locality_order_and_the_partial_slice_stays():
    idx, _ = _table(170, 4)
    mask = np.full(170, 0b1011, dtype=np.int32)        # every slice has weight 3
    order = R.tile_order_ref(idx, mask, 4)
    assert np.array_equal(order, np.argsort(R.tile_key(idx, mask, 4), kind="stable"))
    idx, mask = _table(170, 5)
    order = R.tile_order_ref(idx, mask, 4)
    local = np.argsort(R.tile_key(idx, mask, 4), kind="stable")
    assert np.array_equal(order[160:], local[160:])
    assert np.array_equal(np.sort(order[:160]), np.sort(local[:160])) and not np.array_equal(order, local)


def test_three_full_slices_are_left_unscheduled():
    idx, mask = _table(127, 6)
    assert np.array_equal(R.tile_order_ref(idx, mask, 4), np.argsort(R.tile_key(idx, mask, 4), kind="stable"))
    idx, mask = _table(128, 6)      # four full slices: scheduled
    assert not np.array_equal(R.tile_order_ref(idx, mask, 4), np.argsort(R.tile_key(idx, mask, 4), kind="stable"))


def test_pack_and_mask_helpers():
    nbr = np.array([[0, -1, 2], [-1, -1, 1]], dtype=np.int32)
    assert R.pack_ref(nbr, np.array([2, 0, 1], dtype=np.int32)).tolist() == [[2, 0, -1], [1, -1, -1]]
    assert R.mask_of_nbr(nbr).tolist() == [1, 0, 3]
    assert R.pack_ref(np.zeros((8, 0), dtype=np.int32), np.zeros(0, dtype=np.int32)).shape == (8, 0)
