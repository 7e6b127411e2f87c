"""Inputs of tests/test_gpu_rulebook_build.py, made here so that tests/test_rulebook_build_ref_host.py can check on any
machine that every one of them still reaches the branch of csrc/rulebook.hip it is named after.  Every builder returns
int32 [M, 4] rows (batch, x, y, z), unique, inside the shape, in an order that is not the linear one, and asserts its
own precondition."""
import functools

import numpy as np

import rulebook_ref as R

BM_CHUNK_WORDS = 1024           # words of the output bitmap one workgroup counts (csrc/rulebook.hip BM_WORDS_PER_WG)


def _rows(batch, coords):
    return np.concatenate([np.asarray(batch, dtype=np.int64).reshape(-1, 1), np.asarray(coords, dtype=np.int64)], 1) \
        .astype(np.int32)


def _shuffled(idx, seed):
    idx = np.asarray(idx, dtype=np.int32)
    assert np.unique(idx, axis=0).shape[0] == idx.shape[0], "rows must be unique"
    return np.ascontiguousarray(idx[np.random.RandomState(seed).permutation(idx.shape[0])])


def bitmap_chunks(out_shape, batch_size):
    cells = int(batch_size) * int(out_shape[0]) * int(out_shape[1]) * int(out_shape[2])
    words = (cells + 31) // 32
    return cells, words, (words + BM_CHUNK_WORDS - 1) // BM_CHUNK_WORDS


@functools.lru_cache(maxsize=None)
def random_rows(shape, n_batch, density, seed):
    rng = np.random.RandomState(seed)
    occ = np.argwhere(rng.random_sample((n_batch,) + tuple(shape)) < density)
    assert occ.shape[0] > 0
    return _shuffled(occ, seed + 1)


@functools.lru_cache(maxsize=None)
def block_rows(shape, n_batch=1, seed=5):
    """every cell of ``shape`` in every batch item"""
    return _shuffled(np.argwhere(np.ones((n_batch,) + tuple(shape), dtype=bool)), seed)


# ---- hash probing: wrap from the last slot to slot 0, collision-then-found, collision-then-miss ----------------------
WRAP_SHAPE, WRAP_BATCH = (9, 8, 7), 2


def probe_facts(idx, shape, cap):
    """what the k3 p1 lookups of these rows meet in a table of ``cap`` slots: ``last`` = keys whose first slot is
    cap - 1; ``miss_after_collision`` = queried in-shape neighbour keys that are absent while their first slot holds
    another key; ``found_later`` = pairs of present keys with one first slot that are both queried by a neighbouring row
    (only one of the two can sit in that slot: the other lookup succeeds behind a collision)"""
    idx = np.asarray(idx, dtype=np.int64)
    keys = [int(v) for v in R.lin_keys(idx, shape)]
    present = set(keys)
    taken = R.occupied_slots(keys, cap)
    queried_hit, miss = set(), 0
    for b, x, y, z in idx.tolist():
        for a in (-1, 0, 1):
            for c in (-1, 0, 1):
                for d in (-1, 0, 1):
                    q = (x + a, y + c, z + d)
                    if (a, c, d) == (0, 0, 0) or not all(0 <= q[j] < shape[j] for j in range(3)):
                        continue
                    key = int(R.lin_keys(np.array([[b, q[0], q[1], q[2]]]), shape)[0])
                    if key in present:
                        queried_hit.add(key)
                    elif R.home_slot(key, cap) in taken:
                        miss += 1
    homes = {}
    for key in sorted(queried_hit):
        homes.setdefault(R.home_slot(key, cap), []).append(key)
    return {"last": sum(R.home_slot(k, cap) == cap - 1 for k in keys), "miss_after_collision": miss,
            "found_later": sum(len(v) - 1 for v in homes.values()),
            # queried keys of the last slot beyond the one that can sit in it: found at slot 0 .. through the wrap
            "found_through_wrap": max(len(homes.get(cap - 1, [])) - 1, 0)}


@functools.lru_cache(maxsize=None)
def wrap_rows(M):
    """M rows in WRAP_SHAPE x WRAP_BATCH of which min(M, 3) have the LAST slot of the table as their first slot (all but
    one of them are stored at slots 0, 1: probing wraps), with a collision-then-miss lookup and, from two rows on, a
    collision-then-found one"""
    cap = R.pow2_cap(M)
    cells = np.argwhere(np.ones((WRAP_BATCH,) + WRAP_SHAPE, dtype=bool))
    keys = R.lin_keys(cells, WRAP_SHAPE)
    last = cells[[R.home_slot(int(k), cap) == cap - 1 for k in keys]]
    n_last = min(M, 3)
    assert last.shape[0] >= n_last
    # two of them next to each other where the grid has such a pair: each row then looks the other one up, and only one of
    # the two can sit in the last slot
    near = [(i, j) for i in range(last.shape[0]) for j in range(i + 1, last.shape[0])
            if last[i, 0] == last[j, 0] and np.abs(last[i, 1:] - last[j, 1:]).max() <= 1]
    for seed in range(400):
        rng = np.random.RandomState(seed)
        first = list(near[rng.randint(len(near))]) if near and M >= 2 else []
        others = [i for i in rng.permutation(last.shape[0]).tolist() if i not in first]
        pick = last[(first + others)[:n_last]]
        rows = {tuple(r) for r in pick.tolist()}
        # a neighbour next to each of them (so that their keys are queried), then anything
        for b, x, y, z in pick.tolist():
            if len(rows) >= M:
                break
            q = (b, min(x + 1, WRAP_SHAPE[0] - 1), y, max(z - 1, 0))
            rows.add(q)
        for r in cells[rng.permutation(cells.shape[0])].tolist():
            if len(rows) >= M:
                break
            rows.add(tuple(r))
        idx = np.array(sorted(rows), dtype=np.int32)
        if idx.shape[0] != M:
            continue
        f = probe_facts(idx, WRAP_SHAPE, cap)
        if f["last"] >= n_last and f["miss_after_collision"] >= 1 and (M < 2 or f["found_through_wrap"] >= 1):
            return _shuffled(idx, seed)
    raise AssertionError("no input of %d rows reaches the probing branches" % M)


def _queried_keys(idx, shape):
    """keys of present rows that a k3 p1 lookup of another present row asks for"""
    idx = np.asarray(idx, dtype=np.int64)
    present = {tuple(r) for r in idx.tolist()}
    out = set()
    for b, x, y, z in idx.tolist():
        for a in (-1, 0, 1):
            for c in (-1, 0, 1):
                for d in (-1, 0, 1):
                    q = (b, x + a, y + c, z + d)
                    if (a, c, d) != (0, 0, 0) and q in present:
                        out.add(int(R.lin_keys(np.array([q]), shape)[0]))
    return out


@functools.lru_cache(maxsize=None)
def wrap_in_loop_rows():
    """The wrap INSIDE the probing loop: three keys whose first slot is cap - 2 and nobody else near the end of the table
    occupy slots cap - 2, cap - 1 and 0 whatever the order of insertion, so the key in slot 0 is found by a lookup that
    starts at cap - 2, goes on at cap - 1 and steps from there to slot 0.  Each of the three has a neighbour that looks
    it up.  (With the keys of ``wrap_rows`` the first slot is cap - 1 itself: the step to slot 0 is the first one.)"""
    cells = np.argwhere(np.ones((WRAP_BATCH,) + WRAP_SHAPE, dtype=bool))
    keys = R.lin_keys(cells, WRAP_SHAPE)
    cap = 16
    home = np.array([R.home_slot(int(k), cap) for k in keys])
    three_from = cells[home == cap - 2]
    quiet = cells[(home >= 2) & (home <= 8)]              # neighbours whose own probing stays away from the table's end
    for seed in range(400):
        rng = np.random.RandomState(seed)
        three = three_from[rng.permutation(three_from.shape[0])[:3]]
        rows = {tuple(r) for r in three.tolist()}
        for r in three:
            near = quiet[(quiet[:, 0] == r[0]) & (np.abs(quiet[:, 1:] - r[1:]).max(1) == 1)]
            if near.shape[0]:
                rows.add(tuple(near[rng.randint(near.shape[0])].tolist()))
        idx = np.array(sorted(rows), dtype=np.int32)
        if idx.shape[0] > 8 or R.pow2_cap(idx.shape[0]) != cap:
            continue
        all_keys = [int(k) for k in R.lin_keys(idx, WRAP_SHAPE)]
        mine = [k for k in all_keys if R.home_slot(k, cap) == cap - 2]
        others = [k for k in all_keys if R.home_slot(k, cap) != cap - 2]
        end = {cap - 2, cap - 1, 0}
        if len(mine) == 3 and not (R.occupied_slots(others, cap) & end) and end <= R.occupied_slots(all_keys, cap) \
                and set(mine) <= _queried_keys(idx, WRAP_SHAPE):
            return _shuffled(idx, seed)
    raise AssertionError("no input reaches the wrap inside the probing loop")


# ---- linear keys above 2^31 and 2^32 ---------------------------------------------------------------------------------
BIG_SHAPE = (2048, 2048, 1024)


@functools.lru_cache(maxsize=None)
def big_key_rows():
    """2,000 rows: eight 5 x 5 x 5 clusters per batch item (0 and 1) in the far corner of BIG_SHAPE, one of them touching
    shape - 1 on every axis; odd and even cluster origins (k2 s2 merges them differently)"""
    rng = np.random.RandomState(77)
    origins = [(2043, 2043, 1019)] + [tuple(int(v) for v in (rng.randint(1500, 2040), rng.randint(0, 2040),
                                                              rng.randint(0, 1016))) for _ in range(7)]
    cell = np.argwhere(np.ones((5, 5, 5), dtype=bool))
    rows = [_rows(np.full(125, b), cell + np.asarray(o)) for b in (0, 1) for o in origins]
    idx = _shuffled(np.unique(np.concatenate(rows), axis=0), 78)
    keys = R.lin_keys(idx, BIG_SHAPE)
    assert idx.shape[0] >= 1900
    assert int(keys[idx[:, 0] == 0].min()) > 1 << 31 and int(keys[idx[:, 0] == 0].max()) < 1 << 32
    assert int(keys[idx[:, 0] == 1].min()) > 1 << 32
    assert np.all(idx[:, 1:].max(0) == np.asarray(BIG_SHAPE) - 1)
    out_shape = R.out_shape_of(BIG_SHAPE, 2, 2, 0)
    assert bitmap_chunks(out_shape, 16)[0] > 1 << 31, "batch_size 16: more output cells than the bitmap form takes"
    assert int(R.lin_keys(R.down_tables(idx, BIG_SHAPE, 2, 2, 0)[0], out_shape).max()) > 1 << 29
    return idx


# ---- M_out == 0: every voxel on the odd last plane that k2 s2 drops --------------------------------------------------
@functools.lru_cache(maxsize=None)
def dropped_plane_rows(n_batch=2):
    """shape (3, 3, 3): the cells with coordinate 2 on some axis (output shape (1, 1, 1): none of them has an output)"""
    cells = np.argwhere(np.ones((n_batch, 3, 3, 3), dtype=bool))
    idx = _shuffled(cells[(cells[:, 1:] == 2).any(1)], 9)
    assert R.down_tables(idx, (3, 3, 3), 2, 2, 0)[0].shape[0] == 0
    return idx


# ---- pyramids --------------------------------------------------------------------------------------------------------
ODD_SHAPE = (37, 30, 23)            # (18, 15, 11) -> (9, 7, 5): an odd plane is dropped on two levels


@functools.lru_cache(maxsize=None)
def odd_pyramid_rows():
    idx = random_rows(ODD_SHAPE, 3, 0.15, 31)
    assert (idx[:, 1] == 36).any() and (idx[:, 3] == 22).any()      # rows on the dropped planes of level 0
    return idx


@functools.lru_cache(maxsize=None)
def block20_rows():
    """one (20, 20, 20) block at the origin of (64, 64, 64): 8,000 / 1,000 / 125 / 27 / 8 rows, and 1 on a sixth level"""
    idx = block_rows((20, 20, 20), 1, 41)
    return idx


@functools.lru_cache(maxsize=None)
def box_rows(n_batch, seed):
    """about 1,000 rows per batch item inside a (20, 18, 14) box at the origin, whatever the shape around it"""
    return random_rows((20, 18, 14), n_batch, 0.2, seed)


FORM_SHAPES = [(20, 18, 14), (40, 36, 28), (80, 72, 56), (160, 144, 112), (320, 288, 224), BIG_SHAPE]


@functools.lru_cache(maxsize=None)
def cells45_rows():
    """output grid (5, 3, 3) x 1 = 45 cells: a bit count that is no multiple of 32, 2 words (no multiple of 4)"""
    shape = (11, 6, 7)
    idx = random_rows(shape, 1, 0.5, 51)
    cells, words, chunks = bitmap_chunks(R.out_shape_of(shape, 2, 2, 0), 1)
    assert (cells, words, chunks) == (45, 2, 1) and cells % 32 and words % 4
    return idx, shape


SHEET_SHAPE = (416, 416, 416)


@functools.lru_cache(maxsize=None)
def sheet_rows():
    """about 145,000 rows: a wavy sheet z(x, y) over 416 x 330 cells plus 8,000 scattered voxels.  Output grid 208^3 =
    8,998,912 cells = 281,216 words = 275 chunks of 1,024 words: the chunk-sum scan carries from its first pass of 256
    chunks into a second one"""
    x, y = np.meshgrid(np.arange(416), np.arange(330), indexing="ij")
    z = np.round(208 + 150 * np.sin(x / 37.0) * np.cos(y / 29.0)).astype(np.int64)
    sheet = np.stack([np.zeros(x.size, dtype=np.int64), x.ravel(), y.ravel(), z.ravel()], 1)
    rng = np.random.RandomState(61)
    extra = np.concatenate([np.zeros((8000, 1), dtype=np.int64), rng.randint(0, 416, (8000, 3))], 1)
    idx = _shuffled(np.unique(np.concatenate([sheet, extra]), axis=0), 62)
    cells, words, chunks = bitmap_chunks(R.out_shape_of(SHEET_SHAPE, 2, 2, 0), 1)
    assert 140000 <= idx.shape[0] <= 150000 and cells == 8998912 and chunks == 275 and chunks > 256
    # the level above occupies chunks behind the 256th: the carry is used, not only computed
    out = R.lin_keys(idx[:, [0, 1, 2, 3]] // np.array([1, 2, 2, 2]), (208, 208, 208))
    assert int(out.max()) >> 5 >= 256 * BM_CHUNK_WORDS
    return idx


@functools.lru_cache(maxsize=None)
def empty_level_rows():
    """three levels of shape (6, 6, 6) -> (3, 3, 3) -> (1, 1, 1): every level-0 voxel has a coordinate of 4 or 5 on some
    axis, so every level-1 voxel lies on the odd plane that the second k2 s2 drops: level 2 is empty"""
    cells = np.argwhere(np.ones((2, 6, 6, 6), dtype=bool))
    idx = cells[(cells[:, 1:] >= 4).any(1)]
    idx = _shuffled(idx[np.random.RandomState(71).random_sample(idx.shape[0]) < 0.6], 72)
    lv = R.pyramid(idx, (6, 6, 6), 3, 2, 4)
    assert lv[1]["indices"].shape[0] > 0 and lv[2]["indices"].shape[0] == 0
    return idx
