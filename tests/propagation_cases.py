"""Inputs of tests/test_gpu_propagation_edges.py (label propagation, csrc/affinity.hip a17), made here so that
tests/test_propagation_cases_host.py can check on any machine that every one of them still reaches the kernel branch it is
named after.  Every builder returns ``(Case, branches)``: ``Case`` = (eu, ev, aff float32, adjacency, pred, conf, label,
class_num) and ``branches`` names what the case is for.

Two kinds.  EXACT cases: every affinity, row sum and transition entry is k / 2^q with q * (iterations + 1) <= 52, so a
float64 sum of such terms is exact in any order -- device (both forms) and oracle/affinity_ref.py must agree bit for bit,
and equal scores (ties) are equal on every side.  TOLERANCED cases: random float32 affinities, compared at the bound of
tests/test_gpu_ops.py; their seed is chosen so that in every column the best score beats the runner-up by a relative gap
of more than 1e-8 (within each class and across classes), so a summation order cannot flip an argmax.

``chain`` is a second statement of the operator, independent of affinity_ref: the row-vector products
x_{i+1} = x_i T0_c of the labelled rows only, k ascending -- what the sparse kernels compute."""
import functools
from collections import namedtuple

import numpy as np

from oracle import affinity_ref

Case = namedtuple("Case", "eu ev aff adjacency pred conf label class_num")
THR = np.float32(0.7)
THR_UP = np.nextafter(np.float32(0.7), np.float32(1))
ITERATIONS = (0, 1, 2, 3)
GAP = 1e-8
RTOL, ATOL = 1e-10, 1e-14       # the operator's bound on scores (tests/test_gpu_ops.py::test_label_propagation)
UNLABELLED = -100


def _case(eu, ev, aff, adjacency, pred, conf, label, class_num):
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    aff = np.asarray(aff, dtype=np.float32)
    assert eu.shape == ev.shape == aff.shape and (aff >= 0).all()
    S = len(pred)
    assert np.asarray(adjacency).shape == (S, S) and len(conf) == S and len(label) == S
    return Case(eu, ev, aff, np.asarray(adjacency, dtype=np.int64), np.asarray(pred, dtype=np.int64),
                np.asarray(conf, dtype=np.float32), np.asarray(label, dtype=np.int64), int(class_num))


def _adjacency(S, eu, ev):
    adj = np.zeros((S, S), dtype=np.int64)
    off = eu != ev
    adj[eu[off], ev[off]] = 1
    return adj


def _symmetric(pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    both = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0)
    return both[:, 0], both[:, 1]


# ---- the operator, stated a second time -------------------------------------------------------------------------------
def stored_entries(case):
    """the non-zeros of W0 = A * (adjacency + I), row-major (k, then j ascending): the CSR the sparse form builds"""
    S = len(case.pred)
    A = np.zeros((S, S))
    A[case.eu, case.ev] = case.aff.astype(np.float64)        # (repeated pairs carry equal values)
    W = A * (case.adjacency + np.eye(S, dtype=np.int64))
    k, j = np.nonzero(W)
    return k, j, W[k, j]


def chain(case, iterations):
    """{class: (scores [S], arg [S], X [rows, S], rows)} for the labelled classes: X[i] = row rows[i] of T0_c^(iterations+1)"""
    S = len(case.pred)
    k, j, w = stored_entries(case)
    out = {}
    for c in range(case.class_num):
        rows = np.flatnonzero(case.label == c)
        if rows.size == 0:
            continue
        m = (case.pred == c) & (case.conf > THR)
        wc = np.where((m[k] & m[j]) | ((k == j) & (case.label[k] == c)), w, 0.0)
        d = np.bincount(k, weights=wc, minlength=S)          # (adds in entry order: the columns of a row, ascending)
        d[d == 0] = 1.0
        t = wc / d[k]
        X = np.zeros((rows.size, S))
        for i, r in enumerate(rows):
            x = np.zeros(S)
            x[j[k == r]] = t[k == r]
            for _ in range(iterations):
                x = np.bincount(j, weights=x[k] * t, minlength=S)        # k ascending within every column
            X[i] = x
        best = X.max(axis=0)                                 # (affinities are >= 0, and so is every score)
        out[c] = (best, np.where(best > 0, rows[X.argmax(axis=0)], 0), X, rows)
    return out


def merge(per_class, label):
    """(final, scores, pseudo) of scannetv2_dataset.py:722-736 from {class: (scores, arg, ...)}: first present class wins"""
    S = len(label)
    if not per_class:
        return np.full(S, float(UNLABELLED)), np.zeros(S), np.zeros(S, dtype=np.int64)
    classes = sorted(per_class)
    sc = np.stack([per_class[c][0] for c in classes])
    ar = np.stack([np.asarray(per_class[c][1], dtype=np.int64) for c in classes])
    ind = np.argmax(sc, axis=0)[None]
    scores, pseudo = np.take_along_axis(sc, ind, 0)[0], np.take_along_axis(ar, ind, 0)[0]
    final = np.full(S, float(UNLABELLED))
    unknown = (scores != 0) & (np.asarray(label) == UNLABELLED)
    final[unknown] = pseudo[unknown]
    return final, scores, pseudo


def gap_ok(case, iterations):
    """True when, for every column with a non-zero score, the best score beats the runner-up by a relative gap of more
    than GAP: among the labelled rows of each class, and among the classes"""
    pc = chain(case, iterations)
    for best, _, X, _ in pc.values():
        if X.shape[0] > 1:
            second = np.partition(X, -2, axis=0)[-2]
            if not (((best - second) > GAP * best) | (best == 0)).all():
                return False
    if len(pc) > 1:
        sc = np.sort(np.stack([v[0] for v in pc.values()]), axis=0)
        if not (((sc[-1] - sc[-2]) > GAP * sc[-1]) | (sc[-1] == 0)).all():
            return False
    return True


def _pick_seed(build, first_seed):
    """the first seed from ``first_seed`` on whose case has the gap at every iteration count"""
    for seed in range(first_seed, first_seed + 32):
        case, branches = build(seed)
        if all(gap_ok(case, it) for it in ITERATIONS):
            return case, dict(branches, seed=seed)
    raise AssertionError("no seed with a score gap")


# ---- the reference --------------------------------------------------------------------------------------------------
def reference_call(case, iterations):
    """oracle/affinity_ref.py on a case -> (final, scores, {class: (scores, arg, T0)}); the reference's code has no
    answer for a scene without any label (np.argmax of nothing): nothing is propagated there"""
    S = len(case.pred)
    if not any((case.label == c).any() for c in range(case.class_num)):
        return np.full(S, float(UNLABELLED)), np.zeros(S), {}
    A = affinity_ref.affinity_matrix(case.eu, case.ev, case.aff, S)
    return affinity_ref.weak_label_propagation(A, case.adjacency, case.conf, case.pred, case.label, iterations,
                                               case.class_num)


@functools.lru_cache(maxsize=None)
def reference(name, iterations):
    """computed once per (case, iterations) and shared: (final, scores, {class: (scores, arg)}); read only"""
    final, scores, per_class = reference_call(get(name)[0], iterations)
    out = (final, scores, {c: (v[0], v[1]) for c, v in per_class.items()})
    for a in (final, scores) + tuple(x for v in out[2].values() for x in v):
        a.setflags(write=False)
    return out


def reference_power(case, iterations, reverse=False):
    """{class: T0_c^(iterations + 1)} from the reference's T0_c, the products added one k at a time (ascending, or
    descending with ``reverse``); for the small exact cases"""
    out = {}
    for c, (_, _, t) in reference_call(case, 0)[2].items():
        T = t
        order = range(len(t) - 1, -1, -1) if reverse else range(len(t))
        for _ in range(iterations):
            acc = np.zeros_like(T)
            for k in order:
                acc += T[:, k:k + 1] * t[k:k + 1, :]
            T = acc
        out[c] = T
    return out


# ---- exact cases ----------------------------------------------------------------------------------------------------
def torus(n=8):
    """4-neighbour n x n torus, every affinity 1/4, one class, all confident, labels at 0, 2 and n*n - 1: row sums 1,
    T0 entries 1/4, symmetric neighbourhoods -> tied columns at every iteration count"""
    S = n * n
    idx = np.arange(S).reshape(n, n)
    pairs = np.concatenate([np.stack([idx.ravel(), np.roll(idx, s, axis=a).ravel()], 1) for a in (0, 1) for s in (1, -1)])
    eu, ev = _symmetric(pairs)
    label = np.full(S, UNLABELLED)
    label[[0, 2, S - 1]] = 0
    case = _case(eu, ev, np.full(len(eu), 0.25), _adjacency(S, eu, ev), np.zeros(S), np.full(S, 0.9), label, 1)
    return case, {"exact": True, "q": 2, "tied": True, "row_entries": [4], "s_mod_64": S % 64, "s_mod_4": S % 4}


def bipartite(m):
    """complete bipartite K(m, m), every affinity 2^-3, one class, labels at 1, 5 and m + 3: every row stores exactly m
    entries (m = 64: one full chunk of the 64-entry walks; m = 128: two), rows 1 and 5 are equal -> half of all columns tie"""
    S = 2 * m
    left, right = np.meshgrid(np.arange(m), np.arange(m, S), indexing="ij")
    eu, ev = _symmetric(np.stack([left.ravel(), right.ravel()], 1))
    label = np.full(S, UNLABELLED)
    label[[1, 5, m + 3]] = 0
    case = _case(eu, ev, np.full(len(eu), 0.125), _adjacency(S, eu, ev), np.zeros(S), np.full(S, 0.9), label, 1)
    q = int(np.log2(m))
    return case, {"exact": True, "q": q, "tied": True, "row_entries": [m], "s_mod_64": 0, "s_mod_4": 0}


def components():
    """disjoint components, one per class (S = 35; S % 4 = 3, one ragged 64-column step):
      0..7    8-cycle of class 0, labels at 0 and 4 (columns 2 and 6 are equally far from both: ties within the class)
      8..15   8-cycle of class 1, labels at 8 and 10;  16..23 its mirror image in class 2, labels at 16 and 18
      24, 25  24 is labelled 1, predicted 2, with a self edge; 25 is labelled 2 and its only entry leads to 24: column 24
              scores exactly 1 in class 1 (row 24) and in class 2 (row 25) at every iteration count -- a tie ACROSS classes,
              the first present class (1) wins.  (A column without a label can only score in the class it is predicted as,
              so a non-zero tie across classes needs a labelled column; it shows in the scores and the merged pseudo
              label, `final` keeps the given label there.)
      26      isolated, labelled 3, unconfident, self edge 1/2: only the diagonal clause keeps its row alive
      27      isolated, labelled 3, no self edge: row sum 0
      28..30  isolated, unlabelled: row sum 0 in every class
      31..34  a path predicted 4, a class that is never labelled"""
    S = 35
    pairs, affs = [], []

    def cycle(first, a):
        for i in range(8):
            for s in (1, -1):
                pairs.append((first + i, first + (i + s) % 8))
                affs.append(a)
    cycle(0, 0.5)
    cycle(8, 0.25)
    cycle(16, 0.25)
    pairs += [(24, 24), (25, 24), (26, 26), (31, 32), (32, 31), (32, 33), (33, 32), (33, 34), (34, 33)]
    affs += [0.5, 0.5, 0.5, 0.25, 0.25, 0.5, 0.5, 0.25, 0.25]
    eu, ev = np.array(pairs).T
    adj = _adjacency(S, eu, ev)
    adj[24, 25] = adj[25, 24] = 1
    pred = np.zeros(S, dtype=np.int64)
    pred[8:16], pred[16:24], pred[24:26], pred[26:28], pred[28:31], pred[31:35] = 1, 2, 2, 3, 0, 4
    conf = np.full(S, 0.9)
    conf[26:31] = 0.5
    label = np.full(S, UNLABELLED)
    label[[0, 4]], label[[8, 10, 24]], label[[16, 18, 25]], label[[26, 27]] = 0, 1, 2, 3
    case = _case(eu, ev, affs, adj, pred, conf, label, 5)
    return case, {"exact": True, "q": 1, "tied": True, "tied_across": True, "zero_rows": 4, "self_edge_rows": [24, 26],
                  "s_mod_64": 35, "s_mod_4": 3, "never_labelled": [4]}


# ---- toleranced cases -----------------------------------------------------------------------------------------------
def _random_pairs(rng, S, per_node=4):
    if S == 1:
        return np.array([[0, 0]])
    u = np.repeat(np.arange(S), per_node)
    v = (u + rng.randint(1, max(2, min(25, S)), u.size) * rng.choice([-1, 1], u.size)) % S       # neighbours are near in index
    return np.stack([u, v], 1)[u != v]


def _coherent_pred(rng, S, classes, noise=0.15):
    """predictions in ``classes`` runs along the index with some noise: neighbours mostly agree, as in a scene, so that few
    rows keep a single entry (two labelled rows that each keep only the same one column would tie at exactly 1)"""
    pred = np.arange(S) * classes // S
    flip = rng.random_sample(S) < noise
    pred[flip] = rng.randint(0, classes, flip.sum())
    return pred


SIZES = {1: 3, 2: 3, 63: 4, 64: 5, 65: 6, 255: 3, 257: 4, 1023: 3, 1024: 4, 1025: 3, 2049: 4}     # S -> classes


def sized(S):
    """symmetric random graph of about 8 neighbours, SIZES[S] classes, about 10 % labelled; S = 2049 keeps two present
    classes (the numpy reference multiplies S x S matrices per class).  S = 1: one labelled superpoint with a self edge"""
    classes = SIZES[S]

    def build(seed):
        rng = np.random.RandomState(seed)
        eu, ev = _symmetric(_random_pairs(rng, S))
        aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.01)
        pred = _coherent_pred(rng, S, classes)
        conf = (0.45 + 0.55 * rng.random_sample(S)).astype(np.float32)
        pool = np.flatnonzero(pred < 2) if S == 2049 else np.arange(S)
        ids = rng.choice(pool, max(1, S // 10), replace=False)
        label = np.full(S, UNLABELLED)
        label[ids] = pred[ids]
        conf[ids[::2]] = 0.95
        return _case(eu, ev, aff, _adjacency(S, eu, ev), pred, conf, label, classes), \
            {"exact": False, "s_mod_64": S % 64, "s_mod_4": S % 4, "scan_per": -(-S // 1024)}
    return _pick_seed(build, S)


HUB_ENTRIES = (63, 64, 65, 129)


def hubs():
    """S = 300: hubs 0..3 with 63, 64, 65 and 129 stored entries on a sparse graph; hubs 0 (class 0) and 1 (class 1) are
    adjacent, so are 2 (class 0) and 3 (class 1); the hubs' neighbours are of three classes and about half confident, so
    part of every hub row is masked out.  Hubs 0 and 3 are labelled (the first fill of a row vector walks them), hubs 1
    and 2 are reached from a labelled neighbour (the chain walks them)"""
    S = 300

    def build(seed):
        rng = np.random.RandomState(seed)
        rest = np.arange(4, S)
        pairs = [rest[_random_pairs(rng, S - 4, 2)]]
        pairs.append(np.array([[0, 1], [2, 3]]))
        for h, n in enumerate(HUB_ENTRIES):
            pairs.append(np.stack([np.full(n - 1, h), rng.choice(rest, n - 1, replace=False)], 1))
        eu, ev = _symmetric(np.concatenate(pairs))
        aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.01)
        pred = rng.randint(0, 3, S)
        pred[:4] = (0, 1, 0, 1)
        conf = (0.4 + 0.6 * rng.random_sample(S)).astype(np.float32)
        conf[:4] = 0.9
        label = np.full(S, UNLABELLED)
        ids = rng.choice(rest, 24, replace=False)
        label[ids] = pred[ids]
        label[0], label[3] = 0, 1
        for h in (1, 2):            # a labelled, confident neighbour of the hub's class
            nb = ev[(eu == h) & (ev >= 4)]
            nb = nb[pred[nb] == pred[h]][0]
            label[nb], conf[nb] = pred[h], 0.9
        return _case(eu, ev, aff, _adjacency(S, eu, ev), pred, conf, label, 3), \
            {"exact": False, "row_entries": list(HUB_ENTRIES), "s_mod_64": S % 64, "s_mod_4": S % 4}
    return _pick_seed(build, 300)


BOUNDARY = {"at": 40, "above": 41, "labelled_at": 46}       # conf == float32(0.7), one ulp above, and 0.7 on a labelled row


def boundary():
    """S = 48: a random graph on 0..39 and three gadgets.  A labelled, confident pair (44, 45, class 0) and a boundary
    superpoint b joined to both, with a tail superpoint behind b; the triangle makes walks of every length reach b.  b = 40
    has conf == float32(0.7): masked out, b and its tail 42 stay unlabelled.  b = 41 is one ulp above: kept, 41 and (from
    one iteration on) its tail 43 take a label.  46 is LABELLED 0 with conf == float32(0.7) and a self edge, and is the only
    neighbour of 47: as a row it keeps its diagonal alone, so 47 stays unlabelled (one ulp more and 47 takes label 46)."""
    S = 48

    def build(seed):
        rng = np.random.RandomState(seed)
        pairs = [_random_pairs(rng, 40, 3)]
        pairs.append(np.array([[44, 45], [44, 40], [45, 40], [40, 42], [44, 41], [45, 41], [41, 43], [46, 46], [46, 47]]))
        eu, ev = _symmetric(np.concatenate(pairs))
        aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.01)
        pred = rng.randint(0, 3, S)
        pred[40:] = 0
        conf = (0.4 + 0.6 * rng.random_sample(S)).astype(np.float32)
        conf[40:] = 0.9
        conf[BOUNDARY["at"]], conf[BOUNDARY["above"]], conf[BOUNDARY["labelled_at"]] = THR, THR_UP, THR
        label = np.full(S, UNLABELLED)
        ids = rng.choice(40, 5, replace=False)
        label[ids] = pred[ids]
        label[44] = label[45] = label[46] = 0
        return _case(eu, ev, aff, _adjacency(S, eu, ev), pred, conf, label, 3), \
            {"exact": False, "boundary": dict(BOUNDARY), "self_edge_rows": [46], "s_mod_64": S % 64, "s_mod_4": S % 4}
    return _pick_seed(build, 46)


def present_zeros():
    """S = 50: zero affinity on present edges (the CSR drops them, the dense form keeps a 0), adjacency counts of 2, 3 and
    255, a self edge on a masked-out row (7: unlabelled, unconfident) and one on a labelled row (11)"""
    S = 50

    def build(seed):
        rng = np.random.RandomState(seed)
        eu, ev = _symmetric(np.concatenate([_random_pairs(rng, S), [[7, 7], [11, 11]]]))
        aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.01)
        off = np.flatnonzero(eu != ev)
        zero = rng.choice(off, 12, replace=False)
        aff[zero] = 0.0
        adj = _adjacency(S, eu, ev)
        counted = rng.choice(np.setdiff1d(off, zero), 9, replace=False)
        adj[eu[counted], ev[counted]] = np.tile([2, 3, 255], 3)
        adj[eu[zero[0]], ev[zero[0]]] = 255                 # a count on a zero affinity: still nothing stored
        pred = rng.randint(0, 3, S)
        conf = (0.5 + 0.5 * rng.random_sample(S)).astype(np.float32)
        conf[7] = 0.3
        label = np.full(S, UNLABELLED)
        ids = np.setdiff1d(rng.choice(S, 8, replace=False), [7])
        label[ids] = pred[ids]
        label[11], conf[11] = pred[11], 0.9
        return _case(eu, ev, aff, adj, pred, conf, label, 3), \
            {"exact": False, "zero_affinities": 12, "counts": [2, 3, 255], "self_edge_rows": [7, 11],
             "s_mod_64": S % 64, "s_mod_4": S % 4}
    return _pick_seed(build, 50)


def class_table():
    """S = 61, class_num = 5: class 0 and 3 ordinary, class 1 predicted and never labelled, class 2 labelled while every
    superpoint predicted 2 is unconfident (its rows are zero: the class is present and scores 0), and one superpoint
    carries the label class_num + 3 (no class: it is neither propagated from nor overwritten)"""
    S, classes = 61, 5

    def build(seed):
        rng = np.random.RandomState(seed)
        eu, ev = _symmetric(_random_pairs(rng, S))
        aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.01)
        pred = rng.choice([0, 1, 2, 3], S)
        conf = (0.5 + 0.5 * rng.random_sample(S)).astype(np.float32)
        conf[pred == 2] = 0.6
        label = np.full(S, UNLABELLED)
        for c in (0, 2, 3):
            ids = rng.choice(np.flatnonzero(pred == c), 3, replace=False)
            label[ids] = c
        label[np.flatnonzero(label == UNLABELLED)[5]] = classes + 3
        return _case(eu, ev, aff, _adjacency(S, eu, ev), pred, conf, label, classes), \
            {"exact": False, "never_labelled": [1, 4], "all_unconfident": [2], "label_out_of_range": classes + 3,
             "n_present": 3, "s_mod_64": S % 64, "s_mod_4": S % 4}
    return _pick_seed(build, 61)


def one_present(labelled=True):
    """S = 30, three predicted classes, labels of class 1 only (n_present = 1) -- or, ``labelled=False``, no label at all"""
    S = 30

    def build(seed):
        rng = np.random.RandomState(seed)
        eu, ev = _symmetric(_random_pairs(rng, S))
        aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.01)
        pred = rng.randint(0, 3, S)
        conf = (0.6 + 0.4 * rng.random_sample(S)).astype(np.float32)
        label = np.full(S, UNLABELLED)
        if labelled:
            label[rng.choice(np.flatnonzero(pred == 1), 3, replace=False)] = 1
        return _case(eu, ev, aff, _adjacency(S, eu, ev), pred, conf, label, 3), \
            {"exact": False, "n_present": int(labelled), "s_mod_64": S % 64, "s_mod_4": S % 4}
    return _pick_seed(build, 30)


BUILDERS = {"torus8": torus, "bipartite64": functools.partial(bipartite, 64), "bipartite128": functools.partial(bipartite, 128),
            "components": components}
BUILDERS.update({"S%d" % S: functools.partial(sized, S) for S in SIZES})
BUILDERS.update({"hubs": hubs, "boundary": boundary, "present_zeros": present_zeros, "class_table": class_table,
                 "one_present": one_present, "no_label": functools.partial(one_present, False)})
NAMES = tuple(BUILDERS)
EXACT = ("torus8", "bipartite64", "bipartite128", "components")
TOLERANCED = tuple(n for n in NAMES if n not in EXACT)


@functools.lru_cache(maxsize=None)
def get(name):
    """(Case, branches) of a named case, built once; the arrays are read only"""
    case, branches = BUILDERS[name]()
    for a in case[:7]:
        a.setflags(write=False)
    return case, branches
