"""Label propagation (csrc/affinity.hip a17: dense_build, transition, dgemm, colmax and the six prop_* kernels of the
sparse form) against oracle/affinity_ref.py at every branch of the kernels: rows of 63 / 64 / 65 / 129 stored entries, the
one-workgroup scan at 1, 2 and 3 elements per thread, ragged 64-column ballot steps and ragged four-row workgroups, exact
ties (first row, first class wins), rows that the mask empties, the strict confidence threshold one ulp either side,
iterations 0..3, class-table edges, and the LDS attribute growing and then being reused by a small scene.

The inputs come from tests/propagation_cases.py; tests/test_propagation_cases_host.py proves on the host that they reach
those branches.  Exact cases (dyadic values: fp64 sums are exact in any order) are compared bit for bit; toleranced cases
at the operator's bound of tests/test_gpu_ops.py (rtol 1e-10, atol 1e-14 on scores, labels equal), their inputs chosen with a
1e-8 relative gap between the best and the second score so that no summation order flips an argmax."""
import functools

import numpy as np
import pytest
import torch

import propagation_cases as C
import wsis_ops
from oracle import affinity_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMS = pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
ITS = pytest.mark.parametrize("it", C.ITERATIONS)
CASES = pytest.mark.parametrize("name", C.NAMES)


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the cases' arrays are read only)


def _lib():
    import wsis_native as _n
    return _n, _n.hip()


@functools.lru_cache(maxsize=None)
def _device(name):
    """(A, adj_u8, pred, conf, label, present classes) of a case on the device, made once"""
    case, _ = C.get(name)
    S = len(case.pred)
    A = wsis_ops.affinity_matrix(_up(case.eu), _up(case.ev), _up(case.aff), S)
    present = [c for c in range(case.class_num) if (case.label == c).any()]
    return (A, wsis_ops.adjacency_u8(_up(case.adjacency), S, DEV), _up(case.pred).to(torch.int32), _up(case.conf),
            _up(case.label).to(torch.int32), present)


def _per_class(name, it, dense):
    """{class: (scores, arg)} straight from propagate_sparse / propagate_class: the rows the merge is made of"""
    A, adj, pred, conf, label, present = _device(name)
    if not present:
        return {}
    if dense:
        out = {c: wsis_ops.propagate_class(A, adj, pred, conf, label, c, it) for c in present}
    else:
        s, a = wsis_ops.propagate_sparse(A, adj, pred, conf, label, present, C.get(name)[0].class_num, it)
        assert s.shape == a.shape == (len(present), A.shape[0])
        out = {c: (s[i], a[i]) for i, c in enumerate(present)}
    return {c: (s.cpu().numpy(), a.cpu().numpy()) for c, (s, a) in out.items()}


def _same_scores(got, want, exact):
    if exact:
        return got.dtype == want.dtype == np.float64 and got.tobytes() == want.tobytes()
    return np.allclose(got, want, rtol=C.RTOL, atol=C.ATOL) and np.array_equal(got == 0, want == 0)


def _run(name, it, dense):
    case = C.get(name)[0]
    adjacency, conf, pred, label = (np.array(a) for a in (case.adjacency, case.conf, case.pred, case.label))     # (copies)
    return wsis_ops.weak_label_propagation(_device(name)[0], adjacency, conf, pred, label, it, case.class_num, dense=dense)


# ---------------------------------------------------------------- the cases
@CASES
def test_affinity_matrix_equals_the_reference_byte_for_byte(name):
    case, _ = C.get(name)
    S = len(case.pred)
    want = affinity_ref.affinity_matrix(case.eu, case.ev, case.aff, S)
    got = _device(name)[0].cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@FORMS
@ITS
@CASES
def test_propagation_gives_the_reference_labels_and_scores(name, it, dense):
    e_final, e_scores, _ = C.reference(name, it)
    final, scores = _run(name, it, dense)
    assert _same_scores(scores, e_scores, C.get(name)[1]["exact"])
    assert np.array_equal(final, e_final)


@FORMS
@ITS
@CASES
def test_every_class_row_matches_the_reference_not_only_the_merge(name, it, dense):
    case, br = C.get(name)
    _, _, e_pc = C.reference(name, it)
    got = _per_class(name, it, dense)
    assert sorted(got) == sorted(e_pc)
    for c, (e_scores, e_arg) in e_pc.items():
        scores, arg = got[c]
        assert _same_scores(scores, e_scores, br["exact"]), c
        assert np.array_equal(arg, e_arg), c                # first row among equal maxima
        unreached = e_scores == 0
        assert not scores[unreached].any() and not arg[unreached].any(), c
    if br.get("tied_across"):
        # column 24 scores 1 in class 1 (row 24) and in class 2 (row 25): the merge keeps the first present class
        assert got[1][0][24] == got[2][0][24] == 1.0 and (got[1][1][24], got[2][1][24]) == (24, 25)
        assert C.merge(got, case.label)[2][24] == C.merge(e_pc, case.label)[2][24] == 24


@FORMS
@ITS
@CASES
def test_two_calls_give_the_same_bytes(name, it, dense):
    """no atomics anywhere in the chain: scores and arguments repeat exactly"""
    first, second = _per_class(name, it, dense), _per_class(name, it, dense)
    for c in first:
        assert first[c][0].tobytes() == second[c][0].tobytes() and first[c][1].tobytes() == second[c][1].tobytes(), c


@pytest.mark.parametrize("name", ["S1", "S63", "S1023", "S1024", "S1025", "S2049", "components", "class_table"])
def test_sparse_form_reads_no_word_it_did_not_write(name):
    """the C entry on a workspace, CSR arrays and outputs filled with 0x7f bytes (ints of 2.1e9, doubles of 1.4e306): the
    scan's last threads (lo >= n), the two spare words behind the row counts, the rows of X that no wavefront owns and the
    CSR slots behind the last entry must never be read, so the poison cannot show in any score or argument"""
    _n, lib = _lib()
    case, br = C.get(name)
    A, adj, pred, conf, label, present = _device(name)
    S, n = A.shape[0], len(present)

    def poisoned(count, dtype):
        return torch.full((count * torch.empty(0, dtype=dtype).element_size(),), 0x7F, dtype=torch.uint8, device=DEV).view(dtype)
    cls_of = torch.tensor(present, dtype=torch.int32, device=DEV)
    ci = np.full(case.class_num, -1, dtype=np.int32)
    ci[present] = np.arange(n, dtype=np.int32)
    ci_of_cls = _up(ci)
    nnz = int(torch.count_nonzero(A))
    ws_bytes = lib.wsis_affinity_propagate_sparse_workspace_bytes(S, n)
    for it in (0, 2):
        col, val = poisoned(nnz + 64, torch.int32), poisoned(nnz + 64, torch.float64)
        scores, arg = poisoned(n * S, torch.float64), poisoned(n * S, torch.int32)
        ws = poisoned(ws_bytes, torch.uint8)
        _n.check(lib.wsis_affinity_propagate_sparse(_n.ptr(A), _n.ptr(adj), _n.ptr(pred), _n.ptr(conf), _n.ptr(label),
                                                    _n.ptr(cls_of), _n.ptr(ci_of_cls), n, case.class_num, 0.7, it, S,
                                                    _n.ptr(col), _n.ptr(val), nnz, _n.ptr(scores), _n.ptr(arg), _n.ptr(ws),
                                                    ws_bytes, _n.stream_ptr()), "affinity_propagate_sparse")
        got_s, got_a = scores.view(n, S).cpu().numpy(), arg.view(n, S).cpu().numpy()
        e_pc = C.reference(name, it)[2]
        for i, c in enumerate(present):
            assert _same_scores(got_s[i], e_pc[c][0], br["exact"]) and np.array_equal(got_a[i], e_pc[c][1]), (c, it)
        assert bool((col[nnz:] == 0x7F7F7F7F).all())           # nothing stored behind the last entry


# ---------------------------------------------------------------- dense_build
def _build(eu, ev, aff, S):
    return wsis_ops.affinity_matrix(_up(np.asarray(eu, dtype=np.int64)), _up(np.asarray(ev, dtype=np.int64)),
                                    _up(np.asarray(aff, dtype=np.float32)), S).cpu().numpy()


def test_dense_build_drops_out_of_range_endpoints():
    S = 10
    rng = np.random.RandomState(1)
    eu, ev = rng.randint(0, S, 40), rng.randint(0, S, 40)
    _, first = np.unique(eu * S + ev, return_index=True)        # (distinct pairs)
    eu, ev = eu[first], ev[first]
    aff = rng.random_sample(len(eu)).astype(np.float32) + np.float32(0.5)
    want = affinity_ref.affinity_matrix(eu, ev, aff, S)
    bad_u = np.array([-1, 3, S, 2, 2 ** 40, 1, -1, 2 ** 40])
    bad_v = np.array([3, -1, 2, S, 1, 2 ** 40, S, -1])
    order = rng.permutation(len(eu) + len(bad_u))
    got = _build(np.concatenate([eu, bad_u])[order], np.concatenate([ev, bad_v])[order],
                 np.concatenate([aff, np.full(len(bad_u), 7.0, dtype=np.float32)])[order], S)
    assert got.tobytes() == want.tobytes()
    assert not (got == 7.0).any()


def test_dense_build_without_edges_gives_zeros():
    for S in (1, 5, 65):
        got = _build([], [], [], S)
        assert got.shape == (S, S) and got.dtype == np.float64 and not got.any()


def test_dense_build_of_one_superpoint():
    got = _build([0], [0], [0.375], 1)
    assert got.tolist() == [[0.375]]


def test_dense_build_repeated_pairs_with_equal_values():
    """the graph build repeats a pair with the same softmax logits, so with the same value"""
    S = 7
    eu = np.array([0, 3, 0, 6, 3, 0, 6, 6])
    ev = np.array([1, 3, 1, 0, 3, 1, 0, 0])
    vals = {(0, 1): 0.3, (3, 3): 0.6, (6, 0): 0.9}
    aff = np.array([vals[p] for p in zip(eu.tolist(), ev.tolist())], dtype=np.float32)
    got = _build(eu, ev, aff, S)
    assert got.tobytes() == affinity_ref.affinity_matrix(eu, ev, aff, S).tobytes()
    assert np.count_nonzero(got) == 3


# ---------------------------------------------------------------- dgemm
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (1, 64, 1), (63, 65, 4), (64, 64, 16), (65, 63, 17), (129, 1, 3), (5, 5, 0)])
def test_dgemm_edges(M, N, K):
    """one element, one full tile, tiles with ragged rows / columns, a depth below, at and one past the 16-deep step, and
    no depth at all (C = 0)"""
    g = torch.Generator().manual_seed(M * 1000 + K)
    A, B = torch.randn(M, K, generator=g, dtype=torch.float64), torch.randn(K, N, generator=g, dtype=torch.float64)
    Cm = wsis_ops.dgemm(A.to(DEV), B.to(DEV))
    assert Cm.shape == (M, N)
    assert torch.allclose(Cm.cpu(), A @ B, rtol=1e-12, atol=1e-12)


def test_dgemm_with_no_depth_writes_zeros():
    """K = 0: A is [M, 0] and B is [0, N] (no storage at all), C = 0 must be WRITTEN, not left as allocated"""
    _n, lib = _lib()
    for M, N in ((5, 5), (65, 3)):
        Cm = torch.full((M, N), float("nan"), dtype=torch.float64, device=DEV)
        _n.check(lib.wsis_dgemm(None, None, _n.ptr(Cm), M, N, 0, _n.stream_ptr()), "dgemm")
        assert not Cm.cpu().numpy().any()
        via = wsis_ops.dgemm(torch.empty((M, 0), dtype=torch.float64, device=DEV),
                             torch.empty((0, N), dtype=torch.float64, device=DEV))
        assert via.shape == (M, N) and not via.cpu().numpy().any()


def test_dgemm_of_small_integers_is_exact():
    g = torch.Generator().manual_seed(9)
    A = torch.randint(-8, 9, (70, 37), generator=g).double()
    B = torch.randint(-8, 9, (37, 45), generator=g).double()
    assert torch.equal(wsis_ops.dgemm(A.to(DEV), B.to(DEV)).cpu(), A @ B)


# ---------------------------------------------------------------- one process, a large scene and then a small one
def test_small_scene_after_a_large_one_in_one_process():
    """prop_rows_kernel's dynamic-LDS attribute only grows (a function-local static): S = 2049 raises it, the S = 64 torus
    then runs below it and must give what it gave before -- and the reference's bits"""
    before = [_per_class("torus8", it, False) for it in C.ITERATIONS]
    e_final, e_scores, _ = C.reference("S2049", 1)
    final, scores = _run("S2049", 1, False)
    assert _same_scores(scores, e_scores, False) and np.array_equal(final, e_final)
    for it in C.ITERATIONS:
        after = _per_class("torus8", it, False)
        e_pc = C.reference("torus8", it)[2]
        for c in e_pc:
            assert after[c][0].tobytes() == before[it][c][0].tobytes() == e_pc[c][0].tobytes()
            assert np.array_equal(after[c][1], before[it][c][1]) and np.array_equal(after[c][1], e_pc[c][1])


# ---------------------------------------------------------------- the S <= PROP_SPARSE_MAX_S bound
def test_wrapper_takes_the_dense_form_above_the_bound(monkeypatch):
    calls = []
    real = wsis_ops.propagate_sparse

    def spy(*args, **kwargs):
        calls.append(args[0].shape[0])
        return real(*args, **kwargs)
    monkeypatch.delenv("WSIS_PROP_DENSE", raising=False)
    monkeypatch.setattr(wsis_ops, "propagate_sparse", spy)
    e_final, e_scores, _ = C.reference("S255", 2)
    final, scores = _run("S255", 2, None)
    assert calls == [255]                                       # (the spy sees the default form)
    assert _same_scores(scores, e_scores, False) and np.array_equal(final, e_final)
    monkeypatch.setattr(wsis_ops, "PROP_SPARSE_MAX_S", 100)
    final, scores = _run("S255", 2, None)
    assert calls == [255]                                       # not reached again
    assert _same_scores(scores, e_scores, False) and np.array_equal(final, e_final)


def test_c_entry_refuses_one_past_the_bound_and_writes_nothing():
    """S = 8189 needs 163,844 bytes of LDS: a status, a message that names the bound, outputs untouched.  The buffers have
    their honest sizes and are never filled (nothing may read them)"""
    _n, lib = _lib()
    S = wsis_ops.PROP_SPARSE_MAX_S + 1
    A = torch.empty((S, S), dtype=torch.float64, device=DEV)
    adj = torch.empty((S, S), dtype=torch.uint8, device=DEV)
    pred = torch.empty(S, dtype=torch.int32, device=DEV)
    conf = torch.empty(S, dtype=torch.float32, device=DEV)
    label = torch.empty(S, dtype=torch.int32, device=DEV)
    cls_of = torch.zeros(1, dtype=torch.int32, device=DEV)
    ci_of_cls = torch.zeros(1, dtype=torch.int32, device=DEV)
    col = torch.empty(16, dtype=torch.int32, device=DEV)
    val = torch.empty(16, dtype=torch.float64, device=DEV)
    scores = torch.full((1, S), -7.0, dtype=torch.float64, device=DEV)
    arg = torch.full((1, S), -7, dtype=torch.int32, device=DEV)
    ws_bytes = lib.wsis_affinity_propagate_sparse_workspace_bytes(S, 1)
    assert ws_bytes >= S * S * 8
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    status = lib.wsis_affinity_propagate_sparse(_n.ptr(A), _n.ptr(adj), _n.ptr(pred), _n.ptr(conf), _n.ptr(label),
                                                _n.ptr(cls_of), _n.ptr(ci_of_cls), 1, 1, 0.7, 1, S, _n.ptr(col), _n.ptr(val),
                                                16, _n.ptr(scores), _n.ptr(arg), _n.ptr(ws), ws_bytes, _n.stream_ptr())
    torch.cuda.synchronize()
    assert status != 0
    assert str(wsis_ops.PROP_SPARSE_MAX_S) in lib.wsis_last_error().decode()
    with pytest.raises(_n.WsisError, match=str(wsis_ops.PROP_SPARSE_MAX_S)):
        _n.check(status, "affinity_propagate_sparse")
    assert bool((scores == -7.0).all()) and bool((arg == -7).all())
    del A, adj, ws
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- adjacency counts and the uint8 the kernels read
def _counted_case(count, diagonal=False):
    """a 6-cycle of one class, labels at 0 and 3; one adjacency entry (off the diagonal: (0, 1); on it: (2, 2), which has
    a self edge) carries ``count``"""
    S = 6
    eu, ev = C._symmetric([(i, (i + 1) % S) for i in range(S)] + [(2, 2)])
    aff = (np.arange(len(eu)) % 5 + 1).astype(np.float32) / np.float32(8)
    adj = C._adjacency(S, eu, ev)
    if diagonal:
        adj[2, 2] = count
    else:
        adj[0, 1] = count
    label = np.full(S, C.UNLABELLED)
    label[[0, 3]] = 0
    return C._case(eu, ev, aff, adj, np.zeros(S), np.full(S, 0.9), label, 1)


@FORMS
def test_adjacency_count_of_255_is_the_last_that_fits(dense):
    for case in (_counted_case(255), _counted_case(254, diagonal=True)):           # (254 + I = 255 on the diagonal)
        S = len(case.pred)
        A = wsis_ops.affinity_matrix(_up(case.eu), _up(case.ev), _up(case.aff), S)
        assert int(wsis_ops.adjacency_u8(case.adjacency, S, DEV).max()) == 255
        for it in C.ITERATIONS:
            e_final, e_scores, _ = C.reference_call(case, it)
            final, scores = wsis_ops.weak_label_propagation(A, case.adjacency, case.conf, case.pred, case.label, it, 1,
                                                            dense=dense)
            assert np.allclose(scores, e_scores, rtol=C.RTOL, atol=C.ATOL) and np.array_equal(final, e_final)


@FORMS
@pytest.mark.parametrize("count,diagonal", [(256, False), (1000, False), (255, True), (-1, False)])
def test_adjacency_count_that_does_not_fit_a_byte_raises(count, diagonal, dense):
    """256 would wrap to 0 (the edge vanishes), 255 + I on the diagonal as well: ValueError that names the limit"""
    case = _counted_case(count, diagonal)
    S = len(case.pred)
    A = wsis_ops.affinity_matrix(_up(case.eu), _up(case.ev), _up(case.aff), S)
    with pytest.raises(ValueError, match="255"):
        wsis_ops.weak_label_propagation(A, case.adjacency, case.conf, case.pred, case.label, 1, 1, dense=dense)
    with pytest.raises(ValueError, match="255"):
        wsis_ops.adjacency_u8(torch.from_numpy(case.adjacency).to(DEV), S, DEV)
