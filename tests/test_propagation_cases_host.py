"""The inputs of tests/test_gpu_propagation_edges.py, checked without a GPU: the exact cases are exact (every entry of
T0^(n+1) is k / 2^q and a reversed summation order gives the same bits) and have ties, the toleranced ones have the score
gap that keeps a summation order from flipping an argmax, every case reaches the kernel branch it names, and the second
statement of the operator (propagation_cases.chain) agrees with oracle/affinity_ref.py on all of them."""
import numpy as np
import pytest

import propagation_cases as C


def _tied_within(T, rows):
    """columns whose non-zero maximum over the labelled rows is reached by more than one of them"""
    X = T[rows]
    best = X.max(axis=0)
    return int(((X == best).sum(axis=0) > 1)[best > 0].sum())


@pytest.mark.parametrize("name", C.EXACT)
def test_exact_case_is_exact_in_any_order_and_has_ties(name):
    case, br = C.get(name)
    tied = []
    for it in C.ITERATIONS:
        q = br["q"] * (it + 1)
        assert q <= 52
        fwd, rev = C.reference_power(case, it), C.reference_power(case, it, reverse=True)
        _, _, per_class = C.reference(name, it)
        n = 0
        for c, T in fwd.items():
            scaled = T * 2.0 ** q
            assert np.array_equal(scaled, np.rint(scaled)) and T.max() <= 1.0, (c, it)      # k / 2^q, k <= 2^q
            assert T.tobytes() == rev[c].tobytes(), (c, it)
            rows = np.flatnonzero(case.label == c)
            inst = np.zeros_like(T)
            inst[rows] = T[rows]
            assert inst.max(axis=0).tobytes() == per_class[c][0].tobytes()
            assert np.array_equal(inst.argmax(axis=0), per_class[c][1])
            n += _tied_within(T, rows)
        tied.append(n)
    assert min(tied) >= 1, tied
    if name == "torus8":
        assert tied[:3] == [3, 2, 6]


def test_mirror_case_ties_across_classes_and_the_first_class_wins():
    case, br = C.get("components")
    assert br["tied_across"]
    for it in C.ITERATIONS:
        final, scores, per_class = C.reference("components", it)
        classes = sorted(per_class)
        sc = np.stack([per_class[c][0] for c in classes])
        top = sc.max(axis=0)
        cols = np.flatnonzero(((sc == top).sum(axis=0) > 1) & (top > 0))
        assert cols.tolist() == [24]
        assert [classes[i] for i in np.flatnonzero(sc[:, 24] == top[24])] == [1, 2]
        _, m_scores, pseudo = C.merge(per_class, case.label)
        assert pseudo[24] == per_class[1][1][24] == 24 and per_class[2][1][24] == 25
        assert np.array_equal(m_scores, scores)


@pytest.mark.parametrize("name", C.TOLERANCED)
def test_toleranced_case_has_the_score_gap(name):
    case, _ = C.get(name)
    for it in C.ITERATIONS:
        assert C.gap_ok(case, it), it


@pytest.mark.parametrize("name", C.NAMES)
def test_chain_restatement_agrees_with_the_reference(name):
    case, br = C.get(name)
    for it in C.ITERATIONS:
        final, scores, per_class = C.reference(name, it)
        mine = C.chain(case, it)
        assert sorted(mine) == sorted(per_class)
        for c, (e_scores, e_arg) in per_class.items():
            if br["exact"]:
                assert mine[c][0].tobytes() == e_scores.tobytes(), (c, it)
            else:
                assert np.allclose(mine[c][0], e_scores, rtol=1e-12, atol=0.0), (c, it)
                assert np.array_equal(mine[c][0] == 0, e_scores == 0)
            assert np.array_equal(mine[c][1], e_arg), (c, it)
        m_final, m_scores, _ = C.merge(mine, case.label)
        assert np.array_equal(m_final, final)
        assert np.allclose(m_scores, scores, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", C.NAMES)
def test_case_reaches_the_branches_it_names(name):
    case, br = C.get(name)
    S = len(case.pred)
    k, j, w = C.stored_entries(case)
    entries = np.bincount(k, minlength=S)
    assert S % 64 == br["s_mod_64"] and S % 4 == br["s_mod_4"]
    for n in br.get("row_entries", ()):
        assert (entries == n).any(), n
    if "scan_per" in br:
        assert -(-S // 1024) == br["scan_per"]
    if br["exact"] and "row_entries" in br:
        assert set(entries.tolist()) == set(br["row_entries"])               # every row: exactly that many entries
    if "zero_rows" in br:
        assert (entries == 0).sum() >= br["zero_rows"]
    for r in br.get("self_edge_rows", ()):
        assert ((k == r) & (j == r)).any()
    if "n_present" in br:
        assert sum((case.label == c).any() for c in range(case.class_num)) == br["n_present"]
    for c in br.get("never_labelled", ()):
        assert not (case.label == c).any()
    for c in br.get("all_unconfident", ()):
        assert (case.label == c).any() and (case.pred == c).any() and not ((case.pred == c) & (case.conf > C.THR)).any()
        for it in C.ITERATIONS:
            assert not C.reference(name, it)[2][c][0].any()         # present, and scores nothing
    if "label_out_of_range" in br:
        assert (case.label == br["label_out_of_range"]).sum() == 1 and br["label_out_of_range"] >= case.class_num


def test_sizes_cover_the_scan_and_ballot_edges():
    assert {S % 64 for S in C.SIZES} >= {0, 1, 63} and {S % 4 for S in C.SIZES} >= {0, 1, 2, 3}
    assert {-(-S // 1024) for S in C.SIZES} == {1, 2, 3} and {1023, 1024, 1025, 2049} <= set(C.SIZES)
    case, _ = C.get("S2049")
    assert sum((case.label == c).any() for c in range(case.class_num)) == 2


def test_hub_rows_are_partly_masked_and_walked():
    case, _ = C.get("hubs")
    k, j, _ = C.stored_entries(case)
    for h, n in enumerate(C.HUB_ENTRIES):
        cols = j[k == h]
        assert len(cols) == n
        c = case.pred[h]
        kept = (case.pred[cols] == c) & (case.conf[cols] > C.THR)
        assert 0 < kept.sum() < n                                        # masked by class or by confidence, not all
        assert (case.pred[cols] != c).any() and ((case.pred[cols] == c) & ~(case.conf[cols] > C.THR)).any()
    assert case.pred[0] != case.pred[1] and ((k == 0) & (j == 1)).any() and ((k == 2) & (j == 3)).any()
    assert case.label[0] == 0 and case.label[3] == 1 and case.label[1] == case.label[2] == C.UNLABELLED
    for it in (1, 2, 3):        # the unlabelled hubs carry weight in the chain: their columns score after the first step
        scores = C.reference("hubs", it)[1]
        assert scores[1] > 0 and scores[2] > 0


def test_present_zeros_case_has_what_it_names():
    case, br = C.get("present_zeros")
    zero = case.aff == 0
    assert zero.sum() == br["zero_affinities"] and (case.adjacency[case.eu[zero], case.ev[zero]] >= 1).all()
    counts = case.adjacency[case.eu[~zero], case.ev[~zero]]
    assert all((counts == n).any() for n in br["counts"]) and case.adjacency.max() == 255
    k, j, _ = C.stored_entries(case)
    assert len(k) == (~zero).sum()                                       # the CSR drops the zeros
    assert case.label[7] == C.UNLABELLED and case.conf[7] <= C.THR and case.label[11] == case.pred[11]


def test_one_ulp_of_confidence_changes_a_label():
    case, br = C.get("boundary")
    at, above, lab = br["boundary"]["at"], br["boundary"]["above"], br["boundary"]["labelled_at"]
    assert case.conf[at] == case.conf[lab] == C.THR and case.conf[above] == C.THR_UP and case.conf.dtype == np.float32
    assert case.label[lab] == case.pred[lab] == 0 and case.label[at] == case.label[above] == C.UNLABELLED
    assert C.THR_UP > C.THR and np.nextafter(C.THR_UP, np.float32(0)) == C.THR
    up, down = case.conf.copy(), case.conf.copy()
    up[at], up[lab], down[above] = C.THR_UP, C.THR_UP, C.THR
    for it in C.ITERATIONS:
        final = C.reference("boundary", it)[0]
        assert final[at] == C.UNLABELLED and final[above] != C.UNLABELLED
        f_up = C.reference_call(case._replace(conf=up), it)[0]
        f_down = C.reference_call(case._replace(conf=down), it)[0]
        assert f_up[at] != C.UNLABELLED and f_down[above] == C.UNLABELLED
        assert final[47] == C.UNLABELLED and f_up[47] == lab      # the labelled row at the threshold keeps its diagonal only
        if it >= 1:             # the tails behind the boundary superpoints follow them
            assert final[42] == C.UNLABELLED and final[43] != C.UNLABELLED and f_up[42] != C.UNLABELLED
