"""CPU: the fp64 loss reference of tests/loss_ref.py against MultiTaskLoss on the golden inputs (the module is itself
pinned to the reference project's golden vectors by tests/test_golden.py), the hinge mix of the clustered scenes that
tests/test_gpu_loss_edges.py runs, and the empty selection -- a crop without a labelled point or superpoint -- through
the fp64 reference and through the module's non-indexed torch formulations: NaN (or 0 for the offset terms) as value,
every gradient finite and exactly zero."""
import math
import os
import types

import numpy as np
import pytest
import torch

import loss_ref
import losses_3D_WSIS
from test_golden import G, _loss_inputs

IGN = -100


def _crit(classes=20):
    pl = types.SimpleNamespace(ignore_label=IGN, supervise_instance_size=True, joint_training_epoch=0,
                               semantic_dice=True, supervise_sp_offset=True)
    return losses_3D_WSIS.MultiTaskLoss(None, pl, types.SimpleNamespace(classes=classes))


def _ref_terms(z):
    """the seven terms of the joint loss on the golden inputs, from loss_ref, with their fp64 leaves"""
    t = lambda k: torch.from_numpy(z[k])
    leaves = {k: loss_ref.f64(t("in_" + k), True)
              for k in ("semantic_scores", "sp_semantic", "pred_off", "disc", "pred_occ", "pred_size")}
    sp_sem, sp_ins = t("in_sp_sem"), t("in_sp_ins")
    sem, _ = loss_ref.semantic_point(leaves["semantic_scores"], t("in_sem_lab"), IGN)
    sp_ce, _, _ = loss_ref.sp_cross_entropy(leaves["sp_semantic"], sp_sem, IGN)
    l_norm, l_dir, l_occ, l_size, _ = loss_ref.sp_regression(
        leaves["pred_off"], loss_ref.f64(t("in_gt_off")), leaves["pred_occ"], loss_ref.f64(t("in_gt_occ")),
        leaves["pred_size"], loss_ref.f64(t("in_gt_size")), sp_sem, sp_ins, IGN)
    offs = [int(o) for o in z["in_sp_off"]]
    scenes = []
    for b, e in zip(offs[:-1], offs[1:]):
        n_slots = max(int(sp_ins[b:e].max()) + 1, 1)
        scenes.append(loss_ref.discriminative(leaves["disc"][b:e], sp_ins[b:e], sp_sem[b:e], n_slots, IGN))
    disc = torch.stack(scenes).mean()
    terms = {"semantic_loss": sem, "superpoint_semantic_loss": sp_ce, "offset_norm_loss": l_norm,
             "offset_dir_loss": l_dir, "superpoint_discriminative_loss": disc, "occupancy_loss": l_occ,
             "instance_size_loss": l_size}
    return leaves, terms


@pytest.mark.parametrize("slots", [False, True])
def test_loss_ref_matches_module_on_golden_inputs(slots):
    """term by term, values and gradients, at the rtol / atol of tests/test_golden.py"""
    z = np.load(os.path.join(G, "loss_golden.npz"))
    crit = _crit()
    leaves, loss_inp = _loss_inputs(z)
    if slots:
        ins, off = z["in_sp_ins"], z["in_sp_off"]
        loss_inp["sp_instance_slots"] = [max(int(ins[off[i]:off[i + 1]].max()) + 1, 1) for i in range(len(off) - 1)]
    loss, loss_out = crit(loss_inp, 5)
    loss.backward()
    ref_leaves, terms = _ref_terms(z)
    assert set(terms) == set(loss_out)
    for k, want in terms.items():
        assert np.allclose(loss_out[k][0].item(), want.item(), rtol=1e-5, atol=1e-6), k
    total = sum(terms.values())
    total.backward()
    assert np.allclose(loss.item(), total.item(), rtol=1e-5, atol=1e-6)
    for k, v in leaves.items():
        assert np.allclose(v.grad.numpy(), ref_leaves[k].grad.numpy(), rtol=1e-4, atol=1e-7), k
    # the point term alone, before joint training
    leaves, loss_inp = _loss_inputs(z)
    loss, loss_out = crit(loss_inp, 0)
    assert set(loss_out) == {"semantic_loss"}
    assert np.allclose(loss.item(), terms["semantic_loss"].item(), rtol=1e-5, atol=1e-6)


def _assert_mix(x, ins, sem, slots, what):
    push, pull, pairs = loss_ref.hinge_mix(x, ins, sem, slots, IGN)
    print(f"{what}: push hinge active on {push:.2f} of {pairs} pairs, pull hinge on {pull:.2f} of the rows")
    assert 0.2 <= pull <= 0.8
    assert (pairs > 0 and 0.2 <= push <= 0.8) if slots > 1 else pairs == 0


@pytest.mark.parametrize("S,I,seed,cs,sp", loss_ref.CLUSTERED_CASES)
def test_clustered_scenes_have_both_hinge_branches(S, I, seed, cs, sp):
    """a condition on the INPUTS of the GPU tests: in fp64 the push hinge is active on 20 % .. 80 % of the ordered
    instance pairs and the pull hinge on 20 % .. 80 % of the rows (a single instance has no pair)"""
    x, ins = loss_ref.clustered_embeddings(S, I, seed, cs, sp)
    _assert_mix(x, ins, torch.zeros_like(ins), I, f"S={S} I={I}")


def test_dispatch_batch_scenes_have_both_hinge_branches():
    """the same condition on the three scenes of the dispatch batch, with the labels the batch carries"""
    inp, slots = loss_ref.dispatch_batch()
    offs = [int(o) for o in inp["sp_off"]]
    assert [e - b for b, e in zip(offs[:-1], offs[1:])] == [4096, 4097, 300] and slots == [64, 64, 65]
    for i, (b, e) in enumerate(zip(offs[:-1], offs[1:])):
        _assert_mix(inp["disc"][b:e], inp["sp_ins"][b:e], inp["sp_sem"][b:e], slots[i], f"scene {i}")


def _zero_grad(t):
    return t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) == 0.0


def test_loss_ref_empty_selection_is_nan_with_zero_gradients():
    g = torch.Generator().manual_seed(0)
    S, C = 37, 20
    ign = torch.full((S,), IGN, dtype=torch.int64)
    some = torch.randint(0, C, (S,), generator=g)
    x = loss_ref.f64(torch.randn(S, C, generator=g), True)
    loss, n = loss_ref.semantic_point(x, ign, IGN)
    (loss * 1.7).backward()
    assert n == 0 and math.isnan(float(loss.detach())) and _zero_grad(x)
    x = loss_ref.f64(torch.randn(S, C, generator=g), True)
    loss, total, n = loss_ref.sp_cross_entropy(x, ign, IGN)
    (loss * -0.6).backward()
    assert n == 0 and math.isnan(float(loss.detach())) and _zero_grad(x) and float(total.detach()) == float(x.detach().sum())
    # all superpoints invalid: one half by the semantic label, the other by the instance label
    sem, ins = some.clone(), some.clone()
    sem[: S // 2] = IGN
    ins[S // 2:] = IGN
    po, oc, sz = (loss_ref.f64(torch.randn(S, 3, generator=g), True), loss_ref.f64(torch.randn(S, generator=g), True),
                  loss_ref.f64(torch.randn(S, generator=g), True))
    l_norm, l_dir, l_occ, l_size, n = loss_ref.sp_regression(
        po, loss_ref.f64(torch.randn(S, 3, generator=g)), oc, torch.full((S,), -math.inf, dtype=torch.float64), sz,
        loss_ref.f64(torch.rand(S, generator=g)), sem, ins, IGN)
    assert n == 0 and float(l_norm.detach()) == 0.0 and float(l_dir.detach()) == 0.0
    assert math.isnan(float(l_occ.detach())) and math.isnan(float(l_size.detach()))
    (0.7 * l_norm + 1.3 * l_dir - 0.9 * l_occ + 1.1 * l_size).backward()
    assert _zero_grad(po) and _zero_grad(oc) and _zero_grad(sz)
    x = loss_ref.f64(torch.randn(S, 7, generator=g), True)
    loss = loss_ref.discriminative(x, ins, sem, 20, IGN)
    (loss * 1.3).backward()
    assert math.isnan(float(loss.detach())) and _zero_grad(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_module_formulations_on_an_empty_selection_give_zero_gradients(dtype):
    """discriminative_loss_slots, discriminative_loss_masked, _masked_l1 and the (n_valid + 1e-6) offset terms -- the
    torch path behind the fused kernels -- on a scene with no valid row: the indexed formula's value (NaN, or 0 for the
    offset terms) and finite, zero gradients, so a crop without labels does not poison the weights"""
    g = torch.Generator().manual_seed(1)
    S = 41
    crit = _crit()
    valid = torch.zeros(S, dtype=torch.bool)
    ins = torch.randint(0, 9, (S,), generator=g)
    for name in ("slots", "masked"):
        x = torch.randn(S, 7, generator=g).to(dtype).requires_grad_(True)
        loss = (crit.discriminative_loss_slots(x, ins, valid, 9) if name == "slots"
                else crit.discriminative_loss_masked(x, ins, valid))
        (loss * 1.3).backward()
        assert math.isnan(float(loss.detach())), name
        assert _zero_grad(x), name
    for shape in ((S,), (S, 1), (S, 3)):
        p = torch.randn(shape, generator=g).to(dtype).requires_grad_(True)
        t = torch.randn(shape, generator=g).to(dtype)
        t[::2] = -math.inf                               # log voxel count of an unlabelled superpoint
        loss = losses_3D_WSIS._masked_l1(p, t, valid)
        (loss * -0.9).backward()
        assert math.isnan(float(loss.detach())) and _zero_grad(p), shape
    # the offset terms through MultiTaskLoss.forward (CPU: the unfused branch), every superpoint invalid
    C = 20
    leaves = {"semantic_scores": torch.randn(50, C, generator=g), "sp_semantic": torch.randn(S, C, generator=g),
              "pred_off": torch.randn(S, 3, generator=g), "disc": torch.randn(S, 7, generator=g),
              "pred_occ": torch.randn(S, generator=g), "pred_size": torch.randn(S, generator=g)}
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in leaves.items()}
    sp_sem = torch.randint(0, C, (S,), generator=g)
    sp_ins = torch.full((S,), IGN, dtype=torch.int64)
    loss_inp = {
        "point_labels": (torch.randint(0, C, (50,), generator=g), torch.zeros(50, dtype=torch.int64)),
        "semantic_scores": leaves["semantic_scores"],
        "superpoint_labels": (sp_sem, sp_ins), "sp_semantic": leaves["sp_semantic"],
        "sp_offset_vector": (leaves["pred_off"], torch.randn(S, 3, generator=g).to(dtype)),
        "sp_occupancy": (leaves["pred_occ"], torch.full((S,), -math.inf, dtype=dtype)),
        "sp_instance_size": (leaves["pred_size"], torch.rand(S, generator=g).to(dtype)),
        "sp_discriminative_features": (leaves["disc"], torch.tensor([0, 20, S])),
        "sp_instance_slots": [9, 600],                  # the slot and the masked formulation
    }
    loss, loss_out = crit(loss_inp, 5)
    loss.backward()
    assert loss_out["offset_norm_loss"][0].item() == 0.0 and loss_out["offset_dir_loss"][0].item() == 0.0
    for k in ("superpoint_discriminative_loss", "occupancy_loss", "instance_size_loss"):
        assert math.isnan(loss_out[k][0].item()), k
    assert math.isnan(float(loss.detach()))
    for k in ("pred_off", "disc", "pred_occ", "pred_size"):
        assert _zero_grad(leaves[k]), k
    for k in ("semantic_scores", "sp_semantic"):         # the terms with labels still train
        assert bool(torch.isfinite(leaves[k].grad).all()) and float(leaves[k].grad.abs().max()) > 0.0, k


def test_masked_l1_keeps_its_bits_on_a_non_empty_selection():
    """the selection form of _masked_l1 against the product form it replaces: value and gradient bit for bit"""
    g = torch.Generator().manual_seed(2)
    for shape in ((300,), (300, 3)):
        valid = torch.rand(300, generator=g) < 0.4
        p0 = torch.randn(shape, generator=g)
        t = torch.randn(shape, generator=g)
        p = p0.clone().requires_grad_(True)
        got = losses_3D_WSIS._masked_l1(p, t, valid)
        (got * 1.7).backward()
        q = p0.clone().requires_grad_(True)
        w = valid.float()
        while w.dim() < q.dim():
            w = w.unsqueeze(-1)
        want = torch.sum(torch.abs(q - t) * w) / (valid.sum() * (3 if len(shape) > 1 else 1))
        (want * 1.7).backward()
        assert torch.equal(got, want) and torch.equal(p.grad, q.grad)


def test_loss_sum_reference_order():
    v = [0.1234567, 3.7654321e-3, -0.91234, 0.3333333, 2.25e-5, 1.0101, 0.77]
    f = [np.float32(x) for x in v]
    assert loss_ref.loss_sum(v, 1 << 2) == ((((f[0] + f[1]) + (f[2] + f[3])) + f[4]) + f[5]) + f[6]
    assert loss_ref.loss_sum(v[:1]) == f[0]
    assert loss_ref.loss_sum(v[:2], 1) == f[0] + f[1]
