"""GPU: the five fused loss pairs of csrc/loss.hip against the fp64 reference of tests/loss_ref.py at every launch and
hinge branch the kernels have.

  semantic point loss   the forward grid-stride loop re-entered (more than 256 x 256 rows), the backward tile drain on a
                        second sweep (more than 2048 x 256 rows), kept rows straddling a sweep boundary, the final
                        kernel's groups of 64 partial rows (nblk = 1, 2, 9, 64, 65), C = 1, 2, 31, 32 (masked columns, the
                        C | 1 tile pitch), the C = 33 refusal and its torch fallback, empty and one-row selections,
                        saturated logits, a strided view as input
  superpoint CE         S around the 256-row workgroup, C = 1 .. 32, the self-resetting ticket over launches of different
                        grid sizes on one stream and on a second one
  superpoint regression S around the 1024-thread walk, rows dropped by either label, zero / tiny / equal vectors
  discriminative loss   clustered embeddings with both branches of both hinges present (tests/test_loss_ref_host.py
                        asserts the mix), every chunk count of dl_chunks, degenerate instances, the row and slot limits
  term sum              every pairing mask, bit for bit
  MultiTaskLoss.forward the fused / unfused dispatch on one three-scene batch, with every WSIS_FUSE_* switch and the
                        side-stream variant

Bounds.  Inputs of a kind tests/test_gpu_ops.py already runs (N <= 40,000, logits of scale 3) keep that file's bounds:
loss 2e-6 (discriminative 3e-6) of |want| + 1e-7, gradient 1e-5 (2e-5) of the reference gradient's largest entry.  For
the new input classes (several sweeps, saturated logits, clustered embeddings, tiny norms) the same formulation is also
evaluated with torch in fp32 on the GPU -- the module's unfused path -- and the kernel's bound is the larger of the
project bound and 4 x that evaluation's own error against fp64 (4: a different but legitimate order of additions).
Both errors are printed.  Counts, zero gradients and repeat runs are compared exactly.

Measured on an MI355X (loss: absolute error / gradient: largest absolute error; kernel | fp32 torch | bound applied):
  semantic 65,536 x 20        1.5e-7 | 3.2e-7 | 1.4e-5      2.4e-11 | 1.7e-11 | 3.9e-10
  semantic 65,537 x 20        7.4e-8 | 7.4e-8 | 1.4e-5      2.3e-11 | 1.8e-11 | 3.8e-10
  semantic 196,685 x 13       2.8e-8 | 2.8e-8 | 1.3e-5      8.7e-12 | 5.5e-12 | 1.3e-10
  semantic 70,000, 24 kept    4.1e-7 | 5.5e-7 | 1.5e-5      5.1e-9  | 6.1e-9  | 3.9e-7
  semantic 524,545 x 4        7.1e-8 | 7.1e-8 | 8.3e-6      8.3e-13 | 7.0e-13 | 2.5e-11
  semantic logits x 1e4       1.6e-3 | 1.6e-3 | 1.1e-1      2.9e-11 | 7.1e-11 | 8.1e-9     (loss 55,125)
  semantic equal / -200 rows  4.3e-7 | 5.0e-8 | 1.4e-5      4.3e-10 | 2.8e-10 | 8.6e-9
  sp CE logits x 1e4          4.1e-4 | 4.1e-4 | 1.1e-1      3.1e-11 | 9.0e-11 | 1.1e-8     (loss 55,605)
  regression |p| <= 1e-8      (losses <= 2.9e-8 | 2.9e-8)   7.0e-3  | 7.0e-3  | 1.2        (gradient 1.2e5)
  regression |p| = 1e-4                                      8.1e-7  | 1.3e-6  | 1.2e-4     (gradient 12.4)
  discriminative, clustered   <= 2.4e-8 | <= 4.2e-8 | 3e-6 |want| + 1e-7     <= 1.3e-8 | <= 1.2e-8 | 2e-5 max|grad|
  dispatch, total             5.6e-7 | 5.6e-7 | 4.8e-5
Every kernel figure is inside the project bound; 4 x the fp32-torch error was the larger bound nowhere."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref
import losses_3D_WSIS
import wsis_native as _n
import wsis_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGN = -100
SEM_L, SEM_G = 2e-6, 1e-5            # semantic, regression and cross entropy: loss / gradient
DISC_L, DISC_G = 3e-6, 2e-5          # discriminative
G_FLOOR = 1e-12                      # absolute floor of a gradient bound (a reference gradient that is 0 throughout)


def _crit(classes=20, joint_epoch=0):
    pl = types.SimpleNamespace(ignore_label=IGN, supervise_instance_size=True, joint_training_epoch=joint_epoch,
                               semantic_dice=True, supervise_sp_offset=True)
    return losses_3D_WSIS.MultiTaskLoss(None, pl, types.SimpleNamespace(classes=classes))


def _val(t):
    return float(t.detach().double().cpu())


def _check_loss(what, got, want, project, torch32=None):
    """|got - want| within project * |want| + 1e-7, or within 4 x the fp32-torch error where that is larger"""
    got, want = _val(got), _val(want)
    err = abs(got - want)
    bound = project * abs(want) + 1e-7
    msg = f"[loss-edges] {what}: loss {want:.9g} kernel err {err:.3e}"
    if torch32 is not None:
        terr = abs(_val(torch32) - want)
        bound = max(bound, 4.0 * terr)
        msg += f" fp32-torch err {terr:.3e}"
    print(msg + f" bound {bound:.3e}")
    assert math.isfinite(got) and err <= bound, (what, got, want, err, bound)


def _check_grad(what, got, want, project, torch32=None):
    """max |got - want| within project * max |want|, or within 4 x the fp32-torch gradient's error where that is larger"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    gmax = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    bound = project * gmax + G_FLOOR
    msg = f"[loss-edges] {what}: grad max {gmax:.3e} kernel err {err:.3e}"
    if torch32 is not None:
        terr = float((torch32.detach().double().cpu() - want).abs().max())
        bound = max(bound, 4.0 * terr)
        msg += f" fp32-torch err {terr:.3e}"
    print(msg + f" bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _all_zero(t):
    return bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


# ---------------------------------------------------------------- semantic point loss

def _sem_torch32(monkeypatch, x, y, ignore, up):
    """the module's unfused evaluation (nn.CrossEntropyLoss + dice on the masked softmax) in fp32 on the GPU"""
    monkeypatch.setenv("WSIS_FUSE_SEM_LOSS", "0")
    monkeypatch.delenv("WSIS_LOSS_INDEXED", raising=False)
    crit = _crit(x.shape[1], joint_epoch=0)
    crit.ignore_label = ignore
    crit.semantic_criterion = torch.nn.CrossEntropyLoss(ignore_index=ignore)
    leaf = x.to(DEV).requires_grad_(True)
    loss, _ = crit({"point_labels": (y.to(DEV).long(), None), "semantic_scores": leaf}, 0)
    (loss * up).backward()
    monkeypatch.delenv("WSIS_FUSE_SEM_LOSS")
    return loss.detach(), leaf.grad


def _sem_case(what, x, y, ignore=IGN, up=1.7, monkeypatch=None, repeat=False):
    """kernel against loss_ref on the same fp32 scores; ``monkeypatch`` given = a new input class (fp32-torch bound)"""
    leaf = x.to(DEV).requires_grad_(True)
    yd = y.to(DEV)
    loss, n_kept = wsis_ops.semantic_point_loss(leaf, yd, ignore)
    (loss * up).backward()
    ref = loss_ref.f64(x, True)
    want, n = loss_ref.semantic_point(ref, y, ignore)
    (want * up).backward()
    assert int(n_kept) == n, (what, int(n_kept), n)
    keep = (y.long() != ignore)
    if n == 0:
        assert math.isnan(_val(loss)) and math.isnan(_val(want)), what
        assert _all_zero(leaf.grad) and _all_zero(ref.grad), what
        return
    t_loss = t_grad = None
    if monkeypatch is not None:
        t_loss, t_grad = _sem_torch32(monkeypatch, x, y, ignore, up)
    _check_loss(what, loss, want, SEM_L, t_loss)
    _check_grad(what, leaf.grad, ref.grad, SEM_G, t_grad)
    if not bool(keep.all()):
        assert _all_zero(leaf.grad[(~keep).to(DEV)]), what
    if repeat:
        leaf2 = x.to(DEV).requires_grad_(True)
        l2, _ = wsis_ops.semantic_point_loss(leaf2, yd, ignore)
        (l2 * up).backward()
        assert torch.equal(l2, loss) and torch.equal(leaf2.grad, leaf.grad), what


def _scores(N, C, seed, frac_ignored):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g) * 3
    y = torch.randint(0, C, (N,), generator=g)
    y[torch.rand(N, generator=g) < frac_ignored] = IGN
    return x, y


@pytest.mark.parametrize("N,C", [(65536, 20), (65537, 20), (196685, 13)])
def test_semantic_forward_sweeps(N, C, monkeypatch):
    """256 workgroups x 256 rows cover 65,536 rows: one full sweep, one row more (thread 0 re-enters the loop), three
    sweeps and a partial one with an odd C; the 196,685-row case twice, bit for bit"""
    x, y = _scores(N, C, N, 0.3)
    y[-1] = 1                                              # the row past the sweep boundary is a kept row
    _sem_case(f"sem sweeps N={N} C={C}", x, y, monkeypatch=monkeypatch, repeat=N == 196685)


def test_semantic_weak_supervision_straddles_the_sweep_boundary(monkeypatch):
    """70,000 rows, 24 of them labelled: 8 in the first workgroup, 8 around row 65,536 (second trip of workgroup 0
    and last rows of workgroup 255), 8 in the last 256 rows; every other workgroup contributes zeros"""
    N, C = 70000, 20
    x, y = _scores(N, C, 7, 0.0)
    kept = torch.tensor([0, 3, 63, 64, 100, 127, 200, 255, 65530, 65532, 65534, 65535, 65536, 65537, 65541, 65545,
                         N - 256, N - 200, N - 130, N - 65, N - 64, N - 3, N - 2, N - 1])
    lab = y[kept].clone()
    y[:] = IGN
    y[kept] = lab
    _sem_case("sem weak 70000 rows / 24 kept", x, y, up=0.9, monkeypatch=monkeypatch)


def test_semantic_backward_second_sweep(monkeypatch):
    """2048 workgroups x 256 rows cover 524,288 rows: 257 rows more drain the LDS tile on a second sweep, the last
    tile holds one row; C = 4 gives the tile pitch 5; negative upstream gradient"""
    N, C = 2048 * 256 + 257, 4
    x, y = _scores(N, C, 5, 0.5)
    y[-1], y[-2], y[2048 * 256] = 2, IGN, 0
    _sem_case(f"sem bwd sweep N={N} C={C}", x, y, up=-0.6, monkeypatch=monkeypatch)


@pytest.mark.parametrize("N", [255, 256, 257, 2049, 16129, 16385])
def test_semantic_final_kernel_boundaries(N):
    """nblk = 1, 1, 2, 9, 64, 65 partial rows through the final kernel's eight sub-sums of stride 8"""
    x, y = _scores(N, 20, N, 0.3)
    _sem_case(f"sem final N={N}", x, y, up=1.3)


@pytest.mark.parametrize("C", [1, 2, 31, 32])
def test_semantic_class_edges(C):
    """31, 30, 1 and 0 masked register columns; backward tile pitch C | 1 = 1, 3, 31, 33"""
    x, y = _scores(1000, C, 100 + C, 0.4)
    _sem_case(f"sem classes C={C}", x, y, up=-1.1 if C == 2 else 1.7)


def test_semantic_33_classes_refused_and_module_falls_back(monkeypatch):
    """the C ABI refuses C = 33 with a status and a message that names the limit; MultiTaskLoss with 33 classes takes
    the torch evaluation (bounds of tests/test_golden.py) and never calls the kernel"""
    lib = _n.hip()
    N, C = 1000, 33
    x, y = _scores(N, C, 33, 0.3)
    xd, yd = x.to(DEV), y.to(DEV)
    out = torch.zeros(2, device=DEV)
    saved = torch.zeros(2 * C + 1, device=DEV)
    ws_bytes = lib.wsis_semantic_loss_workspace_bytes(N)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    assert lib.wsis_semantic_loss_fwd(xd.data_ptr(), yd.data_ptr(), N, C, IGN, out.data_ptr(), saved.data_ptr(),
                                      ws.data_ptr(), ws_bytes, _n.stream_ptr()) != 0
    assert b"32" in lib.wsis_last_error()
    g1 = torch.ones(1, device=DEV)
    dx = torch.zeros_like(xd)
    assert lib.wsis_semantic_loss_bwd(xd.data_ptr(), yd.data_ptr(), N, C, IGN, saved.data_ptr(), g1.data_ptr(),
                                      dx.data_ptr(), _n.stream_ptr()) != 0
    assert b"32" in lib.wsis_last_error() and _all_zero(dx)
    calls = []
    real = wsis_ops.semantic_point_loss
    monkeypatch.setattr(wsis_ops, "semantic_point_loss", lambda *a, **k: calls.append(1) or real(*a, **k))
    leaf = xd.clone().requires_grad_(True)
    loss, loss_out = _crit(C)({"point_labels": (yd, None), "semantic_scores": leaf}, 0)
    (loss * 1.7).backward()
    ref = loss_ref.f64(x, True)
    want, _ = loss_ref.semantic_point(ref, y, IGN)
    (want * 1.7).backward()
    assert not calls and set(loss_out) == {"semantic_loss"}
    assert np.allclose(_val(loss), _val(want), rtol=1e-5, atol=1e-6)
    assert float((leaf.grad.double().cpu() - ref.grad).abs().max()) <= 1e-4 * float(ref.grad.abs().max())


@pytest.mark.parametrize("kind", ["all_ignored", "one_kept", "one_class", "ignore_255", "int32"])
def test_semantic_label_edges(kind):
    """no kept row (NaN value, zero gradient, n_kept = 0), one kept row, one class only, another ignore value,
    int32 labels"""
    N, C = 1000, 20
    x, y = _scores(N, C, 50, 0.5)
    ignore = IGN
    if kind == "all_ignored":
        y[:] = IGN
    elif kind == "one_kept":
        y[:] = IGN
        y[777] = 4
    elif kind == "one_class":
        y[y != IGN] = 7
    elif kind == "ignore_255":
        ignore = 255
        y[y == IGN] = 255
    elif kind == "int32":
        y = y.int()
    _sem_case(f"sem labels {kind}", x, y, ignore=ignore, up=-0.8 if kind == "one_kept" else 1.7)


@pytest.mark.parametrize("kind", ["saturated", "equal_and_losing"])
def test_semantic_logit_edges(kind, monkeypatch):
    """rows scaled by 1e4 (p is exactly 0 or 1 in fp32; m + logZ - x_l of some 1e4 must stay finite); a row of equal
    logits and a row whose label logit loses by 200 (p_label underflows to 0, the row's CE is 200)"""
    N, C = 3000, 20
    x, y = _scores(N, C, 60, 0.3)
    if kind == "saturated":
        x = x * 1e4
    else:
        y[0], y[1] = 3, 5
        x[0] = 1.25
        x[1, 5] = x[1].max() - 200.0
    _sem_case(f"sem logits {kind}", x, y, monkeypatch=monkeypatch)


def test_semantic_view_input_reaches_the_leaf():
    """scores = wide[:, 3:3 + C] of an [N, C + 5] leaf: the gradient arrives in those columns, the others get zero"""
    N, C = 3000, 20
    g = torch.Generator().manual_seed(70)
    wide = torch.randn(N, C + 5, generator=g) * 3
    _, y = _scores(N, C, 71, 0.3)
    leaf = wide.to(DEV).requires_grad_(True)
    loss, n_kept = wsis_ops.semantic_point_loss(leaf[:, 3:3 + C], y.to(DEV), IGN)
    (loss * 1.7).backward()
    ref = loss_ref.f64(wide, True)
    want, n = loss_ref.semantic_point(ref[:, 3:3 + C], y, IGN)
    (want * 1.7).backward()
    assert int(n_kept) == n
    _check_loss("sem view", loss, want, SEM_L)
    _check_grad("sem view", leaf.grad, ref.grad, SEM_G)
    assert _all_zero(leaf.grad[:, :3]) and _all_zero(leaf.grad[:, 3 + C:])


# ---------------------------------------------------------------- superpoint cross entropy

def _ce_launch(x, y, up):
    leaf = x.to(DEV).requires_grad_(True)
    loss, total = wsis_ops.superpoint_cross_entropy(leaf, y.to(DEV), IGN)
    (loss * up).backward()
    return leaf, loss, total


def _ce_compare(what, x, y, up, got, new=False):
    leaf, loss, total = got
    ref = loss_ref.f64(x, True)
    want, want_sum, n = loss_ref.sp_cross_entropy(ref, y, IGN)
    (want * up).backward()
    assert abs(_val(total) - _val(want_sum)) <= 1e-5 * float(x.double().abs().sum()), what
    if n == 0:
        assert math.isnan(_val(loss)) and math.isnan(_val(want)) and _all_zero(leaf.grad) and _all_zero(ref.grad), what
        return
    t_loss = t_grad = None
    if new:                                                # the module's unfused path: nn.CrossEntropyLoss in fp32
        t_leaf = x.to(DEV).requires_grad_(True)
        t_loss = F.cross_entropy(t_leaf, y.to(DEV), ignore_index=IGN)
        (t_loss * up).backward()
        t_grad = t_leaf.grad
    _check_loss(what, loss, want, SEM_L, t_loss)
    _check_grad(what, leaf.grad, ref.grad, SEM_G, t_grad)
    assert _all_zero(leaf.grad[(y == IGN).to(DEV)]) if bool((y == IGN).any()) else True, what


@pytest.mark.parametrize("C", [1, 2, 20, 32])
def test_sp_cross_entropy_shapes(C):
    """one row per thread, 256 rows per workgroup: S = 1, 255, 256, 257, 513, 2,289 (1, 1, 1, 2, 3, 9 workgroups)"""
    for S in (1, 255, 256, 257, 513, 2289):
        x, y = _scores(S, C, 1000 * C + S, 0.3 if S > 1 else 0.0)
        up = -0.7 if S == 257 else 1.7
        _ce_compare(f"sp ce S={S} C={C}", x, y, up, _ce_launch(x, y, up))


def test_sp_cross_entropy_label_and_logit_edges():
    """all rows ignored (NaN value, zero gradient; one row and three workgroups); saturated logits"""
    for S in (1, 600):
        x, y = _scores(S, 20, S, 1.1)
        assert bool((y == IGN).all())
        _ce_compare(f"sp ce all ignored S={S}", x, y, 1.7, _ce_launch(x, y, 1.7))
    x, y = _scores(2289, 20, 9, 0.3)
    x = x * 1e4
    _ce_compare("sp ce saturated", x, y, 1.7, _ce_launch(x, y, 1.7), new=True)


@pytest.mark.parametrize("other_stream", [False, True])
def test_sp_cross_entropy_ticket_reuse(other_stream):
    """launches of 3, 1, 2 and 2 workgroups back to back on one stream share one ticket word: each must find it zero
    (a ticket left at 3 would keep the one-workgroup launch from ever being the last arrival).  The same on a stream of
    its own, which gets its own sync block."""
    cases = [_scores(S, 20, 2000 + S, 0.3) for S in (600, 1, 300, 257)]
    cases[1][1][0] = 2
    stream = torch.cuda.Stream() if other_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = [_ce_launch(x, y, 1.3) for x, y in cases]          # nothing is read back between the launches
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for (x, y), g in zip(cases, got):
        _ce_compare(f"sp ce ticket S={x.shape[0]} other_stream={other_stream}", x, y, 1.3, g)
    assert not _n.sync_errors()


def test_sp_cross_entropy_33_classes_refused():
    lib = _n.hip()
    S, C = 8, 33
    x = torch.zeros(S, C, device=DEV)
    y = torch.zeros(S, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, device=DEV)
    ws_bytes = lib.wsis_sp_ce_loss_workspace_bytes(S)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    assert lib.wsis_sp_ce_loss_fwd(x.data_ptr(), y.data_ptr(), S, C, IGN, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                   _n.sync_block(x.device).data_ptr(), _n.stream_ptr()) != 0
    assert b"32" in lib.wsis_last_error()
    g1 = torch.ones(1, device=DEV)
    d = torch.zeros_like(x)
    assert lib.wsis_sp_ce_loss_bwd(x.data_ptr(), y.data_ptr(), S, C, IGN, out.data_ptr(), g1.data_ptr(), d.data_ptr(),
                                   _n.stream_ptr()) != 0
    assert b"32" in lib.wsis_last_error()


# ---------------------------------------------------------------- superpoint regression

REG_UP = [0.7, -1.3, 0.9, 1.1]


def _reg_inputs(S, seed):
    g = torch.Generator().manual_seed(seed)
    t = {"pred_off": torch.randn(S, 3, generator=g), "gt_off": torch.randn(S, 3, generator=g),
         "pred_occ": torch.randn(S, generator=g), "gt_occ": torch.randn(S, generator=g),
         "pred_size": torch.randn(S, generator=g), "gt_size": torch.rand(S, generator=g)}
    sem = torch.randint(0, 20, (S,), generator=g)
    ins = torch.randint(0, 9, (S,), generator=g)
    return t, sem, ins


def _reg_torch32(t, sem, ins):
    """the module's unfused formulas (losses_3D_WSIS.py, MultiTaskLoss.forward) in fp32 on the GPU"""
    leaves = [t[k].to(DEV).requires_grad_(True) for k in ("pred_off", "pred_occ", "pred_size")]
    gt_off, gt_occ, gt_size = t["gt_off"].to(DEV), t["gt_occ"].to(DEV), t["gt_size"].to(DEV)
    valid = ((sem != IGN) & (ins != IGN)).to(DEV)
    n_valid = valid.sum()
    pt_dist = torch.sum(torch.abs(leaves[0] - gt_off), dim=-1)
    l_norm = torch.sum(pt_dist * valid) / (n_valid + 1e-6)
    gt_dir = gt_off / (torch.norm(gt_off, p=2, dim=1).unsqueeze(-1) + 1e-8)
    pt_dir = leaves[0] / (torch.norm(leaves[0], p=2, dim=1).unsqueeze(-1) + 1e-8)
    l_dir = torch.sum(-(gt_dir * pt_dir).sum(-1) * valid) / (n_valid + 1e-6)
    l_occ = losses_3D_WSIS._masked_l1(leaves[1], gt_occ, valid)
    l_size = losses_3D_WSIS._masked_l1(leaves[2], gt_size, valid)
    outs = (l_norm, l_dir, l_occ, l_size)
    sum(w * o for w, o in zip(REG_UP, outs)).backward()
    return outs, [l.grad for l in leaves]


def _reg_case(what, t, sem, ins, new=False, groups=None):
    """``groups``: {name: rows} whose offset gradient is orders of magnitude above the others' (d/dp of p / (|p| + 1e-8)
    is of the order 1 / |p|); every group is compared on its own scale and the remaining rows on theirs"""
    names = ("pred_off", "pred_occ", "pred_size")
    leaves = [t[k].to(DEV).requires_grad_(True) for k in names]
    outs = wsis_ops.sp_regression_losses(leaves[0], t["gt_off"].to(DEV), leaves[1], t["gt_occ"].to(DEV), leaves[2],
                                         t["gt_size"].to(DEV), sem.to(DEV), ins.to(DEV), IGN)
    sum(w * o for w, o in zip(REG_UP, outs[:4])).backward()
    ref = [loss_ref.f64(t[k], True) for k in names]
    want = loss_ref.sp_regression(ref[0], loss_ref.f64(t["gt_off"]), ref[1], loss_ref.f64(t["gt_occ"]), ref[2],
                                  loss_ref.f64(t["gt_size"]), sem, ins, IGN)
    n = want[4]
    valid = (sem != IGN) & (ins != IGN)
    assert float(outs[4]) == float(n), what
    if n == 0:
        assert _val(outs[0]) == 0.0 and _val(outs[1]) == 0.0 and _val(want[0]) == 0.0 and _val(want[1]) == 0.0, what
        assert all(math.isnan(_val(v)) for v in (outs[2], outs[3], want[2], want[3])), what
        sum(w * o for w, o in zip(REG_UP, want[:4])).backward()
        assert all(_all_zero(a.grad) and _all_zero(b.grad) for a, b in zip(leaves, ref)), what
        return
    sum(w * o for w, o in zip(REG_UP, want[:4])).backward()
    t_outs, t_grads = _reg_torch32(t, sem, ins) if new else ((None,) * 4, (None,) * 3)
    for name, got, w, tv in zip(("norm", "dir", "occ", "size"), outs[:4], want[:4], t_outs):
        _check_loss(f"{what} {name}", got, w, SEM_L, tv)
    for k, a, b, tg in zip(names, leaves, ref, t_grads):
        if k == "pred_off" and groups is not None:
            rest = torch.ones(a.shape[0], dtype=torch.bool)
            masks = []
            for tag, idx in groups.items():
                m = torch.zeros(a.shape[0], dtype=torch.bool)
                m[torch.tensor(idx)] = True
                rest &= ~m
                masks.append((tag, m))
            for tag, rows in masks + [("other rows", rest)]:
                _check_grad(f"{what} d{k} {tag}", a.grad[rows.to(DEV)], b.grad[rows],
                            SEM_G, None if tg is None else tg[rows.to(DEV)])
        else:
            _check_grad(f"{what} d{k}", a.grad, b.grad, SEM_G, tg)
        if not bool(valid.all()):
            assert _all_zero(a.grad[(~valid).to(DEV)]), (what, k)


@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 2049])
def test_sp_regression_shapes_and_row_edges(S):
    """one workgroup of 1024 threads walks the rows: S = 1, 1,023, 1,024, 1,025 (a second trip for thread 0), 2,049;
    rows dropped by the semantic label only and by the instance label only, a zero target vector, prediction ==
    target in single components and in both scalar terms (sign 0), -inf occupancy targets on the dropped rows"""
    t, sem, ins = _reg_inputs(S, 300 + S)
    if S > 1:
        g = torch.Generator().manual_seed(S)
        sem[torch.rand(S, generator=g) < 0.25] = IGN
        ins[torch.rand(S, generator=g) < 0.25] = IGN
        sem[:8], ins[:8] = 3, 1
        sem[8], ins[8] = IGN, 2                            # dropped by the semantic label only
        sem[9], ins[9] = 4, IGN                            # dropped by the instance label only
        t["gt_off"][2] = 0.0
        t["pred_off"][3, 1] = t["gt_off"][3, 1]
        t["pred_off"][4] = t["gt_off"][4]
        t["pred_occ"][5] = t["gt_occ"][5]
        t["pred_size"][6] = t["gt_size"][6]
        sem[-1], ins[-1] = 5, 0                            # the last row is a kept row
        valid = (sem != IGN) & (ins != IGN)
        t["gt_occ"][~valid] = float("-inf")
    _reg_case(f"sp reg S={S}", t, sem, ins)


def test_sp_regression_no_valid_row():
    """0 / 1e-6 = 0 for the offset terms, NaN for the L1 terms, n = 0, every gradient exactly zero"""
    S = 1500
    t, sem, ins = _reg_inputs(S, 9)
    sem[: S // 2] = IGN
    ins[S // 2:] = IGN
    t["gt_occ"][:] = float("-inf")
    _reg_case("sp reg empty", t, sem, ins)


def test_sp_regression_zero_and_tiny_predictions(monkeypatch):
    """predicted vectors that are zero (torch's norm backward is 0 there) or of norm 1e-8 and 1e-4: d/dp of
    p / (|p| + 1e-8) is of the order 1e8 and 1e4 there, so these rows are compared on their own scales"""
    S = 1200
    t, sem, ins = _reg_inputs(S, 10)
    sem[torch.arange(S) % 5 == 4] = IGN
    big = torch.tensor([1, 2, 3, 6, 7, 8])
    sem[big], ins[big] = 3, 1
    unit = F.normalize(t["pred_off"][big].double(), dim=1)
    t["pred_off"][big] = (unit * torch.tensor([0.0, 1e-8, 1e-4, 0.0, 1e-8, 1e-4], dtype=torch.float64).unsqueeze(1)).float()
    _reg_case("sp reg tiny", t, sem, ins, new=True, groups={"|p| <= 1e-8": [1, 2, 6, 7], "|p| = 1e-4": [3, 8]})


# ---------------------------------------------------------------- discriminative loss

def _disc_launch(x, ins, sem, n_slots, up, crit):
    leaf = x.to(DEV).requires_grad_(True)
    loss = wsis_ops.discriminative_loss(leaf, ins.to(DEV), sem.to(DEV), n_slots, IGN, crit.delta_v, crit.delta_d,
                                        crit.param_var, crit.param_dist, crit.param_reg)
    (loss * up).backward()
    return leaf, loss


def _disc_case(what, x, ins, sem, n_slots, up=1.3, new=False, repeat=False):
    crit = _crit()
    leaf, loss = _disc_launch(x, ins, sem, n_slots, up, crit)
    ref = loss_ref.f64(x, True)
    want = loss_ref.discriminative(ref, ins, sem, n_slots, IGN, crit.delta_v, crit.delta_d, crit.param_var,
                                   crit.param_dist, crit.param_reg)
    (want * up).backward()
    valid = (ins != IGN) & (sem != IGN) & (ins >= 0) & (ins < n_slots)
    if not bool(valid.any()):
        assert math.isnan(_val(loss)) and math.isnan(_val(want)) and _all_zero(leaf.grad) and _all_zero(ref.grad), what
        return
    t_loss = t_grad = None
    if new:                                                # the module's unfused path: the slot formulation in fp32
        t_leaf = x.to(DEV).requires_grad_(True)
        t_loss = crit.discriminative_loss_slots(t_leaf, ins.to(DEV), valid.to(DEV), n_slots)
        (t_loss * up).backward()
        t_grad = t_leaf.grad
    _check_loss(what, loss, want, DISC_L, t_loss)
    _check_grad(what, leaf.grad, ref.grad, DISC_G, t_grad)
    if not bool(valid.all()):
        assert _all_zero(leaf.grad[(~valid).to(DEV)]), what
    if repeat:
        leaf2, l2 = _disc_launch(x, ins, sem, n_slots, up, crit)
        assert torch.equal(l2, loss) and torch.equal(leaf2.grad, leaf.grad), what


@pytest.mark.parametrize("S,I,seed,cs,sp", loss_ref.CLUSTERED_CASES)
def test_discriminative_clustered_embeddings(S, I, seed, cs, sp):
    """tight clusters far apart: both branches of the push hinge (per pair) and of the pull hinge (per row) are present
    at once; 10, 2, 2, 3, 14, 16, 16, 8 and 4 row chunks; the 4,096-row maximum, run twice bit for bit"""
    x, ins = loss_ref.clustered_embeddings(S, I, seed, cs, sp)
    _disc_case(f"disc clustered S={S} I={I}", x, ins, torch.zeros_like(ins), I, up=-1.3 if S == 300 else 1.3,
               new=True, repeat=(S, I) == (4096, 64))


def _dyadic(g, *shape):
    """multiples of 1/64 in [-1, 1): sums of a few of them are exact in fp32 and fp64 in any order"""
    return torch.randint(-64, 64, shape, generator=g).float() / 64.0


def test_discriminative_degenerate_instances():
    """an instance of two identical rows (distance to the mean exactly 0), an instance {x, -x} (mean exactly 0: no
    regulariser gradient), two instances built from the same four rows (L1 distance 0: sign 0 in the push term)
    next to ordinary instances; an id >= n_slots and a negative id that is not the ignore label are dropped"""
    g = torch.Generator().manual_seed(3)
    rows, ids = [], []
    a = _dyadic(g, 1, 7)
    rows += [a, a]
    ids += [0, 0]
    b = _dyadic(g, 1, 7)
    rows += [b, -b]
    ids += [1, 1]
    four = _dyadic(g, 4, 7)
    for k in range(4):                                     # interleaved: the two copies sit at different rows
        rows += [four[k:k + 1], _dyadic(g, 1, 7), four[3 - k:4 - k]]
        ids += [2, 4 + k % 2, 3]
    rows += [_dyadic(g, 6, 7)]
    ids += [4, 5, 9, -3, 4, 5]                             # 9 >= n_slots = 8 and -3 are dropped
    x, ins = torch.cat(rows), torch.tensor(ids)
    sem = torch.zeros_like(ins)
    sem[-1] = IGN
    _disc_case("disc degenerate", x, ins, sem, 8)


@pytest.mark.parametrize("kind", ["single_instance", "no_valid_row", "one_row", "one_row_dropped"])
def test_discriminative_small_selections(kind):
    """one instance (n = 1: no push term, divisor max(n (n - 1), 1)); no valid row (NaN value, zero gradient); S = 1"""
    g = torch.Generator().manual_seed(4)
    S = 1 if kind.startswith("one_row") else 700
    x = torch.randn(S, 7, generator=g) * 0.3
    ins = torch.full((S,), 2, dtype=torch.int64)
    sem = torch.zeros(S, dtype=torch.int64)
    if kind == "single_instance":
        sem[::7] = IGN
    elif kind == "no_valid_row":
        sem[: S // 2] = IGN
        ins[S // 2:] = IGN
    elif kind == "one_row_dropped":
        ins[0] = IGN
    _disc_case(f"disc {kind}", x, ins, sem, 5, up=-0.9 if kind == "one_row" else 1.3)


def test_discriminative_limits_refused():
    """S = 4,097 and n_slots = 65: a non-zero status from both directions, nothing launched"""
    lib = _n.hip()
    x = torch.zeros(4097, 7, device=DEV)
    lab = torch.zeros(4097, dtype=torch.int64, device=DEV)
    out = torch.zeros(1, device=DEV)
    saved = torch.zeros(lib.wsis_disc_loss_saved_floats(), device=DEV)
    dx = torch.zeros_like(x)
    g1 = torch.ones(1, device=DEV)
    for S, slots in ((4097, 64), (4096, 65), (0, 8), (16, 0)):
        args = (x.data_ptr(), lab.data_ptr(), lab.data_ptr(), S, 7, slots, IGN, 0.1, 1.5, 1.0, 1.0, 0.001)
        assert lib.wsis_disc_loss_fwd(*args, out.data_ptr(), saved.data_ptr(), _n.stream_ptr()) != 0, (S, slots)
        assert b"4096" in lib.wsis_last_error() and b"64" in lib.wsis_last_error()
        assert lib.wsis_disc_loss_bwd(*args, saved.data_ptr(), g1.data_ptr(), dx.data_ptr(), _n.stream_ptr()) != 0
    with pytest.raises(_n.WsisError):
        wsis_ops.discriminative_loss(x, lab, lab, 64)
    assert _all_zero(dx) and _all_zero(out)


# ---------------------------------------------------------------- term sum

@pytest.mark.parametrize("n", [1, 2, 8])
def test_loss_sum_pairings_bit_for_bit(n):
    """no pair, bit 0, bit n - 2 and alternating bits against the numpy float32 evaluation in the kernel's order; a
    pair bit on the last term is refused"""
    vals = [0.1234567, 3.7654321e-3, -0.91234, 0.3333333, 2.25e-5, 1.0101, 0.77, -1.9e-7][:n]
    masks = {0}
    if n >= 2:
        masks |= {1, 1 << (n - 2), sum(1 << i for i in range(0, n - 1, 2))}
    for paired in sorted(masks):
        terms = [torch.tensor(v, dtype=torch.float32, device=DEV, requires_grad=True) for v in vals]
        got = wsis_ops.loss_sum(terms, paired)
        (got * -2.5).backward()
        want = loss_ref.loss_sum(vals, paired)
        assert np.float32(got.item()) == want, (n, paired, got.item(), want)
        assert all(float(t.grad) == -2.5 for t in terms), (n, paired)
    lib = _n.hip()
    terms = [torch.tensor(v, dtype=torch.float32, device=DEV) for v in vals]
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in terms])
    out = torch.zeros((), device=DEV)
    assert lib.wsis_loss_sum(arr, n, 1 << (n - 1), out.data_ptr(), _n.stream_ptr()) != 0
    assert b"successor" in lib.wsis_last_error() and float(out) == 0.0


# ---------------------------------------------------------------- MultiTaskLoss.forward

LEAVES = ("semantic_scores", "sp_semantic", "pred_off", "disc", "pred_occ", "pred_size")
TERMS = ("semantic_loss", "superpoint_semantic_loss", "offset_norm_loss", "offset_dir_loss",
         "superpoint_discriminative_loss", "occupancy_loss", "instance_size_loss")
FUSE_VARS = ("WSIS_FUSE_SEM_LOSS", "WSIS_FUSE_SP_CE", "WSIS_FUSE_SP_LOSS", "WSIS_FUSE_DISC_LOSS")
UP = 1.3


def _module_run(inp, slots, epoch=5, joint_epoch=0):
    leaves = {k: inp[k].to(DEV).requires_grad_(True) for k in LEAVES}
    d = lambda k: inp[k].to(DEV)
    loss_inp = {
        "point_labels": (d("sem_lab"), d("ins_lab")), "semantic_scores": leaves["semantic_scores"],
        "superpoint_labels": (d("sp_sem"), d("sp_ins")), "sp_semantic": leaves["sp_semantic"],
        "sp_offset_vector": (leaves["pred_off"], d("gt_off")), "sp_occupancy": (leaves["pred_occ"], d("gt_occ")),
        "sp_instance_size": (leaves["pred_size"], d("gt_size")),
        "sp_discriminative_features": (leaves["disc"], inp["sp_off"]), "sp_instance_slots": slots,
    }
    loss, loss_out = _crit(inp["semantic_scores"].shape[1], joint_epoch)(loss_inp, epoch)
    (loss * UP).backward()
    torch.cuda.synchronize()
    return loss.detach(), {k: v[0].detach() for k, v in loss_out.items()}, {k: v.grad for k, v in leaves.items()}, loss_out


def _dispatch_reference(inp, slots):
    leaves = {k: loss_ref.f64(inp[k], True) for k in LEAVES}
    sem, n_kept = loss_ref.semantic_point(leaves["semantic_scores"], inp["sem_lab"], IGN)
    ce, _, _ = loss_ref.sp_cross_entropy(leaves["sp_semantic"], inp["sp_sem"], IGN)
    l_norm, l_dir, l_occ, l_size, n_reg = loss_ref.sp_regression(
        leaves["pred_off"], loss_ref.f64(inp["gt_off"]), leaves["pred_occ"], loss_ref.f64(inp["gt_occ"]),
        leaves["pred_size"], loss_ref.f64(inp["gt_size"]), inp["sp_sem"], inp["sp_ins"], IGN)
    offs = [int(o) for o in inp["sp_off"]]
    scenes = [loss_ref.discriminative(leaves["disc"][b:e], inp["sp_ins"][b:e], inp["sp_sem"][b:e], slots[i], IGN)
              for i, (b, e) in enumerate(zip(offs[:-1], offs[1:]))]
    terms = dict(zip(TERMS, (sem, ce, l_norm, l_dir, torch.stack(scenes).mean(), l_occ, l_size)))
    total = sum(terms.values())
    (total * UP).backward()
    return total.detach(), {k: v.detach() for k, v in terms.items()}, {k: v.grad for k, v in leaves.items()}, n_kept, n_reg


def test_multitask_loss_dispatch(monkeypatch):
    """MultiTaskLoss.forward on a three-scene batch of 4,096 / 4,097 / 300 superpoints with slots [64, 64, 65]: the
    fused discriminative kernel for the first scene only (rows 4096 | 4097, slots 64 | 65); total, every loss_out
    entry and every leaf gradient against loss_ref -- with every WSIS_FUSE_* switch off (the bounds of
    tests/test_golden.py for the torch path) and on (the kernels' bounds; the discriminative term, on clustered
    embeddings, at 4 x the torch path's own error if that is larger); WSIS_BRANCH_LOSS=1 bit-identical to the default;
    epoch <= joint_training_epoch returns the point term alone"""
    for v in FUSE_VARS + ("WSIS_LOSS_INDEXED", "WSIS_BRANCH_LOSS", "WSIS_FUSE_LOSS_SUM", "WSIS_BRANCH"):
        monkeypatch.delenv(v, raising=False)
    inp, slots = loss_ref.dispatch_batch()
    want, want_terms, want_grads, n_kept, n_reg = _dispatch_reference(inp, slots)
    assert math.isfinite(_val(want)) and n_reg > 1000

    for v in FUSE_VARS:
        monkeypatch.setenv(v, "0")
    calls = []
    real = wsis_ops.discriminative_loss
    monkeypatch.setattr(wsis_ops, "discriminative_loss", lambda x, *a, **k: calls.append(x.shape[0]) or real(x, *a, **k))
    t_loss, t_terms, t_grads, _ = _module_run(inp, slots)
    assert not calls
    assert set(t_terms) == set(TERMS)
    for k in TERMS:
        assert np.allclose(_val(t_terms[k]), _val(want_terms[k]), rtol=1e-5, atol=1e-6), k
    assert np.allclose(_val(t_loss), _val(want), rtol=1e-5, atol=1e-6)
    for k in LEAVES:
        gmax = float(want_grads[k].abs().max())
        assert float((t_grads[k].double().cpu() - want_grads[k]).abs().max()) <= 1e-4 * gmax + G_FLOOR, k

    for v in FUSE_VARS:
        monkeypatch.delenv(v)
    loss, terms, grads, loss_out = _module_run(inp, slots)
    assert calls == [4096]
    assert set(terms) == set(TERMS)
    assert int(loss_out["semantic_loss"][1]) == n_kept and int(loss_out["offset_norm_loss"][1]) == n_reg
    assert int(loss_out["occupancy_loss"][1]) == n_reg and loss_out["superpoint_discriminative_loss"][1] == 8493
    tot_bound = 0.0
    for k in TERMS:
        disc = k == "superpoint_discriminative_loss"
        _check_loss(f"dispatch {k}", terms[k], want_terms[k], DISC_L if disc else SEM_L, t_terms[k] if disc else None)
        tot_bound += max((DISC_L if disc else SEM_L) * abs(_val(want_terms[k])) + 1e-7,
                         4.0 * abs(_val(t_terms[k]) - _val(want_terms[k])) if disc else 0.0)
    tot_bound += 8 * 2.0 ** -24 * sum(abs(_val(v)) for v in want_terms.values())      # the fp32 additions of the sum
    print(f"[loss-edges] dispatch total: loss {_val(want):.9g} kernel err {abs(_val(loss) - _val(want)):.3e} "
          f"fp32-torch err {abs(_val(t_loss) - _val(want)):.3e} bound {tot_bound:.3e}")
    assert abs(_val(loss) - _val(want)) <= tot_bound
    assert np.float32(_val(loss)) == loss_ref.loss_sum([_val(terms[k]) for k in TERMS], 1 << 2)
    for k in LEAVES:
        disc = k == "disc"
        _check_grad(f"dispatch d{k}", grads[k], want_grads[k], DISC_G if disc else SEM_G, t_grads[k] if disc else None)

    assert wsis_ops.branch_stream(torch.device(DEV, torch.cuda.current_device()), 1) is not None
    monkeypatch.setenv("WSIS_BRANCH_LOSS", "1")
    b_loss, b_terms, b_grads, _ = _module_run(inp, slots)
    monkeypatch.delenv("WSIS_BRANCH_LOSS")
    assert torch.equal(b_loss, loss) and all(torch.equal(b_terms[k], terms[k]) for k in TERMS)
    assert all(torch.equal(b_grads[k], grads[k]) for k in LEAVES)

    e_loss, e_terms, e_grads, _ = _module_run(inp, slots, epoch=3, joint_epoch=3)
    assert set(e_terms) == {"semantic_loss"} and torch.equal(e_loss, terms["semantic_loss"])
    assert torch.equal(e_grads["semantic_scores"], grads["semantic_scores"])
    assert all(e_grads[k] is None for k in LEAVES[1:])
