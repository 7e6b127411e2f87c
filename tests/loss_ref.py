"""Plain fp64 reference of the five loss terms of csrc/loss.hip, written from the formulas (reference
modules/model/losses_3D_WSIS.py:52-151, 157-253) and not from the code under test: CPU torch in float64 with
autograd, rows chosen by boolean selection as the reference project does.  An empty selection therefore gives what the
indexed formula gives: the mean of nothing (NaN) with zero gradients, or 0 / 1e-6 = 0 for the two offset terms.

Every function takes fp64 CPU tensors (``f64`` converts) and returns 0-dim fp64 tensors that autograd can walk."""
import numpy as np
import torch


def f64(t, grad=False):
    """detached fp64 CPU copy of a tensor (a fresh leaf when ``grad``)"""
    return t.detach().cpu().double().clone().requires_grad_(grad)


def _lab(t):
    return t.detach().cpu().long()


def _cross_entropy(rows, labels):
    """mean over the rows of logsumexp(row) - row[label]; NaN for no row"""
    m = rows.max(dim=1, keepdim=True).values if rows.shape[0] else rows.new_zeros(0, 1)
    lse = (rows - m).exp().sum(1).log() + m.squeeze(1)
    picked = rows.gather(1, labels.unsqueeze(1)).squeeze(1)
    return (lse - picked).mean()


def _softmax(rows):
    m = rows.max(dim=1, keepdim=True).values if rows.shape[0] else rows.new_zeros(0, 1)
    e = (rows - m).exp()
    return e / e.sum(1, keepdim=True)


def semantic_point(scores, labels, ignore=-100):
    """CE with ignore + mean_c(1 - (2 A_c + 1e-5) / (B_c + K_c + 1e-4 + 1e-5)) on the softmax of the kept rows.
    Returns (loss, n_kept)."""
    assert scores.dtype == torch.float64
    labels = _lab(labels)
    keep = labels != ignore
    rows, lab = scores[keep], labels[keep]
    C = scores.shape[1]
    ce = _cross_entropy(rows, lab)
    p = _softmax(rows)
    hit = torch.zeros(rows.shape[0], C, dtype=torch.float64)
    hit[torch.arange(rows.shape[0]), lab] = 1.0
    A, B, K = (p * hit).sum(0), (p * p).sum(0), hit.sum(0)
    dice = (2.0 * A + 1e-5) / (B + K + 1e-4 + 1e-5)
    return ce + (1.0 - dice).mean(), int(keep.sum())


def sp_cross_entropy(scores, labels, ignore=-100):
    """returns (loss, scores.sum(), n_kept)"""
    assert scores.dtype == torch.float64
    labels = _lab(labels)
    keep = labels != ignore
    return _cross_entropy(scores[keep], labels[keep]), scores.sum(), int(keep.sum())


def sp_regression(pred_off, gt_off, pred_occ, gt_occ, pred_size, gt_size, sem, ins, ignore=-100):
    """offset L1 and cosine over (n + 1e-6), occupancy and size L1 over n; rows with both labels set.
    Returns (l_norm, l_dir, l_occ, l_size, n)."""
    assert pred_off.dtype == torch.float64
    valid = (_lab(sem) != ignore) & (_lab(ins) != ignore)
    n = int(valid.sum())
    p, g = pred_off[valid], gt_off[valid]
    l_norm = (p - g).abs().sum(1).sum() / (n + 1e-6)
    gd = g / (torch.linalg.vector_norm(g, dim=1, keepdim=True) + 1e-8)
    pd = p / (torch.linalg.vector_norm(p, dim=1, keepdim=True) + 1e-8)
    l_dir = (-(gd * pd).sum(1)).sum() / (n + 1e-6)
    l_occ = (pred_occ.reshape(-1)[valid] - gt_occ.reshape(-1)[valid]).abs().mean()
    l_size = (pred_size.reshape(-1)[valid] - gt_size.reshape(-1)[valid]).abs().mean()
    return l_norm, l_dir, l_occ, l_size, n


def _disc_parts(x, ins, sem, n_slots, ignore):
    ins, sem = _lab(ins), _lab(sem)
    valid = (ins != ignore) & (sem != ignore) & (ins >= 0) & (ins < n_slots)
    rows, lab = x[valid], ins[valid]
    ids, inv, cnt = torch.unique(lab, return_inverse=True, return_counts=True)
    n = int(ids.numel())
    mu = torch.zeros(n, x.shape[1], dtype=torch.float64).index_add(0, inv, rows) / cnt.double().reshape(-1, 1)
    t = torch.linalg.vector_norm(rows - mu[inv], dim=1)
    l1 = (mu.unsqueeze(0) - mu.unsqueeze(1)).abs().sum(-1)
    return valid, rows, inv, cnt, n, mu, t, l1


def discriminative(x, ins, sem, n_slots, ignore=-100, delta_v=0.1, delta_d=1.5, p_var=1.0, p_dist=1.0, p_reg=0.001):
    """pull / push / regulariser over the instances present among the rows with both labels set and 0 <= ins < n_slots;
    the push term over ordered pairs, divided by max(n (n - 1), 1)"""
    assert x.dtype == torch.float64
    _, rows, inv, cnt, n, mu, t, l1 = _disc_parts(x, ins, sem, n_slots, ignore)
    pull = (t - delta_v).clamp(min=0.0).square()
    l_var = torch.zeros(n, dtype=torch.float64).index_add(0, inv, pull / cnt.double()[inv]).sum() / n
    off_diag = 1.0 - torch.eye(n, dtype=torch.float64)
    l_dist = ((2.0 * delta_d - l1).clamp(min=0.0).square() * off_diag).sum() / max(n * (n - 1), 1)
    l_reg = torch.linalg.vector_norm(mu, dim=1).sum()
    return p_var * l_var + p_dist * l_dist + p_reg * l_reg


def hinge_mix(x, ins, sem, n_slots, ignore=-100, delta_v=0.1, delta_d=1.5):
    """(fraction of the ordered instance pairs with an active push hinge, fraction of the counted rows with an active
    pull hinge, number of ordered pairs) of a scene, in fp64"""
    _, rows, inv, cnt, n, mu, t, l1 = _disc_parts(f64(x), ins, sem, n_slots, ignore)
    pairs = n * (n - 1)
    off = ~torch.eye(n, dtype=torch.bool)
    push = float(((l1 < 2.0 * delta_d) & off).sum()) / pairs if pairs else float("nan")
    pull = float((t > delta_v).sum()) / max(int(rows.shape[0]), 1)
    return push, pull, pairs


def loss_sum(values, paired=0):
    """t_0 + t_1 + ... in numpy float32, left to right; bit i of ``paired`` adds (t_i + t_{i+1}) first"""
    v = [np.float32(x) for x in values]
    acc, i = None, 0
    while i < len(v):
        term = v[i]
        if (paired >> i) & 1:
            term = np.float32(term + v[i + 1])
            i += 1
        acc = term if acc is None else np.float32(acc + term)
        i += 1
    return acc


def clustered_embeddings(S, I, seed, centre_scale=0.4, spread=0.04):
    """trained-looking embeddings: I centres randn(I, 7) * centre_scale, S rows = the centre of a uniformly drawn
    instance + randn * spread.  Returns (x fp32 [S, 7], instance ids int64 [S])."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(I, 7, generator=g) * centre_scale
    ins = torch.randint(0, I, (S,), generator=g)
    x = centres[ins] + torch.randn(S, 7, generator=g) * spread
    return x.float(), ins


# the clustered scenes of tests/test_gpu_loss_edges.py: (S, I, seed, centre_scale, spread); the host suite asserts that
# both hinges of every one are active on 20 % .. 80 % of their pairs / rows
CLUSTERED_CASES = [
    (600, 12, 0, 0.4, 0.04),
    (4096, 64, 0, 0.4, 0.04),
    (4095, 43, 0, 0.4, 0.04),
    (2289, 33, 0, 0.4, 0.04),
    (300, 9, 0, 0.4, 0.04),
    (64, 8, 0, 0.4, 0.04),
    (5, 1, 0, 0.4, 0.04),
    (1000, 16, 0, 0.4, 0.04),       # 8 row chunks
    (900, 32, 0, 0.4, 0.04),        # 4 row chunks
]
# the three scenes of the dispatch batch: (rows, slots, instances, seed, centre_scale, spread)
DISPATCH_SCENES = [
    (4096, 64, 60, 1, 0.4, 0.04),
    (4097, 64, 50, 2, 0.4, 0.04),
    (300, 65, 65, 3, 0.4, 0.04),
]


def dispatch_batch(n_points=20000, classes=20, ignore=-100, seed=11):
    """one synthetic three-scene batch for MultiTaskLoss.forward (CPU tensors, fp32 / int64): the scenes of
    DISPATCH_SCENES, a fifth of the superpoints without semantic label, a fifth without instance label, -inf occupancy
    targets on the dropped rows.  Returns (inputs, slots): ``inputs`` holds the six prediction tensors under the names of
    tests/test_golden.py's leaves plus the labels, targets and scene offsets."""
    g = torch.Generator().manual_seed(seed)
    xs, ids = zip(*[clustered_embeddings(S, I, sd, cs, sp) for S, _, I, sd, cs, sp in DISPATCH_SCENES])
    disc, sp_ins = torch.cat(xs), torch.cat(ids)
    S = disc.shape[0]
    sp_sem = torch.randint(0, classes, (S,), generator=g)
    sp_sem[torch.rand(S, generator=g) < 0.2] = ignore
    sp_ins[torch.rand(S, generator=g) < 0.2] = ignore
    valid = (sp_sem != ignore) & (sp_ins != ignore)
    sem_lab = torch.randint(0, classes, (n_points,), generator=g)
    sem_lab[torch.rand(n_points, generator=g) < 0.6] = ignore
    gt_occ = torch.randn(S, generator=g)
    gt_occ[~valid] = float("-inf")
    offs = [0]
    for sc in DISPATCH_SCENES:
        offs.append(offs[-1] + sc[0])
    inputs = {
        "semantic_scores": torch.randn(n_points, classes, generator=g) * 3, "sem_lab": sem_lab,
        "ins_lab": torch.zeros(n_points, dtype=torch.int64),
        "sp_semantic": torch.randn(S, classes, generator=g) * 3, "sp_sem": sp_sem, "sp_ins": sp_ins,
        "pred_off": torch.randn(S, 3, generator=g), "gt_off": torch.randn(S, 3, generator=g),
        "pred_occ": torch.randn(S, generator=g), "gt_occ": gt_occ,
        "pred_size": torch.randn(S, generator=g), "gt_size": torch.rand(S, generator=g),
        "disc": disc, "sp_off": torch.tensor(offs),
    }
    return inputs, [sc[1] for sc in DISPATCH_SCENES]
