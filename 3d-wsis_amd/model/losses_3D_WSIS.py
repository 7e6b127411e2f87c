"""``MultiTaskLoss`` of 3D-WSIS (caller side of the hot path) -- same constructor, forward
signature, ``loss_inp`` keys and returned ``(loss, loss_out)`` as the reference's
modules/model/losses_3D_WSIS.py:13-253; pinned against the imported reference by tests/golden/loss_golden.npz.

Pure torch; ``device`` follows the inputs instead of the reference's hard-coded 'cuda' attribute (:33).

Two evaluations of the same formulas: the reference's shape (boolean-mask indexing, ``torch.unique`` -- every one of
them a device->host sync, 12+ per step) and the default MASKED one, which keeps every intermediate at its full,
host-known shape (rows that the reference drops get weight 0; per-instance means come from a dense same-instance
matrix instead of ``unique``), so the host never waits for the GPU inside the loss and can keep issuing the backward
pass while the forward is still running.  ``WSIS_LOSS_INDEXED=1`` selects the reference-shaped evaluation; both are
checked against the golden vectors."""
import functools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F


class _NullLogger(object):
    def info(self, *a, **k):
        pass


def _ops():
    """the device operators and their kernels' limits: the one import site, lazy (the host evaluations do without)"""
    import wsis_ops
    return wsis_ops


def _on(switch, default="1"):
    return os.environ.get(switch, default) != "0"


class MultiTaskLoss(nn.Module):
    def __init__(self, logger, param_loss, param_model):
        super().__init__()
        self.logger = logger if logger is not None else _NullLogger()
        self.ignore_label = param_loss.ignore_label
        self.supervise_instance_size = param_loss.supervise_instance_size
        self.joint_training_epoch = param_loss.joint_training_epoch
        self.semantic_dice = param_loss.semantic_dice
        self.semantic_class_num = param_model.classes
        self.discriminative_feature_dim = 7
        self.delta_v = 0.1
        self.delta_d = 1.5
        self.param_var = 1.
        self.param_dist = 1.
        self.param_reg = 0.001
        self.supervise_sp_offset = getattr(param_loss, "supervise_sp_offset", True)
        self.log_values = getattr(param_loss, "log_values", False)   # the reference logs (= syncs) every term
        self.semantic_criterion = nn.CrossEntropyLoss(ignore_index=self.ignore_label)
        self.occupany_L1loss = nn.L1Loss()
        self.instance_size_L1loss = nn.L1Loss()
        self.superpoint_semantic_criterion = nn.CrossEntropyLoss(ignore_index=self.ignore_label)

    def _log(self, name, value):
        if self.log_values:
            self.logger.info("{}: {:.4f}".format(name, value))

    def forward(self, loss_inp, epoch):
        loss_out = {}
        indexed = os.environ.get("WSIS_LOSS_INDEXED", "0") == "1"

        @functools.lru_cache(maxsize=None)
        def valid():
            # (mask, count) of the superpoints that both labels keep: only the unfused branches read them (the fused
            # kernels take the two label tensors), so they are formed on first use -- four launches the default device
            # path never needs
            sp_sem_labels, sp_ins_labels = loss_inp["superpoint_labels"]
            m = (sp_ins_labels != self.ignore_label) & (sp_sem_labels != self.ignore_label)
            return m, m.sum()

        semantic_loss, side_join = self._point_semantic(loss_inp, indexed, loss_out)
        terms, paired = [("point semantic loss", semantic_loss)], 0
        if epoch > self.joint_training_epoch:
            terms.append(("sp semantic loss", self._sp_semantic(loss_inp, indexed, loss_out)))
            offset_norm, offset_dir, occupancy, instance_size, n_reg = self._sp_regression(loss_inp, indexed, valid)
            if self.supervise_sp_offset:
                loss_out["offset_norm_loss"], loss_out["offset_dir_loss"] = (offset_norm, n_reg), (offset_dir, n_reg)
                paired |= 1 << len(terms)                  # loss + (offset_norm_loss + offset_dir_loss)
                terms += [("sp offset norm loss", offset_norm), ("sp offset dir loss", offset_dir)]
            terms.append(("sp discriminative loss", self._sp_discriminative(loss_inp, indexed, valid, loss_out)))
            if self.supervise_instance_size:
                loss_out["occupancy_loss"], loss_out["instance_size_loss"] = (occupancy, n_reg), (instance_size, n_reg)
                terms += [("sp occupancy loss", occupancy), ("sp instance size loss", instance_size)]
        if side_join is not None:       # the point term joins the others here
            main, side, made = side_join
            main.wait_stream(side)
            for t in made:
                t.record_stream(main)
        return self._sum_terms(terms, paired), loss_out

    def _point_semantic(self, inp, indexed, loss_out):
        """CrossEntropy(ignore_index) (+ dice) of the point scores -> (term, side-stream join or None)"""
        semantic_labels, semantic_scores = inp["point_labels"][0], inp["semantic_scores"]
        if (not indexed and self.semantic_dice and semantic_scores.is_cuda and _on("WSIS_FUSE_SEM_LOSS")
                and semantic_scores.shape[1] <= _ops().LOSS_MAX_CLASSES):
            # CE + dice in two passes over [N, C] (csrc/loss.hip) instead of ~40 torch launches
            wsis_ops = _ops()
            # on the point-level head's branch stream (backbone_3D_WSIS.py): the two passes over [N, C] and their backward
            # run beside the superpoint terms instead of in front of them
            side = wsis_ops.branch_stream(semantic_scores.device, 1)
            join = None
            if side is not None and _on("WSIS_BRANCH_LOSS", "0"):      # (measured: within the noise)
                main = torch.cuda.current_stream()
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    semantic_loss, n_kept = wsis_ops.semantic_point_loss(semantic_scores, semantic_labels,
                                                                         self.ignore_label)
                semantic_scores.record_stream(side)
                semantic_labels.record_stream(side)
                join = (main, side, (semantic_loss, n_kept))
            else:
                semantic_loss, n_kept = wsis_ops.semantic_point_loss(semantic_scores, semantic_labels, self.ignore_label)
            loss_out["semantic_loss"] = (semantic_loss, n_kept)
            return semantic_loss, join
        semantic_loss = self.semantic_criterion(semantic_scores, semantic_labels)
        if self.semantic_dice:
            keep = semantic_labels != self.ignore_label
            if indexed:
                semantic_scores = F.softmax(semantic_scores[keep], dim=-1)
                one_hot = F.one_hot(semantic_labels[keep], num_classes=self.semantic_class_num)
            else:       # dropped rows -> zero rows: every column sum of the dice terms is unchanged
                w = keep.unsqueeze(1).to(semantic_scores.dtype)
                semantic_scores = F.softmax(semantic_scores, dim=-1) * w
                # (dropped rows -> class 0: any ignore_label, negative or not, stays inside one_hot's range)
                one_hot = F.one_hot(torch.where(keep, semantic_labels, torch.zeros_like(semantic_labels)),
                                    num_classes=self.semantic_class_num) * w
            semantic_loss = semantic_loss + dice_loss_multi_classes(semantic_scores, one_hot).mean()
        loss_out["semantic_loss"] = (semantic_loss, semantic_scores.sum())
        return semantic_loss, None

    def _sp_semantic(self, inp, indexed, loss_out):
        """CrossEntropy(ignore_index) of the superpoint scores, logged with their sum"""
        scores, sp_sem_labels = inp["sp_semantic"], inp["superpoint_labels"][0]
        if (not indexed and scores.is_cuda and scores.dim() == 2 and scores.shape[0] >= 1
                and _on("WSIS_FUSE_SP_CE") and scores.shape[1] <= _ops().LOSS_MAX_CLASSES):
            # cross entropy + the logged sum of the scores: one launch each way (csrc/loss.hip)
            loss, score_sum = _ops().superpoint_cross_entropy(scores, sp_sem_labels, self.ignore_label)
        else:
            loss = self.superpoint_semantic_criterion(scores, sp_sem_labels)
            score_sum = scores.sum()
        loss_out["superpoint_semantic_loss"] = (loss, score_sum)
        return loss

    def _sp_regression(self, inp, indexed, valid):
        """offset L1, offset cosine, occupancy L1 and instance-size L1 over the labelled superpoints and their number
        (None for a term that is not supervised)"""
        if (not indexed and self.supervise_sp_offset and self.supervise_instance_size
                and inp["sp_offset_vector"][0].is_cuda and _on("WSIS_FUSE_SP_LOSS")):
            return _ops().sp_regression_losses(      # all four in one launch (csrc/loss.hip)
                *inp["sp_offset_vector"], *inp["sp_occupancy"], *inp["sp_instance_size"], *inp["superpoint_labels"],
                self.ignore_label)
        sp_valid, n_valid = valid()
        offset_norm_loss = offset_dir_loss = occupancy_loss = instance_size_loss = None
        if self.supervise_sp_offset:
            pred_off, gt_off = inp["sp_offset_vector"]
            pt_dist = torch.sum(torch.abs(pred_off - gt_off), dim=-1)
            offset_norm_loss = torch.sum(pt_dist * sp_valid) / (n_valid + 1e-6)
            gt_dir = gt_off / (torch.norm(gt_off, p=2, dim=1).unsqueeze(-1) + 1e-8)
            pt_dir = pred_off / (torch.norm(pred_off, p=2, dim=1).unsqueeze(-1) + 1e-8)
            direction_diff = -(gt_dir * pt_dir).sum(-1)
            offset_dir_loss = torch.sum(direction_diff * sp_valid) / (n_valid + 1e-6)
        if self.supervise_instance_size:
            pred_occ, gt_occ = inp["sp_occupancy"]
            pred_size, gt_size = inp["sp_instance_size"]
            if indexed:
                occupancy_loss = self.occupany_L1loss(pred_occ[sp_valid], gt_occ[sp_valid])
                instance_size_loss = self.instance_size_L1loss(pred_size[sp_valid], gt_size[sp_valid])
            else:
                occupancy_loss = _masked_l1(pred_occ, gt_occ, sp_valid)
                instance_size_loss = _masked_l1(pred_size, gt_size, sp_valid)
        return offset_norm_loss, offset_dir_loss, occupancy_loss, instance_size_loss, n_valid

    def _sp_discriminative(self, inp, indexed, valid, loss_out):
        """mean over the scenes of the pull / push / reg loss of their superpoint embeddings"""
        feats, sp_batch_offsets = inp["sp_discriminative_features"]
        sp_sem_labels, sp_ins_labels = inp["superpoint_labels"]
        offs = [int(o) for o in sp_batch_offsets]
        slots = inp.get("sp_instance_slots")      # host-known bound of the instance ids per scene (optional)
        d_losses = []
        for i in range(1, len(offs)):
            b, e = offs[i - 1], offs[i]
            n_slots = int(slots[i - 1]) if slots is not None else 0
            ins = sp_ins_labels[b:e]
            if indexed:
                keep = valid()[0][b:e]
                d_loss, _, _, _ = self.discriminative_loss(feats[b:e][keep], ins[keep])
            elif (feats.is_cuda and self.discriminative_feature_dim == 7 and _on("WSIS_FUSE_DISC_LOSS")
                  and 1 <= n_slots <= _ops().DISC_MAX_SLOTS and 1 <= e - b <= _ops().DISC_MAX_ROWS):
                # one launch each way (csrc/loss.hip)
                d_loss = _ops().discriminative_loss(feats[b:e], ins, sp_sem_labels[b:e], n_slots, self.ignore_label,
                                                    self.delta_v, self.delta_d, self.param_var, self.param_dist,
                                                    self.param_reg)
            elif 1 <= n_slots <= 512:
                d_loss = self.discriminative_loss_slots(feats[b:e], ins, valid()[0][b:e], n_slots)
            else:
                d_loss = self.discriminative_loss_masked(feats[b:e], ins, valid()[0][b:e])
            d_losses.append(d_loss.view(-1))
        # mean over the scenes; one scene: the mean of one value is that value (x / 1 is exact)
        sp_d_loss = torch.mean(torch.cat(d_losses)) if len(d_losses) != 1 else d_losses[0].reshape(())
        loss_out["superpoint_discriminative_loss"] = (sp_d_loss, feats.shape[0])
        return sp_d_loss

    def _sum_terms(self, terms, paired):
        """the terms and the pairs of the reference's expression (losses_3D_WSIS.py:130-151: loss = 0.0 + 1.0 * term +
        ...), summed left to right.  All weights are 1.0 there, and 0.0 + x and 1.0 * x are exact in floating point: the
        same sum in the same order without the seven scalar multiplications (each one a launch forward and one backward)"""
        for name, t in terms:
            self._log(name, t)
        terms = [t for _, t in terms]
        if (len(terms) > 1 and all(torch.is_tensor(t) and t.is_cuda and t.numel() == 1 for t in terms)
                and _on("WSIS_FUSE_LOSS_SUM") and len(terms) <= _ops().LOSS_SUM_MAX_TERMS):
            return _ops().loss_sum(terms, paired)      # one launch instead of one per `loss = loss + term`
        loss, i = terms[0], 1
        while i < len(terms):
            pair = (paired >> i) & 1       # bit i: loss + (t_i + t_i+1)
            loss = loss + ((terms[i] + terms[i + 1]) if pair else terms[i])
            i += 1 + pair
        return loss

    def discriminative_loss(self, prediction, correct_label):
        """pull (delta_v) / push (L1 cdist, delta_d) / reg terms over the instances of one scene
        (losses_3D_WSIS.py:157-230)."""
        dev = prediction.device
        pred = torch.reshape(prediction, [-1, self.discriminative_feature_dim])
        unique_labels, unique_id, counts = torch.unique(correct_label, sorted=False, return_inverse=True,
                                                        return_counts=True)
        counts = counts.float()
        n = unique_labels.size(0)
        seg_sum = torch.zeros(n, self.discriminative_feature_dim, device=dev).index_add_(0, unique_id, pred)
        mu = seg_sum / counts.reshape(-1, 1)
        dist = torch.norm(pred - mu[unique_id], p=2, dim=1)
        dist = torch.square(torch.clamp(dist - self.delta_v, min=0.))
        l_var = torch.zeros(n, device=dev).index_add_(0, unique_id, dist)
        l_var = torch.sum(l_var / counts) / n
        if n <= 1:
            l_dist = torch.tensor(0., device=dev)
        else:
            d = 2. * self.delta_d - torch.cdist(mu, mu, p=1)
            d = d - torch.diagflat(torch.diag(d, 0))
            l_dist = torch.sum(torch.square(torch.clamp(d, min=0.))) / (n * (n - 1))
        l_reg = torch.sum(torch.norm(mu, p=2, dim=1))
        l_var = self.param_var * l_var
        l_dist = self.param_dist * l_dist
        l_reg = self.param_reg * l_reg
        return l_var + l_dist + l_reg, l_var, l_dist, l_reg

    def discriminative_loss_slots(self, prediction, label, valid, n_slots):
        """the same terms with the instances in ``n_slots`` fixed slots (slot = instance id; ``n_slots`` is a bound the
        HOST knows from the batch, so no ``unique`` and no sync): a one-hot [S, n_slots] membership matrix replaces
        the [S, S] same-instance matrix of ``discriminative_loss_masked`` -- instance means by one small GEMM, the
        push term on [n_slots, n_slots] instead of [S, S].  Empty slots carry weight 0.  Deterministic (no atomics)."""
        pred = torch.reshape(prediction, [-1, self.discriminative_feature_dim])
        slot = torch.arange(n_slots, device=pred.device, dtype=label.dtype)
        oh = ((label.unsqueeze(1) == slot.unsqueeze(0)) & valid.unsqueeze(1)).to(pred.dtype)      # [S, I]
        cnt = oh.sum(0)                                          # members per slot
        present = (cnt > 0).to(pred.dtype)
        n = present.sum()                                        # number of instances (0-dim tensor, no sync)
        inv = 1.0 / cnt.clamp(min=1.0)
        mu = (oh.t() @ pred) * inv.unsqueeze(1)                  # [I, D] instance means (0 for empty slots)
        mu_rows = oh @ mu                                        # [S, D] the mean of the row's instance
        dist = torch.norm(pred - mu_rows, p=2, dim=1)
        dist = torch.square(torch.clamp(dist - self.delta_v, min=0.))
        w = oh @ inv                                             # [S] 1 / size of the row's instance, 0 if dropped
        l_var = torch.sum(dist * w) / n.clamp(min=1.0)           # (n >= 1: x / n unchanged; n == 0: see _nan_if_empty)
        l1 = (mu.unsqueeze(0) - mu.unsqueeze(1)).abs().sum(-1)   # [I, I]
        d = 2. * self.delta_d - l1
        pair = present.unsqueeze(0) * present.unsqueeze(1) * (1.0 - torch.eye(n_slots, device=pred.device, dtype=pred.dtype))
        l_dist = torch.sum(torch.square(torch.clamp(d, min=0.)) * pair) / torch.clamp(n * (n - 1), min=1.0)
        l_reg = torch.sum(torch.norm(mu, p=2, dim=1) * present)
        return _nan_if_empty(self.param_var * l_var + self.param_dist * l_dist + self.param_reg * l_reg, n)

    def discriminative_loss_masked(self, prediction, label, valid):
        """the same pull / push / reg terms (losses_3D_WSIS.py:157-230) without ``unique`` / mask indexing: rows with
        ``valid`` False get weight 0; same[i,j] = both valid and the same instance; count_i = size of i's
        instance; an instance-level sum over c becomes a row-level sum weighted by 1/count_i."""
        pred = torch.reshape(prediction, [-1, self.discriminative_feature_dim])
        v = valid.to(pred.dtype)
        same = ((label.unsqueeze(0) == label.unsqueeze(1)) & valid.unsqueeze(0) & valid.unsqueeze(1)).to(pred.dtype)
        count = same.sum(1).clamp(min=1.0)                       # [S] (1 for invalid rows: their weight is 0 anyway)
        w = v / count                                            # sums to 1 over each instance
        n = torch.round(w.sum())                                 # number of instances (0-dim tensor, no sync)
        mu = (same @ pred) / count.unsqueeze(1)                  # [S,D]: the mean of the row's instance
        dist = torch.norm(pred - mu, p=2, dim=1)
        dist = torch.square(torch.clamp(dist - self.delta_v, min=0.))
        l_var = torch.sum(dist * w) / n.clamp(min=1.0)           # (n >= 1: x / n unchanged; n == 0: see _nan_if_empty)
        # L1 distance of every row pair (row pair (i,j) stands for instance pair (c_i,c_j)).  Broadcast form:
        # torch.cdist(p=1) took 0.85 ms forward + 0.52 ms backward for 1190 rows (one thread per pair, 7-term loop)
        l1 = (mu.unsqueeze(0) - mu.unsqueeze(1)).abs().sum(-1)
        d = 2. * self.delta_d - l1
        other = (1.0 - same) * v.unsqueeze(0) * v.unsqueeze(1)   # valid rows of DIFFERENT instances
        pair_w = other * w.unsqueeze(0) * w.unsqueeze(1)         # every ordered instance pair weighs 1 in total
        l_dist = torch.sum(torch.square(torch.clamp(d, min=0.)) * pair_w) / torch.clamp(n * (n - 1), min=1.0)
        l_reg = torch.sum(torch.norm(mu, p=2, dim=1) * w)
        return _nan_if_empty(self.param_var * l_var + self.param_dist * l_dist + self.param_reg * l_reg, n)


def _nan_if_empty(value, n):
    """``value`` for n > 0, NaN for n == 0 -- what the reference's mean over an empty selection gives.  The NaN is
    SELECTED, not computed: ``value`` is formed with its denominator clamped to 1, so the untaken branch hands a zero
    gradient (not 0 * inf = NaN) to every input, as boolean indexing does, and the other loss terms of a crop without
    a labelled superpoint still train.  For n > 0 value and gradient keep their bits."""
    return torch.where(n > 0, value, torch.full_like(value, float("nan")))


def _masked_l1(pred, target, row_valid):
    """nn.L1Loss()(pred[row_valid], target[row_valid]) without the boolean indexing; dropped rows are selected away,
    not multiplied by 0 (the log voxel count of an unlabelled superpoint is -inf, and inf * 0 is NaN)"""
    w = row_valid
    while w.dim() < pred.dim():
        w = w.unsqueeze(-1)
    per_row = pred[0].numel() if pred.dim() > 1 else 1
    diff = torch.abs(pred - target)
    den = row_valid.sum() * per_row
    return _nan_if_empty(torch.sum(torch.where(w, diff, torch.zeros_like(diff))) / den.clamp(min=1), den)


def dice_loss_multi_classes(input, target, epsilon=1e-5, weight=None):
    """per-class dice on [N, nClass] probabilities / one-hot targets (losses_3D_WSIS.py:233-253)"""
    assert input.size() == target.size()
    input = input.transpose(0, 1)
    target = target.transpose(0, 1).float()
    dice = (2 * torch.sum(input * target, dim=1) + epsilon) / \
           (torch.sum(input * input, dim=1) + torch.sum(target * target, dim=1) + 1e-4 + epsilon)
    return 1. - dice
