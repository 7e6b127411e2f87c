"""AdamW step of the training iteration (``train_scannetv2.py:251``, optimizer of
``config/ScanNet_v2_3D_WSIS.yaml:58-61``) as ONE launch of ``wsis_adamw_step`` over all parameters -- of
``wsis_adamw_step_groups`` when the optimizer has several parameter groups, each with its own learning rate, betas, eps
and weight decay (``split_decay_groups`` makes the usual pair: weights with decay, norm parameters and biases without).

Same update rule as ``torch.optim.AdamW`` (tested against it step by step); the moments live in two flat buffers, a
small (pointer, size) table per step tells the kernel where each parameter, gradient and moment slice is.  The table
goes through a ring of pinned host buffers: the copy of step t is still queued on the stream while the host already
prepares step t+1 (gradient tensors of most parameters are new objects every backward pass).

fp16 training: ``LossScaler`` is dynamic loss scaling with its state on the device -- the non-finite check
(``wsis_grad_nonfinite``), the unscale, the skip decision and the step count (``wsis_adamw_step_scaled``) and the scale
update (``wsis_loss_scale_update``) are three launches, and nothing is read back: the host never learns whether a step
was skipped.  ``torch.amp.GradScaler`` drives ``FlatAdamW`` through torch's fused-optimizer protocol as well."""
import numpy as np
import torch

import wsis_native as _n

_RING = 4
_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay")
_UNSUPPORTED = ("amsgrad", "maximize", "foreach", "capturable")       # other update rules / other launch plans


def group_rows(param_groups):
    """the group table of wsis_adamw_step_groups: float64 [G, 5] = (lr, beta1, beta2, eps, weight_decay) per group, read
    from the live group dicts"""
    return np.array([[g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]] for g in param_groups],
                    dtype=np.float64).reshape(len(param_groups), 5)


def trainable(params):
    """the parameters of one group the optimizer keeps: those that require a gradient, in order"""
    return [p for p in params if p.requires_grad]


def segment_groups(group_sizes):
    """group index of every segment of the flat parameter list (the groups' lists concatenated in group order); an
    empty group keeps its index and owns no segment"""
    return np.repeat(np.arange(len(group_sizes), dtype=np.int32), np.asarray(group_sizes, dtype=np.int64))


def group_param_indices(group_sizes):
    """``params`` of every group in a state_dict: indices into the flat list, counting on across groups (the layout of
    torch.optim.Optimizer.state_dict)"""
    ends = np.cumsum([0] + list(group_sizes))
    return [list(range(int(a), int(b))) for a, b in zip(ends[:-1], ends[1:])]


def split_decay_groups(model, weight_decay, no_decay_types=(torch.nn.BatchNorm1d,), no_decay_bias=True):
    """two parameter groups over the trainable parameters of ``model``: weights with ``weight_decay``, then the
    parameters of ``no_decay_types`` modules and (``no_decay_bias``) every bias with ``weight_decay=0``.  Every
    parameter that requires a gradient lands in exactly one of them (a shared one where it is met first)."""
    decay, no_decay, seen = [], [], set()
    for module in model.modules():
        for name, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            plain = isinstance(module, tuple(no_decay_types)) or (no_decay_bias and name.split("_")[0] == "bias")
            (no_decay if plain else decay).append(p)
    return [{"params": decay, "weight_decay": float(weight_decay)}, {"params": no_decay, "weight_decay": 0.0}]


def _checked_group(group):
    """a copy of a caller's group dict with the parameters that need no gradient dropped; what FlatAdamW's one update
    rule cannot do is refused"""
    if not isinstance(group, dict):
        raise TypeError("a parameter group is a dict")
    group = dict(group)
    params = group["params"]
    group["params"] = trainable([params] if isinstance(params, torch.Tensor) else list(params))
    for k in _UNSUPPORTED:
        if group.get(k):
            raise ValueError(f"FlatAdamW: {k} is not supported")
    return group


class FlatAdamW(torch.optim.Optimizer):
    """A ``torch.optim.Optimizer`` with the constructor of ``torch.optim.AdamW``: an iterable of tensors or a list of
    group dicts with their own ``lr``, ``betas``, ``eps``, ``weight_decay``.  ``param_groups`` is live -- every step reads
    the hyper-parameters from it, so the reference's ``PolyLR`` (an ``_LRScheduler``, stepped per epoch,
    ``utils/lr_scheduler.py``), a ``LambdaLR`` with one lambda per group and the reference's ``save_checkpoint``
    isinstance check work on it unchanged.  Parameters that need no gradient are dropped inside their group; a group left
    empty keeps its index.  However many groups, a step is ONE launch: a segment names its group, the kernel reads that
    group's row (``wsis_adamw_step_groups``); one group takes ``wsis_adamw_step`` as it always did.  ``params``, ``steps``,
    ``exp_avg``, ``exp_avg_sq`` are flat over the groups' lists in group order.

    Loss scaling: the step honours torch's protocol attributes ``grad_scale`` and ``found_inf`` (fp32 one-element device
    tensors; absent or None: scale 1 / never skipped), so ``torch.amp.GradScaler.step`` hands both over without reading
    ``found_inf`` back.  A step the device skips writes nothing and counts itself per parameter on the device
    (``_skipped``); ``steps`` keeps counting calls with a gradient.  A parameter without a gradient clamp keeps the SCALED
    values in ``.grad`` after a scaled step (the step does not write its gradient back); a clamped one holds the clamped
    unscaled values."""
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        params = list(params)
        if not (params and isinstance(params[0], dict)):
            params = [{"params": params}]
        groups = [_checked_group(g) for g in params]
        if not any(g["params"] for g in groups):
            raise ValueError("no parameters to optimise")
        self.params = []                                            # flat: the groups' lists in group order
        self.steps = np.zeros(0, dtype=np.int64)                    # updates per parameter (torch counts per parameter)
        self.exp_avg = self.exp_avg_sq = None
        self._table = np.zeros((0, 7), dtype=np.int64)              # p, g, m, v, numel, (step_size, inv_sqrt_bc2), (g_clamp fp32, group int32)
        self._numel = np.zeros(0, dtype=np.int64)
        self._total = 0                                             # floats in each moment buffer
        self._done = [None] * _RING
        self._skipped = None        # int32 [n]: steps the device skipped, per parameter; made by the first scaled step
        self._laid_out = False
        super().__init__(groups, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                      weight_decay=float(weight_decay)))
        self._layout()
        self._laid_out = True

    def add_param_group(self, param_group):
        """torch's rules (defaults filled in, a parameter already present is a ValueError) behind the filter of the
        constructor; moments, counts, skip counters and clamps of the parameters already here survive"""
        super().add_param_group(_checked_group(param_group))
        if self.__dict__.get("_laid_out"):
            self._layout()

    def _layout(self):
        """(re)build what depends on the parameter list.  Groups are only ever appended, so the flat list grows at its
        end: old moment slices keep their offsets, new ones are zero with count 0."""
        params = [p for g in self.param_groups for p in g["params"]]
        n0, n = len(self.params), len(params)
        assert all(a is b for a, b in zip(self.params, params))
        dev = params[0].device
        if dev.type != "cuda":
            raise _n.WsisError("FlatAdamW runs on the MI355X only (there is no CPU fallback)")
        for p in params[n0:]:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("FlatAdamW expects contiguous fp32 parameters on one device")
        lib = _n.hip()
        assert lib.wsis_adamw_segment_bytes() == 56 and lib.wsis_adamw_group_bytes() == 40
        chunk = lib.wsis_adamw_chunk()
        numel = np.asarray([p.numel() for p in params], dtype=np.int64)
        # moments: one flat buffer each; slices start at multiples of 4 floats so the float4 path applies
        padded = (numel + 3) // 4 * 4
        starts = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        total = int(padded.sum())
        for name in ("exp_avg", "exp_avg_sq"):
            buf = torch.zeros(total, dtype=torch.float32, device=dev)
            if self._total:
                buf[:self._total].copy_(getattr(self, name))
            setattr(self, name, buf)
        self.steps = np.concatenate([self.steps, np.zeros(n - n0, dtype=np.int64)])
        if self._skipped is not None:
            self._skipped = torch.cat([self._skipped, torch.zeros(n - n0, dtype=torch.int32, device=dev)])
        table = np.zeros((n, 7), dtype=np.int64)
        table[:n0] = self._table                                    # the clamps of set_grad_clamp
        table[:, 2] = self.exp_avg.data_ptr() + 4 * starts
        table[:, 3] = self.exp_avg_sq.data_ptr() + 4 * starts
        self._group_of = segment_groups([len(g["params"]) for g in self.param_groups])
        table.view(np.int32)[:, 13] = self._group_of
        self.params, self._table, self._numel, self._total = params, table, numel, total
        blocks = np.concatenate([np.stack([np.full((k + chunk - 1) // chunk, i, dtype=np.int32),
                                           np.arange((k + chunk - 1) // chunk, dtype=np.int32)], 1)
                                 for i, k in enumerate(numel.tolist())])
        self._blocks = torch.from_numpy(np.ascontiguousarray(blocks)).to(dev)
        self._n_blocks = int(blocks.shape[0])
        # one ring slot = the segment rows, then the [G, 5] group rows: a step issues one host-to-device copy
        for ev in self._done:
            if ev is not None:
                ev.synchronize()            # a copy out of the old pinned buffers may still be queued
        words = 7 * n + 5 * len(self.param_groups)
        self._host = [torch.empty(words, dtype=torch.int64).pin_memory() for _ in range(_RING)]
        self._dev = [torch.empty(words, dtype=torch.int64, device=dev) for _ in range(_RING)]
        self._done = [None] * _RING
        self._slot = 0

    # hyper-parameters live in param_groups (schedulers write there); the attributes are views of group 0
    lr = property(lambda self: float(self.param_groups[0]["lr"]),
                  lambda self, v: self.param_groups[0].__setitem__("lr", float(v)))
    betas = property(lambda self: tuple(float(b) for b in self.param_groups[0]["betas"]))
    eps = property(lambda self: float(self.param_groups[0]["eps"]))
    weight_decay = property(lambda self: float(self.param_groups[0]["weight_decay"]))

    def set_grad_clamp(self, params, bound):
        """gradients of ``params`` are clamped to [-bound, bound] inside the step's ONE launch (and written back, like the
        reference's ``p.grad.data.clamp_(-1, 1)`` over the ECC parameters, train_scannetv2.py:247-249); bound <= 0: off"""
        ids = {id(p) for p in params}
        clamp = self._table.view(np.float32)[:, 12]
        n = 0
        for i, p in enumerate(self.params):
            if id(p) in ids:
                clamp[i] = max(float(bound), 0.0)
                n += 1
        return n

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _stage_table(self, scaled):
        """fill the segment table and the group rows of this step (the ONE place), queue their copy through the ring,
        return the device table: the segment rows, the group rows behind them (``_groups_ptr``).  ``scaled``: slot 5
        carries the host's update count (wsis_adamw_step_scaled forms the bias corrections from it and the skip
        counters), else the two corrections as fp32, from the segment's own group's lr and betas."""
        tab = self._table
        grads = [p.grad for p in self.params]
        for i, g in enumerate(grads):                 # slow path only for a gradient the kernel cannot read as is
            if g is not None and (g.dtype != torch.float32 or not g.is_contiguous()):
                grads[i] = self.params[i].grad = g.contiguous().float()
        g_ptr = np.fromiter((0 if g is None else g.data_ptr() for g in grads), dtype=np.int64, count=len(grads))
        tab[:, 0] = np.fromiter((p.data_ptr() for p in self.params), dtype=np.int64, count=len(grads))
        tab[:, 1] = g_ptr
        live = g_ptr != 0
        tab[:, 4] = np.where(live, self._numel, 0)
        self.steps += live
        rows = group_rows(self.param_groups)
        if scaled:
            tab[:, 5] = self.steps
        else:
            t = np.maximum(self.steps, 1).astype(np.float64)
            lr, beta1, beta2 = rows[self._group_of, :3].T
            corr = np.stack([lr / (1.0 - beta1 ** t), 1.0 / np.sqrt(1.0 - beta2 ** t)], 1)
            tab[:, 5] = np.ascontiguousarray(corr.astype(np.float32)).view(np.int64).reshape(-1)
        k = self._slot
        self._slot = (k + 1) % _RING
        if self._done[k] is not None:
            self._done[k].synchronize()               # the copy issued _RING steps ago has long finished
        host = self._host[k].numpy()
        host[:tab.size] = tab.reshape(-1)
        host[tab.size:] = rows.reshape(-1).view(np.int64)
        self._dev[k].copy_(self._host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._done[k] = ev
        return self._dev[k]

    def _groups_ptr(self, dev_tab):
        return dev_tab.data_ptr() + 8 * self._table.size

    def _step_scaled(self, grad_scale, found_inf, check):
        """the step through wsis_adamw_step_scaled (several groups: wsis_adamw_step_scaled_groups); ``check``:
        wsis_grad_nonfinite first, over the same table slot"""
        for t in (grad_scale, found_inf):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                raise ValueError("grad_scale / found_inf: one-element fp32 tensors on the device")
        if self._skipped is None:
            self._skipped = torch.zeros(len(self.params), dtype=torch.int32, device=self.params[0].device)
        lib, dev_tab, st = _n.hip(), self._stage_table(True), _n.stream_ptr()
        if check:
            _n.check(lib.wsis_grad_nonfinite(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks, _n.ptr(found_inf), st),
                     "grad_nonfinite")
        if len(self.param_groups) == 1:
            _n.check(lib.wsis_adamw_step_scaled(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks, self.lr, self.betas[0],
                                                self.betas[1], self.eps, self.weight_decay, _n.ptr(grad_scale),
                                                _n.ptr(found_inf), _n.ptr(self._skipped), st), "adamw_step_scaled")
        else:
            _n.check(lib.wsis_adamw_step_scaled_groups(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks,
                                                       self._groups_ptr(dev_tab), len(self.param_groups),
                                                       _n.ptr(grad_scale), _n.ptr(found_inf), _n.ptr(self._skipped), st),
                     "adamw_step_scaled_groups")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if self._skipped is not None or grad_scale is not None or found_inf is not None:
            # once a step may have been skipped on the device, only the device knows the update counts
            self._step_scaled(grad_scale, found_inf, False)
            return loss
        dev_tab = self._stage_table(False)
        if len(self.param_groups) == 1:
            _n.check(_n.hip().wsis_adamw_step(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks, self.lr,
                                              self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                              _n.stream_ptr()), "adamw_step")
        else:
            _n.check(_n.hip().wsis_adamw_step_groups(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks,
                                                     self._groups_ptr(dev_tab), len(self.param_groups),
                                                     _n.stream_ptr()), "adamw_step_groups")
        return loss

    # state in the layout of torch.optim.AdamW.state_dict() (checkpoint interchange)
    def state_dict(self):
        state, off = {}, 0
        steps = self.steps          # updates that took effect: the one read-back of loss scaling, at checkpoint time
        if self._skipped is not None:
            steps = steps - self._skipped.cpu().numpy()
        for i, p in enumerate(self.params):
            n = p.numel()
            if steps[i] == 0:
                off += (n + 3) // 4 * 4
                continue                                  # torch creates the state at the first update
            state[i] = {"step": torch.tensor(float(steps[i])),
                        "exp_avg": self.exp_avg[off:off + n].view_as(p).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + n].view_as(p).clone()}
            off += (n + 3) // 4 * 4
        groups = []
        for g, idx in zip(self.param_groups, group_param_indices([len(g["params"]) for g in self.param_groups])):
            group = {k: v for k, v in g.items() if k != "params"}                  # incl. a scheduler's initial_lr
            group["params"] = idx
            groups.append(group)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for g, mine in zip(sd["param_groups"], self.param_groups):
            if len(g["params"]) != len(mine["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            for k in _UNSUPPORTED:
                if g.get(k):
                    raise ValueError(f"FlatAdamW: {k} is not supported")
        off = 0
        if self._skipped is not None:
            self._skipped.zero_()                         # the checkpoint's counts are the effective ones
        for i, p in enumerate(self.params):
            n = p.numel()
            st = sd["state"].get(i)
            if st is not None:
                self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                self.steps[i] = int(st["step"])
            else:       # absent from the checkpoint = never updated there: no stale moments survive a resume
                self.exp_avg[off:off + n].zero_()
                self.exp_avg_sq[off:off + n].zero_()
                self.steps[i] = 0
            off += (n + 3) // 4 * 4
        for g, mine in zip(sd["param_groups"], self.param_groups):
            for k, v in g.items():
                if k != "params":
                    mine[k] = tuple(v) if k == "betas" else v


class LossScaler(object):
    """Dynamic loss scaling for fp16 training: the subset of ``torch.amp.GradScaler`` the training loop uses, with the
    scale, the growth tracker and the overflow flag in one small device block and no read-back in a step::

        scaler.scale(loss).backward()      # one multiply by the device scale
        scaler.step(optimizer)             # wsis_grad_nonfinite + wsis_adamw_step_scaled over one table slot
        scaler.update()                    # wsis_loss_scale_update (one thread), clears the flag

    An overflow step writes no parameter, moment or gradient byte and halves the scale; ``growth_interval`` clean steps
    in a row double it (never to inf).  Several ranks: ``step`` runs after the gradient all-reduce, in which inf and NaN
    survive the sum, so every rank sees the same flag and takes the same decision without another collective."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True,
                 device=None):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _n.WsisError("LossScaler runs on the MI355X only (there is no CPU fallback)")
        if growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or int(growth_interval) < 1:
            raise ValueError("LossScaler: growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval, self.enabled = int(growth_interval), bool(enabled)
        self._block = torch.zeros(4, dtype=torch.float32, device=dev)       # scale, found_inf, tracker (int32), unused
        self._block[0] = float(init_scale)
        self._scale, self._found_inf = self._block[0:1], self._block[1:2]
        self._tracker = self._block[2:3].view(torch.int32)
        self._stepped = False

    def scale(self, loss):
        return loss * self._block[0] if self.enabled else loss

    def step(self, optimizer):
        if not isinstance(optimizer, FlatAdamW):
            raise TypeError("LossScaler.step drives wsis_optim.FlatAdamW only (torch.amp.GradScaler takes any optimizer)")
        if not self.enabled:
            return optimizer.step()
        if self._stepped:
            raise RuntimeError("step() has already been called since the last update()")
        with torch.no_grad():
            optimizer._step_scaled(self._scale, self._found_inf, True)
        self._stepped = True

    def update(self):
        if not self.enabled:
            return
        _n.check(_n.hip().wsis_loss_scale_update(_n.ptr(self._scale), _n.ptr(self._tracker), _n.ptr(self._found_inf),
                                                 self.growth_factor, self.backoff_factor, self.growth_interval,
                                                 _n.stream_ptr()), "loss_scale_update")
        self._stepped = False

    def get_scale(self):
        """the current scale -- a SYNCHRONISING read of the device (for logs, not for the step)"""
        return float(self._block[0]) if self.enabled else 1.0

    def state_dict(self):
        """the layout of ``torch.amp.GradScaler.state_dict()`` (its ``_growth_tracker`` is ``growth_tracker`` here; a
        checkpoint of either loads); reads the device"""
        if not self.enabled:
            return {}
        return {"scale": float(self._block[0]), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "growth_tracker": int(self._tracker[0])}

    def load_state_dict(self, sd):
        if not self.enabled:
            return
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self._block[0] = float(sd["scale"])
        self._tracker[0] = int(sd["growth_tracker"] if "growth_tracker" in sd else sd["_growth_tracker"])
        self._found_inf.zero_()
        self._stepped = False
