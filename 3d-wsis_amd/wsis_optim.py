"""AdamW step of the training iteration (``train_scannetv2.py:251``, optimizer of
``config/ScanNet_v2_3D_WSIS.yaml:58-61``) as ONE launch of ``wsis_adamw_step`` over all parameters.

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


class FlatAdamW(torch.optim.Optimizer):
    """A ``torch.optim.Optimizer`` (one parameter group): ``param_groups[0]`` is live -- the step reads ``lr``,
    ``betas``, ``eps`` and ``weight_decay`` from it, so the reference's ``PolyLR`` (an ``_LRScheduler``, stepped per
    epoch, ``utils/lr_scheduler.py``) and its ``save_checkpoint`` isinstance check work on it unchanged.

    Loss scaling: the step honours torch's protocol attributes ``grad_scale`` and ``found_inf`` (fp32 one-element device
    tensors; absent or None: scale 1 / never skipped), so ``torch.amp.GradScaler.step`` hands both over without reading
    ``found_inf`` back.  A step the device skips writes nothing and counts itself per parameter on the device
    (``_skipped``); ``steps`` keeps counting calls with a gradient.  A parameter without a gradient clamp keeps the SCALED
    values in ``.grad`` after a scaled step (the step does not write its gradient back); a clamped one holds the clamped
    unscaled values."""
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError("FlatAdamW takes ONE parameter group (one set of hyper-parameters per launch)")
            params = list(params[0]["params"])
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no parameters to optimise")
        super().__init__(params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                      weight_decay=float(weight_decay)))
        self.params = self.param_groups[0]["params"]
        dev = self.params[0].device
        if dev.type != "cuda":
            raise _n.WsisError("FlatAdamW runs on the MI355X only (there is no CPU fallback)")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("FlatAdamW expects contiguous fp32 parameters on one device")
        lib = _n.hip()
        self.steps = np.zeros(len(self.params), dtype=np.int64)    # updates per parameter (torch counts per parameter)
        numel = [p.numel() for p in self.params]
        # moments: one flat buffer each; slices start at multiples of 4 floats so the float4 path applies
        starts, total = [], 0
        for n in numel:
            starts.append(total)
            total += (n + 3) // 4 * 4
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        seg_bytes = lib.wsis_adamw_segment_bytes()
        assert seg_bytes == 56
        chunk = lib.wsis_adamw_chunk()
        n = len(self.params)
        self._table = np.zeros((n, 7), dtype=np.int64)            # p, g, m, v, numel, (step_size, inv_sqrt_bc2), (g_clamp, 0) as 2 x fp32
        self._table[:, 0] = [p.data_ptr() for p in self.params]
        self._table[:, 2] = [self.exp_avg.data_ptr() + 4 * s for s in starts]
        self._table[:, 3] = [self.exp_avg_sq.data_ptr() + 4 * s for s in starts]
        self._numel = np.asarray(numel, dtype=np.int64)
        blocks = np.concatenate([np.stack([np.full((k + chunk - 1) // chunk, i, dtype=np.int32),
                                           np.arange((k + chunk - 1) // chunk, dtype=np.int32)], 1)
                                 for i, k in enumerate(numel)])
        self._blocks = torch.from_numpy(np.ascontiguousarray(blocks)).to(dev)
        self._n_blocks = int(blocks.shape[0])
        self._host = [torch.empty((n, 7), dtype=torch.int64).pin_memory() for _ in range(_RING)]
        self._dev = [torch.empty((n, 7), dtype=torch.int64, device=dev) for _ in range(_RING)]
        self._done = [None] * _RING
        self._slot = 0
        self._skipped = None        # int32 [n]: steps the device skipped, per parameter; made by the first scaled step

    # hyper-parameters live in param_groups[0] (schedulers write there); the attributes are views of it
    lr = property(lambda self: float(self.param_groups[0]["lr"]),
                  lambda self, v: self.param_groups[0].__setitem__("lr", float(v)))
    betas = property(lambda self: tuple(float(b) for b in self.param_groups[0]["betas"]))
    eps = property(lambda self: float(self.param_groups[0]["eps"]))
    weight_decay = property(lambda self: float(self.param_groups[0]["weight_decay"]))

    def set_grad_clamp(self, params, bound):
        """gradients of ``params`` are clamped to [-bound, bound] inside the step's ONE launch (and written back, like the
        reference's ``p.grad.data.clamp_(-1, 1)`` over the ECC parameters, train_scannetv2.py:247-249); bound <= 0: off"""
        ids = {id(p) for p in params}
        pair = np.array([max(float(bound), 0.0), 0.0], dtype=np.float32).view(np.int64)[0]
        n = 0
        for i, p in enumerate(self.params):
            if id(p) in ids:
                self._table[i, 6] = pair
                n += 1
        return n

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _stage_table(self, scaled):
        """fill the segment table of this step (the ONE place), queue its copy through the ring, return the device
        table.  ``scaled``: slot 5 carries the host's update count (wsis_adamw_step_scaled forms the bias corrections
        from it and the skip counters), else the two corrections as fp32."""
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
        if scaled:
            tab[:, 5] = self.steps
        else:
            t = np.maximum(self.steps, 1).astype(np.float64)
            corr = np.stack([self.lr / (1.0 - self.betas[0] ** t), 1.0 / np.sqrt(1.0 - self.betas[1] ** t)], 1)
            tab[:, 5] = np.ascontiguousarray(corr.astype(np.float32)).view(np.int64).reshape(-1)
        k = self._slot
        self._slot = (k + 1) % _RING
        if self._done[k] is not None:
            self._done[k].synchronize()               # the copy issued _RING steps ago has long finished
        self._host[k].numpy()[:] = tab
        self._dev[k].copy_(self._host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._done[k] = ev
        return self._dev[k]

    def _step_scaled(self, grad_scale, found_inf, check):
        """the step through wsis_adamw_step_scaled; ``check``: wsis_grad_nonfinite first, over the same table slot"""
        for t in (grad_scale, found_inf):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                raise ValueError("grad_scale / found_inf: one-element fp32 tensors on the device")
        if self._skipped is None:
            self._skipped = torch.zeros(len(self.params), dtype=torch.int32, device=self.params[0].device)
        lib, dev_tab, st = _n.hip(), self._stage_table(True), _n.stream_ptr()
        if check:
            _n.check(lib.wsis_grad_nonfinite(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks, _n.ptr(found_inf), st),
                     "grad_nonfinite")
        _n.check(lib.wsis_adamw_step_scaled(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks, self.lr, self.betas[0],
                                            self.betas[1], self.eps, self.weight_decay, _n.ptr(grad_scale),
                                            _n.ptr(found_inf), _n.ptr(self._skipped), st), "adamw_step_scaled")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdamW takes ONE parameter group")
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if self._skipped is not None or grad_scale is not None or found_inf is not None:
            # once a step may have been skipped on the device, only the device knows the update counts
            self._step_scaled(grad_scale, found_inf, False)
            return loss
        dev_tab = self._stage_table(False)
        _n.check(_n.hip().wsis_adamw_step(_n.ptr(dev_tab), _n.ptr(self._blocks), self._n_blocks, self.lr,
                                          self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                          _n.stream_ptr()), "adamw_step")
        return loss

    # state in the layout of torch.optim.AdamW.state_dict()["state"] (checkpoint interchange)
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
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}   # incl. a scheduler's initial_lr
        group["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
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
        g = sd["param_groups"][0]
        for k, v in g.items():
            if k != "params":
                self.param_groups[0][k] = tuple(v) if k == "betas" else v


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
        if len(optimizer.param_groups) != 1:
            raise ValueError("FlatAdamW takes ONE parameter group")
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
