"""Native execution of the sparse UNet (input_conv -> UBlock -> output_layer) through the op-list executor.

The module tree of ``Network`` (same parameters, same state-dict) is walked ONCE per (model, mode) to record the
forward pass and -- from the closures the forward walk leaves behind, a hand-written tape for the four op kinds of
the UNet -- the backward pass as SYMBOLIC ``wsis_op`` templates (include/wsis_hip.h: device pointers + sizes): row
counts are level indices, activations are arena allocation ids, gather tables are slots.  Per step the templates are
instantiated with a handful of vectorised numpy assignments (row counts of the scene's pyramid, table pointers,
arena bases) and ONE C call per pass (``wsis_run_ops``) issues every kernel.
Numerically this is the same kernel sequence the per-module path (spconv.SubMConv3d / BatchNorm / ...) launches,
so both paths agree bit for bit; what disappears is ~450 Python-dispatched autograd nodes per step
(sparse_unet3d.py:103-350 walked by torch in the reference).

The walk (``_residual_block`` / ``_ublock``) exists once and emits through ``_TrainEmitter`` (fp32 ops, backward closures,
everything that lives for one recording) or ``_LpEmitter(train)`` (the 16-bit ops: the evaluation forward, or forward and
backward closures of the training pass); ops under construction are ``_Op`` records, their pointer slots go by the
``S_*`` names.  ``_record`` and ``_record_lp`` end in ``_program_of``, which sets what every compiled program carries.
tests/test_unet_program_host.py pins the recordings of all three passes byte for byte on the CPU.

Activations live in one arena per pass (bump allocation, nothing is freed before the backward: 288 GB of HBM make
rematerialisation pointless at these sizes), parameter gradients densely in one flat buffer whose views become
``p.grad`` (and which ``parallel.GradSync`` all-reduces in place).

``Network.forward`` takes the fp32 pass for fp32 features outside autocast.  For 16-bit features or under
``torch.autocast`` (spconv.ops.compute_dtype) it walks the modules -- except for an evaluation-mode forward without
gradients with WSIS_NATIVE_LP=1 (``lp_pass_wanted``), which runs the 16-bit forward program of
``UNetProgram.compiled_lp`` (``run_unet_lp``), and a training-mode pass with
WSIS_NATIVE_LP_TRAIN=1 (``lp_train_pass_wanted``), which runs the 16-bit forward + backward programs of
``UNetProgram.compiled_lp_train`` (``UNetLpTrainFunction``; with a SyncBatchNorm group only
under WSIS_NATIVE_LP_SYNC=1, then issued in parts around every layer's exchange like the fp32 pass).  Both switches go through one rule
(``_lp_wanted``), and all three passes through one driver: ``_issue_forward`` / ``_issue_backward`` lay out the arenas,
instantiate and run, ``_store_grads`` hands the gradients to the parameters.
"""
import collections
import os
import types

import numpy as np
import torch
from torch import nn
from torch.autograd import Function

import wsis_native as _n
import wsis_ops
from spconv import ops as sp_ops

OP_CONV, OP_BN_RELU, OP_CAT, OP_SPLIT, OP_ADD, OP_CONV_BWD, OP_BN_RELU_BWD = 1, 2, 3, 4, 5, 6, 7
F_RELU, F_TRAINING, F_UPDATE, F_FLIP, F_STATS, F_BN_IN, F_STAT_FIN = 1, 2, 4, 8, 16, 32, 64
N_IN, N_OUT = 12, 8
OP_CAST_LP = 8
F_LP, F_OUT_F32 = 128, 256      # 16-bit op (dtype code in wsis_op.reserved); fp32 output of a 16-bit BatchNorm op
F_LP_TRAIN = 512                # with F_LP: op of a 16-bit TRAINING pass (training BatchNorm and the backward forms need it)
_LPT = F_LP | F_LP_TRAIN

OP_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("M_in", "<i8"), ("M_out", "<i8"), ("K", "<i4"),
                     ("Cin", "<i4"), ("Cout", "<i4"), ("reserved", "<i4"), ("eps", "<f4"), ("momentum", "<f4"),
                     ("momentum2", "<f4"), ("reserved2", "<f4"), ("inp", "<u8", (N_IN,)), ("out", "<u8", (N_OUT,))])
assert OP_DTYPE.itemsize == 216          # sizeof(wsis_op)

# symbolic pointer = tag | id; plain device pointers (parameters, BN buffers) carry no tag
_FWD = 1 << 62      # allocation id in the FORWARD arena
_BWD = 1 << 61      # allocation id in the BACKWARD arena
_PAR = 1 << 60      # allocation id in the flat PARAMETER-GRADIENT buffer
_TBL = 1 << 59      # gather-table slot: level*6 + {0 subm.nbr, 1 subm.order, 2 down.nbr, 3 down.order, 4 up.nbr, 5 up.order}
_EXT = 1 << 58      # external tensor: 0 = input features, 1 = gradient of the output
_TAGS = (_FWD, _BWD, _PAR, _TBL, _EXT)
_ID_MASK = (1 << 32) - 1       # allocation id / slot
_OFF_SHIFT = 32                # bits 32..57: offset into the allocation, in floats (a channel range of a statistics vector)
_OFF_MASK = (1 << 26) - 1


def _at(handle, floats):
    """symbolic pointer ``floats`` floats into an allocation; a plain device pointer is simply advanced"""
    if floats == 0 or handle == 0:
        return handle
    if any(handle & t for t in _TAGS):
        return handle + (int(floats) << _OFF_SHIFT)
    return handle + 4 * int(floats)


def _fuse_fin_enabled():
    """BatchNorm statistics finished inside the producing convolution's launch (last-arrival tickets,
    WSIS_FUSE_BN_FIN=1; default off: finish + apply in one launch behind the convolution).  Measured on the C2 scene:
    40 launches fewer, but every workgroup of the convolution then waits for its partial stores and a ticket before it
    retires -- the level-0 layers run 59 -> 71 us, which is what the shorter apply pass (25 -> 10 us) gives back:
    10.56 / 10.77 against 10.52 / 10.70 ms per step in alternating runs."""
    on = os.environ.get("WSIS_FUSE_BN_FIN", "0") != "0"
    if on:
        _n.require_experimental("WSIS_FUSE_BN_FIN (statistics finished inside the convolution)")
    return on


def _fuse_apply_level():
    """pyramid level from which the BatchNorm(+ReLU) in front of a convolution is applied by that convolution as it reads
    its input (WSIS_FUSE_BN_APPLY=<level>; default off).  Measured on the C2 scene: the 64 VALU + 13 LDS instructions per
    (offset, chunk) step are not hidden under the MFMAs -- the fused layers run 12-20 % longer (level 0: +11.5 us per
    launch against a 10 us apply pass, level 3: +4 us against 3 us) and the own-rows weight gradient 30 % longer, so the
    apply pass stays a launch of its own; the fused form remains for memory-tight runs (no activation copy)."""
    v = os.environ.get("WSIS_FUSE_BN_APPLY", "")
    lvl = int(v) if v.lstrip("-").isdigit() else 99
    if lvl < 99:
        _n.require_experimental("WSIS_FUSE_BN_APPLY (BatchNorm applied by the consuming convolution)")
    return lvl


def _fuse_stats_enabled():
    """BatchNorm statistics from the producing convolution's epilogue (WSIS_FUSE_BN_STATS=0: separate pass over x,
    bit-identical to the per-module walk)"""
    return os.environ.get("WSIS_FUSE_BN_STATS", "1") != "0"


def _lvl(level):
    """symbolic row count of a pyramid level (negative code, resolved per scene)"""
    return -(level + 1)


# slots of wsis_op.in[] / .out[] per op kind: the table in the comment above ``wsis_op`` in include/wsis_hip.h, by name
class S_CONV(object):      # OP_CONV
    X, NBR, ORDER, W, BIAS, RESIDUAL = range(6)                      # in[]
    BN_IN = slice(6, 10)                                             # in[]: mean, var, gamma, beta (F_BN_IN)
    FIN0_RUNNING = slice(10, 12)                                     # in[]: running mean, var of finish target 0
    Y, PARTS = 0, 1                                                  # out[]: output, its BatchNorm partials (F_STATS)
    FIN0 = slice(2, 4)                                               # out[]: mean, var of finish target 0 (F_STAT_FIN)
    FIN1 = slice(4, 8)                                               # out[]: mean, var, running mean, running var of
    FIN1_MEAN = 4                                                    # finish target 1 (momentum2); NULL mean: unused


class S_CONV_BWD(object):      # OP_CONV_BWD
    X, W, DY, NBR_F, ORDER_F, NBR_B, ORDER_B = range(7)              # in[]
    BN_IN = slice(7, 11)                                             # in[]: mean, var, gamma, beta (F_BN_IN)
    DX, DW = 0, 1                                                    # out[]


class S_BN(object):      # OP_BN_RELU
    X, GAMMA, BETA, RMEAN, RVAR = range(5)                           # in[]
    PARTS0, PARTS1 = 5, 6                                            # in[]: partials of channels [0, K) and [K, Cin)
    Y, MEAN, VAR = range(3)                                          # out[]


class S_BN_BWD(object):      # OP_BN_RELU_BWD
    X, DY, MEAN, VAR, GAMMA, BETA, ADDEND = range(7)                 # in[]
    DIN_PARTS = 7                                                    # in[]: (sum dz, sum dz*xhat) partials of the dIn pass
    DX, DGAMMA, DBETA = range(3)                                     # out[]


class _Op(object):
    """a ``wsis_op`` being recorded: one attribute per field of the struct, ``inp`` / ``out`` as lists of N_IN / N_OUT
    handles (later ops patch earlier ones: statistics targets, epilogue reductions)"""
    __slots__ = ("kind", "flags", "M_in", "M_out", "K", "Cin", "Cout", "eps", "momentum", "momentum2", "inp", "out")

    def __init__(self, kind, flags=0, M_in=0, M_out=0, K=0, Cin=0, Cout=0, eps=0.0, momentum=0.0, inp=(), out=()):
        """``inp`` / ``out``: the leading slots in the order of the S_* classes"""
        self.kind, self.flags, self.M_in, self.M_out = kind, flags, M_in, M_out
        self.K, self.Cin, self.Cout = K, Cin, Cout
        self.eps, self.momentum, self.momentum2 = eps, momentum, 0.0
        self.inp = list(inp) + [0] * (N_IN - len(inp))
        self.out = list(out) + [0] * (N_OUT - len(out))


class _Recorder(object):
    """symbolic op list + allocation table of one arena"""

    def __init__(self, tag, align=256):
        self.tag, self.align = tag, align
        self.ops = []
        self.alloc_level, self.alloc_mult, self.alloc_slices = [], [], []

    def alloc(self, level, mult, per_slice=False):
        """``mult`` floats per row of pyramid level ``level`` (level < 0: ``mult`` floats in total); ``per_slice``:
        per 32-row slice of the level instead (BatchNorm partials of a convolution output)"""
        self.alloc_level.append(level)
        self.alloc_mult.append(int(mult))
        self.alloc_slices.append(bool(per_slice))
        return self.tag | (len(self.alloc_level) - 1)

    def op(self, *args, **kwargs):
        """appends an ``_Op`` and returns it"""
        self.ops.append(_Op(*args, **kwargs))
        return self.ops[-1]


class _Arena(object):
    """allocation table -> per-scene byte offsets"""

    def __init__(self, rec):
        self.level = np.asarray(rec.alloc_level, dtype=np.int64)
        self.mult = np.asarray(rec.alloc_mult, dtype=np.int64)
        self.slices = np.asarray(rec.alloc_slices, dtype=bool)
        self.align = rec.align

    def layout(self, Mvec):
        if len(self.level) == 0:
            return np.zeros(0, dtype=np.int64), 0
        rows = np.where(self.level >= 0, Mvec[np.maximum(self.level, 0)], 1)
        rows = np.where(self.slices, (rows + 31) // 32, rows)
        size = (rows * self.mult * 4 + self.align - 1) // self.align * self.align
        end = np.cumsum(size)
        return end - size, int(end[-1])


class _Template(object):
    """op records with every static field filled in; row counts and tagged pointers are patched per scene"""

    def __init__(self, rec):
        ops = rec.ops
        n = len(ops)
        self.arr = np.zeros(n, dtype=OP_DTYPE)
        for field in ("kind", "flags", "K", "Cin", "Cout", "eps", "momentum", "momentum2"):
            self.arr[field] = [getattr(o, field) for o in ops]
        ptr = np.array([o.inp + o.out for o in ops], dtype=np.uint64).reshape(n, N_IN + N_OUT)
        m_in, m_out = (np.array([getattr(o, f) for o in ops], dtype=np.int64) for f in ("M_in", "M_out"))
        self.m_in_lit, self.m_out_lit = np.maximum(m_in, 0), np.maximum(m_out, 0)
        self.m_in_lvl, self.m_out_lvl = np.maximum(-m_in - 1, 0), np.maximum(-m_out - 1, 0)
        self.m_in_sym, self.m_out_sym = m_in < 0, m_out < 0
        flat = ptr.reshape(-1)
        self.static = flat.copy()
        self.patch = {}
        for tag in _TAGS:
            pos = np.nonzero((flat & np.uint64(tag)) != 0)[0]
            off = ((flat[pos] >> np.uint64(_OFF_SHIFT)) & np.uint64(_OFF_MASK)) * np.uint64(4)      # bytes
            self.patch[tag] = (pos, (flat[pos] & np.uint64(_ID_MASK)).astype(np.int64), off)
            self.static[pos] = 0

    def instantiate(self, Mvec, luts):
        arr = self.arr.copy()
        arr["M_in"] = np.where(self.m_in_sym, Mvec[self.m_in_lvl], self.m_in_lit)
        arr["M_out"] = np.where(self.m_out_sym, Mvec[self.m_out_lvl], self.m_out_lit)
        flat = self.static.copy()
        for tag, (pos, idx, off) in self.patch.items():
            if len(pos):
                flat[pos] = luts[tag][idx] + off
        ptr = flat.reshape(-1, N_IN + N_OUT)
        arr["inp"] = ptr[:, :N_IN]
        arr["out"] = ptr[:, N_IN:]
        return arr


def _ptr(t):
    return 0 if t is None else t.data_ptr()


# gather tables of one conv as slots: forward (rows = outputs) and dIn (rows = inputs) + flip flag
_Table = collections.namedtuple("_Table", "nbr_f order_f nbr_b order_b flip", defaults=(0, 0, 0, 0, 0))


def _subm(l):
    return _Table(_TBL | (l * 6), _TBL | (l * 6 + 1), _TBL | (l * 6), _TBL | (l * 6 + 1), 1)


def _down(l):
    return _Table(_TBL | (l * 6 + 2), _TBL | (l * 6 + 3), _TBL | (l * 6 + 4), _TBL | (l * 6 + 5), 0)


def _up(l):
    return _Table(_TBL | (l * 6 + 4), _TBL | (l * 6 + 5), _TBL | (l * 6 + 2), _TBL | (l * 6 + 3), 0)


def _conv_dims(conv):
    assert conv.bias is None, "the UNet convolutions carry no bias (sparse_unet3d.py)"
    return int(np.prod(conv.kernel_size)), conv.in_channels, conv.out_channels


class _Emitter(object):
    """what the emitters share: the parameter-gradient handles of one recording (``prec``, ``grad``)"""

    def grad_handle(self, p):
        # parameter gradients live densely in their own flat buffer (one all-reduce for data parallelism)
        if id(p) not in self.grad:
            self.grad[id(p)] = self.prec.alloc(-1, p.numel())
        return self.grad[id(p)]


class _TrainEmitter(_Emitter):
    """the fp32 ops of a training or evaluation pass, with everything that lives for ONE recording: the three recorders,
    the gradient handles, the profiler's entries, the statistics sources and the BatchNorm layers applied by their
    consumer.  ``conv`` / ``bn_relu`` / ``cat`` return (out_handle, backward_closure): a hand-written tape, the closures
    emit into the backward recorder when ``UNetProgram`` calls them in reverse."""

    def __init__(self, synced):
        self.rec, self.recb, self.prec = _Recorder(_FWD), _Recorder(_BWD), _Recorder(_PAR, align=16)
        self.grad = {}
        self.acc_f, self.acc_b, self.count = [], [], []
        self.stats_src, self.fuse_stats = {}, _fuse_stats_enabled()
        # virt: handle of a BatchNorm applied by its consumer -> (x, C, F_BN_IN | F_RELU, eps, (mean, var, gamma, beta))
        self.virt, self.fuse_apply_lvl = {}, _fuse_apply_level()
        self.fuse_fin = _fuse_fin_enabled() and self.fuse_stats
        self.fuse_fin_lvl = int(os.environ.get("WSIS_FUSE_BN_FIN_LVL", "0"))      # (EXPERIMENTAL build: from this level on)
        if synced:      # every BatchNorm layer stays an op of its own: _run_synced runs it between parts
            self.fuse_fin, self.fuse_apply_lvl = False, 99

    def conv(self, x, conv, table, lvl_in, lvl_out, residual=0, stats=True):
        rec, recb = self.rec, self.recb
        K, Cin, Cout = _conv_dims(conv)
        W = conv.weight
        y = rec.alloc(lvl_out, Cout)
        t = table if table is not None else _Table()
        # BatchNorm statistics of the output from the convolution's own epilogue (training passes, layers on the
        # wave-autonomous kernel): per-slice (sum, sum of squares) partials next to the output
        part = 0
        if stats and self.fuse_stats and sp_ops._use_fwd2(K, Cin, Cout):
            part = rec.alloc(lvl_out, 2 * Cout, per_slice=True)
        # the input may be a BatchNorm(+ReLU) that is applied while this convolution reads it (see bn_relu)
        x, C_in, bn_flags, eps, bn_in = self.virt.get(x, (x, Cin, 0, 0.0, (0, 0, 0, 0)))
        assert C_in == Cin and (not bn_flags or sp_ops._use_fwd2(K, Cin, Cout))
        op = rec.op(OP_CONV, bn_flags | (F_STATS if part else 0), _lvl(lvl_in), _lvl(lvl_out), K, Cin, Cout, eps=eps,
                    inp=(x, t.nbr_f, t.order_f, W.data_ptr(), 0, residual), out=(y, part))
        op.inp[S_CONV.BN_IN] = bn_in
        if part:
            self.stats_src[y] = [(part, Cout, op)]
        self.acc_f.append(("spconv_fwd_kernel", t.nbr_f, lvl_out, Cin, Cout))

        def bwd(dy, need_dx=True):
            dx = recb.alloc(lvl_in, Cin) if need_dx else 0
            dW = self.grad_handle(W)
            bop = recb.op(OP_CONV_BWD, bn_flags | (F_FLIP if t.flip else 0), _lvl(lvl_in), _lvl(lvl_out), K, Cin, Cout, eps=eps,
                          inp=(x, W.data_ptr(), dy, t.nbr_f, t.order_f, t.nbr_b, t.order_b), out=(dx, dW))
            bop.inp[S_CONV_BWD.BN_IN] = bn_in
            if need_dx:
                self.acc_b.append(("spconv_fwd_kernel", t.nbr_b, lvl_in, Cout, Cin))
            self.acc_b.append(("spconv_dw_kernel", t.nbr_f, lvl_out, Cin, Cout))
            return dx
        return y, bwd

    def bn_relu(self, x, bn, lvl, relu=True, fuse=False):
        """BatchNorm1d(+ReLU).  ``fuse``: the only consumer is a convolution on the wave-autonomous kernel, which applies
        the BatchNorm while it reads its input (the returned handle is virtual: nothing is written).  Training
        statistics come from the producing convolutions' epilogue partials where they exist -- finished inside those
        launches (F_STAT_FIN) or by a finalize op -- otherwise from a pass over x."""
        rec, recb = self.rec, self.recb
        C = bn.num_features
        training = bn.training or not bn.track_running_stats
        update = bn.training and bn.track_running_stats
        flags = (F_RELU if relu else 0) | (F_TRAINING if training else 0) | (F_UPDATE if update else 0)
        if update and bn.num_batches_tracked is not None:
            assert bn.momentum is not None, "cumulative-average BatchNorm is not used by 3D-WSIS"
            self.count.append(bn)
        fuse = fuse and lvl >= self.fuse_apply_lvl and self.fuse_stats and C % 32 == 0
        momentum = bn.momentum if bn.momentum is not None else 0.1
        mean = rec.alloc(-1, C) if training else bn.running_mean.data_ptr()
        var = rec.alloc(-1, C) if training else bn.running_var.data_ptr()
        src = self.stats_src.get(x) if training else None
        have_parts = src is not None and sum(c for _, c, _ in src) == C and len(src) <= 2
        stats_done = False
        if (have_parts and self.fuse_fin and lvl >= self.fuse_fin_lvl
                and all(p.out[S_CONV.FIN1_MEAN] == 0 for _, _, p in src)):
            # every producer finishes its channel range of this BatchNorm's statistics inside its own launch
            c0 = 0
            running = (_ptr(bn.running_mean), _ptr(bn.running_var)) if update else (0, 0)
            for _, c, p in src:
                tgt = [_at(h, c0) for h in (mean, var) + running]
                if not (p.flags & F_STAT_FIN):
                    p.flags |= F_STAT_FIN
                    p.out[S_CONV.FIN0], p.inp[S_CONV.FIN0_RUNNING] = tgt[:2], tgt[2:]
                    p.momentum = momentum
                else:
                    p.out[S_CONV.FIN1] = tgt
                    p.momentum2 = momentum
                c0 += c
            stats_done = True
        y = rec.alloc(lvl, 0 if fuse else C)
        if fuse:
            self.virt[y] = (x, C, F_BN_IN | (F_RELU if relu else 0), bn.eps, (mean, var, _ptr(bn.weight), _ptr(bn.bias)))
        if training and not stats_done:
            K0, parts, sflags = 0, (0, 0), flags
            if have_parts:
                sflags |= F_STATS            # the producers' epilogues wrote the partials: no statistics pass over x
                K0 = src[0][1]
                parts = (src[0][0], src[1][0] if len(src) == 2 else 0)
            op = rec.op(OP_BN_RELU, sflags, _lvl(lvl), _lvl(lvl), K0, C, C, bn.eps, momentum,
                        inp=(x, _ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean), _ptr(bn.running_var)),
                        out=(0 if fuse else y, mean, var))
            op.inp[S_BN.PARTS0], op.inp[S_BN.PARTS1] = parts
            # algorithmic bytes of the op (bench.py's BatchNorm line): x read + y written; a statistics pass over x
            # (no epilogue partials) reads x once more
            self.acc_f.append(("bn_op", 0, lvl, C, (0 if fuse else 2) + (0 if have_parts else 1)))
        elif not fuse:
            # statistics known (finished by the producers, or evaluation mode): apply pass only
            rec.op(OP_BN_RELU, flags & ~(F_TRAINING | F_UPDATE), _lvl(lvl), _lvl(lvl), 0, C, C, bn.eps, momentum,
                   inp=(x, _ptr(bn.weight), _ptr(bn.bias), mean, var), out=(y,))
            self.acc_f.append(("bn_op", 0, lvl, C, 2))

        def bwd(dy, addend=0):
            # ``addend``: gradient arriving at x over a second path (residual skip / UNet skip connection), added
            # in the same pass instead of a separate accumulation kernel
            dx = recb.alloc(lvl, C)
            dg = self.grad_handle(bn.weight) if bn.weight is not None else recb.alloc(-1, C)
            db = self.grad_handle(bn.bias) if bn.bias is not None else recb.alloc(-1, C)
            recb.op(OP_BN_RELU_BWD, flags & ~F_STATS, _lvl(lvl), _lvl(lvl), 0, C, C, bn.eps, 0.0,      # (F_STATS: fuse_bn_bwd)
                    inp=(x, dy, mean, var, _ptr(bn.weight), _ptr(bn.bias), addend), out=(dx, dg, db))
            # x and dy read, dx written, the addend read where there is one (a separate reduction pass over x and dy,
            # taken when the producing dIn pass left no partials, is not counted: algorithmic = the fused form)
            self.acc_b.append(("bn_op", 0, lvl, C, 3 + (1 if addend else 0)))
            return dx
        return y, bwd

    def cat(self, a, b, lvl, C0):
        """[a | b] of C0 channels each; the closure splits the gradient: d -> (d_a, d_b)"""
        rec, recb = self.rec, self.recb
        cat = rec.alloc(lvl, 2 * C0)
        rec.op(OP_CAT, 0, _lvl(lvl), _lvl(lvl), 0, C0, C0, inp=(a, b), out=(cat,))
        if a in self.stats_src and b in self.stats_src:      # statistics of a concatenation = both halves'
            self.stats_src[cat] = self.stats_src[a] + self.stats_src[b]

        def bwd(d):
            d_a = recb.alloc(lvl, C0)
            d_b = recb.alloc(lvl, C0)
            recb.op(OP_SPLIT, 0, _lvl(lvl), _lvl(lvl), 0, C0, C0, inp=(d,), out=(d_a, d_b))
            return d_a, d_b
        return cat, bwd

    def fuse_bn_bwd(self):
        """dIn passes whose output is the dy of a BatchNorm backward a few ops later (training mode, layer on the
        wave-autonomous kernel) also write that op's (sum dz, sum dz*xhat) slice partials from their epilogue: both
        ops get F_STATS and the BatchNorm op the partial buffer (WSIS_FUSE_BN_BWD=0: separate pass)"""
        if os.environ.get("WSIS_FUSE_BN_BWD", "1") == "0" or not self.fuse_stats:
            return
        ops = self.recb.ops
        for i, r in enumerate(ops):
            dx = r.out[S_CONV_BWD.DX] if r.kind == OP_CONV_BWD else 0
            if not dx or not sp_ops._use_fwd2(r.K, r.Cout, r.Cin):      # the dIn product gathers dY: roles of the channels swap
                continue
            for b in ops[i + 1:i + 5]:
                if (b.kind == OP_BN_RELU_BWD and b.inp[S_BN_BWD.DY] == dx and (b.flags & F_TRAINING) and b.Cin == r.Cin
                        and b.M_in == r.M_in):
                    b.inp[S_BN_BWD.DIN_PARTS] = self.recb.alloc(-b.M_in - 1, 2 * r.Cin, per_slice=True)      # (_lvl undone)
                    b.flags |= F_STATS
                    r.flags |= F_STATS
                    break


class _LpEmitter(_Emitter):
    """the 16-bit ops: a 16-bit activation (or gradient) of C channels is C / 2 floats per row of the arena, every
    BatchNorm is an op of its own (no virtual handles, no epilogue partials, no fused forms).  ``train`` False: the
    evaluation-mode forward (F_LP ops), running statistics only, no backward: every closure is None.  ``train`` True: the
    training pass (F_LP | F_LP_TRAIN ops, forward and backward): a training-mode BatchNorm takes its batch statistics in
    fp32 from the 16-bit x, parameter gradients are fp32 in the same flat buffer as the fp32 pass's, ``conv`` /
    ``bn_relu`` / ``cat`` return (out_handle, backward_closure) as ``_TrainEmitter`` does.  ``f32_dx_of``: the handle
    whose gradient leaves the 16-bit domain (the rounded output of the fp32 input convolution): the BatchNorm backward
    that produces it stores fp32."""

    def __init__(self, train):
        self.train, self.lp = train, _LPT if train else F_LP
        self.rec, self.count, self.f32_dx_of = _Recorder(_FWD), [], 0
        if train:
            self.recb, self.prec, self.grad = _Recorder(_BWD), _Recorder(_PAR, align=16), {}

    def conv(self, x, conv, table, lvl_in, lvl_out, residual=0, stats=True):
        rec = self.rec
        K, Cin, Cout = _conv_dims(conv)
        W = conv.weight
        t = table if table is not None else _Table()
        y = rec.alloc(lvl_out, Cout // 2)
        # (the executor casts the fp32 weight to 16-bit B^T slices inside the call: the pass follows the optimizer;
        # a skip path is added in the epilogue before its one rounding -- the walk adds two rounded tensors)
        rec.op(OP_CONV, self.lp, _lvl(lvl_in), _lvl(lvl_out), K, Cin, Cout,
               inp=(x, t.nbr_f, t.order_f, W.data_ptr(), 0, residual), out=(y,))
        if not self.train:
            return y, None
        recb = self.recb

        def bwd(dy):
            # dIn rounded once from its fp32 accumulators; dW fp32 straight into the flat gradient buffer.  As in the fp32
            # pass the program does not depend on requires_grad (one recording serves every setting): a frozen weight's
            # product still runs and _GradArena hands out no view of its slot
            dx = recb.alloc(lvl_in, Cin // 2)
            recb.op(OP_CONV_BWD, self.lp | (F_FLIP if t.flip else 0), _lvl(lvl_in), _lvl(lvl_out), K, Cin, Cout,
                    inp=(x, W.data_ptr(), dy, t.nbr_f, t.order_f, t.nbr_b, t.order_b), out=(dx, self.grad_handle(W)))
            return dx
        return y, bwd

    def bn_relu(self, x, bn, lvl, relu=True, fuse=False, out=0, out_f32=False):
        """``out``: a tensor of the caller's instead of an allocation of the arena; ``out_f32``: y stored as fp32"""
        rec = self.rec
        C = bn.num_features
        # (the evaluation program applies the running statistics whatever the layer's mode)
        training = self.train and (bn.training or not bn.track_running_stats)
        update = self.train and bn.training and bn.track_running_stats
        flags = self.lp | (F_RELU if relu else 0) | (F_TRAINING if training else 0)
        if update and bn.num_batches_tracked is not None:
            assert bn.momentum is not None, "cumulative-average BatchNorm is not used by 3D-WSIS"
            self.count.append(bn)
        # Two differences between the passes that no kernel reads but the byte-identity test
        # (tests/test_unet_program_host.py) keeps: an op that applies running statistics records momentum 0.0 and
        # out=(y,) in the evaluation program, the layer's own momentum (0.1 here) in a training pass
        momentum = (bn.momentum if bn.momentum is not None else 0.1) if self.train else 0.0
        mean = rec.alloc(-1, C) if training else _ptr(bn.running_mean)
        var = rec.alloc(-1, C) if training else _ptr(bn.running_var)
        y = out or rec.alloc(lvl, C if out_f32 else C // 2)
        rec.op(OP_BN_RELU, flags | (F_UPDATE if update else 0) | (F_OUT_F32 if out_f32 else 0), _lvl(lvl), _lvl(lvl), 0, C, C,
               bn.eps, momentum,
               inp=(x, _ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean), _ptr(bn.running_var)),
               out=(y, mean, var) if training else (y,))
        if not self.train:
            return y, None
        recb = self.recb

        def bwd(dy, addend=0):
            # the skip gradient is added in fp32 before the ONE rounding of dx (the walk adds two rounded tensors)
            f32 = x == self.f32_dx_of
            dx = recb.alloc(lvl, C if f32 else C // 2)
            dg = self.grad_handle(bn.weight) if bn.weight is not None else recb.alloc(-1, C)
            db = self.grad_handle(bn.bias) if bn.bias is not None else recb.alloc(-1, C)
            recb.op(OP_BN_RELU_BWD, flags | (F_OUT_F32 if f32 else 0), _lvl(lvl), _lvl(lvl), 0, C, C, bn.eps, 0.0,
                    inp=(x, dy, mean, var, _ptr(bn.weight), _ptr(bn.bias), addend), out=(dx, dg, db))
            return dx
        return y, bwd

    def cat(self, a, b, lvl, C0):
        cat = self.rec.alloc(lvl, C0)                  # 2 * C0 16-bit channels
        self.rec.op(OP_CAT, self.lp, _lvl(lvl), _lvl(lvl), 0, C0, C0, inp=(a, b), out=(cat,))
        if not self.train:
            return cat, None
        recb = self.recb

        def bwd(d):
            d_a = recb.alloc(lvl, C0 // 2)
            d_b = recb.alloc(lvl, C0 // 2)
            recb.op(OP_SPLIT, self.lp, _lvl(lvl), _lvl(lvl), 0, C0, C0, inp=(d,), out=(d_a, d_b))
            return d_a, d_b
        return cat, bwd


# ---- the one walk of the module tree: ``em`` is an emitter, every step returns (out_handle, backward_closure); what the
# closures do -- and whether anybody calls them -- is the emitter's business (the 16-bit program has no backward)
def _residual_block(em, x, blk, lvl):
    seq = blk.conv_branch
    bn1, conv1, bn2, conv2 = seq[0], seq[2], seq[3], seq[5]
    table = _subm(lvl)
    a1, b_bn1 = em.bn_relu(x, bn1, lvl, fuse=True)
    z1, b_c1 = em.conv(a1, conv1, table, lvl, lvl)
    a2, b_bn2 = em.bn_relu(z1, bn2, lvl, fuse=True)
    first = blk.i_branch[0]
    if isinstance(first, nn.Identity):
        res, b_i = x, None
    else:
        res, b_i = em.conv(x, first, None, lvl, lvl, stats=False)   # 1x1 projection of the skip path
    out, b_c2 = em.conv(a2, conv2, table, lvl, lvl, residual=res)

    def bwd(d_out):
        d_a1 = b_c1(b_bn2(b_c2(d_out)))
        d_skip = d_out if b_i is None else b_i(d_out)
        return b_bn1(d_a1, addend=d_skip)
    return out, bwd


def _blocks(em, x, blocks, lvl):
    bwds = []
    for blk in blocks:
        x, b = _residual_block(em, x, blk, lvl)
        bwds.append(b)

    def bwd(d):
        for b in reversed(bwds):
            d = b(d)
        return d
    return x, bwd


def _ublock(em, x, ub, lvl):
    x, b_head = _blocks(em, x, ub.blocks, lvl)
    if len(ub.nPlanes) == 1:
        return x, b_head
    a, b_bn = em.bn_relu(x, ub.conv[0], lvl, fuse=True)
    d, b_down = em.conv(a, ub.conv[2], _down(lvl), lvl, lvl + 1)
    u, b_u = _ublock(em, d, ub.u, lvl + 1)
    a2, b_bn2 = em.bn_relu(u, ub.deconv[0], lvl + 1, fuse=True)
    up, b_up = em.conv(a2, ub.deconv[2], _up(lvl), lvl + 1, lvl)
    cat, b_cat = em.cat(x, up, lvl, ub.nPlanes[0])
    y, b_tail = _blocks(em, cat, ub.blocks_tail, lvl)

    def bwd(d_y):
        d_id, d_up = b_cat(b_tail(d_y))
        d_a = b_down(b_u(b_bn2(b_up(d_up))))
        return b_head(b_bn(d_a, addend=d_id))
    return y, bwd


class UNetProgram(object):
    """records forward and backward of input_conv + unet + output_layer of a ``Network``"""

    def __init__(self, net):
        self.net = net
        self.params = [p for m in (net.input_conv, net.unet, net.output_layer) for p in m.parameters()]
        self.bns = [m for mod in (net.unet, net.output_layer) for m in mod.modules() if isinstance(m, nn.BatchNorm1d)]
        self.flat_grad, self.flat_params = None, []
        self.flat_tail = None        # spare floats behind the gradients (parallel.GradSync packs the other
        self.tail_floats = 0         # parameters' gradients there: ONE collective per step)
        self.overlap = None          # wsis_parallel.GradSync: early all-reduce of the finished first part (see backward)
        self._garena = None          # _GradArena of the last backward program
        # True (default): ``.grad`` of the UNet's parameters are views of ONE buffer that the next backward pass
        # overwrites once the gradients were cleared -- a tensor the caller kept from the previous step changes under
        # it.  False (or WSIS_PERSISTENT_GRADS=0): every backward pass writes a buffer of its own (the aliasing is
        # gone; a 44 MB allocation + the cached views rebuilt per step, data-parallel exchange still in place).
        self.persistent_grads = os.environ.get("WSIS_PERSISTENT_GRADS", "1") != "0"
        self.bn_sync = None          # _BnSync while the model's BatchNorm layers share their statistics across ranks
        self._cache = {}             # compiled programs by mode key
        self.Mvec = self.table_lut = self.table_tensors = self.keep = None      # the scene's pyramid (bind)

    # ---- compile (once per mode) / bind (per scene) ------------------------------------------------------------
    def _cached(self, key, record):
        c = self._cache.get(key)
        if c is None:
            if len(self._cache) > 8:
                self._cache.clear()
            c = self._cache[key] = record()
        return c

    def compiled_lp(self, dtype, out_f32):
        """the 16-bit evaluation-mode forward program of ``dtype`` (bf16 / fp16); ``out_f32``: the output layer's
        BatchNorm+ReLU stores fp32.  The output is external slot 1 (a tensor of the caller's): the arena of the pass is
        free once the call has been issued."""
        # (dtypes in the key too: a parameter converted to 16 bits may reuse a freed fp32 address)
        key = ("lp", dtype, bool(out_f32), tuple((p.data_ptr(), p.dtype) for p in self.params),
               tuple((_ptr(bn.running_mean), _ptr(bn.running_var), bn.running_var.dtype if bn.running_var is not None
                      else None) for bn in self.bns))
        return self._cached(key, lambda: self._record_lp(dtype, out_f32, False, False))

    def compiled_lp_train(self, dtype, out_f32, need_dx):
        """the 16-bit training programs (forward + backward) of ``dtype``; ``out_f32``: the output layer's
        BatchNorm+ReLU stores fp32; ``need_dx``: the input features take a gradient"""
        key = ("lp_train", dtype, bool(out_f32), bool(need_dx), tuple(bn.training for bn in self.bns),
               tuple((p.data_ptr(), p.dtype) for p in self.params),
               tuple((_ptr(bn.running_mean), _ptr(bn.running_var)) for bn in self.bns))
        return self._cached(key, lambda: self._record_lp(dtype, out_f32, True, need_dx))

    def _record_lp(self, dtype, out_f32, train, need_dx):
        """the 16-bit program(s): the forward alone (``train`` False) or forward + backward"""
        net = self.net
        if not lp_params_fp32(net, net.input_conv[0].weight.device):
            raise ValueError("the 16-bit native pass reads the model's parameters and running statistics as contiguous "
                             "fp32 tensors (lp_params_fp32); a model with 16-bit parameters walks the modules")
        em = _LpEmitter(train)
        rec = em.rec
        # boundary: the 6 -> 32 input convolution lies outside the 16-bit domain: the fp32 op on the rounded-and-widened
        # features (external slot 0), its output rounded once (what the module walk's fallback does,
        # spconv.ops._forward_lp); the output layer writes the caller's tensor (external slot 1)
        conv0 = net.input_conv[0]
        K0, Cin0, C0 = _conv_dims(conv0)
        t0 = _subm(0)
        W0 = conv0.weight.data_ptr()
        y32 = rec.alloc(0, C0)
        rec.op(OP_CONV, 0, _lvl(0), _lvl(0), K0, Cin0, C0, inp=(_EXT | 0, t0.nbr_f, t0.order_f, W0, 0, 0), out=(y32,))
        y = em.f32_dx_of = rec.alloc(0, C0 // 2)
        rec.op(OP_CAST_LP, em.lp, _lvl(0), _lvl(0), 0, C0, C0, inp=(y32,), out=(y,))
        u, b_u = _ublock(em, y, net.unet, 0)
        _, b_out = em.bn_relu(u, net.output_layer[0], 0, out=_EXT | 1, out_f32=out_f32)
        dx = 0
        if train:
            # backward: external slot 1 is the incoming gradient in ``dtype``; the rounding is straight-through, so the
            # fp32 dx of the first block's BatchNorm is the dY of the fp32 input convolution
            recb = em.recb
            d32 = b_u(b_out(_EXT | 1))
            assert recb.ops[-1].kind == OP_BN_RELU_BWD and recb.ops[-1].flags & F_OUT_F32 and recb.ops[-1].out[S_BN_BWD.DX] == d32
            dx = recb.alloc(0, Cin0) if need_dx else 0
            recb.op(OP_CONV_BWD, F_FLIP, _lvl(0), _lvl(0), K0, Cin0, C0,
                    inp=(_EXT | 0, W0, d32, t0.nbr_f, t0.order_f, t0.nbr_b, t0.order_b), out=(dx, em.grad_handle(conv0.weight)))
        c = self._program_of(em, -1, dx if need_dx else -1)
        for t in (c.fwd, c.bwd):
            if t is not None:      # the dtype code of every 16-bit op
                t.arr["reserved"] = np.where((t.arr["flags"] & F_LP) != 0, sp_ops._LP_DTYPES[dtype], 0)
        return c

    def _program_of(self, em, out, dx):
        """what every compiled program of one (model, mode) carries: the templates, the three arenas, the ids of the
        output and of the input's gradient (handles; -1: none), the parameter-gradient ids, the BatchNorm layers whose
        batch counter a pass advances, the channel counts.  A program without a backward has ``bwd = None``, no backward
        or parameter arena and no gradient ids."""
        c = types.SimpleNamespace()
        c.fwd, c.fwd_arena = _Template(em.rec), _Arena(em.rec)
        c.bwd = c.bwd_arena = c.par_arena = None
        c.grad_ids = []
        if getattr(em, "recb", None) is not None:
            c.bwd, c.bwd_arena, c.par_arena = _Template(em.recb), _Arena(em.recb), _Arena(em.prec)
            c.grad_ids = [(em.grad[id(p)] & _ID_MASK) if id(p) in em.grad else -1 for p in self.params]
        c.out_id, c.dx_id = (h & _ID_MASK if h >= 0 else -1 for h in (out, dx))
        c.count = em.count
        c.in_channels, c.out_channels = self.net.input_conv[0].in_channels, self.net.output_layer[0].num_features
        return c

    def _mode_key(self, need_dx):
        # bn_sync: the synced pass intercepts training-mode BatchNorm ops only -- the forms that finish the statistics
        # inside the producing convolution or apply them inside the consuming one leave no such op, so a program
        # compiled with them must never serve a synced pass (and the other way round)
        return (need_dx, self.bn_sync is not None, _fuse_stats_enabled(), _fuse_fin_enabled(), _fuse_apply_level(),
                os.environ.get("WSIS_FUSE_BN_FIN_LVL", "0"), os.environ.get("WSIS_FUSE_BN_BWD", "1"),
                os.environ.get("WSIS_FWD2", "1"), tuple(bn.training for bn in self.bns), tuple(p.data_ptr() for p in self.params),
                tuple(bn.running_mean.data_ptr() if bn.running_mean is not None else 0 for bn in self.bns))

    def compiled(self, need_dx):
        return self._cached(self._mode_key(need_dx), lambda: self._record(need_dx))

    def _record(self, need_dx):
        net = self.net
        em = _TrainEmitter(synced=self.bn_sync is not None)
        y, b_in = em.conv(_EXT | 0, net.input_conv[0], _subm(0), 0, 0)
        y, b_u = _ublock(em, y, net.unet, 0)
        out, b_out = em.bn_relu(y, net.output_layer[0], 0)
        dx = b_in(b_u(b_out(_EXT | 1)), need_dx)
        em.fuse_bn_bwd()
        c = self._program_of(em, out, dx if need_dx else -1)
        c.acc_f, c.acc_b = em.acc_f, em.acc_b
        # milestone of the backward list: the op after which the first ~half of the flat parameter-gradient buffer is
        # final (gradients are allocated in the order the backward pass produces them)
        last = [max([(h & _ID_MASK) + 1 for h in o.out if h & _PAR] or [0]) for o in em.recb.ops]
        c.bwd_grads_done = np.maximum.accumulate(np.array(last, dtype=np.int64))
        return c

    def bind(self, tensor):
        """rulebooks of the pyramid of ``tensor`` (built if missing) -> row counts and the table-pointer LUT"""
        net = self.net
        sp_ops.prebuild_unet_rulebooks(tensor, net.blocks)
        L = net.blocks
        self.Mvec = np.zeros(L, dtype=np.int64)
        self.table_lut = np.zeros(L * 6, dtype=np.uint64)
        self.table_tensors = [None] * (L * 6)
        pyr = getattr(tensor.indice_dict, "pyramid", None)
        if pyr is not None and pyr.n_levels == L:
            # the pyramid came from one native call into one arena: row counts and table pointers straight from its
            # layout, no per-table tensor views (they are made only if the profiler asks for pair counts)
            lay, base = pyr.layout, np.uint64(pyr.base)
            self.Mvec[:] = lay[:, sp_ops.PYR_ROWS]
            fields = (sp_ops.PYR_SUBM_NBR_P, sp_ops.PYR_SUBM_ORDER, sp_ops.PYR_DOWN_NBR_P, sp_ops.PYR_DOWN_ORDER,
                      sp_ops.PYR_UP_NBR_P, sp_ops.PYR_UP_ORDER)
            off = lay[:, fields]                                   # [L, 6]
            self.table_lut[:] = np.where(off >= 0, off.astype(np.uint64) + base, np.uint64(0)).reshape(-1)
            self.table_tensors = _LazyTables(tensor.indice_dict, L)
            self.keep = [tensor.indice_dict]
            return
        for lvl in range(L):
            rb = tensor.indice_dict["subm%d" % (lvl + 1)]
            self.Mvec[lvl] = rb.in_indices.shape[0]
            ts = [rb.nbr_p, rb.order, None, None, None, None]
            if lvl + 1 < L:
                rd = tensor.indice_dict["spconv%d" % (lvl + 1)]
                ts[2:] = [rd.nbr_p, rd.order, rd.nbr_up_p, rd.order_up]
            for j, t in enumerate(ts):
                self.table_lut[lvl * 6 + j] = _ptr(t)
                self.table_tensors[lvl * 6 + j] = t
        self.keep = [tensor.indice_dict]     # the tables must outlive the backward pass

    def account(self, entries, Mvec, tensors):
        prof = sp_ops.PROFILER
        if prof is None:
            return
        for name, nbr, lvl, Cin, Cout in entries:
            if name == "bn_op":      # (Cin = channels, Cout = tensors of [rows, channels] the op reads + writes)
                M = int(Mvec[lvl])
                prof.end(name, None, M * Cin * Cout * 4, 0, (M, Cin, Cout, M))
                continue
            t = tensors[nbr & _ID_MASK] if nbr else None
            P = prof.pairs(t, int(Mvec[lvl]))
            prof.end(name, None, P * (Cin + Cout) * 4 + P * 8, 2 * P * Cin * Cout, (int(Mvec[lvl]), Cin, Cout, P))


class _LazyTables(object):
    """table_tensors[level*6 + slot] made on demand from the pyramid's rulebooks (the profiler's pair counts)"""

    def __init__(self, indice_dict, L):
        self.d, self.L = indice_dict, L

    def __getitem__(self, i):
        lvl, slot = divmod(int(i), 6)
        if slot < 2:
            rb = self.d["subm%d" % (lvl + 1)]
            return (rb.nbr_p, rb.order)[slot]
        rd = self.d["spconv%d" % (lvl + 1)]
        return (rd.nbr_p, rd.order, rd.nbr_up_p, rd.order_up)[slot - 2]


def _arena_tensor(nbytes, device, zero=False):
    make = torch.zeros if zero else torch.empty
    t = make(nbytes + 256, dtype=torch.uint8, device=device)
    return t, (t.data_ptr() + 255) // 256 * 256


def _luts(fwd, tables, ext0, ext1, bwd=None, par=None):
    """look-up tables of ``_Template.instantiate``: arena bases per allocation id, table pointers, the two external tensors"""
    none = fwd[:0]
    return {_FWD: fwd, _BWD: none if bwd is None else bwd, _PAR: none if par is None else par, _TBL: tables,
            _EXT: np.array([ext0, ext1], dtype=np.uint64)}


def _view(arena, base, offset, shape):
    numel = int(np.prod(shape))
    off = base + int(offset) - arena.data_ptr()
    return arena[off:off + numel * 4].view(torch.float32).view(shape)


class _GradArena(object):
    """the flat parameter-gradient buffer of a compiled backward program, with the per-parameter views of it.  Kept by
    the program from one backward pass to the next (the executor overwrites every gradient in it; the alignment gaps and
    the tail were zeroed once): a pass costs the host no allocation, no 230 slice / view calls."""

    @staticmethod
    def key_of(prog, c, ptotal, tail, dev):
        return (id(c), int(ptotal), int(tail), dev, tuple(p.requires_grad for p in prog.params))

    @staticmethod
    def of_pass(prog, c, poffs, ptotal, dev):
        """the program's own gradient buffer while no parameter still holds a gradient (zero_grad(set_to_none=True), the
        reference's loop); otherwise (gradient accumulation, a second backward pass) a buffer of this pass's own"""
        tail = int(prog.tail_floats) * 4
        ga = prog._garena
        if ga is None or ga.key != _GradArena.key_of(prog, c, ptotal, tail, dev):
            ga = prog._garena = _GradArena(prog, c, poffs, ptotal, tail, dev)
        if not prog.persistent_grads or any(p.grad is not None for p in ga.params):
            ga = _GradArena(prog, c, poffs, ptotal, tail, dev)
        return ga

    def __init__(self, prog, c, poffs, ptotal, tail, dev):
        self.key = self.key_of(prog, c, ptotal, tail, dev)
        self.c = c                                   # (keeps id(c) from being reused while this buffer lives)
        self.arena, self.base = _arena_tensor(ptotal + tail, dev, zero=True)   # alignment gaps are all-reduced too
        self.flat = self.arena.view(torch.float32)
        self.first = (self.base - self.arena.data_ptr()) // 4
        self.lut = poffs.astype(np.uint64) + np.uint64(self.base)
        self.params, self.views = [], []
        for i, p in enumerate(prog.params):
            gid = c.grad_ids[i]
            if gid >= 0 and p.requires_grad:
                off = self.first + int(poffs[gid]) // 4
                self.params.append(p)
                self.views.append(self.flat[off:off + p.numel()].view(p.shape))
        t0 = self.first + (ptotal + 3) // 4
        self.tail = self.flat[t0:t0 + prog.tail_floats] if prog.tail_floats else None


# ---- the pass driver: what the fp32 pass, the 16-bit training pass and the 16-bit evaluation pass do alike.  ``ext0`` /
# ``ext1``: device pointers of the two external tensors; ``sy``: the _BnSync state of a synced pass
def _issue_forward(prog, c, ext0, ext1, device, sy=None):
    """lays out the forward arena of the bound scene and issues the forward program -> (arena, base, offs, fwd_lut)"""
    for bn in c.count:
        wsis_ops._defer_batch_count(bn)
    Mvec = prog.Mvec
    offs, total = c.fwd_arena.layout(Mvec)
    arena, base = _arena_tensor(total, device)
    fwd_lut = offs.astype(np.uint64) + np.uint64(base)
    ops = c.fwd.instantiate(Mvec, _luts(fwd_lut, prog.table_lut, ext0, ext1))
    if sy is not None:
        sy.arenas = [arena]
        _run_synced(_n.hip(), ops, device, sy)
    else:
        _run(_n.hip(), ops, device)
    return arena, base, offs, fwd_lut


def _issue_backward(prog, c, Mvec, fwd_lut, table_lut, ext0, ext1, device, sy=None, arenas=(), overlap=None):
    """lays out the backward arena, takes the program's parameter-gradient buffer and issues the backward program ->
    (garena, gbase, boffs, ga).  ``arenas``: the forward pass's, which a synced layer reads; ``overlap``: a
    wsis_parallel.GradSync whose all-reduce of the first part of the gradient buffer starts inside the pass"""
    boffs, btotal = c.bwd_arena.layout(Mvec)
    poffs, ptotal = c.par_arena.layout(Mvec)
    garena, gbase = _arena_tensor(btotal, device)
    ga = _GradArena.of_pass(prog, c, poffs, ptotal, device)
    ops = c.bwd.instantiate(Mvec, _luts(fwd_lut, table_lut, ext0, ext1, bwd=boffs.astype(np.uint64) + np.uint64(gbase),
                                        par=ga.lut))
    if sy is not None:
        sy.arenas = list(arenas) + [garena, ga.arena]
        _run_synced(_n.hip(), ops, device, sy)
    elif overlap is not None and overlap.ready() and len(poffs) > 1:
        # all-reduce of the first part of the gradient buffer starts while the rest of the pass still runs
        starts = np.append(poffs, ptotal)
        want = ptotal // 2
        op_i = int(np.searchsorted(starts[c.bwd_grads_done], want))          # first op with >= half final
        op_i = min(op_i, len(c.bwd_grads_done) - 2)
        split = int(starts[c.bwd_grads_done[op_i]]) // 4
        _run(_n.hip(), ops, device, mark_op=op_i, waiter=overlap.comm_stream_ptr())
        overlap.early(ga.flat[ga.first:ga.first + split], ga.first + split)
    else:
        _run(_n.hip(), ops, device)
    return garena, gbase, boffs, ga


def _store_grads(prog, ga):
    """``.grad`` of the parameters from the views of the pass's gradient buffer (accumulated into a gradient that is
    still there) and the data-parallel hook: the gradients of ``flat_params`` are views of ``flat_grad``
    (parallel.GradSync)"""
    for p, v in zip(ga.params, ga.views):
        p.grad = v if p.grad is None else p.grad + v
    prog.flat_grad, prog.flat_params, prog.flat_tail = ga.flat, ga.params, ga.tail


class UNetFunction(Function):
    """features [M0, Cin] -> [M0, m]; ``prog`` is a bound UNetProgram.  Its parameters are NOT inputs of the node:
    ``backward`` stores their gradients (views of the program's flat buffer) in ``.grad`` itself -- what 230
    AccumulateGrad nodes did, ~1 ms of host time per step.  ``anchor`` (any parameter that requires a gradient) only
    makes autograd run the node when the input features need no gradient."""

    @staticmethod
    def forward(ctx, x, prog, anchor=None):
        _n.require_cuda(x)
        x = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.contiguous().float()
        need_dx = bool(x.requires_grad)
        c = prog.compiled(need_dx)
        Mvec, table_lut, tensors = prog.Mvec, prog.table_lut, prog.table_tensors
        sy = prog.bn_sync.new_pass() if prog.bn_sync is not None else None      # row counts / arenas belong to THIS pass
        arena, base, offs, fwd_lut = _issue_forward(prog, c, x.data_ptr(), 0, x.device, sy)
        ctx.sy = sy
        # tables sized from the batch's host-side level counts: the device's own counts are compared inside the SAME
        # pass -- an inference pass right here (its result is used next; the read waits for the rulebook chain on the
        # side stream only), a training pass at the end of its backward pass, i.e. before the optimizer can use a
        # gradient (reading here would park the issuing thread for the length of the rulebook chain, ~1 ms per step)
        if not (torch.is_grad_enabled() and (need_dx or anchor is not None)):
            sp_ops.verify_pending_counts()
        prog.account(c.acc_f, Mvec, tensors)
        out = _view(arena, base, offs[c.out_id], (int(Mvec[0]), c.out_channels))
        ctx.prog, ctx.c, ctx.arena, ctx.fwd_lut, ctx.x = prog, c, arena, fwd_lut, x
        ctx.Mvec, ctx.table_lut, ctx.tensors, ctx.keep = Mvec, table_lut, tensors, prog.keep
        return out

    @staticmethod
    def backward(ctx, d_out):
        prog, c, Mvec = ctx.prog, ctx.c, ctx.Mvec
        d_out = d_out if (d_out.dtype == torch.float32 and d_out.is_contiguous()) else d_out.contiguous().float()
        garena, gbase, boffs, ga = _issue_backward(prog, c, Mvec, ctx.fwd_lut, ctx.table_lut, ctx.x.data_ptr(),
                                                   d_out.data_ptr(), d_out.device, ctx.sy, (ctx.arena,), prog.overlap)
        prog.account(c.acc_b, Mvec, ctx.tensors)
        _store_grads(prog, ga)
        dx = _view(garena, gbase, boffs[c.dx_id], tuple(ctx.x.shape)) if c.dx_id >= 0 else None
        sp_ops.verify_pending_counts()       # (see forward: the counts of this pass's rulebooks, long written by now)
        return dx, None, None


class UNetLpTrainFunction(Function):
    """the 16-bit training pass beside ``UNetFunction``: features [M0, Cin] -> [M0, m] of ``out_dtype`` through the
    programs of ``UNetProgram.compiled_lp_train``.  The forward arena (16-bit activations, fp32 batch statistics) lives
    until the backward pass; parameter gradients are stored as in ``UNetFunction.backward`` (fp32 views of the flat buffer;
    parameters with ``requires_grad_(False)`` get none); the early all-reduce milestone (``prog.overlap``) is not used.
    With ``prog.bn_sync`` set both programs are issued in parts (``_run_synced``): the same programs, the layers' 16-bit
    synced forms between the parts."""

    @staticmethod
    def forward(ctx, x, prog, dtype, out_dtype, anchor=None):
        _n.require_cuda(x)
        need_dx = bool(x.requires_grad)
        x32 = x.detach().to(dtype).float().contiguous()      # what the walk's input convolution reads
        c = prog.compiled_lp_train(dtype, out_dtype == torch.float32, need_dx)
        Mvec = prog.Mvec
        out = torch.empty((int(Mvec[0]), c.out_channels), dtype=out_dtype, device=x.device)
        # shared BatchNorm statistics: the same programs, issued in parts around every layer (_run_synced)
        sy = ctx.sy = prog.bn_sync.new_pass() if prog.bn_sync is not None else None
        arena, _, _, fwd_lut = _issue_forward(prog, c, x32.data_ptr(), out.data_ptr(), x.device, sy)
        if not (torch.is_grad_enabled() and (need_dx or anchor is not None)):
            sp_ops.verify_pending_counts()      # (see UNetFunction.forward)
        ctx.prog, ctx.c, ctx.arena, ctx.fwd_lut, ctx.x32, ctx.dtype, ctx.in_dtype = prog, c, arena, fwd_lut, x32, dtype, x.dtype
        ctx.Mvec, ctx.table_lut, ctx.keep = Mvec, prog.table_lut, prog.keep
        return out

    @staticmethod
    def backward(ctx, d_out):
        prog, c, Mvec = ctx.prog, ctx.c, ctx.Mvec
        d16 = sp_ops._aligned(d_out.to(ctx.dtype))      # the incoming gradient, cast once
        # (overlap=None: the early all-reduce milestone is not used by this pass)
        garena, gbase, boffs, ga = _issue_backward(prog, c, Mvec, ctx.fwd_lut, ctx.table_lut, ctx.x32.data_ptr(),
                                                   d16.data_ptr(), d16.device, ctx.sy, (ctx.arena,))
        _store_grads(prog, ga)
        dx = None
        if c.dx_id >= 0:
            dx = _view(garena, gbase, boffs[c.dx_id], (int(Mvec[0]), c.in_channels)).to(ctx.in_dtype)
        sp_ops.verify_pending_counts()
        return dx, None, None, None, None


class _BnSync(object):
    """SyncBatchNorm INSIDE the executor's pass (train_scannetv2.py:734-736 converts every BatchNorm when num_gpus > 1):
    the op list is issued in parts (``wsis_run_ops_part``) that end in front of every training-mode BatchNorm op; the
    layer itself runs here -- local statistics from the producers' epilogue partials, ONE all-gather of (mean, var,
    count) combined in fp64 (Chan), apply; backward: local (sum dz, sum dz xhat), ONE all-reduce, dx with the global sums
    -- and the next part follows.  Convolutions, concatenations and the weight-gradient side stream stay in the native
    executor; every rank issues the same collectives in the same order (same op list), zero-row ranks included."""

    def __init__(self, prog, group):
        self.group = group
        self.by_ptr = {}
        for bn in prog.bns:
            for t in (bn.running_mean, bn.running_var):
                if t is not None:
                    self.by_ptr[t.data_ptr()] = t
        self.counts = {}          # mean pointer of a layer -> global row count (fp64 device scalar), forward -> backward
        self.arenas = []

    def new_pass(self):
        """the state of one forward + backward pass: two forward passes before a backward (gradient accumulation, an
        extra training-mode forward) must not wipe each other's global row counts"""
        p = _BnSync.__new__(_BnSync)
        p.group, p.by_ptr, p.counts, p.arenas = self.group, self.by_ptr, {}, []
        return p

    def view(self, ptr, numel):
        ptr = int(ptr)
        for a in self.arenas:
            base = a.data_ptr()
            if base <= ptr < base + a.numel():
                return a[ptr - base:ptr - base + 4 * numel].view(torch.float32)
        raise _n.WsisError("synced BatchNorm: pointer outside the pass's arenas")


def _bn_fwd_synced(lib, op, sy, dev, st, slot):
    import torch.distributed as dist
    M, C, flags = int(op["M_in"]), int(op["Cin"]), int(op["flags"])
    inp, out = [int(v) for v in op["inp"]], [int(v) for v in op["out"]]
    mom, eps = float(op["momentum"]), float(op["eps"])
    x, y, p_mean, p_var = inp[S_BN.X], out[S_BN.Y], out[S_BN.MEAN], out[S_BN.VAR]
    parts0, parts1 = inp[S_BN.PARTS0], inp[S_BN.PARTS1]
    mean, var = sy.view(p_mean, C), sy.view(p_var, C)
    if M > 0 and (flags & F_STATS):
        n_part = (M + 31) // 32
        C0 = int(op["K"]) if parts1 else C
        wsb = lib.wsis_bn_stats_finalize_workspace_bytes(n_part, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _n.check(lib.wsis_bn_stats_finalize(parts0, n_part, M, C0, p_mean, p_var, None, None, mom, _n.ptr(ws), wsb, slot, st),
                 "bn_stats_finalize")
        if parts1:
            _n.check(lib.wsis_bn_stats_finalize(parts1, n_part, M, C - C0, p_mean + 4 * C0, p_var + 4 * C0, None, None, mom,
                                                _n.ptr(ws), wsb, slot, st), "bn_stats_finalize")
    elif M > 0:
        wsb = lib.wsis_bn_workspace_bytes(M, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _n.check(lib.wsis_bn_stats(x, M, C, p_mean, p_var, None, None, mom, _n.ptr(ws), wsb, st), "bn_stats")
    else:
        mean.zero_()
        var.zero_()
    t = torch.cat((mean.double(), var.double(), torch.full((1,), float(M), dtype=torch.float64, device=dev)))
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size(sy.group))]
    dist.all_gather(parts, t, group=sy.group)
    g = torch.stack(parts)
    n_i = g[:, 2 * C:2 * C + 1]
    N = n_i.sum()
    mean64 = (g[:, :C] * n_i).sum(0) / N
    dm = g[:, :C] - mean64
    var64 = ((g[:, C:2 * C] + dm * dm) * n_i).sum(0) / N
    mean.copy_(mean64.float())
    var.copy_(var64.float())
    if flags & F_UPDATE:
        rm, rv = sy.by_ptr[inp[S_BN.RMEAN]], sy.by_ptr[inp[S_BN.RVAR]]
        unb = var64 * (N / (N - 1.0).clamp_min(1.0))
        rm.mul_(1.0 - mom).add_(mean, alpha=mom)
        rv.mul_(1.0 - mom).add_(unb.float(), alpha=mom)
    sy.counts[p_mean] = N
    if y and M > 0:
        _n.check(lib.wsis_bn_apply(x, p_mean, p_var, inp[S_BN.GAMMA] or None, inp[S_BN.BETA] or None, eps,
                                   1 if flags & F_RELU else 0, y, M, C, st), "bn_apply")


def _bn_bwd_synced(lib, op, sy, dev, st):
    import torch.distributed as dist
    S = S_BN_BWD
    M, C, flags = int(op["M_in"]), int(op["Cin"]), int(op["flags"])
    inp, out = [int(v) for v in op["inp"]], [int(v) for v in op["out"]]
    eps, relu = float(op["eps"]), 1 if flags & F_RELU else 0
    # x, dy, mean, var, gamma, beta: the leading arguments of both kernels
    args = (inp[S.X], inp[S.DY], inp[S.MEAN], inp[S.VAR], inp[S.GAMMA] or None, inp[S.BETA] or None)
    dg, db = sy.view(out[S.DGAMMA], C), sy.view(out[S.DBETA], C)
    if M > 0:
        wsb = lib.wsis_bn_workspace_bytes(M, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _n.check(lib.wsis_bn_bwd(*args, eps, relu, 1, None, out[S.DGAMMA], out[S.DBETA], None, M, C, _n.ptr(ws), wsb, st),
                 "bn_bwd")
    else:
        dg.zero_()
        db.zero_()
    g = torch.cat((dg, db)).double()
    dist.all_reduce(g, group=sy.group)
    N = sy.counts[inp[S.MEAN]]
    if M > 0:
        sc = (g * (float(M) / N)).float()      # the kernel divides by the local row count
        _n.check(lib.wsis_bn_bwd_apply(*args, _n.ptr(sc[:C]), _n.ptr(sc[C:]), eps, relu, out[S.DX], inp[S.ADDEND] or None,
                                       M, C, st), "bn_bwd_apply")


def _bn_fwd_synced_lp(lib, op, sy, dev, st):
    """the forward form of a synced layer of the 16-bit pass: local statistics of the 16-bit x, ONE all-gather of
    (mean, var, rows) packed and combined by one small kernel on either side (wsis_bn_sync_pack / _combine: the
    expressions of ``_bn_fwd_synced``), apply.  A rank without rows enters the collective with zeros."""
    import torch.distributed as dist
    M, C, flags, code = int(op["M_in"]), int(op["Cin"]), int(op["flags"]), int(op["reserved"])
    inp, out = [int(v) for v in op["inp"]], [int(v) for v in op["out"]]
    x, p_mean, p_var = inp[S_BN.X], out[S_BN.MEAN], out[S_BN.VAR]
    R = dist.get_world_size(sy.group)
    # rows 0 .. R-1: the ranks' contributions (the all-gather writes views of them: no stack), row R: this rank's own
    buf = torch.empty((R + 1, 2 * C + 1), dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.float64, device=dev)
    if M > 0:
        wsb = lib.wsis_bn_workspace_bytes(M, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _n.check(lib.wsis_bn_stats_lp(x, M, C, p_mean, p_var, None, None, 0.0, _n.ptr(ws), wsb, code, st), "bn_stats_lp")
    _n.check(lib.wsis_bn_sync_pack(p_mean, p_var, M, C, _n.ptr(buf[R]), st), "bn_sync_pack")
    dist.all_gather(list(buf[:R].unbind(0)), buf[R], group=sy.group)
    upd = bool(flags & F_UPDATE)
    _n.check(lib.wsis_bn_sync_combine(_n.ptr(buf), R, C, p_mean, p_var, inp[S_BN.RMEAN] if upd else None,
                                      inp[S_BN.RVAR] if upd else None, float(op["momentum"]), _n.ptr(count), st),
             "bn_sync_combine")
    sy.counts[p_mean] = count
    _n.check(lib.wsis_bn_apply_lp(x, p_mean, p_var, inp[S_BN.GAMMA] or None, inp[S_BN.BETA] or None, float(op["eps"]),
                                  1 if flags & F_RELU else 0, out[S_BN.Y], 1 if flags & F_OUT_F32 else 0, M, C, code, st),
             "bn_apply_lp")


def _bn_bwd_synced_lp(lib, op, sy, dev, st):
    """the backward form: local (sum dz xhat, sum dz) -- they stay the layer's dgamma / dbeta in the flat gradient buffer,
    as in ``_bn_bwd_synced`` --, ONE all-reduce of their fp64 copies, dx from the global sums scaled by M / N"""
    import torch.distributed as dist
    S = S_BN_BWD
    M, C, flags, code = int(op["M_in"]), int(op["Cin"]), int(op["flags"]), int(op["reserved"])
    inp, out = [int(v) for v in op["inp"]], [int(v) for v in op["out"]]
    eps, relu = float(op["eps"]), 1 if flags & F_RELU else 0
    args = (inp[S.X], inp[S.DY], inp[S.MEAN], inp[S.VAR], inp[S.GAMMA] or None, inp[S.BETA] or None)
    g = torch.empty(2 * C, dtype=torch.float64, device=dev)
    if M > 0:
        wsb = lib.wsis_bn_workspace_bytes(M, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _n.check(lib.wsis_bn_bwd_lp(*args, eps, relu, 1, None, 0, out[S.DGAMMA], out[S.DBETA], None, M, C, code, _n.ptr(ws),
                                    wsb, st), "bn_bwd_lp")
    else:
        sy.view(out[S.DGAMMA], C).zero_()
        sy.view(out[S.DBETA], C).zero_()
    _n.check(lib.wsis_bn_sync_sums_pack(out[S.DGAMMA], out[S.DBETA], C, _n.ptr(g), st), "bn_sync_sums_pack")
    dist.all_reduce(g, group=sy.group)
    if M > 0:
        sc = torch.empty(2 * C, dtype=torch.float32, device=dev)
        _n.check(lib.wsis_bn_sync_sums_scale(_n.ptr(g), M, _n.ptr(sy.counts[inp[S.MEAN]]), C, _n.ptr(sc), _n.ptr(sc[C:]), st),
                 "bn_sync_sums_scale")
        _n.check(lib.wsis_bn_bwd_apply_lp(*args, _n.ptr(sc), _n.ptr(sc[C:]), eps, relu, out[S.DX],
                                          1 if flags & F_OUT_F32 else 0, inp[S.ADDEND] or None, M, C, code, st),
                 "bn_bwd_apply_lp")


def _run_synced(lib, ops, device, sy):
    n = len(ops)
    base, item = ops.ctypes.data, ops.dtype.itemsize
    kinds = ops["kind"]
    # backward: the dIn epilogue's partials pair a CONV_BWD op with the BatchNorm op behind it INSIDE one list; the parts
    # end in front of that op and the synced layer makes its own reduction pass, so the pairing is switched off
    bwd_pair = (kinds == OP_CONV_BWD) | (kinds == OP_BN_RELU_BWD)
    ops["flags"] = np.where(bwd_pair, ops["flags"] & ~F_STATS, ops["flags"])
    flags = ops["flags"]
    is_bn = ((kinds == OP_BN_RELU) | (kinds == OP_BN_RELU_BWD)) & ((flags & F_TRAINING) != 0)
    sync = _n.ptr(_n.sync_block(device))
    st = _n.stream_ptr()
    keep = []                     # every part's workspace stays alive until the weight-gradient side stream is joined
    # whatever happens between the parts (a collective that times out, a failed check), the joining call must be issued:
    # it clears the side stream's pending join and orders the queued weight-gradient launches before `keep` is freed
    try:
        i = 0
        while i < n:
            j = i
            while j < n and not is_bn[j]:
                j += 1
            if j > i:
                p = base + i * item
                wsb = lib.wsis_run_ops_workspace_bytes(p, j - i)
                if wsb < 0:
                    raise _n.WsisError("run_ops workspace query failed")
                ws = torch.empty(wsb, dtype=torch.uint8, device=device)
                keep.append(ws)
                _n.check(lib.wsis_run_ops_part(p, j - i, _n.ptr(ws), wsb, sync, st, 0), "run_ops_part")
            if j < n:
                fwd, lp = int(kinds[j]) == OP_BN_RELU, bool(int(flags[j]) & F_LP)
                if lp:      # a layer of the 16-bit pass: its own forms, the exchange in one small kernel per side
                    (_bn_fwd_synced_lp if fwd else _bn_bwd_synced_lp)(lib, ops[j], sy, device, st)
                elif fwd:
                    _bn_fwd_synced(lib, ops[j], sy, device, st, sync)
                else:
                    _bn_bwd_synced(lib, ops[j], sy, device, st)
                j += 1
            i = j
    finally:
        _n.check(lib.wsis_run_ops_part(None, 0, None, 0, sync, st, 1), "run_ops_part")
    return keep


def _run(lib, ops, device, mark_op=-1, waiter=None):
    n = len(ops)
    p = ops.ctypes.data
    ws_bytes = lib.wsis_run_ops_workspace_bytes(p, n)
    if ws_bytes < 0:
        raise _n.WsisError("run_ops workspace query failed")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    sync = _n.ptr(_n.sync_block(device))
    if mark_op >= 0:
        _n.check(lib.wsis_run_ops_marked(p, n, _n.ptr(ws), ws_bytes, sync, _n.stream_ptr(), int(mark_op), waiter),
                 "run_ops")
    else:
        _n.check(lib.wsis_run_ops(p, n, _n.ptr(ws), ws_bytes, sync, _n.stream_ptr()), "run_ops")


_EXPERIMENTAL_SWITCHES = ("WSIS_DEEP", "WSIS_FWD2P", "WSIS_RING", "WSIS_GRAPH", "WSIS_BN_FUSED_APPLY", "WSIS_BN_FUSED_FWD", "WSIS_BN_FUSED_BWD")


# launch-plan / tuning knobs the C layer reads through tune_env() (csrc/common.h): live in the EXPERIMENTAL build, compiled
# to their measured defaults in the default library (tests/test_abi.py keeps this list equal to the sources)
TUNE_KNOBS = (
    "WSIS_BN_FUSED_GRID", "WSIS_BN_TICKET", "WSIS_DW2", "WSIS_DW2_HI", "WSIS_DW2_LO",
    "WSIS_DW2_WAVES", "WSIS_DW2_XCD", "WSIS_DW2_XSH", "WSIS_DW2_DENSE_WG", "WSIS_DW2_RED", "WSIS_DW2_PFLOOR", "WSIS_DW_BAL", "WSIS_DW_H16", "WSIS_DW_DIV", "WSIS_DW_THREAD", "WSIS_FWD2P_MIN",
    "WSIS_FWD2_BD", "WSIS_FWD2_DA_NW4", "WSIS_FWD2_DEAL", "WSIS_FWD2_NOSLAB", "WSIS_FWD2_NW", "WSIS_FWD2_NW_MAX",
    "WSIS_FWD2_NW_MAX_NOSLAB", "WSIS_FWD2_RG", "WSIS_FWD2_RGH", "WSIS_FWD2_RGH_LATE", "WSIS_FWD2_SNAKE",
    "WSIS_FWD2_TR", "WSIS_FWD2_TR_DA", "WSIS_FWD2_WAVES", "WSIS_FWD2_XCD", "WSIS_FWD2_ZS", "WSIS_FWD_NB_SMALL",
    "WSIS_FWD_SMALL_TILES", "WSIS_KSPLIT_TARGET", "WSIS_SL_BLOCKS", "WSIS_TILE_BAND", "WSIS_TILE_SCHED",
    "WSIS_TILE_SCHED_MIN", "WSIS_XCD_AWARE")
_WARNED_KNOBS = set()
_KNOB_SCAN = [0]


def _check_experimental_switches():
    """the switches of the retired designs exist in the EXPERIMENTAL build only: asking for one on
    the default library is an error, not a silent no-op; a tuning knob that is set while the default library is loaded
    (where it compiles to its default) gets ONE warning -- an A/B tool run on the wrong flavour must not report A == B
    silently"""
    for k in _EXPERIMENTAL_SWITCHES:
        if os.environ.get(k, "0") not in ("", "0"):
            _n.require_experimental(k + "=" + os.environ[k])
    _KNOB_SCAN[0] += 1
    if _KNOB_SCAN[0] > 4 and _KNOB_SCAN[0] % 64:       # (the scan is ~10 us of host time: the first passes, then 1 in 64)
        return
    ignored = [k for k in TUNE_KNOBS if k in os.environ and k not in _WARNED_KNOBS]
    if ignored and not _n.experimental():
        import warnings
        _WARNED_KNOBS.update(ignored)
        warnings.warn("tuning knob(s) %s are set but the DEFAULT libwsis_hip.so is loaded: they are live in the "
                      "EXPERIMENTAL build only (make -C 3d-wsis_amd/csrc EXPERIMENTAL=1) and have no effect here"
                      % ", ".join(ignored), RuntimeWarning, stacklevel=2)


def lp_pass_wanted(env, compute_dtype, grad_enabled, params_fp32, bn_eval, in_domain):
    """does ``Network.forward`` take the 16-bit native pass?  ``env``: the environment (WSIS_NATIVE_LP=1 switches it on,
    WSIS_NATIVE_UNET=0 off), ``compute_dtype``: spconv.ops.compute_dtype of the input features, ``grad_enabled``:
    torch.is_grad_enabled(); the model's conditions, each a bool or a callable that returns one: ``params_fp32``: every
    parameter and running statistic the pass reads is a contiguous fp32 tensor on the features' device
    (``lp_params_fp32``: the executor reads them as fp32 through raw pointers), ``bn_eval``: every BatchNorm layer of the
    UNet in evaluation mode with running statistics (``lp_bn_eval``), ``in_domain``: every product inside
    spconv.ops.lp_supported (``lp_in_domain``).  The cheap conditions come first: a callable runs only when everything
    in front of it holds.  Pure: no device."""
    return _lp_wanted(env, "WSIS_NATIVE_LP", compute_dtype, grad_enabled, False, (params_fp32, bn_eval, in_domain))


def lp_train_pass_wanted(env, compute_dtype, grad_enabled, params_fp32, bn_train, in_domain, synced):
    """does ``Network.forward`` take the 16-bit native TRAINING pass?  ``env``: the environment (WSIS_NATIVE_LP_TRAIN=1
    switches it on, WSIS_NATIVE_UNET=0 off), ``compute_dtype`` / ``grad_enabled`` as for ``lp_pass_wanted``; then, each a
    bool or a callable that returns one: ``synced``: a SyncBatchNorm group is present -- that refuses the pass unless
    WSIS_NATIVE_LP_SYNC=1 opts into its synced form (the statistics exchange between the parts of the pass,
    ``_bn_fwd_synced_lp`` / ``_bn_bwd_synced_lp``; with the switch the group is not asked for here: ``Network.forward``
    hands it to ``run_unet_lp_train``) --, ``params_fp32`` (``lp_params_fp32``), ``bn_train``: every BatchNorm layer of
    the UNet in training mode with running statistics (``lp_bn_train``), ``in_domain``: every forward, dIn and dW product
    inside spconv.ops.lp_supported (``lp_train_in_domain``).  The cheap conditions come first: a callable runs only when
    everything in front of it holds.  Pure: no device."""
    sync_ok = lambda: env.get("WSIS_NATIVE_LP_SYNC", "0") == "1" or not _holds(synced)      # noqa: E731
    return _lp_wanted(env, "WSIS_NATIVE_LP_TRAIN", compute_dtype, grad_enabled, True,
                      (sync_ok, params_fp32, bn_train, in_domain))


def _holds(check):
    return bool(check() if callable(check) else check)


def _lp_wanted(env, switch, compute_dtype, grad_enabled, want_grad, checks):
    """the one dispatch rule of the 16-bit native passes: ``switch`` is on and WSIS_NATIVE_UNET not off, 16-bit compute
    dtype, ``grad_enabled`` as the pass wants it, then ``checks`` in order, each run only if all before it hold"""
    if not (env.get(switch, "0") == "1" and env.get("WSIS_NATIVE_UNET", "1") != "0"
            and compute_dtype in (torch.bfloat16, torch.float16) and bool(grad_enabled) == want_grad):
        return False
    return all(_holds(c) for c in checks)


def _lp_modules(net):
    return [m for mod in (net.unet, net.output_layer) for m in mod.modules()]


def _lp_bns(net, training):
    """the BatchNorm layers of unet + output_layer if every one is in the mode ``training`` and keeps running statistics,
    else None"""
    bns = [m for m in _lp_modules(net) if isinstance(m, nn.BatchNorm1d)]
    ok = all(m.training == training and m.track_running_stats and m.running_mean is not None and m.running_var is not None
             for m in bns)
    return bns if ok else None


def _lp_convs(net):
    """(K, Cin, Cout) of every sparse convolution of the UNet"""
    import spconv
    return [(int(np.prod(m.kernel_size)), m.in_channels, m.out_channels)
            for m in net.unet.modules() if isinstance(m, spconv.conv.SparseConvolution)]


def lp_params_fp32(net, device):
    """every parameter of input_conv + unet + output_layer and every BatchNorm running statistic is a contiguous fp32
    tensor on ``device`` (a model converted with ``.to(torch.bfloat16)`` walks the modules, which widen its weights)"""
    dev = torch.device(device)
    ts = [p for m in (net.input_conv, net.unet, net.output_layer) for p in m.parameters()]
    ts += [t for m in _lp_modules(net) if isinstance(m, nn.BatchNorm1d) for t in (m.running_mean, m.running_var)
           if t is not None]
    return all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in ts)


def lp_bn_eval(net):
    """every BatchNorm layer of unet + output_layer normalises with its running statistics"""
    return _lp_bns(net, False) is not None


def lp_bn_train(net):
    """every BatchNorm layer of unet + output_layer takes batch statistics and updates running ones (channel counts
    inside the 16-bit BatchNorm kernels' domain)"""
    bns = _lp_bns(net, True)
    return bns is not None and all(m.momentum is not None and m.num_features % 8 == 0 and m.num_features <= 1024 for m in bns)


def lp_train_in_domain(net, rows):
    """every sparse product of a training pass of the UNet inside spconv.ops.lp_supported: forward, dIn (the channel
    counts swap) and dW (its dY below 2 GiB too); ``rows``: the finest level's row count, an upper bound of every level's"""
    return all(sp_ops.lp_supported(K, Cin, Cout, rows) and sp_ops.lp_supported(K, Cout, Cin, rows)
               and rows * Cout * 2 < (1 << 31) for K, Cin, Cout in _lp_convs(net))


def lp_in_domain(net, rows):
    """every sparse product of the UNet (forward) inside spconv.ops.lp_supported; ``rows``: the finest level's row count,
    an upper bound of every level's"""
    return all(sp_ops.lp_supported(K, Cin, Cout, rows) for K, Cin, Cout in _lp_convs(net))


def lp_out_dtype(compute_dtype, autocast):
    """the dtype the module walk returns for the UNet: the output layer's BatchNorm1d keeps its 16-bit input's dtype
    unless autocast casts batch_norm, then fp32.  torch's documented CUDA autocast lists do not name batch_norm; the
    dispatcher is asked where it can be (a torch without that query: the documented behaviour)"""
    has_kernel = getattr(torch._C, "_dispatch_has_kernel_for_dispatch_key", None)
    if autocast and has_kernel is not None:
        try:
            if has_kernel("aten::batch_norm", "AutocastCUDA"):
                return torch.float32
        except (RuntimeError, TypeError):
            pass
    return compute_dtype


def _program(net):
    """the model's UNetProgram (made on first use, kept on the model)"""
    prog = getattr(net, "_native_prog", None)
    if prog is None:
        prog = net._native_prog = UNetProgram(net)
    return prog


def run_unet_lp(net, input_tensor, dtype, out_dtype):
    """the 16-bit evaluation-mode forward of input_conv + unet + output_layer (no gradient): features -> [M0, m] of
    ``out_dtype`` (``dtype`` or fp32).  The input features are rounded to ``dtype`` and widened, exactly what the walk's
    input convolution reads; every 16-bit value of the pass is rounded once (input convolution output, convolution
    epilogues after the residual, BatchNorm applies), concatenations copy bits."""
    _check_experimental_switches()
    prog = _program(net)
    prog.bind(input_tensor)
    x = input_tensor.features
    _n.require_cuda(x)
    x = x.detach().to(dtype).float().contiguous()
    c = prog.compiled_lp(dtype, out_dtype == torch.float32)
    out = torch.empty((int(prog.Mvec[0]), c.out_channels), dtype=out_dtype, device=x.device)
    _issue_forward(prog, c, x.data_ptr(), out.data_ptr(), x.device)      # (the arena is free once the call is issued)
    sp_ops.verify_pending_counts()
    return out


def _select_bn_sync(prog, sync_group):
    """the program's _BnSync for ``sync_group`` (None: per-rank statistics), kept while the group stays the same"""
    if sync_group is None:
        prog.bn_sync = None
    elif prog.bn_sync is None or prog.bn_sync.group is not sync_group:
        prog.bn_sync = _BnSync(prog, sync_group)


def run_unet_lp_train(net, input_tensor, dtype, out_dtype, sync_group=None):
    """the 16-bit training pass of input_conv + unet + output_layer: features -> [M0, m] of ``out_dtype`` with a
    backward pass (``UNetLpTrainFunction``; rounding contract: DESIGN.md section 10.2).  ``sync_group``: the process group
    the BatchNorm layers take their batch statistics over (None: per rank)"""
    _check_experimental_switches()
    prog = _program(net)
    _select_bn_sync(prog, sync_group)
    prog.bind(input_tensor)
    anchor = next((p for p in prog.params if p.requires_grad), None)
    return UNetLpTrainFunction.apply(input_tensor.features, prog, dtype, out_dtype, anchor)


def run_unet(net, input_tensor, sync_group=None):
    """input_conv + unet + output_layer of ``net`` on ``input_tensor`` (SparseConvTensor) -> features [M0, m].
    ``sync_group``: the process group the BatchNorm layers take their batch statistics over (None: per rank)"""
    _check_experimental_switches()
    prog = _program(net)
    _select_bn_sync(prog, sync_group)
    prog.bind(input_tensor)
    anchor = next((p for p in prog.params if p.requires_grad), None) if torch.is_grad_enabled() else None
    return UNetFunction.apply(input_tensor.features, prog, anchor)
