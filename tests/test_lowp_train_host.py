"""CPU: the 16-bit native TRAINING pass of the UNet without a GPU -- the dispatch rule as a pure function, the forward and
backward op lists UNetProgram records for it, and the executor's workspace queries and refusals for the 16-bit training
ops (host-only: every refusal happens before anything touches the device)."""
import ctypes

import numpy as np
import pytest
import torch

import harness
import unet_native as un
import wsis_native

DT = (torch.bfloat16, torch.float16)
ON = {"WSIS_NATIVE_LP_TRAIN": "1"}
ALL = (True, True, True, False)      # params_fp32, bn_train, in_domain, synced


def test_predicate_needs_every_condition():
    for dt in DT:
        assert un.lp_train_pass_wanted(ON, dt, True, *ALL)
    assert not un.lp_train_pass_wanted({}, torch.bfloat16, True, *ALL), "the switch defaults to off"
    assert not un.lp_train_pass_wanted({"WSIS_NATIVE_LP": "1"}, torch.bfloat16, True, *ALL), "the inference switch is another one"
    assert not un.lp_train_pass_wanted({"WSIS_NATIVE_LP_TRAIN": "0"}, torch.bfloat16, True, *ALL)
    assert not un.lp_train_pass_wanted(dict(ON, WSIS_NATIVE_UNET="0"), torch.bfloat16, True, *ALL)
    assert un.lp_train_pass_wanted(dict(ON, WSIS_NATIVE_UNET="1"), torch.bfloat16, True, *ALL)
    for cd in (None, torch.float32, torch.float64):
        assert not un.lp_train_pass_wanted(ON, cd, True, *ALL)
    assert not un.lp_train_pass_wanted(ON, torch.bfloat16, False, *ALL), "no_grad: not a training pass"
    assert not un.lp_train_pass_wanted(ON, torch.bfloat16, True, False, True, True, False), "16-bit (or misplaced) parameters"
    assert not un.lp_train_pass_wanted(ON, torch.bfloat16, True, True, False, True, False), "an evaluation-mode BatchNorm"
    assert not un.lp_train_pass_wanted(ON, torch.float16, True, True, True, False, False), "a product outside the domain"
    assert not un.lp_train_pass_wanted(ON, torch.float16, True, True, True, True, True), "a SyncBatchNorm group"


def test_predicate_runs_the_model_checks_last_and_lazily():
    calls = []

    def check(name, value):
        return lambda: calls.append(name) or value

    def wanted(env, cd, grad, p=True, b=True, d=True, s=False):
        return un.lp_train_pass_wanted(env, cd, grad, check("p", p), check("b", b), check("d", d), check("s", s))
    for args in (({}, torch.bfloat16, True), (ON, None, True), (ON, torch.bfloat16, False),
                 (dict(ON, WSIS_NATIVE_UNET="0"), torch.bfloat16, True)):
        assert not wanted(*args)
    assert calls == [], "a failed cheap condition: no model check runs"
    assert wanted(ON, torch.bfloat16, True)
    assert sorted(calls) == ["b", "d", "p", "s"]
    for failing in "pbds":
        calls.clear()
        assert not wanted(ON, torch.bfloat16, True, **{failing: failing == "s"})
        assert calls[-1] == failing and len(calls) == len(set(calls)), "the first failing check ends it"


def _model():
    model, _, _ = harness.build_model(harness.default_cfg(), "cpu")
    return model.train()


def test_bn_train_and_domain_of_the_model():
    model = _model()
    assert un.lp_bn_train(model)
    assert un.lp_train_in_domain(model, 778_000)
    assert not un.lp_train_in_domain(model, 1 << 25), "2 GiB gathered tensors are outside the 16-bit kernels"
    model.unet.blocks.block0.conv_branch[0].eval()
    assert not un.lp_bn_train(model), "one evaluation-mode BatchNorm"
    model.train()
    model.output_layer[0].track_running_stats = False
    assert not un.lp_bn_train(model)
    m16 = _model().to(torch.bfloat16)
    with pytest.raises(ValueError):
        un.UNetProgram(m16).compiled_lp_train(torch.bfloat16, False, False)


FAKE = np.uint64(1 << 40)
M = (5000, 1200, 300, 80, 20)


def _instantiate(c):
    """both templates with fake (never dereferenced) device addresses: enough for the host-side queries"""
    Mvec = np.asarray(M, dtype=np.int64)
    lut = {}
    for k, (tag, arena) in enumerate(((un._FWD, c.fwd_arena), (un._BWD, c.bwd_arena), (un._PAR, c.par_arena))):
        offs, _ = arena.layout(Mvec)
        lut[tag] = offs.astype(np.uint64) + FAKE * np.uint64(k + 2)
    lut[un._TBL] = np.arange(1, 31, dtype=np.uint64) * np.uint64(4096) + FAKE
    lut[un._EXT] = np.array([FAKE, FAKE + np.uint64(1 << 30)], dtype=np.uint64)
    return c.fwd.instantiate(Mvec, lut), c.bwd.instantiate(Mvec, lut)


def _activation_floats(arena):
    """floats per scene of the per-row allocations of an arena (not the per-channel vectors, not per-slice partials)"""
    rows = np.asarray(M, dtype=np.int64)[np.maximum(arena.level, 0)]
    return np.where((arena.level >= 0) & ~arena.slices, rows * arena.mult, 0)


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp16"])
def test_recorded_program(dt, out_f32, need_dx, monkeypatch):
    model = _model()
    prog = un.UNetProgram(model)
    c = prog.compiled_lp_train(dt, out_f32, need_dx)
    assert prog.compiled_lp_train(dt, out_f32, need_dx) is c, "cached per (model, dtype, output dtype, need_dx, mode)"
    assert prog.compiled_lp_train(dt, not out_f32, need_dx) is not c
    assert prog.compiled_lp_train(dt, out_f32, not need_dx) is not c
    fwd, bwd = _instantiate(c)
    code = 0 if dt == torch.bfloat16 else 1
    kinds, flags = fwd["kind"], fwd["flags"]
    # forward: input conv (fp32 op), its rounding, then 16-bit ops only, every BatchNorm in training form
    assert kinds[0] == un.OP_CONV and flags[0] == 0 and fwd["Cin"][0] == 6 and fwd["inp"][0][0] == int(FAKE)
    assert kinds[1] == un.OP_CAST_LP
    assert np.all(flags[1:] & un.F_LP) and np.all(fwd["reserved"][1:] == code) and fwd["reserved"][0] == 0
    assert np.all(flags[1:] & un.F_LP_TRAIN) and not flags[0] & un.F_LP_TRAIN, "recorded as a training pass"
    is_bn = kinds == un.OP_BN_RELU
    both = un.F_TRAINING | un.F_UPDATE
    assert np.all((flags[is_bn] & both) == both)
    assert np.all(fwd["out"][is_bn][:, 1] != 0) and np.all(fwd["out"][is_bn][:, 2] != 0), "mean / var of every layer are saved"
    fused = un.F_STATS | un.F_BN_IN | un.F_STAT_FIN
    assert not np.any(flags & fused) and not np.any(bwd["flags"] & fused)
    assert set(kinds.tolist()) == {un.OP_CONV, un.OP_CAST_LP, un.OP_BN_RELU, un.OP_CAT}
    n_bn = sum(1 for m in list(model.unet.modules()) + list(model.output_layer.modules())
               if isinstance(m, torch.nn.BatchNorm1d))
    assert int(is_bn.sum()) == n_bn
    assert kinds[-1] == un.OP_BN_RELU and fwd["out"][-1][0] == int(FAKE + np.uint64(1 << 30)), "output: the caller's tensor"
    assert int(np.sum((flags & un.F_OUT_F32) != 0)) == (1 if out_f32 else 0) and bool(flags[-1] & un.F_OUT_F32) == out_f32
    # backward: one CONV_BWD per CONV, one BN_RELU_BWD per BN_RELU (the layers in reverse), one SPLIT per CAT
    bk, bf = bwd["kind"], bwd["flags"]
    assert set(bk.tolist()) == {un.OP_CONV_BWD, un.OP_BN_RELU_BWD, un.OP_SPLIT}
    assert int(np.sum(bk == un.OP_SPLIT)) == int(np.sum(kinds == un.OP_CAT)) == model.blocks - 1
    bbn = bk == un.OP_BN_RELU_BWD
    assert bwd["inp"][bbn][:, 0].tolist() == fwd["inp"][is_bn][:, 0].tolist()[::-1], "x of every layer, in reverse"
    assert bwd["inp"][bbn][:, 2].tolist() == fwd["out"][is_bn][:, 1].tolist()[::-1], "its saved mean"
    assert bwd["inp"][bbn][:, 3].tolist() == fwd["out"][is_bn][:, 2].tolist()[::-1], "its saved var"
    assert np.all((bf[bbn] & un.F_TRAINING) != 0) and not np.any(bf[bbn] & un.F_UPDATE)
    assert np.all((bf[bbn] & un.F_RELU) == (flags[is_bn] & un.F_RELU)[::-1])
    conv_f, conv_b = kinds == un.OP_CONV, bk == un.OP_CONV_BWD

    def shapes(ops, sel, x_slot):
        return sorted(zip(ops["K"][sel].tolist(), ops["Cin"][sel].tolist(), ops["Cout"][sel].tolist(),
                          ops["M_in"][sel].tolist(), ops["M_out"][sel].tolist(), ops["inp"][sel][:, x_slot].tolist()))
    assert shapes(fwd, conv_f, 0) == shapes(bwd, conv_b, 0), "same products on the same saved inputs"
    assert bk[-1] == un.OP_CONV_BWD and bf[-1] == un.F_FLIP and bwd["Cin"][-1] == 6, "the fp32 input convolution comes last"
    assert (bwd["out"][-1][0] != 0) == need_dx
    assert np.all(bf[:-1] & un.F_LP) and np.all(bwd["reserved"][:-1] == code) and bwd["reserved"][-1] == 0
    assert np.all(bf[:-1] & un.F_LP_TRAIN)
    assert np.all(bwd["out"][conv_b][:-1, 0] != 0), "every 16-bit convolution passes a gradient down"
    sub = (bwd["K"] == 27) & conv_b
    assert np.all((bf[sub] & un.F_FLIP) != 0) and not np.any(bf[conv_b & (bwd["K"] == 8)] & un.F_FLIP)
    # fp32 dx exactly on the first block's BatchNorm backward (the last one issued); the input convolution reads it
    f32 = np.nonzero(bf & un.F_OUT_F32)[0]
    assert f32.tolist() == [len(bwd) - 2] and bk[f32[0]] == un.OP_BN_RELU_BWD
    assert bwd["inp"][f32[0]][0] == fwd["out"][1][0], "x of that layer is the rounded output of the input convolution"
    assert bwd["inp"][-1][2] == bwd["out"][f32[0]][0]
    assert bwd["inp"][0][1] == int(FAKE + np.uint64(1 << 30)), "the incoming gradient is external slot 1"
    # every parameter has a gradient slot, each written by exactly one op
    assert all(g >= 0 for g in c.grad_ids) and len(set(c.grad_ids)) == len(prog.params)
    offs, _ = c.par_arena.layout(np.asarray(M))
    written = [int(v) for o in bwd for v in (o["out"][1:3] if o["kind"] == un.OP_BN_RELU_BWD else o["out"][1:2])
               if o["kind"] != un.OP_SPLIT]
    assert sorted(written) == sorted(int(FAKE * np.uint64(4)) + int(offs[g]) for g in c.grad_ids)
    # 16-bit activations take half the floats of the fp32 program's (same tensors: the fp32 program without its fused
    # forms keeps one activation per op too; its output BatchNorm writes into the arena, this one to the caller)
    for k in ("WSIS_FUSE_BN_STATS", "WSIS_FUSE_BN_BWD"):
        monkeypatch.setenv(k, "0")
    c32 = prog.compiled(need_dx)
    a16 = _activation_floats(c.fwd_arena)
    a32 = _activation_floats(c32.fwd_arena)
    out32 = M[0] * c.out_channels
    y32 = M[0] * int(fwd["Cout"][0])                 # the fp32 output of the input convolution (in front of its rounding)
    assert 2 * (int(a16.sum()) - y32) == int(a32.sum()) - out32
    g16, g32 = _activation_floats(c.bwd_arena), _activation_floats(c32.bwd_arena)
    dx_in = M[0] * 6 if need_dx else 0
    d32 = M[0] * int(fwd["Cout"][0])                 # the one fp32 gradient of the 16-bit pass
    assert 2 * (int(g16.sum()) - dx_in - d32) == int(g32.sum()) - dx_in - d32
    # the executor sizes both lists: the 16-bit weights of every product live in the call's workspace
    lib = wsis_native.hip()
    wf = lib.wsis_run_ops_workspace_bytes(fwd.ctypes.data, len(fwd))
    wb = lib.wsis_run_ops_workspace_bytes(bwd.ctypes.data, len(bwd))
    wt = sum(int(o["K"]) * int(o["Cin"]) * int(o["Cout"]) * 2 for o in fwd[2:] if o["kind"] == un.OP_CONV)
    assert wf >= wt > 0 and wb >= wt, (wf, wb, wt)


def test_program_follows_the_batchnorm_mode():
    model = _model()
    prog = un.UNetProgram(model)
    c = prog.compiled_lp_train(torch.bfloat16, False, False)
    model.unet.blocks.block0.conv_branch[0].eval()
    c2 = prog.compiled_lp_train(torch.bfloat16, False, False)
    assert c2 is not c, "the mode of every BatchNorm layer is part of the key"
    n_eval = int(np.sum((c2.fwd.arr["kind"] == un.OP_BN_RELU) & ((c2.fwd.arr["flags"] & un.F_TRAINING) == 0)))
    assert n_eval == 1
    model.train()
    assert prog.compiled_lp_train(torch.bfloat16, False, False) is c


def _op(kind, flags, M=1000, K=27, Cin=64, Cout=64, dtype=0, inp=(), out=()):
    a = np.zeros(1, dtype=un.OP_DTYPE)
    a["kind"], a["flags"], a["M_in"], a["M_out"] = kind, flags, M, M
    a["K"], a["Cin"], a["Cout"], a["reserved"] = K, Cin, Cout, dtype
    a["eps"] = 1e-4
    fake = 1 << 40
    a["inp"][0, :len(inp)] = [fake + 4096 * i if i else 0 for i in inp]             # (0: a NULL slot)
    a["out"][0, :len(out)] = [fake + (1 << 30) + 4096 * i if i else 0 for i in out]
    return a


LP, F32, TR = un.F_LP | un.F_LP_TRAIN, un.F_OUT_F32, un.F_TRAINING      # (LP: a flagged op of a TRAINING pass)
INFER = un.F_LP                                                          # the flag of an inference list alone
VALID = {
    "bn_training": _op(un.OP_BN_RELU, LP | TR, inp=(1, 2, 3, 4, 5), out=(1, 2, 3)),
    "bn_training_update_f32": _op(un.OP_BN_RELU, LP | TR | un.F_UPDATE | F32 | un.F_RELU, dtype=1, inp=(1, 2, 3, 4, 5), out=(1, 2, 3)),
    "bn_training_no_running": _op(un.OP_BN_RELU, LP | TR, inp=(1, 2, 3), out=(1, 2, 3)),
    "conv_bwd": _op(un.OP_CONV_BWD, LP, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "conv_bwd_flip_fp16": _op(un.OP_CONV_BWD, LP | un.F_FLIP, K=8, Cin=96, Cout=160, dtype=1, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "conv_bwd_no_din": _op(un.OP_CONV_BWD, LP, inp=(1, 2, 3, 4, 5, 6, 7), out=(0, 2)),
    "conv_bwd_frozen": _op(un.OP_CONV_BWD, LP, inp=(1, 2, 3, 4, 5, 6, 7), out=(1,)),
    "bn_bwd": _op(un.OP_BN_RELU_BWD, LP | TR, inp=(1, 2, 3, 4, 5, 6), out=(1, 2, 3)),
    "bn_bwd_f32_addend": _op(un.OP_BN_RELU_BWD, LP | TR | F32 | un.F_RELU, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2, 3)),
    "bn_bwd_no_dx": _op(un.OP_BN_RELU_BWD, LP, inp=(1, 2, 3, 4), out=(0, 2, 3)),
    "split": _op(un.OP_SPLIT, LP, Cin=32, Cout=32, inp=(1,), out=(1, 2)),
    # the ops both kinds of pass have may carry the training flag
    "conv_fwd": _op(un.OP_CONV, LP, inp=(1, 2, 3, 4, 0, 6), out=(1,)),
    "bn_eval": _op(un.OP_BN_RELU, LP | un.F_RELU, inp=(1, 2, 3, 4, 5), out=(1,)),
    "cat": _op(un.OP_CAT, LP, Cin=32, Cout=32, inp=(1, 2), out=(1,)),
}
REFUSED = {
    "bn_training_stats": _op(un.OP_BN_RELU, LP | TR | un.F_STATS, inp=(1, 2, 3, 4, 5, 6), out=(1, 2, 3)),
    "bn_training_no_mean": _op(un.OP_BN_RELU, LP | TR, inp=(1, 2, 3, 4, 5), out=(1,)),
    "bn_training_c4": _op(un.OP_BN_RELU, LP | TR, Cin=36, inp=(1, 2, 3, 4, 5), out=(1, 2, 3)),
    "bn_update_no_running": _op(un.OP_BN_RELU, LP | TR | un.F_UPDATE, inp=(1, 2, 3), out=(1, 2, 3)),
    "bn_bwd_stats": _op(un.OP_BN_RELU_BWD, LP | TR | un.F_STATS, inp=(1, 2, 3, 4, 5, 6, 0, 8), out=(1, 2, 3)),
    "bn_bwd_no_dgamma": _op(un.OP_BN_RELU_BWD, LP | TR, inp=(1, 2, 3, 4, 5, 6), out=(1,)),
    "conv_bwd_stats": _op(un.OP_CONV_BWD, LP | un.F_STATS, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "conv_bwd_bn_in": _op(un.OP_CONV_BWD, LP | un.F_BN_IN, inp=(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11), out=(1, 2)),
    "conv_bwd_input_channels": _op(un.OP_CONV_BWD, LP, Cin=6, Cout=32, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "conv_bwd_wide": _op(un.OP_CONV_BWD, LP, Cin=32, Cout=544, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "conv_bwd_2gib_dy": _op(un.OP_CONV_BWD, LP, M=1 << 25, inp=(1, 2, 3, 4, 5, 6, 7), out=(0, 2)),
    "conv_bwd_no_weight": _op(un.OP_CONV_BWD, LP, inp=(1, 0, 3, 4, 5, 6, 7), out=(1, 2)),
    "split_odd": _op(un.OP_SPLIT, LP, Cin=33, Cout=31, inp=(1,), out=(1, 2)),
    "add": _op(un.OP_ADD, LP, inp=(1,), out=(1,)),
    # the forms of a training pass in a list that was not recorded as one, and the training flag on its own
    "bn_training_infer": _op(un.OP_BN_RELU, INFER | TR | un.F_UPDATE, inp=(1, 2, 3, 4, 5), out=(1, 2, 3)),
    "conv_bwd_infer": _op(un.OP_CONV_BWD, INFER | un.F_FLIP, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "bn_bwd_infer": _op(un.OP_BN_RELU_BWD, INFER | TR, inp=(1, 2, 3, 4, 5, 6), out=(1, 2, 3)),
    "split_infer": _op(un.OP_SPLIT, INFER, Cin=32, Cout=32, inp=(1,), out=(1, 2)),
    "train_flag_alone": _op(un.OP_CONV_BWD, un.F_LP_TRAIN, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_executor_sizes_16bit_training_ops(name):
    op = VALID[name]
    lib = wsis_native.hip()
    wsb = lib.wsis_run_ops_workspace_bytes(op.ctypes.data, 1)
    assert wsb > 0, lib.wsis_last_error().decode()
    if op["kind"][0] == un.OP_CONV_BWD:
        K, Cin, Cout, Mr = (int(op[f][0]) for f in ("K", "Cin", "Cout", "M_out"))
        need = 0
        if op["out"][0][0]:      # the rounded weight of the dIn product
            need += K * Cin * Cout * 2
        if op["out"][0][1]:      # the slabs of the weight gradient
            need += lib.wsis_spconv_dw_lp_workspace_bytes(Mr, K, Cin, Cout)
        assert wsb >= need
    if op["kind"][0] == un.OP_BN_RELU_BWD or (op["kind"][0] == un.OP_BN_RELU and op["flags"][0] & TR):      # a reduction
        assert wsb >= lib.wsis_bn_workspace_bytes(int(op["M_in"][0]), int(op["Cin"][0]))


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_executor_refuses_16bit_training_ops_it_cannot_run(name):
    lib = wsis_native.hip()
    op = REFUSED[name]
    assert lib.wsis_run_ops_workspace_bytes(op.ctypes.data, 1) == -1
    assert lib.wsis_run_ops(op.ctypes.data, 1, None, 0, None, None) != 0
    assert "op 0" in lib.wsis_last_error().decode()
    two = np.concatenate([VALID["bn_bwd"], op])
    assert lib.wsis_run_ops_workspace_bytes(two.ctypes.data, 2) == -1


def test_unflagged_backward_ops_unchanged_by_the_16bit_forms():
    lib = wsis_native.hip()
    plain = _op(un.OP_CONV_BWD, un.F_FLIP, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2))
    lp = _op(un.OP_CONV_BWD, LP | un.F_FLIP, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2))
    assert lib.wsis_run_ops_workspace_bytes(lp.ctypes.data, 1) > 0
    a = lib.wsis_run_ops_workspace_bytes(plain.ctypes.data, 1)
    b = lib.wsis_run_ops_workspace_bytes(np.concatenate([plain, lp]).ctypes.data, 2)
    assert a > 0 and b >= a + 27 * 64 * 64 * 2
    layout = np.zeros(11 + 4, dtype=np.int64)
    fn = lib.wsis_debug_run_ops_layout      # (diagnostic entry point: not in the bound table)
    fn.restype, fn.argtypes = ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    both = np.concatenate([plain, lp])
    assert fn(both.ctypes.data, 2, layout.ctypes.data) == 0
    assert layout[11] == -1 and layout[12] == 0, "16-bit weights for the flagged op only"


def test_entry_point_refusals():
    lib = wsis_native.hip()
    p = ctypes.c_void_p(1 << 40)
    q = ctypes.c_void_p((1 << 40) + 8)
    wsb = lib.wsis_bn_workspace_bytes(100, 64)

    def stats(M=100, C=64, dtype=0, ws=wsb, x=p, rm=p, rv=p):
        return lib.wsis_bn_stats_lp(x, M, C, p, p, rm, rv, 0.1, p, ws, dtype, None)
    for bad in (dict(dtype=2), dict(C=36), dict(C=1032), dict(M=0), dict(ws=wsb - 1), dict(x=None), dict(x=q), dict(rv=None)):
        assert stats(**bad) != 0, bad

    def bwd(M=100, C=64, dtype=0, ws=wsb, x=p, dy=p, dx=p, dg=p, addend=None):
        return lib.wsis_bn_bwd_lp(x, dy, p, p, p, p, 1e-4, 1, 1, dx, 0, dg, p, addend, M, C, dtype, p, ws, None)
    for bad in (dict(dtype=-1), dict(C=4), dict(M=0), dict(ws=0), dict(dy=None), dict(dg=None), dict(dx=q), dict(addend=q)):
        assert bwd(**bad) != 0, bad
