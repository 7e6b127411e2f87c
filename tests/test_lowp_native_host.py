"""CPU: the 16-bit evaluation-mode native UNet pass without a GPU -- the dispatch rule of Network.forward as a pure function,
the dtype the pass returns, the op list UNetProgram records for it, and the executor's refusals and workspace queries for
16-bit ops (host-only: every refusal happens before anything touches the device)."""
import ctypes

import numpy as np
import pytest
import torch

import harness
import unet_native as un
import wsis_native

DT = (torch.bfloat16, torch.float16)
ON = {"WSIS_NATIVE_LP": "1"}


def test_predicate_needs_every_condition():
    for dt in DT:
        assert un.lp_pass_wanted(ON, dt, False, True, True, True)
    assert not un.lp_pass_wanted({}, torch.bfloat16, False, True, True, True), "the switch defaults to off"
    assert not un.lp_pass_wanted({"WSIS_NATIVE_LP": "0"}, torch.bfloat16, False, True, True, True)
    assert not un.lp_pass_wanted(dict(ON, WSIS_NATIVE_UNET="0"), torch.bfloat16, False, True, True, True)
    assert un.lp_pass_wanted(dict(ON, WSIS_NATIVE_UNET="1"), torch.bfloat16, False, True, True, True)
    for cd in (None, torch.float32, torch.float64):
        assert not un.lp_pass_wanted(ON, cd, False, True, True, True)
    assert not un.lp_pass_wanted(ON, torch.bfloat16, True, True, True, True), "gradients need the training pass"
    assert not un.lp_pass_wanted(ON, torch.bfloat16, False, False, True, True), "16-bit (or misplaced) parameters"
    assert not un.lp_pass_wanted(ON, torch.bfloat16, False, True, False, True), "training-mode BatchNorm"
    assert not un.lp_pass_wanted(ON, torch.float16, False, True, True, False), "a product outside the 16-bit domain"


def test_predicate_runs_the_model_checks_last_and_lazily():
    calls = []

    def check(name, value):
        return lambda: calls.append(name) or value
    # a training forward (gradients on), fp32 features, the switch off: no model check runs
    for args in (({}, torch.bfloat16, False), (ON, None, False), (ON, torch.bfloat16, True)):
        assert not un.lp_pass_wanted(*args, check("p", True), check("b", True), check("d", True))
    assert calls == []
    assert un.lp_pass_wanted(ON, torch.bfloat16, False, check("p", True), check("b", True), check("d", True))
    assert calls == ["p", "b", "d"]
    calls.clear()
    assert not un.lp_pass_wanted(ON, torch.bfloat16, False, check("p", False), check("b", True), check("d", True))
    assert calls == ["p"], "the first failing check ends it"


def test_output_dtype_follows_the_walk_rule(monkeypatch):
    # the walk's output layer is a torch BatchNorm1d on 16-bit input: it keeps that dtype unless autocast casts batch_norm
    casts = torch._C._dispatch_has_kernel_for_dispatch_key("aten::batch_norm", "AutocastCUDA")
    for dt in DT:
        assert un.lp_out_dtype(dt, False) == dt
        assert un.lp_out_dtype(dt, True) == (torch.float32 if casts else dt)
    # a torch without the dispatcher query, or one whose query fails: the documented lists (no batch_norm)
    monkeypatch.delattr(torch._C, "_dispatch_has_kernel_for_dispatch_key")
    assert un.lp_out_dtype(torch.bfloat16, True) == torch.bfloat16

    def broken(*a):
        raise RuntimeError("no such dispatch key")
    monkeypatch.setattr(torch._C, "_dispatch_has_kernel_for_dispatch_key", broken, raising=False)
    assert un.lp_out_dtype(torch.float16, True) == torch.float16


def _model():
    cfg = harness.default_cfg()
    model, _, _ = harness.build_model(cfg, "cpu")
    return model.eval()


def test_bn_eval_and_domain_of_the_model():
    model = _model()
    assert un.lp_bn_eval(model)
    assert un.lp_in_domain(model, 778_000)
    assert not un.lp_in_domain(model, 1 << 25), "2 GiB gathered tensors are outside the 16-bit kernels"
    model.unet.blocks.block0.conv_branch[0].train()
    assert not un.lp_bn_eval(model)
    model.eval()
    model.output_layer[0].track_running_stats = False
    assert not un.lp_bn_eval(model)


def test_params_fp32_of_the_model():
    model = _model()
    assert un.lp_params_fp32(model, "cpu")
    assert not un.lp_params_fp32(model, "cuda"), "parameters on another device"
    m16 = _model().to(torch.bfloat16)
    assert not un.lp_params_fp32(m16, "cpu"), "a model converted to bf16"
    with pytest.raises(ValueError):
        un.UNetProgram(m16).compiled_lp(torch.bfloat16, False)
    for what in ("weight", "running_var", "gamma", "strided"):
        m = _model()
        if what == "weight":
            conv = m.unet.u.blocks.block1.conv_branch[2]
            conv.weight.data = conv.weight.data.half()
        elif what == "running_var":
            bn = m.output_layer[0]
            bn.running_var = bn.running_var.to(torch.bfloat16)
        elif what == "gamma":
            bn = m.unet.blocks.block0.conv_branch[0]
            bn.weight.data = bn.weight.data.to(torch.float16)
        else:
            conv = m.input_conv[0]
            conv.weight.data = conv.weight.data.transpose(3, 4).contiguous().transpose(3, 4)
            assert not conv.weight.is_contiguous()
        assert not un.lp_params_fp32(m, "cpu"), what


def _instantiate(c, M=(5000, 1200, 300, 80, 20)):
    """the template with fake (never dereferenced) device addresses: enough for the host-side queries"""
    Mvec = np.asarray(M, dtype=np.int64)
    offs, _ = c.fwd_arena.layout(Mvec)
    fake = np.uint64(1 << 40)
    luts = {un._FWD: offs.astype(np.uint64) + fake, un._TBL: np.arange(1, 31, dtype=np.uint64) * np.uint64(4096) + fake,
            un._EXT: np.array([fake, fake + np.uint64(1 << 30)], dtype=np.uint64),
            un._BWD: np.zeros(0, np.uint64), un._PAR: np.zeros(0, np.uint64)}
    return c.fwd.instantiate(Mvec, luts), Mvec


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp16"])
def test_recorded_program(dt, out_f32):
    model = _model()
    prog = un.UNetProgram(model)
    c = prog.compiled_lp(dt, out_f32)
    assert prog.compiled_lp(dt, out_f32) is c, "cached per (model, dtype, output dtype)"
    assert prog.compiled_lp(dt, not out_f32) is not c
    ops, Mvec = _instantiate(c)
    kinds, flags = ops["kind"], ops["flags"]
    # input conv (fp32 op), its rounding, then 16-bit ops only
    assert kinds[0] == un.OP_CONV and flags[0] == 0 and ops["Cin"][0] == 6
    assert kinds[1] == un.OP_CAST_LP
    assert np.all(flags[1:] & un.F_LP)
    assert np.all(ops["reserved"][1:] == (0 if dt == torch.bfloat16 else 1)) and ops["reserved"][0] == 0
    assert not np.any(np.isin(kinds, (un.OP_CONV_BWD, un.OP_BN_RELU_BWD, un.OP_SPLIT, un.OP_ADD)))
    assert not np.any(flags & (un.F_TRAINING | un.F_UPDATE | un.F_STATS | un.F_BN_IN | un.F_STAT_FIN))
    n_conv = sum(1 for m in model.unet.modules() if hasattr(m, "kernel_size") and hasattr(m, "subm"))
    assert int(np.sum(kinds == un.OP_CONV)) == n_conv + 1
    assert int(np.sum(kinds == un.OP_CAT)) == model.blocks - 1
    n_bn = sum(1 for m in list(model.unet.modules()) + list(model.output_layer.modules())
               if isinstance(m, torch.nn.BatchNorm1d))
    assert int(np.sum(kinds == un.OP_BN_RELU)) == n_bn
    # the output layer writes the caller's tensor (external slot 1), fp32 only when asked
    assert kinds[-1] == un.OP_BN_RELU and ops["out"][-1][0] == int(np.uint64(1 << 40) + np.uint64(1 << 30))
    assert bool(flags[-1] & un.F_OUT_F32) == out_f32
    assert int(np.sum((flags & un.F_OUT_F32) != 0)) == (1 if out_f32 else 0)
    # residual blocks: the second 3x3x3 convolution of each block carries its skip path
    from sparse_unet3d import ResidualBlock
    n_res = sum(1 for m in model.unet.modules() if isinstance(m, ResidualBlock))
    assert int(np.sum((kinds == un.OP_CONV) & (ops["inp"][:, 5] != 0))) == n_res == 18
    lib = wsis_native.hip()
    wsb = lib.wsis_run_ops_workspace_bytes(ops.ctypes.data, len(ops))
    wt = sum(int(o["K"]) * int(o["Cin"]) * int(o["Cout"]) * 2 for o in ops if o["kind"] == un.OP_CONV and o["flags"])
    assert wsb >= wt > 0, (wsb, wt)


def _op(kind, flags, M=1000, K=27, Cin=64, Cout=64, dtype=0, inp=(), out=()):
    a = np.zeros(1, dtype=un.OP_DTYPE)
    a["kind"], a["flags"], a["M_in"], a["M_out"] = kind, flags, M, M
    a["K"], a["Cin"], a["Cout"], a["reserved"] = K, Cin, Cout, dtype
    a["eps"] = 1e-4
    fake = 1 << 40
    a["inp"][0, :len(inp)] = [fake + 4096 * i for i in inp]
    a["out"][0, :len(out)] = [fake + (1 << 30) + 4096 * i for i in out]
    return a


LP, F32 = un.F_LP, un.F_OUT_F32
VALID = {
    "conv": _op(un.OP_CONV, LP, inp=(1, 2, 3, 4, 0, 6), out=(1,)),
    "conv_flip_fp16": _op(un.OP_CONV, LP | un.F_FLIP, K=8, Cin=96, Cout=160, dtype=1, inp=(1, 2, 3, 4), out=(1,)),
    "conv_dense": _op(un.OP_CONV, LP, K=1, Cin=128, Cout=64, inp=(1, 0, 0, 4), out=(1,)),
    "bn": _op(un.OP_BN_RELU, LP | un.F_RELU, inp=(1, 2, 3, 4, 5), out=(1,)),
    "bn_f32": _op(un.OP_BN_RELU, LP | F32, inp=(1, 0, 0, 4, 5), out=(1,)),
    "cat": _op(un.OP_CAT, LP, Cin=32, Cout=32, inp=(1, 2), out=(1,)),
    "cast": _op(un.OP_CAST_LP, LP, Cin=32, inp=(1,), out=(1,)),
}
REFUSED = {
    "bn_training": _op(un.OP_BN_RELU, LP | un.F_TRAINING, inp=(1, 2, 3, 4, 5), out=(1, 2, 3)),
    "bn_update": _op(un.OP_BN_RELU, LP | un.F_UPDATE, inp=(1, 2, 3, 4, 5), out=(1,)),
    "bn_no_running": _op(un.OP_BN_RELU, LP, inp=(1, 2, 3), out=(1,)),
    "conv_bwd": _op(un.OP_CONV_BWD, LP, inp=(1, 2, 3, 4, 5, 6, 7), out=(1, 2)),
    "bn_bwd": _op(un.OP_BN_RELU_BWD, LP | un.F_TRAINING, inp=(1, 2, 3, 4, 5, 6), out=(1, 2, 3)),
    "conv_input_channels": _op(un.OP_CONV, LP, Cin=6, Cout=32, inp=(1, 2, 3, 4), out=(1,)),
    "conv_wide": _op(un.OP_CONV, LP, Cin=544, Cout=32, inp=(1, 2, 3, 4), out=(1,)),
    "conv_2gib": _op(un.OP_CONV, LP, M=1 << 25, Cin=64, inp=(1, 2, 3, 4), out=(1,)),
    "conv_stats": _op(un.OP_CONV, LP | un.F_STATS, inp=(1, 2, 3, 4), out=(1, 2)),
    "conv_bn_in": _op(un.OP_CONV, LP | un.F_BN_IN, inp=(1, 2, 3, 4), out=(1,)),
    "conv_no_weight": _op(un.OP_CONV, LP, inp=(1, 2, 3), out=(1,)),
    "cat_odd": _op(un.OP_CAT, LP, Cin=33, Cout=31, inp=(1, 2), out=(1,)),
    "split": _op(un.OP_SPLIT, LP, Cin=32, Cout=32, inp=(1,), out=(1, 2)),
    "dtype2": _op(un.OP_BN_RELU, LP, dtype=2, inp=(1, 2, 3, 4, 5), out=(1,)),
    "cast_unflagged": _op(un.OP_CAST_LP, 0, Cin=32, inp=(1,), out=(1,)),
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_executor_sizes_valid_16bit_ops(name):
    op = VALID[name]
    wsb = wsis_native.hip().wsis_run_ops_workspace_bytes(op.ctypes.data, 1)
    assert wsb > 0
    if op["kind"][0] == un.OP_CONV:       # the op's 16-bit weights live in the call's workspace
        assert wsb >= int(op["K"][0]) * int(op["Cin"][0]) * int(op["Cout"][0]) * 2


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_executor_refuses_16bit_ops_it_cannot_run(name):
    lib = wsis_native.hip()
    op = REFUSED[name]
    assert lib.wsis_run_ops_workspace_bytes(op.ctypes.data, 1) == -1
    # the call itself fails before it looks at the workspace or the stream
    assert lib.wsis_run_ops(op.ctypes.data, 1, None, 0, None, None) != 0
    msg = lib.wsis_last_error().decode()
    assert "op 0" in msg, msg
    # an unflagged list around it is not enough: one refused op refuses the call
    two = np.concatenate([VALID["bn"], op])
    assert lib.wsis_run_ops_workspace_bytes(two.ctypes.data, 2) == -1


def test_unflagged_ops_unchanged_by_the_16bit_region():
    lib = wsis_native.hip()
    plain = _op(un.OP_CONV, 0, inp=(1, 2, 3, 4), out=(1,))
    lp = _op(un.OP_CONV, LP, inp=(1, 2, 3, 4), out=(1,))
    a = lib.wsis_run_ops_workspace_bytes(plain.ctypes.data, 1)
    b = lib.wsis_run_ops_workspace_bytes(np.concatenate([plain, lp]).ctypes.data, 2)
    assert a > 0 and b >= a + 27 * 64 * 64 * 2


def test_entry_point_refusals():
    lib = wsis_native.hip()
    p = ctypes.c_void_p(1 << 40)
    # wsis_spconv_fwd_lp_res: dtype, channel domain, null pointers -- refused before any launch
    args = dict(M_in=100, M_out=100, K=27, Cin=64, Cout=64, dtype=0)

    def fwd(**kw):
        a = dict(args, **kw)
        return lib.wsis_spconv_fwd_lp_res(p, p, None, p, 0, None, p, kw.get("out", p), a["M_in"], a["M_out"], a["K"],
                                          a["Cin"], a["Cout"], a["dtype"], None, 256, None)
    assert fwd(dtype=2) != 0
    assert fwd(Cin=6) != 0
    assert fwd(Cout=48) != 0
    assert fwd(out=None) != 0
    assert fwd(M_in=-1) != 0
    assert fwd(M_out=0) == 0, "no rows: nothing to do"

    def bn(**kw):
        a = dict(M=100, C=64, dtype=0, x=p, y=p, mean=p)
        a.update(kw)
        return lib.wsis_bn_apply_lp(a["x"], a["mean"], p, None, None, 1e-4, 1, a["y"], 0, a["M"], a["C"], a["dtype"],
                                    None)
    assert bn(dtype=2) != 0
    assert bn(C=0) != 0
    assert bn(M=-1) != 0
    assert bn(x=None) != 0
    assert bn(mean=None) != 0
    assert bn(y=ctypes.c_void_p((1 << 40) + 2)) != 0, "a 16-bit quad needs 8-byte alignment"
    assert bn(M=0, x=None, y=None) == 0, "no rows: nothing to do"
