"""CPU: the synced form of the 16-bit native training pass without a GPU -- the dispatch rule with its second switch
(WSIS_NATIVE_LP_SYNC=1 lets a SyncBatchNorm group through), and the refusals of the entry points it adds
(wsis_bn_bwd_apply_lp, wsis_bn_sync_*): every one happens before anything touches the device."""
import ctypes

import torch

import unet_native as un
import wsis_native

DT = (torch.bfloat16, torch.float16)
ON = {"WSIS_NATIVE_LP_TRAIN": "1"}
SYNC = dict(ON, WSIS_NATIVE_LP_SYNC="1")


def test_the_second_switch_lets_a_group_through():
    for dt in DT:
        assert un.lp_train_pass_wanted(SYNC, dt, True, True, True, True, True)
        assert un.lp_train_pass_wanted(SYNC, dt, True, True, True, True, False), "no group: the pass as before"
        assert not un.lp_train_pass_wanted(ON, dt, True, True, True, True, True), "switch absent: a group refuses"
        assert not un.lp_train_pass_wanted(dict(ON, WSIS_NATIVE_LP_SYNC="0"), dt, True, True, True, True, True)
    bf = torch.bfloat16
    assert not un.lp_train_pass_wanted({"WSIS_NATIVE_LP_SYNC": "1"}, bf, True, True, True, True, True), "the new switch alone"
    assert not un.lp_train_pass_wanted(dict(SYNC, WSIS_NATIVE_LP_TRAIN="0"), bf, True, True, True, True, True)
    assert not un.lp_train_pass_wanted(dict(SYNC, WSIS_NATIVE_UNET="0"), bf, True, True, True, True, True)
    for cd in (None, torch.float32):
        assert not un.lp_train_pass_wanted(SYNC, cd, True, True, True, True, True)
    assert not un.lp_train_pass_wanted(SYNC, bf, False, True, True, True, True), "no_grad"
    assert not un.lp_train_pass_wanted(SYNC, bf, True, False, True, True, True), "16-bit parameters"
    assert not un.lp_train_pass_wanted(SYNC, bf, True, True, False, True, True), "an evaluation-mode BatchNorm"
    assert not un.lp_train_pass_wanted(SYNC, bf, True, True, True, False, True), "a product outside the domain"


def test_checks_stay_lazy_with_the_second_switch():
    calls = []

    def check(name, value):
        return lambda: calls.append(name) or value
    assert not un.lp_train_pass_wanted(SYNC, None, True, check("p", True), check("b", True), check("d", True), check("s", True))
    assert calls == [], "a failed cheap condition: no model check runs"
    assert un.lp_train_pass_wanted(SYNC, torch.float16, True, check("p", True), check("b", True), check("d", True), check("s", True))
    assert calls == ["p", "b", "d"], "with the switch the group is not asked for; the model checks keep their order"
    calls.clear()
    assert not un.lp_train_pass_wanted(SYNC, torch.float16, True, check("p", True), check("b", False), check("d", True),
                                       check("s", True))
    assert calls == ["p", "b"], "the first failing check ends it"


def test_run_function_takes_a_group():
    import inspect
    sig = inspect.signature(un.run_unet_lp_train)
    assert list(sig.parameters)[-1] == "sync_group" and sig.parameters["sync_group"].default is None


def test_entry_point_refusals():
    lib = wsis_native.hip()
    p = ctypes.c_void_p(1 << 40)
    q = ctypes.c_void_p((1 << 40) + 8)

    def apply(M=100, C=64, dtype=0, x=p, dy=p, s1=p, s2=p, dx=p, addend=None, mean=p):
        return lib.wsis_bn_bwd_apply_lp(x, dy, mean, p, p, p, s1, s2, 1e-4, 1, dx, 0, addend, M, C, dtype, None)
    for bad in (dict(dx=None), dict(dtype=2), dict(dtype=-1), dict(C=36), dict(C=4), dict(C=1032), dict(M=0), dict(x=None),
                dict(dy=None), dict(s1=None), dict(s2=None), dict(mean=None), dict(dx=q), dict(x=q), dict(addend=q)):
        assert apply(**bad) != 0, bad
        assert wsis_native.hip().wsis_last_error(), bad

    def pack(M=100, C=64, mean=p, var=p, out=p):
        return lib.wsis_bn_sync_pack(mean, var, M, C, out, None)
    for bad in (dict(out=None), dict(C=0), dict(M=-1), dict(mean=None), dict(var=None)):
        assert pack(**bad) != 0, bad

    def combine(R=2, C=64, g=p, mean=p, var=p, rm=p, rv=p, count=p):
        return lib.wsis_bn_sync_combine(g, R, C, mean, var, rm, rv, 0.1, count, None)
    for bad in (dict(R=0), dict(R=-1), dict(C=0), dict(g=None), dict(mean=None), dict(var=None), dict(count=None),
                dict(rv=None), dict(rm=None)):
        assert combine(**bad) != 0, bad

    def sums_pack(C=64, out=p):
        return lib.wsis_bn_sync_sums_pack(p, p, C, out, None)
    for bad in (dict(out=None), dict(C=0)):
        assert sums_pack(**bad) != 0, bad

    def sums_scale(M=100, C=64, sums=p, count=p, a=p, b=p):
        return lib.wsis_bn_sync_sums_scale(sums, M, count, C, a, b, None)
    for bad in (dict(a=None), dict(b=None), dict(sums=None), dict(count=None), dict(C=0), dict(M=-1)):
        assert sums_scale(**bad) != 0, bad
