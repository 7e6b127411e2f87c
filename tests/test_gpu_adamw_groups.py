"""GPU: FlatAdamW with several parameter groups in the step's one launch (wsis_adamw_step_groups,
wsis_adamw_step_scaled_groups).

Parameters of 1, 3, 4, 5, 1023, 1024, 1025 and 2051 elements: the tail loop, one float4, a float4 and a tail, the chunk
edge from both sides and a third chunk with a tail.  The gradient of the 2051 tensor is a view that starts one element
into a larger buffer, so all three of its chunks take the scalar path.  GROUPS: four group dicts -- three with parameters
and an empty one (its only tensor needs no gradient) between two of them; different lr (one 0), betas, eps; one
weight_decay 0; one group of a single one-element parameter.

1. against torch.optim.AdamW with the same groups and a LambdaLR with one lambda per group, six steps
2. three groups with equal hyper-parameters against the one-group optimizer: byte-equal, plain and through LossScaler
3. LossScaler and torch.amp.GradScaler drive the grouped optimizer alike; an overflow step leaves every byte; no read-back
4. the gradient clamp inside one group
5. add_param_group after two steps, straight behind a step
6. checkpoints in both directions with torch.optim.AdamW
7. unsupported flags

Bounds of 1., 5., 6.: the project's own of the one-group comparison (test_gpu_loss_scale: 2e-6 * max|ref| + 1e-9 for
parameters, 1e-6 * max|ref| + 1e-30 for moments)."""
import pytest
import torch

import wsis_optim as optim

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUMEL = [1023, 4, 2051, 1, 3, 5, 1024, 1025]
VIEW = 2                                                  # the parameter whose gradient is the unaligned view
LAGS = 1                                                  # the parameter without a gradient in steps 2 and 3
SPLIT = [(0, 3), None, (3, 4), (4, 8)]                    # None: the empty group
HYPER = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
         dict(lr=7e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-3),
         dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
         dict(lr=0.0, betas=(0.95, 0.98), eps=1e-7, weight_decay=5e-2)]
LAMBDAS = [lambda e: 1.0 / (1 + e), lambda e: 1.0, lambda e: 0.5 ** e, lambda e: 1.0 + e]
STEPS = 6                                                 # past the ring of 4 table slots
INF, NAN = float("inf"), float("nan")


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _close(p, q, what):
    err, ref = float((p.detach() - q.detach()).abs().max()), float(q.detach().abs().max())
    assert err <= 2e-6 * ref + 1e-9, (what, err, ref)


def _params(seed, numel=NUMEL):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).cuda().requires_grad_(True) for n in numel], g


def _clones(params):
    return [t.detach().clone().requires_grad_(True) for t in params]


def _groups(params, hyper=HYPER, split=SPLIT):
    """group dicts for either optimizer; the empty group holds one tensor that needs no gradient (FlatAdamW drops it,
    torch gets the group without it)"""
    return [dict(h, params=[torch.zeros(2, device=DEV)] if s is None else params[s[0]:s[1]]) for h, s in zip(hyper, split)]


def _torch_adamw(params, hyper=HYPER, split=SPLIT):
    groups = _groups(params, hyper, split)
    for grp in groups:
        grp["params"] = [p for p in grp["params"] if p.requires_grad]
    return torch.optim.AdamW(groups, foreach=False, fused=False)


def _script(g, steps=STEPS, numel=NUMEL, scale=1.0):
    """gradients of every step (None: no gradient), magnitudes spread over the tensors"""
    return [[None if (i == LAGS and step in (2, 3)) else torch.randn(n, generator=g).cuda() * (scale * 10.0 ** (i % 4 - 2))
             for i, n in enumerate(numel)] for step in range(steps)]


def _set_grads(params, values, flat=None):
    """values[i] None: no gradient; parameter VIEW gets a view one element into ``flat``, the others own allocations"""
    for i, (p, v) in enumerate(zip(params, values)):
        if v is None:
            p.grad = None
        elif i == VIEW and flat is not None:
            view = flat[1:1 + p.numel()]
            view.copy_(v)
            assert view.data_ptr() % 16 == 4
            p.grad = view
        else:
            p.grad = v.clone()


def _moments_match(mine, ref, n):
    sd, rs = mine.state_dict(), ref.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in rs["param_groups"]]
    assert sorted(sd["state"]) == sorted(rs["state"]) == list(range(n))
    for i in range(n):
        assert float(sd["state"][i]["step"]) == float(rs["state"][i]["step"]), i
        for name in ("exp_avg", "exp_avg_sq"):
            want = rs["state"][i][name]
            err = float((sd["state"][i][name] - want).abs().max())
            assert err <= 1e-6 * float(want.abs().max()) + 1e-30, (i, name, err)
    return sd


# ---- 1. against torch ------------------------------------------------------------------------------------------------

def test_grouped_step_matches_torch_adamw_with_the_same_groups():
    a, g = _params(3)
    b = _clones(a)
    mine, ref = optim.FlatAdamW(_groups(a)), _torch_adamw(b)
    assert len(mine.param_groups) == 4 and [len(grp["params"]) for grp in mine.param_groups] == [3, 0, 1, 4]
    assert all(x is y for x, y in zip(mine.params, a)) and len(mine.params) == 8
    assert (mine.lr, mine.betas, mine.eps, mine.weight_decay) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)      # views of group 0
    s_mine = torch.optim.lr_scheduler.LambdaLR(mine, LAMBDAS)
    s_ref = torch.optim.lr_scheduler.LambdaLR(ref, LAMBDAS)
    start = _clones(a)
    flat = torch.zeros(NUMEL[VIEW] + 3, device=DEV)
    for step, values in enumerate(_script(g)):
        _set_grads(a, values, flat)
        _set_grads(b, values)
        mine.step()
        ref.step()
        s_mine.step()
        s_ref.step()
        assert [grp["lr"] for grp in mine.param_groups] == [grp["lr"] for grp in ref.param_groups]
        for i, (p, q) in enumerate(zip(a, b)):
            _close(p, q, (step, i))
    assert mine._skipped is None and mine.steps.tolist() == [6, 4, 6, 6, 6, 6, 6, 6]
    sd = _moments_match(mine, ref, len(a))
    assert [grp["lr"] for grp in sd["param_groups"]] == [h["lr"] * lam(STEPS) for h, lam in zip(HYPER, LAMBDAS)]
    assert sd["param_groups"][0]["lr"] < 2e-4 and sd["param_groups"][1]["lr"] == 7e-4 and sd["param_groups"][3]["lr"] == 0.0
    # the lr = 0 group: decay = 1 - 0 * weight_decay = 1 and a zero step, so no byte moves while its moments advance
    for i in range(4, 8):
        assert _same(a[i], start[i]) and _same(b[i], start[i]), i
        assert float(sd["state"][i]["exp_avg"].abs().max()) > 0.0 and float(sd["state"][i]["exp_avg_sq"].abs().max()) > 0.0
    assert not any(_same(a[i], start[i]) for i in range(4))


# ---- 2. exactness against the one-group path -------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["plain", "loss_scaler"])
def test_equal_groups_give_the_bytes_of_the_one_group_step(path):
    """the double-then-round discipline of the new kernels: their constants and corrections are those the one-group
    entry points get from the host"""
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    a, g = _params(7)
    b = _clones(a)
    grouped = optim.FlatAdamW(_groups(a, [hyper] * 3, [(0, 3), (3, 4), (4, 8)]))
    single = optim.FlatAdamW(b, **hyper)
    assert len(grouped.param_groups) == 3 and len(single.param_groups) == 1
    for opt, params in ((grouped, a), (single, b)):
        assert opt.set_grad_clamp([params[LAGS], params[VIEW], params[7]], 0.5) == 3
    scalers = [optim.LossScaler(init_scale=2.0 ** 10) for _ in range(2)] if path == "loss_scaler" else None
    S = 2.0 ** 10 if scalers else 1.0
    flats = [torch.zeros(NUMEL[VIEW] + 3, device=DEV) for _ in range(2)]
    for step, values in enumerate(_script(g, scale=S)):
        if scalers and step == 4:
            values[6][1023] = INF                         # the overflow step: every parameter has a gradient, both skip
        for k, (opt, params) in enumerate(((grouped, a), (single, b))):
            _set_grads(params, values, flats[k])
            if scalers:
                scalers[k].step(opt)
                scalers[k].update()
            else:
                opt.step()
        for i, (p, q) in enumerate(zip(a, b)):
            assert _same(p, q), (path, step, i, "parameter")
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or _same(p.grad, q.grad)), (path, step, i, "gradient")
        assert _same(grouped.exp_avg, single.exp_avg) and _same(grouped.exp_avg_sq, single.exp_avg_sq), (path, step)
        if not (scalers and step == 4):                   # clamped (the UNSCALED value) and written back
            assert float(a[VIEW].grad.abs().max()) == 0.5 == float(a[7].grad.abs().max())
    if scalers:
        assert grouped._skipped.tolist() == single._skipped.tolist() == [1] * 8
        assert scalers[0].get_scale() == scalers[1].get_scale() == 2.0 ** 9
    else:
        assert grouped._skipped is None and single._skipped is None


# ---- 3. loss scaling with groups -------------------------------------------------------------------------------------

def _torch_scaler(**kw):
    scaler = torch.amp.GradScaler("cuda", **kw)
    scaler.scale(torch.zeros((), device=DEV))             # torch makes its scale tensor when a loss is first scaled
    return scaler


def test_loss_scaler_and_grad_scaler_drive_the_grouped_optimizer_alike():
    a, g = _params(11)
    c = _clones(a)
    mine, theirs = optim.FlatAdamW(_groups(a)), optim.FlatAdamW(_groups(c))
    s_mine, s_theirs = optim.LossScaler(init_scale=2.0 ** 10), _torch_scaler(init_scale=2.0 ** 10)
    script = _script(g, scale=2.0 ** 10)
    script[2][7][1024] = NAN          # step 2 overflows (the one-element second chunk) while parameter LAGS has no gradient
    flats = [torch.zeros(NUMEL[VIEW] + 3, device=DEV) for _ in range(2)]

    def snapshot(params, opt):
        return ([p.detach().clone() for p in params], [None if p.grad is None else p.grad.clone() for p in params],
                opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    before, after = [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()              # the mode does raise on a read-back under this torch
        for values in script:                             # nothing in here may read the device back: compared below
            for k, (params, opt, sc) in enumerate(((a, mine, s_mine), (c, theirs, s_theirs))):
                _set_grads(params, values, flats[k])
                before.append(snapshot(params, opt))
                sc.step(opt)
                sc.update()
                after.append(snapshot(params, opt))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for step in range(STEPS):
        (p0, g0, m0, v0), (p1, g1, m1, v1) = before[2 * step], after[2 * step]
        for i in range(8):
            assert _same(p1[i], after[2 * step + 1][0][i]), (step, i, "LossScaler and GradScaler part ways")
        if step == 2:                                     # every group skips: no byte of p, m, v, g changes
            for b4, af in ((before[4], after[4]), (before[5], after[5])):
                for i in range(8):
                    assert _same(af[0][i], b4[0][i]), (i, "parameter written on the skipped step")
                    assert (af[1][i] is None) == (b4[1][i] is None) and (b4[1][i] is None or _same(af[1][i], b4[1][i])), i
                assert _same(af[2], b4[2]) and _same(af[3], b4[3])
        else:
            assert not _same(p1[0], p0[0]) and not _same(p1[3], p0[3]) and not _same(m1, m0), (step, "no update")
    want = [0 if i == LAGS else 1 for i in range(8)]      # one skip for every parameter that had a gradient then
    assert mine._skipped.tolist() == want == theirs._skipped.tolist()
    assert mine.steps.tolist() == [6, 4, 6, 6, 6, 6, 6, 6]
    assert s_mine.get_scale() == 2.0 ** 9 == s_theirs.get_scale()
    steps = [float(mine.state_dict()["state"][i]["step"]) for i in range(8)]
    assert steps == [5.0, 4.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0]


def test_scaled_grouped_step_matches_torch_fed_the_unscaled_gradients():
    """the gradients of step 3 on carry half the scale the earlier ones carried: LossScaler halves after the overflow"""
    a, g = _params(13)
    b = _clones(a)
    mine, ref = optim.FlatAdamW(_groups(a)), _torch_adamw(b)
    scaler = optim.LossScaler(init_scale=2.0 ** 10)
    flat = torch.zeros(NUMEL[VIEW] + 3, device=DEV)
    S = 2.0 ** 10
    for step, values in enumerate(_script(g)):
        scaled = [None if v is None else v * S for v in values]
        if step == 2:
            scaled[VIEW][2050] = INF                      # the scalar path's last element
        _set_grads(a, scaled, flat)
        scaler.step(mine)
        scaler.update()
        if step == 2:
            S *= 0.5
        else:
            _set_grads(b, [None if v is None else v * (1.0 / S) for v in scaled])
            ref.step()
        for i, (p, q) in enumerate(zip(a, b)):
            _close(p, q, (step, i))
    _moments_match(mine, ref, len(a))


# ---- 4. clamp inside one group ---------------------------------------------------------------------------------------

def test_gradient_clamp_inside_one_group():
    a, g = _params(5)
    b = _clones(a)
    mine, ref = optim.FlatAdamW(_groups(a)), _torch_adamw(b)
    clamped = (0, VIEW)                                   # both in group 0: the float4 path and the scalar path
    assert mine.set_grad_clamp([a[i] for i in clamped], 1.0) == 2
    flat = torch.zeros(NUMEL[VIEW] + 3, device=DEV)
    values = [torch.randn(n, generator=g).cuda() * 3.0 for n in NUMEL]
    values[0][5], values[VIEW][2050] = NAN, NAN
    assert all(float(values[i][torch.isfinite(values[i])].abs().max()) > 1.0 for i in clamped)
    _set_grads(a, values, flat)
    _set_grads(b, [v.clamp(-1.0, 1.0) if i in clamped else v for i, v in enumerate(values)])
    mine.step()
    ref.step()
    for i, (p, q, v) in enumerate(zip(a, b, values)):
        if i in clamped:
            assert torch.equal(p.grad.nan_to_num(nan=7.0), v.clamp(-1.0, 1.0).nan_to_num(nan=7.0)), (i, "clamped and written back")
            assert bool(torch.isnan(p.grad).sum() == 1) and bool(torch.isnan(p.detach()).sum() == 1), (i, "NaN stays NaN")
            keep = torch.isfinite(v)
            _close(p[keep], q[keep], i)
        else:
            assert _same(p.grad, v), (i, "a gradient without a clamp is left alone")
            _close(p, q, i)


# ---- 5. add_param_group ----------------------------------------------------------------------------------------------

def test_add_param_group_after_two_steps():
    a, g = _params(17)
    b = _clones(a)
    hyper, split = [HYPER[0], HYPER[2]], [(0, 3), (3, 5)]
    mine, ref = optim.FlatAdamW(_groups(a[:5], hyper, split)), _torch_adamw(b[:5], hyper, split)
    assert mine.set_grad_clamp([a[VIEW]], 1.0) == 1
    flat = torch.zeros(NUMEL[VIEW] + 3, device=DEV)
    script = _script(g)

    def both(values, n):
        _set_grads(a[:n], values[:n], flat)
        _set_grads(b[:n], [v.clamp(-1.0, 1.0) if i == VIEW else v for i, v in enumerate(values[:n])])
        mine.step()
        ref.step()
        for i, (p, q) in enumerate(zip(a[:n], b[:n])):
            _close(p, q, i)
    for step in range(2):
        both(script[step], 5)
    m0, v0, steps0 = mine.exp_avg.clone(), mine.exp_avg_sq.clone(), mine.steps.copy()
    # straight behind the step, its table copy possibly still queued; one new tensor needs no gradient and is dropped
    new = dict(HYPER[3], lr=2e-3, params=a[5:] + [torch.zeros(2, device=DEV)])
    mine.add_param_group(new)
    ref.add_param_group(dict(HYPER[3], lr=2e-3, params=b[5:]))
    n_old = m0.numel()
    assert mine.params == a and [len(grp["params"]) for grp in mine.param_groups] == [3, 2, 3]
    assert _same(mine.exp_avg[:n_old], m0) and _same(mine.exp_avg_sq[:n_old], v0)
    assert float(mine.exp_avg[n_old:].abs().max()) == 0.0 == float(mine.exp_avg_sq[n_old:].abs().max())
    assert mine.steps.tolist() == steps0.tolist() + [0, 0, 0] == [2, 2, 2, 2, 2, 0, 0, 0]
    assert mine.param_groups[2]["betas"] == (0.95, 0.98) and "params" in new and len(new["params"]) == 4
    with pytest.raises(ValueError):
        mine.add_param_group({"params": [a[6]]})          # a parameter already present
    with pytest.raises(ValueError):
        mine.add_param_group({"params": [torch.zeros(3, device=DEV, requires_grad=True)], "amsgrad": True})
    assert len(mine.param_groups) == 3 and len(mine.params) == 8
    for step in range(2, 6):                              # the clamp of parameter VIEW survived: `both` clamps torch's copy
        both(script[step], 8)
    assert float(a[VIEW].grad.abs().max()) == 1.0
    _moments_match(mine, ref, 8)
    assert mine.steps.tolist() == [6, 4, 6, 6, 6, 4, 4, 4]


def test_add_param_group_under_loss_scaling_keeps_the_skip_counters():
    a, g = _params(19, NUMEL[:4])
    mine = optim.FlatAdamW(_groups(a[:2], HYPER[:1], [(0, 2)]))
    scaler = optim.LossScaler(init_scale=4.0)
    for p in a[:2]:
        p.grad = torch.full_like(p, INF)
    scaler.step(mine)
    scaler.update()
    mine.add_param_group(dict(HYPER[2], params=a[2:]))
    assert mine._skipped.tolist() == [1, 1, 0, 0]
    start = _clones(a)
    for p in a:
        p.grad = torch.ones_like(p)
    scaler.step(mine)
    scaler.update()
    assert not any(_same(p, q) for p, q in zip(a, start))
    assert [float(s["step"]) for s in mine.state_dict()["state"].values()] == [1.0] * 4


# ---- 6. checkpoints --------------------------------------------------------------------------------------------------

def test_checkpoints_interchange_with_torch_adamw_in_both_directions():
    a, g = _params(23)
    script = _script(g)
    flat = torch.zeros(NUMEL[VIEW] + 3, device=DEV)
    # the pair that never changes hands
    stay_mine, stay_ref = _clones(a), _clones(a)
    o_mine, o_ref = optim.FlatAdamW(_groups(stay_mine)), _torch_adamw(stay_ref)
    for values in script:
        _set_grads(stay_mine, values, flat)
        _set_grads(stay_ref, values)
        o_mine.step()
        o_ref.step()
    # FlatAdamW -> torch.optim.AdamW -> FlatAdamW, two steps each
    first = optim.FlatAdamW(_groups(a))
    sched = torch.optim.lr_scheduler.LambdaLR(first, LAMBDAS)       # leaves initial_lr in every group; never stepped
    for values in script[:2]:
        _set_grads(a, values, flat)
        first.step()
    sd = first.state_dict()
    assert [grp["params"] for grp in sd["param_groups"]] == [[0, 1, 2], [], [3], [4, 5, 6, 7]]
    assert all("initial_lr" in grp for grp in sd["param_groups"]) and sched.last_epoch == 0
    b = _clones(a)
    middle = _torch_adamw(b)
    middle.load_state_dict(sd)
    for values in script[2:4]:
        _set_grads(b, values)
        middle.step()
    c = _clones(b)
    last = optim.FlatAdamW(_groups(c))
    last.load_state_dict(middle.state_dict())
    assert last.steps.tolist() == [4, 2, 4, 4, 4, 4, 4, 4] and last.param_groups[3]["betas"] == (0.95, 0.98)
    for values in script[4:]:
        _set_grads(c, values, flat)
        last.step()
    for i, (p, q, r) in enumerate(zip(c, stay_mine, stay_ref)):
        _close(p, q, i)
        _close(p, r, i)
    _moments_match(last, o_ref, 8)
    # torch's refusals
    sd = last.state_dict()
    fewer = dict(sd, param_groups=sd["param_groups"][:3])
    moved = dict(sd, param_groups=[dict(grp) for grp in sd["param_groups"]])
    moved["param_groups"][0]["params"], moved["param_groups"][1]["params"] = [0, 1], [2]
    for bad in (fewer, moved):
        with pytest.raises(ValueError):
            last.load_state_dict(bad)
        with pytest.raises(ValueError):
            middle.load_state_dict(bad)
    one = optim.FlatAdamW(_clones(a))
    with pytest.raises(ValueError):
        one.load_state_dict(sd)


# ---- 7. unsupported flags --------------------------------------------------------------------------------------------

def test_unsupported_flags_are_refused():
    a, _ = _params(29, NUMEL[:3])
    with pytest.raises(ValueError, match="amsgrad"):
        optim.FlatAdamW([{"params": a[:2]}, {"params": a[2:], "amsgrad": True}])
    opt = optim.FlatAdamW([{"params": a[:2]}, {"params": a[2:], "amsgrad": False, "foreach": None}])
    assert len(opt.param_groups) == 2
    with pytest.raises(ValueError):
        optim.FlatAdamW([{"params": [torch.zeros(3, device=DEV)]}])            # no parameter at all
