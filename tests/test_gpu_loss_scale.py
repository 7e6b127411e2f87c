"""GPU: dynamic loss scaling on the device (wsis_grad_nonfinite, wsis_adamw_step_scaled, wsis_loss_scale_update;
wsis_optim.LossScaler, FlatAdamW under torch.amp.GradScaler, harness.train_step(scaler=)).

1. The check kernel finds one +-inf / NaN wherever a launch path could lose it, ignores what is finite or outside every
   segment, never reads a gradient-less parameter and never clears the flag.
2. The scaled step against torch.optim.AdamW fed the unscaled gradients, with overflow steps that must leave every byte.
3. The ECC clamp acts on the unscaled gradient.
4. The scale schedule equals torch.amp.GradScaler's.
5. torch.amp.GradScaler drives FlatAdamW through the fused-optimizer protocol; no step reads the device back.
6. The whole fp16 training step with a scaler; an absurd scale backs off until a step goes through.
7. Accuracy of the fp16 native pass with a scaled output gradient.

   Measured on one MI355X (set-up of test_gpu_lowp_train.test_accuracy_against_fp32_native_pass, fp16; 1 - cos of the 139
   parameter gradients against the fp32 native pass):
     unscaled        median 2.516e-4, worst 1.738e-1
     scaled by 2^16  median 7.103e-5, worst 1.539e-3
   Asserted: each scaled figure <= 1.25 x the unscaled one (WALK_FACTOR); the 113-fold gain of the worst parameter is a
   measurement, not a bound.

The tensors of 1.-5. are those of test_gpu_ops.test_flat_adamw_matches_torch_adamw_step_by_step, gradients as views that
start 4 bytes into one flat buffer: no view is 16-byte aligned, so every element there goes through the scalar path; the
same gradients as allocations of their own ("own") reach the float4 path, its tail and the one-element second chunk.
"""
import numpy as np
import pytest
import torch

import harness
import wsis_native as _n
import wsis_optim as optim

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 3, 3, 6, 32), (32,), (7, 64), (1,), (1025,), (96, 32), (20,)]
INF, NAN = float("inf"), float("nan")
FLT_MAX = float(np.finfo(np.float32).max)


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes], g


def _set_grads(params, flat, values, layout):
    """values[i] None: no gradient.  "views": packed from 4 bytes into ``flat`` (what is left of it keeps its bytes);
    "own": one allocation each"""
    off = 1
    for p, v in zip(params, values):
        if v is None:
            p.grad = None
        elif layout == "own":
            p.grad = v.clone()
        else:
            view = flat[off:off + p.numel()].view(p.shape)
            view.copy_(v)
            off += p.numel()
            p.grad = view
    return off


def _torch_scaler(**kw):
    scaler = torch.amp.GradScaler("cuda", **kw)
    scaler.scale(torch.zeros((), device=DEV))             # torch makes its scale tensor when a loss is first scaled
    return scaler


# ---- 1. the check kernel ---------------------------------------------------------------------------------------------

def _check(opt, flag):
    tab = opt._stage_table(True)
    _n.check(_n.hip().wsis_grad_nonfinite(_n.ptr(tab), _n.ptr(opt._blocks), opt._n_blocks, _n.ptr(flag), _n.stream_ptr()),
             "grad_nonfinite")
    return float(flag)


# (tensor, flat element): first element; last element of a float4 and of a chunk; element 1024 of the 1025 tensor (a
# second chunk of one element); the tail of a view / of a tensor that is no multiple of four; the one-element tensor
PLACES = [(0, 0), (0, 3), (0, 1023), (0, 5183), (4, 1024), (4, 1023), (2, 447), (6, 19), (1, 31), (3, 0)]


@pytest.mark.parametrize("layout", ["views", "own"])
def test_check_kernel_finds_one_nonfinite_element(layout):
    a, g = _params(SHAPES, 3)
    opt = optim.FlatAdamW(a, lr=1e-3, weight_decay=1e-4)
    flat = torch.zeros(sum(p.numel() for p in a) + 3, device=DEV)
    clean = [torch.randn(p.shape, generator=g).cuda() for p in a]
    flag = torch.zeros(1, device=DEV)
    for i, e in PLACES:
        for bad in (INF, -INF, NAN):
            vals = [c.clone() for c in clean]
            vals[i].view(-1)[e] = bad
            _set_grads(a, flat, vals, layout)
            flag.zero_()
            assert _check(opt, flag) == 1.0, (layout, i, e, bad)
    # finite, however odd: largest float, signed zero, denormals (smallest and largest)
    vals = [c.clone() for c in clean]
    for i, _ in PLACES:
        v = vals[i].view(-1)
        v[0], v[-1] = FLT_MAX, -FLT_MAX
        if v.numel() > 4:
            v[1], v[2], v[3] = -0.0, 1e-45, -1.1754942e-38
    vals[3].view(-1)[0] = 1e-45
    end = _set_grads(a, flat, vals, layout)
    b4 = _bits(a[4].grad)[:4].tolist()                      # the odd values arrived as such: -0.0 and two denormals
    assert b4[1] == -2 ** 31 and b4[2] == 1 and b4[3] == -2 ** 31 + 0x007fffff, b4
    flag.zero_()
    assert _check(opt, flag) == 0.0, layout
    # non-finite values in the buffer outside every segment: the three pad floats
    if layout == "views":
        assert end == flat.numel() - 2
        flat[0], flat[-2], flat[-1] = NAN, INF, -INF
        assert _check(opt, flag) == 0.0
    # a parameter without a gradient (pointer 0, n 0) is not read; the others still are
    vals[3] = None
    _set_grads(a, flat, vals, layout)
    assert _check(opt, flag) == 0.0, layout
    vals[6].view(-1)[19] = NAN
    _set_grads(a, flat, vals, layout)
    assert _check(opt, flag) == 1.0, layout
    # the kernel never clears the flag: clean gradients leave a set one alone (whatever its value)
    _set_grads(a, flat, clean, layout)
    assert _check(opt, flag) == 1.0, layout
    flag.fill_(7.0)
    assert _check(opt, flag) == 7.0, layout


# ---- 2. the scaled step against torch, and the script the protocol test shares -----------------------------------------

STEPS = 8
# (step, tensor, element, value), steps counted from 0 as in the fp32 test, where parameter 3 has no gradient on even
# steps.  Step 2: an overflow while parameter 3 has no gradient -- its count must not move, which is why the skip counters
# are per segment.  Step 4: the same with a NaN, in the tail of the last view.  Step 5: a NaN in the one-element tensor,
# which has a gradient on odd steps only (a NaN there "on step 4" cannot exist: that step is added, none is dropped).
OVERFLOW = {2: (4, 1024, INF), 4: (6, 19, NAN), 5: (3, 0, NAN)}


def _script_gradients(shapes, g):
    """the unscaled gradients of every step (None: no gradient) and of one more, on which every parameter has one"""
    out = []
    for step in range(STEPS + 1):
        out.append([None if (i == 3 and step % 2 == 0 and step < STEPS) else
                    torch.randn(s, generator=g).cuda() * (10.0 ** (i - 3)) for i, s in enumerate(shapes)])
    return out


def _run_script(driver, layout="views"):
    """eight steps from scale 2^10 (halved after every overflow step: growth is out of reach).  driver: "loss_scaler",
    "grad_scaler" (torch.amp.GradScaler.step through the fused-optimizer protocol) or "grad_scaler_unscale" (torch's
    unscale_ -> step recipe).  Checks every step against torch.optim.AdamW; returns what the callers compare."""
    a, g = _params(SHAPES, 3)
    b = [t.detach().clone().requires_grad_(True) for t in a]
    mine = optim.FlatAdamW(a, lr=1e-3, weight_decay=1e-4)
    ref = torch.optim.AdamW(b, lr=1e-3, weight_decay=1e-4, foreach=False, fused=False)
    if driver == "loss_scaler":
        scaler = optim.LossScaler(init_scale=2.0 ** 10)
    else:
        scaler = _torch_scaler(init_scale=2.0 ** 10)
    flat = torch.zeros(sum(t.numel() for t in a) + 3, device=DEV)
    grads = _script_gradients(SHAPES, g)
    S = 2.0 ** 10
    for step in range(STEPS):
        scaled = [None if v is None else v * S for v in grads[step]]
        if step in OVERFLOW:
            i, e, bad = OVERFLOW[step]
            scaled[i].view(-1)[e] = bad
        _set_grads(a, flat, scaled, layout)
        before = [(p.detach().clone(), None if p.grad is None else p.grad.clone()) for p in a]
        m0, v0 = mine.exp_avg.clone(), mine.exp_avg_sq.clone()
        if driver == "grad_scaler_unscale":
            scaler.unscale_(mine)
        scaler.step(mine)
        scaler.update()
        if step in OVERFLOW:
            for i, (p, (p0, g0)) in enumerate(zip(a, before)):
                assert _same(p, p0), (driver, step, i, "parameter written on a skipped step")
                if driver != "grad_scaler_unscale":         # (torch's unscale_ has multiplied .grad in place by then)
                    assert (p.grad is None) == (g0 is None) and (g0 is None or _same(p.grad, g0)), (driver, step, i)
            assert _same(mine.exp_avg, m0) and _same(mine.exp_avg_sq, v0), (driver, step, "moments")
            S *= 0.5
        else:
            inv = 1.0 / S
            for q, v in zip(b, scaled):
                q.grad = None if v is None else v * inv
            ref.step()
            assert not _same(a[0], before[0][0]), (driver, step, "no update")
            if driver == "loss_scaler":                     # no clamp: .grad is not written back, it stays scaled
                for p, v in zip(a, scaled):
                    assert p.grad is None or torch.equal(p.grad, v), (driver, step)
        for p, q in zip(a, b):
            assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * float(q.detach().abs().max()) + 1e-9, (driver, step, p.shape)
        assert float(scaler.get_scale()) == S, (driver, step)
    return a, b, mine, ref, scaler, grads[STEPS], flat


@pytest.mark.parametrize("layout", ["views", "own"])
def test_scaled_step_matches_torch_and_skips_leave_every_byte(layout):
    a, b, mine, ref, scaler, last, flat = _run_script("loss_scaler", layout)
    assert mine._skipped.tolist() == [3, 3, 3, 1, 3, 3, 3]             # parameter 3: only the step it had a gradient on
    assert mine.steps.tolist() == [8, 8, 8, 4, 8, 8, 8]                # calls with a gradient: the host's meaning
    sd, rs = mine.state_dict(), ref.state_dict()["state"]
    assert sorted(sd["state"]) == sorted(rs) == list(range(len(a)))
    for i in range(len(a)):
        assert float(sd["state"][i]["step"]) == float(rs[i]["step"]), i
        for name in ("exp_avg", "exp_avg_sq"):
            want = rs[i][name]
            assert float((sd["state"][i][name] - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-30, (i, name)
    # round trip into a fresh optimizer (and into one that has skipped before: its counters are zeroed)
    c = [t.detach().clone().requires_grad_(True) for t in a]
    other = optim.FlatAdamW(c, lr=1e-3, weight_decay=1e-4)
    other.load_state_dict(sd)
    assert other._skipped is None and other.steps.tolist() == [5, 5, 5, 3, 5, 5, 5]
    mine.load_state_dict(sd)
    assert mine._skipped.tolist() == [0] * 7 and (mine.steps == other.steps).all()
    S = scaler.get_scale()
    other_scaler = optim.LossScaler(init_scale=S)
    flat2 = torch.zeros_like(flat)
    _set_grads(a, flat, [v * S for v in last], layout)
    _set_grads(c, flat2, [v * S for v in last], layout)
    for q, v in zip(b, last):
        q.grad = (v * S) * (1.0 / S)
    scaler.step(mine)
    scaler.update()
    other_scaler.step(other)
    other_scaler.update()
    ref.step()
    for i, (p, r, q) in enumerate(zip(a, c, b)):
        assert _same(p, r), (i, "an optimizer that skipped and one resumed from its checkpoint take different steps")
        assert float((r.detach() - q.detach()).abs().max()) <= 2e-6 * float(q.detach().abs().max()) + 1e-9, i
    assert [float(other.state_dict()["state"][i]["step"]) for i in range(7)] == [6.0, 6.0, 6.0, 4.0, 6.0, 6.0, 6.0]


def test_plain_step_stays_on_the_fp32_entry_point_until_a_scaler_appears():
    a, g = _params([(33,), (1025,)], 9)
    b = [t.detach().clone().requires_grad_(True) for t in a]
    mine = optim.FlatAdamW(a, lr=1e-3, weight_decay=1e-4)
    ref = torch.optim.AdamW(b, lr=1e-3, weight_decay=1e-4, foreach=False, fused=False)

    def grads():
        for p, q in zip(a, b):
            p.grad = torch.randn(p.shape, generator=g).cuda()
            q.grad = p.grad.clone()
    for _ in range(2):
        grads()
        mine.step()
        ref.step()
    assert mine._skipped is None
    # torch's attribute protocol by hand: a flag without a scale (the stage after unscale_), then neither
    mine.found_inf = torch.ones(1, device=DEV)
    grads()
    p0 = [p.detach().clone() for p in a]
    mine.step()
    assert all(_same(p, q) for p, q in zip(a, p0)) and mine._skipped.tolist() == [1, 1]
    mine.found_inf = None
    mine.grad_scale = None
    for _ in range(2):          # the counters stay honoured without a scaler: t = 4 - 1, 5 - 1
        grads()
        mine.step()
        ref.step()
        for p, q in zip(a, b):
            assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * float(q.detach().abs().max()) + 1e-9
    assert float(mine.state_dict()["state"][0]["step"]) == 4.0 == float(ref.state_dict()["state"][0]["step"])
    with pytest.raises(ValueError):
        mine.found_inf = torch.zeros(1)
        mine.step()


# ---- 3. clamp under scaling ------------------------------------------------------------------------------------------

def test_clamp_acts_on_the_unscaled_gradient():
    shapes = [(96, 32), (33,), (1025,), (7, 5)]
    a, g = _params(shapes, 5)
    b = [t.detach().clone().requires_grad_(True) for t in a]
    mine = optim.FlatAdamW(a, lr=1e-3, weight_decay=1e-4)
    assert mine.set_grad_clamp([a[0], a[2], a[3]], 1.0) == 3
    ref = torch.optim.AdamW(b, lr=1e-3, weight_decay=1e-4, foreach=False, fused=False)
    scaler = optim.LossScaler(init_scale=2.0 ** 8)
    S, inv = 2.0 ** 8, 1.0 / 2.0 ** 8
    flat = torch.zeros(sum(t.numel() for t in a) + 3, device=DEV)
    for step in range(3):
        scaled = [torch.randn(p.shape, generator=g).cuda() * 3.0 * S for p in a]
        _set_grads(a, flat, scaled, "views")
        for i, (q, v) in enumerate(zip(b, scaled)):
            q.grad = (v * inv).clamp(-1.0, 1.0) if i != 1 else v * inv
        assert float((scaled[0] * inv).abs().max()) > 1.0        # the clamp has something to do
        scaler.step(mine)
        scaler.update()
        ref.step()
        for i, (p, q) in enumerate(zip(a, b)):
            assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * float(q.detach().abs().max()) + 1e-9, (step, i)
            if i != 1:
                assert torch.equal(p.grad, q.grad), (step, i, "clamp(g / scale) written back")
            else:
                assert torch.equal(p.grad, scaled[1]), (step, "the unclamped gradient is untouched and still scaled")
    # a NaN in a clamped tensor (vector path of the step has none here; its scalar tail): the step is a skipped one
    scaled = [torch.randn(p.shape, generator=g).cuda() * 3.0 * S for p in a]
    scaled[2].view(-1)[1024] = NAN
    _set_grads(a, flat, scaled, "views")
    p0 = [p.detach().clone() for p in a]
    m0, v0 = mine.exp_avg.clone(), mine.exp_avg_sq.clone()
    scaler.step(mine)
    scaler.update()
    for i, (p, q, v) in enumerate(zip(a, p0, scaled)):
        assert _same(p, q) and _same(p.grad, v), i
    assert _same(mine.exp_avg, m0) and _same(mine.exp_avg_sq, v0)
    assert scaler.get_scale() == S / 2 and mine._skipped.tolist() == [1, 1, 1, 1]


# ---- 4. the scale schedule -------------------------------------------------------------------------------------------

def _schedule_pair(init_scale, growth_interval):
    p, q = torch.zeros(5, device=DEV, requires_grad=True), torch.zeros(5, device=DEV, requires_grad=True)
    return (optim.LossScaler(init_scale=init_scale, growth_interval=growth_interval), optim.FlatAdamW([p]), p,
            _torch_scaler(init_scale=init_scale, growth_interval=growth_interval), torch.optim.SGD([q], lr=0.1), q)


def _schedule_step(pair, overflow):
    mine, opt, p, theirs, sgd, q = pair
    p.grad = torch.full((5,), INF if overflow else 1.0, device=DEV)
    q.grad = p.grad.clone()
    mine.step(opt)
    mine.update()
    theirs.step(sgd)
    theirs.update()
    return mine.get_scale(), theirs.get_scale()


def test_scale_schedule_equals_grad_scalers():
    pair = _schedule_pair(2.0 ** 10, 3)
    # grow; back off; an overflow with the tracker at 2; grow again; two overflows in a row
    pattern = [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 1]
    seen = []
    for step, o in enumerate(pattern):
        got, want = _schedule_step(pair, o)
        assert got == want, (step, got, want)
        seen.append(got)
        if step == 7:       # tracker at 1: a checkpoint carries it
            sd = pair[0].state_dict()
            assert sd == {"scale": got, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 3, "growth_tracker": 1}
            assert pair[3].state_dict()["_growth_tracker"] == 1
            resumed = optim.LossScaler()
            resumed.load_state_dict(sd)
            assert resumed.state_dict() == sd
            pair = (resumed,) + pair[1:]
    assert seen == [2.0 ** k for k in (10, 10, 11, 10, 10, 10, 9, 9, 9, 10, 9, 8)]
    # the largest power of two does not grow to inf
    pair = _schedule_pair(2.0 ** 127, 1)
    for step in range(3):
        assert _schedule_step(pair, 0) == (2.0 ** 127, 2.0 ** 127), step
    assert _schedule_step(pair, 1) == (2.0 ** 126, 2.0 ** 126)
    assert _schedule_step(pair, 0) == (2.0 ** 127, 2.0 ** 127)


def test_loss_scaler_interface():
    p = torch.ones(5, device=DEV, requires_grad=True)
    opt = optim.FlatAdamW([p])
    scaler = optim.LossScaler(init_scale=4.0)
    loss = (p * 0.5).sum()
    scaled = scaler.scale(loss)
    assert scaled.shape == loss.shape and float(scaled.detach()) == 4.0 * float(loss.detach())
    scaled.backward()
    assert torch.equal(p.grad, torch.full((5,), 2.0, device=DEV))
    scaler.step(opt)
    with pytest.raises(RuntimeError):
        scaler.step(opt)                                  # two steps without an update, as torch refuses them
    scaler.update()
    scaler.step(opt)
    scaler.update()
    with pytest.raises(TypeError):
        scaler.step(torch.optim.SGD([p], lr=0.1))
    # disabled: every method passes through to the plain step
    q = torch.ones(5, device=DEV, requires_grad=True)
    plain = optim.FlatAdamW([q])
    off = optim.LossScaler(enabled=False)
    loss = (q * 0.5).sum()
    assert off.scale(loss) is loss and off.get_scale() == 1.0 and off.state_dict() == {}
    loss.backward()
    off.step(plain)
    off.step(plain)
    off.update()
    assert plain._skipped is None and plain.steps.tolist() == [2] and not torch.equal(q.detach(), torch.ones_like(q))


# ---- 5. torch's protocol ---------------------------------------------------------------------------------------------

def test_grad_scaler_drives_flat_adamw_like_loss_scaler():
    a = _run_script("loss_scaler")[0]
    for driver in ("grad_scaler", "grad_scaler_unscale"):
        c, _, opt = _run_script(driver)[:3]
        assert opt._skipped.tolist() == [3, 3, 3, 1, 3, 3, 3], driver
        for i, (p, r) in enumerate(zip(a, c)):
            assert _same(p, r), (driver, i)


def test_no_step_reads_the_device_back():
    a, g = _params(SHAPES, 3)
    c = [t.detach().clone().requires_grad_(True) for t in a]
    mine, theirs = optim.FlatAdamW(a), optim.FlatAdamW(c)
    s_mine, s_theirs = optim.LossScaler(init_scale=2.0 ** 10), _torch_scaler(init_scale=2.0 ** 10)
    steps = 6                                             # past the ring of table slots
    vals = [[torch.randn(p.shape, generator=g).cuda() * 2.0 ** 10 for p in a] for _ in range(steps)]
    vals[2][4].view(-1)[1024] = INF
    p0 = [p.detach().clone() for p in a]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()              # the mode does raise on a read-back under this torch
        for step in range(steps):
            for params, opt, sc in ((a, mine, s_mine), (c, theirs, s_theirs)):
                for p, v in zip(params, vals[step]):
                    p.grad = v
                sc.step(opt)
                sc.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert mine._skipped.tolist() == [1] * 7 == theirs._skipped.tolist()
    for p, q, r in zip(a, p0, c):
        assert not _same(p, q) and _same(p, r)
    assert s_mine.get_scale() == 2.0 ** 9 == s_theirs.get_scale()


# ---- 6. the whole step in fp16 ---------------------------------------------------------------------------------------

def _scene():
    return harness.make_scene(0, room=(3.0, 3.0, 2.4), n_box=2, max_points=10000)


def _param_bytes(model):
    return [p.detach().clone() for p in model.parameters()]


def test_whole_fp16_step_with_a_scaler(monkeypatch):
    monkeypatch.setenv("WSIS_NATIVE_LP_TRAIN", "1")
    monkeypatch.delenv("WSIS_NATIVE_UNET", raising=False)
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([_scene()]), DEV)

    def step(model, crit, opt, scaler):
        with torch.autocast("cuda", dtype=torch.float16):
            loss, _ = harness.train_step(model, crit, opt, batch, cfg, scaler=scaler)
        assert model.last_pass == "native_lp_train"
        return loss.clone()

    runs = []
    for _ in range(2):
        model, crit, opt = harness.build_model(cfg, DEV)
        model.train()
        start = _param_bytes(model)
        scaler = optim.LossScaler()
        losses = torch.stack([step(model, crit, opt, scaler) for _ in range(4)])
        assert bool(torch.isfinite(losses).all()), losses.tolist()
        end = _param_bytes(model)
        unet = [i for i, (k, _) in enumerate(model.named_parameters()) if k.startswith(("input_conv.", "unet.", "output_layer."))]
        still = [i for i in unet if _same(start[i], end[i])]      # every UNet parameter has a gradient in this pass
        assert unet and not still, f"{len(still)} of {len(unet)} UNet parameters did not move in four steps (scale {scaler.get_scale()})"
        runs.append((losses, end, scaler.get_scale()))
    print(f"fp16 whole step: losses {runs[0][0].tolist()}, scale after four steps {runs[0][2]}")
    assert _same(runs[0][0], runs[1][0]), (runs[0][0].tolist(), runs[1][0].tolist())
    assert all(_same(p, q) for p, q in zip(runs[0][1], runs[1][1])) and runs[0][2] == runs[1][2]

    # a scale at which any output gradient of the UNet above 6e-8 overflows fp16: the first step is a skipped one
    model, crit, opt = harness.build_model(cfg, DEV)
    model.train()
    start = _param_bytes(model)
    scaler = optim.LossScaler(init_scale=2.0 ** 40)
    loss = step(model, crit, opt, scaler)
    assert bool(torch.isfinite(loss))
    assert all(_same(p, q) for p, q in zip(model.parameters(), start)), "the first step at scale 2^40 was not skipped"
    assert scaler.get_scale() == 2.0 ** 39
    assert int(opt._skipped[0]) == 1 and int(opt._skipped.max()) == 1
    through = None
    for k in range(1, 40):
        step(model, crit, opt, scaler)
        if not _same(next(model.parameters()), start[0]):
            through = k
            break
    assert through is not None, f"no step went through in 40; scale {scaler.get_scale()}"
    print(f"fp16 whole step from scale 2^40: step {through} went through, scale then {scaler.get_scale()}")
    assert scaler.get_scale() == 2.0 ** (40 - through)
    steps = opt.state_dict()["state"][0]["step"]
    assert float(steps) == 1.0


# ---- 7. accuracy -----------------------------------------------------------------------------------------------------

def test_accuracy_with_a_scaled_output_gradient():
    """fp16 native pass, output gradient multiplied by S and parameter gradients divided by it, S the largest power of two
    (from 2^16 down) without a non-finite gradient; 1 - cos per parameter gradient against the fp32 native pass.

    The figures are printed; the measured ones are in the module docstring and in DESIGN.md section 10.2."""
    import test_gpu_lowp_train as lp
    import unet_native as un
    dt = torch.float16
    model, crit, batch, cfg, state = lp._trained()
    params = un._program(model).params
    G = torch.randn((int(lp._input(batch, cfg).features.shape[0]), model.output_layer[0].num_features), device=DEV,
                    generator=torch.Generator(device=DEV).manual_seed(11)) * 0.01

    def run(kind, S=1.0):
        lp._restore(model, state)
        inp = lp._input(batch, cfg)
        out = un.run_unet(model, inp) if kind == "fp32" else un.run_unet_lp_train(model, inp, dt, dt)
        out.backward((G * S).to(out.dtype))
        return [p.grad.detach().clone().float() * (1.0 / S) for p in params]
    try:
        g32 = run("fp32")
        g_plain = run("native")
        S = 2.0 ** 16
        while True:
            g_scaled = run("native", S)
            if all(bool(torch.isfinite(t).all()) for t in g_scaled):
                break
            S *= 0.5
            assert S >= 1.0, "no power of two leaves the gradients finite"
    finally:
        lp._restore(model, state)
    c_plain = np.array([lp._one_minus_cos(a, b) for a, b in zip(g_plain, g32)])
    c_scaled = np.array([lp._one_minus_cos(a, b) for a, b in zip(g_scaled, g32)])
    print(f"fp16 native pass, 1 - cos of {len(params)} parameter gradients against the fp32 native pass: unscaled median "
          f"{np.median(c_plain):.3e}, worst {c_plain.max():.3e}; scaled by 2^{int(np.log2(S))} median "
          f"{np.median(c_scaled):.3e}, worst {c_scaled.max():.3e}")
    assert S > 1.0, "scaling by 1 shows nothing"
    assert np.median(c_scaled) <= lp.WALK_FACTOR * np.median(c_plain), (np.median(c_scaled), np.median(c_plain))
    assert c_scaled.max() <= lp.WALK_FACTOR * c_plain.max(), (c_scaled.max(), c_plain.max())
