"""GPU: the whole per-scene path (Network + MultiTaskLoss, fwd + bwd) on the HIP operators against the CPU
oracle restatement (oracle/network_ref.py) with the same weights and the same synthetic batch."""
import numpy as np
import pytest
import torch

import harness
from oracle import network_ref

pytestmark = pytest.mark.gpu


def _setup(n_scenes, seed0, room):
    cfg = harness.default_cfg()
    scenes = [harness.make_scene(seed0 + i, room=room, n_box=1) for i in range(n_scenes)]
    batch_host = harness.collate(scenes)
    cfg.batch_size = n_scenes
    model, crit, opt = harness.build_model(cfg, "cuda")
    ref = network_ref.RefNetwork()
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    return cfg, batch_host, model, crit, opt, ref


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("n_scenes", [1, 2])
def test_network_forward_backward_matches_oracle(n_scenes):
    cfg, batch_host, model, crit, opt, ref = _setup(n_scenes, 10, (1.4, 1.1, 0.9))
    batch = harness.to_device(batch_host, "cuda")
    model.train()
    ref.train()
    loss, ret = harness.forward_loss(model, crit, batch, cfg)
    loss.backward()
    r_loss, r_ret = network_ref.forward_loss_cpu(ref, crit, batch_host)
    r_loss.backward()
    # forward tensors: fp32 through 49 conv + 53 BN layers; tolerance stated here: 2e-3 relative L2
    for k in ("semantic_scores", "sp_semantic_scores", "pred_sp_offset_vectors", "pred_sp_occupancy",
              "pred_sp_ins_size", "edge_affinity", "sp_discriminative_feats"):
        assert ret[k].shape == r_ret[k].shape, k
        assert _rel(ret[k], r_ret[k]) < 2e-3, (k, _rel(ret[k], r_ret[k]))
    assert abs(float(loss) - float(r_loss)) < 2e-3 * abs(float(r_loss))
    # gradients of every parameter: 2e-2 relative L2 (accumulated through the whole backward)
    ref_params = dict(ref.named_parameters())
    gmax = max(float(p.grad.norm()) for p in ref.parameters() if p.grad is not None)
    worst = ("", 0.0)
    for name, p in model.named_parameters():
        rp = ref_params[name]
        if rp.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        # parameters whose true gradient is zero (biases feeding a BatchNorm) hold only rounding noise:
        # the error is measured against the parameter's own gradient norm plus 1e-5 of the largest one
        diff = float((p.grad.detach().cpu().double() - rp.grad.double()).norm())
        e = diff / (float(rp.grad.norm()) + 1e-5 * gmax)
        if e > worst[1]:
            worst = (name, e)
    assert worst[1] < 2e-2, worst
    # running statistics of every BatchNorm updated identically
    ref_bufs = dict(ref.named_buffers())
    for name, b in model.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            assert _rel(b, ref_bufs[name]) < 1e-3, name


def test_network_gradients_against_the_fp64_oracle_per_parameter():
    """the 2e-2 bound above compares two fp32 evaluations (both drift).  Here the oracle runs in fp64, so the error
    is the HIP path's own: every parameter gradient of the 49-conv / 53-BN network within 6e-3 relative L2 of the
    double-precision value, the median over the 361 tensors below 6e-4 (measured: median 7.5e-5, 90th percentile
    8.2e-4, worst 3.5e-3 on a BatchNorm bias of the first block -- fp32 rounding through ~100 layers each way; with
    WSIS_FUSE_BN_STATS=0 the median is 3.7e-4), forward heads within 2e-4."""
    cfg, batch_host, model, crit, opt, ref = _setup(2, 10, (1.4, 1.1, 0.9))
    batch = harness.to_device(batch_host, "cuda")
    model.train()
    ref = ref.double().train()
    loss, ret = harness.forward_loss(model, crit, batch, cfg)
    loss.backward()
    r_loss, r_ret = network_ref.forward_loss_cpu(ref, crit, batch_host, dtype=torch.float64)
    r_loss.backward()
    for k in ("semantic_scores", "sp_semantic_scores", "pred_sp_offset_vectors", "edge_affinity",
              "sp_discriminative_feats"):
        assert _rel(ret[k], r_ret[k]) < 2e-4, (k, _rel(ret[k], r_ret[k]))
    ref_params = dict(ref.named_parameters())
    gmax = max(float(p.grad.norm()) for p in ref.parameters() if p.grad is not None)
    errs = []
    for name, p in model.named_parameters():
        rp = ref_params[name]
        if rp.grad is None:
            continue
        diff = float((p.grad.detach().cpu().double() - rp.grad).norm())
        errs.append((diff / (float(rp.grad.norm()) + 1e-5 * gmax), name))
    errs.sort()
    print("fp64-oracle gradient errors: median %.2e  p90 %.2e  worst %.2e (%s)" %
          (errs[len(errs) // 2][0], errs[int(len(errs) * 0.9)][0], errs[-1][0], errs[-1][1]))
    assert errs[-1][0] < 6e-3, errs[-1]
    assert errs[len(errs) // 2][0] < 6e-4, errs[len(errs) // 2]


def test_batchnorm_statistics_from_the_conv_epilogue_match_the_separate_pass(monkeypatch):
    """WSIS_FUSE_BN_STATS=1 (default): the per-channel sums come from the producing convolution's epilogue as 32-row
    partials (one BatchNorm keeps its own pass: the one behind the 6-channel input conv); against the separate pass
    the loss agrees to 1e-6 relative, every running statistic to 1e-6, the gradients to 1e-2 in relative L2 over all
    parameters and 5e-2 of the largest entry per parameter (two fp32 evaluations of a 100-layer network on this small
    scene -- a few dozen rows at the deepest level -- drift apart chaotically whenever ANY rounding changes: the worst
    parameter read 3.5e-3 of the largest gradient with the round-3 kernels, 6.1e-3 and 3.0e-2 after two unrelated
    rounding changes of round 4, each mode inside the fp64 oracle's bound on the oracle test's scene -- the accuracy gate is
    the fp64-oracle test above, where the fused statistics score better than the separate pass: median error 7.5e-5
    against 3.7e-4), and the fused mode is bit-deterministic."""
    cfg = harness.default_cfg()
    batch_host = harness.collate([harness.make_scene(21, room=(1.8, 1.4, 1.1), n_box=2)])
    res = {}
    for mode in ("0", "1", "1b"):
        monkeypatch.setenv("WSIS_FUSE_BN_STATS", mode[0])
        model, crit, opt = harness.build_model(cfg, "cuda")
        batch = harness.to_device(batch_host, "cuda")
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
        loss.backward()
        res[mode] = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
                     {n: b.clone() for n, b in model.named_buffers() if "running" in n})
    l0, g0, b0 = res["0"]
    l1, g1, b1 = res["1"]
    assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0))
    gmax = max(float(v.abs().max()) for v in g0.values())
    for n in g0:
        assert float((g0[n] - g1[n]).abs().max()) <= 5e-2 * gmax, n
    num = sum(float(((g0[n] - g1[n]).double() ** 2).sum()) for n in g0)
    den = sum(float((g0[n].double() ** 2).sum()) for n in g0)
    assert (num / den) ** 0.5 <= 1e-2
    for n in b0:
        assert float((b0[n] - b1[n]).abs().max()) <= 1e-6 * max(float(b0[n].abs().max()), 1.0), n
    assert torch.equal(res["1"][0], res["1b"][0]) and all(torch.equal(g1[n], res["1b"][1][n]) for n in g1)


def test_batchnorm_backward_reduction_from_the_din_epilogue_matches_the_separate_pass(monkeypatch):
    """WSIS_FUSE_BN_BWD=1 (default): the (sum dz, sum dz*xhat) reduction of every BatchNorm backward whose dy comes out
    of a dIn convolution is made by that convolution's epilogue (32-row partials, fp64 sum).  The forward pass is
    untouched (loss EQUAL); against the separate reduction pass every gradient agrees to 2e-3 of the largest (the
    sums are re-associated; the accuracy gate is the fp64-oracle test), and the fused mode is bit-deterministic.
    Full-size scene: on small ones every dIn launch is split into offset slabs and the executor keeps the BatchNorm's
    own one-launch reduction."""
    cfg = harness.default_cfg()
    batch_host = harness.collate([harness.make_scene(21)])
    res = {}
    for mode in ("0", "1", "1b"):
        monkeypatch.setenv("WSIS_FUSE_BN_BWD", mode[0])
        model, crit, opt = harness.build_model(cfg, "cuda")
        batch = harness.to_device(batch_host, "cuda")
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
        loss.backward()
        res[mode] = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    (l0, g0), (l1, g1) = res["0"], res["1"]
    assert torch.equal(l0, l1)
    gmax = max(float(v.abs().max()) for v in g0.values())
    worst = max(float((g0[n] - g1[n]).abs().max()) for n in g0)
    assert worst <= 2e-3 * gmax, (worst, gmax)
    assert any(not torch.equal(g0[n], g1[n]) for n in g0), "the fused reduction did not run"
    assert all(torch.equal(g1[n], res["1b"][1][n]) for n in g1)


def test_train_step_decreases_loss_and_is_deterministic():
    cfg, batch_host, model, crit, opt, ref = _setup(1, 20, (1.4, 1.1, 0.9))
    batch = harness.to_device(batch_host, "cuda")
    l0, _ = harness.train_step(model, crit, opt, batch, cfg)
    for _ in range(4):
        l1, _ = harness.train_step(model, crit, opt, batch, cfg)
    assert float(l1) < float(l0)
    # same seed, same batch => bit-identical first loss (no atomics anywhere in the forward path)
    model2, crit2, opt2 = harness.build_model(cfg, "cuda")
    batch2 = harness.to_device(harness.collate([harness.make_scene(20, room=(1.4, 1.1, 0.9), n_box=1)]), "cuda")
    m0, _ = harness.train_step(model2, crit2, opt2, batch2, cfg)
    assert float(m0) == float(l0)


def test_eval_mode_and_state_dict_roundtrip():
    cfg, batch_host, model, crit, opt, ref = _setup(1, 30, (1.2, 1.0, 0.8))
    batch = harness.to_device(batch_host, "cuda")
    model.eval()
    ref.eval()
    with torch.no_grad():
        loss, ret = harness.forward_loss(model, crit, batch, cfg)
        r_loss, r_ret = network_ref.forward_loss_cpu(ref, crit, batch_host)
    assert _rel(ret["semantic_scores"], r_ret["semantic_scores"]) < 2e-3
    sd = model.state_dict()
    assert len(sd) == 361 and sum(p.numel() for p in model.parameters()) == 11101637
    assert sd["input_conv.0.weight"].shape == (3, 3, 3, 6, 32)
    assert sd["unet.u.u.u.u.blocks.block1.conv_branch.5.weight"].shape == (3, 3, 3, 160, 160)
    assert sd["unet.blocks_tail.block0.i_branch.0.weight"].shape == (1, 1, 1, 64, 32)
    assert sd["unet.conv.2.weight"].shape == (2, 2, 2, 32, 64) and sd["unet.deconv.2.weight"].shape == (2, 2, 2, 64, 32)
    assert sd["ecc.0._cell.weight_ih"].shape == (96, 32) and sd["ecc.0._fnet.7.weight"].shape == (1024, 64)


def _one_pass(monkeypatch, native, batch_host, cfg):
    monkeypatch.setenv("WSIS_NATIVE_UNET", "1" if native else "0")
    model, crit, opt = harness.build_model(cfg, "cuda")
    batch = harness.to_device(batch_host, "cuda")
    loss, ret = harness.forward_loss(model, crit, batch, cfg)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    stats = {n: v.clone() for n, v in model.state_dict().items() if "running_" in n or "num_batches" in n}
    return float(loss), grads, stats, ret["semantic_scores"].detach().clone()


@pytest.mark.parametrize("train", [True, False])
def test_native_unet_executor_is_bit_identical_to_the_module_walk(monkeypatch, train):
    """WSIS_NATIVE_UNET=1 (one wsis_run_ops call per pass, model/unet_native.py) and =0 (spconv modules walked by
    torch) launch the same kernels in the same order: loss, every gradient and every BN buffer must be EQUAL."""
    cfg = harness.default_cfg()
    monkeypatch.setenv("WSIS_FUSE_BN_STATS", "0")     # statistics from a separate pass over x, as the modules compute them
    batch_host = harness.collate([harness.make_scene(21, room=(1.8, 1.4, 1.1), n_box=2)])
    if not train:
        orig = harness.build_model

        def build_eval(*a, **k):
            m, c, o = orig(*a, **k)
            m.eval()
            return m, c, o
        monkeypatch.setattr(harness, "build_model", build_eval)
    l0, g0, s0, y0 = _one_pass(monkeypatch, False, batch_host, cfg)
    l1, g1, s1, y1 = _one_pass(monkeypatch, True, batch_host, cfg)
    assert l0 == l1 and torch.equal(y0, y1)
    assert set(g0) == set(g1) and len(g0) > 150
    assert [n for n in g0 if not torch.equal(g0[n], g1[n])] == []
    assert [n for n in s0 if not torch.equal(s0[n], s1[n])] == []


@pytest.mark.parametrize("dw_stream", ["1", "0"])
def test_batched_slab_sums_give_the_bits_of_the_per_product_sums(monkeypatch, dw_stream):
    """round 6: the executor finishes the weight gradients of a backward pass with ONE dw2_reduce_batch launch per part
    (WSIS_DW_BATCH_REDUCE=1; opt-in: measured slower in the step; every product's slabs in a region of their own) instead
    of one slab-sum launch per product (=0, default: what the module walk and a direct caller of wsis_spconv_dw get): same body, same order of additions --
    every gradient EQUAL, on the side stream with the worker thread and on the caller's stream."""
    cfg = harness.default_cfg()
    monkeypatch.setenv("WSIS_DW_STREAM", dw_stream)
    batch_host = harness.collate([harness.make_scene(s, room=(1.7, 1.3, 1.0), n_box=2) for s in (41, 42)])
    cfg.batch_size = 2
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("WSIS_DW_BATCH_REDUCE", mode)
        batch = harness.to_device(batch_host, "cuda")
        model, crit, opt = harness.build_model(cfg, "cuda")
        model.train()
        losses = []
        for _ in range(2):                      # (the second pass reuses the program's persistent gradient buffer)
            model.zero_grad(set_to_none=True)
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
            loss.backward()
            losses.append(float(loss))
        torch.cuda.synchronize()
        res[mode] = (losses, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert res["0"][0] == res["1"][0]
    g0, g1 = res["0"][1], res["1"][1]
    assert set(g0) == set(g1) and len(g0) > 150
    assert [n for n in g0 if not torch.equal(g0[n], g1[n])] == []


def test_scheduling_switches_of_the_executor_do_not_change_a_bit(monkeypatch):
    """round 6: WHEN and on WHICH stream the executor issues a weight gradient (forked in front of its op's dIn launch,
    the last one of a pass on the caller's stream) and the pass's weight transposes (side stream, joined in front of the
    first reader) changed; the kernels did not.  Loss and every gradient of two passes are EQUAL with each switch off."""
    cfg = harness.default_cfg()
    batch_host = harness.collate([harness.make_scene(s, room=(1.6, 1.3, 1.0), n_box=2) for s in (51, 52)])
    cfg.batch_size = 2

    def run(env):
        for k in ("WSIS_DW_EARLY", "WSIS_DW_TAIL_MAIN", "WSIS_WT_SIDE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        torch.manual_seed(0)
        batch = harness.to_device(batch_host, "cuda")
        model, crit, opt = harness.build_model(cfg, "cuda")
        model.train()
        losses = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
            loss.backward()
            losses.append(float(loss))
        torch.cuda.synchronize()
        return losses, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    base_l, base_g = run({})
    for env in ({"WSIS_DW_EARLY": "0"}, {"WSIS_DW_EARLY": "1"}, {"WSIS_DW_TAIL_MAIN": "0"}, {"WSIS_WT_SIDE": "0"},
                {"WSIS_DW_EARLY": "0", "WSIS_DW_TAIL_MAIN": "0", "WSIS_WT_SIDE": "0"}):
        l, g = run(env)
        assert l == base_l, env
        assert [n for n in base_g if not torch.equal(base_g[n], g[n])] == [], env


def test_training_over_scenes_of_varying_size_is_reproducible():
    """36 optimizer steps cycling over 9 batches of very different sizes (1.8 m room ... 8 m room, one batch of three
    scenes), twice from the same seed: identical loss sequences, no NaN.  Every launch plan, the slice queues of the
    persistent conv kernel and the BatchNorm tickets see a different shape at every step (tools/soak.py runs the same for
    600 steps)."""
    import math
    cfg = harness.default_cfg()
    rooms = [(8.0, 6.5, 2.8), (5.0, 4.0, 2.6), (3.0, 2.5, 2.4), (1.8, 1.4, 1.1), (6.5, 6.0, 2.8), (4.2, 3.1, 2.5),
             (2.2, 2.0, 1.6), (7.3, 5.1, 2.7)]
    scenes = [harness.collate([harness.make_scene(100 + i, room=r, n_box=3 + i % 4)]) for i, r in enumerate(rooms)]
    scenes.append(harness.collate([harness.make_scene(200 + i, room=rooms[i % 3 + 1], n_box=3) for i in range(3)]))

    def run():
        torch.manual_seed(0)
        model, crit, opt = harness.build_model(cfg, "cuda")
        out = []
        for it in range(36):
            b = harness.to_device(scenes[it % len(scenes)], "cuda")
            loss, _ = harness.train_step(model, crit, opt, b, cfg)
            out.append(float(loss))
        return out
    a, b = run(), run()
    assert not any(math.isnan(x) for x in a)
    assert a == b


@pytest.mark.experimental
def test_graph_replay_of_the_op_list_equals_eager_launches(monkeypatch):
    """WSIS_GRAPH=16: the executor records its launches (dW side stream included) into HIP graphs of ~16 ops and
    replays them; loss and every gradient must be EQUAL to the eagerly launched pass, also for a second scene of a
    different size that goes through hipGraphExecUpdate / re-instantiation."""
    cfg = harness.default_cfg()
    res = {}
    for mode in ("0", "16"):
        monkeypatch.setenv("WSIS_GRAPH", mode)
        model, crit, opt = harness.build_model(cfg, "cuda")
        out = []
        for seed, room in ((21, (1.8, 1.4, 1.1)), (22, (1.5, 1.2, 1.0)), (21, (1.8, 1.4, 1.1))):
            batch = harness.to_device(harness.collate([harness.make_scene(seed, room=room, n_box=2)]), "cuda")
            model.zero_grad(set_to_none=True)
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
            loss.backward()
            out.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
        res[mode] = out
    for (l0, g0), (l1, g1) in zip(res["0"], res["16"]):
        assert torch.equal(l0, l1)
        assert [n for n in g0 if not torch.equal(g0[n], g1[n])] == []


def test_rulebook_prefetcher_builds_the_same_pyramid_in_the_background():
    """spconv.ops.RulebookPrefetcher (helper thread + side stream) against the inline build: identical tables"""
    import spconv
    from spconv import ops
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([harness.make_scene(31, room=(1.6, 1.3, 1.0), n_box=2)]), "cuda")
    idx, shape = batch["voxel_coords_int"], batch["spatial_shape"]
    pre = ops.RulebookPrefetcher(5)
    pre.submit(idx, shape, batch.get("coords_ready_event"))
    rs = pre.result()
    t = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device="cuda"), idx, shape, 1)
    rs.attach(t)
    ref = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device="cuda"), idx, shape, 1)
    ops.prebuild_unet_rulebooks(ref, 5)
    torch.cuda.synchronize()
    assert set(t.indice_dict) == set(ref.indice_dict) and len(t.indice_dict) == 9
    for k, rb in ref.indice_dict.items():
        other = t.indice_dict[k]
        for name in ("nbr", "nbr_up", "order", "order_up", "nbr_p", "nbr_up_p", "out_indices"):
            a, b = getattr(rb, name, None), getattr(other, name, None)
            assert (a is None) == (b is None), (k, name)
            if a is not None:
                assert torch.equal(a, b), (k, name)
    # a forward pass on the attached tensor finds every key and builds nothing
    ops.prebuild_unet_rulebooks(t, 5)
    assert all(t.indice_dict[k] is rs.indice_dict[k] for k in rs.indice_dict)


def test_gradsync_allreduces_the_flat_unet_gradient_buffer_in_place():
    """single-rank RCCL process group: the native UNet pass leaves its parameter gradients in one dense buffer and
    parallel.GradSync all-reduces that buffer without flatten / copy-back; gradients are unchanged at world 1"""
    import torch.distributed as dist
    import wsis_parallel as parallel
    if dist.is_initialized():
        pytest.skip("process group already initialised in this process")
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([harness.make_scene(32, room=(1.5, 1.2, 1.0), n_box=2)]), "cuda")
    model, crit, opt = harness.build_model(cfg, "cuda")
    dist.init_process_group("nccl", rank=0, world_size=1, init_method="tcp://127.0.0.1:29631")
    try:
        gs = parallel.GradSync(model)
        gs.world = 2                      # exercise the collective + averaging code path with one rank
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
        loss.backward()
        before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        gs(model)
        torch.cuda.synchronize()
        assert gs.last_flat_params == len(model._native_prog.params) > 100
        for n, p in model.named_parameters():
            if p.grad is not None:     # sum over one rank, divided by the pretended world of 2
                assert torch.allclose(p.grad, before[n] / 2, rtol=0, atol=0), n
        # second step: the native pass now leaves room behind its gradients and the remaining parameters'
        # gradients travel in the same (single) collective
        assert model._native_prog.tail_floats > 0
        opt.zero_grad(set_to_none=True)
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
        loss.backward()
        before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert model._native_prog.flat_tail is not None
        gs(model)
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            if p.grad is not None:
                assert torch.allclose(p.grad, before[n] / 2, rtol=0, atol=0), n
        # third call freezes the collective plan; from then on the first ~half of the flat buffer is exchanged from
        # INSIDE the backward pass (milestone of wsis_run_ops_marked) on the communication stream
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
            loss.backward()
            gs(model)
        want = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert gs.enable_overlap(model) and gs.ready()      # (GradSync switches it on by itself once the plan is frozen)
        early0 = getattr(gs, "early_count", 0)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
            loss.backward()
            assert gs._early is not None and 0 < gs._early[1].numel() < model._native_prog.flat_grad.numel()
            gs(model)
            torch.cuda.synchronize()
            for n, p in model.named_parameters():
                if p.grad is not None:
                    assert torch.equal(p.grad, want[n]), n
        assert gs.early_count - early0 == 2
    finally:
        dist.destroy_process_group()


def test_native_unet_input_gradient_matches_module_walk(monkeypatch):
    """need_dx path of the executor (features that require grad): dX of input_conv equal to the module walk's"""
    import numpy as np
    monkeypatch.setenv("WSIS_FUSE_BN_STATS", "0")     # the modules compute their statistics in a separate pass
    import spconv
    import unet_native
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([harness.make_scene(33, room=(1.4, 1.2, 1.0), n_box=2)]), "cuda")
    model, _, _ = harness.build_model(cfg, "cuda")
    idx, shape = batch["voxel_coords_int"], batch["spatial_shape"]
    M = idx.shape[0]
    x0 = torch.randn(M, model.input_channel, device="cuda")
    outs = []
    for native in (False, True):
        x = x0.clone().requires_grad_(True)
        t = spconv.SparseConvTensor(x, idx, shape, 1)
        if native:
            y = unet_native.run_unet(model, t)
        else:
            spconv.ops.prebuild_unet_rulebooks(t, model.blocks)
            y = model.output_layer(model.unet(model.input_conv(t))).features
        model.zero_grad(set_to_none=True)
        (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
        outs.append((y.detach().clone(), x.grad.clone(), model.input_conv[0].weight.grad.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


def test_rulebook_pipeline_slices_give_the_inline_pyramid_and_the_same_step():
    """spconv.ops.RulebookPipeline (chain advanced between the phases of a step, no helper thread): same tables as
    the inline build, and a training step fed by it produces the same loss as the inline step"""
    import spconv
    from spconv import ops
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([harness.make_scene(34, room=(1.6, 1.3, 1.0), n_box=2)]), "cuda")
    idx, shape = batch["voxel_coords_int"], batch["spatial_shape"]
    pipe = ops.RulebookPipeline(5)
    pipe.start(idx, shape, batch.get("coords_ready_event"))
    pipe.pump()
    rs = pipe.finish()
    ref = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device="cuda"), idx, shape, 1)
    ops.prebuild_unet_rulebooks(ref, 5)
    torch.cuda.synchronize()
    for k, rb in ref.indice_dict.items():
        for name in ("nbr_p", "nbr_up_p", "order", "order_up", "out_indices"):
            a, b = getattr(rb, name, None), getattr(rs.indice_dict[k], name, None)
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (k, name)
    losses = []
    for use_pipe in (False, True):
        model, crit, opt = harness.build_model(cfg, "cuda")
        b = dict(batch)
        p = harness.make_pipeline(model) if use_pipe else None
        if p is not None:
            harness.start_rulebooks(p, b)
            b["rulebooks"] = p.finish()
            harness.start_rulebooks(p, b)
        loss, _ = harness.train_step(model, crit, opt, b, cfg, pipeline=p)
        if p is not None:
            b["rulebooks"] = p.finish()
        loss2, _ = harness.train_step(model, crit, opt, b, cfg)
        losses.append((float(loss), float(loss2)))
    assert losses[0] == losses[1]


def test_augmented_cropped_batch_from_the_reference_pipeline_matches_oracle():
    """The reference's host pipeline (datasets.ScenePrep: jitter/flip/rotation, crop, id re-compaction, graph
    restriction; datasets.collate_fn) feeds the HIP path; forward tensors and the loss against the CPU oracle."""
    import wsis_datasets as datasets
    cfg = harness.default_cfg()
    cfg.batch_size = 2
    scenes = [harness.make_scene(5 + i, room=(1.0, 0.9, 0.8), n_box=2) for i in range(2)]
    prep = datasets.ScenePrep(max_npoint=11000, aug=True, seed=4)
    batch_host = datasets.collate_fn([prep(*datasets.synthetic_scene_to_reference_format(sc)) for sc in scenes])
    assert int(batch_host["offsets"][-1]) < sum(len(sc["xyz"]) for sc in scenes)          # the crop removed points
    # stage-3 targets the synthetic graph carries raw; -inf/NaN-free after the crop
    assert torch.isfinite(batch_host["superpoint_instance_voxel_num"]).all()
    model, crit, opt = harness.build_model(cfg, "cuda")
    ref = network_ref.RefNetwork()
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    batch = harness.to_device(batch_host, "cuda")
    model.train(); ref.train()
    loss, ret = harness.forward_loss(model, crit, batch, cfg)
    loss.backward()
    r_loss, r_ret = network_ref.forward_loss_cpu(ref, crit, batch_host)
    for k in ("semantic_scores", "sp_semantic_scores", "pred_sp_offset_vectors", "edge_affinity",
              "sp_discriminative_feats"):
        assert ret[k].shape == r_ret[k].shape, k
        assert _rel(ret[k], r_ret[k]) < 2e-3, (k, _rel(ret[k], r_ret[k]))
    assert abs(float(loss) - float(r_loss)) < 2e-3 * abs(float(r_loss))
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@pytest.mark.parametrize("n_scenes", [1, 3])
def test_batched_tile_order_equals_the_per_table_orders(monkeypatch, n_scenes):
    """wsis_tile_order_batch (all 13 tables of the pyramid from one sort, table number in the top key bits, batched
    tile scheduling) against wsis_tile_order called table by table: identical orders and packed tables."""
    import spconv
    from spconv import ops
    scenes = [harness.make_scene(40 + i, room=(1.8, 1.5, 1.1), n_box=2) for i in range(n_scenes)]
    batch = harness.to_device(harness.collate(scenes), "cuda")
    idx, shape = batch["voxel_coords_int"], batch["spatial_shape"]
    assert idx.shape[0] // 128 >= 150                      # level 0 is large enough for the tile scheduling

    def build(flag, batch_size):
        monkeypatch.setenv("WSIS_TILE_BATCH", flag)
        t = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device="cuda"), idx, shape, batch_size)
        ops.prebuild_unet_rulebooks(t, 5)
        torch.cuda.synchronize()
        return t

    one, per = build("1", n_scenes), build("0", n_scenes)
    far = build("1", 17)                                   # batch_size > 16: the batched form steps aside
    assert len(one.indice_dict) == 9
    for other in (per, far):
        for k, rb in one.indice_dict.items():
            for name in ("order", "order_up", "nbr_p", "nbr_up_p"):
                a, b = getattr(rb, name, None), getattr(other.indice_dict[k], name, None)
                assert (a is None) == (b is None), (k, name)
                if a is not None:
                    assert torch.equal(a, b), (k, name)
    # every order is a permutation of its rows
    for k, rb in one.indice_dict.items():
        for o in (rb.order, rb.order_up):
            if o is not None:
                assert torch.equal(torch.sort(o.long())[0], torch.arange(o.numel(), device="cuda"))


@pytest.mark.gpu
def test_rulebooks_sized_from_host_counts_equal_the_read_back_build(monkeypatch):
    """prebuild_unet_rulebooks with the batch's host-side ``level_counts`` (no device read-back, no host stop) builds the
    tables of the default path bit for bit; the device counts are verified at the next build, and a wrong hint is
    reported there."""
    import spconv
    from spconv import ops
    import wsis_native as _n
    bt = harness.to_device(harness.collate([harness.make_scene(17, room=(2.0, 1.7, 1.2), n_box=3),
                                            harness.make_scene(18, room=(1.6, 1.3, 1.0), n_box=2)]), "cuda")
    shape, idx = bt["spatial_shape"], bt["voxel_coords_int"]
    feats = torch.zeros(idx.shape[0], 1, device="cuda")

    def build(counts):
        t = spconv.SparseConvTensor(feats, idx, shape, 2)
        if counts is not None:
            t._level_counts = counts
        ops.prebuild_unet_rulebooks(t, 5)
        torch.cuda.synchronize()
        return t.indice_dict

    ref = build(None)
    assert len(bt["level_counts"]) == 4
    hinted = build(bt["level_counts"])
    assert len(ops._PENDING_COUNTS) == 4
    for key, rb in ref.items():
        other = hinted[key]
        for name in ("nbr", "nbr_up", "order", "order_up", "nbr_p", "nbr_up_p", "out_indices"):
            a, b = getattr(rb, name, None), getattr(other, name, None)
            assert (a is None) == (b is None), (key, name)
            if a is not None:
                assert torch.equal(a, b), (key, name)
    ops.verify_pending_counts()
    assert not ops._PENDING_COUNTS
    wrong = list(bt["level_counts"])
    wrong[2] -= 1
    build(wrong)
    with pytest.raises(_n.WsisError):
        ops.verify_pending_counts()


@pytest.mark.gpu
def test_branch_stream_gives_the_results_of_one_stream(monkeypatch):
    """the filter net and the point-level head on the rulebook side stream (WSIS_BRANCH=1, the default; their backward
    follows them there) against everything on the current stream (WSIS_BRANCH=0): the same kernels on the same inputs, so
    every loss of 8 optimizer steps over scenes of three sizes and every final parameter must be EQUAL -- a missed
    cross-stream dependency shows up here as a difference (or as a NaN)"""
    cfg = harness.default_cfg()
    rooms = [(3.0, 2.5, 2.4), (1.8, 1.4, 1.1), (4.2, 3.1, 2.5)]
    scenes = [harness.collate([harness.make_scene(500 + i, room=r, n_box=3)]) for i, r in enumerate(rooms)]

    def run(flag):
        monkeypatch.setenv("WSIS_BRANCH", flag)
        torch.manual_seed(0)
        model, crit, opt = harness.build_model(cfg, "cuda")
        out = []
        for it in range(8):
            b = harness.to_device(scenes[it % len(scenes)], "cuda")
            loss, _ = harness.train_step(model, crit, opt, b, cfg)
            out.append(float(loss))
        torch.cuda.synchronize()
        return out, {k: v.detach().clone() for k, v in model.state_dict().items()}

    la, pa = run("1")
    lb, pb = run("0")
    lc, pc = run("1")
    assert la == lb == lc and all(x == x for x in la)
    assert [k for k in pa if not torch.equal(pa[k], pb[k])] == []
    assert [k for k in pa if not torch.equal(pa[k], pc[k])] == []


def test_unet_gradients_accumulate_and_follow_requires_grad():
    """the UNet's parameters are not inputs of its autograd node (model/unet_native.py): its backward pass stores the
    gradients in ``.grad`` itself.  The semantics of autograd must hold all the same: a second backward pass without
    ``zero_grad`` ADDS to what is there (exactly: the two passes are identical, so every gradient doubles), a parameter
    with ``requires_grad=False`` gets none while its neighbours keep theirs, and the fast path (gradients as views of the
    program's persistent buffer) comes back once the gradients are cleared."""
    cfg, batch_host, model, crit, opt, _ = _setup(1, 31, (1.5, 1.2, 1.0))
    batch = harness.to_device(batch_host, "cuda")
    model.train()

    def grads():
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
        loss.backward()
        return {n: p.grad for n, p in model.named_parameters() if p.grad is not None}

    model.zero_grad(set_to_none=True)
    g1 = {n: g.clone() for n, g in grads().items()}
    unet_names = [n for n in g1 if n.startswith(("unet.", "input_conv.", "output_layer."))]
    assert len(unet_names) > 100
    prog = model._native_prog
    lo, hi = prog.flat_grad.data_ptr(), prog.flat_grad.data_ptr() + prog.flat_grad.numel() * 4
    params = dict(model.named_parameters())
    assert all(lo <= params[n].grad.data_ptr() < hi for n in unet_names)             # views of the flat buffer
    g2 = grads()                                                                       # no zero_grad: accumulate
    for n in g1:
        assert torch.equal(g2[n], g1[n] + g1[n]), n
    assert not any(lo <= params[n].grad.data_ptr() < hi for n in unet_names)           # (a buffer of their own now)
    # frozen parameter
    model.zero_grad(set_to_none=True)
    frozen = unet_names[len(unet_names) // 2]
    params[frozen].requires_grad_(False)
    g3 = grads()
    assert frozen not in g3
    for n in g1:
        if n != frozen:
            assert torch.equal(g3[n], g1[n]), n
    params[frozen].requires_grad_(True)
    model.zero_grad(set_to_none=True)
    g4 = grads()
    for n in g1:
        assert torch.equal(g4[n], g1[n]), n
    lo, hi = prog.flat_grad.data_ptr(), prog.flat_grad.data_ptr() + prog.flat_grad.numel() * 4
    assert all(lo <= params[n].grad.data_ptr() < hi for n in unet_names)


def test_unet_gradient_buffer_aliasing_contract_and_opt_out():
    """INTEGRATION "Differences": with the default ``prog.persistent_grads = True`` the UNet's ``.grad`` tensors are
    views of one buffer that the NEXT backward pass overwrites after ``zero_grad(set_to_none=True)`` -- a gradient the
    caller kept from the previous step (logging, clipping snapshots, manual accumulation) changes under it unless it
    was cloned.  ``prog.persistent_grads = False`` (``WSIS_PERSISTENT_GRADS=0``) gives every pass a buffer of its own:
    the kept tensor keeps its values, the new gradients are the same bits."""
    cfg, batch_host, model, crit, opt, _ = _setup(1, 37, (1.4, 1.1, 0.9))
    batch_a = harness.to_device(batch_host, "cuda")
    sc_b = harness.make_scene(38, room=(1.3, 1.2, 0.9), n_box=2)
    batch_b = harness.to_device(harness.collate([sc_b]), "cuda")
    model.train()
    prog_name = next(n for n, _ in model.named_parameters() if n.startswith("unet."))
    par = dict(model.named_parameters())[prog_name]

    def backward(batch):
        model.zero_grad(set_to_none=True)
        loss, _ = harness.forward_loss(model, crit, batch, cfg)
        loss.backward()
        return par.grad

    kept = backward(batch_a)                   # NOT cloned
    copy_a = kept.clone()
    new = backward(batch_b)
    assert not torch.equal(new, copy_a)        # a different batch: a different gradient
    assert kept.data_ptr() == new.data_ptr() and torch.equal(kept, new)       # the kept tensor was overwritten
    prog = model._native_prog
    prog.persistent_grads = False
    try:
        kept = backward(batch_a)
        assert torch.equal(kept, copy_a)
        new2 = backward(batch_b)
        assert kept.data_ptr() != new2.data_ptr()
        assert torch.equal(kept, copy_a)       # survives the next pass
        assert torch.equal(new2, new)          # and the pass computes the same bits
    finally:
        prog.persistent_grads = True


def test_warm_streams_is_idempotent_and_leaves_results_alone():
    """wsis_parallel.warm_streams() (what init_distributed runs before it creates a process group: every stream of a
    step takes its hardware queue first) can be called at any time, any number of times"""
    import wsis_parallel
    cfg, batch_host, model, crit, opt, _ = _setup(1, 33, (1.2, 1.0, 0.8))
    batch = harness.to_device(batch_host, "cuda")
    model.train()
    wsis_parallel.warm_streams()
    l0, _ = harness.forward_loss(model, crit, batch, cfg)
    wsis_parallel.warm_streams()
    wsis_parallel.warm_streams("cuda:0")
    l1, _ = harness.forward_loss(model, crit, batch, cfg)
    assert torch.equal(l0, l1)


def test_error_exit_orders_the_callers_stream_behind_the_forked_weight_transposes(monkeypatch):
    """A pass forks its weight transposes to the library's side stream and makes the caller's stream wait for them in
    front of their first reader.  A pass that fails BEFORE that reader must wait all the same (PassRun::finish): the
    caller hands the workspace back to the allocator next, and the side stream is still writing into it.  Op 0 is of an
    unknown kind (sized as zero bytes, refused when it is issued); ops 1 and 2 are forward convolutions on the kernel
    that reads B^T.  After the failed call only the CALLER's stream is synchronised: op 1's slot must hold W^T."""
    import ctypes
    import unet_native as un
    import wsis_native as _n
    from spconv import ops as sp_ops
    for k in ("WSIS_WT_SIDE", "WSIS_DW_STREAM", "WSIS_FWD2"):
        monkeypatch.delenv(k, raising=False)
    lib = _n.hip()
    dev = torch.device("cuda", 0)
    K, C, M = 27, 32, 64            # 64 rows: two 32-row slices
    rng = np.random.default_rng(5)
    shape = (8, 8, 4)
    occ = np.stack(np.unravel_index(np.sort(rng.permutation(int(np.prod(shape)))[:M]), shape), 1)
    idx = torch.from_numpy(np.concatenate([np.zeros((M, 1), np.int64), occ], 1).astype(np.int32)).to(dev)
    caller = torch.cuda.Stream(dev)
    with torch.cuda.stream(caller):
        rb = sp_ops.build_subm_rulebook(idx, shape, [3, 3, 3], [1, 1, 1])
        X = torch.randn(M, C, device=dev)
        W = [torch.randn(K, C, C, device=dev) for _ in range(2)]
        Y = [torch.empty(M, C, device=dev) for _ in range(2)]
        want = W[0].transpose(1, 2).contiguous()          # [K, Cout, Cin]
        ops = np.zeros(3, dtype=un.OP_DTYPE)
        ops["kind"][0] = 99
        for j in (1, 2):
            ops["kind"][j], ops["M_in"][j], ops["M_out"][j] = un.OP_CONV, M, M
            ops["K"][j], ops["Cin"][j], ops["Cout"][j] = K, C, C
            ops["inp"][j, :4] = [X.data_ptr(), rb.nbr_p.data_ptr(), _n.ptr(rb.order) or 0, W[j - 1].data_ptr()]
            ops["out"][j, 0] = Y[j - 1].data_ptr()
        layout = lib.wsis_debug_run_ops_layout
        layout.restype = ctypes.c_int32
        layout.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        plan = np.zeros(11 + 2 * 3, dtype=np.int64)
        assert layout(ops.ctypes.data, 3, plan.ctypes.data) == 0
        total, wt_at, wt_off = int(plan[10]), int(plan[2]), plan[11 + 3:]
        assert total == lib.wsis_run_ops_workspace_bytes(ops.ctypes.data, 3)
        assert wt_off[0] == -1 and wt_off[1] == 0 and wt_off[2] == K * C * C * 4, "ops 1 and 2 read a transposed weight"
        ws = torch.zeros(total, dtype=torch.uint8, device=dev)
        sync = _n.sync_block(dev)
        rc = lib.wsis_run_ops(ops.ctypes.data, 3, ws.data_ptr(), total, sync.data_ptr(), _n.stream_ptr())
        assert rc == -1 and "unknown op kind" in lib.wsis_last_error().decode()        # WSIS_ERR_ARG, from host code
        caller.synchronize()                                # the caller's stream ONLY
        a = wt_at + int(wt_off[1])
        got = ws[a:a + K * C * C * 4].view(torch.float32).reshape(K, C, C)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
