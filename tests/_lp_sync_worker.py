"""Child process of tests/test_gpu_lowp_sync_ranks.py: ONE rank of a world of two, both on cuda:0, process group on gloo
(the environment of tests/test_gpu_two_ranks.py).  Runs every scenario of the synced 16-bit native training pass
(WSIS_NATIVE_LP_TRAIN=1 + WSIS_NATIVE_LP_SYNC=1) in this one launch on smoke-size scenes and saves what the parent
compares; tensors that are only compared for equality are saved as SHA-1 digests of their bytes.

    python tests/_lp_sync_worker.py <out_dir>      (RANK / WORLD_SIZE / MASTER_* from the environment)

  g  BatchNorm not converted: two optimizer steps of the 16-bit pass with GradSync alone (bf16; fp16 with LossScaler)
  d  the SAME scene on both ranks: the unsynced 16-bit pass, then -- the UNet's BatchNorm layers converted -- the synced one
  e  a different scene per rank, whole model converted: synced 16-bit native pass, synced 16-bit module walk, synced fp32
     native pass of the UNet with one fixed output gradient
  f  whole model converted: two optimizer steps with GradSync (bf16; fp16 with LossScaler)
"""
import hashlib
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import harness  # noqa: E402
import spconv  # noqa: E402
import unet_native as un  # noqa: E402
import wsis_ops  # noqa: E402
import wsis_optim  # noqa: E402
import wsis_parallel as parallel  # noqa: E402
from spconv import ops as sp_ops  # noqa: E402

DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))
UNET = ("input_conv.", "unet.", "output_layer.")


def digest(t):
    return hashlib.sha1(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def snapshot(model):
    wsis_ops.flush_bn_counters(model)
    return {k: v.clone() for k, v in model.state_dict().items()}


def restore(model, state):
    wsis_ops.flush_bn_counters(model)
    model.load_state_dict(state)
    for p in model.parameters():
        p.grad = None


def perturb_bn(model, dev):
    """affine BatchNorm parameters that are not the initial ones (same seed, same values on every rank)"""
    g = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d) and m.weight is not None:
                C = m.num_features
                m.weight.copy_(torch.rand(C, device=dev, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, device=dev, generator=g) * 0.1)


def unet_input(batch, cfg):
    import pointgroup_ops
    feats = batch["feats"]
    if cfg.model.use_coords:
        feats = torch.cat((feats, batch["locs_float"]), 1)
    vf = pointgroup_ops.voxelization(feats, batch["v2p_map"], cfg.mode)
    return spconv.SparseConvTensor(vf, batch["voxel_coords_int"], batch["spatial_shape"], max(int(cfg.batch_size), 1))


def fwd_bwd(model, crit, batch, cfg, dt):
    """one forward + backward of the whole Network under autocast -> what (d) compares, with the UNet's output captured
    where Network.forward receives it"""
    seen = []
    orig = un.run_unet_lp_train

    def capture(*a, **k):
        out = orig(*a, **k)
        seen.append(out.detach().clone())
        return out
    un.run_unet_lp_train = capture
    try:
        with torch.autocast("cuda", dtype=dt):
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
    finally:
        un.run_unet_lp_train = orig
    for p in model.parameters():
        p.grad = None
    loss.backward()
    torch.cuda.synchronize()
    prog = model._native_prog
    grads = {n: p.grad for n, p in model.named_parameters() if n.startswith(UNET)}
    assert len(seen) == 1 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    return {"loss": loss.detach().cpu(), "out": seen[0].cpu(), "grads": {n: digest(g) for n, g in grads.items()},
            "last_pass": model.last_pass, "bn_sync": prog.bn_sync is not None}


def two_steps(cfg, dev, batch, dt, converted):
    """(f) / (g): a fresh model (same seed on every rank), two optimizer steps of the 16-bit pass with GradSync"""
    model, crit, opt = harness.build_model(cfg, dev)
    for t in list(model.parameters()) + list(model.buffers()):
        dist.broadcast(t.data, 0)
    if converted:
        parallel.convert_sync_batchnorm(model)
        assert parallel.sync_batchnorm_active(model)
    model.train()
    sync = parallel.GradSync(model)
    scaler = wsis_optim.LossScaler(device=dev) if dt == torch.float16 else None
    losses, passes = [], []
    for _ in range(2):
        harness.build_batch_graphs(batch)
        with torch.autocast("cuda", dtype=dt):
            loss, _ = harness.forward_loss(model, crit, batch, cfg)
        passes.append(model.last_pass)
        opt.zero_grad(set_to_none=True)
        (loss if scaler is None else scaler.scale(loss)).backward()
        sync(model)
        opt.set_grad_clamp(list(model.ecc.parameters()), 1.0)      # train_scannetv2.py:247-249, as harness.train_step
        if scaler is None:
            opt.step()
        else:
            scaler.step(opt)
            scaler.update()
        losses.append(float(loss))
    torch.cuda.synchronize()
    prog = model._native_prog
    wsis_ops.flush_bn_counters(model)
    return {"losses": losses, "passes": passes, "bn_sync": prog.bn_sync is not None, "flat_params": sync.last_flat_params,
            "n_unet_params": len(prog.params), "weights": {n: digest(p) for n, p in model.named_parameters()},
            "stats": {n: digest(b) for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))}}


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def one_minus_cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(1.0 - (a @ b) / (a.norm() * b.norm()))


def three_passes(model, state, batch, cfg, dt, group, G):
    """(e): errors of the synced 16-bit native pass and of the synced 16-bit module walk against the synced fp32 native pass"""
    params = un._program(model).params
    ms = {}

    def run(kind):
        restore(model, state)
        inp = unet_input(batch, cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "fp32":
            out = un.run_unet(model, inp, sync_group=group)
        elif kind == "native":
            out = un.run_unet_lp_train(model, inp, dt, dt, sync_group=group)
        else:
            with torch.autocast("cuda", dtype=dt):
                out = model.output_layer(model.unet(model.input_conv(inp))).features
            sp_ops.verify_pending_counts()
        out.backward(G.to(out.dtype))
        torch.cuda.synchronize()
        ms[kind] = (time.perf_counter() - t0) * 1e3
        return out.detach().clone(), [p.grad.detach().clone().float() for p in params]
    for kind in ("fp32", "native", "walk"):      # (first calls: compilation of the programs, allocator growth -- not timed)
        run(kind)
    o32, g32 = run("fp32")
    o_n, g_n = run("native")
    o_w, g_w = run("walk")
    assert model._native_prog.bn_sync is not None
    c_n = np.array([one_minus_cos(a, b) for a, b in zip(g_n, g32)])
    c_w = np.array([one_minus_cos(a, b) for a, b in zip(g_w, g32)])
    return {"out_native": rel(o_n, o32), "out_walk": rel(o_w, o32), "grad_native": float(np.median(c_n)),
            "grad_walk": float(np.median(c_w)), "grad_worst_native": float(c_n.max()), "grad_worst_walk": float(c_w.max()),
            "ms_native": ms["native"], "ms_walk": ms["walk"], "ms_fp32": ms["fp32"]}


def main():
    out_dir = sys.argv[1]
    rank, _, world = parallel.init_distributed()
    assert world == 2 and dist.get_backend() == "gloo"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = harness.default_cfg()
    same = harness.to_device(harness.collate([harness.make_scene(0, room=(1.2, 1.0, 0.8), n_box=1)]), dev)
    own = harness.to_device(harness.collate([harness.make_scene(11 + rank, room=(1.2 + 0.3 * rank, 1.0, 0.8), n_box=1)]), dev)
    res = {"rank": rank, "voxels_same": int(same["voxel_locs"].shape[0]), "voxels_own": int(own["voxel_locs"].shape[0])}
    os.environ["WSIS_NATIVE_LP_TRAIN"] = "1"
    os.environ.pop("WSIS_NATIVE_LP_SYNC", None)
    os.environ.pop("WSIS_NATIVE_UNET", None)

    # (g) BatchNorm not converted
    for name, dt in DTYPES:
        res["g_" + name] = two_steps(cfg, dev, own, dt, converted=False)

    # (d) the same scene on both ranks
    model, crit, _ = harness.build_model(cfg, dev)
    for t in list(model.parameters()) + list(model.buffers()):
        dist.broadcast(t.data, 0)
    perturb_bn(model, dev)
    model.train()
    state = snapshot(model)
    for name, dt in DTYPES:
        restore(model, state)
        res["d_unsynced_" + name] = fwd_bwd(model, crit, same, cfg, dt)
    # the UNet's layers only: what lies behind the UNet (heads, GNN) then computes the same function of the UNet's output
    # in both runs, so the loss and the gradient arriving at the UNet are equal exactly when the UNet's output is
    parallel.convert_sync_batchnorm(model.unet)
    parallel.convert_sync_batchnorm(model.output_layer)
    assert parallel.sync_batchnorm_active(model)
    os.environ["WSIS_NATIVE_LP_SYNC"] = "1"
    for name, dt in DTYPES:
        restore(model, state)
        res["d_synced_" + name] = fwd_bwd(model, crit, same, cfg, dt)

    # (e) different scenes, the whole model converted
    parallel.convert_sync_batchnorm(model)
    rows = int(unet_input(own, cfg).features.shape[0])
    G = torch.randn((rows, model.output_layer[0].num_features), device=dev,
                    generator=torch.Generator(device=dev).manual_seed(11 + rank)) * 0.01
    for name, dt in DTYPES:
        res["e_" + name] = three_passes(model, state, own, cfg, dt, dist.group.WORLD, G)
    restore(model, state)

    # (f) two optimizer steps, the whole model converted
    for name, dt in DTYPES:
        res["f_" + name] = two_steps(cfg, dev, own, dt, converted=True)

    torch.save(res, os.path.join(out_dir, f"lp_sync{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
