"""What the statistics exchange costs a native pass of the UNet, without a network: forward + backward of input_conv ->
unet -> output_layer on the C2 scene (harness.bench_scene(1)) in ONE process, with a world-of-one gloo group handed
straight to the run functions -- the 16-bit native training pass (bf16, fp16) and the fp32 native pass, each unsynced and
synced.  A world of one prices the parts of the op list (one wsis_run_ops_part call and workspace per part), the helper
launches of every layer and the collective's fixed cost (gloo stages device tensors through the host); it says nothing
about a network.

Per mode: device-event time and host time of the call (median of --iters after --warmup), and the device kernels of one
pass counted with torch.profiler; (synced - unsynced) / layers = the launches a synced layer adds, forward + backward.

    python tools/lp_sync_bench.py [--iters 30] [--warmup 5] [--out profiles/lp_sync_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import harness  # noqa: E402
import spconv  # noqa: E402
import unet_native  # noqa: E402

MODES = ("bf16_native_lp", "bf16_native_lp_synced", "fp16_native_lp", "fp16_native_lp_synced", "fp32_native",
         "fp32_native_synced")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _input(batch, cfg):
    import pointgroup_ops
    feats = batch["feats"]
    if cfg.model.use_coords:
        feats = torch.cat((feats, batch["locs_float"]), 1)
    vf = pointgroup_ops.voxelization(feats, batch["v2p_map"], cfg.mode)
    return spconv.SparseConvTensor(vf, batch["voxel_coords_int"], batch["spatial_shape"], max(int(cfg.batch_size), 1))


def pass_fn(model, batch, cfg, mode, group, G):
    inp = _input(batch, cfg)
    params = unet_native._program(model).params
    grp = group if mode.endswith("_synced") else None
    prec = mode.split("_", 1)[0]

    def run():
        for p in params:
            p.grad = None
        if prec == "fp32":
            out = unet_native.run_unet(model, inp, sync_group=grp)
        else:
            out = unet_native.run_unet_lp_train(model, inp, DT[prec], DT[prec], sync_group=grp)
        out.backward(G.to(out.dtype))
    return run


def kernels_of_one_pass(fn):
    """device kernels / device copies of one call (None where the profiler gives no device events)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        copies = sum(1 for e in dev if "memcpy" in e.name.lower())
        return (len(dev) - copies, copies) if dev else (None, None)
    except Exception as exc:      # noqa: BLE001 (a profiler that is not there is not this tool's subject)
        print("no kernel count:", exc)
        return None, None


def measure(fn, warmup, iters, count):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        b.record()
        b.synchronize()
        dev_ms.append(a.elapsed_time(b))
    kernels, copies = kernels_of_one_pass(fn) if count else (None, None)
    return {"ms": round(statistics.median(dev_ms), 4), "min_ms": round(min(dev_ms), 4),
            "host_ms": round(statistics.median(host_ms), 4), "n": iters, "kernels": kernels, "copies": copies}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-kernel-count", action="store_true", help="skip the torch.profiler pass")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_sync_bench.json"))
    args = ap.parse_args()
    cfg = harness.default_cfg()
    dev = "cuda"
    store = os.path.join(tempfile.mkdtemp(prefix="lp_sync_bench"), "store")
    dist.init_process_group("gloo", init_method="file://" + store, rank=0, world_size=1)
    model, _, _ = harness.build_model(cfg, dev)
    model.train()
    batch = harness.to_device(harness.collate([harness.bench_scene(1)]), dev)
    rows = int(batch["voxel_coords_int"].shape[0])
    G = torch.randn((rows, model.output_layer[0].num_features), device=dev,
                    generator=torch.Generator(device=dev).manual_seed(11)) * 0.01
    layers = len(unet_native._program(model).bns)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "scene": "c2", "voxels": rows, "bn_layers": layers, "world": 1, "backend": "gloo", "modes": {}}
    for mode in MODES:
        res["modes"][mode] = measure(pass_fn(model, batch, cfg, mode, dist.group.WORLD, G), args.warmup, args.iters,
                                     not args.no_kernel_count)
    print(f"c2: {rows} voxels, {layers} BatchNorm layers, forward + backward of the UNet, world of one (gloo)")
    print(f"  {'mode':<24}{'device ms':>11}{'host ms':>10}{'kernels':>9}{'copies':>8}{'+ per layer':>13}")
    for mode in MODES:
        m = res["modes"][mode]
        base = res["modes"].get(mode[:-len("_synced")]) if mode.endswith("_synced") else None
        if base is not None and m["kernels"] is not None and base["kernels"] is not None:
            m["kernels_per_layer_added"] = round((m["kernels"] - base["kernels"]) / layers, 2)
        extra = m.get("kernels_per_layer_added")
        print(f"  {mode:<24}{m['ms']:>11.3f}{m['host_ms']:>10.3f}{str(m['kernels']):>9}{str(m['copies']):>8}"
              f"{'' if extra is None else format(extra, '.2f'):>13}")
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
