"""Evaluation-mode forward under torch.no_grad in 16 bits: the native 16-bit pass (WSIS_NATIVE_LP=1) against the 16-bit
module walk and the fp32 native pass, on the C2 scene (harness.bench_scene(1)) and the C4 room (bench.py's inference
config).  For each scene and mode: the UNet alone (input_conv -> unet -> output_layer: unet_native.run_unet /
run_unet_lp, or the walk of the three modules on 16-bit features) and the whole harness.forward_loss (16-bit modes under
torch.autocast); device-event time per call (median of --iters after --warmup) and torch.cuda.max_memory_allocated
(absolute, and above what was allocated in front of the call).  The model first takes --train-steps fp32 training steps
on the C2 scene, so that the running statistics are not the initial ones.

    python tools/lowp_infer_bench.py [--iters 30] [--warmup 5] [--out profiles/lowp_infer_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")

import torch  # noqa: E402

import harness  # noqa: E402
import spconv  # noqa: E402
import unet_native  # noqa: E402

SCENES = {"c2": dict(seed=1), "c4": dict(seed=5, room=(13.0, 10.0, 3.0), n_box=36)}
MODES = ("fp32_native", "bf16_walk", "bf16_native_lp", "fp16_walk", "fp16_native_lp")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _input(batch, cfg, dtype=None):
    import pointgroup_ops
    feats = batch["feats"]
    if cfg.model.use_coords:
        feats = torch.cat((feats, batch["locs_float"]), 1)
    vf = pointgroup_ops.voxelization(feats, batch["v2p_map"], cfg.mode)
    if dtype is not None:
        vf = vf.to(dtype)
    return spconv.SparseConvTensor(vf, batch["voxel_coords_int"], batch["spatial_shape"], max(int(cfg.batch_size), 1))


def measure(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return {"ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "n": iters,
            "peak_mib": round(peak / 2 ** 20, 1), "above_start_mib": round((peak - before) / 2 ** 20, 1)}


def unet_fn(model, batch, cfg, mode):
    if mode == "fp32_native":
        inp = _input(batch, cfg)
        return lambda: unet_native.run_unet(model, inp)
    prec, kind = mode.split("_", 1)
    dt = DT[prec]
    if kind == "walk":
        inp = _input(batch, cfg, dt)
        spconv.ops.prebuild_unet_rulebooks(inp, model.blocks)

        def walk():
            out = model.output_layer(model.unet(model.input_conv(inp))).features
            spconv.ops.verify_pending_counts()
            return out
        return walk
    inp = _input(batch, cfg, dt)
    return lambda: unet_native.run_unet_lp(model, inp, dt, dt)


def loss_fn(model, crit, batch, cfg, mode):
    def run():
        if mode == "fp32_native":
            os.environ.pop("WSIS_NATIVE_LP", None)
            return harness.forward_loss(model, crit, batch, cfg)[0]
        prec, kind = mode.split("_", 1)
        if kind == "walk":
            os.environ.pop("WSIS_NATIVE_LP", None)
        else:
            os.environ["WSIS_NATIVE_LP"] = "1"
        with torch.autocast("cuda", dtype=DT[prec]):
            return harness.forward_loss(model, crit, batch, cfg)[0]
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowp_infer_bench.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "the median of at least 20 calls"
    cfg = harness.default_cfg()
    dev = "cuda"
    model, crit, opt = harness.build_model(cfg, dev)
    batches = {k: harness.to_device(harness.collate([harness.bench_scene(**kw)]), dev) for k, kw in SCENES.items()}
    for _ in range(args.train_steps):
        harness.train_step(model, crit, opt, batches["c2"], cfg)
    model.eval()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters,
           "warmup": args.warmup, "train_steps": args.train_steps, "scenes": {}}
    with torch.no_grad():
        for name, batch in batches.items():
            sc = res["scenes"][name] = {"voxels": int(batch["voxel_coords_int"].shape[0]), "unet": {}, "forward_loss": {}}
            for mode in MODES:
                sc["unet"][mode] = measure(unet_fn(model, batch, cfg, mode), args.warmup, args.iters)
                sc["forward_loss"][mode] = measure(loss_fn(model, crit, batch, cfg, mode), args.warmup, args.iters)
                assert model.last_pass == {"fp32_native": "native", "walk": "modules"}.get(
                    mode if mode == "fp32_native" else mode.split("_", 1)[1], "native_lp"), (mode, model.last_pass)
            os.environ.pop("WSIS_NATIVE_LP", None)
            print(f"{name}: {sc['voxels']} voxels")
            print(f"  {'mode':<16}{'UNet ms':>10}{'UNet MiB':>10}{'fwd+loss ms':>13}{'fwd+loss MiB':>14}")
            for mode in MODES:
                u, f = sc["unet"][mode], sc["forward_loss"][mode]
                print(f"  {mode:<16}{u['ms']:>10.3f}{u['above_start_mib']:>10.1f}{f['ms']:>13.3f}{f['above_start_mib']:>14.1f}")
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
