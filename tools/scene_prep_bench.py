"""Per-scene preparation on the MI355X (wsis_datasets.DeviceScenePrep, csrc/sceneprep.hip) against the host class
ScenePrep on this machine's host, one thread, on the C2 scene of bench.py (harness.bench_scene), seed 1, augmentation
on: once uncropped (max_npoint above the scene) and once cropped (--crop-max-npoint, default half the scene; the number of
crop rounds that takes is recorded -- the reference's window shrinks by 32 voxels a round from 512, so on a room of
230 x 180 voxels the first rounds keep every point).  Per case: median of --iters ``DeviceScenePrep.__call__`` between two
device events (the call ends with a read-back, so this is the item's wall time on the stream), the launches of the native
entry points and the read-backs the class counts, every device kernel of one call as torch's profiler sees it (null
where the profiler is not available), and ``ScenePrep.__call__`` on the host.  Both classes are re-seeded before every
call, so every call does the same work.  Not a test: no threshold.

``--elastic`` adds an ``elastic`` section: the same two cases under the same protocol with ``with_elastic=True`` on both
classes, and per device call the host time of drawing the six noise grids (``rng.randn`` inside the timed call, on a
host clock), their cell count, and the launches and read-backs the two elastic calls add.

    python tools/scene_prep_bench.py [--elastic] [--out profiles/scene_prep_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")

import torch  # noqa: E402

import harness  # noqa: E402
import wsis_datasets as datasets  # noqa: E402


def reseed(prep, seed):
    prep.rng.seed(seed)
    prep.gen.manual_seed(seed)


class TimedDraws(object):
    """a RandomState that clocks its three-dimensional ``randn`` draws: the noise grids of ``elastic``"""

    def __init__(self, rng):
        self._rng, self.seconds, self.cells = rng, 0.0, 0

    def randn(self, *shape):
        if len(shape) != 3:
            return self._rng.randn(*shape)
        t0 = time.perf_counter()
        out = self._rng.randn(*shape)
        self.seconds += time.perf_counter() - t0
        self.cells += out.size
        return out

    def __getattr__(self, name):
        return getattr(self._rng, name)


def device_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")))
    except Exception:
        return None


def run_cases(args, tup, graph, **kw):
    """the two cases with the constructor arguments ``kw`` on both classes"""
    N, cases = len(tup[0]), {}
    for name, max_npoint in (("uncropped", 250000 if N <= 250000 else N), ("cropped", args.crop_max_npoint or N // 2)):
        host = datasets.ScenePrep(max_npoint=max_npoint, aug=True, seed=args.seed, **kw)
        dev = datasets.DeviceScenePrep(max_npoint=max_npoint, aug=True, seed=args.seed, device="cuda", **kw)
        dev.rng = draws = TimedDraws(dev.rng)
        resident = dev.upload(tup, graph)
        times, draw_times = [], []
        for i in range(args.warmup + args.iters):
            reseed(dev, args.seed)
            draws.seconds, draws.cells = 0.0, 0
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            item = dev(resident)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
                draw_times.append(draws.seconds)
        stats = dict(dev.last_stats)
        reseed(dev, args.seed)
        kernels = device_kernels(lambda: dev(resident))
        host_times = []
        for _ in range(args.host_iters):
            reseed(host, args.seed)
            t0 = time.perf_counter()
            want = host(tup, graph)
            host_times.append(time.perf_counter() - t0)
        elastic_calls = len(dev.elastic_calls())
        cases[name] = {
            "max_npoint": int(max_npoint), "points_kept": int(item.n), "superpoints_kept": int(item.S),
            "crop_rounds": int(stats["readbacks"]) - 2 - elastic_calls,
            "device_ms_per_call": round(statistics.median(times), 4),
            "native_launches": int(stats["launches"]), "read_backs": int(stats["readbacks"]),
            "device_kernels_per_call_profiler": kernels,
            "host_ms_per_call_one_thread": round(statistics.median(host_times) * 1e3, 2),
            "same_points_as_host": bool(torch.equal(item.loc.cpu(), want[1])),
        }
        if elastic_calls:
            cases[name].update({
                "noise_cells_drawn_per_call": int(draws.cells),
                "host_ms_drawing_noise_per_call": round(statistics.median(draw_times) * 1e3, 3),
                "elastic_native_launches": 7 * elastic_calls, "elastic_read_backs": elastic_calls})
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--crop-max-npoint", type=int, default=0)
    ap.add_argument("--elastic", action="store_true", help="also measure both cases with with_elastic=True")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_prep_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_prep_bench needs the MI355X: a CPU run measures only the host class")
    torch.set_num_threads(1)
    sc = harness.bench_scene(args.seed)
    tup, graph = datasets.synthetic_scene_to_reference_format(sc)
    N = len(tup[0])
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "scene": {"points": int(N), "superpoints": int(graph.vcount), "edges": int(len(graph.edges)),
                     "instances": int(sc["n_inst"])}, "cases": {}}
    res["cases"] = run_cases(args, tup, graph)
    if args.elastic:
        res["elastic"] = run_cases(args, tup, graph, with_elastic=True)
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
