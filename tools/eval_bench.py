"""Evaluation on the MI355X (3d-wsis_amd/wsis_eval.py, csrc/evalcount.hip) on the C2-shaped scene of harness.bench_scene:
about 100 predictions made by perturbing the ground-truth instances (a fifth of the points dropped, a twentieth added
elsewhere), masks held on the device as the int64 [n, N] tensor ``clustering_in_graph(as_tensor=True)`` returns.
Device-event time of one ``process`` call of each of the three evaluators (ids to columns, kernels, read-back of the
small tables and the host arithmetic of ``add_counts``) and of the two kernels alone; median of --iters calls after
--warmup.  The bytes wsis_mask_overlap reads once (P * N * element size + 4 N) over its time are set against the 8 TB/s
HBM peak.  The loop-per-pair numpy form of tests/eval_ref.py runs on the same inputs on this machine's host: the only
stand-in available here for the reference's evaluators.  Not a test: no threshold.

    python tools/eval_bench.py [--out profiles/eval_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
importlib.import_module("3d-wsis_amd")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_ref  # noqa: E402
import harness  # noqa: E402
import wsis_eval  # noqa: E402

HBM_PEAK = 8.0e12


def event_ms(fn, warmup, iters):
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
    return round(statistics.median(times), 4)


def host_ms(fn, iters=1):
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return round(statistics.median(times) * 1e3, 2)


def make_case(seed, n_pred):
    """ground truth: the scene's objects cut into 1 m cells (tens of instances), classes dealt round; predictions:
    perturbed instances in turn"""
    sc = harness.bench_scene(seed)
    rng = np.random.default_rng(seed)
    xyz, N = sc["xyz"], len(sc["xyz"])
    obj = np.unique(sc["sp_size"], return_inverse=True)[1].reshape(-1)[sc["superpoint"]]
    key = np.concatenate([obj[:, None], np.floor(xyz).astype(np.int64)], 1)
    inst = np.unique(key, axis=0, return_inverse=True)[1].reshape(-1)
    n_inst = int(inst.max()) + 1
    ids = np.array(wsis_eval.SCANNET_INSTANCE_CLASS_IDS)
    inst_cls = ids[np.arange(n_inst) % len(ids)]
    gt_ids = (inst_cls * 1000 + np.arange(n_inst) // len(ids) + 1)[inst]
    gt_ids[rng.random(N) < 0.03] = 0
    masks = np.zeros((n_pred, N), dtype=bool)
    label = np.zeros(n_pred, dtype=np.int64)
    for p in range(n_pred):
        j = p % n_inst
        idx = np.nonzero(inst == j)[0]
        masks[p, idx[rng.random(len(idx)) >= 0.2]] = True
        masks[p, rng.choice(N, len(idx) // 20, replace=False)] = True
        label[p] = inst_cls[j]
    sem_gt = (inst_cls[inst] % 13).astype(np.int64)
    sem_pred = np.where(rng.random(N) < 0.15, rng.integers(0, 13, N), sem_gt)
    return dict(masks=masks, conf=rng.random(n_pred), label=label, gt_ids=gt_ids.astype(np.int64), inst=inst.astype(np.int64),
                sem_gt=sem_gt, sem_pred=sem_pred, n_inst=n_inst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--predictions", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the MI355X: a CPU run measures nothing")
    c = make_case(args.seed, args.predictions)
    P, N = c["masks"].shape
    dev = "cuda"
    m64 = torch.from_numpy(c["masks"]).to(dev).to(torch.int64)
    m8 = torch.from_numpy(c["masks"]).to(dev).view(torch.uint8)
    gt_d, inst_d = torch.from_numpy(c["gt_ids"]).to(dev), torch.from_numpy(c["inst"]).to(dev)
    sem_gt_d, sem_pred_d = torch.from_numpy(c["sem_gt"]).to(dev), torch.from_numpy(c["sem_pred"]).to(dev)
    s3_label = c["label"] % 13 + 1
    gt_id, col_h = np.unique(c["gt_ids"], return_inverse=True)
    G = len(gt_id)
    col = torch.from_numpy(col_h.astype(np.int32)).to(dev)
    a32, b32 = sem_gt_d.to(torch.int32), sem_pred_d.to(torch.int32)

    ins, s3, sem = wsis_eval.InstanceEvaluator.scannet(), wsis_eval.S3DISInstanceEvaluator(), wsis_eval.SemanticEvaluator.s3dis()
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "scene": {"points": int(N), "predictions": int(P), "distinct_gt_ids": int(G), "instances": int(c["n_inst"])},
           "ms_per_call": {}, "ms_kernel": {}}
    calls = {
        "InstanceEvaluator.process_int64_masks": lambda: ins.process("s", c["conf"], c["label"], m64, gt_d),
        "InstanceEvaluator.process_uint8_masks": lambda: ins.process("s", c["conf"], c["label"], m8, gt_d),
        "S3DISInstanceEvaluator.process_int64_masks": lambda: (s3.reset(), s3.process(c["conf"], s3_label, m64, sem_gt_d, inst_d)),
        "SemanticEvaluator.process": lambda: sem.process(sem_pred_d, sem_gt_d),
    }
    for name, fn in calls.items():
        res["ms_per_call"][name] = event_ms(fn, args.warmup, args.iters)
    out = (torch.empty((P, G), dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int64, device=dev))
    out2 = torch.empty((13, 13), dtype=torch.int64, device=dev)
    for name, m in (("wsis_mask_overlap_int64", m64), ("wsis_mask_overlap_uint8", m8)):
        ms = event_ms(lambda: wsis_eval.mask_overlap(m, col, G, out=out), args.warmup, args.iters)
        nbytes = P * N * m.element_size() + 4 * N
        res["ms_kernel"][name] = {"ms": ms, "bytes_read": int(nbytes), "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                                  "fraction_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    res["ms_kernel"]["wsis_label_pairs_13x13"] = {"ms": event_ms(lambda: wsis_eval.label_pairs(a32, b32, 13, 13, out=out2),
                                                                 args.warmup, args.iters)}
    res["ms_kernel"]["torch_unique_of_gt_ids"] = {"ms": event_ms(
        lambda: torch.unique(gt_d, sorted=True, return_inverse=True, return_counts=True), args.warmup, args.iters)}
    table_ok = np.array_equal(out[0].cpu().numpy(), eval_ref.overlap_table(c["masks"], col_h, G)[0])
    res["table_equals_numpy"] = bool(table_ok)
    # the loop-per-pair form on this host
    ids = wsis_eval.SCANNET_INSTANCE_CLASS_IDS
    ref = eval_ref.S3DISRef()
    res["ms_numpy_loop_per_pair_host"] = {
        "instance_assign_scene": host_ms(lambda: eval_ref.assign_scene(ids, c["conf"], c["label"], c["masks"], c["gt_ids"])),
        "s3dis_process": host_ms(lambda: ref.process(s3_label, c["masks"], c["sem_gt"], c["inst"])),
        "semantic_add_at": host_ms(lambda: eval_ref.pair_table(c["sem_gt"], c["sem_pred"], 14, 14), 3),
    }
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
