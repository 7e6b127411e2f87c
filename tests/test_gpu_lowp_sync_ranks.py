"""GPU, two real ranks: the synced 16-bit native training pass of the UNet (WSIS_NATIVE_LP_TRAIN=1 + WSIS_NATIVE_LP_SYNC=1)
through ``Network.forward``.  Two child processes (tests/_lp_sync_worker.py), both on cuda:0, process group on gloo -- the
environment of tests/test_gpu_two_ranks.py -- are launched ONCE for the module and run every scenario on smoke-size scenes;
the parent compares what they saved.

(d) the same scene on both ranks: the pass is taken (``last_pass``, ``prog.bn_sync``) and loss, UNet output and every UNet
    parameter gradient equal, bit for bit, the unsynced 16-bit pass of the same rank in the same process, and the other
    rank's: 2 m n / (2 n) = m in fp64 for fp32 m and n < 2^24, the centred term is 0, 2 s * (M / N = 0.5) = s.  (The UNet's
    BatchNorm layers are the converted ones: the heads and GNN layers behind it take another kernel path once converted,
    and the comparison is about the UNet's pass.)
(e) a different scene per rank, the whole model converted: error of the UNet output (relative Frobenius) and of the UNet
    parameter gradients (median 1 - cos) against the synced fp32 native pass, with the synced 16-bit module walk -- what
    such a user gets without the second switch -- as the yardstick: native / walk <= WALK_FACTOR.
(f) two optimizer steps with GradSync, whole model converted (bf16; fp16 with LossScaler): every weight and running
    statistic bit-equal across the ranks, finite losses, the flat path of GradSync.
(g) the same two steps with BatchNorm not converted: the 16-bit pass with GradSync alone.
"""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_lp_sync_worker.py")
NAMES = ("bf16", "fp16")
# the bound and ladder (1.25 / 1.5 / 2) of tests/test_gpu_lowp_train.py for the unsynced pass
WALK_FACTOR = 1.25


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out_dir = tmp_path_factory.mktemp("lp_sync")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ)
        env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), WSIS_DIST_BACKEND="gloo", WSIS_DIST_TIMEOUT="240",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, WORKER, str(out_dir)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=420)
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()            # exactly the children started above
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank} failed:\n{out[-4000:]}"
    res = [torch.load(os.path.join(out_dir, f"lp_sync{r}.pt"), weights_only=False) for r in range(2)]
    assert res[0]["voxels_same"] == res[1]["voxels_same"] and res[0]["voxels_own"] != res[1]["voxels_own"]
    return res


@pytest.mark.parametrize("name", NAMES)
def test_same_scene_on_both_ranks_equals_the_unsynced_pass(ranks, name):
    for r in ranks:
        u, s = r["d_unsynced_" + name], r["d_synced_" + name]
        assert u["last_pass"] == s["last_pass"] == "native_lp_train"
        assert not u["bn_sync"] and s["bn_sync"], "the synced run must go through the statistics exchange"
        assert bool(torch.isfinite(s["loss"])) and float(s["out"].float().abs().max()) > 0
        assert torch.equal(s["out"].view(torch.int16), u["out"].view(torch.int16)), \
            f"rank {r['rank']}: {int((s['out'] != u['out']).sum())} of {u['out'].numel()} output elements differ"
        assert torch.equal(s["loss"], u["loss"]), (float(s["loss"]), float(u["loss"]))
        assert len(s["grads"]) > 100 and set(s["grads"]) == set(u["grads"])
        assert [n for n in s["grads"] if s["grads"][n] != u["grads"][n]] == [], f"rank {r['rank']}: UNet parameter gradients"
    a, b = ranks[0]["d_synced_" + name], ranks[1]["d_synced_" + name]
    assert torch.equal(a["out"].view(torch.int16), b["out"].view(torch.int16)) and torch.equal(a["loss"], b["loss"])
    assert a["grads"] == b["grads"], "the two ranks' results are equal"


@pytest.mark.parametrize("name", NAMES)
def test_different_scenes_against_the_synced_walk(ranks, name):
    for r in ranks:
        e = r["e_" + name]
        print(f"rank {r['rank']} {name}: UNet output rel. Frobenius error native {e['out_native']:.3e}, walk {e['out_walk']:.3e}, "
              f"ratio {e['out_native'] / e['out_walk']:.3f}; median 1 - cos of the parameter gradients native "
              f"{e['grad_native']:.3e}, walk {e['grad_walk']:.3e}, ratio {e['grad_native'] / e['grad_walk']:.3f}; worst native "
              f"{e['grad_worst_native']:.3e}, walk {e['grad_worst_walk']:.3e}; forward + backward of the UNet on the host clock "
              f"(two processes share the GPU: orientation only) native {e['ms_native']:.1f} ms, walk {e['ms_walk']:.1f} ms, "
              f"fp32 native {e['ms_fp32']:.1f} ms")
    for r in ranks:
        e = r["e_" + name]
        assert e["out_walk"] > 0 and e["grad_walk"] > 0, "the walk is as exact as fp32: the yardstick shows nothing"
        assert e["out_native"] <= WALK_FACTOR * e["out_walk"], (e["out_native"], e["out_walk"])
        assert e["grad_native"] <= WALK_FACTOR * e["grad_walk"], (e["grad_native"], e["grad_walk"])


def _two_steps(ranks, key, converted):
    a, b = ranks[0][key], ranks[1][key]
    for r in (a, b):
        assert r["passes"] == ["native_lp_train"] * 2 and r["bn_sync"] == converted
        assert all(l == l and abs(l) != float("inf") for l in r["losses"]), r["losses"]
        assert r["flat_params"] >= r["n_unet_params"] > 100, "GradSync took the flat path"
    assert a["losses"][0] != b["losses"][0], "different scenes, different losses"
    assert len(a["weights"]) > a["n_unet_params"] and set(a["weights"]) == set(b["weights"])
    assert [n for n in a["weights"] if a["weights"][n] != b["weights"][n]] == [], "weights differ across the ranks"
    return a, b


@pytest.mark.parametrize("name", NAMES)
def test_two_steps_with_gradsync_keep_the_ranks_identical(ranks, name):
    a, b = _two_steps(ranks, "f_" + name, True)
    assert len(a["stats"]) > 80 and set(a["stats"]) == set(b["stats"])
    assert [n for n in a["stats"] if a["stats"][n] != b["stats"][n]] == [], "running statistics differ across the ranks"


@pytest.mark.parametrize("name", NAMES)
def test_two_steps_with_gradsync_alone(ranks, name):
    a, b = _two_steps(ranks, "g_" + name, False)
    unet = [n for n in a["stats"] if n.startswith(("unet.", "output_layer."))]
    assert any(a["stats"][n] != b["stats"][n] for n in unet), "per-rank statistics: the ranks saw different scenes"
