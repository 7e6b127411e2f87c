"""executor_layout_golden.json: what ``wsis_run_ops_workspace_bytes`` answers for the op lists of
``unet_program_golden.npz`` (complete forward and backward programs with fake addresses: the size query never
dereferences them and needs no device), under every environment that changes the layout of a pass's workspace.

The file pins the sizes to the revision it was generated at, so that a change of ``csrc/executor.hip`` that is meant to
leave the layout alone is checked on the CPU (tests/test_executor_layout_host.py).  It holds one table per build flavour:
``default`` has all 15 programs, ``experimental`` the three programs whose fused BatchNorm forms only that build runs
(the other twelve size the same on both).  Each run rewrites the table of the flavour it ran on and keeps the other:

    python __graft_entry__.py && python tests/golden/make_executor_layout_golden.py
    WSIS_EXPERIMENTAL=1 python __graft_entry__.py && python tests/golden/make_executor_layout_golden.py

(rebuild the default flavour afterwards)
"""
import contextlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "executor_layout_golden.json")

# name -> the switches of the pass that change its workspace layout
ENVS = {"default": {}, "batch_reduce": {"WSIS_DW_BATCH_REDUCE": "1"}, "no_fwd2": {"WSIS_FWD2": "0"}}
SWITCHES = ("WSIS_DW_BATCH_REDUCE", "WSIS_FWD2", "WSIS_DEEP")
SIDES = ("fwd", "bwd")


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def programs():
    """{case: {side: op array}} of unet_program_golden.npz"""
    import unet_native as un
    from tests.golden import make_unet_program_golden as prog
    return {name: {side: np.frombuffer(arrays[side].tobytes(), dtype=un.OP_DTYPE) for side in SIDES}
            for name, arrays in prog.load().items()}


def needs_experimental(name):
    from tests.golden import make_unet_program_golden as prog
    return bool(prog.CASES[name][3])


def sizes(lib, ops):
    """{environment name: bytes} of one op list"""
    out = {}
    for env_name, env in ENVS.items():
        with environment(env):
            out[env_name] = int(lib.wsis_run_ops_workspace_bytes(ops.ctypes.data, len(ops)))
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    sys.path.insert(0, ROOT)
    importlib.import_module("3d-wsis_amd")
    import wsis_native
    lib = wsis_native.hip()
    flavour = "experimental" if wsis_native.experimental() else "default"
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True).stdout.strip()
    commit = git("rev-parse", "HEAD") or "unknown"
    dirty = bool(git("status", "--porcelain", "--", "3d-wsis_amd/csrc", "include"))
    print("commit %s%s, %s flavour" % (commit, " + uncommitted changes of the C sources" if dirty else "", flavour))
    table = {}
    for name, sides in programs().items():
        if flavour == "experimental" and not needs_experimental(name):
            continue
        table[name] = {side: sizes(lib, sides[side]) for side in SIDES}
        print("%-32s %s" % (name, json.dumps(table[name])))
    doc = load() if os.path.exists(FIXTURE) else {}
    doc[flavour] = table
    doc.setdefault("commit", {})[flavour] = commit + ("+" if dirty else "")
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("executor_layout_golden.json: %d programs of the %s flavour" % (len(table), flavour))


if __name__ == "__main__":
    main()
