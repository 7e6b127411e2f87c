"""dw_plan_golden.json: what the library answers, without a device, about the fp32 weight gradient of every shape of
``tests/dw_plan_ref.py`` (CASES): ``wsis_spconv_dw_workspace_bytes``, ``wsis_spconv_dw_bn_supported``,
``wsis_spconv_dw_bn_workspace_bytes`` and, where the shape is on the wave-autonomous kernels, the wave count of the launch
under ``wsis_hint_batch_rows`` 0 / 249,999 / 250,000 / 625,000.

The file pins these figures to the revision it was generated at -- the one before the launch plan got one definition
(csrc/spconv_dw2.hip: dw_plan) -- so that a change of the host code that is meant to leave sizes and grids alone is checked
on the CPU (tests/test_dw_plan_host.py).  That revision has no plan query; it tells the wave count through
``wsis_debug_dw2_diag``, which writes ``*n_waves = grid.x * grid.y * 4`` before it looks at the stamp buffer: a call with
``dbg_bytes = 0`` returns an argument error after the write and launches nothing (the table pointers are dummies, never
dereferenced).  A shape it refuses before the write is not on those kernels: ``waves`` is null.

    python __graft_entry__.py && python tests/golden/make_dw_plan_golden.py

refuses to run on modified C sources.
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "dw_plan_golden.json")
DUMMY = 1 << 12      # a 16-byte aligned non-null address


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def sizes(lib, c):
    """the three size queries of a case's shape"""
    return {"ws": int(lib.wsis_spconv_dw_workspace_bytes(c.M_out, c.K, c.Cin, c.Cout)),
            "bn_supported": int(lib.wsis_spconv_dw_bn_supported(c.K, c.Cin, c.Cout)),
            "bn_ws": int(lib.wsis_spconv_dw_bn_workspace_bytes(c.M_in, c.K, c.Cin, c.Cout))}


def _waves(lib, c, ref):
    fn = lib.wsis_debug_dw2_diag
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_int32] * 3 + [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    nbr = DUMMY if c.table != ref.NO_TABLE else None
    order = DUMMY if c.table == ref.TABLE else None
    out = {}
    for rows in ref.HINTS:
        assert lib.wsis_hint_batch_rows(rows) == 0
        nw = ctypes.c_int64(-1)
        rc = fn(DUMMY, nbr, order, DUMMY, c.M_in, c.M_out, c.K, c.Cin, c.Cout, DUMMY, DUMMY, 0, ctypes.byref(nw), None)
        assert rc != 0, "a call without a stamp buffer launches nothing"
        out[str(rows)] = int(nw.value) if nw.value >= 0 else None
    assert lib.wsis_hint_batch_rows(0) == 0
    if any(v is None for v in out.values()):
        assert all(v is None for v in out.values())
        return None
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dw_plan_ref as ref
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True).stdout.strip()
    commit = git("rev-parse", "HEAD") or "unknown"
    if git("status", "--porcelain", "--", "3d-wsis_amd/csrc", "include"):
        sys.exit("the C sources differ from %s: the figures would not be that revision's" % commit)
    for k in ("WSIS_DW3", "WSIS_IN_CONV"):
        os.environ.pop(k, None)
    lib = ref.lib()
    table = {}
    for c in ref.CASES:
        table[c.name] = dict(sizes(lib, c), waves=_waves(lib, c, ref))
        print("%-28s %s" % (c.name, json.dumps(table[c.name])))
    with open(FIXTURE, "w") as f:
        json.dump({"commit": commit, "cases": table}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("dw_plan_golden.json: %d shapes at %s" % (len(table), commit))


if __name__ == "__main__":
    main()
