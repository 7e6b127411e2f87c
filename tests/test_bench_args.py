"""CPU: bench.py's command line -- a plain run is the headline alone, everything else waits for --full."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("wsis_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and a.steps == 7 and a.warmup == 2 and a.setup_steps == 300


def test_full_keeps_its_trimming_options(monkeypatch):
    a = _args(monkeypatch, "--full", "--no-stages", "--no-cpu-baseline", "--profile-steps", "4")
    assert a.full and a.no_stages and a.no_cpu_baseline and a.profile_steps == 4
