"""CPU: the op lists, arena layouts and bookkeeping that model/unet_native.py records for the sparse UNet are byte for byte
what tests/golden/unet_program_golden.npz holds (tests/golden/make_unet_program_golden.py: fp32 training and evaluation
programs under every compile-time switch, the synced-BatchNorm recording, the 16-bit inference programs, the 16-bit
training programs of kind ``"lp_train"``, one of them with a BatchNorm layer in evaluation mode).  The recorder
needs no device; what it hands the executor is a byte array, so a change of the recorder that is meant to leave the
passes alone is checked here, without a GPU."""
import os

import numpy as np
import pytest

import unet_native as un
from tests.golden import make_unet_program_golden as gen

CASES = [pytest.param(name, marks=pytest.mark.experimental) if spec[3] else name for name, spec in gen.CASES.items()]


@pytest.fixture(scope="module")
def golden():
    return gen.load()


@pytest.fixture(scope="module")
def model():
    return gen.build_model()


def test_fixture_holds_every_case_and_nothing_else(golden):
    assert len(gen.CASES) == 20
    assert set(golden) == set(gen.CASES)
    assert os.path.getsize(gen.FIXTURE) < 100 * 1024


def _first_difference(got, want):
    """the first differing op and field of two op byte arrays, for the failure message"""
    if got.size != want.size:
        return "%d ops recorded, %d in the fixture" % (got.size // un.OP_DTYPE.itemsize, want.size // un.OP_DTYPE.itemsize)
    a, b = np.frombuffer(got.tobytes(), dtype=un.OP_DTYPE), np.frombuffer(want.tobytes(), dtype=un.OP_DTYPE)
    for i in range(len(a)):
        for f in un.OP_DTYPE.names:
            if not np.array_equal(a[i][f], b[i][f]):
                return "op %d (kind %d) field %s: recorded %s, fixture %s" % (i, b[i]["kind"], f, a[i][f], b[i][f])
    return "equal"


@pytest.mark.parametrize("name", CASES)
def test_recorded_program_is_byte_identical_to_the_fixture(name, model, golden):
    got = gen.record(model, name)
    want = golden[name]
    assert set(got) == set(want)
    for side in ("fwd", "bwd"):
        assert got[side].dtype == want[side].dtype == np.uint8
        assert np.array_equal(got[side], want[side]), "%s ops: %s" % (side, _first_difference(got[side], want[side]))
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def test_sanity_of_the_default_training_program(golden):
    """the figures the fixture was checked against when it was made: 98 ops each way, 88 + 88 of them with F_STATS"""
    for side in ("fwd", "bwd"):
        ops = np.frombuffer(golden["train_dx1"][side].tobytes(), dtype=un.OP_DTYPE)
        assert len(ops) == 98 and int(np.sum((ops["flags"] & un.F_STATS) != 0)) == 88
        off = np.frombuffer(golden["train_no_fused_stats"][side].tobytes(), dtype=un.OP_DTYPE)
        assert len(off) == 98 and not np.any(off["flags"] & un.F_STATS)
