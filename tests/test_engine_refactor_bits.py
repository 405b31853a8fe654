"""The engine's host orchestration computes, on the CPU emulator build, exactly the bits recorded in
tests/golden/engine_refactor_bits.npz (tests/golden/make_engine_refactor_golden.py names the commit they came from): a train-mode
forward + loss + backward, a 2-step first-order and a 2-step second-order meta_grad, and a pass with a frame-level feature — tiny
dims, two ragged tasks, dropout on with a fixed seed.  Losses, mel_post, every per-task parameter gradient and the outer gradient,
no tolerance: a refactor of csrc/engine.h, engine_so.inc or engine_imaml.inc that changes a launch argument shows here."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as ge

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_engine_refactor_golden as MG  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return MG.record(ge.build_emulator())


@pytest.fixture(scope="module")
def golden():
    return MG.unpack(np.load(MG.FIXTURE))


def test_same_arrays_as_the_fixture(recorded, golden):
    assert sorted(recorded) == sorted(golden)


@pytest.mark.parametrize("case", ["train", "fo", "so", "frame"])
def test_same_bits_as_the_recorded_commit(recorded, golden, case):
    keys = [k for k in golden if k.startswith(case + "/")]
    assert any("/grad/" in k for k in keys) and case + "/losses" in keys
    assert (case in ("fo", "so")) == any("/outer/" in k for k in keys)
    for k in keys:
        np.testing.assert_array_equal(recorded[k], golden[k], err_msg=k)


def test_recording_is_deterministic(recorded):
    """What exact equality rests on: the same build records the same bits twice."""
    again = MG.record(ge.build_emulator())
    for k in recorded:
        np.testing.assert_array_equal(again[k], recorded[k], err_msg=k)
