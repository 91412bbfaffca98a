"""Gradient accumulation and clipping under the deterministic mode on the host emulator: clipped windows are bitwise reproducible, and the
default arguments leave the train step's bits alone.  A file of its own so that a parallel run can place these two long tests beside
tests/test_accum_clip_emu.py instead of behind it.  Cases: tests/accum_clip_cases.py."""
import pytest

import accum_clip_cases as acc
from transfuser_amd import ops


@pytest.fixture(autouse=True)
def _backend(emu_backend):
    prev = ops.is_deterministic()
    try:
        yield
    finally:
        ops.set_deterministic(prev)


def test_deterministic_eager_windows_bitwise():
    acc.check_bitwise_runs("cpu", False)


def test_defaults_unchanged():
    acc.check_defaults_unchanged("cpu")
