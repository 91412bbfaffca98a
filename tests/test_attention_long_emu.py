"""Fused attention at 192 < T <= 1024 (column-chunked kernels) on the host emulator; the same checks run on the MI355X in
tests/test_attention_long_gpu.py (shared cases in tests/attention_long_cases.py)."""
import pytest

import attention_long_cases as alc
import kernel_cases as kc
import redzone
from transfuser_amd import ops


@pytest.fixture(autouse=True)
def _backend(emu_backend, request):
    yield from redzone.fixture_guard(request, ops, alc, kc)      # guard bands + NaN poison around every tensor ops / the cases allocate


@pytest.mark.parametrize("case", alc.PARITY_CASES, ids=str)
def test_long_attention_parity(case):
    alc.check_parity("cpu", *case)


@pytest.mark.parametrize("case", alc.SKEW_CASES, ids=str)
def test_long_attention_maximum_in_a_later_chunk(case):
    alc.check_parity("cpu", *case[:5], skew=case[5])


def test_long_attention_reproducible_without_atomics():
    alc.check_reproducible("cpu")


def test_long_attention_predicate():
    alc.check_predicate("cpu")


def test_long_attention_gpt_stage():
    alc.check_gpt_stage("cpu")
