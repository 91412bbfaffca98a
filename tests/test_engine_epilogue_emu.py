"""The 16-byte (transposed-accumulator) epilogue of the register-staged GEMM engine on the host-emulated build: the emulator reproduces the
MFMA's lane layout, so the same cases as tests/test_engine_epilogue_gpu.py run on the CPU (shared case lists in tests/epilogue_cases.py)."""
import pytest

import epilogue_cases as ec
import kernel_cases as kc
import redzone
from transfuser_amd import ops


@pytest.fixture(autouse=True)
def _backend(emu_backend, request):
    yield from redzone.fixture_guard(request, ops, ec, kc)      # guard bands + NaN poison around every tensor ops / the cases allocate


@pytest.mark.parametrize("plan", ec.PLANS, ids=str)
def test_switch_on_equals_switch_off_bitwise(plan):
    ec.check_bitwise("cpu", *plan)


@pytest.mark.parametrize("case", ec.PAIR_CASES, ids=str)
def test_pair_bracket_bitwise(case):
    ec.check_pair_bitwise("cpu", *case)


def test_ineligible_calls_keep_the_4_byte_epilogue():
    ec.check_fallbacks("cpu")


@pytest.mark.parametrize("plan", ec.TRN_PLANS, ids=str)
def test_statistics_with_the_switch_on(plan):
    ec.check_stats("cpu", *plan)


def test_grouped_conv_bias_offset_by_one_float():
    ec.check_grouped_bias_alignment("cpu")
