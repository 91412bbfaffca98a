"""The 16-byte (transposed-accumulator) epilogue of the register-staged GEMM engine on a real MI355X: switch on == switch off bit for bit,
ineligible calls provably keep the 4-byte epilogue, BatchNorm statistics with the switch on.  Same cases as tests/test_engine_epilogue_emu.py."""
import pytest
import torch

import epilogue_cases as ec
import kernel_cases as kc
import redzone
from transfuser_amd import ops


pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu(request):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from transfuser_amd import _lib
    assert not _lib.is_test_backend()
    _lib.load()  # raises if libtransfuser_hip.so is missing: no fallback
    yield from redzone.fixture_guard(request, ops, ec, kc)      # guard bands + NaN poison around every tensor ops / the cases allocate
    torch.cuda.synchronize()


@pytest.mark.parametrize("plan", ec.PLANS, ids=str)
def test_switch_on_equals_switch_off_bitwise(plan):
    ec.check_bitwise("cuda", *plan)


@pytest.mark.parametrize("case", ec.PAIR_CASES, ids=str)
def test_pair_bracket_bitwise(case):
    ec.check_pair_bitwise("cuda", *case)


def test_ineligible_calls_keep_the_4_byte_epilogue():
    ec.check_fallbacks("cuda")


@pytest.mark.parametrize("plan", ec.TRN_PLANS, ids=str)
def test_statistics_with_the_switch_on(plan):
    ec.check_stats("cuda", *plan)


def test_grouped_conv_bias_offset_by_one_float():
    ec.check_grouped_bias_alignment("cuda")
