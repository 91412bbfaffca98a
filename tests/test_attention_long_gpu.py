"""Fused attention at 192 < T <= 1024 (column-chunked kernels) on the MI355X; shared cases in tests/attention_long_cases.py."""
import pytest
import torch

import attention_long_cases as alc
import kernel_cases as kc
import redzone
from transfuser_amd import ops

pytestmark = pytest.mark.gpu
CAPTURES_A_GRAPH = ("test_long_attention_tiny_model_and_engine",)      # outside the guard: the Engine's captured step


@pytest.fixture(autouse=True)
def _gpu(request):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from transfuser_amd import _lib
    assert not _lib.is_test_backend()
    _lib.load()  # raises if libtransfuser_hip.so is missing: no fallback
    yield from redzone.fixture_guard(request, ops, alc, kc, outside=CAPTURES_A_GRAPH)      # guard bands + NaN poison around every tensor ops / the cases allocate
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", alc.PARITY_CASES + alc.PARITY_CASES_GPU, ids=str)
def test_long_attention_parity(case):
    alc.check_parity("cuda", *case)


@pytest.mark.parametrize("case", alc.SKEW_CASES + alc.SKEW_CASES_GPU, ids=str)
def test_long_attention_maximum_in_a_later_chunk(case):
    alc.check_parity("cuda", *case[:5], skew=case[5])


def test_long_attention_reproducible_without_atomics():
    alc.check_reproducible("cuda")


def test_long_attention_predicate():
    alc.check_predicate("cuda")


def test_long_attention_gpt_stage():
    alc.check_gpt_stage("cuda")


def test_long_attention_tiny_model_and_engine():
    alc.check_tiny_model("cuda")
