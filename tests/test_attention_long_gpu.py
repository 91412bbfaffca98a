"""Fused attention at 192 < T <= 1024 (column-chunked kernels) on the MI355X; shared cases in tests/attention_long_cases.py."""
import pytest

import attention_long_cases as alc

pytestmark = pytest.mark.gpu


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
