"""Gradient accumulation and fused global-norm clipping on the MI355X: the kernels against float64, the accumulation window against single
runs, the captured window (piece graphs + one optimizer graph) against the eager one, bitwise reproducibility under the deterministic mode
and the unchanged defaults.  Cases: tests/accum_clip_cases.py."""
import pytest
import torch

import accum_clip_cases as acc
import kernel_cases as kc
import redzone
from transfuser_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPTURES_A_GRAPH = ("test_graph_windows_match_eager", "test_deterministic_windows_bitwise[graph]")      # outside the guard


@pytest.fixture(autouse=True)
def _gpu(request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, acc, kc, outside=CAPTURES_A_GRAPH)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
        ops.force_plan(0)


@pytest.mark.parametrize("n", acc.SUMSQ_SIZES)
def test_grad_sumsq(n):
    acc.check_sumsq(DEV, n)


@pytest.mark.parametrize("case", acc.CLIP_CASES)
def test_adamw_clip(case):
    acc.check_adamw_clip(DEV, case)


@pytest.mark.parametrize("arch", ["regnety_tiny", "convnext_mini"])
def test_window_is_sum_of_micro_batch_gradients(arch):
    acc.check_window_is_sum(DEV, arch)


def test_graph_windows_match_eager():
    acc.check_graph_matches_eager(DEV)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_deterministic_windows_bitwise(use_graph):
    acc.check_bitwise_runs(DEV, use_graph)


def test_defaults_unchanged():
    acc.check_defaults_unchanged(DEV)


def test_refusals():
    acc.check_refusals(DEV)
