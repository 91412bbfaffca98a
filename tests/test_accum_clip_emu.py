"""Gradient accumulation and fused global-norm clipping on the host emulator (the HIP sources compiled for the host): the kernels against
float64, the accumulation window against single runs and against the CPU oracle's two-rank arithmetic.  Cases: tests/accum_clip_cases.py;
the same kernel and window checks run on the MI355X in tests/test_accum_clip_gpu.py."""
import pytest

import accum_clip_cases as acc
import kernel_cases as kc
import redzone
from transfuser_amd import ops


@pytest.fixture(autouse=True)
def _backend(emu_backend, request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, acc, kc)      # guard bands + NaN poison around every tensor ops / the cases allocate
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("n", acc.SUMSQ_SIZES)
def test_grad_sumsq(n):
    acc.check_sumsq("cpu", n)


@pytest.mark.parametrize("case", acc.CLIP_CASES)
def test_adamw_clip(case):
    acc.check_adamw_clip("cpu", case)


@pytest.mark.parametrize("arch", ["regnety_tiny", "convnext_mini"])
def test_window_is_sum_of_micro_batch_gradients(arch):
    acc.check_window_is_sum("cpu", arch)


def test_window_matches_oracle_two_rank_mean_and_clip_norm():
    acc.check_ddp_equivalence_vs_oracle("cpu")


def test_fp16_dynamic_loss_scale_window():
    acc.check_fp16_dynamic_window("cpu")


def test_refusals():
    acc.check_refusals("cpu")
