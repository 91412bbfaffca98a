"""Weight EMA on the MI355X: the tick / apply / table / swap kernels against float64 and the formula, refusals, the Engine's average against a
shadow advanced with the same launches (eager and captured), the captured step against the eager one, ema_weights() in fp32 and bf16 storage,
checkpoints, resume and the command line.  Cases: tests/ema_cases.py."""
import pytest
import torch

import accum_clip_cases as acc
import ema_cases as ec
import kernel_cases as kc
import redzone
from transfuser_amd import ema as ema_module
from transfuser_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPTURES_A_GRAPH = ("test_captured_equals_eager", "test_captured_trajectory_equals_shadow", "test_main_saves_and_resumes_the_average")      # outside the guard


@pytest.fixture(autouse=True)
def _gpu(request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, ec, ema_module, acc, kc, outside=CAPTURES_A_GRAPH)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
        ops.force_plan(0)


@pytest.mark.parametrize("n", ec.APPLY_SIZES)
def test_apply_against_float64(n):
    ec.check_apply(DEV, n)


def test_apply_multi_against_float64():
    ec.check_apply_multi(DEV)


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.999, 0.5])
def test_tick_coefficients(decay, warmup):
    ec.check_tick(DEV, decay, warmup)


def test_tick_every_and_repeated_step():
    ec.check_tick_every(DEV)


def test_fp16_skipped_step_skips_the_average():
    ec.check_fp16_skip(DEV)


def test_swap():
    ec.check_swap(DEV)


def test_kernel_argument_refusals():
    ec.check_kernel_refusals(DEV)


def test_no_float_atomics_in_deterministic_mode():
    ec.check_deterministic_counter(DEV)


def test_ema_never_feeds_back():
    ec.check_never_feeds_back(DEV)


@pytest.mark.parametrize("case", list(ec.TRAJECTORIES))
def test_trajectory_equals_shadow(case):
    ec.check_trajectory(DEV, case)


def test_captured_trajectory_equals_shadow():
    eng = ec.check_trajectory(DEV, "plain", use_graph=True)
    assert eng._graphs is not None


def test_captured_equals_eager():
    ec.check_captured_equals_eager(DEV)


def test_ema_weights_context():
    ec.check_ema_weights(DEV)


def test_bf16_storage_swap_refreshes_the_weight_copies():
    ec.check_bf16_swap_refreshes_copies(DEV)


def test_engine_refusals():
    ec.check_refusals(DEV)


def test_trainer_save_validate_resume(tmp_path):
    ec.check_trainer_save_resume(DEV, tmp_path)


def test_main_saves_and_resumes_the_average(tmp_path):
    ec.check_main_resume(tmp_path)
