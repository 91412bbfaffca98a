"""Weight EMA on the host emulator (the HIP sources compiled for the host): the tick / apply / table / swap kernels against float64 and the
formula, refusals, the Engine's average against a shadow advanced with the same launches, ema_weights(), state, checkpoints and resume.
Cases: tests/ema_cases.py; the same checks run on the MI355X in tests/test_ema_gpu.py."""
import pytest

import accum_clip_cases as acc
import ema_cases as ec
import kernel_cases as kc
import redzone
from transfuser_amd import ema as ema_module
from transfuser_amd import ops


@pytest.fixture(autouse=True)
def _backend(emu_backend, request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, ec, ema_module, acc, kc)      # guard bands + NaN poison, the WeightEMA's own buffers included
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("n", ec.APPLY_SIZES)
def test_apply_against_float64(n):
    ec.check_apply("cpu", n)


def test_apply_multi_against_float64():
    ec.check_apply_multi("cpu")


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.999, 0.5])
def test_tick_coefficients(decay, warmup):
    ec.check_tick("cpu", decay, warmup)


def test_tick_every_and_repeated_step():
    ec.check_tick_every("cpu")


def test_fp16_skipped_step_skips_the_average():
    ec.check_fp16_skip("cpu")


def test_swap():
    ec.check_swap("cpu")


def test_kernel_argument_refusals():
    ec.check_kernel_refusals("cpu")


def test_no_float_atomics_in_deterministic_mode():
    ec.check_deterministic_counter("cpu")


def test_ema_never_feeds_back():
    ec.check_never_feeds_back("cpu")


@pytest.mark.parametrize("case", [c for c in ec.TRAJECTORIES if c != "warmup_every2"])      # that one runs on the GPU only: an emulated step takes ~25 s
def test_trajectory_equals_shadow(case):
    ec.check_trajectory("cpu", case)


def test_ema_weights_context():
    ec.check_ema_weights("cpu")


def test_engine_refusals():
    ec.check_refusals("cpu")


def test_trainer_save_validate_resume(tmp_path):
    ec.check_trainer_save_resume("cpu", tmp_path)


def test_cli_flags():
    ec.check_cli_flags()
