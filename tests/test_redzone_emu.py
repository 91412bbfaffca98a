"""The guard-band harness (tests/redzone.py) on the host emulator: the harness checked on itself, pins that the op-level checks really allocate
through it, one eager model step under it, and guarded fp64 / exact checks of ops entry points that had none.  The same cases run on the
MI355X in tests/test_redzone_gpu.py (shared cases in tests/redzone_cases.py)."""
import pytest

import redzone_cases as rc


@pytest.fixture(autouse=True)
def _backend(emu_backend):
    yield


def test_band_writes_are_reported_with_site_side_and_offset():
    rc.check_band_reports("cpu")


def test_empty_reads_as_poison_and_fills_keep_their_value():
    rc.check_poison_and_fill("cpu")


def test_band_size_rule():
    rc.check_band_size()


def test_strides_are_real_torchs_and_the_interior_is_512_byte_aligned():
    rc.check_strides_and_alignment("cpu")


def test_passthroughs_are_counted_with_their_reason():
    rc.check_passthroughs("cpu")


def test_real_torch_is_back_after_the_guard_also_after_an_exception():
    rc.check_restored("cpu")


def test_guard_covers_gemm_outputs():
    rc.check_pin_gemm("cpu")


def test_guard_covers_colstat_buffers():
    rc.check_pin_colstat("cpu")


def test_guard_covers_the_splitk_scratch():
    rc.check_pin_splitk_scratch("cpu")


def test_tiny_model_step_under_the_guard():
    rc.check_model_step("cpu")


def test_sigmoid():
    rc.check_sigmoid("cpu")


def test_weighted_sum_and_its_backward():
    rc.check_weighted_sum("cpu")


def test_cast_f32():
    rc.check_cast_f32("cpu")


def test_adamw_dynscale_finite_and_overflowed_steps():
    rc.check_adamw_dynscale("cpu")


@pytest.mark.parametrize("case", rc.BN_ROWS_CASES, ids=str)
def test_bn_rows_dev_bwd(case):
    rc.check_bn_rows_dev_bwd("cpu", *case)


@pytest.mark.parametrize("case", rc.PILLAR_CLOUDS, ids=str)
def test_pillar_scatter_max_canvas_and_backward_equal_a_numpy_scatter(case):
    rc.check_pillar_scatter_canvas("cpu", *case)
