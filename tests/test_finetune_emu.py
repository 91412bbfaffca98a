"""Fine-tuning on the host emulator (the HIP sources compiled for the host): AdamW parameter groups and the group-aware norm against float64,
the frozen-statistics BatchNorm backward against float64 autograd, frozen parameters / groups through the Engine against the CPU oracle with
torch.optim.AdamW param groups, resume, refusals and the Trainer's epoch loop.  Cases: tests/finetune_cases.py; the same kernel and Engine
checks run on the MI355X in tests/test_finetune_gpu.py."""
import pytest

import accum_clip_cases as acc
import finetune_cases as ft
import kernel_cases as kc
import redzone
from transfuser_amd import ops


@pytest.fixture(autouse=True)
def _backend(emu_backend, request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, ft, acc, kc)      # guard bands + NaN poison around every tensor ops / the cases allocate
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("arena,table", ft.GROUP_ADAMW_CASES)
def test_group_adamw(arena, table):
    ft.check_group_adamw("cpu", arena, table)


def test_one_default_group_is_plain_adamw_bitwise():
    ft.check_one_group_is_plain_adamw("cpu")


def test_group_sumsq_and_clip():
    ft.check_group_sumsq_clip("cpu")


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "frozen_affine"])
@pytest.mark.parametrize("relu,with_res", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("shape", ft.BN_FROZEN_SHAPES)
def test_bn_bwd_frozen(shape, relu, with_res, affine):
    ft.check_bn_frozen("cpu", *shape, relu, with_res, affine)


def test_eval_mode_batchnorm_module_backward():
    ft.check_eval_bn_module_backward("cpu")


def test_kernel_argument_refusals():
    ft.check_kernel_refusals("cpu")


@pytest.mark.parametrize("by_hand", [False, True], ids=["freeze_arg", "requires_grad_false"])
def test_frozen_parameters_stay_put(by_hand):
    ft.check_frozen_stay("cpu", by_hand)


@pytest.mark.parametrize("case", ["lr_mult", "no_decay_1d"])
@pytest.mark.parametrize("arch", ["regnety_tiny", "resnet_tiny"])
def test_frozen_trunk_and_groups_match_oracle(arch, case):
    ft.check_vs_oracle("cpu", arch, case)


@pytest.mark.parametrize("groups", [False, True], ids=["frozen", "frozen_groups"])
def test_clip_norm_leaves_frozen_gradients_out(groups):
    ft.check_clip_norm_frozen("cpu", groups)


def test_deterministic_runs_bitwise():
    ft.check_bitwise_runs("cpu")


def test_defaults_unchanged():
    ft.check_defaults_unchanged("cpu")


def test_resume():
    ft.check_resume("cpu")


def test_refusals():
    ft.check_refusals("cpu")


def test_eval_batchnorm1d_under_gradients_refused():
    ft.check_bn1d_eval_refused("cpu")


def test_trainer_keeps_frozen_batchnorms_in_eval(tmp_path):
    ft.check_trainer_keeps_frozen_bn("cpu", tmp_path)
