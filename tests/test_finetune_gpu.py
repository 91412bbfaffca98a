"""Fine-tuning on the MI355X: the parameter-group AdamW / norm kernels and the frozen-statistics BatchNorm backward against float64, frozen
parameters and groups through the Engine against the CPU oracle, the captured step against the eager one (with set_group between replays),
bitwise reproducibility, resume and the unchanged defaults.  Cases: tests/finetune_cases.py."""
import pytest
import torch

import accum_clip_cases as acc
import finetune_cases as ft
import kernel_cases as kc
import redzone
from transfuser_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPTURES_A_GRAPH = ("test_graph_matches_eager_and_set_group_between_replays",)      # outside the guard


@pytest.fixture(autouse=True)
def _gpu(request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, ft, acc, kc, outside=CAPTURES_A_GRAPH)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
        ops.force_plan(0)


@pytest.mark.parametrize("arena,table", ft.GROUP_ADAMW_CASES)
def test_group_adamw(arena, table):
    ft.check_group_adamw(DEV, arena, table)


def test_one_default_group_is_plain_adamw_bitwise():
    ft.check_one_group_is_plain_adamw(DEV)


def test_group_sumsq_and_clip():
    ft.check_group_sumsq_clip(DEV)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "frozen_affine"])
@pytest.mark.parametrize("relu,with_res", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("shape", ft.BN_FROZEN_SHAPES)
def test_bn_bwd_frozen(shape, relu, with_res, affine):
    ft.check_bn_frozen(DEV, *shape, relu, with_res, affine)


def test_eval_mode_batchnorm_module_backward():
    ft.check_eval_bn_module_backward(DEV)


def test_kernel_argument_refusals():
    ft.check_kernel_refusals(DEV)


@pytest.mark.parametrize("by_hand", [False, True], ids=["freeze_arg", "requires_grad_false"])
def test_frozen_parameters_stay_put(by_hand):
    ft.check_frozen_stay(DEV, by_hand)


@pytest.mark.parametrize("case", ["lr_mult", "no_decay_1d"])
@pytest.mark.parametrize("arch", ["regnety_tiny", "resnet_tiny"])
def test_frozen_trunk_and_groups_match_oracle(arch, case):
    ft.check_vs_oracle(DEV, arch, case)


@pytest.mark.parametrize("groups", [False, True], ids=["frozen", "frozen_groups"])
def test_clip_norm_leaves_frozen_gradients_out(groups):
    ft.check_clip_norm_frozen(DEV, groups)


def test_graph_matches_eager_and_set_group_between_replays():
    ft.check_graph_matches_eager(DEV)


def test_deterministic_runs_bitwise():
    ft.check_bitwise_runs(DEV)


def test_defaults_unchanged():
    ft.check_defaults_unchanged(DEV)


def test_resume():
    ft.check_resume(DEV)


def test_refusals():
    ft.check_refusals(DEV)


def test_eval_batchnorm1d_under_gradients_refused():
    ft.check_bn1d_eval_refused(DEV)
