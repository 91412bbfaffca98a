"""Deterministic mode on the MI355X: the fixed-order forms of every reduction that by default ends in fp32 atomics are bitwise reproducible,
never launch a float-atomic kernel form, agree with float64 references, and make a whole fp32 train step (eager and captured) a pure function
of its inputs.  Cases: tests/determinism_cases.py."""
import pytest
import torch

import determinism_cases as dc
import kernel_cases as kc
import redzone
from transfuser_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPTURES_A_GRAPH = ("test_train_step_bitwise_regnet[graph]",)      # outside the guard


@pytest.fixture(autouse=True)
def _gpu(request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, dc, kc, outside=CAPTURES_A_GRAPH)      # guard bands + NaN poison around every tensor ops / the cases allocate
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
        ops.force_plan(0)
        ops.gemm_epi16(None)


# 1. engine k-split, plain
@pytest.mark.parametrize("m", dc.KSPLIT_M)
@pytest.mark.parametrize("splitk", dc.KSPLIT_S)
@pytest.mark.parametrize("variant", dc.ENGINE_VARIANTS)
def test_engine_ksplit_plain(variant, splitk, m):
    dc.check_engine_ksplit_plain(DEV, variant, splitk, m)


def test_engine_ksplit_trunk_shape_unpinned():
    dc.check_engine_ksplit_trunk_shape(DEV)


# 2. engine k-split, implicit-GEMM convolution weight gradient
@pytest.mark.parametrize("case", dc.engine_wgrad_conv_cases(), ids=lambda c: "x".join(map(str, c)))
def test_engine_ksplit_conv_wgrad(case):
    dc.check_engine_ksplit_conv(DEV, *case)


def test_engine_conv_case_list_covers_the_new_case():
    cases = dc.engine_wgrad_conv_cases()
    assert (2, 12, 20, 40, 72, 3, 2, 1) in cases and any(c[7] == 1 for c in cases)


@pytest.mark.parametrize("site", dc.QUERY_SITES)
def test_scratch_query_agrees_with_launch(site):
    dc.check_scratch_query_agrees(DEV, site)


# 3. the other sites
@pytest.mark.parametrize("rows,C", dc.LN_CASES)
def test_layernorm_dw(rows, C):
    dc.check_layernorm_dw(DEV, rows, C)


@pytest.mark.parametrize("B,C,Cr", dc.SE_CASES)
def test_se_excite_bwd(B, C, Cr):
    dc.check_se_excite_bwd(DEV, B, C, Cr)


def test_smallm_dgrad():
    dc.check_smallm_dgrad(DEV)


def test_skinny_wgrad():
    dc.check_skinny_wgrad(DEV)


@pytest.mark.parametrize("stride", [1, 2])
def test_grouped_wgrad(stride):
    dc.check_grouped_wgrad(DEV, stride)


# 4. the existing kernel case lists under the switch
def test_existing_gemm_cases_under_the_switch():
    with ops.deterministic():
        for case in kc.GEMM_CASES:
            kc.check_gemm(DEV, *case)


def test_existing_conv_cases_under_the_switch():
    with ops.deterministic():
        for case in kc.CONV_CASES:
            kc.check_conv(DEV, *case)


def test_existing_reduction_cases_under_the_switch():
    with ops.deterministic():
        a0 = ops.float_atomic_launches()
        for rows, C in [(37, 72), (9, 216), (5, 1512), (6, 576), (3, 2048), (4, 70), (2, 2052), (130, 288)]:      # the list of tests/test_kernels_gpu.py::test_layernorm
            kc.check_layernorm(DEV, rows, C)
        kc.check_fused_finalize(DEV)
        kc.check_skinny_wgrad(DEV)
        assert ops.float_atomic_launches() == a0


# 5. train step, eager and captured
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_train_step_bitwise_regnet(use_graph):
    dc.check_train_step_bitwise(DEV, "regnety_tiny", use_graph)


def test_train_step_bitwise_resnet():
    dc.check_train_step_bitwise(DEV, "resnet_tiny", False)


# 6. mode agreement
def test_mode_agreement():
    dc.check_mode_agreement(DEV)


# 7. refusals
def test_refusals():
    dc.check_refusals(DEV)
    torch.cuda.synchronize()
