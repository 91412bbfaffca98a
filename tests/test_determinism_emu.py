"""Deterministic mode on the host emulator: the cases of tests/test_determinism_gpu.py against the same float64 references (the emulator runs
blocks sequentially: this pins indexing, ragged edges and scratch sizing of the fixed-order forms, not ordering), the two modes side by side on
the tiny model, and the switch itself.  Cases: tests/determinism_cases.py."""
import os
import subprocess
import sys

import pytest

import determinism_cases as dc
import kernel_cases as kc
import redzone
from transfuser_amd import ops

DEV = "cpu"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(autouse=True)
def _backend(emu_backend, request):
    prev = ops.is_deterministic()
    try:
        yield from redzone.fixture_guard(request, ops, dc, kc)      # guard bands + NaN poison around every tensor ops / the cases allocate
    finally:
        ops.set_deterministic(prev)
        ops.force_plan(0)
        ops.gemm_epi16(None)


def test_flag_round_trip():
    dc.check_flag_round_trip()


def test_environment_sets_the_initial_value():
    """TF_DETERMINISTIC=1 is how `python bench.py` runs in the mode: a fresh process starts with the flag on, without it off."""
    emu = os.path.join(ROOT, "tests", "emu", "libtransfuser_emu.so")          # built by the emu_backend fixture; the flag lives in the library
    code = "import ctypes; from transfuser_amd import _lib, ops; _lib._install_test_backend(ctypes.CDLL(%r)); print(int(ops.is_deterministic()))" % emu
    for val, want in (("1", "1"), (None, "0"), ("0", "0")):
        env = {k: v for k, v in os.environ.items() if k != "TF_DETERMINISTIC"}
        if val is not None:
            env["TF_DETERMINISTIC"] = val
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want, (val, out.stdout, out.stderr)


@pytest.mark.parametrize("m", dc.KSPLIT_M)
@pytest.mark.parametrize("splitk", dc.KSPLIT_S)
@pytest.mark.parametrize("variant", dc.ENGINE_VARIANTS)
def test_engine_ksplit_plain(variant, splitk, m):
    dc.check_engine_ksplit_plain(DEV, variant, splitk, m)


@pytest.mark.parametrize("case", dc.engine_wgrad_conv_cases(), ids=lambda c: "x".join(map(str, c)))
def test_engine_ksplit_conv_wgrad(case):
    dc.check_engine_ksplit_conv(DEV, *case)


@pytest.mark.parametrize("site", dc.QUERY_SITES)
def test_scratch_query_agrees_with_launch(site):
    dc.check_scratch_query_agrees(DEV, site)


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


def test_mode_agreement():
    dc.check_mode_agreement(DEV)


def test_refusals():
    dc.check_refusals(DEV)
