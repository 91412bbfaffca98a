"""Deterministic mode, measurement 3 of its pull request: the dominant weight-gradient shapes as (a) the default atomic k-split, (b) the ordered
slab k-split of the same plan under ops.deterministic(), (c) unsplit under the flag (ops.force_plan(..., splitk=1): the trivial deterministic
form, best of a few tiles).  Event timing, warm-up, three alternating rounds, no profiler.  `python tools/determinism_bench.py` on an MI355X."""
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from transfuser_amd import ops  # noqa: E402

SHAPES = [(7040, 576, 576), (28160, 216, 216), (28160, 72, 216), (112640, 72, 72)]      # (rows, out features of dy, features of x)
UNSPLIT_TILES = [(64, 64, 32), (128, 64, 32), (128, 128, 16)]


def timed(fn, iters=50, warm=10):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us per call


def main():
    ops.plans_load(os.path.join(ROOT, "transfuser_amd", "plans", "mi355x.txt"))
    ops.L().tf_build_id.restype = __import__("ctypes").c_char_p
    print("build id %s" % ops.L().tf_build_id().decode())
    print("%-22s %-10s %s" % ("dy x (rows, n, k)", "form", "us per call, three rounds"))
    for rows, n, k in SHAPES:
        g = torch.Generator().manual_seed(0)
        dy, x = torch.randn(rows, n, generator=g).cuda(), torch.randn(rows, k, generator=g).cuda()
        dw = torch.zeros(n, k, device="cuda")
        call = lambda: ops.linear_wgrad(dy, x, dw, accumulate=True)
        res = {"atomic (default)": [], "slab (flag)": [], "unsplit (flag)": []}
        for _ in range(3):
            with ops.deterministic(False):
                a0 = ops.float_atomic_launches()
                res["atomic (default)"].append(timed(call))
                atomic_ran = ops.float_atomic_launches() > a0
            with ops.deterministic(True):
                s0 = ops.slab_splitk_launches()
                res["slab (flag)"].append(timed(call))
                slab_ran = ops.slab_splitk_launches() > s0
                best = 1e30
                for bm, bn, bk in UNSPLIT_TILES:
                    ops.force_plan(bm, bn, bk, 1)
                    try:
                        best = min(best, timed(call, iters=20, warm=3))
                    finally:
                        ops.force_plan(0)
                res["unsplit (flag)"].append(best)
        for name, v in res.items():
            note = "" if name != "atomic (default)" or atomic_ran else "  (plan does not split K)"
            note = note if name != "slab (flag)" or slab_ran else "  (no slab launch: plan does not split K)"
            print("%-22s %-18s %s%s" % ((rows, n, k), name, "  ".join("%9.1f" % t for t in v), note))


if __name__ == "__main__":
    main()
