"""Cases for the 16-byte epilogue of the register-staged GEMM engine (transposed accumulator, GemmEpi::trn in tf_gemm_engine.h).  ``dev`` is
"cpu" for the emulated build (tests/test_engine_epilogue_emu.py) and "cuda" for the MI355X (tests/test_engine_epilogue_gpu.py).

Shapes are GEMM dimensions (M, N, K): an (M, N) output, a reduction over K.  The three of SHAPES are ragged in M, in N against the
32-column tile, and in the last k tile.  The switch (TF_GEMM_EPI16) is flipped inside the process through ops.gemm_epi16; whether a launch
really took the transposed form is read from ops.gemm_epi16_launches() - a counter, never a result-changing switch."""
import torch
import torch.nn.functional as F

from kernel_cases import R, TOL, c64, cl, close, _bn_from_parts
from transfuser_amd import ops

PLANS = [(64, 64, 16), (64, 64, 32), (128, 32, 16), (128, 32, 32), (128, 64, 32)]     # the last one has two tiles per wave (TM != TN): 4-byte epilogue
TRN_PLANS = PLANS[:4]
SHAPES = [(130, 216, 40), (203, 72, 40), (97, 24, 36)]
PAIR_CASES = [(132, 216, 40, 1), (260, 132, 72, 4)]


class switch:
    """with switch(on): the 16-byte epilogue forced on / off; the environment's setting comes back afterwards."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        assert ops.gemm_epi16(self.on) == self.on
        return self

    def __exit__(self, *a):
        ops.gemm_epi16(None)
        return False


def _counted(fn):
    n0 = ops.gemm_epi16_launches()
    out = fn()
    return out, ops.gemm_epi16_launches() - n0


def _ops_of(dev, M, N, K):
    """name -> (callable returning the output, fp64 reference)"""
    x, w, b, r = R(M, K, dev=dev), R(N, K, seed=1, dev=dev) * 0.1, R(N, seed=2, dev=dev), R(M, N, seed=3, dev=dev)
    seed = torch.tensor([4321], dtype=torch.int32, device=dev)
    dy, wd, act, acc0 = R(M, K, seed=4, dev=dev), R(K, N, seed=5, dev=dev) * 0.1, R(M, N, seed=6, dev=dev), R(M, N, seed=7, dev=dev)
    prod = c64(x) @ c64(w).t() + c64(b)
    return {
        "fwd bias relu": (lambda: ops.linear_fwd(x, w, b, relu=True), torch.relu(prod)),
        "fwd residual": (lambda: ops.linear_fwd(x, w, b, res=r), prod + c64(r)),
        "fwd dropout residual": (lambda: ops.linear_fwd(x, w, b, res=r, drop=(seed, 5, 0.1)), r),       # no fp64 reference: the kept share is checked
        # the library takes a ReLU mask with a plain store only (tf_gemm_f32): the mask and the += epilogue are two cases
        "dgrad mask": (lambda: ops.linear_dgrad(dy, wd, mask=act), (c64(dy) @ c64(wd)) * (c64(act) > 0)),
        "dgrad accumulate": (lambda: ops.linear_dgrad(dy, wd, out=acc0.clone(), accumulate=True), c64(acc0) + c64(dy) @ c64(wd)),
    }


def check_bitwise(dev, bm, bn, bk):
    """Switch on == switch off, bit for bit, from one build; on a one-tile-per-wave plan the on run must really be the transposed form."""
    trn = (bm, bn, bk) in TRN_PLANS
    ops.force_plan(bm, bn, bk, 1)
    try:
        for (M, N, K) in SHAPES:
            for name, (fn, ref) in _ops_of(dev, M, N, K).items():
                what = "%s %s plan %s" % (name, (M, N, K), (bm, bn, bk))
                with switch(True):
                    on, n_on = _counted(fn)
                with switch(False):
                    off, n_off = _counted(fn)
                assert n_off == 0, what
                assert n_on == (1 if trn else 0), (what, n_on)
                assert torch.equal(on, off), "%s: max diff %.3e" % (what, (on - off).abs().max().item())
                if ref.dtype == torch.float64:
                    close(on, ref, what=what)
                else:
                    kept = (on != ref).float().mean().item()
                    assert abs(kept - 0.9) < 0.05, (what, kept)
    finally:
        ops.force_plan(0)


def check_pair_bitwise(dev, M, N, K, splitk, bks=((32, 16), (16, 32))):
    """The pair bracket: the input-gradient side takes the transposed epilogue (mask + residual), the weight-gradient side keeps its atomics."""
    dy, x, w = R(M, N, dev=dev), R(M, K, seed=1, dev=dev), R(N, K, seed=2, dev=dev) * 0.1
    res, act = R(M, K, seed=3, dev=dev), R(M, K, seed=4, dev=dev)
    dw0 = R(N, K, seed=5, dev=dev) * 0.1
    want_dw = (dw0.double() + dy.double().t() @ x.double()).float()
    want_dx = ((dy.double() @ w.double() + res.double()) * (act > 0)).float()

    def run(bkw, bkd):
        n0 = ops.gemm_pair_count()
        dw = dw0.clone()
        try:
            with ops.gemm_pair(dy) as gp:
                assert gp.on
                ops.force_plan(64, 64, bkw, splitk)
                ops.linear_wgrad(dy, x, dw)
                ops.force_plan(64, 64, bkd, 1)
                dx = ops.linear_dgrad(dy, w, res=res, mask=act)
        finally:
            ops.force_plan(0)
        assert ops.gemm_pair_count() == n0 + 1, "the joint kernel did not run"
        return dw, dx

    for (bkw, bkd) in bks:
        what = "pair %s" % ((M, N, K, splitk, bkw, bkd),)
        with switch(True):
            (dw_on, dx_on), n_on = _counted(lambda: run(bkw, bkd))
        with switch(False):
            (dw_off, dx_off), n_off = _counted(lambda: run(bkw, bkd))
        # splitk 1: the weight gradient is a plain += and eligible as well; an atomic k-split is not
        assert n_off == 0 and n_on == (2 if splitk == 1 else 1), (what, n_on, n_off)
        assert torch.equal(dx_on, dx_off), "%s dgrad: max diff %.3e" % (what, (dx_on - dx_off).abs().max().item())
        close(dx_on, want_dx, tol=2e-5 * max(1, N // 64), what=what + " dgrad")
        close(dw_on, want_dw, tol=2e-5 * max(1, M // 64), what=what + " wgrad")
        close(dw_on, dw_off, tol=1e-6, what=what + " wgrad on vs off")


def check_fallbacks(dev, plan=(64, 64, 16)):
    """Calls the transposed epilogue cannot serve: right within TOL against fp64, and the counter shows they kept the 4-byte epilogue."""
    M, N, K = 130, 216, 40
    x, w, b, r = R(M, K, dev=dev), R(N, K, seed=1, dev=dev) * 0.1, R(N, seed=2, dev=dev), R(M, N, seed=3, dev=dev)
    want = c64(x) @ c64(w).t()
    ops.force_plan(*plan, 1)
    try:
        with switch(True):
            y, n = _counted(lambda: ops.linear_fwd(x, w, b, res=r))          # control: this one is eligible
            assert n == 1, n
            close(y, want + c64(b) + c64(r), what="aligned control")
            for n_odd in (90, 33):
                w2, b2 = R(n_odd, K, seed=1, dev=dev) * 0.1, R(n_odd, seed=2, dev=dev)
                y, n = _counted(lambda: ops.linear_fwd(x, w2, b2, relu=True))
                assert n == 0, (n_odd, n)
                close(y, torch.relu(c64(x) @ c64(w2).t() + c64(b2)), tol=TOL, what="N = %d" % n_odd)
            buf = torch.zeros(M * N + 4, device=dev)
            out = buf[1:1 + M * N].view(M, N)
            y, n = _counted(lambda: ops.linear_fwd(x, w, b, out=out))
            assert n == 0 and y.data_ptr() % 16 == 4, n
            close(y, want + c64(b), tol=TOL, what="output offset by one float")
            assert buf[0] == 0 and torch.all(buf[1 + M * N:] == 0)
            blong = R(N + 1, seed=9, dev=dev)
            y, n = _counted(lambda: ops.linear_fwd(x, w, blong[1:]))
            assert n == 0, n
            close(y, want + c64(blong)[1:], tol=TOL, what="bias[1:]")
            rbig = R(M, N + 2, seed=10, dev=dev)
            y, n = _counted(lambda: ops.linear_fwd(x, w, b, res=rbig[:, :N]))
            assert n == 0, n
            close(y, want + c64(b) + c64(rbig)[:, :N], tol=TOL, what="ldres % 4 != 0")
            # batched: the context product of an attention layer with head size 54 (transfuser.py:523-527) - head z writes at z * 54 floats
            B, nh, T, hs = 1, 4, 50, 54
            C, Tp = nh * hs, 52
            att = torch.zeros(B * nh, T, Tp, device=dev)
            att[:, :, :T] = torch.softmax(R(B * nh, T, T, seed=11, dev=dev), -1)
            qkv = R(B, T, 3 * C, seed=12, dev=dev, scale=0.5)
            yb = torch.empty(B, T, C, device=dev)
            _, n = _counted(lambda: ops.gemm(att, qkv[..., 2 * C:], yb, T, hs, T, Tp, 3 * C, C, b_trans=True, batch=B * nh, inner=nh,
                                             sa=(nh * T * Tp, T * Tp), sb=(T * 3 * C, hs), sc=(T * C, hs)))
            assert n == 0, n
            vh = c64(qkv)[..., 2 * C:].reshape(B, T, nh, hs).transpose(1, 2)
            ref = (c64(att)[:, :, :T].reshape(B, nh, T, T) @ vh).transpose(1, 2).reshape(B, T, C)
            close(yb, ref, tol=TOL, what="batched, sc_inner = 54")
    finally:
        ops.force_plan(0)


def check_stats(dev, bm, bn, bk):
    """BatchNorm statistics from the epilogue with the switch on: counts exact, moments within 1e-3 (inputs shifted by +3: mean >> spread).
    The eligibility rule keeps these launches on the column-per-lane epilogue; the counter pins that."""
    old_fuse = ops.FUSE_BN_STATS
    ops.FUSE_BN_STATS = True
    ops.force_plan(bm, bn, bk, 1)
    try:
        with switch(True):
            for (m, n, k) in ((203, 72, 40), (130, 216, 64), (97, 24, 36)):
                x = R(m, k, dev=dev) + 3.0
                w = R(n, k, seed=5, dev=dev) * 0.2
                (y, cs), n16 = _counted(lambda: ops.linear_fwd(x, w, colstat=True))
                assert n16 == 0, "launches that carry statistics keep the column-per-lane epilogue (tf_gemm_engine.h: epi16_eligible)"
                close(y, c64(x) @ c64(w).t(), what="linear with colstat %s" % ((m, n, k),))
                _bn_from_parts(dev, y.view(1, 1, m, n), cs, relu=(n != 24), res=R(1, 1, m, n, seed=8, dev=dev) if n == 72 else None)
    finally:
        ops.force_plan(0)
        ops.FUSE_BN_STATS = old_fuse


def check_grouped_bias_alignment(dev, B=1, H=9, W=13, C=48):
    """The direct grouped 3x3 kernel's transposed form loads its bias 16 bytes at a time; the launcher sends a bias pointer that is not 16-byte
    aligned to the other form.  This case checks the RESULT of such a call only: the library has no query for which grouped instantiation ran, and a
    misaligned 16-byte load also works on gfx950 and in the emulator, so it does not prove that the guard was taken."""
    from transfuser_amd.ops import ptr, wptr, stream_of, check
    x = R(B, C, H, W, dev="cpu")
    w = R(C, 24, 3, 3, seed=1, dev="cpu") * 0.1
    blong = R(C + 1, seed=2, dev="cpu")
    want = torch.relu(F.conv2d(x.double(), w.double(), blong[1:].double(), 1, 1, 1, C // 24))
    xh, wh, bh = x.permute(0, 2, 3, 1).contiguous().to(dev), cl(w).to(dev), blong.to(dev)[1:]
    assert bh.data_ptr() % 16 == 4
    yh = torch.empty(B, H, W, C, device=dev)
    check(ops.L().tf_conv3x3_grouped_fwd_f32(ptr(xh), wptr(wh), ptr(bh), ptr(yh), B, H, W, C, 1, stream_of(xh)), "grouped fwd")
    close(yh.permute(0, 3, 1, 2), want, what="grouped fwd, bias offset by one float")
