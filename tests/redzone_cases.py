"""Shared cases of tests/test_redzone_emu.py (host emulator) and tests/test_redzone_gpu.py (MI355X), in three groups:

1. the guard harness of tests/redzone.py checked on itself (every write goes through torch indexing INTO the harness's own base buffer:
   inside the allocation, no kernel involved);
2. coverage pins: under the guard the op-level checks really allocate through it (output, ColStat buffer, k-split scratch);
3. one eager model step and the entry points of ops.py that had no op-level check, against float64 / exact references, under the guard and at
   ragged sizes.

Tolerances of group 3 (kernel_cases.close: max abs error <= tol * max(1, max |reference|)): 1e-5 for element-wise fp32 arithmetic of up to
~10 operations and for sums of at most 37 fp32 terms (fp32 epsilon 6e-8 x operations x a safety factor of ~10; the bound check_adamw uses for
the same AdamW arithmetic); exact (torch.equal) wherever the result is a copy, a selection or an exactly representable product."""
import math

import numpy as np
import pytest
import torch

import kernel_cases as kc
import model_cases as mc
import redzone
from transfuser_amd import ops

REAL_TORCH = torch
INT32_MAX = 2147483647


# ---------------------------------------------------------------- 1. the harness on itself
def check_band_reports(dev):
    """One element written into the band before and one into the band after: each reported with the allocating function, the side and the offset."""
    with redzone.guarded(ops) as g:
        for dtype, value in ((torch.float32, 1.5), (torch.int32, 7), (torch.bfloat16, 0.0), (torch.uint8, 3)):
            t = ops.torch.empty(5, 7, dtype=dtype, device=dev)
            rec = g.records[-1]
            g.verify()                                          # untouched: clean (and the record is dropped)
            assert g.records == []
            for side, index, offset in (("before", rec.band - 3, -3), ("after", rec.band + t.numel() + 5, 5)):
                t = ops.torch.empty(5, 7, dtype=dtype, device=dev)
                rec = g.records[-1]
                rec.base[index] = value
                with pytest.raises(AssertionError) as e:
                    g.verify()
                msg = str(e.value)
                assert "check_band_reports (redzone_cases.py:" in msg and "torch.empty" in msg and "band %s broken at offsets %d .. %d (1 elements" % (side, offset, offset) in msg, msg
                assert str(dtype).replace("torch.", "") in msg and "[5, 7]" in msg, msg
                assert ("before" if side == "after" else "after") + " broken" not in msg, msg
                g.verify()                                      # cleared by the failing call
        # a write INSIDE the tensor, first and last element, is not reported
        t = ops.torch.zeros(3, 5, device=dev)
        t[0, 0], t[2, 4] = 1.0, 2.0
        g.verify()
        # two broken allocations: both listed, first and last offset of a run
        a, b = ops.torch.empty(9, device=dev), ops.torch.ones(4, 300, dtype=torch.int64, device=dev)
        ra, rb = g.records[-2:]
        ra.after()[0:4] = 0.0
        rb.before()[-2:] = 1
        with pytest.raises(AssertionError) as e:
            g.verify()
        msg = str(e.value)
        assert "2 guard band(s) written" in msg and "band after broken at offsets 0 .. 3 (4 elements" in msg and "band before broken at offsets -2 .. -1 (2 elements" in msg, msg


def check_poison_and_fill(dev):
    """An untouched ``empty`` reads as all-NaN / all-sentinel; zeros / ones / full hold their value inside and poison outside."""
    with redzone.guarded(ops) as g:
        pt = ops.torch
        for dtype, pat in redzone.POISON.items():
            t = pt.empty(3, 11, dtype=dtype, device=dev)
            rec = g.records[-1]
            assert t.dtype == dtype and t.shape == (3, 11) and t.device.type == torch.device(dev).type
            assert bool(t.isnan().all()) if pat != pat else bool((t == pat).all()), dtype
            assert bool(redzone._is_poison(rec.base).all())
            z = pt.zeros(3, 11, dtype=dtype, device=dev)
            rec = g.records[-1]
            assert bool((z == 0).all()), dtype
            assert bool(redzone._is_poison(rec.before()).all()) and bool(redzone._is_poison(rec.after()).all()) and rec.before().numel() == rec.band == rec.after().numel()
            assert rec.band * rec.base.element_size() == 4096
        o, f, fl = pt.ones(4, device=dev), pt.full((1,), 777, dtype=torch.int32, device=dev), pt.full_like(torch.zeros(2, 3, device=dev), 2.5)
        assert bool((o == 1).all()) and f.tolist() == [777] and f.dtype == torch.int32 and bool((fl == 2.5).all()) and fl.shape == (2, 3)
        assert pt.full((2,), 3, device=dev).dtype == torch.full((2,), 3).dtype and pt.ones_like(f).tolist() == [1]
        assert bool(pt.empty_like(o).isnan().all()) and bool((pt.zeros_like(o) == 0).all())
        s = pt.empty((), dtype=torch.float32, device=dev)            # 0-dim: one element
        assert s.dim() == 0 and math.isnan(float(s))
        assert pt.zeros(2, 2, device=dev, requires_grad=True).requires_grad
        g.verify()
        assert g.passthroughs == [], g.passthroughs


def check_band_size():
    """max(4096 bytes, two rows) per side, a multiple of 512 bytes, at most 1 MiB."""
    assert redzone.band_elems((1,), 4) == 1024 and redzone.band_elems((), 4) == 1024 and redzone.band_elems((40, 1), 4) == 1024
    assert redzone.band_elems((600, 1), 4) == 1280          # 4800 bytes -> 5120
    assert redzone.band_elems((9, 3000, 1), 2) == 6144      # 12000 bytes -> 12288: the row stride, not the outer one
    assert redzone.band_elems((1 << 20, 1), 4) == (1 << 20) // 4
    assert redzone.band_elems((513, 1), 1) == 4096 and redzone.band_elems((2049, 1), 8) == 4160


def check_strides_and_alignment(dev):
    """Shapes and strides are real torch's (channels_last, ``*_like`` of a permuted tensor and of a sliced view); the interior starts on a
    512-byte boundary whatever the dtype and size."""
    with redzone.guarded(ops) as g:
        pt = ops.torch
        cl = torch.zeros(2, 6, 5, 7, device=dev).to(memory_format=torch.channels_last)
        perm = torch.zeros(4, 5, 6, device=dev).permute(2, 0, 1)
        sliced = torch.zeros(9, 40, device=dev)[:, 8:29]
        for like in (cl, perm, sliced, sliced.t(), torch.zeros(3, device=dev)):
            for fn in ("empty_like", "zeros_like", "ones_like"):
                want = getattr(torch, fn)(like)
                got = getattr(pt, fn)(like)
                assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype and got.device == want.device, (fn, like.stride())
                assert got.data_ptr() % 512 == 0
            want, got = torch.full_like(like, 3.0), pt.full_like(like, 3.0)
            assert got.stride() == want.stride() and torch.equal(got, want)
        assert pt.empty_like(cl).is_contiguous(memory_format=torch.channels_last)
        want = torch.empty(2, 6, 5, 7, device=dev, memory_format=torch.channels_last)
        got = pt.empty(2, 6, 5, 7, device=dev, memory_format=torch.channels_last)
        assert got.stride() == want.stride()
        assert pt.empty_like(cl, dtype=torch.int32).dtype == torch.int32 and pt.empty_like(cl, memory_format=torch.contiguous_format).is_contiguous()
        for dtype in redzone.POISON:
            for n in (1, 3, 1003, 4097):
                t = pt.empty(n, dtype=dtype, device=dev)
                assert t.data_ptr() % 512 == 0 and t.is_contiguous() and t.numel() == n
        assert pt.empty((7, 3), device=dev).shape == (7, 3) and pt.zeros([2, 2], device=dev).shape == (2, 2) and pt.empty(torch.Size((4,)), device=dev).shape == (4,)
        g.verify()
        assert g.passthroughs == []


def check_passthroughs(dev):
    """What the guard cannot serve goes to real torch and is counted, with the calling site and the reason."""
    with redzone.guarded(ops) as g:
        pt = ops.torch
        assert pt.empty(0, 5, device=dev).shape == (0, 5)
        assert pt.zeros(3, dtype=torch.complex64, device=dev).dtype == torch.complex64
        dst = torch.ones(4, device=dev)
        assert pt.zeros(4, out=dst) is dst and bool((dst == 0).all())
        assert pt.zeros_like(torch.zeros(0, device=dev)).numel() == 0
        assert g.guarded == 0 and len(g.records) == 0
        reasons = [r for _, r in g.passthroughs]
        assert len(reasons) == 4 and reasons[0] == "zero elements" and "complex64" in reasons[1] and "out" in reasons[2] and reasons[3] == "zero elements", reasons
        assert all(site.startswith("check_passthroughs (redzone_cases.py:") for site, _ in g.passthroughs), g.passthroughs
        pt.empty(1, device=dev)
        assert g.guarded == 1 and len(g.passthroughs) == 4
        g.verify()


def check_restored(dev):
    """The real torch (and the real R) are back after the block, also after an exception; the tensor caches of ops are empty on both sides."""
    assert ops.torch is REAL_TORCH and kc.torch is REAL_TORCH
    real_R = kc.R
    ops.workspace(torch.device(dev))
    assert ops._ws_cache
    with redzone.guarded(ops, kc) as g:
        assert ops.torch is not REAL_TORCH and kc.torch is ops.torch and kc.R is not real_R and ops.torch.float32 is torch.float32
        assert not ops._ws_cache and not ops._zpool
        ws = ops.workspace(torch.device(dev))
        assert g.records[-1].func == "workspace" and bool((ws == 0).all())
        x = kc.R(5, 3, dev=dev)
        assert torch.equal(x.cpu(), real_R(5, 3)) and g.records[-1].func == "check_restored" and bool(g.records[-1].after().isnan().all())
    assert ops.torch is REAL_TORCH and kc.torch is REAL_TORCH and kc.R is real_R and not ops._ws_cache and g.records == []
    with pytest.raises(ZeroDivisionError):
        with redzone.guarded(ops, kc):
            ops.workspace(torch.device(dev))
            1 / 0
    assert ops.torch is REAL_TORCH and kc.torch is REAL_TORCH and kc.R is real_R and not ops._ws_cache


# ---------------------------------------------------------------- 2. coverage pins
def check_pin_gemm(dev):
    with redzone.guarded(ops, kc) as g:
        kc.check_gemm(dev, 130, 216, 40)
        n_ops = sum(n for site, n in g.sites.items() if "(ops.py:" in site)
        assert n_ops >= 3 and g.passthroughs == [], (g.sites, g.passthroughs)
        assert any(site.startswith("check_gemm (kernel_cases.py:") for site in g.sites), g.sites      # the operands (R)
        g.verify()


def check_pin_colstat(dev):
    with redzone.guarded(ops, kc) as g:
        kc.check_bn_fused_stats(dev, plans=((0, 128, 32, 16), (2, 0, 0, 0)))
        assert sum(n for site, n in g.sites.items() if site.startswith("ColStat.__init__ (ops.py:")) >= 1, g.sites
        g.verify()


def check_pin_splitk_scratch(dev):
    with redzone.guarded(ops, kc) as g:
        kc.check_two_pass_splitk(dev, *kc.TWO_PASS_CASES[0])
        assert sum(n for site, n in g.sites.items() if site.startswith("gemm (ops.py:")) >= 1, g.sites       # skws, sized by tf_gemm_splitk_ws_floats
        g.verify()


# ---------------------------------------------------------------- 3a. one eager model step
def check_model_step(dev):
    """The tiny RegNetY TransFuser pair of test_tiny_model_losses_and_grads, forward and backward, with every tensor the product allocates
    between guard bands: the same comparison with the oracle, then the bands.  No graph capture."""
    from transfuser_amd import functions, model, regnet, transfuser
    with redzone.guarded(ops, functions, model, transfuser, regnet, mc) as g:
        if dev == "cpu":
            cfg = mc.tiny_config(n_layer=2)
            prod, ref = mc.build_pair(cfg, "regnety_tiny", dev)
            batch = mc.small_batch(2, 32, 64, 64, 40)
            lp, lr = mc.run_pair(prod, ref, cfg, batch, dev)
            mc.compare(prod, ref, lp, lr, verbose=True)
        else:
            cfg = mc.tiny_config(n_layer=2, lidar_res=128)
            prod, ref = mc.build_pair(cfg, "regnety_tiny", dev)
            batch = mc.small_batch(2, 160, 352, 128, 40)
            lp, lr = mc.run_pair(prod, ref, cfg, batch, dev)
            mc.compare(prod, ref, lp, lr, grad_tol=5e-3, verbose=True, metric="l2")
        assert g.guarded >= 100 and sum(n for site, n in g.sites.items() if "(ops.py:" in site) >= 100, g.guarded
        g.verify()


# ---------------------------------------------------------------- 3b. entry points without an op-level check
def _inputs(dev, *shape, seed=None, scale=1.0):
    """kernel_cases.R inside the guard: the operand sits between NaN bands."""
    assert kc.R is not getattr(kc.R, "__wrapped__", kc.R), "call inside redzone.guarded(ops, kernel_cases)"
    return kc.R(*shape, seed=seed, dev=dev, scale=scale)


def _guarded_copy(t):
    """A computed operand moved between bands as well."""
    out = ops.torch.empty(t.shape, dtype=t.dtype, device=t.device)
    assert out.data_ptr() != t.data_ptr() and ops.torch is not REAL_TORCH
    out.copy_(t)
    return out


def check_sigmoid(dev):
    with redzone.guarded(ops, kc) as g:
        for shape in ((1003,), (1,), (3, 5, 7), (257, 129)):
            x = _inputs(dev, *shape, scale=4.0)
            if x.numel() > 8:
                x.view(-1)[:4] = torch.tensor([-100.0, 100.0, 0.0, -20.0], device=dev)       # saturation on both sides
            y = ops.sigmoid(x)
            assert y.shape == x.shape and bool(torch.isfinite(y).all())
            kc.close(y, 1.0 / (1.0 + torch.exp(-kc.c64(x))), tol=1e-5, what="sigmoid")
        g.verify()


def check_weighted_sum(dev):
    """n = 1, 5 and 16 scalar terms, each an element of its own 1003-element allocation (the last term is the LAST element, next to the band);
    added in index order."""
    with redzone.guarded(ops, kc) as g:
        for n in (1, 5, 16):
            hold = [_inputs(dev, 1003, seed=n * 20 + i) for i in range(n)]
            terms = [t[1002 if i == n - 1 else (i * 67) % 1003] for i, t in enumerate(hold)]
            weights = [0.25 * (i + 1) * (-1) ** i for i in range(n)]
            got = ops.weighted_sum(terms, weights)
            assert got.shape == () and got.dtype == torch.float32
            want = sum(w * float(t) for w, t in zip(weights, terms))
            assert abs(float(got) - want) <= 1e-5 * max(1.0, sum(abs(w * float(t)) for w, t in zip(weights, terms))), (n, float(got), want)
            out = ops.torch.empty(3, device=dev)                  # a caller's buffer: only out[0] may change
            ops.weighted_sum(terms, weights, out=out)
            assert float(out[0]) == float(got) and bool(out[1:].isnan().all())
            dtotal = _inputs(dev, 1, seed=5)
            for d in (dtotal, None):
                gb = ops.weighted_sum_bwd(d, weights, torch.device(dev))
                assert gb.shape == (n,)
                scale = np.float32(1.0) if d is None else np.float32(float(d))
                assert gb.tolist() == [float(np.float32(w) * scale) for w in weights], (n, gb.tolist())
        with pytest.raises(RuntimeError):
            ops.weighted_sum([_inputs(dev, 1)] * 17, [1.0] * 17)
        g.verify()


def check_cast_f32(dev):
    """bf16 -> fp32 with a scale: exact for a power-of-two scale, one rounding otherwise."""
    with redzone.guarded(ops, kc) as g:
        for n in (1003, 1, 4096 + 5):
            xb = _guarded_copy(_inputs(dev, n, scale=3.0).to(torch.bfloat16))
            out = ops.torch.empty(n, dtype=torch.float32, device=dev)
            assert ops.cast_f32(xb, out) is out and torch.equal(out, xb.float())
            out = ops.torch.empty(n, dtype=torch.float32, device=dev)
            assert torch.equal(ops.cast_f32(xb, out, scale=0.125), xb.float() * 0.125)
            out = ops.torch.empty(n, dtype=torch.float32, device=dev)
            assert torch.equal(ops.cast_f32(xb, out, scale=1.0 / 3.0).cpu(), (xb.float().cpu() * np.float32(1.0 / 3.0)))
            back = ops.cast_bf16(out)                            # and its inverse, fp32 -> bf16 round to nearest even
            assert back.dtype == torch.bfloat16 and torch.equal(back, out.to(torch.bfloat16))
        g.verify()


def _adamw64(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.01):
    p, g, m, v = (kc.c64(t) for t in (p, g, m, v))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p * (1 - lr * wd) - lr / (1 - b1 ** step) * (m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps))
    return p, m, v


def check_adamw_dynscale(dev, n=1003):
    """Two finite steps (gradients divided by the loss scale, clean-step count advanced, scale doubled at the growth interval of 2), then a step
    with an inf in the LAST element of the checked arena (outside the parameters' own gradient, on the arena's scalar tail) and one with a NaN in
    its vector body: parameters and moments bit-identical, the step count unchanged, the scale halved but never below 1."""
    with redzone.guarded(ops, kc) as g:
        lr, scale = 1e-2, 1024.0
        p, m, v = _inputs(dev, n), _inputs(dev, n, seed=1, scale=0.1), _guarded_copy(_inputs(dev, n, seed=2, scale=0.1).abs())
        arena = _guarded_copy(_inputs(dev, 2 * n + 45, seed=3) * scale)            # 2051 elements: three past the last float4
        grad = arena[:n]
        state = _guarded_copy(torch.tensor([0.0, lr], device=dev))
        ls = _guarded_copy(torch.tensor([scale, 0.0, 0.0, 2.0], device=dev))          # [scale, clean steps, found_inf, growth interval]
        lr32 = float(np.float32(lr))
        for step in (1, 2):
            want = _adamw64(p, kc.c64(grad) / scale, m, v, step, lr)
            ops.adamw_dynscale_(p, grad, m, v, state, ls, arena)
            for got, ref, what in zip((p, m, v), want, ("p", "m", "v")):
                kc.close(got, ref, tol=1e-5, what="adamw_dynscale step %d %s" % (step, what))
            assert state.tolist() == [float(step), lr32], state.tolist()
            assert ls.tolist() == ([scale, 1.0, 0.0, 2.0] if step == 1 else [2 * scale, 0.0, 0.0, 2.0]), ls.tolist()
        before = [t.clone() for t in (p, m, v)]
        arena[-1] = float("inf")
        ops.adamw_dynscale_(p, grad, m, v, state, ls, arena)
        for got, old, what in zip((p, m, v), before, ("p", "m", "v")):
            assert torch.equal(got, old), "adamw_dynscale: %s changed in a skipped step" % what
        assert state.tolist() == [2.0, lr32] and ls.tolist() == [scale, 0.0, 0.0, 2.0], (state.tolist(), ls.tolist())
        arena[-1] = 0.0
        arena[n + 8] = float("nan")
        ls.copy_(torch.tensor([1.0, 1.0, 0.0, 2.0]))
        ops.adamw_dynscale_(p, grad, m, v, state, ls, arena)
        assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)) and ls.tolist() == [1.0, 0.0, 0.0, 2.0] and float(state[0]) == 2.0
        g.verify()


def _close_abs(a, b, bound, what):
    err = float((kc.c64(a) - b).abs().max())
    assert err <= bound, "%s: max err %.3e (bound %.3e)" % (what, err, bound)      # (a NaN fails: the comparison is False)


BN_ROWS_CASES = [(37, 37, 64), (37, 23, 64), (1, 1, 64), (37, 37, 8), (37, 37, 7), (1, 1, 7)]      # (rows_cap, live rows, C)


def check_bn_rows_dev_bwd(dev, rows, live, C):
    """BatchNorm1d + ReLU backward over the first ``live`` rows (the count read on the device) against float64 on the same inputs (z, save_mean,
    save_invstd from the product's forward): dx, ACCUMULATED dgamma / dbeta, dx rows beyond the count zero.  The kernels exist for widths
    dividing 256: C = 7 must be refused by both directions with nothing written."""
    with redzone.guarded(ops, kc) as g:
        x, dz = _guarded_copy(_inputs(dev, rows, C, scale=2.0) + 0.5), _inputs(dev, rows, C, seed=1)
        gamma, beta = _guarded_copy(_inputs(dev, C, seed=2).abs() + 0.5), _inputs(dev, C, seed=3, scale=0.3)
        nrows = ops.torch.full((2,), live, dtype=torch.int32, device=dev)
        rm, rv = ops.torch.zeros(C, device=dev), ops.torch.ones(C, device=dev)
        dgamma0, dbeta0 = _inputs(dev, C, seed=4), _inputs(dev, C, seed=5)
        dgamma, dbeta = _guarded_copy(dgamma0), _guarded_copy(dbeta0)
        if 256 % C:
            with pytest.raises(RuntimeError, match="dividing 256"):
                ops.bn_rows_dev_fwd(x, nrows, gamma, beta, rm, rv, 0.1, 1e-5)
            sm, si, z = _inputs(dev, C, seed=6), _inputs(dev, C, seed=7), _inputs(dev, rows, C, seed=8)
            with pytest.raises(RuntimeError, match="dividing 256"):
                ops.bn_rows_dev_bwd(dz, z, x, nrows, gamma, sm, si, dgamma, dbeta)
            assert torch.equal(dgamma, dgamma0) and torch.equal(dbeta, dbeta0) and bool((rm == 0).all()) and bool((rv == 1).all())
            g.verify()
            return
        z, sm, si = ops.bn_rows_dev_fwd(x, nrows, gamma, beta, rm, rv, 0.1, 1e-5)
        x64 = kc.c64(x)[:live]
        mean, var = x64.mean(0), x64.var(0, unbiased=False)
        kc.close(sm, mean, tol=1e-5, what="bn_rows_dev save_mean")
        kc.close(si, 1.0 / torch.sqrt(var + 1e-5), tol=1e-5, what="bn_rows_dev save_invstd")
        # Both apply passes are the usual scale / shift forms (z = x * sc + sh with sh = beta - mean * sc; dx = A g + Bc x + Cc with A = gamma * invstd):
        # differences of products of size |x| * gamma * invstd resp. A * |g|, each product rounded to fp32 (unit round-off 2^-24).  With ONE live row
        # invstd is 1 / sqrt(eps) = 316, so the absolute bound is that product magnitude x 2^-24 x 8 (the handful of roundings in the form), on top
        # of the 1e-5 of this module's docstring - worked out from the operands, not from what the kernel returns.
        u, A = 2.0 ** -24, kc.c64(gamma) * kc.c64(si)
        zr = torch.relu((x64 - mean) / torch.sqrt(var + 1e-5) * kc.c64(gamma) + kc.c64(beta))
        _close_abs(z[:live], zr, 1e-5 + 8 * u * float((x64.abs() * A).max()), "bn_rows_dev z")
        assert bool((z[live:] == 0).all())
        dx = ops.bn_rows_dev_bwd(dz, z, x, nrows, gamma, sm, si, dgamma, dbeta)
        xhat = (x64 - kc.c64(sm)) * kc.c64(si)
        gm = kc.c64(dz)[:live] * (kc.c64(z)[:live] > 0)
        db, dg = gm.sum(0), (gm * xhat).sum(0)
        want = A * (gm - db / live - xhat * dg / live)
        assert dx.shape == x.shape and bool(torch.isfinite(dx).all())
        _close_abs(dx[:live], want, 1e-5 + 8 * u * float((A * gm.abs()).max() + (A * kc.c64(si) * dg.abs() / live * x64.abs()).max()), "bn_rows_dev_bwd dx")
        assert bool((dx[live:] == 0).all()), "rows beyond the device count must be written as zero"
        kc.close(dbeta, kc.c64(dbeta0) + db, tol=1e-5, what="bn_rows_dev_bwd dbeta (+=)")
        kc.close(dgamma, kc.c64(dgamma0) + dg, tol=1e-5, what="bn_rows_dev_bwd dgamma (+=)")
        g.verify()


PILLAR_CLOUDS = [kc.PILLAR_CASES[2], kc.PILLAR_CASES[1]]      # (1, 64, (64,)) and (2, 3000, (0, 3000)): a tiny cloud, an empty sample
assert PILLAR_CLOUDS == [(1, 64, (64,)), (2, 3000, (0, 3000))]


def _pillar_cell(key, GX, GY, H, W):
    cy, cx, b = key % GY, (key // GY) % GX, key // (GY * GX)
    return (b * H + np.minimum(cy, H - 1)) * W + np.minimum(cx, W - 1)


def check_pillar_scatter_canvas(dev, B, N, npts, C=5, Ce=1):
    """ops.pillar_scatter_max / pillar_canvas / pillar_canvas_bwd on a real pillar index against a numpy scatter: EXACT (a maximum, a copy,
    a selection).  C = 5: no vector width divides the rows; ties (duplicated feature rows) resolve to the lowest point row."""
    with redzone.guarded(ops, kc) as g:
        pts = kc.pillar_cloud(B, N)
        ix = ops.pillar_index(pts.to(dev), torch.tensor(npts, dtype=torch.int32).to(dev), -16, 16, -32, 0, 8)
        n, P, GX, GY, H, W = ix["N"], ix["P"], ix["GX"], ix["GY"], ix["nx"], ix["ny"]
        assert n > 0 and 0 < P <= n and (H, W) == (256, 256)
        z = torch.relu(_inputs(dev, n, C, seed=4))                # post-ReLU features: about half are exact zeros
        z[1::2][:n // 4] = z[0::2][:n // 4]                         # ties between neighbouring rows
        z = _guarded_copy(z)
        inv, key = ix["inv"].cpu().numpy().astype(np.int64), ix["cellkey"].cpu().numpy().astype(np.int64)
        pf, arg = ops.pillar_scatter_max(z, ix["inv"], P)
        zn = z.cpu().numpy()
        pf_ref = np.zeros((P, C), np.float32)
        np.maximum.at(pf_ref, inv, zn)
        arg_ref = np.full((P, C), INT32_MAX, np.int64)
        hit = (zn > 0) & (zn == pf_ref[inv])
        np.minimum.at(arg_ref, inv, np.where(hit, np.arange(n)[:, None], INT32_MAX))
        assert pf.shape == (P, C) and arg.dtype == torch.int32
        assert np.array_equal(pf.cpu().numpy(), pf_ref), "pillar_scatter_max: features"
        assert np.array_equal(arg.cpu().numpy(), arg_ref), "pillar_scatter_max: arg (lowest row attaining the maximum)"
        extra = (torch.rand(B, Ce, H, W, generator=torch.Generator().manual_seed(4)) < 0.05).float()
        extra_d = _guarded_copy(extra.to(dev))
        for ex, ce in ((extra_d, Ce), (None, 0)):
            out, owner = ops.pillar_canvas(pf, ix["cellkey"], B, H, W, GX, GY, ex)
            owner_ref = np.full(B * H * W, -1, np.int64)
            np.maximum.at(owner_ref, _pillar_cell(key, GX, GY, H, W), np.arange(P))           # index_put: the highest-rank duplicate wins
            out_ref = np.zeros((B * H * W, C + ce), np.float32)
            out_ref[:, :C] = np.where(owner_ref[:, None] >= 0, pf_ref[np.maximum(owner_ref, 0)], 0.0)
            if ce:
                out_ref[:, C:] = extra.permute(0, 2, 3, 1).reshape(B * H * W, ce).numpy()
            assert np.array_equal(owner.cpu().numpy(), owner_ref), "pillar_canvas: owner"
            assert out.shape == (B, H, W, C + ce) and np.array_equal(out.cpu().numpy().reshape(B * H * W, C + ce), out_ref), "pillar_canvas: canvas"
            dout = _inputs(dev, B, H, W, C + ce, seed=6)
            dz = ops.pillar_canvas_bwd(dout, owner, ix["cellkey"], ix["inv"], arg, C, GX, GY)
            cell = _pillar_cell(key[inv], GX, GY, H, W)
            live = (arg_ref[inv] == np.arange(n)[:, None]) & (owner_ref[cell] == inv)[:, None]
            dz_ref = np.where(live, dout.cpu().numpy().reshape(B * H * W, C + ce)[cell][:, :C], np.float32(0.0))
            assert dz.shape == (n, C) and np.array_equal(dz.cpu().numpy(), dz_ref), "pillar_canvas_bwd"
            assert 0 < int(live.sum()) < live.size
        g.verify()
