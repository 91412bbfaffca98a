"""Deterministic mode (ops.set_deterministic / tf_set_deterministic): shared cases of tests/test_determinism_gpu.py (MI355X) and
tests/test_determinism_emu.py (host emulator).  Every case runs a reduction that by default ends in fp32 atomics through its fixed-order form
and checks three things: the launch counters (tf_float_atomic_launches stands still, and moves for the same call with the flag off - so the
counter is live), bitwise equality of repeated calls from identical inputs, and the value against a float64 CPU reference within the tolerance
the site's existing kernel_cases.check_* applies (kernel_cases.close, TOL = 1e-3 of the reference's scale; 3e-5 for the skinny weight gradient).
The emulator runs blocks sequentially, so there the cases pin indexing, ragged edges and scratch sizing rather than ordering."""
import contextlib
import ctypes

import torch
import torch.nn.functional as F

import kernel_cases as kc
from transfuser_amd import ops

close, c64, R = kc.close, kc.c64, kc.R


def repeats(dev):
    return 3      # (on the emulator too: a repeated call meets the scratch its predecessor left behind)


def run_det(dev, fn, slab=None):
    """fn() -> tensor(s), called repeats(dev) times with the flag on: the float-atomic counter must not move, every call returns the same bits;
    slab: True / False = the ordered slab k-split counter must / must not advance on every call.  Returns the first result."""
    outs = []
    with ops.deterministic():
        for _ in range(repeats(dev)):
            a0, s0 = ops.float_atomic_launches(), ops.slab_splitk_launches()
            out = fn()
            out = tuple(o.detach().clone() for o in (out if isinstance(out, (tuple, list)) else (out,)))
            assert ops.float_atomic_launches() == a0, "a float-atomic kernel form ran under the deterministic flag"
            if slab is not None:
                assert (ops.slab_splitk_launches() > s0) == slab, ("slab k-split launches", s0, ops.slab_splitk_launches(), slab)
            outs.append(out)
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), "repeated deterministic calls differ"
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


def atomic_form_is_counted(fn):
    """The same call with the flag off takes its atomic form and moves tf_float_atomic_launches."""
    with ops.deterministic(False):
        a0 = ops.float_atomic_launches()
        fn()
        assert ops.float_atomic_launches() > a0, "the default form of this call did not count as a float-atomic launch"


# ---------------------------------------------------------------- 1. engine k-split, plain GEMM
ENGINE_VARIANTS = ("reg4", "reg16", "dma")      # register-staged kernel with the 4-byte / the 16-byte epilogue, an LDS-DMA kind
KSPLIT_M = (72, 12)                             # 12: the default mode's swapped (column-strided) orientation, which this mode must not take
KSPLIT_S = (3, 7)


class pinned:
    """with pinned(variant, splitk): one engine tiling for every call inside."""

    def __init__(self, variant, splitk):
        self.variant, self.splitk = variant, splitk

    def __enter__(self):
        if self.variant == "dma":
            ops.force_dma(2, self.splitk)                     # 64 x 64 x 16 LDS-DMA configuration
        else:
            ops.gemm_epi16(self.variant == "reg16")
            ops.force_plan(64, 64, 16, self.splitk)
        return self

    def __exit__(self, *a):
        ops.force_plan(0)
        ops.gemm_epi16(None)
        return False


def check_engine_ksplit_plain(dev, variant, splitk, m):
    """linear_wgrad, dy (2056, m), x (2056, 136) into a non-zero dW: K = 2056 leaves a ragged last slice for 3 and 7 slices, 72 / 12 / 136 ragged tiles."""
    dy, x, dw0 = R(2056, m, dev=dev), R(2056, 136, seed=1, dev=dev), R(m, 136, seed=2, dev=dev)
    want = c64(dw0) + c64(dy).t() @ c64(x)
    call = lambda: ops.linear_wgrad(dy, x, dw0.clone(), accumulate=True)
    with pinned(variant, splitk):
        e0 = ops.gemm_epi16_launches()
        dw = run_det(dev, call, slab=True)
        if variant == "reg16":
            assert ops.gemm_epi16_launches() > e0, "the slab store did not take the 16-byte epilogue"
        if variant == "reg4":
            assert ops.gemm_epi16_launches() == e0
        atomic_form_is_counted(call)
    close(dw, want, what="slab k-split wgrad %s S=%d m=%d" % (variant, splitk, m))


def check_engine_ksplit_trunk_shape(dev):
    """One unpinned call at the dominant weight-gradient shape of the trunks (dy, x: (7040, 576)) with the shipped plans: the scratch the query
    sizes for a real plan is what the launch uses."""
    import os
    plan_file = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "plans", "mi355x.txt")
    if os.path.exists(plan_file):
        ops.plans_load(plan_file)
    dy, x, dw0 = R(7040, 576, dev=dev, scale=0.1), R(7040, 576, seed=1, dev=dev, scale=0.1), R(576, 576, seed=2, dev=dev)
    dw = run_det(dev, lambda: ops.linear_wgrad(dy, x, dw0.clone(), accumulate=True))
    close(dw, c64(dw0) + c64(dy).t() @ c64(x), what="slab k-split wgrad (7040, 576, 576)")


# ---------------------------------------------------------------- 2. engine k-split, implicit-GEMM convolution weight gradient
def engine_wgrad_conv_cases():
    """The kernel_cases.CONV_CASES that ops._conv_wgrad sends to tf_conv2d_wgrad_f32 (not thin, direct or grouped) + a 3x3 / stride-2 case with
    ragged channel counts."""
    out = []
    for (B, Hi, Wi, Cin, Cout, ks, stride, groups) in kc.CONV_CASES + [(2, 12, 20, 40, 72, 3, 2, 1)]:
        shape, pad = (B, Hi, Wi, Cin), ks // 2
        if ops._thin_ok(shape, Cout, Cin, ks, stride, pad, groups) or ops._grouped_ok(shape, Cout, Cin, ks, stride, pad, groups) or \
                ops._grouped_s2_ok(shape, Cout, Cin, ks, stride, pad, groups):
            continue
        if ops._direct_ok(shape, Cout, Cin, ks, stride, pad, groups) and (Cout <= ops._DIRECT_WGRAD_MAX_COUT or ops._DIRECT_MIN_PIXELS == 0):
            continue
        out.append((B, Hi, Wi, Cin, Cout, ks, stride, groups))
    return out


def check_engine_ksplit_conv(dev, B, Hi, Wi, Cin, Cout, ks, stride, groups, splitk=3):
    x = R(B, Cin, Hi, Wi, dev="cpu")
    w64 = (c64(R(Cout, Cin // groups, ks, ks, dev="cpu")) * 0.1).requires_grad_(True)
    y = F.conv2d(c64(x), w64, None, stride, ks // 2, 1, groups)
    dy = R(*y.shape, seed=1, dev="cpu")
    (gw,) = torch.autograd.grad(y, [w64], c64(dy))
    xh, dyh = x.permute(0, 2, 3, 1).contiguous().to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
    dw0 = kc.cl(R(Cout, Cin // groups, ks, ks, seed=2, dev="cpu")).to(dev)
    call = lambda: ops.conv_wgrad(dyh, xh, dw0.clone(memory_format=torch.preserve_format), stride, None, groups)
    with pinned("reg4", splitk):
        # one group: the k-slices go through the slabs; grouped calls are batched GEMMs, which this mode runs unsplit
        dw = run_det(dev, call, slab=(groups == 1))
        atomic_form_is_counted(call)
    close(dw, c64(dw0) + gw, what="slab k-split conv wgrad %s" % ((B, Hi, Wi, Cin, Cout, ks, stride, groups),))


# ---------------------------------------------------------------- 2b. the scratch query agrees with the launch
# pins of the engine plan; the two-pass / stream-K codes are kernel_cases.TWO_PASS / STREAM_K (include/transfuser_hip.h, tf_force_dma)
QUERY_PINS = {"none": None, "reg3": ("reg4", 3), "dma3": ("dma", 3), "dma-twopass3": ("dma", kc.TWO_PASS + 3), "dma-streamk": ("dma", kc.STREAM_K)}
QUERY_SITES = ("tn72", "tn12", "tn136", "conv24", "conv48", "stem7")


def _query_site(dev, site):
    """-> (query() -> floats, call(ws, floats) -> result, float64 reference, (m, n) of the engine's row-major output, plain operands?)."""
    from ctypes import byref, c_long
    from transfuser_amd.ops import ptr, wptr, stream_of, check, c_p
    L = ops.L()
    if site.startswith("tn"):          # plain [tn] accumulation, k = 1030; m = 12 is the shape whose default orientation is swapped; 136 x 136: 9 tiles of 64 x 64 (a cut stream-K launch)
        m, n, k = int(site[2:]), (136 if site == "tn136" else 96), 1030
        dy, x, dw0 = R(k, m, dev=dev), R(k, n, seed=1, dev=dev), R(m, n, seed=2, dev=dev)
        flags = ops._sk_flags(dy.device)

        def desc(dw, ws, floats):
            return ops.GemmDesc(a=ptr(dy), b=ptr(x), c=ptr(dw), bias=c_p(0), res=c_p(0), m=m, n=n, k=k, a_trans=1, b_trans=1, lda=m, ldb=n, ldc=n, ldres=0, batch=1,
                                inner=1, alpha=1.0, relu=0, accumulate=1, mask=c_p(0), ldmask=0, splitk_ws=ptr(ws), splitk_ws_floats=floats, sk_flags=ptr(flags))

        def call(ws, floats):
            dw = dw0.clone()
            check(L.tf_gemm_f32(byref(desc(dw, ws, floats)), stream_of(dy)), "tf_gemm_f32")
            assert not flags.any(), "stream-K flags must be clear between launches"
            return dw
        return (lambda: ops._ws_query()(byref(desc(dw0, None, 0)))), call, c64(dw0) + c64(dy).t() @ c64(x), (m, n), True
    if site.startswith("conv"):        # one-group 3x3 convolution weight gradient; Cout = 24 is swapped by default
        B, H, W, Cin, Cout = 2, 6, 10, 8, int(site[4:])
        x = R(B, Cin, H, W, dev="cpu")
        w64 = (c64(R(Cout, Cin, 3, 3, dev="cpu")) * 0.1).requires_grad_(True)
        y = F.conv2d(c64(x), w64, None, 1, 1)
        dy = R(*y.shape, seed=1, dev="cpu")
        (gw,) = torch.autograd.grad(y, [w64], c64(dy))
        xh, dyh = x.permute(0, 2, 3, 1).contiguous().to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
        dw0 = kc.cl(R(Cout, Cin, 3, 3, seed=2, dev="cpu")).to(dev)
        g = ops.conv_geom(xh.shape, Cout, 3, 1, 1, 1)
        L.tf_conv2d_wgrad_ws_floats.restype = c_long

        def call(ws, floats):
            dw = dw0.clone(memory_format=torch.preserve_format)
            check(L.tf_conv2d_wgrad_ws_f32(byref(g), ptr(dyh), ptr(xh), wptr(dw), 1, ptr(ws), c_long(floats), stream_of(dyh)), "tf_conv2d_wgrad_ws_f32")
            return dw
        return (lambda: L.tf_conv2d_wgrad_ws_floats(byref(g))), call, c64(dw0) + gw, (Cout, 9 * Cin), False
    # the 7x7 / stride 2 stem weight gradient: ops.stem_conv_wgrad asks tf_stem_conv_wgrad_ws_floats and brings exactly that
    rgb = torch.randint(0, 256, (2, 3, 32, 32), generator=torch.Generator().manual_seed(0)).float().to(dev)
    w64 = (c64(R(16, 3, 7, 7, dev=dev)) * 0.1).requires_grad_(True)
    mean, std = c64(torch.tensor([0.485, 0.456, 0.406], device=dev)).view(1, 3, 1, 1), c64(torch.tensor([0.229, 0.224, 0.225], device=dev)).view(1, 3, 1, 1)
    y = F.conv2d((c64(rgb) / 255.0 - mean) / std, w64, None, 2, 3)
    dy = R(*y.shape, seed=1, dev=dev)
    (gw,) = torch.autograd.grad(y, [w64], c64(dy))
    dyh, dw0 = dy.permute(0, 2, 3, 1).contiguous(), kc.cl(R(16, 3, 7, 7, seed=2, dev=dev))
    g = ops.conv_geom((2, 32, 32, 3), 16, 7, 2, 3, 1)
    L.tf_stem_conv_wgrad_ws_floats.restype = c_long
    call = lambda ws, floats: ops.stem_conv_wgrad(dyh, rgb, None, dw0.clone(memory_format=torch.preserve_format), True, True, 2, 3)
    return (lambda: L.tf_stem_conv_wgrad_ws_floats(byref(g), 3, 0)), call, c64(dw0) + gw, (16, 147), False


def check_scratch_query_agrees(dev, site):
    """Every pin of QUERY_PINS, flag on and off: ask the site's scratch query, make the call with EXACTLY that scratch, and read off the counters
    that the launch took the form the answer implies (both come from resolve_plan, csrc/gemm_plan.cpp):
    under the flag the float-atomic counter stands still, the slab counter moves exactly when an atomic-split plan (pinned or heuristic) was
    answered with need > 0, and never with need == 0; a pinned stream-K plan runs as stream-K exactly when need > 0 (the 136 x 136 output is cut
    on the 8 emulated CUs and on the MI355X alike, the 4-tile outputs never are); a pinned two-pass plan is answered with its 3 slices of
    m * round_up(n, 4) for a row-major plain call and with 0 where the launch cannot take it (column-strided swapped orientation, implicit-GEMM
    operands).  Results: bitwise equal run to run wherever no float atomics ran, and close (TOL) to the float64 product."""
    query, call, want, (m, n), plain = _query_site(dev, site)
    L = ops.L()
    L.tf_streamk_launches.restype = ctypes.c_long
    slice_floats = m * ((n + 3) // 4 * 4)
    for pin, spec in QUERY_PINS.items():
        for flag in (True, False):
            with ops.deterministic(flag), (pinned(*spec) if spec else contextlib.nullcontext()):
                need = query()
                ws = torch.empty(need, dtype=torch.float32, device=dev) if need > 0 else None
                outs = []
                for _ in range(2):
                    a0, s0, k0 = ops.float_atomic_launches(), ops.slab_splitk_launches(), L.tf_streamk_launches()
                    outs.append(call(ws, need))
                    atomic, slab, streamk = ops.float_atomic_launches() > a0, ops.slab_splitk_launches() > s0, L.tf_streamk_launches() > k0
                    what = "%s pin %s flag %d: need %d atomic %d slab %d stream-K %d" % (site, pin, flag, need, atomic, slab, streamk)
                    assert streamk == (pin == "dma-streamk" and need > 0), what
                    if flag:
                        assert not atomic, what
                        assert slab == (need > 0 and pin in ("none", "reg3", "dma3")), what
                    else:
                        assert not slab, what
                    if pin == "dma-twopass3":
                        swapped = not flag and site in ("tn12", "conv24")
                        assert need == (3 * slice_floats if plain and not swapped else 0), what
                        assert not atomic and not slab, what
                    if pin == "dma-streamk":
                        assert (need > 0) == (site == "tn136"), what
                if not atomic:
                    assert torch.equal(outs[0], outs[1]), what + ": repeated calls differ"
                close(outs[0], want, what=what)


# ---------------------------------------------------------------- 3. the other sites
LN_CASES = [(130, 288), (37, 72)]
SE_CASES = [(2, 72, 18), (3, 576, 144)]


def check_layernorm_dw(dev, rows, C):
    x, dy = R(rows, C, dev=dev), R(rows, C, seed=3, dev=dev)
    g, b = R(C, seed=1, dev=dev) * 0.3 + 1, R(C, seed=2, dev=dev)
    dg0, db0 = R(C, seed=4, dev=dev), R(C, seed=5, dev=dev)
    x64, g64, b64 = c64(x).requires_grad_(True), c64(g).requires_grad_(True), c64(b).requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(F.layer_norm(x64, (C,), g64, b64, 1e-5), [x64, g64, b64], c64(dy))
    _, mean, rstd = ops.layernorm_fwd(x, g, b)

    def call():
        dg, db = dg0.clone(), db0.clone()
        return ops.layernorm_bwd(dy, x, g, mean, rstd, dg, db), dg, db
    dx, dg, db = run_det(dev, call)
    atomic_form_is_counted(call)
    close(dx, gx, what="ln dx")
    close(dg, c64(dg0) + gg, what="ln dgamma (accumulated)")
    close(db, c64(db0) + gb, what="ln dbeta (accumulated)")
    # the dropout-fused backward takes the same route
    seed = torch.tensor([1234], dtype=torch.int32, device=dev)

    def call_drop():
        dg, db = dg0.clone(), db0.clone()
        return ops.layernorm_bwd(dy, x, g, mean, rstd, dg, db, drop=(seed, 3, 0.1))[0], dg, db
    dx2, dg2, db2 = run_det(dev, call_drop)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)


def check_se_excite_bwd(dev, B, C, Cr):
    s = R(B, C, dev=dev)
    w1, b1 = R(Cr, C, 1, 1, seed=1, dev=dev, scale=0.1), R(Cr, seed=2, dev=dev, scale=0.1)
    w2, b2 = R(C, Cr, 1, 1, seed=3, dev=dev, scale=0.1), R(C, seed=4, dev=dev, scale=0.1)
    dgate = R(B, C, seed=5, dev=dev)
    s64, p64 = c64(s).requires_grad_(True), [c64(t).requires_grad_(True) for t in (w1, b1, w2, b2)]
    ref = F.linear(F.relu(F.linear(s64, p64[0].view(Cr, C), p64[1])), p64[2].view(C, Cr), p64[3])
    gs, *gp = torch.autograd.grad(ref, [s64] + p64, c64(dgate))
    acc = [R(*t.shape, seed=6 + i, dev=dev) for i, t in enumerate((w1, b1, w2, b2))]

    def call():
        g1, _ = ops.se_excite_fwd(s, w1, b1, w2, b2)
        out = [a.clone() for a in acc]
        return (ops.se_excite_bwd(dgate, s, g1, w1, w2, *out), *out)
    ds, *out = run_det(dev, call)
    atomic_form_is_counted(call)
    close(ds, gs, what="se excite ds")
    for o, a, g, n in zip(out, acc, gp, ("dW1", "db1", "dW2", "db2")):
        close(o, c64(a) + g, what="se excite " + n)


def check_smallm_dgrad(dev, M=2, N=600, K=70):
    dy, w = R(M, N, dev=dev), R(N, K, seed=1, dev=dev)
    call = lambda: ops.linear_dgrad(dy, w)
    dx = run_det(dev, call)
    atomic_form_is_counted(call)
    close(dx, c64(dy) @ c64(w), what="small-m dgrad")
    dx0 = R(M, K, seed=2, dev=dev)
    acc = run_det(dev, lambda: ops.linear_dgrad(dy, w, out=dx0.clone(), accumulate=True))
    close(acc, c64(dx0) + c64(dy) @ c64(w), what="small-m dgrad (accumulate)")


def check_skinny_wgrad(dev, rows=4096 + 37, no=3, C=64):
    dyb = R(rows, no + 3, dev=dev)
    dy = dyb[:, 1:1 + no]
    x, dw0 = R(rows, C, seed=1, dev=dev), R(no, C, seed=2, dev=dev)
    call = lambda: ops.gemm(dy, x, dw0.clone(), no, C, rows, dyb.stride(0), x.stride(0), C, a_trans=True, b_trans=True, accumulate=True)
    dw = run_det(dev, call, slab=False)
    atomic_form_is_counted(call)
    close(dw, c64(dw0) + c64(dy).t() @ c64(x), tol=3e-5, what="skinny wgrad")


def check_grouped_wgrad(dev, stride, B=2, H=6, W=10, C=48):
    """Both strides of the grouped 3x3 weight gradient (group width 24) and their BatchNorm-apply-folded twins, accumulating into a non-zero dW."""
    from transfuser_amd.ops import ptr, wptr, stream_of, check, c_p
    groups = C // 24
    x = R(B, C, H, W, dev="cpu")
    sc, sh = R(C, seed=7, dev="cpu") * 0.5 + 1.0, R(C, seed=8, dev="cpu") * 0.7 + 0.3
    z = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    w64 = (c64(R(C, 24, 3, 3, dev="cpu")) * 0.1).requires_grad_(True)
    y = F.conv2d(c64(x), w64, None, stride, 1, 1, groups)
    dy = R(*y.shape, seed=1, dev="cpu")
    (gw,) = torch.autograd.grad(y, [w64], c64(dy))
    (gwz,) = torch.autograd.grad(F.conv2d(c64(z), w64, None, stride, 1, 1, groups), [w64], c64(dy))
    xh, dyh = x.permute(0, 2, 3, 1).contiguous().to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
    dw0 = kc.cl(R(C, 24, 3, 3, seed=2, dev="cpu")).to(dev)
    coef = torch.cat([sc, sh]).to(dev)
    L, ws = ops.L(), ops._grouped_ws(xh.device)

    def run(folded):
        dw = dw0.clone(memory_format=torch.preserve_format)
        cf = ptr(coef) if folded else c_p(0)
        if stride == 2:
            check(L.tf_conv3x3_grouped_s2_wgrad_f32(ptr(dyh), ptr(xh), cf, wptr(dw), B, H, W, C, 1, ptr(ws), stream_of(xh)), "grouped s2 wgrad")
        elif folded:
            check(L.tf_conv3x3_grouped_bnrelu_wgrad_f32(ptr(dyh), ptr(xh), cf, wptr(dw), B, H, W, C, 1, ptr(ws), stream_of(xh)), "grouped bnrelu wgrad")
        else:
            check(L.tf_conv3x3_grouped_wgrad_f32(ptr(dyh), ptr(xh), wptr(dw), B, H, W, C, 1, ptr(ws), stream_of(xh)), "grouped wgrad")
        return dw
    for folded, want in ((False, gw), (True, gwz)):
        dw = run_det(dev, lambda: run(folded))
        atomic_form_is_counted(lambda: run(folded))
        close(dw, c64(dw0) + want, what="grouped wgrad stride %d folded %d" % (stride, folded))
    if stride == 1:      # and through the public dispatch
        dw = run_det(dev, lambda: ops.conv_wgrad(dyh, xh, dw0.clone(memory_format=torch.preserve_format), 1, None, groups))
        close(dw, c64(dw0) + gw, what="ops.conv_wgrad -> grouped")


# ---------------------------------------------------------------- 5 / 6. the train step and the two modes side by side
LOSS_W = [1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.3, 0.4]


def train_run(dev, arch, use_graph, deterministic, steps=3):
    """`steps` Engine.train_step calls on a freshly built tiny model (same seed every time) -> (losses of every step, final parameter arena,
    float-atomic launches issued meanwhile)."""
    import model_cases as mc
    import transfuser_amd.transfuser as ptf
    from transfuser_amd.train import Engine
    cfg = mc.tiny_config(n_layer=2, lidar_res=64, dropout=0.1)
    batch = {k: v.to(dev) for k, v in mc.small_batch(2, 32, 64, 64, 40).items()}
    prev = ops.is_deterministic()
    try:
        ptf.GPT._site_base = 0          # dropout sites are numbered per constructed GPT: the same masks for every run
        prod, _ = mc.build_pair(cfg, arch, dev)
        prod.train()
        eng = Engine(prod, cfg, lr=1e-3, use_graph=use_graph, autotune=False, deterministic=deterministic)
        a0 = ops.float_atomic_launches()
        losses = []
        for _ in range(steps):
            tot, det = eng.train_step(batch)
            losses.append([float(tot)] + [float(det[k]) for k in cfg.detailed_losses])
        if dev != "cpu":
            torch.cuda.synchronize()
        return losses, eng.arena.params.detach().clone(), ops.float_atomic_launches() - a0
    finally:
        ops.set_deterministic(prev)


def check_train_step_bitwise(dev, arch, use_graph):
    la, pa, na = train_run(dev, arch, use_graph, True)
    lb, pb, nb = train_run(dev, arch, use_graph, True)
    assert la == lb, (la, lb)
    assert torch.equal(pa, pb), "parameter arenas differ after 3 deterministic steps: %d of %d elements" % (int((pa != pb).sum()), pa.numel())
    if not use_graph:
        assert na == 0 and nb == 0, "float-atomic kernel forms ran in a deterministic eager step: %d" % na
        _, _, nd = train_run(dev, arch, False, False, steps=1)
        assert nd > 0, "a default-mode step issued no float-atomic launch: the counter is not live"


def forward_backward(dev, deterministic):
    import model_cases as mc
    import transfuser_amd.transfuser as ptf
    cfg = mc.tiny_config(n_layer=2, lidar_res=64, dropout=0.1)
    b = {k: v.to(dev) for k, v in mc.small_batch(2, 32, 64, 64, 40).items()}
    w = dict(zip(cfg.detailed_losses, LOSS_W))
    with ops.deterministic(deterministic):
        ptf.GPT._site_base = 0
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        prod.train()
        lp = prod(b['rgb'], b['lidar'], ego_waypoint=b['ego_waypoint'], target_point=b['target_point'], target_point_image=b['target_point_image'],
                  ego_vel=b['ego_vel'].reshape(-1, 1), bev=b['bev'], label=b['label'], depth=b['depth'], semantic=b['semantic'])
        sum(w[k] * v for k, v in lp.items()).backward()
    return {k: float(v.detach()) for k, v in lp.items()}, {n: q.grad.detach().clone() for n, q in prod.named_parameters() if q.grad is not None}


def check_mode_agreement(dev):
    """Default and deterministic mode compute the same sums in another order: losses within 1e-6 relative, every gradient within 1e-5 of its
    tensor's max (the bounds model_cases.check_round5_fusions_bitwise uses for summation-order differences)."""
    (la, ga), (lb, gb) = forward_backward(dev, False), forward_backward(dev, True)
    assert all(abs(la[k] - lb[k]) <= 1e-6 * max(1.0, abs(lb[k])) for k in lb), (la, lb)
    assert ga.keys() == gb.keys()
    for n in ga:
        err = (ga[n] - gb[n]).abs().max().item() / max(gb[n].abs().max().item(), 1e-6)
        assert err < 1e-5, (n, err)


# ---------------------------------------------------------------- 7. refusals
def check_refusals(dev):
    import pytest
    import model_cases as mc
    from transfuser_amd.train import Engine
    B, H, W, C = 1, 8, 8, 16
    x, dy = R(B, H, W, C, dev=dev), R(B, H, W, C, seed=1, dev=dev)
    dw, db = torch.zeros(C, 1, 7, 7, device=dev), torch.zeros(C, device=dev)
    with ops.deterministic():
        with pytest.raises(RuntimeError, match="tf_set_deterministic"):
            ops.dwconv7_wgrad(dy, x, dw, db)
    ops.dwconv7_wgrad(dy, x, dw, db)            # the default mode runs it
    assert float(dw.abs().max()) > 0
    prev = ops.is_deterministic()
    try:
        cfg = mc.tiny_config(n_layer=1)
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        with pytest.raises(NotImplementedError, match="fp32"):
            Engine(prod, cfg, precision="bf16", deterministic=True, autotune=False)
    finally:
        ops.set_precision("fp32")
        ops.set_deterministic(prev)


def check_flag_round_trip():
    prev = ops.is_deterministic()
    try:
        ops.set_deterministic(True)
        assert ops.is_deterministic() and ops.L().tf_get_deterministic() == 1
        with ops.deterministic(False):
            assert not ops.is_deterministic() and ops.L().tf_get_deterministic() == 0
            with ops.deterministic():
                assert ops.is_deterministic()
            assert not ops.is_deterministic()
        assert ops.is_deterministic() and ops.L().tf_get_deterministic() == 1
        ops.set_deterministic(False)
        assert not ops.is_deterministic() and ops.L().tf_get_deterministic() == 0
    finally:
        ops.set_deterministic(prev)
