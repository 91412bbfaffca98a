"""Shared cases of tests/test_finetune_emu.py (host emulator) and tests/test_finetune_gpu.py (MI355X): frozen parameters, frozen-statistics
BatchNorm and AdamW parameter groups (Engine(freeze=..., param_groups=..., freeze_bn=...), FlatAdamW(groups=...), ops.adamw_groups_,
ops.grad_sumsq_groups, ops.bn_bwd(frozen=True)).

Tolerances, none of them measured on the code under test:
* group AdamW vs a float64 restatement per group: 1e-5 (kernel_cases.close), the bound of kernel_cases.check_adamw / accum_clip_cases.check_adamw_clip
  for the same arithmetic; frozen tiles and everything outside the updated range: torch.equal;
* sum of squares / norm without the frozen tiles vs float64 of the same fp32 data: accum_clip_cases.sumsq_bound (roundings on the longest path);
* frozen-statistics BatchNorm vs float64 autograd of F.batch_norm(training=False): kernel_cases.close's default 1e-3, as kernel_cases.check_bn;
* Engine vs the CPU oracle with torch.optim.AdamW param groups: losses 1e-3 relative and parameters 4.4e-3 x lr_mult after two steps at lr 1e-3
  (test_model_emu.test_engine_two_steps_match_oracle_adamw: AdamW moves a weight by ~lr sign(g) when |g| is at round-off level, so two fp32
  implementations may differ by 2 lr per step on isolated elements - with a group's lr = lr x lr_mult); frozen parameters torch.equal;
* graph vs eager: the bounds of accum_clip_cases.check_graph_matches_eager."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import accum_clip_cases as acc
import kernel_cases as kc
import model_cases as mc
from transfuser_amd import ops

R = kc.R
TILE = 64                       # floats per arena tile (train._ALIGN, ops.GROUP_TILE)
BLOCK_SPAN = 1024               # floats one block of the group AdamW kernel covers per trip: 256 threads x one float4 = 16 tiles
GROUP_GRID_CAP = 2048           # its grid cap (csrc/misc.cpp kGroupGridCap): past 2048 x 1024 floats a block takes a second grid-stride trip
PREFIX = "_model.image_encoder"

# rows (lr_mult, weight_decay, frozen): the frozen group first, in the middle, last; lr_mult in {0.1, 1, 3}, weight_decay in {0, 0.01, 0.3}
TABLES = {
    "frozen_first": [(3.0, 0.3, True), (1.0, 0.01, False), (0.1, 0.0, False)],
    "frozen_middle": [(3.0, 0.01, False), (1.0, 0.0, True), (0.1, 0.3, False)],
    "frozen_last": [(0.1, 0.3, False), (3.0, 0.0, False), (1.0, 0.01, True)],
}
# name -> (tile ids of the whole arena, first updated tile, one past the last updated tile, gradient scale)
ARENAS = {
    "one_tile": (lambda: [1], 0, 1, 1.0),
    "five_tiles": (lambda: [0, 1, 1, 1, 2], 0, 5, 1.0),                                  # three groups changing at tile 1 and at tile 4
    # 2048 blocks x 16 tiles fill the first trip; 3 more tiles (one of each group) make block 0's first 48 threads take a second trip
    "second_trip": (lambda: [t % 3 for t in range(GROUP_GRID_CAP * BLOCK_SPAN // TILE + 3)], 0, GROUP_GRID_CAP * BLOCK_SPAN // TILE + 3, 1.0),
    "shard": (lambda: [0, 0, 1, 1, 2, 2, 0, 1, 2], 3, 8, 0.5),                           # a ZeRO-1 style sub-range that starts at tile 3
}
GROUP_ADAMW_CASES = [(a, t) for a in ("one_tile", "five_tiles", "shard") for t in TABLES] + [("second_trip", "frozen_middle")]


def own(t, dev):
    """A fresh allocation on dev holding t (torch.empty: inside the guard bands of redzone.fixture_guard)."""
    return torch.empty(t.shape, dtype=t.dtype, device=dev).copy_(t)


def adamw64(p, g, m, v, step, lr, wd, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.AdamW's update restated in float64 (redzone_cases._adamw64 with the group's lr and weight decay)."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p * (1 - lr * wd) - lr / (1 - b1 ** step) * (m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps))
    return p, m, v


def f32(x):
    return float(np.float32(x))


def group_setup(dev, arena, table_name):
    ids, lo_t, hi_t, gs = ARENAS[arena]
    ids = torch.tensor(ids(), dtype=torch.uint8)
    rows = TABLES[table_name]
    table = torch.tensor([[a, b, 1.0 if c else 0.0] for a, b, c in rows], dtype=torch.float32)
    elem = ids.long().repeat_interleave(TILE)
    frozen = torch.tensor([r[2] for r in rows])[elem]
    return ids, lo_t * TILE, hi_t * TILE, gs, rows, table, elem, frozen


def check_group_adamw(dev, arena, table_name, lr=1e-2):
    """Three steps of ops.adamw_groups_ over tiles [lo, hi) of an arena against float64 per group; NaN gradients in every frozen tile."""
    ids, lo, hi, gs, rows, table, elem, frozen = group_setup(dev, arena, table_name)
    n = ids.numel() * TILE
    if arena == "second_trip":
        assert n // 4 > GROUP_GRID_CAP * 256 and n // 4 - GROUP_GRID_CAP * 256 == 3 * TILE // 4      # the second trip exists and is three tiles long
    p0, m0, v0 = R(n, seed=n), R(n, seed=1) * 0.1, (R(n, seed=2) * 0.1).abs()
    p, tiles, tab = own(p0, dev), own(ids, dev), own(table, dev)
    m, v = own(m0[lo:hi], dev), own(v0[lo:hi], dev)
    state = own(torch.tensor([0.0, lr]), dev)
    want = [kc.c64(t) for t in (p0, m0, v0)]
    live = ~frozen
    live[:lo] = False
    live[hi:] = False
    for step in (1, 2, 3):
        g0 = R(n, seed=10 + step)
        g0[frozen] = float("nan")                     # a frozen tile's gradient must not be read into anything
        g = own(g0, dev)
        ops.adamw_groups_(p[lo:hi], g[lo:hi], m, v, state, tiles[lo // TILE:], tab, grad_scale=gs)
        assert state.tolist() == [float(step), f32(lr)], state.tolist()
        g64 = kc.c64(g0) * f32(gs)
        for gi, (lr_mult, wd, fr) in enumerate(rows):
            sel = live & (elem == gi)
            if fr or not bool(sel.any()):
                continue
            new = adamw64(want[0][sel], g64[sel], want[1][sel], want[2][sel], step, f32(lr) * f32(lr_mult), f32(wd))
            for w, t in zip(want, new):
                w[sel] = t
    pc, mc_, vc = p.cpu(), torch.zeros(n), torch.zeros(n)
    mc_[lo:hi], vc[lo:hi] = m.cpu(), v.cpu()
    assert bool(live.any()) or arena == "one_tile"
    for got, ref, what in zip((pc, mc_, vc), want, ("p", "m", "v")):
        assert bool(torch.isfinite(got[lo:hi]).all()), "%s: a NaN gradient of a frozen tile was read" % what
        kc.close(got[live], ref[live], tol=1e-5, what="adamw_groups_ %s %s %s" % (arena, table_name, what))
    still = frozen.clone()
    still[:lo] = False
    still[hi:] = False
    for got, old, what in zip((pc, mc_, vc), (p0, m0, v0), ("p", "m", "v")):
        assert torch.equal(got[still], old[still]), "adamw_groups_: frozen %s changed" % what
    outside = torch.ones(n, dtype=torch.bool)
    outside[lo:hi] = False
    assert torch.equal(pc[outside], p0[outside]), "adamw_groups_ wrote outside its range"


def check_one_group_is_plain_adamw(dev, n=5 * TILE):
    """One default group (lr_mult 1, the plain weight decay): the per-element expression sequence is adamw_kernel<>'s - the same bits."""
    a = [own(t, dev) for t in (R(n), R(n, seed=1) * 0.1, (R(n, seed=2) * 0.1).abs(), torch.tensor([0.0, 1e-2]))]
    b = [t.clone() for t in a]
    tiles, tab = own(torch.zeros(n // TILE, dtype=torch.uint8), dev), own(torch.tensor([[1.0, 0.01, 0.0]]), dev)
    for step in range(3):
        g = own(R(n, seed=20 + step), dev)
        ops.adamw_groups_(a[0], g, a[1], a[2], a[3], tiles, tab, grad_scale=0.25)
        ops.adamw_(b[0], g, b[1], b[2], b[3], grad_scale=0.25)
    for x, y, what in zip(a, b, ("p", "m", "v", "state")):
        assert torch.equal(x, y), "one default group: %s differs from ops.adamw_" % what


def check_group_sumsq_clip(dev, ntiles=40, lo_t=8, hi_t=24, gs=0.5, lr=1e-2):
    """Norm over the non-frozen tiles only (2560 floats: three partials; NaN in every frozen tile), then two clipped steps over the strict sub-range
    of tiles [8, 24) against float64 with clip_grad_norm_'s coefficient; everything twice, bitwise."""
    rows = TABLES["frozen_middle"]
    ids = torch.tensor([t % 3 for t in range(ntiles)], dtype=torch.uint8)
    table = torch.tensor([[a, b, 1.0 if c else 0.0] for a, b, c in rows], dtype=torch.float32)
    n, lo, hi = ntiles * TILE, lo_t * TILE, hi_t * TILE
    elem = ids.long().repeat_interleave(TILE)
    frozen = torch.tensor([r[2] for r in rows])[elem]
    g0 = R(n, seed=3)
    g0[frozen] = float("nan")
    a0 = ops.float_atomic_launches()
    bound = acc.sumsq_bound(n)
    g64 = kc.c64(g0)[~frozen] * f32(gs)
    norm64 = float(g64.square().sum().sqrt())
    max_norm = 0.3 * norm64
    coef = min(1.0, f32(max_norm) / (norm64 + 1e-6))
    assert coef < 1.0
    runs = []
    for _ in range(2):
        g, tiles, tab = own(g0, dev), own(ids, dev), own(table, dev)
        parts = ops.grad_sumsq_groups(g, tiles, tab)
        assert parts.shape == (ops.grad_sumsq_parts(n),) == (3,) and bool(torch.isfinite(parts).all()), parts
        got, want = float(kc.c64(parts).sum()), float(kc.c64(g0)[~frozen].square().sum())
        print("  sumsq_groups rel err %.2e (bound %.2e)" % (abs(got - want) / want, bound))
        assert abs(got - want) <= bound * want, (got, want, bound)
        p0, m0, v0 = R(n, seed=4), R(n, seed=5) * 0.1, (R(n, seed=6) * 0.1).abs()
        p, m, v = own(p0, dev), own(m0[lo:hi], dev), own(v0[lo:hi], dev)
        state, norm_out = own(torch.tensor([0.0, lr]), dev), own(torch.tensor([-1.0]), dev)
        ref = [kc.c64(t)[lo:hi] for t in (p0, m0, v0)]
        e, fz = elem[lo:hi], frozen[lo:hi]
        for step in (1, 2):
            ops.grad_sumsq_groups(g, tiles, tab, parts)
            ops.adamw_groups_(p[lo:hi], g[lo:hi], m, v, state, tiles[lo_t:], tab, grad_scale=gs, partials=parts, n_norm=n, max_norm=max_norm, norm_out=norm_out)
            gn = float(norm_out[0])
            assert abs(gn - norm64) <= bound * norm64, (gn, norm64)
            gc = kc.c64(g0)[lo:hi] * f32(gs) * coef
            for gi, (lr_mult, wd, fr) in enumerate(rows):
                sel = (e == gi) & ~fz
                if bool(sel.any()):
                    new = adamw64(ref[0][sel], gc[sel], ref[1][sel], ref[2][sel], step, f32(lr) * f32(lr_mult), f32(wd))
                    for w, t in zip(ref, new):
                        w[sel] = t
        for got_t, ref_t, what in zip((p[lo:hi], m, v), ref, ("p", "m", "v")):
            kc.close(got_t.cpu()[~fz], ref_t[~fz], tol=1e-5, what="clipped adamw_groups_ " + what)
        assert torch.equal(p.cpu()[frozen], p0[frozen]) and torch.equal(m.cpu()[fz], m0[lo:hi][fz]) and torch.equal(v.cpu()[fz], v0[lo:hi][fz])
        runs.append([t.cpu().clone() for t in (parts, p, m, v, norm_out)])
    for x, y in zip(*runs):
        assert torch.equal(x, y), "two runs of the group norm + clipped update differ"
    assert ops.float_atomic_launches() == a0, "a group kernel counted as a float-atomic kernel form"


BN_FROZEN_SHAPES = kc.BN_VARIANT_CASES + [(2, 4, 5, 24)]
nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()


def bn_frozen_reference(dev, B, H, W, C, relu, with_res):
    """Inputs and the float64 autograd of F.batch_norm(x, rm, rv, g, b, False) (+ res) (relu)."""
    x = R(B, C, H, W, dev=dev) * 2 + 0.7
    g, b = R(C, seed=1, dev=dev) * 0.3 + 1, R(C, seed=2, dev=dev)
    res = R(B, C, H, W, seed=4, dev=dev) if with_res else None
    rm, rv = R(C, seed=5, dev=dev) * 0.5 + 0.6, R(C, seed=6, dev=dev).abs() + 0.5
    dy = R(B, C, H, W, seed=3, dev=dev)
    x64, g64, b64 = (kc.c64(t).requires_grad_(True) for t in (x, g, b))
    res64 = kc.c64(res).requires_grad_(True) if with_res else None
    y = F.batch_norm(x64, kc.c64(rm), kc.c64(rv), g64, b64, False, 0.1, 1e-5)
    if with_res:
        y = y + res64
    if relu:
        y = torch.relu(y)
    grads = torch.autograd.grad(y, [x64, g64, b64] + ([res64] if with_res else []), kc.c64(dy))
    return x, g, b, res, rm, rv, dy, y.detach(), grads


def check_bn_frozen(dev, B, H, W, C, relu, with_res, affine):
    x, g, b, res, rm, rv, dy, y, grads = bn_frozen_reference(dev, B, H, W, C, relu, with_res)
    rm0, rv0 = rm.clone(), rv.clone()
    yh, sm, si = ops.bn_fwd(nhwc(x), g, b, rm, rv, nhwc(res) if with_res else None, relu, False)
    kc.close(yh.permute(0, 3, 1, 2), y, what="bn eval fwd")
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0), "eval mode moved the running statistics"
    assert torch.equal(sm, rm), "bn_fwd(training=False): save_mean is not running_mean"
    kc.close(si, (kc.c64(rv) + 1e-5).rsqrt(), tol=1e-6, what="bn_fwd(training=False) save_invstd")
    dg0, db0 = R(C, seed=7, dev=dev), R(C, seed=8, dev=dev)                  # accumulated INTO: not zero
    dg, db = (dg0.clone(), db0.clone()) if affine else (None, None)
    dx, dres = ops.bn_bwd(nhwc(dy), yh if relu else None, nhwc(x), g, sm, si, dg, db, want_dres=with_res, frozen=True)
    kc.close(dx.permute(0, 3, 1, 2), grads[0], what="frozen bn dx")
    if affine:
        kc.close(dg, kc.c64(dg0) + grads[1], what="frozen bn dgamma")
        kc.close(db, kc.c64(db0) + grads[2], what="frozen bn dbeta")
    if with_res:
        kc.close(dres.permute(0, 3, 1, 2), grads[3], what="frozen bn dres")


def check_eval_bn_module_backward(dev, B=3, H=6, W=10, C=48):
    """An eval-mode BatchNorm2d through the block Functions' own helpers (functions._bn / _bn_bwd), as every trunk block runs it."""
    from transfuser_amd import functions as F_
    x, g, b, res, rm, rv, dy, y, grads = bn_frozen_reference(dev, B, H, W, C, True, True)
    bn = torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(g); bn.bias.copy_(b); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.eval()
    bn.weight.grad, bn.bias.grad = torch.zeros_like(bn.weight), torch.zeros_like(bn.bias)
    with F_.inplace_param_grads():
        z, st = F_._bn(nhwc(x), bn, res=nhwc(res), relu=True)
        dx, dres = F_._bn_bwd(nhwc(dy), z, nhwc(x), bn, st, want_dres=True)
    kc.close(z.permute(0, 3, 1, 2), y, what="eval bn module fwd")
    kc.close(dx.permute(0, 3, 1, 2), grads[0], what="eval bn module dx")
    kc.close(bn.weight.grad, grads[1], what="eval bn module dgamma")
    kc.close(bn.bias.grad, grads[2], what="eval bn module dbeta")
    kc.close(dres.permute(0, 3, 1, 2), grads[3], what="eval bn module dres")


def check_kernel_refusals(dev):
    L = ops.L()
    vp, i64, cf = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    t = [own(torch.zeros(2 * TILE + 4), dev) for _ in range(4)]
    tiles, tab, st = own(torch.zeros(4, dtype=torch.uint8), dev), own(torch.tensor([[1.0, 0.01, 0.0]]), dev), own(torch.tensor([0.0, 1e-3]), dev)
    parts = own(torch.zeros(1), dev)
    P = lambda x: vp(x.data_ptr())

    def adamw(p, n, ngroups=1, table=tab):
        return L.tf_adamw_groups_f32(P(p), P(t[1]), P(t[2]), P(t[3]), i64(n), P(st), cf(0.9), cf(0.999), cf(1e-8), cf(1.0), P(tiles), P(table) if table is not None else vp(0),
                                     ngroups, vp(0), 0, i64(0), cf(0.0), vp(0), vp(0))

    def sumsq(g, n, ngroups=1):
        return L.tf_grad_sumsq_groups_f32(P(g), i64(n), P(tiles), P(tab), ngroups, P(parts), vp(0))

    def refused(rc, text):
        assert rc != 0, "accepted: " + text
        msg = L.tf_last_error().decode()
        assert text in msg, (text, msg)
    refused(adamw(t[0][1:], TILE), "16-byte aligned")
    refused(adamw(t[0], TILE + 4), "whole 64-float tiles")
    refused(adamw(t[0], TILE, ngroups=0), "1..255 groups")
    refused(adamw(t[0], TILE, ngroups=256), "1..255 groups")
    refused(adamw(t[0], TILE, table=None), "must not be NULL")
    refused(sumsq(t[0][1:], TILE), "16-byte aligned")
    refused(sumsq(t[0], TILE + 4), "whole 64-float tiles")
    refused(sumsq(t[0], TILE, ngroups=0), "1..255 groups")
    assert st.tolist() == [0.0, f32(1e-3)] and not bool(t[0].any()), "a refused call launched something"
    C, rows = 8, 4
    x, c = own(torch.zeros(rows * C), dev), own(torch.ones(C), dev)
    ws = ops.workspace(x.device)
    bn = lambda rows_, dgamma, dbeta: L.tf_bn_bwd_frozen_f32(P(x), vp(0), P(x), rows_, C, P(c), P(c), P(c), P(t[0]), vp(0), dgamma, dbeta, P(ws), vp(0))
    refused(bn(0, vp(0), vp(0)), "bad arguments")
    refused(bn(rows, P(c), vp(0)), "together")
    refused(bn(rows, vp(0), P(c)), "together")


# ---------------------------------------------------------------- Engine level
PG = {"lr_mult": [{"match": "_model.lidar_encoder", "lr_mult": 0.1}], "no_decay_1d": [{"match_1d": True, "weight_decay": 0.0}]}
BOTH = PG["lr_mult"] + PG["no_decay_1d"]


def under(name, prefix=PREFIX):
    return name.startswith(prefix)


def check_frozen_stay(dev, by_hand):
    """Two steps with the image encoder frozen: its parameters and BatchNorm buffers keep their bits and have no optimizer state; every other
    parameter moves."""
    from transfuser_amd.train import Engine
    if by_hand:
        cfg = mc.tiny_config(n_layer=1, lidar_res=64)
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        prod.train()
        for n, p in prod.named_parameters():
            if under(n):
                p.requires_grad_(False)
        eng = Engine(prod, cfg, lr=1e-3, autotune=False)
    else:
        cfg, prod, _, eng = acc.make_engine(dev, lr=1e-3, freeze=[PREFIX])
    before = {n: p.detach().clone() for n, p in prod.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in prod.named_buffers() if under(n)}
    assert any(under(n) for n in before) and any("running_mean" in n for n in bufs)
    b = acc.batches(dev, 1)[0]
    for _ in range(2):
        eng.train_step(b)
    assert float(eng.optimizer.state[0]) == 2.0
    off = {n: o for n, _, o in eng.arena.layout}
    for n, p in prod.named_parameters():
        if under(n):
            assert not p.requires_grad and torch.equal(p.detach(), before[n]), "frozen parameter %s moved" % n
            assert off[n] >= eng.arena.active_numel, "frozen parameter %s lies inside the optimizer's range" % n      # no moments exist for it
        else:
            assert not torch.equal(p.detach(), before[n]), "trainable parameter %s did not move" % n
    assert eng.optimizer.exp_avg.numel() == eng.arena.active_numel < eng.arena.numel
    for n, t in prod.named_buffers():
        if under(n):
            assert torch.equal(t, bufs[n]), "buffer %s of a frozen BatchNorm moved" % n


def check_vs_oracle(dev, arch, case):
    """Frozen image encoder (its BatchNorms in eval()) + one param group, two steps against torch.optim.AdamW on the CPU oracle."""
    from oracle import model_cpu
    from transfuser_amd.train import Engine
    cfg = mc.tiny_config(n_layer=1)
    prod, ref = mc.build_pair(cfg, arch, dev)
    prod.train(); ref.train()
    lr = 1e-3
    eng = Engine(prod, cfg, lr=lr, freeze=[PREFIX], param_groups=PG[case], autotune=False)
    ref_bn = [m for n, m in ref.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and under(n)]
    assert len(ref_bn) == len(eng._frozen_bn) > 0 and not any(m.training for m in eng._frozen_bn)
    for m in ref_bn:
        m.eval()
    picked, rest = [], []
    for n, p in ref.named_parameters():
        if under(n):
            p.requires_grad_(False)
        elif (p.dim() <= 1) if case == "no_decay_1d" else n.startswith("_model.lidar_encoder"):
            picked.append(n)
        else:
            rest.append(n)
    assert picked and rest
    rp = dict(ref.named_parameters())
    extra = dict(lr=lr * 0.1) if case == "lr_mult" else dict(weight_decay=0.0)
    opt = torch.optim.AdamW([dict(params=[rp[n] for n in rest]), dict(params=[rp[n] for n in picked], **extra)], lr=lr)
    assert sorted(n for n, g in eng.optimizer.state_dict()["param_group"].items() if g == 1) == sorted(picked)
    init = {n: p.detach().clone() for n, p in ref.named_parameters()}
    batch = mc.small_batch(2, 32, 64, 64, 40)
    bd = {k: v.to(dev) for k, v in batch.items()}
    for it in range(2):
        tot_p, _ = eng.train_step(bd)
        tot_r, _ = model_cpu.train_step(ref, opt, batch, cfg)      # switches no modes itself
        assert not any(m.training for m in ref_bn)
        print("  %s %s step %d: loss %.6f vs %.6f" % (arch, case, it, float(tot_p), float(tot_r)))
        assert abs(float(tot_p) - float(tot_r)) <= 1e-3 * max(1.0, abs(float(tot_r))), (it, float(tot_p), float(tot_r))
    worst = {}
    for n, p in prod.named_parameters():
        got = p.detach().cpu()
        if under(n):
            assert torch.equal(got, init[n]) and torch.equal(rp[n].detach(), init[n]), "frozen %s moved" % n
            continue
        mult = 0.1 if (case == "lr_mult" and n in picked) else 1.0
        d = (got - rp[n].detach()).abs().max().item()
        worst[mult] = max(worst.get(mult, (0.0, "")), (d, n))
        assert d < 4.4e-3 * mult, (n, d, mult)
    print("  worst parameter difference per lr_mult: %s" % worst)
    rb = dict(ref.named_buffers())
    for n, t in prod.named_buffers():
        if under(n) and "running" in n:
            assert torch.equal(t.cpu(), rb[n]), n


def check_clip_norm_frozen(dev, groups):
    """optimizer.grad_norm = the float64 norm of the NON-frozen gradients the step left in the arena (masked by layout)."""
    cfg, prod, _, eng = acc.make_engine(dev, lr=1e-3, freeze=[PREFIX], max_grad_norm=1e-2, param_groups=BOTH if groups else None)
    eng.train_step(acc.batches(dev, 1)[0])
    g = kc.c64(eng.arena.grads) * eng.grad_scale()
    n = eng.arena.active_numel
    sq_live = sum(float(g[o:o + p.numel()].square().sum()) for name, p, o in eng.arena.layout if not under(name))
    sq_frozen = sum(float(g[o:o + p.numel()].square().sum()) for name, p, o in eng.arena.layout if under(name))
    assert all((o >= n) == under(name) for name, p, o in eng.arena.layout)
    want, got, bound = sq_live ** 0.5, float(eng.optimizer.grad_norm), acc.sumsq_bound(n)
    print("  grad_norm %.8g, float64 over the trainable gradients %.8g (with the frozen ones %.8g)" % (got, want, (sq_live + sq_frozen) ** 0.5))
    assert want > 1e-2, "the clip must be active"
    assert (sq_live + sq_frozen) ** 0.5 > (1 + 4 * bound) * want, "the frozen trunk has no gradient to leave out: the check would be vacuous"
    assert abs(got - want) <= bound * want, (got, want, bound)


def ft_run(dev, use_graph, steps=3, max_grad_norm=None, **kw):
    cfg, prod, _, eng = acc.make_engine(dev, freeze=[PREFIX], param_groups=BOTH, max_grad_norm=max_grad_norm, use_graph=use_graph, deterministic=True, **kw)
    b = acc.batches(dev, 1)[0]
    losses, grads = [], []
    for _ in range(steps):
        tot, det = eng.train_step(b)
        losses.append([float(tot)] + [float(det[k]) for k in cfg.detailed_losses])
        grads.append((eng.arena.grads.detach().clone(), None if eng.optimizer.grad_norm is None else float(eng.optimizer.grad_norm)))
    return eng, prod, torch.tensor(losses, dtype=torch.float64), grads, eng.arena.params.detach().clone(), b


def check_graph_matches_eager(dev):
    """freeze + groups + an active clip, captured vs eager, under accum_clip_cases.check_graph_matches_eager's set-up (one pinned tiling,
    deterministic mode) and bounds; then set_group between two replays."""
    prev = ops.is_deterministic()
    ops.force_plan(64, 64, 16, 1)
    try:
        probe = ft_run(dev, False, steps=1, max_grad_norm=1e30)
        m = 0.5 * probe[3][0][1]
        assert m > 0
        (ee, _, le, ge, _, _), (eg, prod, lg, gg, _, b) = [ft_run(dev, g, max_grad_norm=m) for g in (False, True)]
        assert ge[0][1] > m, "the clip must be active"
        for i, ((ga, na), (gb, nb)) in enumerate(zip(ge, gg)):
            acc.tensors_agree(ee, gb, ga, "step %d gradients, graph vs eager" % i)
            assert abs(na - nb) <= 1e-5 * na, (i, na, nb)
        rel = ((le - lg).abs() / le.abs().clamp_min(1e-3)).max(dim=1).values
        print("  graph vs eager: max relative loss difference per step %s" % ["%.1e" % v for v in rel.tolist()])
        assert rel[0].item() <= 1e-5 and rel.max().item() <= 2e-4, rel
        # group 1 (the LiDAR encoder's matrices) stands still after set_group(1, lr_mult=0, weight_decay=0); no recapture
        graphs = eg._graphs
        gid = eg.optimizer.state_dict()["param_group"]
        eg.optimizer.set_group(1, lr_mult=0.0, weight_decay=0.0)
        before = {n: p.detach().clone() for n, p in prod.named_parameters()}
        eg.train_step(b)
        torch.cuda.synchronize()
        assert eg._graphs is graphs and float(eg.optimizer.state[0]) == 4.0
        assert sum(1 for n in gid if gid[n] == 1) > 0
        for n, p in prod.named_parameters():
            if under(n) or gid[n] == 1:
                assert torch.equal(p.detach(), before[n]), "%s moved with lr_mult = weight_decay = 0" % n
            elif gid[n] == 0 or bool(p.grad.any()):      # group 2 has no weight decay: a dead head's bias (zero gradient) rightly stands still
                assert not torch.equal(p.detach(), before[n]), "%s did not move" % n
    finally:
        ops.force_plan(0)
        ops.set_deterministic(prev)


def check_bitwise_runs(dev):
    prev = ops.is_deterministic()
    try:
        a = ft_run(dev, False, max_grad_norm=0.05)
        a0 = ops.float_atomic_launches()
        b = ft_run(dev, False, max_grad_norm=0.05)
        assert ops.float_atomic_launches() == a0, "a float-atomic kernel form ran in deterministic mode"
    finally:
        ops.set_deterministic(prev)
    assert a[3][0][1] > 0.05, "the clip must be active"
    assert torch.equal(a[2], b[2]), "losses differ"
    assert [g[1] for g in a[3]] == [g[1] for g in b[3]], "grad_norm differs"
    assert torch.equal(a[4], b[4]), "parameters differ after 3 deterministic steps: %d elements" % int((a[4] != b[4]).sum())


def check_defaults_unchanged(dev):
    """The new arguments at their defaults are the constructor without them: layout, ranges and, after two deterministic steps, the bits."""
    prev = ops.is_deterministic()
    try:
        runs = []
        for kw in ({}, dict(param_groups=None, freeze=None), dict(param_groups=[], freeze=[], freeze_bn=False)):
            cfg, prod, _, eng = acc.make_engine(dev, dropout=0.1, lr=1e-3, deterministic=True, cuts=(3,), **kw)
            b = acc.batches(dev, 1)[0]
            for _ in range(2 if "freeze_bn" not in kw else 0):      # the third spelling is compared by layout only
                eng.train_step(b)
            assert eng.arena.tile_group is None and eng.optimizer.group_table is None and eng.arena.frozen == [] and eng._frozen_bn == []
            assert all(m.training for m in prod.modules())
            runs.append(([(n, o) for n, _, o in eng.arena.layout], eng.arena.segment_ranges, eng.arena.active_numel, eng.arena.numel, eng.arena.params.detach().clone()))
    finally:
        ops.set_deterministic(prev)
    for r in runs[1:]:
        assert r[:4] == runs[0][:4], "layout / segment_ranges / active_numel changed"
    assert torch.equal(runs[1][4], runs[0][4]) and not torch.equal(runs[2][4], runs[0][4])
    assert len(runs[0][1]) == 2 and runs[0][2] == runs[0][3]


def check_resume(dev):
    """Model + optimizer.state_dict() after step 2 into a fresh Engine with the same groups: step 3 has the uninterrupted run's bits.  A state
    written WITHOUT groups or freezing loads as well (moments by name; those of parameters frozen now are ignored)."""
    import io
    prev = ops.is_deterministic()
    kw = dict(freeze=[PREFIX], param_groups=BOTH, max_grad_norm=0.05, deterministic=True, lr=1e-3)
    try:
        cfg, prod, _, eng = acc.make_engine(dev, **kw)
        b = acc.batches(dev, 1)[0]
        for _ in range(2):
            eng.train_step(b)
        eng.optimizer.set_group(2, weight_decay=0.001)
        buf = io.BytesIO()
        torch.save(dict(model=prod.state_dict(), opt={k: (v.cpu() if torch.is_tensor(v) else v) for k, v in eng.optimizer.state_dict().items()}), buf)
        eng.train_step(b)
        want = {n: p.detach().clone() for n, p in prod.named_parameters()}
        buf.seek(0)
        saved = torch.load(buf, weights_only=False)
        assert [g["frozen"] for g in saved["opt"]["groups"]] == [False] * 3 and abs(saved["opt"]["groups"][2]["weight_decay"] - 0.001) < 1e-9
        assert set(saved["opt"]["param_group"].values()) == {0, 1, 2} and not any(under(n) for n in saved["opt"]["param_group"])
        cfg2, prod2, _, eng2 = acc.make_engine(dev, **kw)
        prod2.load_state_dict(saved["model"])
        eng2.optimizer.load_state_dict(saved["opt"])
        assert torch.equal(eng2.optimizer.group_table, eng.optimizer.group_table)
        eng2.train_step(b)
        assert float(eng2.optimizer.state[0]) == 3.0
        for n, p in prod2.named_parameters():
            assert torch.equal(p.detach(), want[n]), "resumed step 3 differs in %s" % n
        # a plain run's state (no groups, nothing frozen) into the fine-tuning Engine
        cfg3, prod3, _, eng3 = acc.make_engine(dev, lr=1e-3, deterministic=True)
        eng3.train_step(b)
        plain = eng3.optimizer.state_dict()
        assert "groups" not in plain and any(under(t[0]) for t in plain["layout"])
        cfg4, prod4, _, eng4 = acc.make_engine(dev, **kw)
        eng4.optimizer.load_state_dict(plain)
        by_name = {t[0]: t for t in plain["layout"]}
        for name, off, cnt in eng4.optimizer._layout():
            src = plain["exp_avg"][by_name[name][1]:by_name[name][1] + cnt]
            assert torch.equal(eng4.optimizer.exp_avg[off:off + cnt], src), name
        assert float(eng4.optimizer.state[0]) == 1.0
    finally:
        ops.set_deterministic(prev)


def check_refusals(dev):
    from transfuser_amd.train import Engine, FlatAdamW, ParamArena
    cfg = mc.tiny_config(n_layer=1)
    for kw in (dict(freeze=["_model.no_such_module"]), dict(param_groups=[{"match": "nothing.here", "lr_mult": 0.1}]),
               dict(param_groups=[{"match": ["_model.lidar_encoder", "nope"], "lr_mult": 0.1}]), dict(param_groups=[{"lr_mult": 0.1}]),
               dict(param_groups=[{"match": PREFIX, "lr": 0.1}])):
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        with pytest.raises(ValueError):
            Engine(prod, cfg, autotune=False, **kw)
    prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
    try:      # groups under the fp16 dynamic loss scale are refused; freezing alone is not
        with pytest.raises(NotImplementedError):
            Engine(prod, cfg, autotune=False, precision="fp16", param_groups=PG["lr_mult"])
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        eng = Engine(prod, cfg, autotune=False, precision="fp16", freeze=[PREFIX])
        assert eng.ls_state is not None and eng.arena.active_numel < eng.arena.numel
    finally:
        ops.set_precision("fp32")
    with pytest.raises(ValueError):
        FlatAdamW(eng.arena, groups=[{"lr_mult": 0.1}])            # an arena without tile ids
    with pytest.raises(ValueError):
        eng.optimizer.set_group(0, lr_mult=0.5)                    # an optimizer without groups


def check_bn1d_eval_refused(dev):
    """PointPillars: a BatchNorm1d of the point net in eval() under gradients raises instead of using the batch-statistics backward."""
    from transfuser_amd.point_pillar import PointPillarNet
    torch.manual_seed(0)
    net = PointPillarNet(9, [16], min_x=-4, max_x=4, min_y=-4, max_y=4, pixels_per_meter=2).to(dev)
    pts = (torch.rand(2, 50, 4) * 8 - 4).to(dev)
    num = torch.tensor([50, 30], dtype=torch.int32, device=dev)
    net.train()
    net(pts, num)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.eval()
    with pytest.raises(NotImplementedError):
        net(pts, num)
    with torch.no_grad():
        net(pts, num)


def check_trainer_keeps_frozen_bn(dev, tmp_path):
    """Trainer.train() calls model.train() every epoch: the frozen BatchNorms go back to eval() and their running buffers stay put over one
    epoch of a two-batch loader; validate() restores them as well."""
    import types
    from transfuser_amd.train import Trainer
    cfg, prod, _, eng = acc.make_engine(dev, lr=1e-3, freeze=[PREFIX])
    loader = [mc.small_batch(2, 32, 64, 64, 40, seed=s) for s in range(2)]
    args = types.SimpleNamespace(logdir=str(tmp_path))
    tr = Trainer(eng, loader, loader[:1], args, cfg, torch.device(dev), rank=0, world_size=1, parallel=False)
    bufs = {n: b.detach().clone() for n, b in prod.named_buffers() if under(n)}
    moving = {n: b.detach().clone() for n, b in prod.named_buffers() if not under(n) and "running_mean" in n}
    assert bufs and moving
    tr.train()
    assert float(eng.optimizer.state[0]) == 2.0
    frozen_bn = [m for n, m in prod.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and under(n)]
    assert frozen_bn and not any(m.training for m in frozen_bn) and prod.training
    for n, t in prod.named_buffers():
        if under(n):
            assert torch.equal(t, bufs[n]), n
        elif n in moving:
            assert not torch.equal(t, moving[n]), "%s: a trainable BatchNorm's statistics stood still" % n
    tr.validate()
    assert not any(m.training for m in frozen_bn) and prod.training
