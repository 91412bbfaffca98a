"""Weight EMA (csrc/ema.cpp, transfuser_amd/ema.py, train.Engine(ema_decay=...)): the kernels against float64 and the formula, the Engine's
average against a shadow advanced with the same launches, the swap, state, checkpoints and resume.  Every function takes the device: "cpu" runs
the host-emulated kernels (tests/test_ema_emu.py), "cuda" the MI355X (tests/test_ema_gpu.py)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import accum_clip_cases as acc
import kernel_cases as kc
import model_cases as mc
from transfuser_amd import ops

R = kc.R
TILE = 64
BLOCK_SPAN = 1024               # floats one block of the flat kernels covers per trip: 256 threads x one float4
GRID_CAP = 2048                 # their grid cap (csrc/ema.cpp kEmaGridCap)
APPLY_SIZES = [TILE, TILE * 33, GRID_CAP * BLOCK_SPAN + TILE]      # one tile; a block's last trip is partial; capped blocks take a second trip
TABLE_COUNTS = [1, 3, 255, 256, 257, 1512]
SPARE = 100                     # a seventh range beside the table's entries that no table names
PREFIX = "_model.image_encoder"
PG = [{"match": "_model.lidar_encoder", "lr_mult": 0.1}, {"match_1d": True, "weight_decay": 0.0}]


def own(t, dev):
    """A fresh allocation on dev holding t (torch.empty: inside the guard bands of redzone.fixture_guard)."""
    return torch.empty(t.shape, dtype=t.dtype, device=dev).copy_(t)


def f32(x):
    return float(np.float32(x))


def new_state(dev, decay):
    return own(torch.tensor([decay, 0.0, 0.0, 0.0], dtype=torch.float32), dev)


def ulp_bound(e0, p0):
    """2 ulp of max(|e|, |p|) per element (float64): the subtraction rounds once - at most 0.5 ulp of |p - e| <= 1 ulp of the maximum - and the
    fused multiply-add once more: 1.5, rounded up to 2."""
    big = torch.maximum(e0.abs(), p0.abs()).numpy().astype(np.float32)
    return 2.0 * torch.from_numpy(np.spacing(big).astype(np.float64))


def within(got, e0, p0, coef, what):
    want = kc.c64(e0) + coef * (kc.c64(p0) - kc.c64(e0))
    err, bound = (kc.c64(got) - want).abs(), ulp_bound(e0, p0)
    worst = float((err / bound).max())
    print("  %s: worst error %.3f of the 2-ulp bound" % (what, worst))
    assert bool((err <= bound).all()), "%s: %d elements beyond 2 ulp of max(|e|, |p|), worst %.3f x the bound" % (what, int((err > bound).sum()), worst)


# ---------------------------------------------------------------- kernel level
def check_apply(dev, n):
    """ema_apply_ against float64; p and the state are not written (the redzone guard of the calling file shows nothing beside e is)."""
    if n == APPLY_SIZES[2]:
        assert n // 4 > GRID_CAP * 256 and n // 4 - GRID_CAP * 256 == TILE // 4      # the second grid-stride trip exists and is one tile long
    e0, p0 = R(n, seed=n) * 3.0, R(n, seed=n + 1)
    e0[:8] = torch.tensor([0.0, 1e-30, -1e30, 5.0, 5.0, -0.0, 1.0, 65504.0])
    p0[:8] = torch.tensor([0.0, 1e30, 1e-30, 5.0, -5.0, 1.0, 1.0 + 2.0 ** -23, -65504.0])
    e, p, st = own(e0, dev), own(p0, dev), new_state(dev, 0.9)
    ops.ema_tick_(st)
    s = st.tolist()
    coef = f32(1.0 - f32(0.9))
    assert s == [f32(0.9), 1.0, 0.0, coef], s
    ops.ema_apply_(e, p, st)
    assert st.tolist() == s and torch.equal(p.cpu(), p0), "ema_apply_ wrote p or the state"
    within(e.cpu(), e0, p0, coef, "ema_apply_ n = %d" % n)
    assert not torch.equal(e.cpu(), e0)


def table_setup(dev, seed=0):
    """Entries of TABLE_COUNTS floats at odd (4-byte aligned, never 8- or 16-byte aligned) offsets of one averaged and one live buffer, gaps
    between; a seventh range of SPARE floats is laid out like them but belongs to no table (it lies outside ``inside``)."""
    offs, off = [], 1
    for c in TABLE_COUNTS + [SPARE]:
        offs.append(off)
        off += c + 6
        off += 1 - off % 2      # odd again
    total = off + 5
    e0, p0 = R(total, seed=seed + 50) * 2.0, R(total, seed=seed + 51)
    e, p = own(e0, dev), own(p0, dev)
    assert e.data_ptr() % 16 == 0 and all(o % 2 == 1 for o in offs)
    pairs = [(e[o:o + c], p[o:o + c]) for o, c in zip(offs, TABLE_COUNTS)]
    inside = torch.zeros(total, dtype=torch.bool)
    for o, c in zip(offs, TABLE_COUNTS):
        inside[o:o + c] = True
    return e0, p0, e, p, pairs, inside


def check_apply_multi(dev):
    e0, p0, e, p, pairs, inside = table_setup(dev)
    table = ops.ema_table(pairs)      # all six counts; the spare range is in no table
    assert table[1] == len(TABLE_COUNTS) and table[2] == sum(TABLE_COUNTS) and int((~inside).sum()) > SPARE
    st = new_state(dev, 0.75)
    ops.ema_tick_(st)
    ops.ema_apply_multi_(table, st)
    got = e.cpu()
    assert torch.equal(p.cpu(), p0) and st.tolist() == [0.75, 1.0, 0.0, 0.25]
    assert torch.equal(got[~inside], e0[~inside]), "ema_apply_multi_ wrote outside its entries (gaps / the range left out of the table)"
    within(got[inside], e0[inside], p0[inside], 0.25, "ema_apply_multi_")
    assert not bool((got[inside] == e0[inside]).all())


def expected_coefs(decay, warmup, updates):
    out = []
    for n in range(updates):
        d = f32(decay)
        if warmup:
            d = min(d, f32((1.0 + n) / (10.0 + n)))
        out.append(f32(1.0 - d))
    return out


def check_tick(dev, decay, warmup):
    """The coefficients of the first 12 updates against the formula in Python floats cast to fp32 (1 + n and 10 + n are exact, an fp32 quotient
    is the rounded float64 quotient, 1 - d is exact in float64)."""
    st = new_state(dev, decay)
    want = expected_coefs(decay, warmup, 12)
    for n, c in enumerate(want):
        ops.ema_tick_(st, None, 1, warmup)
        assert st.tolist() == [f32(decay), float(n + 1), 0.0, c], (n, st.tolist(), c)
    if warmup and decay == 0.5:
        assert want[0] == f32(0.9) and want[7] > 0.5 and want[8] == 0.5 and want[11] == 0.5      # both sides of the min


def check_tick_every(dev):
    """every = 3 fires at optimizer steps 3, 6, ...; a repeated tick at the same optimizer step leaves coef = 0 and the apply changes nothing."""
    st, opt = new_state(dev, 0.9), own(torch.tensor([0.0, 1e-3]), dev)
    e0, p0 = R(TILE * 3, seed=3), R(TILE * 3, seed=4)
    e, p = own(e0, dev), own(p0, dev)
    coef, updates = f32(1.0 - f32(0.9)), 0
    for step in range(1, 8):
        opt[0] = float(step)
        ops.ema_tick_(st, opt, 3, False)
        fired = step % 3 == 0
        updates += int(fired)
        assert st.tolist() == [f32(0.9), float(updates), float(step - step % 3), coef if fired else 0.0], (step, st.tolist())
        before = e.clone()
        ops.ema_apply_(e, p, st)
        assert torch.equal(e, before) != fired, step
    opt[0] = 6.0
    before = e.clone()
    ops.ema_tick_(st, opt, 3, False)      # optimizer step 6 again (it was the last one that updated): nothing moves
    ops.ema_apply_(e, p, st)
    assert st.tolist() == [f32(0.9), 2.0, 6.0, 0.0] and torch.equal(e, before)
    assert opt.tolist() == [6.0, f32(1e-3)]


def check_fp16_skip(dev, n=TILE * 4):
    """An fp16 step skipped for an Inf gradient is not counted by the optimizer, so the average skips it too - without reading ls_state."""
    p0 = R(n, seed=1)
    p, m, v = own(p0, dev), own(torch.zeros(n), dev), own(torch.zeros(n), dev)
    opt, ls = own(torch.tensor([0.0, 1e-2]), dev), own(torch.tensor([1024.0, 0.0, 0.0, 2000.0]), dev)
    e, st = own(p0, dev), new_state(dev, 0.5)

    def step(g):
        ops.adamw_dynscale_(p, g, m, v, opt, ls, g)
        ops.ema_tick_(st, opt, 1, False)
        ops.ema_apply_(e, p, st)
    step(own(R(n, seed=2) * 1024.0, dev))
    assert opt.tolist()[0] == 1.0 and st.tolist()[1:] == [1.0, 1.0, 0.5] and ls.tolist()[0] == 1024.0
    e1, p1 = e.clone(), p.clone()
    assert not torch.equal(e1.cpu(), p0)
    g = R(n, seed=3)
    g[17] = float("inf")
    step(own(g, dev))
    assert opt.tolist()[0] == 1.0 and ls.tolist()[0] == 512.0, "the overflowed step must be skipped and the scale halved"
    assert st.tolist() == [0.5, 1.0, 1.0, 0.0], st.tolist()
    assert torch.equal(e, e1) and torch.equal(p, p1)
    step(own(R(n, seed=4) * 512.0, dev))
    assert opt.tolist()[0] == 2.0 and st.tolist() == [0.5, 2.0, 2.0, 0.5] and not torch.equal(e, e1)


def check_swap(dev):
    n = TILE * 33
    a0, b0 = R(n, seed=7), R(n, seed=8)
    a0[5] = float("nan")      # bits travel, not values
    a, b = own(a0, dev), own(b0, dev)
    bits = lambda t: t.cpu().view(torch.int32)
    ops.swap_(a, b)
    assert torch.equal(bits(a), bits(b0)) and torch.equal(bits(b), bits(a0))
    ops.swap_(a, b)
    assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(b), bits(b0))
    e0, p0, e, p, pairs, inside = table_setup(dev, seed=9)
    table = ops.ema_table(pairs)
    ops.swap_multi_(table)
    ge, gp = e.cpu(), p.cpu()
    assert torch.equal(ge[inside], p0[inside]) and torch.equal(gp[inside], e0[inside]) and torch.equal(ge[~inside], e0[~inside]) and torch.equal(gp[~inside], p0[~inside])
    ops.swap_multi_(table)
    assert torch.equal(e.cpu(), e0) and torch.equal(p.cpu(), p0)
    # overlap: the flat entry refuses on the host; a table's ranges live on the device, ops.ema_table refuses to build one that overlaps
    L = ops.L()
    rc = L.tf_swap_f32(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(a.data_ptr() + 16), ctypes.c_int64(TILE), ctypes.c_void_p(0))
    assert rc != 0 and "overlap" in L.tf_last_error().decode()
    rc = L.tf_swap_f32(ctypes.c_void_p(a.data_ptr() + 16), ctypes.c_void_p(a.data_ptr()), ctypes.c_int64(TILE), ctypes.c_void_p(0))
    assert rc != 0 and "overlap" in L.tf_last_error().decode()
    assert torch.equal(bits(a), bits(a0))
    with pytest.raises(ValueError, match="overlap"):
        ops.ema_table([(e[1:4], e[3:6])])
    with pytest.raises(ValueError, match="overlap"):
        ops.ema_table([(e[1:4], p[1:4]), (e[9:12], p[3:6])])
    with pytest.raises(ValueError):
        ops.ema_table([])


def check_kernel_refusals(dev):
    L = ops.L()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    e0, p0 = R(2 * TILE, seed=11), R(2 * TILE, seed=12)
    e, p, st = own(e0, dev), own(p0, dev), new_state(dev, 0.9)
    ops.ema_tick_(st)
    s0 = st.tolist()
    table = ops.ema_table([(e[1:9], p[1:9])])
    P = lambda x, off=0: vp(x.data_ptr() + off)

    def refused(rc, text):
        assert rc != 0, "accepted: " + text
        msg = L.tf_last_error().decode()
        assert text in msg, (text, msg)
    refused(L.tf_ema_tick_f32(vp(0), vp(0), 1, 0, vp(0)), "ema_state must not be NULL")
    refused(L.tf_ema_tick_f32(P(st), vp(0), 0, 0, vp(0)), "every must be >= 1")
    refused(L.tf_ema_apply_f32(vp(0), P(p), i64(TILE), P(st), vp(0)), "bad arguments")
    refused(L.tf_ema_apply_f32(P(e), vp(0), i64(TILE), P(st), vp(0)), "bad arguments")
    refused(L.tf_ema_apply_f32(P(e), P(p), i64(TILE), vp(0), vp(0)), "bad arguments")
    refused(L.tf_ema_apply_f32(P(e), P(p), i64(TILE + 2), P(st), vp(0)), "whole float4 lanes")
    refused(L.tf_ema_apply_f32(P(e, 4), P(p), i64(TILE), P(st), vp(0)), "16-byte aligned")
    refused(L.tf_ema_apply_f32(P(e), P(p, 8), i64(TILE), P(st), vp(0)), "16-byte aligned")
    refused(L.tf_ema_apply_f32(P(e), P(e, 16), i64(TILE), P(st), vp(0)), "overlap")
    refused(L.tf_ema_apply_f32(P(e, 16), P(e), i64(TILE), P(st), vp(0)), "overlap")
    refused(L.tf_ema_apply_multi_f32(vp(0), 1, P(st), vp(0)), "bad arguments")
    refused(L.tf_ema_apply_multi_f32(P(table[0]), 1, vp(0), vp(0)), "bad arguments")
    refused(L.tf_ema_apply_multi_f32(P(table[0]), 0, P(st), vp(0)), "nentries must be >= 1")
    refused(L.tf_swap_f32(vp(0), P(p), i64(TILE), vp(0)), "bad arguments")
    refused(L.tf_swap_f32(P(e), P(p), i64(TILE + 1), vp(0)), "whole float4 lanes")
    refused(L.tf_swap_f32(P(e, 4), P(p), i64(TILE), vp(0)), "16-byte aligned")
    refused(L.tf_swap_f32(P(e), P(e, 16), i64(TILE), vp(0)), "overlap")
    refused(L.tf_swap_multi_f32(vp(0), 1, vp(0)), "bad arguments")
    refused(L.tf_swap_multi_f32(P(table[0]), 0, vp(0)), "nentries must be >= 1")
    assert st.tolist() == s0 and torch.equal(e.cpu(), e0) and torch.equal(p.cpu(), p0), "a refused call launched something"


def check_deterministic_counter(dev):
    """Every EMA launch is legal under the deterministic mode and none of them is a float-atomic form."""
    e0, p0, e, p, pairs, inside = table_setup(dev, seed=20)
    a, b, st = own(R(TILE * 2, seed=21), dev), own(R(TILE * 2, seed=22), dev), new_state(dev, 0.9)
    table = ops.ema_table(pairs)
    with ops.deterministic():
        n0 = ops.float_atomic_launches()
        ops.ema_tick_(st)
        ops.ema_apply_(a, b, st)
        ops.ema_apply_multi_(table, st)
        ops.swap_(a, b)
        ops.swap_multi_(table)
        assert ops.float_atomic_launches() == n0
    assert st.tolist()[1] == 1.0


# ---------------------------------------------------------------- Engine level
def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def engine(dev, arch="regnety_tiny", **kw):
    kw.setdefault("deterministic", True)
    kw.setdefault("lr", 1e-3)
    return acc.make_engine(dev, arch, **kw)


class Shadow:
    """A clone of an Engine's initial weights / float buffers with its own ema_state, advanced with the ops.ema_* calls on the Engine's live values."""

    def __init__(self, eng, dev, decay, every=1, warmup=False):
        self.eng, self.every, self.warmup = eng, every, warmup
        self.n = eng.arena.active_numel
        self.flat = own(eng.arena.params[:self.n].detach(), dev)
        self.live = [b for _, b in eng.model.named_buffers() if b.is_floating_point()]
        self.bufs = [own(b.detach(), dev) for b in self.live]
        self.table = ops.ema_table(zip(self.bufs, self.live))
        self.st = new_state(dev, decay)

    def step(self):
        ops.ema_tick_(self.st, self.eng.optimizer.state, self.every, self.warmup)
        ops.ema_apply_(self.flat, self.eng.arena.params[:self.n], self.st)
        ops.ema_apply_multi_(self.table, self.st)

    def assert_equal(self, ema, what):
        # {decay, num_updates, last_opt_step}: the shadow also ticks after a micro-batch that is not a window's last, which only clears ITS coef
        assert self.st.tolist()[:3] == ema.state.tolist()[:3], (what, self.st.tolist(), ema.state.tolist())
        assert torch.equal(self.flat, ema.flat), "%s: the averaged arena range differs from the shadow in %d elements" % (what, int((self.flat != ema.flat).sum()))
        assert len(self.bufs) == len(ema.buf_views) > 0
        for s, v, (name, _) in zip(self.bufs, ema.buf_views, ema.buffers):
            assert torch.equal(s.reshape(-1), v), "%s: averaged buffer %s differs from the shadow" % (what, name)


def check_never_feeds_back(dev):
    """4 deterministic fp32 steps with ema_decay=0.9: parameters, moments and losses are bitwise those of an Engine without an average."""
    runs = []
    prev = ops.is_deterministic()
    try:
        for kw in ({}, dict(ema_decay=0.9)):
            cfg, prod, _, eng = engine(dev, **kw)
            b = acc.batches(dev, 1)[0]
            losses = []
            for _ in range(4):
                tot, det = eng.train_step(b)
                losses.append([float(tot)] + [float(det[k]) for k in cfg.detailed_losses])
            sync(dev)
            runs.append((eng, losses, eng.arena.params.detach().clone(), eng.optimizer.exp_avg.clone(), eng.optimizer.exp_avg_sq.clone(),
                         [x.detach().clone() for x in prod.buffers()]))
    finally:
        ops.set_deterministic(prev)
    (off, lo, po, mo, vo, bo), (on, ln, pn, mn, vn, bn) = runs
    assert off.ema is None and on.ema is not None and on.ema.num_updates == 4 and on.ema.state.tolist()[2] == 4.0
    assert lo == ln, "losses differ"
    assert torch.equal(po, pn) and torch.equal(mo, mn) and torch.equal(vo, vn), "the average fed back into the parameters or the moments"
    assert all(torch.equal(x, y) for x, y in zip(bo, bn))
    n = on.arena.active_numel
    assert not torch.equal(on.ema.flat, pn[:n]) and bool(torch.isfinite(on.ema.flat).all())
    assert on.ema.flat.numel() == n and on.ema.flat.data_ptr() != on.arena.params.data_ptr()


TRAJECTORIES = {
    "plain": (dict(), dict(), 5),
    "warmup_every2": (dict(), dict(ema_every=2, ema_warmup=True), 2),
    "accumulate2": (dict(accumulate=2), dict(), 2),
    "freeze": (dict(freeze=[PREFIX]), dict(), 5),
    "param_groups": (dict(param_groups=PG), dict(), 5),
    "convnext_mini": (dict(arch="convnext_mini", deterministic=None), dict(), 5),      # its depthwise weight gradient has no fixed-order form; the shadow needs none
}


def check_trajectory(dev, case, use_graph=False, steps=5):
    """After 5 train_step calls engine.ema equals, bitwise, a shadow advanced after every call with the same launches on the same inputs."""
    ekw, mkw, updates = TRAJECTORIES[case]
    prev = ops.is_deterministic()
    try:
        cfg, prod, _, eng = engine(dev, ema_decay=0.9, use_graph=use_graph, **ekw, **mkw)
        sh = Shadow(eng, dev, 0.9, mkw.get("ema_every", 1), mkw.get("ema_warmup", False))
        sh.assert_equal(eng.ema, "%s at construction" % case)
        bs = acc.batches(dev, 2)
        for i in range(steps):
            eng.train_step(bs[i % 2])
            sh.step()
            sync(dev)
            sh.assert_equal(eng.ema, "%s after call %d" % (case, i + 1))
    finally:
        ops.set_deterministic(prev)
    assert eng.ema.num_updates == updates and eng.ema.state_dict()["num_updates"] == updates, (eng.ema.num_updates, updates)
    if case == "freeze":
        n = eng.arena.active_numel
        assert 0 < n < eng.arena.numel and eng.ema.flat.numel() == n
        sd, live = eng.ema.state_dict()["model"], prod.state_dict()
        frozen = [k for k in live if k.startswith(PREFIX) and live[k].is_floating_point() and "running" not in k]
        assert frozen and all(torch.equal(sd[k], live[k]) for k in frozen), "a frozen parameter is its own average"
    return eng


def check_captured_equals_eager(dev, steps=3):
    """The averaged values and ema_state after 3 replays are bitwise those of 3 eager steps (deterministic mode, one pinned tiling): the capture's
    warm-up steps left no trace in the average."""
    prev = ops.is_deterministic()
    ops.force_plan(64, 64, 16, 1)
    try:
        out = []
        for g in (False, True):
            cfg, prod, _, eng = engine(dev, ema_decay=0.9, use_graph=g)
            b = acc.batches(dev, 1)[0]
            for _ in range(steps):
                eng.train_step(b)
            sync(dev)
            out.append((eng, eng.ema.flat.clone(), eng.ema.buf_flat.clone(), eng.ema.state.tolist(), eng.arena.params.detach().clone()))
    finally:
        ops.force_plan(0)
        ops.set_deterministic(prev)
    (ee, fe, be, se, pe), (eg, fg, bg, sg, pg) = out
    assert eg._graphs is not None and ee._graphs is None
    assert se == sg == [f32(0.9), 3.0, 3.0, f32(1.0 - f32(0.9))], (se, sg)
    print("  captured vs eager: live parameters differ in %d elements, averaged ones in %d, averaged buffers in %d"
          % (int((pe != pg).sum()), int((fe != fg).sum()), int((be != bg).sum())))
    assert torch.equal(fe, fg), "averaged parameters, captured vs eager: %d elements differ" % int((fe != fg).sum())
    assert torch.equal(be, bg), "averaged buffers, captured vs eager: %d elements differ" % int((be != bg).sum())


def eval_loss(eng, b):
    """The 11 detailed losses of a fixed batch in eval mode (BatchNorm normalises with its - possibly swapped - running statistics)."""
    eng.model.eval()
    try:
        with torch.no_grad():
            losses = eng.load_data_compute_loss(b)
        return [float(v) for v in losses.values()]
    finally:
        eng.model.train()
        eng.apply_frozen_modes()


def check_ema_weights(dev):
    """Inside ema_weights() the model computes what a second model computes that loaded ema.state_dict()["model"]; after leaving, everything is
    bitwise what a run that never swapped holds, the next train_step included."""
    prev = ops.is_deterministic()
    try:
        runs = []
        for swaps in (True, False):
            cfg, prod, _, eng = engine(dev, ema_decay=0.5, ema_warmup=True)
            bs = acc.batches(dev, 2)
            for i in range(3):
                eng.train_step(bs[i % 2])
            if swaps:
                live_before = eval_loss(eng, bs[0])
                params, bufs = eng.arena.params.detach().clone(), [x.detach().clone() for x in prod.buffers()]
                flat, buf_flat = eng.ema.flat.clone(), eng.ema.buf_flat.clone()
                sd = eng.ema.state_dict()
                assert sd["num_updates"] == 3 and sd["last_opt_step"] == 3 and sd["decay"] == 0.5 and set(sd["model"]) == set(prod.state_dict())
                with eng.ema_weights():
                    inside = eval_loss(eng, bs[0])
                    assert torch.equal(eng.arena.params[:eng.ema.n], flat) and torch.equal(eng.ema.flat, params[:eng.ema.n])
                    with pytest.raises(RuntimeError):
                        with eng.ema_weights():
                            pass
                    with pytest.raises(RuntimeError):
                        eng.train_step(bs[0])
                with pytest.raises(ZeroDivisionError):      # swapped back on an exception as well
                    with eng.ema_weights():
                        1 / 0
                assert not eng.ema.swapped
                assert inside != live_before, "the averaged weights computed the live loss"
                assert eval_loss(eng, bs[0]) == live_before
                assert torch.equal(eng.arena.params, params) and all(torch.equal(x, y) for x, y in zip(prod.buffers(), bufs))
                assert torch.equal(eng.ema.flat, flat) and torch.equal(eng.ema.buf_flat, buf_flat)
                # a second model that loads the averaged state by name
                cfg2, prod2, _, eng2 = engine(dev)
                prod2.load_reference_checkpoint(sd["model"])
                assert eval_loss(eng2, bs[0]) == inside, "ema_weights() differs from a model loaded with ema.state_dict()['model']"
                # state round trip: bitwise
                cfg3, prod3, _, eng3 = engine(dev, ema_decay=0.5, ema_warmup=True)
                eng3.ema.load_state_dict(sd)
                assert torch.equal(eng3.ema.flat, flat) and torch.equal(eng3.ema.buf_flat, buf_flat) and eng3.ema.state.tolist() == [0.5, 3.0, 3.0, 0.0]
            tot, _ = eng.train_step(bs[1])
            sync(dev)
            runs.append((float(tot), eng.arena.params.detach().clone(), eng.ema.flat.clone(), eng.ema.buf_flat.clone(), eng.ema.state.tolist()))
    finally:
        ops.set_deterministic(prev)
    a, b = runs
    assert a[0] == b[0] and a[4] == b[4] and all(torch.equal(x, y) for x, y in zip(a[1:4], b[1:4])), "a swap round trip left a trace in the next step"


def check_bf16_swap_refreshes_copies(dev):
    """bf16 storage mode: the GPT linear layers read cached 16-bit copies of the weights, so a swap has to rewrite them.  A large 1 - decay and
    lr over three steps put the average far from the live weights: the loss inside the context must differ from the live one (it would not, in
    the transformer, with stale copies - asserted on the copies themselves, bitwise), and it returns afterwards (1e-5: the forward's
    default-mode summation-order bound used throughout this suite; the copies return bitwise).  The loss itself cannot be held to equality:
    the deterministic mode is audited for precision "fp32" only and the Engine refuses it in bf16 (NotImplementedError), so the forward keeps
    its default-mode summation orders; the bitwise claim is carried by the copies."""
    try:
        cfg, prod, _, eng = engine(dev, ema_decay=0.5, lr=1e-2, precision="bf16", deterministic=None)
        assert ops.lowp_storage()
        b = acc.batches(dev, 1)[0]
        for _ in range(3):
            eng.train_step(b)
        copies = lambda: [y.clone() for _, y, _ in ops._lowp["w"].values()]
        live, c0 = eval_loss(eng, b), copies()
        assert c0
        with eng.ema_weights():      # the copies are taken BEFORE the loss: outside the Engine's step every use re-makes them anyway
            c1 = copies()
            inside = eval_loss(eng, b)
        c2 = copies()
        after = eval_loss(eng, b)
        sync(dev)
    finally:
        ops.set_precision("fp32")
    assert any(not torch.equal(x, y) for x, y in zip(c0, c1)), "the 16-bit weight copies were not rewritten by the swap"
    assert all(torch.equal(x, y) for x, y in zip(c0, c2)), "the 16-bit weight copies did not return"
    rel = lambda x, y: max(abs(p - q) / max(abs(q), 1e-3) for p, q in zip(x, y))
    print("  bf16: loss inside vs live %.3e relative, after vs live %.3e" % (rel(inside, live), rel(after, live)))
    assert rel(inside, live) > 1e-3 and rel(after, live) <= 1e-5


def check_refusals(dev):
    from transfuser_amd.train import Engine
    cfg = mc.tiny_config(n_layer=1)
    for kw in (dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.5), dict(ema_decay=1.5), dict(ema_decay=0.9, ema_every=0), dict(ema_every=0),
               dict(ema_decay=0.9, ema_every=1.5)):
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        with pytest.raises(ValueError):
            Engine(prod, cfg, autotune=False, **kw)
    prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
    eng = Engine(prod, cfg, autotune=False)
    assert eng.ema is None
    with pytest.raises(RuntimeError):
        eng.ema_weights()


def check_trainer_save_resume(dev, tmp_path):
    """Trainer over a two-batch loader for 2 epochs with an average: model_ema_1.pth exists, loads through load_reference_checkpoint(strict=True)
    and differs from model_1.pth; val_ema_* keys follow ema_validate; a resumed Engine's average after one more step is the uninterrupted run's."""
    from transfuser_amd.train import Trainer
    prev = ops.is_deterministic()
    try:
        cfg, prod, _, eng = engine(dev, ema_decay=0.9)
        loader = [mc.small_batch(2, 32, 64, 64, 40, seed=s) for s in range(2)]
        args = types.SimpleNamespace(logdir=str(tmp_path), ema_validate="both")
        tr = Trainer(eng, loader, loader[:1], args, cfg, torch.device(dev), rank=0, world_size=1, parallel=False)
        rows = lambda: [json.loads(l) for l in open(os.path.join(str(tmp_path), "losses.jsonl"))]
        tr.train()
        tr.validate()
        tr.save()
        r = rows()
        assert len(r) == 3 and "val_loss_total" in r[1] and "val_ema_loss_total" in r[2] and "val_ema_" + cfg.detailed_losses[0] in r[2] and "val_loss_total" not in r[2]
        assert r[1]["val_loss_total"] != r[2]["val_ema_loss_total"] and all(v == v for x in r for v in x.values())
        p = lambda name: os.path.join(str(tmp_path), name)
        assert os.path.exists(p("model_ema_1.pth"))      # the first epoch's files: strict load, and the average is not the live model
        live1, ema1 = torch.load(p("model_1.pth"), map_location="cpu"), torch.load(p("model_ema_1.pth"), map_location="cpu")
        assert list(live1) == list(ema1) and any(not torch.equal(live1[k], ema1[k]) for k in live1 if k.endswith("weight"))
        cfg1, prod1, _, eng1 = engine(dev)
        assert prod1.load_reference_checkpoint(p("model_ema_1.pth"), strict=True) == ([], [])
        assert all(torch.equal(v.cpu(), ema1[k]) for k, v in prod1.state_dict().items())
        args.ema_validate = "live"
        tr.validate()
        assert len(rows()) == 4 and "val_loss_total" in rows()[3]
        args.ema_validate = "ema"
        tr.validate()
        assert len(rows()) == 5 and "val_ema_loss_total" in rows()[4] and "val_loss_total" not in rows()[4]
        assert prod.training and not eng.ema.swapped
        tr.train()
        tr.save()
        assert all(os.path.exists(p(f)) for f in ("model_1.pth", "model_ema_1.pth", "optimizer_1.pth", "model_2.pth", "model_ema_2.pth", "optimizer_2.pth"))
        live_sd, ema_sd, osd = torch.load(p("model_2.pth"), map_location="cpu"), torch.load(p("model_ema_2.pth"), map_location="cpu"), torch.load(p("optimizer_2.pth"), map_location="cpu", weights_only=False)
        assert list(live_sd) == list(ema_sd) and osd["ema"] == dict(num_updates=4, last_opt_step=4, decay=0.9)
        assert any(not torch.equal(live_sd[k], ema_sd[k]) for k in live_sd if "running_mean" in k) and any(not torch.equal(live_sd[k], ema_sd[k]) for k in live_sd if k.endswith("weight"))
        assert all(torch.equal(ema_sd[k], v.cpu()) for k, v in eng.ema.state_dict()["model"].items())
        cfg2, prod2, _, eng2 = engine(dev)
        assert prod2.load_reference_checkpoint(p("model_ema_2.pth"), strict=True) == ([], [])
        # uninterrupted: one more step
        b = {k: v.to(dev) for k, v in loader[0].items()}
        eng.train_step(b)
        sync(dev)
        # resumed: model + optimizer + average from the files
        cfg3, prod3, _, eng3 = engine(dev, ema_decay=0.9)
        prod3.load_reference_checkpoint(p("model_2.pth"))
        eng3.optimizer.load_state_dict(torch.load(p("optimizer_2.pth"), map_location=dev, weights_only=False))
        assert not torch.equal(eng3.ema.flat, eng.ema.flat)
        assert eng3.load_ema(p("model_ema_2.pth"), p("optimizer_2.pth"), map_location=dev) is True
        assert eng3.ema.state.tolist() == [f32(0.9), 4.0, 4.0, 0.0]
        eng3.train_step(b)
        sync(dev)
        assert eng3.ema.state.tolist() == eng.ema.state.tolist() and eng.ema.num_updates == 5
        assert torch.equal(eng3.arena.params, eng.arena.params)
        assert torch.equal(eng3.ema.flat, eng.ema.flat) and torch.equal(eng3.ema.buf_flat, eng.ema.buf_flat), "the resumed average differs from the uninterrupted one"
        assert eng3.load_ema(p("model_ema_7.pth")) is False
        # Engine.save writes the same three files
        os.makedirs(p("eng"))
        eng.save(p("eng"), 9)
        assert os.path.exists(p("eng/model_ema_9.pth")) and torch.load(p("eng/optimizer_9.pth"), map_location="cpu", weights_only=False)["ema"]["num_updates"] == 5
    finally:
        ops.set_deterministic(prev)


def check_cli_flags():
    from transfuser_amd.train import build_parser
    a = build_parser().parse_args([])
    assert (a.ema_decay, a.ema_every, a.ema_warmup, a.ema_validate) == (0.0, 1, 0, "both")
    a = build_parser().parse_args(["--ema_decay", "0.9999", "--ema_every", "4", "--ema_warmup", "1", "--ema_validate", "ema"])
    assert (a.ema_decay, a.ema_every, a.ema_warmup, a.ema_validate) == (0.9999, 4, 1, "ema")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--ema_validate", "neither"])


def check_main_resume(tmp_path):
    """train.main on synthetic data with --ema_decay: the checkpoint trio is written, --load_file restores the average from the sibling file and
    the counters, and a missing sibling starts the average from the loaded weights."""
    from transfuser_amd import train
    argv = ["--id", "t", "--logdir", str(tmp_path), "--root_dir", "synthetic:4", "--batch_size", "2", "--epochs", "1", "--setting", "02_05_withheld", "--val_every", "1",
            "--parallel_training", "0", "--num_workers", "0", "--image_architecture", "regnety_tiny", "--lidar_architecture", "regnety_tiny", "--n_layer", "1",
            "--height", "32", "--width", "64", "--ema_decay", "0.9", "--ema_validate", "ema"]
    tr = train.main(argv)
    d = os.path.join(str(tmp_path), "t")
    n = tr.eng.ema.num_updates
    assert n == float(tr.eng.optimizer.state[0]) > 0
    rows = [json.loads(l) for l in open(os.path.join(d, "losses.jsonl"))]
    assert any("val_ema_loss_total" in r for r in rows) and not any("val_loss_total" in r for r in rows)
    flat = tr.eng.ema.flat.clone()
    tr2 = train.main(argv[:8] + ["--epochs", "1", "--start_epoch", "1"] + argv[10:] + ["--load_file", os.path.join(d, "model_1.pth")])
    assert tr2.eng.ema.num_updates == n and torch.equal(tr2.eng.ema.flat, flat) and not torch.equal(flat, tr2.eng.arena.params[:flat.numel()])
    os.remove(os.path.join(d, "model_ema_1.pth"))
    tr3 = train.main(argv[:8] + ["--epochs", "1", "--start_epoch", "1"] + argv[10:] + ["--load_file", os.path.join(d, "model_1.pth")])
    assert tr3.eng.ema.num_updates == 0 and torch.equal(tr3.eng.ema.flat, tr3.eng.arena.params[:flat.numel()])
