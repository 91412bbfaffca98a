"""Shared cases of tests/test_accum_clip_emu.py (host emulator) and tests/test_accum_clip_gpu.py (MI355X): micro-batch gradient accumulation
(Engine(accumulate=k)) and global-norm clipping fused into the flat-arena AdamW step (FlatAdamW(max_grad_norm=...), ops.grad_sumsq,
ops.adamw_clip_).

Tolerances, none of them measured on the code under test:
* sum of squares vs float64 of the same fp32 data: every term is non-negative, so the relative error of the sum is at most the number of roundings
  on the longest path times the unit round-off: T = ceil(n / (256 P)) sequential adds per thread, the square, six butterfly steps, four wave
  partials - bounded by (T + 32) * 2^-23 with P = tf_grad_sumsq_parts(n).  The norm (a square root: half the relative error, then one product)
  is held to the same bound;
* adamw_clip_ vs float64 AdamW on float64-clipped gradients: 1e-5 (kernel_cases.close), the bound redzone_cases.check_adamw_dynscale uses for
  the same arithmetic;
* two orders of the same fp32 sums (window vs single runs, graph vs eager, two ranks vs one): 1e-5 of each tensor's max, the bound of
  determinism_cases.check_mode_agreement;
* product vs CPU oracle: model_cases.compare's standing criterion (losses 1e-3, gradients 2e-3 of the tensor's max), the norm at 2e-3."""
import math

import numpy as np
import pytest
import torch

import kernel_cases as kc
import model_cases as mc
from redzone_cases import _adamw64
from transfuser_amd import ops

R = kc.R
BLOCK_SPAN = 1024            # floats one block covers per trip: 256 threads x one float4
GRID_CAP = 1024              # the kernel's own grid cap (tf_grad_sumsq_parts never exceeds it)
# 1, 3: scalar tail only; 4: one float4; 1003: one block, ragged; 4096: four whole blocks; 3 * 1024 + 1: one element more than three blocks' float4
# span; 2 * 1024 * 1024 + 7: the grid cap is reached and every thread of every block makes two grid-stride trips (+ a third for a few, + a tail)
SUMSQ_SIZES = [1, 3, 4, 1003, 4096, 3 * BLOCK_SPAN + 1, 2 * GRID_CAP * BLOCK_SPAN + 7]


def expected_parts(n):
    """tf_grad_sumsq_parts as a pure function of n: one block per 1024 floats up to the cap (asserted against the library on BOTH backends)."""
    return min(GRID_CAP, max(1, -(-n // BLOCK_SPAN)))


def sumsq_bound(n):
    P = ops.grad_sumsq_parts(n)
    return (-(-n // (256 * P)) + 32) * 2.0 ** -23


def plant_positions(n):
    """None (plain data), the LAST element, the first element of the scalar tail, and both sides of a block boundary."""
    pos = [None, n - 1]
    if n % 4 and 4 * (n // 4) != n - 1:
        pos.append(4 * (n // 4))
    if n > BLOCK_SPAN + 1:
        pos += [BLOCK_SPAN - 1, BLOCK_SPAN]
    return pos


def check_sumsq(dev, n):
    P = ops.grad_sumsq_parts(n)
    assert P == expected_parts(n) and 1 <= P <= GRID_CAP, (n, P)
    if n == SUMSQ_SIZES[-1]:
        assert P == GRID_CAP and n // 4 >= 2 * 256 * P      # two trips for every thread at the cap
    base = R(n, seed=n, dev="cpu")
    bound = sumsq_bound(n)
    a0 = ops.float_atomic_launches()
    for pos in plant_positions(n):
        x = base.clone()
        if pos is not None:
            x[pos] = 2.0 * math.sqrt(n) + 1.0            # its square is ~4x the sum of all the others: a dropped element is a gross error
            assert float(x[pos]) ** 2 > 0.5 * float(kc.c64(x).square().sum())
        g = torch.empty(n, dtype=torch.float32, device=dev)
        g.copy_(x)
        want = float(kc.c64(x).square().sum())
        parts = ops.grad_sumsq(g)
        assert parts.shape == (P,) and bool(torch.isfinite(parts).all()), "a block left its partial unwritten"
        got = float(kc.c64(parts).sum())
        print("  sumsq n=%d plant=%s P=%d rel err %.2e (bound %.2e)" % (n, pos, P, abs(got - want) / want, bound))
        assert abs(got - want) <= bound * want, (n, pos, got, want, bound)
        again = ops.grad_sumsq(g, torch.empty(P, dtype=torch.float32, device=dev))
        assert torch.equal(parts, again), "two launches differ"
    assert ops.float_atomic_launches() == a0, "grad_sumsq counted as a float-atomic kernel form"


CLIP_CASES = ["below", "above", "scaled", "shard", "ls_clean", "ls_overflow"]


def check_adamw_clip(dev, case, n_norm=2 * 1003 + 45):
    """Two steps of ops.adamw_clip_ against float64 AdamW on float64-clipped gradients.  The norm range has 2051 elements (three partials, three
    past the last float4); "shard" updates the strict sub-range [64, 64 + 1003) of it, as a ZeRO-1 rank does."""
    lr, lo, hi = 1e-2, 0, n_norm
    if case == "shard":
        lo, hi = 64, 64 + 1003
    gs = {"below": 0.25, "scaled": 1.0 / 3.0}.get(case, 1.0)
    scale = 1024.0 if case.startswith("ls_") else 1.0
    if case.startswith("ls_"):
        gs = 0.5                                               # what is left of the gradient scale under the dynamic loss scale: a window's 1 / k
    n = hi - lo
    own = lambda t: torch.empty(t.shape, dtype=torch.float32, device=dev).copy_(t)
    p, m, v = own(R(n, dev="cpu")), own(R(n, seed=1, dev="cpu") * 0.1), own((R(n, seed=2, dev="cpu") * 0.1).abs())
    arena = own(R(n_norm, seed=3, dev="cpu") * scale)
    state = own(torch.tensor([0.0, lr]))
    ls = own(torch.tensor([scale, 0.0, 0.0, 2.0])) if case.startswith("ls_") else None
    norm_out = own(torch.tensor([-1.0]))
    parts = torch.empty(ops.grad_sumsq_parts(n_norm), dtype=torch.float32, device=dev)
    gs32 = float(np.float32(gs))
    g64 = kc.c64(arena) * gs32 / scale
    norm64 = float(g64.square().sum().sqrt())
    max_norm = (2.0 if case == "below" else 0.3) * norm64
    coef = min(1.0, float(np.float32(max_norm)) / (norm64 + 1e-6))
    assert (coef == 1.0) == (case == "below")
    if case == "ls_overflow":
        before = [t.clone() for t in (p, m, v, state, norm_out)]
        arena[-1] = float("inf")                              # outside the update range's own float4 body: on the norm range's scalar tail
        ops.grad_sumsq(arena, parts)
        ops.adamw_clip_(p, arena[lo:hi], m, v, state, arena, parts, max_norm, norm_out, grad_scale=gs, ls_state=ls)
        for got, old, what in zip((p, m, v, state, norm_out), before, ("p", "m", "v", "state", "norm_out")):
            assert torch.equal(got, old), "adamw_clip_: %s changed in a skipped step" % what
        assert ls.tolist() == [scale / 2, 0.0, 0.0, 2.0], ls.tolist()
        return
    twin = [t.clone() for t in (p, m, v, state)] if case == "below" else None
    for step in (1, 2):
        want = _adamw64(p, g64[lo:hi] * coef, m, v, step, lr)
        ops.grad_sumsq(arena, parts)
        ops.adamw_clip_(p, arena[lo:hi], m, v, state, arena, parts, max_norm, norm_out, grad_scale=gs, ls_state=ls)
        for got, ref, what in zip((p, m, v), want, ("p", "m", "v")):
            kc.close(got, ref, tol=1e-5, what="adamw_clip_ %s step %d %s" % (case, step, what))
        assert state.tolist() == [float(step), float(np.float32(lr))], state.tolist()
        got_norm = float(norm_out[0])
        print("  adamw_clip_ %s step %d: norm %.8g vs %.8g (bound %.2e)" % (case, step, got_norm, norm64, sumsq_bound(n_norm)))
        assert abs(got_norm - norm64) <= sumsq_bound(n_norm) * norm64, (got_norm, norm64)
        if ls is not None:
            assert ls.tolist() == ([scale, 1.0, 0.0, 2.0] if step == 1 else [2 * scale, 0.0, 0.0, 2.0]), ls.tolist()      # doubled at the growth interval of 2
        if twin is not None:                                   # coefficient exactly 1: the same bits as the unclipped kernel with the same scale
            ops.adamw_(twin[0], arena[lo:hi], twin[1], twin[2], twin[3], grad_scale=gs)
            for a, b, what in zip((p, m, v, state), twin, ("p", "m", "v", "state")):
                assert torch.equal(a, b), "adamw_clip_ below max_norm: %s differs from ops.adamw_" % what
    with pytest.raises(RuntimeError, match="partials"):
        ops.adamw_clip_(p, arena[lo:hi], m, v, state, arena[:1000], parts, max_norm, norm_out)
    with pytest.raises(RuntimeError, match="max_norm"):
        ops.adamw_clip_(p, arena[lo:hi], m, v, state, arena, parts, 0.0, norm_out)


# ---------------------------------------------------------------- Engine level
def batches(dev, k):
    return [{n: t.to(dev) for n, t in mc.small_batch(2, 32, 64, 64, 40, seed=s).items()} for s in range(k)]


def make_engine(dev, arch="regnety_tiny", dropout=0.0, lr=1e-4, **kw):
    """Freshly built tiny model (same seed, same dropout site numbering every time) in an Engine."""
    import transfuser_amd.transfuser as ptf
    from transfuser_amd.train import Engine
    cfg = mc.tiny_config(n_layer=1, lidar_res=64, dropout=dropout)
    ptf.GPT._site_base = 0
    prod, ref = mc.build_pair(cfg, arch, dev)
    prod.train()
    return cfg, prod, ref, Engine(prod, cfg, lr=lr, autotune=False, **kw)


def tensors_agree(eng, got, want, what, tol=1e-5):
    """Every parameter's slice of two flat arenas within tol of the tensor's max (determinism_cases.check_mode_agreement)."""
    worst = (0.0, "")
    for name, p, off in eng.arena.layout:
        a, b = got[off:off + p.numel()], want[off:off + p.numel()]
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)
        worst = max(worst, (err, name))
        assert err < tol, "%s: %s differs by %.2e of its max" % (what, name, err)
    print("  %s: worst tensor %.2e (%s)" % (what, worst[0], worst[1]))


def check_window_is_sum(dev, arch):
    """accumulate=2 over (b0, b1) leaves g(b0) + g(b1) in the arena, each g from the same model in its own zeroed arena: catches any
    parameter-gradient path that stores where it must accumulate."""
    cfg, prod, _, eng = make_engine(dev, arch, accumulate=2)
    b0, b1 = batches(dev, 2)
    saved = [b.detach().clone() for b in prod.buffers()]

    def restore():
        with torch.no_grad():
            for b, s in zip(prod.buffers(), saved):
                b.copy_(s)
    singles = []
    for b in (b0, b1):
        eng.arena.zero_grad()
        eng._fwd_bwd(b)
        singles.append(eng.arena.grads.detach().clone())
        restore()
    assert all(float(s.abs().max()) > 0 for s in singles)
    eng.train_step(b0)
    restore()
    assert float(eng.optimizer.state[0]) == 0.0
    eng.train_step(b1)
    assert float(eng.optimizer.state[0]) == 1.0
    tensors_agree(eng, eng.arena.grads, singles[0] + singles[1], "window vs g(b0) + g(b1), %s" % arch)


def _call(model, b):
    return model(b['rgb'], b['lidar'], ego_waypoint=b['ego_waypoint'], target_point=b['target_point'], target_point_image=b['target_point_image'],
                 ego_vel=b['ego_vel'].reshape(-1, 1), bev=b['bev'], label=b['label'], depth=b['depth'], semantic=b['semantic'])


def check_ddp_equivalence_vs_oracle(dev):
    """The oracle on b0, then on b1 without zeroing, divided by 2 = what two data-parallel ranks reduce to; the Engine's arena after the
    window, times its grad_scale, and its grad_norm against that and torch.nn.utils.clip_grad_norm_."""
    import transfuser_amd.transfuser as ptf
    from transfuser_amd.train import Engine
    cfg = mc.tiny_config(n_layer=1)
    ptf.GPT._site_base = 0
    prod, ref = mc.build_pair(cfg, "regnety_tiny", dev)
    prod.train(); ref.train()
    bs = batches("cpu", 2)
    w = dict(zip(cfg.detailed_losses, cfg.detailed_losses_weights))
    ref_losses = []
    for b in bs:
        lr_ = _call(ref, b)
        sum(w[k] * v for k, v in lr_.items()).backward()
        ref_losses.append({k: v.detach() for k, v in lr_.items()})
    live = [p for p in ref.parameters() if p.grad is not None]
    for p in live:
        p.grad.div_(2)
    ref_norm = float(torch.sqrt(sum(kc.c64(p.grad).square().sum() for p in live)))
    m = 0.5 * ref_norm                                          # the clip is active
    eng = Engine(prod, cfg, lr=1e-4, autotune=False, accumulate=2, max_grad_norm=m)
    got_losses = [eng.train_step({n: t.to(dev) for n, t in b.items()})[1] for b in bs]
    assert float(eng.optimizer.state[0]) == 1.0
    assert eng.grad_scale() == 0.5
    eng.arena.grads.mul_(eng.grad_scale())                      # the gradients stay readable after the update; p.grad are views of the arena
    for lp, lr_ in zip(got_losses, ref_losses):
        for k in lr_:
            assert abs(float(lp[k]) - float(lr_[k])) <= 1e-3 * max(1.0, abs(float(lr_[k]))), (k, float(lp[k]), float(lr_[k]))
    mc.compare(prod, ref, got_losses[1], ref_losses[1])
    torch_norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), m))
    got = float(eng.optimizer.grad_norm)
    print("  grad_norm %.6g, clip_grad_norm_ %.6g, fp64 %.6g" % (got, torch_norm, ref_norm))
    assert abs(got - torch_norm) <= 2e-3 * torch_norm, (got, torch_norm)


def window_run(dev, use_graph, max_grad_norm, windows=3, deterministic=None, accumulate=2, **kw):
    """`windows` windows of `accumulate` micro-batches -> per call losses, per window (gradient arena, grad_norm), final parameters, step counter."""
    cfg, prod, _, eng = make_engine(dev, accumulate=accumulate, max_grad_norm=max_grad_norm, use_graph=use_graph, deterministic=deterministic, **kw)
    bs = batches(dev, accumulate)
    losses, per_window = [], []
    for _ in range(windows):
        for b in bs:
            tot, det = eng.train_step(b)
            losses.append([float(tot)] + [float(det[k]) for k in cfg.detailed_losses])
        gn = eng.optimizer.grad_norm
        per_window.append((eng.arena.grads.detach().clone(), None if gn is None else float(gn)))
    if dev != "cpu":
        torch.cuda.synchronize()
    return eng, torch.tensor(losses, dtype=torch.float64), per_window, eng.arena.params.detach().clone(), float(eng.optimizer.state[0])


def check_graph_matches_eager(dev):
    """accumulate=2 with an active clip, captured vs eager over three windows.  One tiling without split-K is pinned, as in
    test_model_gpu.py::test_engine_graph_replay_matches_eager, whose loss criterion is applied.  Both runs are made under the deterministic
    mode: the 1e-5 rule bounds two summation orders of the SAME parameters, and in the default mode that only describes the first window -
    the atomics' last-bit noise in a round-off-level gradient entry becomes +-lr on that weight in the first AdamW update, and the later
    windows then differentiate slightly different models (measured on the MI355X in the default mode at lr 1e-4: 5.0e-6 in window 0, 1.4e-5
    in window 1).  With fixed-order sums what is compared is the orchestration: zeroing, seed bump, the optimizer graph's place."""
    prev = ops.is_deterministic()
    ops.force_plan(64, 64, 16, 1)
    try:
        _, _, first, _, _ = window_run(dev, False, 1e30, windows=1, deterministic=True)
        m = 0.5 * first[0][1]
        assert m > 0
        runs = [window_run(dev, g, m, deterministic=True) for g in (False, True)]
    finally:
        ops.force_plan(0)
        ops.set_deterministic(prev)
    (ee, le, we, pe, se), (eg, lg, wg, pg, sg) = runs
    assert se == 3.0 and sg == 3.0, (se, sg)                    # one AdamW update per window of two calls, graph or not
    assert we[0][1] > m, "the clip must be active"
    for i, ((ga, na), (gb, nb)) in enumerate(zip(we, wg)):
        tensors_agree(ee, gb, ga, "window %d gradients, graph vs eager" % i)
        print("  window %d grad_norm eager %.8g graph %.8g" % (i, na, nb))
        assert abs(na - nb) <= 1e-5 * na, (i, na, nb)
    rel = ((le - lg).abs() / le.abs().clamp_min(1e-3)).max(dim=1).values
    print("  graph vs eager: max relative loss difference per call %s" % ["%.1e" % v for v in rel.tolist()])
    assert rel[0].item() <= 1e-5 and rel[1].item() <= 2e-4 and rel.max().item() <= 2e-4, rel


def check_bitwise_runs(dev, use_graph):
    """Under ops.deterministic(): two runs of three clipped windows end in the same parameter bits (and the same losses and norms)."""
    prev = ops.is_deterministic()
    try:
        a = window_run(dev, use_graph, 0.05, deterministic=True)
        b = window_run(dev, use_graph, 0.05, deterministic=True)
    finally:
        ops.set_deterministic(prev)
    assert a[4] == 3.0 and b[4] == 3.0
    assert torch.equal(a[1], b[1]), "losses differ"
    assert [w[1] for w in a[2]] == [w[1] for w in b[2]], "grad_norm differs"
    assert a[2][0][1] > 0.05, "the clip must be active"
    assert torch.equal(a[3], b[3]), "parameters differ after 3 deterministic windows: %d of %d elements" % (int((a[3] != b[3]).sum()), a[3].numel())


def check_defaults_unchanged(dev):
    """Engine(accumulate=1, max_grad_norm=None) is the constructor without the arguments: same parameter bits after two deterministic steps."""
    prev = ops.is_deterministic()
    try:
        finals = []
        for kw in ({}, dict(accumulate=1, max_grad_norm=None)):
            cfg, prod, _, eng = make_engine(dev, dropout=0.1, lr=1e-3, deterministic=True, **kw)
            b = batches(dev, 1)[0]
            for _ in range(2):
                eng.train_step(b)
            assert eng.optimizer.grad_norm is None and float(eng.optimizer.state[0]) == 2.0
            finals.append(eng.arena.params.detach().clone())
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(finals[0], finals[1])


def check_fp16_dynamic_window(dev):
    """fp16 mode under the dynamic loss scale with accumulate=2: the scale is constant inside a window and is updated with AdamW only; a clean
    window == the static-scale window bit for bit (1 / 1024 and 1 / 2 are exact in either order); an overflowed window is skipped as a whole."""
    from transfuser_amd.train import Engine
    cfg = mc.tiny_config(n_layer=1)
    cfg.loss_scale_growth_interval = 2
    bs = batches(dev, 2)
    try:
        engines = []
        for kw in ({}, dict(loss_scale=1024.0)):
            prod, _ = mc.build_pair(cfg, "regnety_tiny", dev, seed=5)
            prod.train()
            engines.append(Engine(prod, cfg, lr=1e-3, precision="fp16", accumulate=2, autotune=False, **kw))
        eng, ref = engines
        assert eng.ls_state is not None and eng.optimizer.max_grad_norm == float("inf") and ref.ls_state is None
        eng.ls_state[0] = 1024.0
        p0 = eng.arena.params.clone()
        eng.train_step(bs[0])
        assert float(eng.optimizer.state[0]) == 0.0 and eng.ls_state.tolist()[:3] == [1024.0, 0.0, 0.0] and torch.equal(eng.arena.params, p0)
        eng.train_step(bs[1])
        assert float(eng.optimizer.state[0]) == 1.0 and eng.ls_state.tolist()[:3] == [1024.0, 1.0, 0.0]
        for b in bs:
            ref.train_step(b)
        assert torch.equal(ref.arena.params, eng.arena.params), (ref.arena.params - eng.arena.params).abs().max()
        p1, m1 = eng.arena.params.clone(), eng.optimizer.exp_avg.clone()
        eng.ls_state[0] = 2.0 ** 120                             # every half-precision dy overflows
        for b in bs:
            eng.train_step(b)
        assert torch.equal(eng.arena.params, p1) and torch.equal(eng.optimizer.exp_avg, m1)
        assert float(eng.optimizer.state[0]) == 1.0 and eng.ls_state.tolist()[:3] == [2.0 ** 119, 0.0, 0.0]
    finally:
        ops.set_precision("fp32")


def check_refusals(dev):
    from transfuser_amd.train import Engine, FlatAdamW
    cfg = mc.tiny_config(n_layer=1)
    prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
    for kw in (dict(accumulate=0), dict(accumulate=-2), dict(accumulate=1.5), dict(max_grad_norm=0), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            Engine(prod, cfg, autotune=False, **kw)
    eng = Engine(prod, cfg, autotune=False)
    with pytest.raises(ValueError):
        FlatAdamW(eng.arena, max_grad_norm=0.0)
