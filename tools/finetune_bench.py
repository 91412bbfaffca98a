"""Fine-tuning (frozen parameters, frozen BatchNorm, AdamW parameter groups), the measurements of its pull request, one visit, same-lease
alternating rounds:
(a) `python bench.py` of a parent checkout (--parent DIR, built) vs this tree with the default arguments, three pairs: the no-regression claim;
(b) per-call cost at the full arena size (168 M floats): tf_adamw_groups_f32 with one default group and with the image encoder's share of the
    tiles frozen, against tf_adamw_f32; tf_grad_sumsq_groups_f32 against tf_grad_sumsq_f32; tf_bn_bwd_frozen_f32 against tf_bn_bwd_f32 at one
    stage-3 shape of the flagship model (B = 10: 10 x 16 x 44 x 576);
(c) B = 10 fp32 graph step with the image encoder frozen vs unfrozen (the weight gradients of frozen parameters still run: report only).
Event / wall-clock timing, warm-up, no profiler.  `python tools/finetune_bench.py [--parent DIR]` on an MI355X."""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; without it part (a) is skipped")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip_step", action="store_true", help="skip part (c)")
    args = ap.parse_args()
    if args.parent:
        from accum_clip_bench import bench_pairs
        bench_pairs(os.path.abspath(args.parent), args.pairs, args.steps, args.warmup)

    import torch
    from transfuser_amd import ops
    from transfuser_amd.train import _ALIGN
    dev = torch.device("cuda", 0)
    ops.L().tf_build_id.restype = __import__("ctypes").c_char_p
    print("build id %s" % ops.L().tf_build_id().decode())

    def event_ms(fn, iters=10, warm=3):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    n = 168 * 1000 * 1000 // _ALIGN * _ALIGN
    frozen_share = 19.4 / 168.0          # regnety_032 image encoder: 19.4 M of the 168 M parameters
    p, g, m, v = (torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 1e-4, 1e-8))
    v.abs_()
    state = torch.tensor([0.0, 1e-4], device=dev)
    one = torch.tensor([[1.0, 0.01, 0.0]], device=dev)
    two = torch.tensor([[1.0, 0.01, 0.0], [1.0, 0.01, 1.0]], device=dev)
    tiles0 = torch.zeros(n // _ALIGN, dtype=torch.uint8, device=dev)
    tiles1 = tiles0.clone()
    tiles1[:int(frozen_share * tiles1.numel())] = 1
    parts = torch.empty(ops.grad_sumsq_parts(n), dtype=torch.float32, device=dev)
    print("(b) per call at %.1f M floats, ms, three alternating rounds" % (n / 1e6))
    rows = {"tf_adamw_f32": lambda: ops.adamw_(p, g, m, v, state),
            "tf_adamw_groups_f32, one default group": lambda: ops.adamw_groups_(p, g, m, v, state, tiles0, one),
            "tf_adamw_groups_f32, %.1f %% of the tiles frozen" % (100 * frozen_share): lambda: ops.adamw_groups_(p, g, m, v, state, tiles1, two),
            "tf_grad_sumsq_f32": lambda: ops.grad_sumsq(g, parts),
            "tf_grad_sumsq_groups_f32, one default group": lambda: ops.grad_sumsq_groups(g, tiles0, one, parts),
            "tf_grad_sumsq_groups_f32, %.1f %% frozen" % (100 * frozen_share): lambda: ops.grad_sumsq_groups(g, tiles1, two, parts)}
    res = {k: [] for k in rows}
    for _ in range(3):
        for k, fn in rows.items():
            res[k].append(event_ms(fn))
    for k, t in res.items():
        print("  %-52s %s  mean %.3f" % (k, "  ".join("%7.3f" % x for x in t), sum(t) / 3))
    del p, g, m, v, tiles0, tiles1
    B, H, W, C = 10, 16, 44, 576
    x, dz = torch.randn(B, H, W, C, device=dev), torch.randn(B, H, W, C, device=dev)
    gamma, mean, invstd = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
    z = torch.relu(x)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    rows = {"tf_bn_bwd_f32": lambda: ops.bn_bwd(dz, z, x, gamma, mean, invstd, dg, db, want_dres=True),
            "tf_bn_bwd_frozen_f32": lambda: ops.bn_bwd(dz, z, x, gamma, mean, invstd, dg, db, want_dres=True, frozen=True),
            "tf_bn_bwd_frozen_f32, frozen affine": lambda: ops.bn_bwd(dz, z, x, gamma, mean, invstd, None, None, want_dres=True, frozen=True)}
    res = {k: [] for k in rows}
    for _ in range(3):
        for k, fn in rows.items():
            res[k].append(event_ms(fn, iters=50, warm=5) * 1e3)
    print("    BatchNorm backward (ReLU mask, dres) at %d x %d x %d x %d, us per call" % (B, H, W, C))
    for k, t in res.items():
        print("  %-52s %s  mean %.1f" % (k, "  ".join("%7.1f" % x for x in t), sum(t) / 3))
    if args.skip_step:
        return

    from transfuser_amd.config import GlobalConfig
    from transfuser_amd.data import synthetic_batch
    from transfuser_amd.model import LidarCenterNet
    from transfuser_amd.train import Engine
    hist_fn = lambda pts: ops.lidar_hist(torch.from_numpy(pts).to(dev)[None])[0].cpu().numpy()
    batch = {k: t.to(dev) for k, t in synthetic_batch(10, 256, 704, seed=0, hist_fn=hist_fn).items()}

    def engine(**kw):      # bench.py's flagship workload: transFuser, regnety_032 trunks, B = 10, 256 x 704, fp32, captured
        cfg = GlobalConfig()
        cfg.n_layer = 4
        cfg.use_target_point_image = True
        cfg.embd_pdrop = cfg.attn_pdrop = cfg.resid_pdrop = 0.1
        torch.manual_seed(0)
        model = LidarCenterNet(cfg, dev, "transFuser", "regnety_032", "regnety_032", use_velocity=False)
        model.train()
        eng = Engine(model, cfg, lr=cfg.lr, use_graph=True, precision="fp32", **kw)
        for _ in range(args.warmup):
            eng.train_step(batch)
        torch.cuda.synchronize()
        return eng

    def step_ms(eng, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            eng.train_step(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    plain, frozen = engine(), engine(freeze=["_model.image_encoder"])
    print("(c) B = 10 fp32 graph step, ms per step, three alternating rounds (active arena %.1f M vs %.1f M floats, %d frozen BatchNorms)"
          % (plain.arena.active_numel / 1e6, frozen.arena.active_numel / 1e6, len(frozen._frozen_bn)))
    res = {"unfrozen": [], "image encoder frozen": []}
    for _ in range(3):
        res["unfrozen"].append(step_ms(plain, args.steps))
        res["image encoder frozen"].append(step_ms(frozen, args.steps))
    for name, t in res.items():
        print("  %-22s %s  mean %.3f" % (name, "  ".join("%8.3f" % x for x in t), sum(t) / len(t)))


if __name__ == "__main__":
    main()
